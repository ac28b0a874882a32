"""tools/issue_order.py: its parser on a committed disassembly excerpt (tests/golden/issue_order_excerpt.txt: one kernel of
csrc/gemm_sm.hip as llvm-objdump prints it, thinned) and on a few hand-written lines.  Nothing is compiled here."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import issue_order as T  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
KERNEL = "_ZN12_GLOBAL__N_19sm_kernelILi3ELi2ELi8ELi48ELi3ELi1ELb0ELb1ELi6ELi3EEEvNS_6SmArgsE"


def test_excerpt_of_the_decoder_fc2_instance():
    """tile 37 <MF 3, NF 2, 8 waves, 48 k-blocks>: a wave walks 6 k-blocks -- 36 A loads and 24 W loads of 16 bytes + bias + residual;
    the whole W walk and an A ring of 3 (18 + 24 = 42 loads) are queued behind the two epilogue loads, before the first of 72 MFMAs"""
    kernels = T.parse_disassembly(open(os.path.join(GOLDEN, "issue_order_excerpt.txt")).read())
    assert list(kernels) == [KERNEL]
    s = T.summarize(kernels[KERNEL])
    assert (s["loads16"], s["loads"], s["mfmas"]) == (62, 62, 72)
    assert s["before_mfma"] == 44 and s["max_in_flight"] == 42
    words = s["seq"].split()
    assert words[:5] == ["L2", "W0", "L42", "W23", "M1"] and words[-2:] == ["W0", "M2"]
    assert sum(int(w[1:]) for w in words if w[0] == "L") == 62 and sum(int(w[1:]) for w in words if w[0] == "M") == 72
    # the three A refills of 6 loads each follow a k-block's 12 MFMAs
    assert [w for w in words if w[0] == "L"] == ["L2", "L42", "L6", "L6", "L6"]
    r = T.parse_remarks(open(os.path.join(GOLDEN, "issue_order_excerpt_remarks.txt")).read())
    assert r == {KERNEL: {"vgprs": 198, "agprs": 0, "scratch": 0, "occupancy": 2, "lds": 0}}


TEXT = """
Disassembly of section .text:

0000000000001000 <k1>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001000: C0060002 00000000
	s_waitcnt lgkmcnt(0)                                       // 000000001008: BF8CC07F
	global_load_dword v1, v0, s[0:1]                           // 00000000100C: DC508000 01000000
	global_load_dwordx4 v[2:5], v0, s[0:1] offset:16 nt        // 000000001014: DC5E8010 02000000
	buffer_load_dwordx4 v[6:9], v0, s[8:11], 0 offen           // 00000000101C: E05C1000 80020600
	s_waitcnt vmcnt(1) lgkmcnt(0)                              // 000000001024: BF8C0071
	v_mfma_f32_16x16x32_bf16 v[10:13], v[2:5], v[6:9], v[10:13]     // 000000001028: D3B5000A 042A0D02
	v_mfma_f32_16x16x32_bf16 v[10:13], v[2:5], v[6:9], v[10:13]     // 000000001030: D3B5000A 042A0D02
	global_load_dwordx4 v[2:5], v0, s[0:1] offset:32           // 000000001038: DC5C8020 02000000
	s_waitcnt vmcnt(0)                                         // 000000001040: BF8C0F70
	v_mfma_f32_32x32x16_bf16 v[14:29], v[2:5], v[6:9], v[14:29]     // 000000001044: D3B7000E 043A0D02
	global_store_dwordx4 v0, v[10:13], s[2:3]                  // 00000000104C: DC7C8000 00020A00
	s_endpgm                                                   // 000000001054: BF810000

0000000000001100 <k2>:
	s_endpgm                                                   // 000000001100: BF810000
"""


def test_hand_written_lines():
    """a narrow load counts towards vmcnt but not towards the 16-byte loads; a wait without vmcnt is no event; stores are not looked at"""
    kernels = T.parse_disassembly(TEXT)
    assert kernels["k2"] == []
    assert kernels["k1"] == [("L", 4), ("L", 16), ("L", 16), ("W", 1), ("M", 1), ("M", 1), ("L", 16), ("W", 0), ("M", 1)]
    s = T.summarize(kernels["k1"])
    assert s["seq"] == "l1 L2 W1 M2 L1 W0 M1"
    assert (s["loads16"], s["loads"], s["before_mfma"], s["before_mfma_all"], s["mfmas"], s["max_in_flight"]) == (3, 4, 2, 3, 3, 3)
    assert T.summarize(kernels["k2"])["max_in_flight"] == 0
    assert s["hash"] == T.summarize(list(kernels["k1"]))["hash"] != T.summarize(kernels["k1"][:-1])["hash"]


def test_report_prints_one_block_per_kernel():
    import io
    out = io.StringIO()
    T.report(open(os.path.join(GOLDEN, "issue_order_excerpt.txt")).read(), open(os.path.join(GOLDEN, "issue_order_excerpt_remarks.txt")).read(),
             pattern="sm_kernel", wide=100, out=out)
    text = out.getvalue().splitlines()
    assert "sm_kernel" in text[0] and "before_mfma 44" in text[1] and "vgprs 198" in text[1] and "scratch 0" in text[1]
    assert text[2].startswith("  seq L2 W0 L42") and all(len(l) <= 100 for l in text[2:])
