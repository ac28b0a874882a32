"""The weight cache policy changes how weight bytes travel, never what a kernel computes: every launch that has a streaming variant
(lean 196-row GEMMs, small-map and wide 3x3 convolutions, the q-projection attention; csrc/weight_stream.cpp) gives the same bits
with every load on the default policy (mode 0) as with every variant streaming (mode 2) -- torch.equal on every output buffer,
whole buffers (slack and guard bands included), and on every prediction of a 224 x 224 forward replayed from hipGraphs."""
import ctypes as C
import json
import os

import pytest
import torch

import gemm_desc_ref as R
import test_gemm_lean_gpu as TL
import test_head_levels_gpu as TH

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")
ROWS = [(i + 1, json.loads(line)) for i, line in enumerate(open(TABLE))]
# every lean row of the bf16 224 x 224 step with at most two 196-row sides: the ragged 7th M-tile, the paired q/k/v + cross-k/v launch,
# the split-A key MLP, the dyn_n rows of the memory read
LEAN_ROWS = [(ln, r) for ln, r in ROWS if r["lean"] == 1 and "bf16_224" in r["from"] and all(d["M"] <= 392 for d in r["descs"])]


@pytest.fixture(autouse=True)
def _mode_restored():
    from spann3r_amd import lib as L
    before = L.load().sp3_weight_stream_get()
    yield
    assert L.load().sp3_weight_stream_set(before) == 0


def _both_modes(run):
    """run() under mode 0 and mode 2 -> the two lists of output tensors"""
    from spann3r_amd import lib as L
    res = []
    for mode in (0, 2):
        L.check(L.load().sp3_weight_stream_set(mode), "sp3_weight_stream_set")
        outs = run()
        torch.cuda.synchronize()
        res.append(outs)
    return res


def _assert_same(a, b, what=""):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: output %d differs between the cache policies" % (what, i)


def test_rows_cover_the_lean_instances():
    tiles = {t for _, r in LEAN_ROWS for t in r["tiles"]}
    assert {30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 42, 43, 44} <= tiles, sorted(tiles)
    assert any(len(r["descs"]) == 2 for _, r in LEAN_ROWS) and any(r["descs"][0].get("dyn_n") for _, r in LEAN_ROWS)
    assert any(d.get("A2") for _, r in LEAN_ROWS for d in r["descs"])


@pytest.mark.parametrize("line,row", LEAN_ROWS, ids=["L%d-t%s" % (ln, "+".join(str(t) for t in r["tiles"])) for ln, r in LEAN_ROWS])
def test_lean_row(line, row):
    from spann3r_amd import lib as L
    l = L.load()
    for dyn in R.dyn_extents(row):
        def run():
            cases = [c.materialize("cuda") for c in R.row_cases(row, line, dyn)]
            ds = [c.desc(L) for c in cases]
            if len(ds) == 1:
                assert int(l.sp3_gemm_plan(C.byref(ds[0]))) == row["tiles"][0]
                L.check(l.sp3_gemm(C.byref(ds[0]), L.stream_ptr()), "sp3_gemm")
            else:
                arr = (C.POINTER(L.GemmDesc) * len(ds))(*[C.pointer(d) for d in ds])
                t = (C.c_int * len(ds))()
                assert l.sp3_gemm_plan_n(arr, len(ds), t) == 0 and list(t) == row["tiles"]
                L.check(l.sp3_gemm_n(arr, len(ds), L.stream_ptr()), "sp3_gemm_n")
            torch.cuda.synchronize()
            # every output buffer of every descriptor, whole (C, c2, stats_out, vt, the softmax statistics; guard bands included)
            return [s.t.clone() for c in cases for _, s in sorted(c.bufs.items()) if s.out]
        a, b = _both_modes(run)
        _assert_same(a, b, "row %d (extent %r)" % (line, dyn))
        assert any(bool((x[R.GUARD:-R.GUARD] != R.SENT).any()) for x in a)       # (the launch wrote something)


SMALL_MAPS = {"7x7": (1, 7, 7, 256, 256, 1, "rcu2"), "14x14": (1, 14, 14, 256, 256, 1, "rcu2")}


@pytest.mark.parametrize("maps", ["bf16", "fp32"])
@pytest.mark.parametrize("members", [("7x7",), ("14x14",), ("7x7", "14x14")], ids=["7x7", "14x14", "level"])
def test_small_map_convolutions(members, maps):
    """tiles 40 (7 x 7) and 41 (14 x 14), each alone and both as one level launch"""
    ops = TH._ops()
    mdt = BF if maps == "bf16" else torch.float32
    probs = [TH._conv_problem(ops, *SMALL_MAPS[m], mdt, seed=10 * i) for i, m in enumerate(members)]
    a, b = _both_modes(lambda: TH._run_convs(ops, probs, mdt, merged=len(probs) > 1))
    _assert_same(a, b, "+".join(members))
    assert all(bool(torch.isfinite(x.float()).all()) and float(x.float().abs().max()) > 0 for x in a)


@pytest.mark.parametrize("maps", ["bf16", "fp32"])
def test_wide_convolution_smallest_routed_map(maps):
    """56 x 56, B = 1, 256 -> 256: the smallest map the wide tile takes (its 32-channel instance)"""
    ops = TH._ops()
    mdt = BF if maps == "bf16" else torch.float32
    probs = [TH._conv_problem(ops, 1, 56, 56, 256, 256, 1, "rcu2", mdt, seed=5)]
    a, b = _both_modes(lambda: TH._run_convs(ops, probs, mdt, merged=False))
    _assert_same(a, b, "wide conv")
    assert bool(torch.isfinite(a[0].float()).all()) and float(a[0].float().abs().max()) > 0


def test_attention_with_the_q_projection_inside():
    """B = 2 images per side, 12 heads, Nq = Nk = 196: 13 query blocks per head (the last one ragged), 4 key tiles (the last one ragged)"""
    from spann3r_amd.engine import _rope_tables
    ops = TL._ops()
    rnd = TL.rnd
    B, nh, nw, D, heads = 2, 14, 14, 768, 12
    P = nh * nw
    Rr, npad = B * P, (P + 63) // 64 * 64
    xg = ops.PackedAct.group(2, Rr, D, BF, DEV)
    stg = torch.zeros(2, Rr, D // 32, 2, device=DEV)
    Ws, ss, bs = [], [], []
    for s_ in (0, 1):
        ops.pack_stats((rnd(Rr, D, seed=1 + s_) * 2 + 0.2).to(DEV), xg.at(s_), stg[s_], rows=Rr, C_=D)
        W = rnd(D, D, seed=2 + s_) * 0.05
        Ws.append(ops.PackedWeight(W.to(DEV).to(BF)))
        ss.append(TL.bf(W).sum(1))
        bs.append(rnd(D, seed=3 + s_))
    Wg = ops.PackedWeightGroup(Ws)
    sg, bg = torch.stack(ss).to(DEV).contiguous(), torch.stack(bs).to(DEV).contiguous()
    pos = TL._pos(B, nh, nw).reshape(-1, 2).to(torch.int32).to(DEV)
    cos, sin = _rope_tables(64, 100.0, DEV)
    kp = ops.PackedAct.from_dense((rnd(2 * B * npad, D, seed=9) * 1.5).to(DEV).to(BF))
    vtp = rnd(2 * B * heads * npad * 64, seed=10).to(DEV).to(BF)

    def run():
        got = ops.PackedAct.group(2, Rr, D, BF, DEV)
        ops.attention_packed_qproj(xg, stg, Wg, sg, bg, pos, cos, sin, kp, D, 0, npad, vtp, got, D, B=2 * B, heads=heads, Nq=P, Nk=P, scale=0.125,
                                   o_group=B, o_group_rows=xg.rows_pad, eps=1e-6, stats_group_stride=Rr * (D // 32) * 2, vec_group_stride=D)
        return [got.data]
    a, b = _both_modes(run)
    _assert_same(a, b, "attention_packed_qproj")
    assert bool(torch.isfinite(a[0].float()).all()) and float(a[0].float().abs().max()) > 0.05


def test_forward_224(full_sd):
    """three 224 x 224 frames in bf16, hipGraphs on, a fresh model per mode (a captured graph keeps the policy it was captured with)"""
    from spann3r_amd import Spann3R, FULL
    from spann3r_amd.weights import synth_frames
    frames = [{"img": f["img"].to(DEV)} for f in synth_frames(3, 224, 224)]

    def run():
        m = Spann3R(dus3r_name=None, cfg=FULL, init_weights=False)
        m.load_state_dict(full_sd, strict=True)
        m = m.to(DEV).eval().set_precision("bf16")
        m.use_graphs = True
        with torch.no_grad():
            preds, _ = m(frames)
        torch.cuda.synchronize()
        outs = [p[k].clone() for p in preds for k in sorted(p) if torch.is_tensor(p[k])]
        del m
        return outs
    a, b = _both_modes(run)
    assert len(a) >= 6
    _assert_same(a, b, "forward")
    assert all(bool(torch.isfinite(x.float()).all()) for x in a)
