"""tests/gemm_desc_ref.py -- the float64 reference and builder behind the census replay (test_gemm_census_gpu.py) -- checked without a
GPU: each piece of the reference against an independent torch formulation, every fragment layout it writes or reads as a round trip
against the project's own packers, and every row of tests/golden/gemm_plan_table.jsonl constructible with all indices inside the
extents the header's layout rules give."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_desc_ref as R
from conftest import GOLDEN, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(i + 1, json.loads(line)) for i, line in enumerate(open(os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")))]
BF = torch.bfloat16


def rnd(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=torch.float64) * 2 - 1


# ----------------------------------------------------------------------------- pieces of the reference
@pytest.mark.parametrize("stride,H,W", [(1, 7, 9), (2, 7, 9), (2, 8, 6), (1, 1, 5)])
def test_conv_rows_is_conv2d(stride, H, W):
    B, Cin, Cout = 2, 16, 24
    x, w, b = rnd(B, H, W, Cin, seed=1), rnd(Cout, 3, 3, Cin, seed=2), rnd(Cout, seed=3)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    got = (R.conv_rows(x, OH, OW, stride) @ w.reshape(Cout, -1).T + b).reshape(B, OH, OW, Cout)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=1).permute(0, 2, 3, 1)
    assert rel_err(got, ref) < 1e-13


@pytest.mark.parametrize("ks", [2, 4])
def test_pixshuf_is_conv_transpose(ks):
    B, H, W, Cin, Cout = 2, 3, 5, 16, 8
    x, w, b = rnd(B, Cin, H, W, seed=1), rnd(Cin, Cout, ks, ks, seed=2), rnd(Cout, seed=3)
    wp = w.permute(2, 3, 1, 0).reshape(-1, Cin)                                      # [(ky*ks+kx)*Cout + co, ci]
    y = x.permute(0, 2, 3, 1).reshape(-1, Cin) @ wp.T + b.repeat(ks * ks)[None]
    got = R.pixshuf_scatter(y, B, H, W, ks, Cout)
    assert rel_err(got, F.conv_transpose2d(x, w, b, stride=ks).permute(0, 2, 3, 1)) < 1e-13


def test_ln_fold_is_layernorm_then_linear():
    M, Cx, N = 37, 96, 40
    x, gam, beta, W, b = rnd(M, Cx, seed=1) * 2 + 0.3, rnd(Cx, seed=2) * 0.3 + 1, rnd(Cx, seed=3) * 0.2, rnd(N, Cx, seed=4), rnd(N, seed=5)
    stats = torch.stack((x.view(M, Cx // 32, 32).sum(-1), (x * x).view(M, Cx // 32, 32).sum(-1)), -1)
    Wf = W * gam[None]
    got = R.ln_fold_apply(x @ Wf.T, stats, Cx, 1e-6, Wf.sum(1)) + (b + W @ beta)
    assert rel_err(got, F.layer_norm(x, (Cx,), gam, beta, 1e-6) @ W.T + b) < 1e-12


def test_softmax_keep_is_threshold_then_renormalise():
    S = rnd(20, 300, seed=1) * 3
    V = rnd(64, 300, seed=2)
    p, mass, mx, Z = R.softmax_keep(S, 2e-3)
    a = torch.softmax(S, -1)
    a = torch.where(a >= 2e-3, a, torch.zeros_like(a))
    assert 0.05 < float((a == 0).double().mean()) < 0.95
    assert rel_err((p @ V.T) / mass[:, None], (a / a.sum(-1, keepdim=True)) @ V.T) < 1e-13
    assert rel_err(mx, S.max(1).values) == 0 and rel_err(Z, torch.exp(S - S.max(1, keepdim=True).values).sum(1)) < 1e-14
    # the per-32-key partials merge back to the row's (max, Z)
    st = R.group_softmax_stats(S)
    m = st[..., 0].max(1).values
    assert rel_err(m, mx) == 0 and rel_err((st[..., 1] * torch.exp(st[..., 0] - m[:, None])).sum(1), Z) < 1e-13
    assert st.shape == (20, 10, 2)                                                    # ragged last group


@pytest.mark.parametrize("h,w,OH,OW", [(7, 7, 14, 14), (5, 8, 9, 16), (1, 4, 2, 7)])
def test_upsample2x_is_interpolate_align_corners(h, w, OH, OW):
    r = rnd(2, h, w, 12, seed=1)
    ref = F.interpolate(r.permute(0, 3, 1, 2), size=(2 * h, 2 * w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)[:, :OH, :OW]
    assert rel_err(R.upsample2x(r, OH, OW), ref) < 1e-13


def test_rope_columns_against_stored_vectors():
    """ROPE_VT's column formula on the stored reference vectors (tests/golden/rope2d_reference.npz: tok [B,H,N,64], fwd [B,N,H,64])"""
    from oracle import spann3r_oracle as O
    z = np.load(os.path.join(GOLDEN, "rope2d_reference.npz"))
    tok, fwd = torch.from_numpy(z["tok"]).double(), torch.from_numpy(z["fwd"]).double()
    B, H, N, D = tok.shape
    pos = O.positions(B, 5, 7).reshape(-1, 2)
    y = tok.permute(0, 2, 1, 3).reshape(B * N, H * D)
    cos, sin = R.rope_tables("cpu")
    got = R.rope_cols_apply(y, pos, cos, sin).reshape(B, N, H, D)
    assert rel_err(got, fwd) < 2e-6
    assert rel_err(y.reshape(B, N, H, D), fwd) > 1e-2


def test_gelu_is_erf_gelu():
    x = rnd(1000, seed=1) * 4
    assert rel_err(R.gelu(x), F.gelu(x)) < 1e-14


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("rows,K", [(16, 64), (37, 200), (196, 768), (5, 8)])
def test_fragment_order_round_trip(dtype, rows, K):
    from spann3r_amd import ops
    x = rnd(rows, K, seed=1).to(dtype)
    flat = R.frag_pack(x, dtype)
    assert flat.numel() == R.frag_numel(rows, K, dtype)
    assert torch.equal(R.frag_unpack(flat, rows, K, dtype), x)
    # the header's index formula against the packers the model uses, both ways
    pa = ops.PackedAct.from_dense(x)
    assert torch.equal(pa.data.reshape(-1), flat) and torch.equal(pa.to_dense(), R.frag_unpack(flat, rows, K, dtype))
    assert torch.equal(ops.PackedWeight(x).data.reshape(-1), flat)
    off = R.frag_offsets(rows, K, dtype).reshape(-1)
    assert off.unique().numel() == off.numel() and int(off.max()) < flat.numel()
    # allocated wider than used (a bank that grows along K): slack lands only past K
    wide = R.frag_pack(x, dtype, K + 100, 7.0)
    assert torch.equal(R.frag_unpack(wide, rows, K + 100, dtype)[:, :K], x) and bool((R.frag_unpack(wide, rows, K + 100, dtype)[:, K:] == 7.0).all())


@pytest.mark.parametrize("N,K", [(32, 64), (50, 168), (768, 96)])
def test_fp16_plane_weights_round_trip(N, K):
    from spann3r_amd import ops
    w = (rnd(N, K, seed=1) * 0.05).float()
    w[0, :4] = torch.tensor([0.0, 1e-9, -1000.0, 6.1e-5])
    flat = R.planes_pack(w)
    assert torch.equal(ops.PackedWeight(w, halves=True).data.reshape(-1).view(torch.int32), flat.view(torch.int32))
    back = R.planes_unpack(flat, N, K)
    assert rel_err(back, w.double()) < 2e-6                                          # 22 mantissa bits of the (h, l) split
    h = w.to(torch.float16)
    assert torch.equal(back, h.double() + ((w - h.float()) * 2048.0).to(torch.float16).double() / 2048.0)


def test_pv_order_round_trip():
    """PV-operand order [(b,h)][npad/32][4][64][8], restated token by token as the qkv_packed epilogue documents it"""
    B, heads, tok, npad = 2, 3, 50, 64
    v = rnd(B, tok, heads, 64, seed=1).float()
    packed = torch.zeros(B, heads, npad // 32, 4, 64, 8)
    for n in range(tok):
        u, kk = n // 32, n % 32
        w16 = kk % 16
        e, g = (w16 % 4) + 4 * (kk // 16), w16 // 4
        for db in range(4):
            packed[:, :, u, db, g * 16:(g + 1) * 16, e] = v[:, n, :, db * 16:(db + 1) * 16]
    packed = packed.reshape(-1)
    off = R.pv_offsets(B, heads, tok, npad)
    assert torch.equal(packed[off], v) and off.unique().numel() == off.numel() and int(off.max()) < packed.numel()


# ----------------------------------------------------------------------------- the census rows
def _covered():
    from test_gemm_census_gpu import NOT_COVERED
    return NOT_COVERED


def test_not_covered_list_is_pinned():
    nc = _covered()
    print("census rows the replay does not cover: %d" % len(nc))
    for line, why in sorted(nc.items()):
        print("  line %d (tiles %r): %s" % (line, ROWS[line - 1][1]["tiles"], why))
    assert len(nc) == 2 and all(len(w) > 20 for w in nc.values())
    # a row is on the list only because its layout is not restated: the builder itself says so
    for line, row in ROWS:
        try:
            R.row_cases(row, line)
            assert line not in nc, line
        except NotImplementedError:
            assert line in nc, line


def _pointers_stay_inside(c, d):
    """the descriptor desc() returns, problem by problem: base + z * stride (elements, or the sb_* byte offsets) + the extent one problem
    touches lies inside the body of its buffer -- also where the strides are negative (the crossed k/v group starts at the last slot)"""
    f = c.f
    es = lambda n: c.bufs[n].t.element_size()

    def inside(name, base, step_bytes, extent_elems):
        lo = c.bufs[name].ptr()
        hi = lo + c.bufs[name].numel * es(name)
        for z in range(c.batch):
            p = base + z * step_bytes
            assert lo <= p and p + extent_elems * es(name) <= hi, (name, z, p - lo, extent_elems, hi - lo)
    if f.get("a_packed"):
        a_ext = R.frag_numel(c.M, c.K1, c.adt)
    elif c.loader == R.LOAD_CONV3X3:
        a_ext = c.strideA
    else:
        a_ext = (c.M - 1) * c.lda + (c.K1 if c.loader == R.LOAD_PLAIN else c.K)
    inside("A", d.A, d.strideA * es("A"), a_ext)
    inside("W", d.W, d.strideW * es("W"), R.frag_numel(c.N, c.ldw, c.wdt) if f.get("w_packed") else (c.N - 1) * c.ldw + c.K)
    if f.get("A2"):
        inside("A2", d.A2, d.sb_A2, R.frag_numel(c.M, c.K - c.K1, c.adt) if f.get("a_packed") else (c.M - 1) * c.lda2 + c.K - c.K1)
    if c.epi == R.EPI_ROPE_VT:
        c_ext = R.frag_numel(c.rB * f["vt_ld"], f["rope_cols"], BF) if f.get("qkv_packed") else (c.M - 1) * f["ldc"] + f["rope_cols"]
    elif c.epi == R.EPI_PIXSHUF:
        c_ext = c.M * c.N
    elif c.epi == R.EPI_PARTIAL:
        c_ext = (c.splitk * c.M - 1) * f["ldc"] + c.N
    elif f.get("out_packed"):
        c_ext = R.frag_numel(c.M, c.N, c.odt)
    else:
        c_ext = (c.M - 1) * f["ldc"] + c.N
    inside("C", d.C, d.strideC * es("C"), c_ext)
    nvec = c.N if c.epi != R.EPI_PIXSHUF else f["ps_C"]
    for name, ptr, step, ext in (("bias", d.bias, d.sb_bias, nvec), ("ln_s", d.ln_s, d.sb_ln_s, c.N),
                                 ("ln_stats", d.ln_stats, d.sb_ln_stats, c.M * f.get("ln_nt", 0) * 2),
                                 ("stats_out", d.stats_out, d.sb_stats_out, c.M * (c.N // 32) * 2),
                                 ("c2", d.c2, d.sb_c2, R.frag_numel(c.M, c.N, c.wdt)),
                                 ("vt", d.vt, d.sb_vt, getattr(c, "rB", 0) * f.get("heads", 0) * 64 * f.get("vt_ld", 0))):
        if ptr:
            inside(name, ptr, step, ext)
    for i in (1, 2):
        ptr = getattr(d, "res%d" % i)
        if ptr and not (i == 2 and f.get("res2_up_H")):
            inside("res%d" % i, ptr, c.M * f["ldr%d" % i] * es("res%d" % i), (c.M - 1) * f["ldr%d" % i] + c.N)
    assert (d.strideA < 0) == c.crossed and (d.sb_ln_stats < 0) == (c.crossed and bool(f.get("ln_stats")))


def test_every_census_row_is_constructible():
    """layout of every row and every extent of a dyn_n row: each index the builder or the comparison touches lies inside the
    extent the header's layout rule gives; small rows are materialised and run through the reference as well (no launch)"""
    from spann3r_amd import lib as L
    nc, built, run = _covered(), 0, 0
    for line, row in ROWS:
        if line in nc:
            continue
        for dyn in R.dyn_extents(row):
            cases = R.row_cases(row, line, dyn)
            assert len(cases) == len(row["descs"])
            for c in cases:
                f = c.f
                assert dyn is None or (dyn % 4 == 0 and 4 <= dyn <= (c.K if c.loader == R.LOAD_SOFTMAX else c.N))
                b = c.bufs
                # inputs: last element read by the logical extent
                if f.get("a_packed"):
                    assert int(R.frag_offsets(16, c.K1, c.adt).max()) + ((c.M + 15) // 16 - 1) * R.frag_numel(16, c.K1, c.adt) < c.strideA
                elif c.loader != R.LOAD_CONV3X3:
                    assert (c.M - 1) * c.lda + (c.K1 if c.loader == R.LOAD_PLAIN else c.K) <= c.strideA
                assert b["A"].numel >= c.batch * c.strideA and b["W"].numel >= c.batch * c.strideW
                if f.get("w_packed"):
                    assert R.frag_numel(c.N, c.ldw, c.wdt) <= c.strideW
                else:
                    assert (c.N - 1) * c.ldw + c.K <= c.strideW
                # outputs: the layout rule's extent per problem fits the stride, all problems fit the buffer
                assert b["C"].numel >= c.batch * c.strideC and b["C"].out
                if c.epi == R.EPI_ROPE_VT and f.get("qkv_packed"):
                    assert R.frag_numel(c.rB * f["vt_ld"], f["rope_cols"], BF) <= c.strideC
                    if "vt" in b:
                        assert int(R.pv_offsets(c.rB, f["heads"], f["tokens"], f["vt_ld"]).max()) < c.svt
                elif c.epi == R.EPI_PARTIAL:
                    assert c.splitk * c.M * f["ldc"] <= c.strideC
                elif c.epi == R.EPI_PIXSHUF:
                    assert c.M * c.N == c.strideC
                elif f.get("out_packed"):
                    assert R.frag_numel(c.M, c.N, c.odt) <= c.strideC
                else:
                    assert (c.M - 1) * f["ldc"] + (f["rope_cols"] if c.epi == R.EPI_ROPE_VT else c.N) <= c.strideC
                for n, per in (("c2", getattr(c, "sc2", 0)), ("stats_out", getattr(c, "sso", 0)), ("vt", getattr(c, "svt", 0))):
                    if n in b:
                        assert b[n].numel == c.batch * per and b[n].out
                if "sm_stats_out" in b:
                    assert b["sm_stats_out"].numel == c.M * ((c.N + 31) // 32) * 2
                # byte offsets keep the 16-byte alignment the library asks for
                for n, per in (("sbias", 4), ("sstats", 4), ("sso", 4), ("sc2", 2), ("svt", 2), ("strideA2", 2)):
                    assert (getattr(c, n, 0) * per) % 16 == 0, (line, n)
            built += 1
            if sum(c.nbytes() for c in cases) < 6e6:
                for c in cases:
                    c.materialize("cpu")
                    d = c.desc(L)
                    assert d.tile == -1 and d.A and d.W and d.C
                    _pointers_stay_inside(c, d)
                    exp, got = c.expected(), c.got()
                    for k in exp:
                        assert len(exp[k]) == len(got[k]) and all(a.shape == g.shape for a, g in zip(exp[k], got[k])), (line, k)
                        assert all(torch.isfinite(a).all() for a in exp[k]), (line, k)
                    # nothing has been launched: every output still holds the sentinel, every guard is intact
                    assert c.sentinel_faults() == [] and bool((got["C"][0].float() == R.SENT).all())
                run += 1
    print("census rows built: %d layouts (dyn_n rows at three extents), %d materialised and run through the reference" % (built, run))
    assert built == 605 - len(nc) + 2 * sum(1 for ln, r in ROWS if r["descs"][0].get("dyn_n") and ln not in nc) and run > 150


def test_compare_notices_a_wrong_group_and_a_stray_write():
    """the comparison itself: the reference written into the output passes; one 32-column group off by 1e-3 of ITS magnitude fails the
    group bound even where the whole-output norm would not see it; a write into a pad column or a guard band is reported"""
    line, row = next((ln, r) for ln, r in ROWS if r["lean"] == 0 and len(r["descs"]) == 1 and r["descs"][0].get("ldc", 0) > r["descs"][0]["N"]
                     and not r["descs"][0].get("loader") and not r["descs"][0].get("epi") and r["descs"][0]["M"] <= 256 and not r["descs"][0].get("out_bf16"))
    c = R.row_cases(row, line)[0].materialize("cpu")
    exp = c.expected()["C"][0].clone()
    exp[:, :32] *= 1e-3                                       # a small-magnitude region next to large ones
    c.expected = lambda: {"C": [exp]}
    view = c.got()["C"][0]
    view.copy_(exp.float())
    for n in ("sm_stats_out", "stats_out"):
        if n in c.bufs:
            c.bufs[n].body.zero_()
    fails = [f for f in R.compare(c)[0] if not f.startswith(("sm_stats_out", "stats_out"))]
    assert fails == [], fails
    view[:, :32] *= 1.001
    fails = [f for f in R.compare(c)[0] if f.startswith("C[0]")]
    assert len(fails) == 1 and "per 32-column group" in fails[0]
    assert R.block_errors(view, exp)[1] < 2e-5 < R.block_errors(view, exp)[0]
    view.copy_(exp.float())
    c.bufs["C"].body.view(c.M + 2, c.f["ldc"])[3, c.N] = 1.0
    c.bufs["C"].t[-1] = 0.0
    s = c.sentinel_faults()
    assert "C" in s and "C[0] pad" in s


def test_compare_holds_each_softmax_row_quantity_and_each_bf16_element():
    """sm_zout's three columns are three quantities: a zeroed 1/Z column, or a row max off by 1e-5, fails although the block as a whole
    (dominated by the row max) would not notice; a bf16 output one rounding step off in ONE small element fails the elementwise bound"""
    line, row = next((ln, r) for ln, r in ROWS if r["descs"][0].get("sm_zout") and r["lean"] == 0 and r["descs"][0]["K"] == 196 and not r["descs"][0].get("f32x3"))
    c = R.row_cases(row, line)[0].materialize("cpu")
    exp = c.expected()
    c.got()["C"][0].copy_(exp["C"][0].float())
    z = c.bufs["sm_zout"].body.view(c.M, 4)
    z[:, :3] = exp["sm_zout"][0].float()
    if "c2" in c.bufs:
        c.bufs["c2"].body[:R.frag_numel(c.M, c.N, c.wdt)].copy_(R.frag_pack(c.got()["C"][0].to(c.wdt), c.wdt))
    assert R.compare(c)[0] == []
    z[:, 2] = 0.0
    assert [f for f in R.compare(c)[0]] == ["sm_zout 1/Z: 1.000e+00 (bound 1.0e-05)"]
    z[:, 2] = exp["sm_zout"][0][:, 2].float()
    z[:, 1] *= 1.0 + 1e-5
    assert len(R.compare(c)[0]) == 1 and R.compare(c)[0][0].startswith("sm_zout row max")
    e = rnd(40, 64, seed=3) * 4
    e[:, 32:] *= 1e-3
    o = e.float().to(BF)
    assert R.bf16_excess(o, e) <= 1.0 and R.block_errors(o, e)[0] < 4e-3
    o[7, 40] = (o[7, 40].float() * (1 + 2.0 ** -7)).to(BF)                            # one step, in a small element of a small group
    assert R.bf16_excess(o, e) > 1.5 and R.block_errors(o, e)[1] < 4e-3


UP_ROWS = [(ln, r) for ln, r in ROWS if r["descs"][0].get("res2_up_H")]


def test_res2_up_rows_are_the_five():
    assert [ln for ln, _ in UP_ROWS] == [21, 25, 45, 75, 183]
    assert all(r["descs"][0].get("loader") == R.LOAD_CONV3X3 and r["descs"][0].get("out_bf16") and r["descs"][0].get("res_bf16") for _, r in UP_ROWS)


@pytest.mark.parametrize("line,row", UP_ROWS, ids=["L%d" % ln for ln, _ in UP_ROWS])
def test_res2_up_row_takes_either_rounding_of_the_upsampled_residual(line, row):
    """the answer to the census's open question, without a GPU.  An output built the way the kernel builds it -- the half-resolution
    residual interpolated in fp32 (conv_ref.emulate_upsample: sp3_upsample2x's arithmetic) and rounded to bf16, everything else exact,
    one rounding at the store -- is several times outside the elementwise bf16 bound against the float64-interpolated residual alone,
    and inside it once an element within the fp32 interpolation bound of a rounding boundary may take either neighbour.  At most 1 %
    of a row's elements have two candidates."""
    import conv_ref as CR
    c = R.row_cases(row, line)[0].materialize("cpu")
    f = c.f
    r = c.bufs["res2"].body.view(c.cB, f["res2_up_H"], f["res2_up_W"], c.N)
    kernel_res2 = CR.emulate_upsample(r, f["conv_OH"], f["conv_OW"]).to(BF).double().reshape(c.M, c.N)
    exp = c.expected()["C"][0]
    out = (exp - c.res[2][0] + kernel_res2).float().to(BF)
    c.got()["C"][0].copy_(out)
    flips = int((kernel_res2 != c.res[2][0]).sum())
    alone = R.bf16_excess(out, exp)
    fails, errs = R.compare(c)
    print("line %d: %d of %d residual elements on the other neighbour; alone %.1f x the bound, with candidates %.3f x; two-candidate share %.4f"
          % (line, flips, out.numel(), alone, errs["C bf16 steps"], c.res2_two))
    assert flips > 0 and alone > 3.0
    assert fails == [] and errs["C bf16 steps"] <= 1.0 and 0 < c.res2_two <= 0.01
    # the candidate rule is no licence: the residual's NEXT neighbour on a two-candidate element, or the other neighbour on a
    # one-candidate element, still fails
    lo, hi = (c.res[2] + c.res2_alt[0])[0], (c.res[2] + c.res2_alt[1])[0]
    i = int(((hi - lo) / (exp.abs() + 1e-3)).reshape(-1).argmax())         # (a two-candidate element whose residual step is large next to the output)
    bad = out.clone().reshape(-1)
    step = float(hi.reshape(-1)[i] - lo.reshape(-1)[i])
    bad[i] = (exp.reshape(-1)[i] - c.res[2][0].reshape(-1)[i] + hi.reshape(-1)[i] + step).float().to(BF)
    c.got()["C"][0].copy_(bad.view_as(out))
    assert any("elementwise bf16 bound" in s for s in R.compare(c)[0])
    j = int(((lo == hi) & (exp.abs() > 0.5)).reshape(-1).nonzero()[0])
    bad = out.clone().reshape(-1)
    bad[j] = (bad[j].float() * (1 + 2.0 ** -7)).to(BF)
    c.got()["C"][0].copy_(bad.view_as(out))
    assert any("elementwise bf16 bound" in s for s in R.compare(c)[0])
