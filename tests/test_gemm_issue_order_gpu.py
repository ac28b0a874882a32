"""The lean instances whose K loop queues its operand loads in a pinned order by separate depths (csrc/gemm_sm.hip, sm_kernel with
WD / AD): tile 35 (value-encoder fc2, K = 4096) and tile 37 (decoder fc2, K = 3072) through ops.gemm with residual, per-32-column
statistics and the fragment-order bf16 copy; tile 32 (value-encoder fc1, K = 1024) through ops.gemm with the folded LayerNorm and
GELU; tile 30 (value-encoder q/k/v, K = 1024) through ops.proj_rope_vt -- as the engine launches them, with the instance's own K, at
  M = 196, N = one z-slot of 8 N-tiles   the ragged last M-tile with its clamped row blocks, every wave's whole k-walk
  M = 16,  N = one z-slot                a single row block: every other row block of the tile is the clamped one
  M = 196, full N                        the launch of the model (tile 37: both decoder sides as a grouped launch)
against float64 on the rounded operands by the formulas of tests/gemm_desc_ref.py and the bounds test_gemm_lean_gpu.py holds the
instance to (fp32 rows 2e-5, statistics 1e-5, packed copy bit for bit; fc1's bf16 output 4e-3; q / k / v 8e-3), bit-equal between
the weight cache policies 0 and 1 and over two runs."""
import functools

import pytest
import torch

import gemm_desc_ref as R
import test_gemm_lean_gpu as TL
from conftest import rel_err  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

CASES = [(35, 196, 256, 4096, 1), (35, 16, 256, 4096, 1), (35, 196, 1024, 4096, 1),
         (37, 196, 256, 3072, 1), (37, 16, 256, 3072, 1), (37, 196, 768, 3072, 2)]


@pytest.fixture(autouse=True)
def _mode_restored():
    from spann3r_amd import lib as L
    before = L.load().sp3_weight_stream_get()
    yield
    assert L.load().sp3_weight_stream_set(before) == 0


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, G):
    """operands on the CPU and the float64 result of every problem of the launch (computed once, never written again)"""
    Ad = [TL.rnd(M, K, seed=1 + g) for g in range(G)]
    for a in Ad:
        a[:, 0] += torch.arange(M) * (3.0 / M)                   # a ramp down the rows: a row block read from the wrong place shows
    Wd = [TL.rnd(N, K, seed=10 + g) * 0.05 for g in range(G)]
    bias, res = TL.rnd(G, N, seed=5), TL.rnd(G, M, N, seed=6) * 2 + 0.3
    ref = [R.bf(Ad[g]).double() @ R.bf(Wd[g]).double().T + bias[g].double() + res[g].double() for g in range(G)]
    return Ad, Wd, bias, res, ref


def _launch(ops, tile, M, N, K, G, A, Ws, bias, res):
    out = torch.full((G, M, N), float("nan"), device=DEV)
    so = torch.full((G, M, N // 32, 2), float("nan"), device=DEV)
    c2 = ops.PackedAct.group(G, M, N, BF, DEV)
    kw = dict(M=M, N=N, K=K, lda=K, ldc=N, bias=bias, res1=res, ldr1=N, stats_out=so, c2=c2)
    if G > 1:
        kw.update(batch=G, strideA=A.stride, strideW=Ws.stride, strideC=M * N, sb={"bias": N * 4, "stats_out": M * (N // 32) * 8, "c2": c2.stride * 2})
    planned = TL._plan_of(ops, lambda: ops.gemm(A, Ws, out, **kw))
    assert planned == [tile], planned
    torch.cuda.synchronize()
    return out, so, c2


@pytest.mark.parametrize("tile,M,N,K,G", CASES, ids=["t%d-M%d-N%dx%d" % (t, m, n, g) for t, m, n, _, g in CASES])
def test_separate_depth_instances(tile, M, N, K, G):
    from spann3r_amd import lib as L
    ops = TL._ops()
    Ad, Wd, bias, res, ref = _problem(M, N, K, G)
    A = ops.PackedAct.group(G, M, K, BF, DEV)
    for g in range(G):
        A.at(g).data.view(-1)[:A.stride].copy_(ops.PackedAct.from_dense(Ad[g].to(DEV).to(BF)).data.view(-1))
    Ws = ops.PackedWeightGroup([ops.PackedWeight(w.to(DEV).to(BF)) for w in Wd])
    bias_d, res_d = bias.to(DEV), res.to(DEV)
    runs = {}
    for name, mode in (("default", 0), ("shipped", 1), ("again", 1)):
        L.check(L.load().sp3_weight_stream_set(mode), "sp3_weight_stream_set")
        runs[name] = _launch(ops, tile, M, N, K, G, A, Ws, bias_d, res_d)
    out, so, c2 = runs["shipped"]
    for g in range(G):
        got = out[g].cpu()
        assert not torch.isnan(got).any()
        blk, allv = R.block_errors(got, ref[g])
        print("tile %d M=%d N=%d problem %d: per 32-column group %.3e, whole %.3e" % (tile, M, N, g, blk, allv))
        assert blk < 2e-5 and allv < 2e-5, (g, blk, allv)
        assert torch.equal(TL._dense(ops, c2, g, M, N), out[g].to(BF))
        xr, st = got.double(), so[g].cpu().double()
        want = torch.stack((xr.reshape(M, N // 32, 32).sum(-1), (xr * xr).reshape(M, N // 32, 32).sum(-1)), -1)
        for j in (0, 1):
            e = float(((st[..., j] - want[..., j]).abs().amax(0) / want[..., j].abs().amax(0).clamp_min(1e-30)).max())
            assert e < 1e-5, (g, j, e)
    for other in ("default", "again"):
        o2, s2, p2 = runs[other]
        for what, x, y in (("rows", o2, out), ("statistics", s2, so), ("packed copy", p2.data, c2.data)):
            assert torch.equal(x, y), "%s: %s differ from the shipped policy's run" % (other, what)


def _three_runs(launch):
    """launch() under the default policy, the shipped table, and the shipped table again -> the three lists of output tensors"""
    from spann3r_amd import lib as L
    runs = []
    for mode in (0, 1, 1):
        L.check(L.load().sp3_weight_stream_set(mode), "sp3_weight_stream_set")
        runs.append(launch())
        torch.cuda.synchronize()
    for other, what in ((runs[0], "default policy"), (runs[2], "second run")):
        for i, (x, y) in enumerate(zip(other, runs[1])):
            assert torch.equal(x, y), "%s: output %d differs from the shipped policy's run" % (what, i)
    return runs[1]


@functools.lru_cache(maxsize=None)
def _ln_problem(M, N, K):
    """one problem with a folded LayerNorm in front: fp32 rows x (statistics are its partials), W' = W * gamma, bias; float64 y = LN-fold + bias"""
    x = TL.rnd(M, K, seed=1) * 2 + 0.2
    x[:, 0] += torch.arange(M) * (3.0 / M)
    W = TL.rnd(N, K, seed=2) * 0.05 * (TL.rnd(K, seed=31) * 0.3 + 1)[None, :]
    b = TL.rnd(N, seed=3)
    st = torch.stack((x.reshape(M, K // 32, 32).sum(-1), (x * x).reshape(M, K // 32, 32).sum(-1)), -1).contiguous()
    s_n = R.bf(W).sum(1)
    y = R.ln_fold_apply(R.bf(x).double() @ R.bf(W).double().T, st, K, R.LN_EPS, s_n) + b.double()[None]
    return x, W, b, st, s_n, y


FC1 = [(196, 512), (16, 512), (196, 4096)]


@pytest.mark.parametrize("M,N", FC1, ids=["t32-M%d-N%d" % c for c in FC1])
def test_value_encoder_fc1(M, N):
    """tile 32: norm2 (folded) + fc1 + GELU into fragment order (croco/models/blocks.py:74-75)"""
    ops = TL._ops()
    K = 1024
    x, W, b, st, s_n, y = _ln_problem(M, N, K)
    A = ops.PackedAct.from_dense(x.to(DEV).to(BF))
    Wp = ops.PackedWeight(W.to(DEV).to(BF))
    lnf = ops.LnFold(st.to(DEV), K, s_n.to(DEV), R.LN_EPS)
    bias = b.to(DEV)

    def launch():
        h = ops.PackedAct(M, N, BF, DEV)
        planned = TL._plan_of(ops, lambda: ops.gemm(A, Wp, h, M=M, N=N, K=K, lda=K, ldc=N, bias=bias, act=ops.ACT_GELU, ln=lnf))
        assert planned == [32], planned
        return [h.data]
    (data,) = _three_runs(launch)
    got = ops.PackedAct(M, N, BF, DEV, data=data).to_dense().float().cpu()
    err = rel_err(got, R.gelu(y))
    print("tile 32 M=%d N=%d: %.3e" % (M, N, err))
    assert err < 4e-3


QKV = [(196, 512, "q"), (16, 512, "q"), (196, 3072, "qkv")]


@pytest.mark.parametrize("P,N,kind", QKV, ids=["t30-M%d-N%d" % c[:2] for c in QKV])
def test_value_encoder_qkv(P, N, kind):
    """tile 30: norm1 (folded) + q/k/v projection + bias + 2-D RoPE, q / k in fragment order padded to 64-token blocks, V in PV-operand
    order (croco/models/blocks.py:94-112); one image of P tokens"""
    from spann3r_amd.engine import _rope_tables
    ops = TL._ops()
    K = 1024
    rc = N if kind == "q" else 2 * K
    heads = rc // 64 if kind == "q" else K // 64
    npad = (P + 63) // 64 * 64
    nh = 14 if P == 196 else 4
    x, W, b, st, s_n, y = _ln_problem(P, N, K)
    A = ops.PackedAct.from_dense(x.to(DEV).to(BF))
    Wp = ops.PackedWeight(W.to(DEV).to(BF))
    lnf = ops.LnFold(st.to(DEV), K, s_n.to(DEV), R.LN_EPS)
    bias = b.to(DEV)
    pos = TL._pos(1, nh, P // nh).reshape(-1, 2).to(torch.int32)
    cos, sin = _rope_tables(64, 100.0, DEV)
    pos_d = pos.to(DEV)

    def launch():
        qkp = ops.PackedAct(npad, rc, BF, DEV)
        vtp = torch.zeros(heads * npad * 64, device=DEV, dtype=BF) if rc < N else None
        planned = TL._plan_of(ops, lambda: ops.proj_rope_vt(A, Wp, bias, qkp.data, 0, vtp, npad, M=P, N=N, K=K, lda=K, rope_cols=rc, pos=pos_d, cos=cos,
                                                            sin=sin, tokens=P, heads=heads, qkv_packed=True, ln=lnf))
        assert planned == [30], planned
        return [qkp.data] + ([vtp] if vtp is not None else [])
    outs = _three_runs(launch)
    qk = ops.PackedAct(npad, rc, BF, DEV, data=outs[0]).to_dense().float().cpu()
    want = R.rope_cols_apply(y[:, :rc], pos, cos.cpu(), sin.cpu())
    err = rel_err(qk[:P], want)
    print("tile 30 M=%d N=%d: q/k %.3e" % (P, N, err))
    assert err < 8e-3
    assert float(qk[P:].abs().max()) == 0.0 if npad > P else True
    if rc < N:
        v = outs[1].cpu()[R.pv_offsets(1, heads, P, npad)].float()
        errv = rel_err(v, y[:, rc:].reshape(1, P, heads, 64))
        print("tile 30 M=%d N=%d: v %.3e" % (P, N, errv))
        assert errv < 8e-3
