"""DPT head launched by dependency level (ops.level / sp3_gemm_n) and the bilinear x2 folded into the consuming convolution's
epilogue (ops.conv3x3 res2_up): both keep every product, accumulation order and rounding point, so each check is bit for bit --
a level launch against the same problems launched one by one, the half-resolution residual against upsample2x + a plain res2,
and Engine.dpt_head with SP3_HEAD_LEVELS off against on."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _ops():
    from spann3r_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _conv_problem(ops, B, H, W, Cin, Cout, stride, variant, mdt, seed):
    """one small-map convolution of the head: (kwargs of ops.conv3x3 without `out`, output shape); tensors live in the dict"""
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = rnd(B, H, W, Cin, seed=seed).to(DEV).to(mdt)
    wp = ops.PackedWeight((rnd(Cout, 9 * Cin, seed=seed + 1) * 0.05).to(DEV).to(BF))
    kw = dict(x=x, Wp=wp, B=B, H=H, W_=W, Cin=Cin, Cout=Cout, stride=stride)
    if variant != "plain":
        kw["bias"] = rnd(Cout, seed=seed + 2).to(DEV)
    if variant == "rcu1":
        kw.update(relu_in=True, act=ops.ACT_RELU)
    if variant == "rcu2":
        kw.update(relu_in=True, res1=rnd(B, OH, OW, Cout, seed=seed + 3).to(DEV).to(mdt), res2=rnd(B, OH, OW, Cout, seed=seed + 4).to(DEV).to(mdt))
    return kw, (B, OH, OW, Cout)


def _run_convs(ops, probs, mdt, merged):
    import contextlib
    outs = [torch.full(shape, float("nan"), device=DEV, dtype=mdt) for _, shape in probs]
    with (ops.level() if merged else contextlib.nullcontext()):
        for (kw, _), o in zip(probs, outs):
            kw = dict(kw)
            ops.conv3x3(kw.pop("x"), kw.pop("Wp"), o, **kw)
    torch.cuda.synchronize()
    return outs


# the head's levels: (nh, nw) token grids 14 x 14 (224 x 224) and 10 x 14 (160 x 224: the stride-2 map is 5 x 7)
def _levels(B, nh, nw):
    h3, w3 = (nh - 1) // 2 + 1, (nw - 1) // 2 + 1
    return {
        "pp3c+rn2": [(B, nh, nw, 768, 768, 2, "bias"), (B, nh, nw, 384, 256, 1, "plain")],
        "rn1+rn3+ref3.u1.c1": [(B, 2 * nh, 2 * nw, 192, 256, 1, "plain"), (B, h3, w3, 768, 256, 1, "plain"), (B, nh, nw, 256, 256, 1, "rcu1")],
        "ref4.u2.c1+ref2.u1.c1": [(B, h3, w3, 256, 256, 1, "rcu1"), (B, 2 * nh, 2 * nw, 256, 256, 1, "rcu1")],
        "four": [(B, h3, w3, 256, 256, 1, "rcu2"), (B, nh, nw, 256, 256, 1, "rcu2"), (B, h3, w3, 768, 256, 1, "plain"), (B, nh, nw, 384, 256, 1, "bias")],
    }


@pytest.mark.parametrize("maps", ["bf16", "fp32"])
@pytest.mark.parametrize("B,nh,nw", [(1, 14, 14), (1, 10, 14), (9, 14, 14), (9, 10, 14)])
@pytest.mark.parametrize("name", ["pp3c+rn2", "rn1+rn3+ref3.u1.c1", "ref4.u2.c1+ref2.u1.c1", "four"])
def test_conv_level_equals_single_launches(name, B, nh, nw, maps):
    ops = _ops()
    mdt = BF if maps == "bf16" else torch.float32
    probs = [_conv_problem(ops, *p, mdt, seed=10 * i) for i, p in enumerate(_levels(B, nh, nw)[name])]
    one = _run_convs(ops, probs, mdt, merged=False)
    lvl = _run_convs(ops, probs, mdt, merged=True)
    for a, b in zip(one, lvl):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0


def test_conv_level_is_one_launch():
    """the three small-map convolutions of a level reach the library as ONE sp3_gemm_n call (a map the LDS-tiled kernel takes goes
    out on its own, before the group)"""
    ops = _ops()
    probs = [_conv_problem(ops, *p, BF, seed=10 * i) for i, p in enumerate(_levels(1, 14, 14)["rn1+rn3+ref3.u1.c1"])]
    probs.append(_conv_problem(ops, 1, 56, 56, 128, 256, 1, "plain", BF, seed=77))
    sent = []
    send = ops.level._send
    ops.level._send = staticmethod(lambda group, is_conv: (sent.append((len(group), is_conv)), send(group, is_conv))[1])
    try:
        _run_convs(ops, probs, BF, merged=True)
    finally:
        ops.level._send = staticmethod(send)
    assert sent == [(3, True)]


@pytest.mark.parametrize("maps", ["bf16", "fp32"])
@pytest.mark.parametrize("B,R", [(1, 196), (9, 1764), (1, 140)])
def test_gemm_level_equals_pairs(B, R, maps):
    """the four act_postprocess 1x1 convolutions (fp32 hooks, differently shaped) as one launch against two ops.pair() launches"""
    ops = _ops()
    mdt = BF if maps == "bf16" else torch.float32
    dims, ld = (1024, 768, 768, 768), (96, 192, 384, 768)
    A = [rnd(R, dims[i], seed=i).to(DEV) for i in range(4)]
    Ws = [ops.PackedWeight((rnd(ld[i], dims[i], seed=20 + i) * 0.05).to(DEV).to(BF)) for i in range(4)]
    bias = [rnd(ld[i], seed=40 + i).to(DEV) for i in range(4)]
    res = {}
    for mode in ("pairs", "level"):
        outs = [torch.full((R, ld[i]), float("nan"), device=DEV, dtype=mdt) for i in range(4)]
        issue = lambda i: ops.gemm(A[i], Ws[i], outs[i], M=R, N=ld[i], K=dims[i], lda=dims[i], ldc=ld[i], bias=bias[i])
        if mode == "pairs":
            for i0 in (0, 2):
                with ops.pair():
                    issue(i0), issue(i0 + 1)
        else:
            with ops.level():
                for i in range(4):
                    issue(i)
        torch.cuda.synchronize()
        res[mode] = outs
    for a, b in zip(res["pairs"], res["level"]):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()) and float(a.float().abs().max()) > 0


@pytest.mark.parametrize("maps", ["bf16"])
@pytest.mark.parametrize("B,h,w,OH,OW", [(1, 7, 7, 14, 14), (1, 5, 7, 10, 14), (2, 4, 4, 7, 7), (1, 14, 14, 28, 28), (1, 10, 14, 20, 28), (9, 7, 7, 14, 14),
                                         (3, 9, 5, 18, 10)])
def test_half_resolution_residual_equals_upsample_then_add(B, h, w, OH, OW, maps):
    """u1.c2 of a refinenet with res2 = the previous refinenet's out_conv result at half resolution (also cropped, dust3r/heads/
    dpt_head.py:57, and H != W) against upsample2x into memory + the plain res2; tiles 40 and 41"""
    ops = _ops()
    mdt = BF if maps == "bf16" else torch.float32
    F_ = 256
    kw, shape = _conv_problem(ops, B, OH, OW, F_, F_, 1, "rcu2", mdt, seed=3)
    src = rnd(B, h, w, F_, seed=9).to(DEV).to(mdt)
    up = torch.full((B, OH, OW, F_), float("nan"), device=DEV, dtype=mdt)
    ops.upsample2x(src, up, B=B, H=h, W_=w, C_=F_, outH=OH, outW=OW)
    outs = []
    for fold in (False, True):
        k = dict(kw)
        k["res2"] = src if fold else up
        o = torch.full(shape, float("nan"), device=DEV, dtype=mdt)
        ops.conv3x3(k.pop("x"), k.pop("Wp"), o, res2_up=(h, w) if fold else None, **k)
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0].float()).all())
    plain = dict(kw)
    plain["res2"] = None
    o = torch.full(shape, float("nan"), device=DEV, dtype=mdt)
    ops.conv3x3(plain.pop("x"), plain.pop("Wp"), o, **plain)
    assert not torch.equal(o, outs[0])                        # (the residual is not a no-op in this test)


def test_half_resolution_residual_is_refused_elsewhere():
    """only the lean small-map kernels read a half-resolution res2: the LDS-tiled kernel's maps raise instead of reading it as a full map"""
    ops = _ops()
    kw, shape = _conv_problem(ops, 1, 56, 56, 256, 256, 1, "rcu2", BF, seed=3)
    o = torch.zeros(shape, device=DEV, dtype=BF)
    with pytest.raises(ValueError):
        ops.conv3x3(kw.pop("x"), kw.pop("Wp"), o, res2_up=(28, 28), **kw)
    # fp32 maps: the library has no kernel that reproduces the fp32 upsample's bits, the plan says so
    kw, shape = _conv_problem(ops, 1, 14, 14, 256, 256, 1, "rcu2", torch.float32, seed=3)
    o = torch.zeros(shape, device=DEV)
    with pytest.raises(ValueError):
        ops.conv3x3(kw.pop("x"), kw.pop("Wp"), o, res2_up=(7, 7), **kw)


@pytest.fixture(scope="module")
def full_model(full_sd):
    from spann3r_amd import Spann3R, FULL
    m = Spann3R(dus3r_name=None, cfg=FULL, init_weights=False)
    m.load_state_dict(full_sd, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("B,H,W", [(1, 224, 224), (9, 224, 224), (1, 160, 224)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_dpt_head_schedules_agree(full_model, precision, B, H, W):
    """Engine.dpt_head, both heads: the launch-per-op schedule (SP3_HEAD_LEVELS=0) and the level schedule give the same bits"""
    from spann3r_amd import FULL
    ops = _ops()
    full_model.set_precision(precision)
    eng = full_model.engine
    nh, nw = H // FULL.patch, W // FULL.patch
    dims = (FULL.enc_dim, FULL.dec_dim)
    dec = [rnd(B, nh * nw, dims[0] if i == 0 else dims[1], seed=i).to(DEV) for i in range(FULL.dec_depth + 1)]
    keep = ops.HEAD_LEVELS
    res = {}
    try:
        for lv in (False, True):
            ops.HEAD_LEVELS = lv
            for num in (1, 2):
                pts, conf, raw = eng.dpt_head(dec, B, nh, nw, num, want_raw=True)
                torch.cuda.synchronize()
                res[(lv, num)] = [t.clone() for t in (pts, conf, raw)]
    finally:
        ops.HEAD_LEVELS = keep
    for num in (1, 2):
        for a, b in zip(res[(False, num)], res[(True, num)]):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
