"""The 32-channel instance of the wide 3x3 convolution keeps a whole chunk of weights (9 units) in flight per wave; the 64-channel
instance keeps its 3-deep queue.  A deeper queue changes when a weight fragment is requested, never the order in which a wave adds its
(chunk, tap) products or the order in which the four waves' partial tiles are summed, so the two instances must agree bit for bit --
and both with F.conv2d in float64 on the bf16-rounded operands, at the tolerances of test_conv3x3_tile."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"

# B, H, W, Cin, Cout: one chunk (no refill at all) | two chunks, ragged in both directions | three chunks (refills across two chunk
# boundaries, the last chunk refills nothing) with B > 1 | the model's shape
SHAPES = [(1, 8, 16, 128, 64), (1, 9, 17, 256, 64), (2, 5, 20, 384, 128), (1, 56, 56, 256, 256)]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def bf(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _problem(B, H, W, Cin, Cout):
    """operands (CPU, NCHW) and the float64 convolutions of the bf16-rounded operands, with and without the input ReLU: computed once
    per shape, shared by every case, never written to"""
    x, w, b = rnd(B, Cin, H, W, seed=1), rnd(Cout, Cin, 3, 3, seed=2) * 0.05, rnd(Cout, seed=3)
    r1, r2 = rnd(B, Cout, H, W, seed=4), rnd(B, Cout, H, W, seed=5)
    wd = bf(w).double()
    conv = {relu: F.conv2d((F.relu(bf(x)) if relu else bf(x)).double(), wd, None, padding=1) for relu in (False, True)}
    return x, w, b, r1, r2, conv


@pytest.mark.parametrize("maps", ["bf16", "fp32"])
@pytest.mark.parametrize("variant", ["rcu1", "rcu2", "plain"])
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_conv_wide_n32_equals_n64_and_reference(B, H, W, Cin, Cout, variant, maps):
    from spann3r_amd import ops
    mdt = torch.bfloat16 if maps == "bf16" else torch.float32
    x, w, b, r1, r2, conv = _problem(B, H, W, Cin, Cout)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    wp = ops.PackedWeight(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV).to(torch.bfloat16))
    xin, bias, res1, res2 = nhwc(x).to(DEV).to(mdt), b.to(DEV), nhwc(r1).to(DEV), nhwc(r2).to(DEV)
    relu_in = variant != "plain"
    outs = {}
    for px in ("8x16n32", "8x16"):
        out = torch.full((B, H, W, Cout), float("nan"), device=DEV, dtype=mdt)
        kw = dict(B=B, H=H, W_=W, Cin=Cin, Cout=Cout, relu_in=relu_in, force_tile_kernel=True, tile_px=px)
        if variant == "rcu1":
            ops.conv3x3(xin, wp, out, bias=bias, act=ops.ACT_RELU, **kw)
        elif variant == "rcu2":
            ops.conv3x3(xin, wp, out, bias=bias, res1=res1, res2=res2, **kw)
        else:
            ops.conv3x3(xin, wp, out, **kw)
        outs[px] = out
    ref = conv[relu_in]
    if variant == "rcu1":
        ref = F.relu(ref + b.double().view(1, -1, 1, 1))
    elif variant == "rcu2":
        ref = ref + b.double().view(1, -1, 1, 1) + r1.double() + r2.double()
    err = rel_err(outs["8x16n32"].float().cpu(), nhwc(ref))
    same = torch.equal(outs["8x16n32"], outs["8x16"])
    print("n32 vs float64: %.3e   n32 == n64: %s" % (err, same))
    assert same
    assert err < (2e-5 if mdt == torch.float32 else 6e-3)
