"""ops._conv_route is the host's one 3x3-convolution rule (LDS-tiled kernel, lean small-map instance, or a general tile with or
without split-K).  It is host code over sp3_gemm_plan, so every arm is checked here without a GPU; the expected routes, lean
instances and K splits are those of the wrapper before the rule had a function of its own."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32

# (weights dtype, packed, map dtype, B, H, W, Cin, Cout, stride, force_tile_kernel) -> (route, lean instance | None, conv_splitk | None)
ROWS = [
    ((BF, True, BF, 1, 56, 56, 128, 256, 1, False), ("tile", None, None)),
    ((BF, True, BF, 1, 28, 28, 192, 256, 1, False), ("lean", 41, None)),
    ((BF, True, BF, 1, 14, 14, 384, 256, 1, False), ("lean", 40, None)),
    ((BF, True, BF, 1, 7, 7, 768, 256, 1, False), ("lean", 40, None)),
    ((BF, True, BF, 1, 14, 14, 768, 768, 2, False), ("lean", 40, None)),
    ((BF, True, BF, 9, 28, 28, 256, 256, 1, False), ("tile", None, None)),
    ((BF, True, BF, 2, 28, 28, 256, 256, 1, False), ("lean", 41, None)),             # 1568 pixels
    ((BF, True, BF, 1, 32, 64, 256, 256, 1, False), ("tile", None, None)),           # exactly 2048 pixels
    ((BF, True, F32, 1, 14, 14, 256, 256, 1, False), ("lean", 40, None)),
    ((F32, True, F32, 1, 14, 14, 256, 256, 1, False), ("general", None, 8)),
    ((F32, True, F32, 1, 56, 56, 256, 256, 1, False), ("general", None, 1)),
    ((BF, True, F32, 1, 56, 56, 96, 256, 1, False), ("general", None, 1)),
    ((BF, True, F32, 1, 14, 14, 96, 256, 1, False), ("general", None, 2)),
    ((BF, False, F32, 1, 14, 14, 256, 256, 1, False), ("general", None, 8)),         # a plain [Cout, 9 Cin] tensor
    ((BF, True, BF, 1, 14, 1, 256, 256, 1, False), ("general", None, None)),         # one-column map: no lean instance takes it
    ((BF, True, BF, 1, 8, 8, 64, 192, 1, True), ("tile", None, None)),
]

_weights = {}


def _weight(wdt, packed, Cin, Cout):
    from spann3r_amd import ops
    key = (wdt, packed, Cin, Cout)
    if key not in _weights:
        w = torch.zeros(Cout, 9 * Cin, dtype=wdt)
        _weights[key] = ops.PackedWeight(w) if packed else w
    return _weights[key]


@pytest.mark.parametrize("case,want", ROWS, ids=["%s%s-%s-%dx%dx%d-%dto%d-s%d%s" % (
    "bf16" if c[0] == BF else "f32", "p" if c[1] else "", "bf16" if c[2] == BF else "f32", *c[3:9], "-forced" if c[9] else "") for c, _ in ROWS])
def test_conv_route(case, want):
    from spann3r_amd import lib, ops
    wdt, packed, mdt, B, H, W_, Cin, Cout, stride, force = case
    Wp = _weight(wdt, packed, Cin, Cout)
    d = ops._conv_desc(Wp, mdt, mdt, mdt, B=B, H=H, W_=W_, Cin=Cin, Cout=Cout, stride=stride, act=ops.ACT_NONE, relu_in=False, res2_up=None)
    assert (d.loader, d.epi, d.tile, d.K, d.N, d.conv_stride) == (lib.LOAD_CONV3X3, lib.EPI_PLAIN, -1, 9 * Cin, Cout, stride)
    assert d.M == B * ((H - 1) // stride + 1) * ((W_ - 1) // stride + 1)
    assert not d.A and not d.C                              # (the pointers are the caller's; the route probes a copy)
    route, plan, splitk = want
    assert ops._conv_route(d, Wp, force_tile_kernel=force) == route
    assert not d.A and not d.C
    if plan is not None:
        d.A = d.C = 4096
        assert lib.load().sp3_gemm_plan(C.byref(d)) == plan
    if splitk is not None:
        assert ops.conv_splitk(d.M, Cout, 9 * Cin, Wp.dtype) == splitk
    # a caller that names a general tile never leaves the general kernel
    assert ops._conv_route(d, Wp, tile=0, force_tile_kernel=force) == "general"


def test_conv3x3_takes_res2_up_asks_the_rule():
    """the DPT head folds the bilinear x2 into the consuming convolution exactly where that convolution runs on a lean instance"""
    from spann3r_amd import ops
    Wp = _weight(BF, True, 256, 256)
    assert ops.conv3x3_takes_res2_up(Wp, BF, 1, 14, 14) is True
    assert ops.conv3x3_takes_res2_up(Wp, BF, 1, 56, 56) is False
    assert ops.conv3x3_takes_res2_up(Wp, BF, 1, 14, 1) is False      # (the lean instances refuse one-column maps)
    assert ops.conv3x3_takes_res2_up(Wp, F32, 1, 14, 14) is False


def _takes_14x14():
    from spann3r_amd import ops
    print("takes", ops.conv3x3_takes_res2_up(_weight(BF, True, 256, 256), BF, 1, 14, 14), flush=True)


def test_conv3x3_takes_res2_up_lean_instances_off():
    """SP3_LEAN_GEMM is read once per process: asked in a child process with the lean instances off"""
    env = dict(os.environ, SP3_LEAN_GEMM="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "import sys; sys.path.insert(0, %r); import test_conv_route_cpu as t; t._takes_14x14()" % os.path.join(REPO, "tests")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "takes False" in out.stdout, out.stdout + out.stderr


def test_conv3x3_tile_refuses_flags_that_are_not_plain():
    """sp3_conv3x3_tile's out_bf16 / res_bf16 are 0 or 1 and tile_px is 0..3: anything else is refused before a launch (null stream,
    no GPU) -- a C "true" other than 1 selects nothing"""
    from spann3r_amd import lib
    l = lib.load()
    for flags, name in (((2, 0, 0), b"out_bf16"), ((5, 0, 0), b"out_bf16"), ((1, 2, 0), b"res_bf16"), ((1, -1, 0), b"res_bf16"),
                        ((1, 1, 4), b"tile_px"), ((0, 0, -1), b"tile_px")):
        assert l.sp3_conv3x3_tile(4096, 1, 4096, None, None, None, 4096, *flags, 1, 8, 8, 64, 64, 0, 0, None) != 0, flags
        assert name in l.sp3_last_error(), (flags, l.sp3_last_error())
