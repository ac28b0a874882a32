"""sp3_conv3x3_tile in every form Engine.dpt_head launches it in (tests/conv_ref.py: MODEL_FORMS, read from the engine and held to it
by test_tile_forms_are_current), on every instance that accepts the form (8 x 8; 8 x 16 with 64 and with 32 output channels where
Cin % 128 == 0), plus the TIN = float instantiation, one fp32-in / bf16-out case and the smallest unit count (64 -> 64), against
float64.  Every buffer lies between guard bands (NaN around inputs, a sentinel around the NaN-filled output).  Per case:
  1. sentinels untouched, no NaN in the output body;
  2. the exact designs (`ones`, `impulse`) bit for bit;
  3. |got - ref| <= conv_ref.conv_bound per element (2e-5 of the 32-channel group's largest sum of magnitudes, plus half a bf16 step
     for a bf16 output), worst ratio printed;
  4. the whole-tensor bounds of test_conv3x3_tile, 2e-5 and 6e-3;
  5. the 32-channel and the 64-channel wide instance bit-equal.
The shares of the bound measured on an MI355X are in profiles/conv_forms.txt (SP3_CONV_REPORT=<file> appends one JSON line per launch)."""
import json
import os

import pytest
import torch

import conv_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CASES = [(f.name, "bf16") for f in CR.MODEL_FORMS] + [("rn0", "fp32"), ("u.c1", "fp32"), ("u1.c2", "fp32"), ("u.c1", "mixed"), ("c64", "bf16")]


def launch(b, form, dts, shape, inst):
    from spann3r_amd import lib as L
    f, (mdt, odt, rdt), (B, H, W) = CR.FORM[form], CR.DTYPES[dts], shape
    p = lambda n: 0 if b[n] is None else b[n].ptr()
    L.check(L.load().sp3_conv3x3_tile(p("x"), int(mdt == BF), p("w"), p("bias"), p("r1"), p("r2"), p("out"), int(odt == BF),
                                      int(rdt == BF and f.nres > 0), CR.TILE_PX[inst], B, H, W, f.Cin, f.Cout, int(f.relu_in), f.act,
                                      L.stream_ptr()), "sp3_conv3x3_tile")
    torch.cuda.synchronize()


def matrix():
    out = []
    for form, dts in CASES:
        f = CR.FORM[form]
        for group in ("8x8", "wide") if f.Cin % 128 == 0 else ("8x8",):
            for shape in CR.SHAPES[group]:
                for design in CR.designs(f):
                    out.append((form, dts, group, shape, design))
    return out


@pytest.mark.parametrize("form,dts,group,shape,design", matrix(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_form_against_float64(form, dts, group, shape, design):
    outs = {}
    for inst in (("8x8",) if group == "8x8" else ("8x16", "8x16n32")):
        b = CR.conv_buffers(form, dts, shape, design, DEV)
        launch(b, form, dts, shape, inst)
        fails, ratio = CR.judge_conv(form, dts, shape, design, b["out"], {k: v for k, v in b.items() if k != "out"})
        print("%-6s %-5s %-8s %-12s %-8s uses %.3f of the bound, %.3f of the slack" % (form, dts, inst, shape, design, ratio, CR.judge_conv.slack_share))
        if os.environ.get("SP3_CONV_REPORT"):
            with open(os.environ["SP3_CONV_REPORT"], "a") as fh:
                fh.write(json.dumps({"form": form, "dts": dts, "inst": inst, "shape": shape, "design": design, "ratio": ratio,
                                     "slack": CR.judge_conv.slack_share, "fails": fails}) + "\n")
        assert not fails, (inst, fails)
        outs[inst] = b["out"].body.clone()
    if group == "wide":
        assert torch.equal(outs["8x16"].view(torch.int16 if outs["8x16"].dtype == BF else torch.int32),
                           outs["8x16n32"].view(torch.int16 if outs["8x16"].dtype == BF else torch.int32))


def test_matrix_covers_the_table():
    m = matrix()
    for f in CR.MODEL_FORMS:
        for inst_group in (("8x8", "wide") if f.Cin % 128 == 0 else ("8x8",)):
            got = {d for form, dts, g, s, d in m if form == f.name and dts == "bf16" and g == inst_group}
            assert got == set(CR.designs(f)) and {"random", "ones"} <= got
    assert {(f, d) for f, d, *_ in m} >= {("rn0", "fp32"), ("u.c1", "fp32"), ("u1.c2", "fp32"), ("u.c1", "mixed"), ("c64", "bf16")}
    # the slow arm of the 8 x 8 halo loader (256 % chunks per pixel != 0): bf16 maps with 192 / 384 channels; several K chunks with it
    assert 256 % (192 // 8) and 256 % (384 // 8) and 256 % (768 // 4)


def test_tile_forms_are_current(full_sd):
    """every sp3_conv3x3_tile launch of Engine.dpt_head (both heads, bf16 and fp32, 224 x 224 at B = 1 and 9, 160 x 224 and 384 x 512 at
    B = 1) is a row of conv_ref.MODEL_FORMS: a model change that launches the tiled kernel in a form the tests above never ran fails here"""
    from spann3r_amd import Spann3R, FULL
    from spann3r_amd import lib as L
    m = Spann3R(dus3r_name=None, cfg=FULL, init_weights=False)
    m.load_state_dict(full_sd, strict=True)
    m = m.to(DEV).eval()
    l = L.load()
    orig = l.sp3_conv3x3_tile
    seen = {}

    def record(*a):
        seen.setdefault(CR.form_key(a[1], a[7], a[8], a[13], a[14], a[15], a[16], a[3], a[4], a[5]), []).append(a[10:13])
        return orig(*a)
    gen = torch.Generator().manual_seed(5)
    l.sp3_conv3x3_tile = record
    try:
        for prec in ("bf16", "fp32"):
            m.set_precision(prec)
            for B, H, W in ((1, 224, 224), (9, 224, 224), (1, 160, 224), (1, 384, 512)):
                nh, nw = H // FULL.patch, W // FULL.patch
                dec = [(torch.rand(B, nh * nw, FULL.enc_dim if i == 0 else FULL.dec_dim, generator=gen) * 2 - 1).to(DEV) for i in range(FULL.dec_depth + 1)]
                for num in (1, 2):
                    pts, conf, _ = m.engine.dpt_head(dec, B, nh, nw, num)
                    torch.cuda.synchronize()
                    assert bool(torch.isfinite(pts).all()) and bool(torch.isfinite(conf).all())
    finally:
        l.sp3_conv3x3_tile = orig
    keys = CR.table_keys()
    print("tiled-kernel forms launched: %s" % sorted(keys.get(k, "?") for k in seen))
    new = CR.unlisted(seen)
    assert not new, "launched in a form that is not in conv_ref.MODEL_FORMS (in_bf16, out_bf16, res_bf16, Cin, Cout, relu_in, act, bias, residuals): %r" % new
    assert {keys[k] for k in seen} >= {"rn0", "rn1", "u.c1", "u.c2", "u1.c2", "h0", "h2"}
