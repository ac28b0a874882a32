"""tests/conv_ref.py on the CPU: the float64 convolution reference is F.conv2d; the fp32 emulation of both tiled kernels stays inside
the elementwise bound on every data design (the share it uses is printed: profiles/conv_forms.txt); every mutant of the emulation is
caught by a design; the half-resolution residual finding of the GEMM census (fp32 interpolation against float64, both rounded to bf16)
is reproduced; the bilinear x2 and head_final bounds hold for fp32 emulations of those kernels."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import gemm_desc_ref as R

BF, F32 = torch.bfloat16, torch.float32
# (form, dtypes) of tests/test_conv_forms_gpu.py
CASES = [(f.name, "bf16") for f in CR.MODEL_FORMS] + [("rn0", "fp32"), ("u.c1", "fp32"), ("u1.c2", "fp32"), ("u.c1", "mixed"), ("c64", "bf16")]


@pytest.mark.parametrize("form,dts", CASES, ids=["%s-%s" % c for c in CASES])
def test_reference_is_conv2d(form, dts):
    f = CR.FORM[form]
    for shape in ((2, 3, 5), (1, 1, 1)):
        for design in CR.designs(f):
            d = CR.conv_data(form, dts, shape, design)
            x = d.x.float()
            x = F.relu(x) if f.relu_in else x
            w4 = d.w.double().reshape(f.Cout, 3, 3, f.Cin).permute(0, 3, 1, 2)
            y = F.conv2d(CR.bf(x).double().permute(0, 3, 1, 2), w4, None if d.bias is None else d.bias.double(), padding=1).permute(0, 2, 3, 1)
            if f.act == CR.ACT_RELU:
                y = F.relu(y)
            for r in (d.r1, d.r2):
                y = y if r is None else y + r.double()
            ref, S = CR.conv_reference(form, dts, shape, design)
            assert float((ref - y).abs().max()) <= 1e-12 * max(float(S.max()), 1.0), (shape, design)
            assert bool((S + 1e-12 >= ref.abs()).all())
            if design == "cancel":                      # the design's point: outputs small next to S
                assert float(ref.abs().median()) < 0.05 * float(S.median())


def test_designs_are_what_they_say():
    e = CR.impulse_entries(768, 256)
    assert {t for _, t, _ in e} == set(range(9)) and {c for _, _, c in e} == {0, 31, 32, 63, 64, 127, 128, 767}
    assert {c for _, _, c in CR.impulse_entries(64, 64)} == {0, 31, 32, 63} and {t for _, t, _ in CR.impulse_entries(64, 64)} == set(range(9))
    d = CR.conv_data("u.c1", "bf16", (2, 17, 17), "impulse")
    assert int((d.w != 0).sum()) == 256 and bool(((d.w != 0).sum((1, 2)) == 1).all())
    n = CR.conv_data("u.c1", "bf16", (2, 17, 17), "negative").x.float()
    assert 0.85 < float((n < 0).float().mean()) < 0.95
    sub = 2.0 ** -133
    assert bool((n == sub).any()) and bool((n == -sub).any()) and bool(((n == 0) & torch.signbit(n)).any())
    ex = CR.exact_expected("rn0", "bf16", (2, 17, 17), "ones").float()
    assert float(ex[0, 0, 0, 0]) == 4 * 128 and float(ex[1, 0, 5, 3]) == 6 * 128 and float(ex[1, 8, 8, 255]) == 9 * 128
    assert float(CR.exact_expected("rn3", "bf16", (1, 1, 1), "ones")[0, 0, 0, 0]) == 768.0


@pytest.mark.parametrize("form,dts", CASES, ids=["%s-%s" % c for c in CASES])
def test_emulation_stays_inside_the_bound(form, dts):
    """both instances' summation orders, every design, at the shapes of the GPU test; prints the share of the bound used"""
    f = CR.FORM[form]
    for inst in CR.instances(f):
        if inst == "8x16n32":
            continue                                    # (the same order as 8x16: the GPU test holds the two bit-equal)
        for shape in CR.SHAPES["8x8" if inst == "8x8" else "wide"]:
            for design in CR.designs(f):
                out = CR.emulate_conv(form, dts, shape, design, inst)
                fails, ratio = CR.judge_conv(form, dts, shape, design, out)
                print("emulation %-6s %-5s %-5s %-12s %-8s uses %.3f of the bound, %.3f of the slack" % (form, dts, inst, shape, design, ratio, CR.judge_conv.slack_share))
                assert not fails, (inst, shape, design, fails)


MUT_SHAPE = {"8x8": (2, 9, 9), "8x16": (2, 9, 17), "8x16n32": (2, 9, 17)}
MUT_CASES = [("u.c1", "bf16"), ("u1.c2", "bf16"), ("u1.c2", "fp32"), ("c64", "bf16"), ("rn1", "bf16")]


def test_every_mutant_is_caught():
    """each mutant of the emulation leaves the bound, breaks an exact design or writes a sentinel in at least one case; prints which
    design catches which"""
    caught = {m: set() for m in CR.MUTANTS}
    for form, dts in MUT_CASES:
        f = CR.FORM[form]
        for inst in CR.instances(f):
            shape = MUT_SHAPE[inst]
            for design in CR.designs(f):
                assert CR.judge_conv(form, dts, shape, design, CR.emulate_conv(form, dts, shape, design, inst))[0] == []
                for m in CR.MUTANTS:
                    fails, _ = CR.judge_conv(form, dts, shape, design, CR.emulate_conv(form, dts, shape, design, inst, mutant=m))
                    if fails:
                        caught[m].add((design, fails[0].split(":")[0].split(" (")[0]))
    for m in CR.MUTANTS:
        by = {}
        for design, how in sorted(caught[m]):
            by.setdefault(design, []).append(how)
        print("mutant %-15s caught by: %s" % (m, "; ".join("%s (%s)" % (d, ", ".join(sorted(set(h)))) for d, h in by.items()) or "NOTHING"))
    assert all(caught[m] for m in CR.MUTANTS), [m for m in CR.MUTANTS if not caught[m]]
    # the designs earn their place: the exact ones see what they were built for
    assert any(d == "ones" for d, _ in caught["halo_bottom"]) and any(d == "ones" for d, _ in caught["halo_right"])
    assert any(d == "impulse" for d, _ in caught["swap_kykx"])
    assert any(d == "negative" for d, _ in caught["skip_relu_in"])
    assert any(d == "cancel" for d, _ in caught["res_fp32_size"])
    assert any(h == "sentinel" for _, h in caught["store_past_row"])


def test_a_max_norm_bound_does_not_see_a_small_element_off_by_a_step():
    """what the elementwise bound adds: one bf16 step on one small element of a `cancel` case passes the 6e-3 whole-tensor bound"""
    case = ("u1.c2", "bf16", (2, 9, 9), "cancel")
    out = CR.emulate_conv(*case, "8x8")
    ref = CR.conv_reference(*case)[0].reshape(-1)
    i = int(torch.where(ref.abs() <= 0.06, ref.abs(), torch.zeros_like(ref)).argmax())          # in 2^-5 .. 2^-4: a step is 2^-12
    v = out.body[i].float()
    assert 2.0 ** -5 <= abs(float(v)) < 2.0 ** -4
    out.body[i] = (v + 2 * 2.0 ** -12).to(BF)                                                   # two steps
    fails, ratio = CR.judge_conv(*case, out)
    assert len(fails) == 1 and fails[0].startswith("elementwise") and ratio > 1.0


def test_form_table_check_notices_a_missing_form():
    rec = {CR.form_key(1, 1, 0, 128, 256, 0, 0, 0, 0, 0), CR.form_key(1, 1, 1, 256, 256, 0, 0, 4096, 4096, 4096)}
    assert CR.unlisted(rec) == []
    assert len(CR.unlisted(rec, [f for f in CR.MODEL_FORMS if f.name != "u1.c2"])) == 1
    assert len(CR.unlisted({CR.form_key(1, 1, 1, 256, 256, 1, 0, 4096, 4096, 4096)})) == 1         # "rcu2" with an input ReLU: not a model form
    assert len(CR.table_keys()) == len(CR.MODEL_FORMS) == 9


# ----------------------------------------------------------------------------- bilinear x2
UP_SHAPES = [(2, 1, 1, 2, 2), (1, 1, 5, 2, 10), (2, 4, 3, 7, 5), (1, 9, 6, 17, 11), (1, 7, 7, 14, 14), (1, 3, 5, 6, 10)]


def up_data(B, h, w, C, dtype, seed=0):
    """the census builder's residual data: (rnd * 2 + 0.3) in the map dtype"""
    g = torch.Generator().manual_seed(1000 + seed)
    return ((torch.rand(B, h, w, C, generator=g) * 2 - 1) * 2 + 0.3).to(dtype)


@pytest.mark.parametrize("B,h,w,OH,OW", UP_SHAPES)
def test_upsample_emulation_stays_inside_the_fp32_bound(B, h, w, OH, OW):
    for dt in (F32, BF):
        r = CR.upsample_data(B, h, w, 256, dt, seed=h * w)
        emu = CR.emulate_upsample(r, OH, OW)
        fails, ratio = CR.judge_upsample(emu, r, OH, OW)
        assert not fails and ratio <= 1.0
        fb, share = CR.judge_upsample(emu.to(BF), r, OH, OW)
        print("upsample2x emulation %s (%d,%d,%d)->%dx%d: %.3f of the fp32 bound; bf16 two-candidate share %.4f" % (dt, B, h, w, OH, OW, ratio, share))
        assert not fb and share <= 0.01
    ref = F.interpolate(r.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)[:, :, :OH, :OW].permute(0, 2, 3, 1)
    assert float((emu - ref).abs().max()) <= 4e-6 * float(ref.abs().max())


def test_upsample_bound_is_tight_enough_to_matter():
    """a tap taken from the wrong column, or a ratio of in/out instead of (in-1)/(out-1), leaves the bound"""
    r = CR.upsample_data(1, 9, 6, 16, F32, seed=5)
    good = CR.emulate_upsample(r, 17, 11)
    assert CR.judge_upsample(good, r, 17, 11)[0] == []
    assert CR.judge_upsample(good.roll(1, 2), r, 17, 11)[0] != []
    half = F.interpolate(r.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)[:, :, :17, :11].permute(0, 2, 3, 1)
    assert CR.judge_upsample(half, r, 17, 11)[0] != []
    one = good.clone()
    one[0, 8, 5, 3] += 4e-6 * float(one[0, 8, 5, 3].abs()) + 1e-6                     # a few fp32 steps on one element
    assert CR.judge_upsample(one, r, 17, 11)[0] != []


@pytest.mark.parametrize("B,h,w", [(1, 7, 7), (1, 14, 14), (9, 7, 7), (1, 16, 16)])
def test_res2_up_rounding_finding(B, h, w):
    """the census's five res2_up rows: the kernel interpolates the half-resolution residual in fp32 and rounds to bf16, the reference
    interpolated in float64 and rounded -- a small share of elements lands on the other bf16 neighbour, a whole bf16 step of the residual"""
    r = up_data(B, h, w, 256, BF)
    k = CR.emulate_upsample(r, 2 * h, 2 * w).to(BF).float()
    e = R.upsample2x(r.double(), 2 * h, 2 * w).float().to(BF).float()
    diff = k != e
    n = int(diff.sum())
    print("res2_up (%d, %d, %d): %d elements, %d on the other bf16 neighbour, largest difference %.4f" % (B, h, w, k.numel(), n, float((k - e).abs().max())))
    assert 0 < n < 0.005 * k.numel()
    # one bf16 step of the residual: the two roundings of an interval of the fp32 bound's width -- neighbours, except where the taps
    # cancel to a value far below their own step
    ref, bound = R.upsample2x(r.double(), 2 * h, 2 * w), CR.upsample_bound(r, 2 * h, 2 * w)
    step = 2 * CR.half_bf16_step(torch.maximum(k.abs(), e.abs()).double())
    assert bool(((k - e).abs().double()[diff] <= (2 * bound + step)[diff]).all())
    nb = (CR.bf16_ord(k) - CR.bf16_ord(e)).abs()[diff] == 1
    assert float(nb.float().mean()) > 0.9 and bool((ref.abs()[diff][~nb] < 2.0 ** -9).all())
    # every flip is a two-candidate element of the rule the census now applies, and those stay under 1 %
    lo, hi, two = CR.bf16_candidates(ref, bound)
    print("    two-candidate share %.4f" % float(two.float().mean()))
    assert bool(two[diff].all()) and float(two.float().mean()) <= 0.01
    assert bool(((k >= lo.float()) & (k <= hi.float())).all())


# ----------------------------------------------------------------------------- head_final
def test_head_post_bound_holds_for_an_fp32_evaluation():
    g = torch.Generator().manual_seed(3)
    raw = torch.cat([(torch.rand(4000, 4, generator=g) * 2 - 1) * s for s in (1e-6, 1.0, 11.5)])
    raw[:, 3] = torch.linspace(-30, 30, raw.shape[0])
    raw[0, :3] = 0
    pts, conf, bp, bc = CR.head_post_reference(raw)
    x = raw[:, :3]
    d = (x * x).sum(1, keepdim=True).sqrt()
    p32 = x * (torch.expm1(d) / d.clamp_min(1e-8))
    c32 = 1 + torch.exp(raw[:, 3])
    rp = float(((p32.double() - pts).abs() / (bp * pts.abs()).clamp_min(1e-300)).nan_to_num(0).max())
    rc = float(((c32.double() - conf).abs() / (bc * conf)).max())
    print("head_final post-processing in fp32 torch: pts uses %.3f, conf %.3f of the bound; d up to %.1f" % (rp, rc, float(d.max())))
    assert rp <= 1.0 and rc <= 1.0 and float(p32[0].abs().max()) == 0.0 and float(d.max()) > 18
