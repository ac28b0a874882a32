"""Every launch form in which the engine runs the attention kernels (tests/attention_ref.py: forms a-f and the value encoder's
48-wide heads), in every precision and output kind the form accepts, on flat, peaked, tied and shifted softmax rows, against
float64 -- with guard bands around every buffer, NaN-filled outputs, non-minimal leading dimensions, and pads that hold zeros,
stale finite data or NaN.  Per case:
  1. no guard band, input or undefined output element changed, no NaN in the defined output;
  2. |got - ref| <= bound * A per element (attention_ref.bound: derived), plus half a bf16 step for bf16 output;
  3. the whole-tensor max-norm bounds of the older op tests;
  4. stale and NaN pads give the bits of zero pads.
test_ratio_table prints the worst |got - ref| / tolerance per (form, precision, distribution, output dtype) of the run; the figures measured on an
MI355X are in profiles/attention_forms.txt.
"""
import os

import pytest
import torch

import attention_ref as AR
from conftest import rel_err
from gemm_desc_ref import BF

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATIOS = {}          # (form, precision, distribution, output dtype) -> [worst elementwise ratio, worst whole-tensor error / its bound, launches]
MODES = {0: "fp32", 1: "f32x3", 4: "f16x3"}


def _ops():
    from spann3r_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def fills_of(shape):
    return AR.FILLS if shape in AR.STALE_SHAPES else ("zero",)


@pytest.mark.parametrize("dist", AR.DISTS)
@pytest.mark.parametrize("form,shape", AR.matrix())
def test_form_against_float64(form, shape, dist):
    ops = _ops()
    for prec in AR.PRECISIONS[form]:
        c = AR.Case(form, prec, shape, dist)
        for kind in AR.KINDS:
            rec = RATIOS.setdefault((form, prec, dist, "bf16" if kind[0] == BF else "fp32"), [0.0, 0.0, 0])
            base = None
            for fill in fills_of(shape):
                tag = (form, shape, dist, prec, str(kind[0]), "packed" if kind[1] else "rows", fill)
                lay = c.layout(DEV, kind, fill)
                lay.launch(ops)
                torch.cuda.synchronize()
                assert lay.untouched(), tag                                                  # 1
                got = lay.output()
                assert not bool(torch.isnan(got).any()), tag
                r = AR.ratio(c, got, kind[0])
                whole = rel_err(got, c.ref) / AR.whole_bound(c, kind[0])
                rec[0], rec[1], rec[2] = max(rec[0], r), max(rec[1], whole), rec[2] + 1
                print("%-2s %-9s %-6s %-5s %-8s %-6s %-6s ratio %.3f whole %.3f" % (tag + (r, whole)))
                assert r <= 1.0, (tag, r)                                                    # 2
                assert whole < 1.0, (tag, whole)                                             # 3
                raw = lay.raw_output()
                if fill == "zero":
                    base = raw
                else:
                    assert torch.equal(_bits(raw), _bits(base)), tag                         # 4


def test_packed_entry_points_reject_a_scale_that_is_not_positive():
    """attention_packed_kernel takes the tile maximum of the RAW scores; the row kernel scales first and takes any scale"""
    ops = _ops()
    for form in ("c", "e"):
        lay = AR.Case(form, "bf16", "ragged" if form == "c" else "e_small", "flat").layout(DEV)
        for bad in (0.0, -0.125):
            with pytest.raises(RuntimeError, match="scale"):
                lay.launch(ops, scale=bad)
        torch.cuda.synchronize()
        assert bool(torch.isnan(lay.raw_output()).all())
    c = AR.Case("f", "fp32", "ragged", "flat")
    lay = c.layout(DEV)
    lay.launch(ops, scale=-c.scale)
    got = lay.output()
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(-c.scores, -1), c.v.double())
    assert rel_err(got, ref) < 2e-5


def test_ratio_table():
    """the measured worst ratios of this run (runs after the matrix; writes them where SP3_ATTN_FORMS_TABLE points, if anywhere)"""
    if not RATIOS:
        print("the matrix did not run in this process: nothing to report")
        return
    lines = ["worst |got - ref| / (bound * A [+ half a bf16 step]) and worst whole-tensor error / its bound, over shapes, output kinds and pad fills",
             "(with bf16 output the elementwise figure is mostly the output rounding itself: up to half a step out of half a step plus the bound)",
             "%-5s %-6s %-7s %-5s %9s %9s %9s" % ("form", "prec", "dist", "out", "elementw.", "whole", "launches")]
    for (form, prec, dist, odt), (r, w, n) in sorted(RATIOS.items()):
        lines.append("%-5s %-6s %-7s %-5s %9.4f %9.4f %9d" % (form, prec, dist, odt, r, w, n))
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.environ.get("SP3_ATTN_FORMS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write(text)
    assert max(v[0] for v in RATIOS.values()) <= 1.0


# ----------------------------------------------------------------------------- the engine's launches are the matrix's
def _tiny(precision):
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd.weights import synth_state_dict
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(synth_state_dict(0, TINY), strict=True)
    return m.to(DEV).eval().set_precision(precision)


def _frames(n, h, w, seed=1000):
    from spann3r_amd.weights import synth_frames
    return [{"img": f["img"].to(DEV)} for f in synth_frames(n, h, w, seed=seed)]


def test_forms_are_the_models(monkeypatch):
    """One TINY forward per precision and decoder schedule with the three attention entry points wrapped: every launch, reduced to
    (entry point, q and k in one matrix, k_col0 != 0, grouped, output dtype, output layout, precision), is a form the matrix above
    holds to float64.  A launch form added to the engine fails here with its key."""
    ops = _ops()
    seen = {}

    def prec_of(t):
        return "bf16" if t.dtype == BF else MODES.get(ops.get_product_mode(), "mode%d" % ops.get_product_mode())

    real = {n: getattr(ops, n) for n in ("attention", "attention_packed", "attention_packed_qproj")}

    def attention(q, sq, ldq, k, sk, ldk, vt, vt_ld, out, ldo, **kw):
        d = k.data_ptr() - q.data_ptr()
        shared = 0 <= d < ldq * q.element_size()
        key = AR.form_key("attention", shared, d != 0 and shared, 0, out.dtype, isinstance(out, ops.PackedAct), prec_of(vt))
        seen[key] = seen.get(key, 0) + 1
        return real["attention"](q, sq, ldq, k, sk, ldk, vt, vt_ld, out, ldo, **kw)

    def attention_packed(qp, q_cols, q_col0, npad_q, kp, k_cols, k_col0, npad_k, vtp, out, ldo, **kw):
        key = AR.form_key("attention_packed", qp.data_ptr() == kp.data_ptr(), k_col0, kw.get("o_group", 0), out.dtype,
                          isinstance(out, ops.PackedAct), prec_of(vtp))
        seen[key] = seen.get(key, 0) + 1
        return real["attention_packed"](qp, q_cols, q_col0, npad_q, kp, k_cols, k_col0, npad_k, vtp, out, ldo, **kw)

    def attention_packed_qproj(xq, stats, Wq, ln_s, bias, pos, cos, sin, kp, k_cols, k_col0, npad_k, vtp, out, ldo, **kw):
        key = AR.form_key("attention_packed_qproj", False, k_col0, kw.get("o_group", 0), out.dtype, isinstance(out, ops.PackedAct), prec_of(vtp))
        seen[key] = seen.get(key, 0) + 1
        return real["attention_packed_qproj"](xq, stats, Wq, ln_s, bias, pos, cos, sin, kp, k_cols, k_col0, npad_k, vtp, out, ldo, **kw)

    for n, f in (("attention", attention), ("attention_packed", attention_packed), ("attention_packed_qproj", attention_packed_qproj)):
        monkeypatch.setattr(ops, n, f)
    entries = set()
    for precision, grouped in (("bf16", True), ("bf16", False), ("fp32", True)):
        m = _tiny(precision)
        m.grouped_decoder = grouped
        m.use_graphs = False
        before = dict(seen)
        m(_frames(3, 64, 80))
        torch.cuda.synchronize()
        new = {k: v - before.get(k, 0) for k, v in seen.items() if v > before.get(k, 0)}
        print(precision, "grouped" if grouped else "two streams", "lean" if ops.LEAN else "general", sorted(new.items()))
        assert new
        entries |= {k[0] for k in new}
    unknown = sorted(set(seen) - AR.covered_keys())
    assert not unknown, unknown
    assert {"attention", "attention_packed"} <= entries and (not ops.LEAN or "attention_packed_qproj" in entries)
    assert any(k[3] for k in seen) and any(k[0] == "attention_packed" and k[1] and k[2] for k in seen)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_geometries_sharing_a_workspace(precision):
    """224 x 224 frames (196 tokens) and then 240 x 208 frames (195 tokens) through ONE model: same batch, same npad = 256, so the
    q/k/V^T workspaces of the second geometry are the first one's, with its row / column 195 still in what is now a pad.  Every
    output of the second geometry is bit-equal to a freshly built model's -- first call (capture or eager, as the defaults choose) and
    second call (replay)."""
    first, second = _frames(2, 224, 224), _frames(2, 240, 208, seed=2000)

    def run(m, frames):
        out = m(frames)[0]
        torch.cuda.synchronize()
        return [{k: v.clone() for k, v in p.items()} for p in out]

    fresh = _tiny(precision)
    want = [run(fresh, second) for _ in range(2)]
    del fresh
    m = _tiny(precision)
    run(m, first)
    run(m, first)
    got = [run(m, second) for _ in range(2)]
    for call, (g, w) in enumerate(zip(got, want)):
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.keys() == b.keys()
            for k in a:
                assert not bool(torch.isnan(a[k]).any())
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (precision, "call %d frame %d %s" % (call, j, k))
