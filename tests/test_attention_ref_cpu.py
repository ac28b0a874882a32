"""The proof that tests/test_attention_forms_gpu.py can fail, without a GPU: the float64 reference of tests/attention_ref.py against
torch's own attention, the design of the peaked / tie / shift inputs, a torch-fp32 restatement of attention_packed_kernel's
arithmetic that must stay inside the derived elementwise bound on every packed case of the matrix, and eight mutants of that
restatement that must each leave it.

Measured here (worst |emulation - ref| / tolerance over the packed cases of the matrix, pad fills and both output dtypes
included): flat 0.50, peaked 0.00, tie 0.47, shift 0.34 -- correct arithmetic uses half of the derived bound.

Which case catches which mutant (test_every_mutant_is_caught prints it: first catching case per distribution and its ratio to the
tolerance, zero-filled pads unless said):
  l_not_rescaled      b six_tiles: flat 14, shift 10, peaked 211, tie 207
  o_not_rescaled      b six_tiles: flat 32, shift 20, peaked 1.3e5, tie 7.0e3
  merge_own_max       b ragged:    flat 79, shift 38, peaked 3.5e5, tie 2.6e3
  mask_dropped        b ragged:    flat 66, no other distribution with zero pads; with stale pads every distribution, >= 2e4
  mask_off_by_one     b ragged:    flat 2.0, no other distribution with zero pads; with stale pads every distribution, >= 2e4
  k_col0_ignored      b ragged:    flat 673, shift 428, peaked 4.3e5, tie 6.6e3
  group_rows_formula  db ragged:   every distribution (the defined rows keep their NaN pre-fill)
  head_mod            b ragged:    flat 219, shift 116, peaked 1.1e5, tie 3.8e3
No mutant is caught ONLY by peaked, tie or shift: with q = 2 U(-1, 1) the flat scores already spread enough between tiles that a
missing rescale moves a flat row by 10 to 80 times the elementwise tolerance (and by 0.2 to 0.5 of the whole tensor, so the old
whole-tensor check on a five-tile shape would have seen it too).  What the new inputs add is margin -- three to four orders of
magnitude on peaked rows -- and the stale pad fill: an off-by-one key mask sits at twice the tolerance with zero pads (1.3e-2 of
the whole tensor against the old bound of 1e-2) and at 3e4 times the tolerance with stale pads, and is invisible with zero pads on
every distribution but flat.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import attention_ref as AR
from gemm_desc_ref import BF, frag_unpack, pv_offsets

F32ROW = (torch.float32, False)


@functools.lru_cache(maxsize=None)
def case(form, shape, dist):
    return AR.Case(form, "bf16" if form in AR.PACKED_FORMS else "fp32", shape, dist)


def packed_cases():
    return [(f, s, d) for f, s in AR.matrix() if f in AR.PACKED_FORMS for d in AR.DISTS]


def fills_of(shape):
    return AR.FILLS if shape in AR.STALE_SHAPES else ("zero",)


# ----------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("dist", AR.DISTS)
@pytest.mark.parametrize("form,shape", [("f", "six_tiles"), ("c", "ragged"), ("b", "g"), ("e", "e_small")])
def test_reference_is_torchs_attention(form, shape, dist):
    c = case(form, shape, dist)
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (c.q64, c.k, c.v))
    want = F.scaled_dot_product_attention(q, k, v, scale=c.scale).permute(0, 2, 1, 3)
    assert float((c.ref - want).abs().max()) < 1e-12
    assert float((c.A - c.ref.abs()).min()) > -1e-12              # A = softmax @ |v| bounds |ref|
    assert bool((c.bound > 0).all()) and bool(torch.isfinite(c.bound).all())


@pytest.mark.parametrize("form,shape", [("b", "ragged"), ("c", "qb2"), ("db", "six_tiles"), ("e", "e_small")])
@pytest.mark.parametrize("fill", ["zero", "stale"])
def test_packers_round_trip(form, shape, fill):
    """what the layout wrote in fragment / PV order reads back through frag_unpack / pv_offsets as the dense operands"""
    c = case(form, shape, "flat")
    lay = c.layout("cpu", F32ROW, fill)
    Bt, C = c.Bt, c.C
    kbuf = lay.bufs["qk"] if "qk" in lay.bufs else lay.bufs["k"]
    kd = frag_unpack(kbuf.t, Bt * lay.npad_k, lay.k_cols, BF).view(Bt, lay.npad_k, lay.k_cols)
    assert torch.equal(kd[:, :c.Nk, lay.k_col0:lay.k_col0 + C].float(), c.k.reshape(Bt, c.Nk, C))
    if form != "e":
        qbuf = lay.bufs["qk"] if "qk" in lay.bufs else lay.bufs["q"]
        qd = frag_unpack(qbuf.t, Bt * lay.npad_q, lay.q_cols, BF).view(Bt, lay.npad_q, lay.q_cols)
        assert torch.equal(qd[:, :c.Nq, lay.q_col0:lay.q_col0 + C].float(), c.q.reshape(Bt, c.Nq, C))
        pads = qd[:, c.Nq:, lay.q_col0:lay.q_col0 + C].float()
        if pads.numel():
            assert bool((pads == 0).all()) == (fill == "zero")
    vd = lay.bufs["vtp"].t[pv_offsets(Bt, c.heads, lay.npad_k, lay.npad_k).reshape(-1)].float().view(Bt, lay.npad_k, c.heads, 64)
    assert torch.equal(vd[:, :c.Nk], c.v)
    assert bool((vd[:, c.Nk:] == 0).all()) == (fill == "zero")
    assert lay.untouched()
    assert lay.npad_q % 16 == 0 and lay.npad_k % 64 == 0 and lay.ldo > C
    if shape == "qb2" and form == "c":
        assert lay.npad_q == 528
    if shape == AR.WIDE_SHAPE:
        assert lay.npad_k == (c.Nk + 63) // 64 * 64 + 64


# ----------------------------------------------------------------------------- the design of the inputs
@pytest.mark.parametrize("form,shape", AR.matrix())
def test_peaked_rows_sit_where_the_case_says(form, shape):
    c = case(form, shape, "peaked")
    top, arg = c.p.max(-1)                                       # [Bt, heads, Nq]
    assert float(top.min()) > 0.99
    want = torch.tensor(c.J)[torch.arange(c.Nq) % 8]
    assert bool((arg == want[None, None]).all())
    if c.Nk == 323:
        # key, tile and wave: the eight classes reach both ends of wave 0's first tile, wave 1, wave 3's last key, wave 0's SECOND tile
        # (256: the online rescale), the ragged tile's first and last key and a mid-tile key
        assert c.J == [0, 63, 64, 255, 256, 322, 320, 165]
        assert [j // 64 & 3 for j in c.J] == [0, 0, 1, 3, 0, 1, 1, 2] and [j // 64 for j in c.J][4] == 4
    if c.Nk == 65:
        assert c.J[:3] == [0, 63, 64]                            # the ragged tile holds one key, and it is a peak


@pytest.mark.parametrize("form,shape", [(f, s) for f, s in AR.matrix() if s in ("six_tiles", "ten_tiles", "qb2")])
def test_tie_rows_split_between_two_tiles(form, shape):
    c = case(form, shape, "tie")
    top, arg = c.p.topk(2, -1)
    assert float((top - 0.5).abs().max()) < 0.05
    assert bool((arg[..., 0] // 64 != arg[..., 1] // 64).all())
    same_wave = (arg[..., 0] // 64 & 3) == (arg[..., 1] // 64 & 3)
    assert bool(same_wave.any()) and not bool(same_wave.all())      # both meeting places: a wave's online rescale, and the merge


@pytest.mark.parametrize("form,shape", AR.matrix())
def test_shift_moves_every_score_and_not_the_result(form, shape):
    c = case(form, shape, "shift")
    assert float(c.scores.min()) > 88.0                          # exp overflows fp32 there: only the maximum subtraction saves it
    d = float(AR.DELTA) ** 2 * c.scale
    p0 = torch.softmax(c.scores - d, -1)
    assert float((p0 - c.p).abs().max()) < 1e-12


# ----------------------------------------------------------------------------- the kernel's arithmetic stays inside the bound
WORST = {}


@pytest.mark.parametrize("form,shape,dist", packed_cases())
def test_emulation_is_inside_the_bound(form, shape, dist):
    c = case(form, shape, dist)
    base = {}
    for fill in fills_of(shape):
        for kind in (F32ROW, (BF, True)):
            lay = c.layout("cpu", kind, fill)
            out = AR.emulate(lay)
            got = AR.read_payload(lay, out)
            r = AR.ratio(c, got, kind[0])
            WORST[dist] = max(WORST.get(dist, 0.0), r)
            print("%-2s %-9s %-6s %-6s %s: ratio %.3f" % (form, shape, dist, fill, "bf16p" if kind[1] else "f32", r))
            assert r <= 1.0, (form, shape, dist, fill, kind, r)
            # outside the defined region nothing was written, and the pads do not reach the result
            mask = torch.ones(out.numel(), dtype=torch.bool)
            mask[lay.out_index().reshape(-1)] = False
            assert bool(torch.isnan(out[mask].float()).all())
            if fill == "zero":
                base[kind] = out
            else:
                assert torch.equal(out.view(torch.int16 if kind[0] == BF else torch.int32), base[kind].view(torch.int16 if kind[0] == BF else torch.int32))
    print("worst so far", {k: round(v, 3) for k, v in WORST.items()})


# ----------------------------------------------------------------------------- and wrong arithmetic does not
def _old_check(c, got):
    """what test_attention_packed asserts: the whole-tensor max-norm error against 1e-2"""
    return float((got - c.ref).abs().max() / c.ref.abs().max())


# mutants that the OLD style of check (flat inputs, zero pads, whole-tensor 1e-2) misses at every shape of the matrix
OLD_CHECK_MISSES = set()


@pytest.mark.parametrize("mut", AR.MUTANTS)
def test_every_mutant_is_caught(mut):
    caught, caught_stale, old = {}, {}, None
    for form, shape, dist in packed_cases():
        if mut == "k_col0_ignored" and form not in ("b", "db"):
            continue
        if mut == "group_rows_formula" and not case(form, shape, dist).grouped:
            continue
        if mut in ("mask_dropped", "mask_off_by_one") and AR.SHAPES[shape][3] % 64 == 0:
            continue
        c = case(form, shape, dist)
        for fill in fills_of(shape)[:2]:
            lay = c.layout("cpu", F32ROW, fill)
            got = AR.read_payload(lay, AR.emulate(lay, mut))
            r = AR.ratio(c, got, torch.float32)
            if r > 1.0:
                (caught if fill == "zero" else caught_stale).setdefault(dist, (form, shape, round(r, 1)))
            if dist == "flat" and fill == "zero" and not _old_check(c, got) < 1e-2 and old is None:
                old = (form, shape, _old_check(c, got))
    print("MUTANT", mut, "| zero pads:", caught, "| stale pads:", caught_stale, "| old check (flat, whole tensor 1e-2):", old)
    assert caught or caught_stale, mut
    assert (old is None) == (mut in OLD_CHECK_MISSES), (mut, old)
    if mut in ("mask_dropped", "mask_off_by_one"):
        # the stale pad fill is what makes a wrong key mask unmissable: every distribution, four orders of magnitude over the tolerance
        assert set(caught) == {"flat"} and set(caught_stale) == set(AR.DISTS) and min(v[2] for v in caught_stale.values()) > 1e4
    else:
        assert set(caught) == set(AR.DISTS)
        if mut != "group_rows_formula":
            assert caught["peaked"][2] > 10 * caught["flat"][2]


def test_form_keys_cover_the_engines_launches():
    """the static half of test_forms_are_the_models: the keys of the launches engine.py is known to make are in the matrix"""
    keys = AR.covered_keys()
    for entry, shared, col0, grouped, prec in [("attention", True, True, False, "fp32"), ("attention", False, False, False, "fp32"),
                                               ("attention", True, True, False, "f32x3"), ("attention", True, True, False, "f16x3"),
                                               ("attention_packed", True, True, False, "bf16"), ("attention_packed", False, False, False, "bf16"),
                                               ("attention_packed", True, True, True, "bf16"), ("attention_packed", False, False, True, "bf16"),
                                               ("attention_packed_qproj", False, False, True, "bf16")]:
        assert AR.form_key(entry, shared, col0, grouped, BF if prec == "bf16" else torch.float32, True, prec) in keys
