"""The DPT head's helper kernels (csrc/dpt.hip) between guard bands, element by element (tests/conv_ref.py):
  sp3_upsample2x / sp3_upsample2x_bf16 -- the fp32 kernel, the 16-byte bf16 kernel (C % 8 == 0) and the generic bf16 kernel against
      float64 with the exact ratio, inside the fp32 bound derived from the kernel's index arithmetic; a bf16 element must be the bf16
      rounding of SOME value within that bound (two candidates where the interval holds a rounding boundary: at most 1 % of a case);
      the bf16 kernels bit-equal to the fp32 kernel's result rounded;
  sp3_head_final / sp3_head_final_bf16 -- raw against float64 on the stored features (2e-5 of the pixel's largest sum of magnitudes),
      pts and conf against float64 on the kernel's OWN raw (a few fp32 steps: conv_ref.head_post_reference), with d = |xyz| at exactly
      0, near 1e-6, 1 and 20 and logits from -30 to 30; raw = None gives the same bits; a misaligned raw takes the generic kernel;
  sp3_im2col_patch -- every (out_bf16, out_packed) combination, NCHW and NHWC strides, exact."""
import pytest
import torch

import conv_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def _L():
    from spann3r_amd import lib as L
    return L


# ----------------------------------------------------------------------------- bilinear x2
UP_SHAPES = [(2, 1, 1, 2, 2), (1, 1, 5, 2, 10), (2, 4, 3, 7, 5), (1, 9, 6, 17, 11), (1, 7, 7, 14, 14), (1, 3, 5, 6, 10)]


def run_upsample(r, OH, OW):
    L = _L()
    B, h, w, C = r.shape
    src = CR.Buf(r.dtype, r.numel(), DEV).put(r)
    out = CR.Buf(r.dtype, B * OH * OW * C, DEV, out=True)
    fn = L.load().sp3_upsample2x_bf16 if r.dtype == BF else L.load().sp3_upsample2x
    L.check(fn(src.ptr(), out.ptr(), B, h, w, C, OH, OW, L.stream_ptr()), "sp3_upsample2x")
    torch.cuda.synchronize()
    assert src.guards_intact() and out.guards_intact()
    return out.body.reshape(B, OH, OW, C).cpu()


@pytest.mark.parametrize("C", [256, 128, 12])
@pytest.mark.parametrize("B,h,w,OH,OW", UP_SHAPES)
def test_upsample2x(B, h, w, OH, OW, C):
    """C = 256 / 128: the 16-byte bf16 kernel ((1, 3, 5) -> 6 x 10 with C = 256: 320 threads per row, a ragged second workgroup);
    C = 12: the generic one"""
    rb = CR.upsample_data(B, h, w, C, BF, seed=h * w + C)
    got_b = run_upsample(rb, OH, OW)
    got_f = run_upsample(rb.float(), OH, OW)                     # the fp32 kernel on the same values
    fails, share = CR.judge_upsample(got_b, rb, OH, OW)
    f32f, ratio = CR.judge_upsample(got_f, rb, OH, OW)
    rf = CR.upsample_data(B, h, w, C, F32, seed=h * w + C)
    f32g, ratio2 = CR.judge_upsample(run_upsample(rf, OH, OW), rf, OH, OW)
    print("upsample2x (%d,%d,%d,%d)->%dx%d: fp32 kernel uses %.3f / %.3f of the bound; bf16 two-candidate share %.4f" % (B, h, w, C, OH, OW, ratio, ratio2, share))
    assert not fails and not f32f and not f32g, (fails, f32f, f32g)
    # one arithmetic for all three kernels (common.h up2x_taps / up2x_mix): the bf16 kernels are the fp32 kernel's result rounded, and
    # the fp32 kernel is conv_ref.emulate_upsample bit for bit.  (With the fma contraction left to the compiler the kernels differed in
    # the last fp32 bit here and there, and (1, 7, 7) -> 14 x 14 with C = 128 has an element where that crosses a bf16 boundary.)
    assert torch.equal(got_b.view(torch.int16), got_f.to(BF).view(torch.int16))
    assert torch.equal(got_f.view(torch.int32), CR.emulate_upsample(rb, OH, OW).view(torch.int32))


# ----------------------------------------------------------------------------- head_final
PIXELS = [1, 15, 16, 63, 64, 65, 1003]
SCALES = (1e-6, 2.0, 45.0, 0.25)


def head_data(pix, C, dtype, zero=False):
    """post-ReLU features; pixel p is scaled by SCALES[p % 4], so d = |xyz| is near 1e-6, 1 and 20; the last channel carries t in [0, 1]
    and only the fourth filter reads it, with weight 60 and bias -30: logits from -30 to 30"""
    g = torch.Generator().manual_seed(31 * pix + C)
    f = torch.rand(pix, C, generator=g).mul(2).sub(1).clamp_min(0)
    f *= torch.tensor(SCALES)[torch.arange(pix) % 4][:, None]
    f[:, C - 1] = torch.linspace(0, 1, pix) if pix > 1 else 0.5
    w = (torch.rand(4, C, generator=g) * 2 - 1) * 0.1
    w[:, C - 1] = 0
    w[3] = 0
    w[3, C - 1] = 60.0
    b = torch.tensor([0.0, 0.0, 0.0, -30.0])
    if zero:
        w, b = torch.zeros_like(w), torch.zeros_like(b)
    return f.to(dtype), w, b


def run_head(f, w, b, want_raw=True, raw_off=0):
    L = _L()
    pix, C = f.shape
    bufs = {"feat": CR.Buf(f.dtype, f.numel(), DEV).put(f), "w": CR.Buf(F32, w.numel(), DEV).put(w), "b": CR.Buf(F32, 4, DEV).put(b),
            "pts": CR.Buf(F32, pix * 3, DEV, out=True), "conf": CR.Buf(F32, pix, DEV, out=True),
            "raw": CR.Buf(F32, pix * 4 + 8, DEV, out=True)}
    fn = L.load().sp3_head_final_bf16 if f.dtype == BF else L.load().sp3_head_final
    L.check(fn(bufs["feat"].ptr(), bufs["w"].ptr(), bufs["b"].ptr(), pix, C, bufs["pts"].ptr(), bufs["conf"].ptr(),
               bufs["raw"].ptr(raw_off) if want_raw else 0, L.stream_ptr()), "sp3_head_final")
    torch.cuda.synchronize()
    assert CR.guard_faults(bufs) == []
    raw = bufs["raw"].body.cpu()
    rest = torch.cat([raw[:raw_off], raw[raw_off + 4 * pix:]]) if want_raw else raw
    assert bool(torch.isnan(rest).all())                         # nothing stored outside the pixels' own floats
    return bufs["pts"].body.cpu().view(pix, 3), bufs["conf"].body.cpu(), raw[raw_off:raw_off + 4 * pix].view(pix, 4)


def check_head(f, w, b, pts, conf, raw, tag):
    assert not bool(torch.isnan(pts).any() or torch.isnan(conf).any() or torch.isnan(raw).any()), tag
    ref, S = CR.head_raw_reference(f, w, b)
    bound = 2e-5 * S.amax(1, keepdim=True) + CR.U24 * ref.abs()
    r_raw = float(((raw.double() - ref).abs() / bound.clamp_min(1e-300)).max()) if float(S.max()) > 0 else float((raw != 0).any())
    p_ref, c_ref, bp, bc = CR.head_post_reference(raw)
    assert bool((pts[p_ref == 0] == 0).all()), tag
    r_pts = float(((pts.double() - p_ref).abs() / (bp * p_ref.abs()).clamp_min(1e-300))[p_ref != 0].max()) if bool((p_ref != 0).any()) else 0.0
    r_conf = float(((conf.double() - c_ref).abs() / (bc * c_ref)).max())
    print("head_final %-28s raw uses %.3f, pts %.3f, conf %.3f of their bounds" % (tag, r_raw, r_pts, r_conf))
    assert r_raw <= 1.0 and r_pts <= 1.0 and r_conf <= 1.0, (tag, r_raw, r_pts, r_conf)


@pytest.mark.parametrize("pix", PIXELS)
@pytest.mark.parametrize("kind", ["bf16-128", "bf16-64", "bf16-256", "fp32-128"])
def test_head_final(kind, pix):
    dt, C = (BF if kind.startswith("bf16") else F32), int(kind.split("-")[1])
    f, w, b = head_data(pix, C, dt)
    pts, conf, raw = run_head(f, w, b)
    check_head(f, w, b, pts, conf, raw, "%s %d px" % (kind, pix))
    d = raw[:, :3].double().norm(dim=1)
    if pix >= 15:
        assert float(d.min()) < 1e-5 and float(d.max()) > 18 and bool(((d > 0.3) & (d < 3)).any())
        assert float(raw[:, 3].min()) < -29 and float(raw[:, 3].max()) > 29
    p2, c2, _ = run_head(f, w, b, want_raw=False)
    assert torch.equal(p2.view(torch.int32), pts.view(torch.int32)) and torch.equal(c2.view(torch.int32), conf.view(torch.int32))
    # zero weights and zero bias: d = 0 exactly -- pts 0 (not NaN: expm1(0) / max(0, 1e-8)), conf = 1 + exp(0)
    fz, wz, bz = head_data(pix, C, dt, zero=True)
    pz, cz, rz = run_head(fz, wz, bz)
    assert bool((rz == 0).all()) and bool((pz == 0).all()) and bool((cz == 2).all())
    if kind == "bf16-128":
        # raw 16 bytes further on is still aligned: the same 16-byte kernel, the same bits.  raw 4 bytes further on is not: the entry
        # point falls back to the generic kernel, whose raw agrees to the bound and whose pts / conf follow from its own raw
        p4, c4, r4 = run_head(f, w, b, raw_off=4)
        assert torch.equal(r4.view(torch.int32), raw.view(torch.int32)) and torch.equal(p4.view(torch.int32), pts.view(torch.int32))
        p1, c1, r1 = run_head(f, w, b, raw_off=1)
        check_head(f, w, b, p1, c1, r1, "%s %d px, raw misaligned" % (kind, pix))


# ----------------------------------------------------------------------------- patch im2col
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("out_bf16,out_packed", [(0, 1), (1, 1), (0, 0), (1, 0)])
def test_im2col_patch(out_bf16, out_packed, layout):
    """the engine issues the packed forms (Engine.encode_image, Engine.encode_cur_value: a PackedAct in the activation dtype, fp32 or
    bf16), from an NCHW image and from the NHWC pts3d map; the dense forms are what tools and older tests use"""
    from spann3r_amd import ops
    L = _L()
    B, C, H, W, p = 2, 3, 32, 48, 16
    g = torch.Generator().manual_seed(11)
    img = torch.rand(B, C, H, W, generator=g) * 2 - 1
    ref = CR.im2col_reference(img, p)
    M, K = ref.shape
    dt = BF if out_bf16 else F32
    if layout == "nchw":
        store, (sb, sc, sy, sx) = img, img.stride()
    else:
        store = img.permute(0, 2, 3, 1).contiguous()
        sb, sy, sx, sc = store.stride()
    src = CR.Buf(F32, store.numel(), DEV).put(store)
    shape = ops.packed_shape(M, K, dt) if out_packed else (M, K)
    n = 1
    for s in shape:
        n *= s
    out = CR.Buf(dt, n, DEV, out=True, body_fill=CR.SENT)
    L.check(L.load().sp3_im2col_patch(src.ptr(), sb, sc, sy, sx, B, C, H, W, p, out.ptr(), out_bf16, out_packed, L.stream_ptr()), "sp3_im2col_patch")
    torch.cuda.synchronize()
    assert src.guards_intact() and out.guards_intact()
    body = out.body.view(shape)
    if out_packed:
        pa = ops.PackedAct(M, K, dt, DEV, data=body)
        dense = pa.to_dense().cpu()
        full = ops.PackedAct(shape[0] * 16, K, dt, DEV, data=body).to_dense().cpu()
        assert M % 16 and bool((full[M:] == CR.SENT).all())          # the padding rows of the fragment order are not written
    else:
        dense = body.cpu()
    assert torch.equal(dense, ref.to(dt))
