"""Float64 references, elementwise bounds, guarded buffers and data designs for the DPT head's own kernels: sp3_conv3x3_tile (csrc/conv.hip),
sp3_upsample2x(_bf16), sp3_head_final(_bf16) and sp3_im2col_patch (csrc/dpt.hip).  Plain torch, importable without a GPU.

Buffers (Buf): every device buffer is the body of a larger allocation between two guard bands of GUARD elements.  Input bands hold NaN,
so a read outside the extent that reaches an output shows up there; output bodies are NaN-filled (an element the kernel never stored
shows up) and output bands hold SENT, which must come back untouched.  GUARD * element size is a multiple of 16 bytes: bodies keep the
alignment the entry points ask for.

Convolution: conv_reference() is the 3x3 / padding 1 convolution in float64 on the operands as the kernel rounds them (ReLU, then bf16,
for the map; bf16 weights) plus bias, ReLU and the residuals as stored -- nothing else rounded -- and S = conv(|x|, |w|) + |b| + |r1| +
|r2| per element.  conv_bound(): the model is ONE final rounding of an fp32-accumulated value,
    |got - ref| <= slack [+ half a bf16 step at |ref| + slack],   slack = 2e-5 * max S over the element's 32-channel group (same pixel)
2e-5 is the project's figure for fp32 accumulation on rounded operands (gemm_desc_ref.tolerance, the fp32 tolerance of
test_conv3x3_tile).  The slack comes from S and not from |ref|, so the bound stays sound where the residuals cancel the convolution.
emulate_conv() restates the summation order of both tiled kernels in fp32 on the CPU and takes mutants as switches (MUTANTS): the
tests show that every mutant leaves the bound, breaks an exact design or writes a sentinel.
"""
import collections
import functools
import math
import zlib

import torch

import gemm_desc_ref as R

BF, F32 = torch.bfloat16, torch.float32
GUARD = 256
SENT = R.SENT
U24 = 2.0 ** -24                 # half an fp32 step, relative


def bf(t):
    return t.to(BF).to(F32)


# ----------------------------------------------------------------------------- guarded buffers
class Buf:
    """numel elements of dtype between two guard bands.  out: body NaN (or body_fill), bands SENT; input: body zero, bands NaN."""

    def __init__(self, dtype, numel, device, out=False, body_fill=None):
        self.dtype, self.numel, self.out = dtype, int(numel), out
        self.band = SENT if out else math.nan
        self.t = torch.full((self.numel + 2 * GUARD,), self.band, dtype=dtype, device=device)
        self.body.fill_(body_fill if body_fill is not None else (math.nan if out else 0.0))
        assert self.ptr() % 16 == 0

    @property
    def body(self):
        return self.t[GUARD:GUARD + self.numel]

    def put(self, src):
        self.body.copy_(src.reshape(-1).to(self.t.device))
        return self

    def ptr(self, off=0):
        return self.t.data_ptr() + (GUARD + off) * self.t.element_size()

    def guards_intact(self):
        a, b = self.t[:GUARD], self.t[GUARD + self.numel:]
        if math.isnan(self.band):
            return bool(torch.isnan(a).all() and torch.isnan(b).all())
        return bool((a == self.band).all() and (b == self.band).all())


def guard_faults(bufs):
    return [n for n, b in bufs.items() if b is not None and not b.guards_intact()]


# ----------------------------------------------------------------------------- the forms of sp3_conv3x3_tile
Form = collections.namedtuple("Form", "name Cin Cout relu_in act bias nres")
ACT_NONE, ACT_RELU = 0, 2
# the launches of Engine.dpt_head that reach the LDS-tiled kernel (bf16 maps, residuals and output); test_tile_forms_are_current
# holds the model to this table
MODEL_FORMS = (
    Form("rn0", 128, 256, False, ACT_NONE, False, 0),
    Form("rn1", 192, 256, False, ACT_NONE, False, 0),
    Form("rn2", 384, 256, False, ACT_NONE, False, 0),
    Form("rn3", 768, 256, False, ACT_NONE, False, 0),
    Form("u.c1", 256, 256, True, ACT_RELU, True, 0),
    Form("u.c2", 256, 256, False, ACT_NONE, True, 1),
    Form("u1.c2", 256, 256, False, ACT_NONE, True, 2),
    Form("h0", 256, 128, False, ACT_NONE, True, 0),
    Form("h2", 128, 128, False, ACT_RELU, True, 0),
)
C64 = Form("c64", 64, 64, True, ACT_RELU, True, 0)      # not a model form: the smallest unit count (18 units, two waves end one unit early)
FORM = {f.name: f for f in MODEL_FORMS + (C64,)}
DTYPES = {"bf16": (BF, BF, BF), "fp32": (F32, F32, F32), "mixed": (F32, BF, F32)}       # map, output, residuals


def form_key(in_bf16, out_bf16, res_bf16, Cin, Cout, relu_in, act, bias, res1, res2):
    """what test_tile_forms_are_current records of a launch (no pointers, no sizes); the residual dtype only counts where one is read"""
    nres = int(bool(res1)) + int(bool(res2))
    assert not (res2 and not res1)
    return (int(in_bf16), int(out_bf16), int(res_bf16) if nres else None, Cin, Cout, bool(relu_in), act, bool(bias), nres)


def table_keys(forms=MODEL_FORMS):
    return {form_key(1, 1, 1, f.Cin, f.Cout, f.relu_in, f.act, f.bias, f.nres > 0, f.nres > 1): f.name for f in forms}


def unlisted(records, forms=MODEL_FORMS):
    keys = table_keys(forms)
    return sorted({r for r in records if r not in keys}, key=repr)


def instances(form):
    return ("8x8", "8x16", "8x16n32") if form.Cin % 128 == 0 else ("8x8",)


def designs(form):
    d = ["random", "ones"]
    if form.relu_in or form.name in ("rn1", "rn2", "rn3"):       # (the layer_rn forms too: the halo loader's slow arm and several K chunks)
        d.append("impulse")
    if form.relu_in:
        d.append("negative")
    if form.nres:
        d.append("cancel")
    return d


TILE_PX = {"8x8": 1, "8x16": 2, "8x16n32": 3}
# 3 x 3 tiles ragged by one pixel both ways, an interior tile, a batch seam; 18 tiles: a second round of the XCD map and six padding
# workgroups | exactly one wide tile, seven padding workgroups | every halo pixel outside the map
SHAPES = {"8x8": ((2, 17, 17), (1, 1, 1)), "wide": ((2, 17, 33), (1, 8, 16), (1, 1, 1))}


# ----------------------------------------------------------------------------- data designs: functions of (form, dtypes, shape, design)
ConvData = collections.namedtuple("ConvData", "x w bias r1 r2")     # x [B,H,W,Cin] map dtype; w [Cout,9,Cin] bf16; bias fp32; r* res dtype
IMPULSE_CIN = (0, 31, 32, 63, 64, 127, 128)


def _rnd(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def impulse_entries(Cin, Cout):
    """(co, tap, ci) of the single non-zero weight of every output channel: tap = co % 9 and ci walks 0, 31, 32, 63, 64, 127, 128, Cin-1
    (as far as they exist) -- 9 and the list length are coprime or the list is short, so all nine taps and all listed channels occur,
    and every output channel (0, 15, 16, 63, 64, Cout-1 among them) is tested"""
    cins = sorted({c for c in IMPULSE_CIN if c < Cin} | {Cin - 1})
    return [(co, co % 9, cins[(co // 9 + co) % len(cins)]) for co in range(Cout)]


@functools.lru_cache(maxsize=None)
def conv_data(form, dts, shape, design):
    f, (B, H, W) = FORM[form], shape
    mdt, odt, rdt = DTYPES[dts]
    gen = torch.Generator().manual_seed(zlib.crc32(repr((form, dts, shape, design)).encode()))
    x = _rnd(gen, B, H, W, f.Cin)
    w = _rnd(gen, f.Cout, 9, f.Cin) * 0.05
    bias = _rnd(gen, f.Cout) if f.bias else None
    r = [(_rnd(gen, B, H, W, f.Cout) * 2 + 0.3 * (i + 1)) for i in range(f.nres)]
    if design == "ones":
        x, w = torch.ones_like(x), torch.ones_like(w)
        bias = None if bias is None else torch.zeros_like(bias)
        r = [torch.zeros_like(t) for t in r]
    elif design == "impulse":
        wv, w = w, torch.zeros_like(w)
        for co, tap, ci in impulse_entries(f.Cin, f.Cout):
            w[co, tap, ci] = wv[co, tap, ci] + (0.02 if wv[co, tap, ci] >= 0 else -0.02)
    elif design == "negative":
        x = torch.where(torch.rand(x.shape, generator=gen) < 0.9, -x.abs(), x.abs())
        flat = x.view(-1)
        sub = 2.0 ** -133                                          # the smallest bf16 subnormal
        for k, v in enumerate((-0.0, -sub, sub, -sub, -0.0, sub)):
            flat[k::97][:max(flat.numel() // 400, 1)] = v
    x = x.to(mdt)
    w = w.to(BF)
    r = [t.to(rdt) for t in r]
    if design == "cancel":
        y = _conv64(x, w, f.relu_in)
        if bias is not None:
            y = y + bias.double()
        # the random term: outputs of about 1 % of S, yet large enough that the suite's older whole-tensor bound (relative to max |ref|)
        # still means something for fp32 outputs -- fp32 summation of S ~ 5 carries some 1e-7 S, i.e. 5e-6 of an output range of 0.1
        r = [(-y / f.nres + 0.05 * _rnd(gen, *y.shape).double()).float().to(rdt) for _ in range(f.nres)]
    return ConvData(x, w, bias, r[0] if f.nres > 0 else None, r[1] if f.nres > 1 else None)


def _conv64(x, w, relu_in, absolute=False):
    """float64 [B,H,W,Cout] of the map as the kernel rounds it (ReLU, then bf16) with the bf16 weights [Cout, 9, Cin]"""
    B, H, W, _ = x.shape
    xe = x.float().clamp_min(0) if relu_in else x.float()
    xe, we = bf(xe).double(), w.double().reshape(w.shape[0], -1)
    xe = torch.where(xe == 0, torch.zeros_like(xe), xe)             # (-0.0 -> 0.0: the same value)
    if absolute:
        xe, we = xe.abs(), we.abs()
    return (R.conv_rows(xe, H, W, 1) @ we.T).reshape(B, H, W, -1)


@functools.lru_cache(maxsize=None)
def conv_reference(form, dts, shape, design):
    """(ref, S) in float64, computed once per case and shared by every instance; never written to"""
    f, d = FORM[form], conv_data(form, dts, shape, design)
    ref, S = _conv64(d.x, d.w, f.relu_in), _conv64(d.x, d.w, f.relu_in, absolute=True)
    if d.bias is not None:
        ref, S = ref + d.bias.double(), S + d.bias.double().abs()
    if f.act == ACT_RELU:
        ref = ref.clamp_min(0)
    for r in (d.r1, d.r2):
        if r is not None:
            ref, S = ref + r.double(), S + r.double().abs()
    return ref, S


def half_bf16_step(mag):
    return torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - 8)


def group_slack(S, width=32, rel=2e-5):
    """rel * the largest S among the element's `width`-channel group (last dim, same pixel)"""
    n = S.shape[-1]
    nt = (n + width - 1) // width
    g = torch.nn.functional.pad(S, (0, nt * width - n)).reshape(*S.shape[:-1], nt, width).amax(-1, keepdim=True)
    return rel * g.expand(*S.shape[:-1], nt, width).reshape(*S.shape[:-1], nt * width)[..., :n]


def conv_bound(ref, S, odt):
    slack = group_slack(S)
    return slack + half_bf16_step(ref.abs() + slack) if odt == BF else slack + U24 * ref.abs()


def exact_expected(form, dts, shape, design):
    """the bit pattern an exact design must produce, in the output dtype (None for the designs held by the bound only)"""
    f, odt = FORM[form], DTYPES[dts][1]
    B, H, W = shape
    if design == "ones":
        cy = 3 - (torch.arange(H) == 0).int() - (torch.arange(H) == H - 1).int()
        cx = 3 - (torch.arange(W) == 0).int() - (torch.arange(W) == W - 1).int()
        cnt = (cy[:, None] * cx[None, :]).float() * f.Cin          # 4 Cin / 6 Cin / 9 Cin: corner / edge / inside (fewer on 1-pixel maps)
        return cnt[None, :, :, None].expand(B, H, W, f.Cout).to(odt)
    if design == "impulse":
        # one product of two bf16 values is exact in fp32; with the bias the float64 sum is exact, so its fp32 rounding is the kernel's
        return conv_reference(form, dts, shape, design)[0].float().to(odt)
    return None


def judge_conv(form, dts, shape, design, out_buf, in_bufs=None):
    """every assertion of one launch (or one emulation) -> (failures, worst |got - ref| / bound); judge_conv.slack_share is then the
    worst (|got - ref| - half a bf16 step) / slack: what the accumulation itself uses once the store's rounding is taken off"""
    f, odt = FORM[form], DTYPES[dts][1]
    B, H, W = shape
    fails = ["sentinel: " + n for n in guard_faults(dict(in_bufs or {}, out=out_buf))]
    got = out_buf.body.reshape(B, H, W, f.Cout).cpu()
    if bool(torch.isnan(got.float()).any()):
        fails.append("NaN in the output body (%d elements)" % int(torch.isnan(got.float()).sum()))
        return fails, math.inf
    ref, S = conv_reference(form, dts, shape, design)
    ex = exact_expected(form, dts, shape, design)
    if ex is not None:
        same = got == ex
        if not bool(same.all()):
            fails.append("exact design %s: %d elements differ" % (design, int((~same).sum())))
    err, slack = (got.double() - ref).abs(), group_slack(S)
    ratio = float((err / conv_bound(ref, S, odt)).max())
    judge_conv.slack_share = float(((err - (conv_bound(ref, S, odt) - slack)).clamp_min(0) / slack.clamp_min(1e-300)).max())
    if not ratio <= 1.0:
        fails.append("elementwise bound: %.3f x" % ratio)
    whole = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    if not whole < (2e-5 if odt == F32 else 6e-3):
        fails.append("whole-tensor bound: %.3e" % whole)
    return fails, ratio


def conv_buffers(form, dts, shape, design, device):
    """the guarded buffers of one launch: name -> Buf (None where the form has none)"""
    f, d = FORM[form], conv_data(form, dts, shape, design)
    mdt, odt, rdt = DTYPES[dts]
    B, H, W = shape
    wp = R.frag_pack(d.w.reshape(f.Cout, 9 * f.Cin), BF)
    b = {"x": Buf(mdt, d.x.numel(), device).put(d.x), "w": Buf(BF, wp.numel(), device).put(wp),
         "bias": None if d.bias is None else Buf(F32, f.Cout, device).put(d.bias),
         "r1": None if d.r1 is None else Buf(rdt, d.r1.numel(), device).put(d.r1),
         "r2": None if d.r2 is None else Buf(rdt, d.r2.numel(), device).put(d.r2),
         "out": Buf(odt, B * H * W * f.Cout, device, out=True)}
    return b


# ----------------------------------------------------------------------------- fp32 emulation of both tiled kernels
MUTANTS = ("halo_bottom", "halo_right", "drop_last_unit", "dup_last_unit", "skip_wave", "bf16_partials", "bias_shift4", "res_fp32_size",
           "skip_relu_in", "store_past_row", "swap_kykx")


def _halo(xe, mutant):
    """the padded map [B, H+2, W+2, C] the halo loader stages; out-of-image pixels are zeros.  halo_bottom / halo_right: the bound on
    iy / ix is missing, so the loader reads what lies behind in memory -- the next row, the next image, or the NaN band"""
    B, H, W, C = xe.shape
    xp = torch.zeros(B, H + 2, W + 2, C)
    xp[:, 1:-1, 1:-1] = xe
    flat = torch.cat([xe.reshape(B * H * W, C), torch.full((W + 1, C), math.nan)])
    if mutant == "halo_bottom":
        for b in range(B):
            xp[b, H + 1, 1:W + 1] = flat[(b + 1) * H * W:(b + 1) * H * W + W]
    if mutant == "halo_right":
        for b in range(B):
            xp[b, 1:H + 1, W + 1] = flat[b * H * W + W:(b + 1) * H * W + W:W]
    return xp


def unit_order(Cin, instance):
    """per wave, the 32-deep K units (u = tap * Cin/32 + channel group) in the order the wave accumulates them"""
    upt = Cin // 32
    if instance == "8x8":
        return [list(range(w, 9 * upt, 4)) for w in range(4)]
    assert Cin % 128 == 0
    return [[tap * upt + 4 * c + w for c in range(Cin // 128) for tap in range(9)] for w in range(4)]


def emulate_conv(form, dts, shape, design, instance, mutant=None):
    """the kernel's arithmetic in fp32: every wave sums its units' 32-deep products in its order, the four partial tiles are added in
    wave order, then bias, ReLU, residuals and the one rounding.  Returns the output as a Buf (bands included)."""
    f, d = FORM[form], conv_data(form, dts, shape, design)
    mdt, odt, rdt = DTYPES[dts]
    B, H, W = shape
    M = B * H * W
    xe = d.x.float()
    if f.relu_in and mutant != "skip_relu_in":
        xe = torch.where(xe > 0, xe, torch.zeros_like(xe))
    xp = _halo(bf(xe), mutant)
    w = d.w.float()
    upt = f.Cin // 32

    def unit(u):
        tap, c32 = divmod(u, upt)
        ky, kx = divmod(tap, 3)
        if mutant == "swap_kykx":
            ky, kx = kx, ky
        a = xp[:, ky:ky + H, kx:kx + W, 32 * c32:32 * c32 + 32].reshape(M, 32)
        return a @ w[:, tap, 32 * c32:32 * c32 + 32].T
    parts = []
    for wv, seq in enumerate(unit_order(f.Cin, instance)):
        if mutant == "drop_last_unit" and wv == 1:
            seq = seq[:-1]
        if mutant == "dup_last_unit" and wv == 0:
            seq = seq + [seq[-1]]
        acc = torch.zeros(M, f.Cout)
        for u in seq:
            acc = acc + unit(u)
        parts.append(bf(acc) if mutant == "bf16_partials" else acc)
    if mutant == "skip_wave":
        parts[2] = torch.zeros_like(parts[2])
    v = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    if d.bias is not None:
        bias = d.bias
        if mutant == "bias_shift4":
            BN = 32 if instance == "8x16n32" else 64
            idx = torch.arange(f.Cout)
            idx = torch.where(idx >= BN, idx + 4, idx)
            bias = torch.cat([d.bias, torch.full((4,), math.nan)])[idx]
        v = v + bias[None]
    if f.act == ACT_RELU:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    for r in (d.r1, d.r2):
        if r is None:
            continue
        if mutant == "res_fp32_size" and rdt == BF:
            n = r.numel()
            r = torch.cat([r.reshape(-1), torch.full((n,), math.nan, dtype=BF)]).view(F32)[:n].reshape(r.shape)
        v = v + r.float().reshape(M, f.Cout)
    out = Buf(odt, M * f.Cout, "cpu", out=True).put(v.to(odt))
    if mutant == "store_past_row" and H % 8:
        # rows H .. of the last tile row are stored too: row H of image b is row 0 of image b + 1 (a race the right values may win); behind
        # the last image it is the band
        out.t[GUARD + out.numel:][:min(GUARD, W * f.Cout)] = 0.0
    return out


# ----------------------------------------------------------------------------- sp3_upsample2x
def upsample_taps64(n_in, n_out, device="cpu"):
    src = torch.arange(n_out, dtype=torch.float64, device=device) * ((n_in - 1) / (2 * n_in - 1) if n_in > 1 else 0.0)
    i0 = src.floor().long().clamp(0, n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), src - i0


def upsample_bound(r, OH, OW):
    """fp32 bound per element of sp3_upsample2x's result against gemm_desc_ref.upsample2x (float64, exact ratio (in-1)/(2 in-1)), from
    the kernel's index arithmetic, in units of u = 2^-24:
      sh = fl((H-1)/(2H-1)) = sh (1 + e), |e| <= u.  ly = fma(sh, oy, -y0) is the exact weight + sh oy e + one rounding (<= u ly): with
      sh < 1/2 the row weight is off by dy <= u (oy/2 + 1), and hy = fl(1 - ly) by the same amount in the other direction plus one
      rounding.  A weight error moves the result by dy * |bottom row - top row|, at most dy * Dy with Dy the larger of the two tap
      differences down the rows.  (fy = fl(sh oy) truncates to the exact floor wherever the exact source index is no integer: its distance
      to one is >= 1/(2H-1).  It is an integer in the last row of the uncropped output only; there the kernel may hold y0 = H-2 with
      ly ~ 1 where the reference holds y0 = y1 = H-1: the same value up to dy * |row H-1 - row H-2|, so Dy takes that pair there.)
      Likewise in x.  The arithmetic itself -- hy, hx, lx v01, the fma of a row, ly bot, the final fma -- rounds six times on the way
      to the result, each time on a magnitude <= T, the largest tap:
          bound = u (oy/2 + 1) Dy + u (ox/2 + 1) Dx + 6 u T"""
    B, h, w, C = r.shape
    r = r.double()
    y0, y1, _ = upsample_taps64(h, OH, r.device)
    x0, x1, _ = upsample_taps64(w, OW, r.device)
    ya, xa = torch.where(y1 == y0, (y0 - 1).clamp_min(0), y0), torch.where(x1 == x0, (x0 - 1).clamp_min(0), x0)
    g = lambda ys, xs: r[:, ys][:, :, xs]
    Dy = torch.maximum((g(y1, xa) - g(ya, xa)).abs(), (g(y1, x1) - g(ya, x1)).abs())
    Dx = torch.maximum((g(ya, x1) - g(ya, xa)).abs(), (g(y1, x1) - g(y1, xa)).abs())
    T = torch.stack((g(ya, xa), g(ya, x1), g(y1, xa), g(y1, x1))).abs().amax(0)
    oy = torch.arange(OH, dtype=torch.float64, device=r.device)[None, :, None, None]
    ox = torch.arange(OW, dtype=torch.float64, device=r.device)[None, None, :, None]
    return U24 * ((oy / 2 + 1) * Dy + (ox / 2 + 1) * Dx + 6 * T)


def emulate_upsample(r, OH, OW):
    """the kernel's fp32 arithmetic (csrc/dpt.hip, common.h up2x_taps / up2x_mix: fy = fl(sh oy), ly = fma(sh, oy, -y0), the two fma
    contractions of the mix) on the CPU; an fma is a float64 product-sum rounded once"""
    B, h, w, C = r.shape
    v = r.float()

    def taps(n_in, n_out):
        s = torch.tensor((n_in - 1), dtype=F32) / torch.tensor(2 * n_in - 1, dtype=F32) if 2 * n_in > 1 else torch.tensor(0.0)
        o = torch.arange(n_out, dtype=F32)
        i0 = (s * o).to(torch.int64).clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        l = (s.double() * o.double() - i0.double()).float()
        return i0, i1, l, 1.0 - l
    y0, y1, ly, hy = taps(h, OH)
    x0, x1, lx, hx = taps(w, OW)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    lx_, hx_ = lx[None, None, :, None], hx[None, None, :, None]
    ly_, hy_ = ly[None, :, None, None], hy[None, :, None, None]
    top = fma(hx_, v[:, y0][:, :, x0], lx_ * v[:, y0][:, :, x1])
    bot = fma(hx_, v[:, y1][:, :, x0], lx_ * v[:, y1][:, :, x1])
    return fma(hy_, top, ly_ * bot)


def upsample_data(B, h, w, C, dtype, seed=0):
    """maps for the bilinear x2 tests.  bf16: values on the fixed grid of 2^-7 in (-2, 2).  With bf16's few mantissa bits a float64
    interpolant of free bf16 data is an EXACT tie between two bf16 values surprisingly often (weights k / (2 in - 1): whenever two taps
    differ by a multiple of 2 in - 1 steps -- 1.2 % of the elements at in = 5), and fp32 arithmetic may fall to either side of a tie.
    On a fixed grid the interpolant is (an integer) * 2^-7 / (an odd number) and a tie an odd multiple of a smaller power of two: no
    element is an exact tie, and two candidates are left to those within the fp32 bound of a boundary only."""
    g = torch.Generator().manual_seed(7000 + seed)
    x = (torch.rand(B, h, w, C, generator=g) * 2 - 1) * 1.9
    return (torch.round(x * 128) / 128).to(BF) if dtype == BF else x


def bf16_ord(t):
    """bf16 values as integers in their order: neighbours differ by 1"""
    i = t.to(BF).view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


def bf16_candidates(ref, bound):
    """a bf16 store of any value within `bound` of ref: the roundings of the interval's ends (equal, or the two neighbours where the
    interval straddles a rounding boundary) -> (lo, hi, mask of the two-candidate elements)"""
    lo, hi = (ref - bound).float().to(BF), (ref + bound).float().to(BF)
    return lo, hi, lo != hi


def judge_upsample(got, r, OH, OW):
    """-> (failures, share of the bound used (fp32) or two-candidate share (bf16))"""
    ref = R.upsample2x(r.double(), OH, OW)
    bound = upsample_bound(r, OH, OW)
    got = got.cpu()
    if bool(torch.isnan(got.float()).any()):
        return ["NaN in the output body"], math.inf
    if got.dtype == F32:
        ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
        return ([] if ratio <= 1.0 else ["elementwise bound: %.3f x" % ratio]), ratio
    lo, hi, two = bf16_candidates(ref, bound)
    ok = (got.float() >= lo.float()) & (got.float() <= hi.float())
    share = float(two.float().mean())
    fails = [] if bool(ok.all()) else ["%d elements are no bf16 rounding of a value within the fp32 bound" % int((~ok).sum())]
    if share > 0.01:
        fails.append("two-candidate share %.4f > 1 %%: the data does not meet the test's condition" % share)
    return fails, share


# ----------------------------------------------------------------------------- sp3_head_final
def head_raw_reference(feat, w, b):
    """raw = feat @ w^T + b in float64 on the features as stored, and S = |feat| @ |w|^T + |b|"""
    f, w, b = feat.double(), w.double(), b.double()
    return f @ w.T + b, f.abs() @ w.abs().T + b.abs()


def head_post_reference(raw):
    """dust3r/heads/postprocess.py on the kernel's OWN raw, in float64: (pts, conf, relative bounds)
    pts = xyz * expm1(d) / max(d, 1e-8), d = |xyz|.  In units of u = 2^-24: x^2 + y^2 + z^2 carries 3 u (a rounding per square, two adds),
    sqrtf halves that and adds its own step (<= 1 ulp = 2 u): d is off by 3.5 u.  expm1(d) / d reacts to d with the factor
    d e^d / (e^d - 1) - 1 <= d; expm1f is accurate to 1 ulp (2 u), the division to 2.5 ulp (5 u), the final product adds u:
        |pts - ref| <= (3.5 d + 8) u |ref|
    conf = 1 + expf(c): expf to 1 ulp (2 u of e^c <= conf), one rounding of the sum, one u of headroom: |conf - ref| <= 4 u ref"""
    raw = raw.double()
    xyz, c = raw[:, :3], raw[:, 3]
    d = xyz.norm(dim=1, keepdim=True)
    pts = xyz * torch.expm1(d) / d.clamp_min(1e-8)
    conf = 1 + torch.exp(c)
    return pts, conf, (3.5 * d + 8) * U24, 4 * U24


# ----------------------------------------------------------------------------- sp3_im2col_patch
def im2col_reference(img, p):
    """[B, C, H, W] -> rows [B * (H/p) * (W/p), C p p], k = (c, py, px)"""
    return torch.nn.functional.unfold(img, p, stride=p).transpose(1, 2).reshape(-1, img.shape[1] * p * p)
