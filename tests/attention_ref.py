"""Case builder and float64 reference for the attention kernels (csrc/attention.hip) in every launch form the engine uses.

A case is (form, precision, B, heads, Nq, Nk, distribution) plus, when it is laid out in memory, an output kind and a pad fill:

  form  "a"   sp3_attention on the interleaved [R, 2A] q|k buffer (ldq = ldk = 2A, k at column A)          engine._attn_core, fp32
        "f"   sp3_attention, separate row-major q and k with Nq != Nk                                       engine.decoder, fp32
        "b"   sp3_attention_packed on ONE fragment-order matrix, q_cols = k_cols = 2A, k_col0 = A           engine._attn_core, bf16
        "c"   sp3_attention_packed, separate A-wide q and k matrices                                        engine.decoder, bf16
        "db" / "dc"   forms b / c as a grouped launch: 2B images, o_group = B, o_group_rows = Rp            engine.decoder_grouped
        "e"   sp3_attention_packed_qproj: q = RoPE(LN-folded projection) inside the launch, two groups      engine.decoder_grouped
        (g)   the 16 x 48 heads of the value encoder is a SHAPE of forms a and b: dims = 48 of every 64 head columns are used,
              the rest is zero in q, k and v, scale = 48 ** -0.5
  precision   "fp32" | "f32x3" | "f16x3" (row forms, fp32 operands) | "bf16"
  output kind (dtype, packed): fp32 / bf16, row-major with ldo > heads * 64 / fragment order
  pad fill    "zero" | "stale" (finite, 50 x the operands' magnitude: what a workspace shared between geometries holds) |
              "nan-qk" (q / k pads NaN, V pads as in stale)

Case(...) holds the operands as the kernel receives them (bf16-rounded for bf16), the float64 reference softmax(q k^T scale) v, the
elementwise scale A = softmax @ |v| and bound().  layout(device, kind, fill) places them in guarded buffers; Layout.launch(ops) runs
the op, Layout.output() / Layout.untouched() read the result back.  emulate() restates attention_packed_kernel's arithmetic in
torch fp32 on the SAME buffers (so the packers and the column / row geometry are part of what it checks) and takes mutants.
Nothing here touches a GPU at import time.
"""
import math

import torch

from gemm_desc_ref import BF, GUARD, SENT, bf, frag_numel, frag_offsets, frag_pack, frag_unpack, ln_fold_apply, pv_offsets, \
    rope_cols_apply, rope_tables

U32 = 2.0 ** -24                      # unit roundoff of fp32
LOG2E = 1.4426950408889634
ROW_FORMS, PACKED_FORMS = ("a", "f"), ("b", "c", "db", "dc", "e")
FORMS = ROW_FORMS + PACKED_FORMS
PRECISIONS = {"a": ("fp32", "bf16", "f32x3", "f16x3"), "f": ("fp32", "bf16", "f32x3", "f16x3"),
              "b": ("bf16",), "c": ("bf16",), "db": ("bf16",), "dc": ("bf16",), "e": ("bf16",)}
DISTS = ("flat", "peaked", "tie", "shift")
FILLS = ("zero", "stale", "nan-qk")
KINDS = tuple((dt, packed) for dt in (torch.float32, BF) for packed in (False, True))
GAMMA, DELTA = 16.0, 32.0             # spike / common component: exact in bf16; GAMMA^2 / 8 = 32 in logit, DELTA^2 / 8 = 128
# whole-tensor max-norm bounds of the existing op tests (test_ops_gpu.py), asserted next to the elementwise bound
WHOLE = {"fp32": 2e-5, "f32x3": 5e-5, "f16x3": 2e-5, "bf16": 1e-2}
WHOLE_BF16_OUT = 1.5e-2

# (B, heads, Nq, Nk, extra): the smallest shapes that reach every branch
SHAPES = {
    "ragged": (2, 3, 17, 65, {}),                            # ragged q block, a ragged tile that holds one key
    "six_tiles": (1, 2, 33, 323, {}),                        # waves 0 and 1 take two tiles: alpha != 1
    "ten_tiles": (1, 2, 50, 577, {}),                        # wave 0 takes three
    "qb2": (1, 2, 513, 323, {"npad_q": 528}),                # QB = 2; the last workgroup's second block is past the padded rows
    "g": (2, 16, 20, 20, {"dims": 48}),                      # the value encoder's heads
    "e_small": (1, 12, 12, 12, {}),                          # form e: D = 768 fixed
    "e_two": (2, 12, 100, 100, {}),
}
STALE_SHAPES = ("ragged", "six_tiles")
FORM_SHAPES = {"a": ("ragged", "six_tiles", "ten_tiles", "g"), "f": ("ragged", "six_tiles", "ten_tiles"),
               "b": ("ragged", "six_tiles", "ten_tiles", "qb2", "g"), "c": ("ragged", "six_tiles", "ten_tiles", "qb2"),
               "db": ("ragged", "six_tiles", "qb2"), "dc": ("ragged", "six_tiles", "qb2"), "e": ("e_small", "e_two")}
WIDE_SHAPE = "six_tiles"              # the one case per form with vt_ld / npad_k one tile above the minimum
WIDE_SHAPES = (WIDE_SHAPE, "e_two")   # (form e has its own shapes)


def matrix():
    """every (form, shape name) of the test matrix"""
    return [(f, s) for f in FORMS for s in FORM_SHAPES[f]]


def _rnd(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _r(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- which keys carry the peaks
def peak_keys(Nk):
    """eight keys J[c], one per class c = r mod 8, at the positions where the kernels change behaviour: key 0 and 63 (the ends of
    wave 0's first tile), 64 (first key of wave 1), 255 / 256 (the last key of wave 3's first tile / the first key of wave 0's SECOND
    tile, the only place where alpha is neither 1 nor exp(-inf)), Nk - 1 (inside the ragged tile), the ragged tile's first key, one
    mid-tile key.  Positions beyond Nk are replaced by evenly spread free keys (fewer than eight keys: classes share)."""
    rag0 = (Nk - 1) // 64 * 64
    want = [0, 63, 64, 255, 256, Nk - 1, rag0, 64 * ((Nk - 1) // 128) + 37]
    J = []
    for j in want:
        if 0 <= j < Nk and j not in J:
            J.append(j)
    free = [j for j in range(Nk) if j not in J]
    step = max(1, len(free) // 8)
    for j in free[step // 2::step]:
        if len(J) < 8:
            J.append(j)
    while len(J) < 8:
        J.append(J[len(J) % max(1, len(set(J)))])
    return J


def tie_partners(Nk, J):
    """for every class a second key with the same k row: in another tile of the SAME wave where the sequence has one (tile + 4: the
    pair then meets in that wave's online rescale), else in the next tile (another wave: the pair meets in the merge)"""
    nt = (Nk + 63) // 64
    used, out = set(J), []
    for c, j in enumerate(J):
        t = j // 64
        cands = [t + 4, t - 4] if c % 2 == 0 else []
        cands += [(t + 1) % nt, (t + 2) % nt, (t + 3) % nt, t]
        p = None
        for tt in cands:
            if not 0 <= tt < nt:
                continue
            for off in range(64):
                key = tt * 64 + (j + 17 + off) % 64
                if key < Nk and key not in used and (key // 64 != t or nt == 1):
                    p = key
                    break
            if p is not None:
                break
        if p is None:                                  # no free key in another tile (Nk = 65, or a single tile): any free key,
            free = [key for key in range(Nk) if key not in used]          # and none at all below 16 keys: the class stays peaked
            p = free[(7 * c) % len(free)] if free else j
        used.add(p)
        out.append(p)
    return out


class Case:
    def __init__(self, form, prec, shape, dist, seed=0):
        B, heads, Nq, Nk, extra = SHAPES[shape]
        assert form in FORMS and prec in PRECISIONS[form] and dist in DISTS
        self.form, self.prec, self.shape, self.dist = form, prec, shape, dist
        self.grouped = form in ("db", "dc", "e")
        self.Bt = 2 * B if self.grouped else B          # images of the launch
        self.o_group = B if self.grouped else 0
        self.heads, self.Nq, self.Nk, self.C = heads, Nq, Nk, heads * 64
        self.dims = extra.get("dims", 64)
        self.scale = self.dims ** -0.5
        self.wide = shape in WIDE_SHAPES
        self.npad_q_min = extra.get("npad_q")
        self.J = peak_keys(Nk)
        self.J2 = tie_partners(Nk, self.J)
        self.sdim = 31 if form == "e" else self.dims - 1          # form e: a head dimension the (y = 0) positions leave unrotated
        self.gamma = GAMMA
        gen = torch.Generator().manual_seed(1000 * seed + 7 * sum(map(ord, form + shape + dist)))
        Bt = self.Bt
        k, v = _rnd(gen, Bt, Nk, heads, 64), _rnd(gen, Bt, Nk, heads, 64)
        if form == "e":
            self._build_qproj(gen)
            q = None
        else:
            q = _rnd(gen, Bt, Nq, heads, 64) * 2
        if dist in ("peaked", "tie"):
            k[..., :8] = 0
            for c, j in enumerate(self.J):
                if self.J.index(j) == c:
                    k[:, j, :, c] = self.gamma
            if q is not None:
                q[..., :8] = 0
                rows = torch.arange(Nq)
                q[:, rows, :, rows % 8] = self.gamma
            if dist == "tie":
                for c, (j, p) in enumerate(zip(self.J, self.J2)):
                    k[:, p] = k[:, j]
        if dist == "shift":
            k[..., self.sdim] = DELTA
            if q is not None:
                q[..., self.sdim] = DELTA
        if self.dims < 64:
            k[..., self.dims:] = 0
            v[..., self.dims:] = 0
            if q is not None:
                q[..., self.dims:] = 0
        if prec == "bf16":
            k, v = bf(k), bf(v)
            q = bf(q) if q is not None else None
        self.k, self.v = k, v
        if form == "e":
            self.q64, self.qerr = self._qproj_ref()
            self.q = bf(self.q64.float())                           # what the kernel's projection should hand its softmax (emulation)
        else:
            self.q, self.q64, self.qerr = q, q.double(), None
        s = torch.einsum("bqhd,bkhd->bhqk", self.q64, k.double()) * self.scale
        self.scores = s
        self.p = torch.softmax(s, -1)
        self.ref = torch.einsum("bhqk,bkhd->bqhd", self.p, v.double())              # [Bt, Nq, heads, 64]
        self.A = torch.einsum("bhqk,bkhd->bqhd", self.p, v.double().abs())
        self.bound = bound(self)

    # ---- form e: q = RoPE2D(LN(x) Wq^T + b) from bf16 x, bf16 W, the producer's fp32 statistics
    def _build_qproj(self, gen):
        D, G, R = self.C, 2, self.o_group * self.Nq
        assert D == 768
        self.R = R
        x = _rnd(gen, G, R, D) * 2 + 0.2
        gam = _rnd(gen, G, D) * 0.3 + 1
        W = _rnd(gen, G, D, D) * 0.05 * gam[:, None, :]
        b = _rnd(gen, G, D)
        tok = torch.arange(R) % self.Nq
        if self.dist == "flat":
            nw = max(1, int(math.isqrt(self.Nq)))
            pos = torch.stack((tok // nw, tok % nw), -1)
        else:
            # y = 0: the head dimensions 0..31 (which turn with y) keep the structure the distribution puts there, 32..63 still rotate
            pos = torch.stack((torch.zeros_like(tok), tok % 10), -1)
        if self.dist in ("peaked", "tie"):
            # row r of x carries a spike in column c(r); Wq routes column c to head dimension c of every head and to nothing else
            cols = torch.arange(D)
            hd = cols % 64
            W[:, hd < 8, :] = 0
            W[:, :, :8] = 0
            for c in range(8):
                W[:, cols[hd == c], c] = 1.0
            b[:, hd < 8] = 0
            x[:, torch.arange(R), tok % 8] += 64.0
        if self.dist == "shift":
            hd = torch.arange(D) % 64
            W[:, hd == self.sdim, :] = 0
            b[:, hd == self.sdim] = DELTA
        self.x, self.W, self.bias, self.pos = bf(x), bf(W), b, pos.to(torch.int32)
        xs = self.x.double().view(G, R, D // 32, 32)
        self.stats = torch.stack((xs.sum(-1), (xs * xs).sum(-1)), -1).float()              # [G, R, D/32, 2]
        self.ln_s = self.W.double().sum(2).float()                                           # [G, D]
        if self.dist in ("peaked", "tie"):
            # the key spike is sized from the q spike the projection really produces, so that the peak is 32 in logit
            q, _ = self._qproj_ref()
            rows = torch.arange(self.Nq)
            spike = q[:, rows, :, rows % 8].abs().median()
            self.gamma = float(bf(torch.tensor(32.0 / (self.scale * float(spike)))))

    def _qproj_ref(self):
        """(q in float64 [Bt, Nq, heads, 64], a bound on what the kernel's q may differ by: its bf16 rounding plus the fp32
        accumulation of the 768-term projection and of the epilogue)"""
        G, R, D = 2, self.R, self.C
        cos, sin = rope_tables("cpu")
        qs, es = [], []
        for g in range(G):
            x, W = self.x[g].double(), self.W[g].double()
            y = ln_fold_apply(x @ W.T, self.stats[g], D, 1e-6, self.ln_s[g]) + self.bias[g].double()[None]
            q = rope_cols_apply(y, self.pos, cos, sin)
            s1, s2 = self.stats[g][..., 0].double().sum(1), self.stats[g][..., 1].double().sum(1)
            mean = s1 / D
            rstd = 1.0 / torch.sqrt((s2 / D - mean * mean).clamp_min(0) + 1e-6)
            mag = rstd[:, None] * (x.abs() @ W.abs().T) + (rstd * mean).abs()[:, None] * self.ln_s[g].double().abs()[None] + self.bias[g].double().abs()[None]
            mag = mag + mag[:, torch.arange(D) ^ 16]                                        # RoPE mixes a column with its partner
            # the row statistics are fp32 sums too: rstd and mean carry ~ (D / 32 + 4) roundings
            err = 2.0 ** -9 * q.abs() + (D + 64) * U32 * mag
            qs.append(q.view(self.o_group, self.Nq, self.heads, 64))
            es.append(err.view(self.o_group, self.Nq, self.heads, 64))
        return torch.cat(qs), torch.cat(es)

    # ---- geometry
    def out_row(self, b, o_group_rows=None):
        """first output row of image b (header: sp3_attention_packed)"""
        if not self.grouped:
            return b * self.Nq
        rows = self.Rp if o_group_rows is None else o_group_rows
        return (b // self.o_group) * rows + (b % self.o_group) * self.Nq

    @property
    def Rp(self):
        return _r(self.o_group * self.Nq, 16)

    @property
    def out_rows(self):
        return 2 * self.Rp if self.grouped else self.Bt * self.Nq

    def layout(self, device, kind=(torch.float32, False), fill="zero"):
        return Layout(self, device, kind, fill)


def bound(case):
    """Elementwise bound on |got - ref| / A, A = softmax @ |v|, per (image, row, head): derived, not tuned.

    The kernels compute p^_j = exp(s^_j - m) / sum_i exp(s^_i - m) with scaled scores s^_j = s_j + d_j, |d_j| <= ds, round p^ (P, before
    the P.V product) and accumulate in fp32.  Then p^_j / p_j lies in [exp(-2 ds), exp(2 ds)] -- ds from the numerator, ds from the
    sum -- and   |sum_j (p^_j - p_j) v_j| <= (exp(2 ds) - 1) * A.   The terms:
      score    2 * ds, with ds per row from the case's own operands:
                 64 * 2^-24 * max_j sum_i |q_i k_ji| * |scale|        the 64-term fp32 accumulation of q.k (worst case gamma_64)
               + 4 * 2^-24 * max_j |s_j| + 4 * 2^-24                  scaling, the subtraction of the maximum (as an fma or not), the
                                                                      exponential's argument reduction and its last-bit error
               + split modes: the dropped lo * lo product, 2^-16 (f32x3: |lo| <= 2^-8 |x|) or 2^-22 (f16x3: 2^-11 each) of the same sum
               + form e: sum_i dq_i |k_ji - c_i| * |scale| with dq the kernel's own q error (bf16 rounding, 2^-9 |q|, plus the fp32
                 accumulation of the 768-term projection and its LayerNorm / RoPE epilogue), since the reference keeps q in float64;
                 c_i is the midrange of k_i over the keys (a score error common to all keys of a row leaves the softmax alone)
      P        the rounding of P before P.V: 2^-9 (bf16), 2^-17 (f32x3), 2^-23 (f16x3), none for fp32.  The split modes split V the
               same way and drop the lo * lo product of P.V too: 2^-17 + 2^-16, and 2^-23 + 2^-22, on top
      sums     the fp32 accumulation over Nk terms of the numerator and of the row sum: 2 * (Nk + 8) * 2^-24 (8: the merge of the
               four wave states and the final 1 / L)
    and a factor 2 on top for the order of summation (the per-wave partial sums are rescaled by exp(m_w - M), which the worst-case
    figures above take in one piece).  exp(2 ds) - 1 is kept as such: for form e on peaked rows ds is not small.
    Returns [Bt, Nq, heads, 1]; multiply by A.  bf16 OUTPUT adds half a bf16 step of |ref| (out_tol)."""
    q, k = case.q64.abs(), case.k.double().abs()
    sc = abs(case.scale)
    absdot = torch.einsum("bqhd,bkhd->bhqk", q, k).amax(-1) * sc                     # [Bt, heads, Nq]
    smax = case.scores.abs().amax(-1)
    ds = 64 * U32 * absdot + 4 * U32 * smax + 4 * U32
    if case.prec == "f32x3":
        ds = ds + 2.0 ** -16 * absdot
    if case.prec == "f16x3":
        ds = ds + 2.0 ** -22 * absdot
    if case.qerr is not None:
        # sum_i dq_i k_ji = sum_i dq_i (k_ji - c_i) + a term common to all keys of the row, which the softmax does not see:
        # c_i = the midrange of k_i over the keys
        kk = case.k.double()
        mid = (kk.amax(1, keepdim=True) + kk.amin(1, keepdim=True)) / 2
        ds = ds + torch.einsum("bqhd,bkhd->bhqk", case.qerr, (kk - mid).abs()).amax(-1) * sc
    pterm = {"fp32": 0.0, "bf16": 2.0 ** -9, "f32x3": 2.0 ** -17 + 2.0 ** -17 + 2.0 ** -16, "f16x3": 2.0 ** -23 + 2.0 ** -23 + 2.0 ** -22}[case.prec]
    sums = 2 * (case.Nk + 8) * U32
    case.ds = ds
    return (2.0 * (torch.expm1(2 * ds) + pterm + sums)).permute(0, 2, 1)[..., None]


def out_tol(case, out_dtype):
    """the elementwise tolerance [Bt, Nq, heads, 64] of assertion 2"""
    tol = case.bound * case.A
    if out_dtype == BF:
        # half a bf16 step (8 significant bits) at the magnitude of the value that is rounded, which is ref give or take the bound
        _, e = torch.frexp(case.ref.abs() + tol)                            # |x| = m * 2^e, m in [0.5, 1): step 2^(e - 8)
        tol = tol + torch.ldexp(torch.ones_like(tol), e - 9)
    return tol


def whole_bound(case, out_dtype):
    """The whole-tensor figures of the older tests.  fp32 and bf16 hold on every distribution.  The two split modes were only ever
    measured on flat rows (f32x3 < 5e-5, f16x3 < 3e-6: those stay for flat); on the other distributions they are held to the
    split-mode figure 5e-5: both accumulate the raw score in fp32 in 32-wide MFMA steps, and at |s| ~ 150 (shift) ONE rounding of
    that sum is 2^-24 * 1024 * scale ~ 1e-5 of a probability, so f16x3's flat figure cannot be asked there (measured: 2.2e-5)."""
    w = WHOLE[case.prec]
    if case.prec == "f16x3":
        w = 3e-6 if case.dist == "flat" else WHOLE["f32x3"]
    if out_dtype == BF:
        w = WHOLE_BF16_OUT if case.prec == "bf16" else w + 2.0 ** -8
    return w


def ratio(case, got, out_dtype):
    """worst |got - ref| / tolerance; NaN in `got` counts as infinite"""
    r = (got.double() - case.ref).abs() / out_tol(case, out_dtype).clamp_min(1e-300)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


# ----------------------------------------------------------------------------- buffers
class Buf:
    """a flat tensor between two guard bands; .t is the payload view the kernels get"""

    def __init__(self, payload, device):
        n = payload.numel()
        self.full = torch.full((n + 2 * GUARD,), SENT, dtype=payload.dtype)
        self.full[GUARD:GUARD + n] = payload.reshape(-1)
        self.full = self.full.to(device)
        self.t = self.full[GUARD:GUARD + n]
        self.stride = 0

    def data_ptr(self):
        return self.t.data_ptr()

    def element_size(self):
        return self.t.element_size()

    def guards_intact(self):
        g = torch.cat((self.full[:GUARD], self.full[-GUARD:]))
        return bool((g == SENT).all())


def _pad_fill(gen, shape, fill, mag, nan_ok):
    if fill == "zero":
        return torch.zeros(shape)
    if fill == "nan-qk" and nan_ok:
        return torch.full(shape, math.nan)
    x = _rnd(gen, *shape) * (50.0 * mag)
    return torch.where(x.abs() < mag, torch.full_like(x, 50.0 * mag), x)


class Layout:
    """the buffers of one launch.  Pads hold `fill`; outputs are NaN everywhere"""

    def __init__(self, case, device, kind, fill):
        self.case, self.device, self.fill = case, device, fill
        self.out_dtype, self.out_packed = kind
        c = case
        self.opdt = BF if c.prec == "bf16" else torch.float32
        gen = torch.Generator().manual_seed(99)
        Bt, H, Nq, Nk, C = c.Bt, c.heads, c.Nq, c.Nk, c.C
        qmag = 2.0 if c.q is None else float(c.q.abs().max())
        kmag, vmag = float(c.k.abs().max()), float(c.v.abs().max())
        kd = c.k.reshape(Bt, Nk, C)
        qd = None if c.form == "e" else c.q.reshape(Bt, Nq, C)
        self.bufs = {}
        if c.form in ROW_FORMS:
            self.vt_ld = _r(Nk, 64) + (64 if c.wide else 0)
            vt = _pad_fill(gen, (Bt, H, 64, self.vt_ld), fill, vmag, False)
            vt[..., :Nk] = c.v.permute(0, 2, 3, 1)
            self.bufs["vt"] = Buf(vt.to(self.opdt), device)
            if c.form == "a":
                Pa = max(Nq, Nk) + 3                                   # rows of an image in the interleaved buffer, three of them beyond both
                qk = _pad_fill(gen, (Bt, Pa, 2 * C), fill, max(qmag, kmag), True)
                qk[:, :Nq, :C] = qd
                qk[:, :Nk, C:] = kd
                self.bufs["qk"] = Buf(qk.to(self.opdt), device)
                self.ldq = self.ldk = 2 * C
                self.sq = self.sk = Pa * 2 * C
            else:
                self.ldq, self.ldk = C + 8, C + 16
                qf = _pad_fill(gen, (Bt, Nq + 3, self.ldq), fill, qmag, True)
                kf = _pad_fill(gen, (Bt, Nk + 3, self.ldk), fill, kmag, True)
                qf[:, :Nq, :C] = qd
                kf[:, :Nk, :C] = kd
                self.bufs["q"], self.bufs["k"] = Buf(qf.to(self.opdt), device), Buf(kf.to(self.opdt), device)
                self.sq, self.sk = (Nq + 3) * self.ldq, (Nk + 3) * self.ldk
        else:
            shared = c.form in ("b", "db")
            self.npad_k = _r(Nk, 64) + (64 if c.wide else 0)
            self.npad_q = c.npad_q_min or _r(Nq, 16)
            if shared:
                self.npad_q = self.npad_k = max(_r(self.npad_q, 64), self.npad_k)
            vp = _pad_fill(gen, (Bt, self.npad_k, H, 64), fill, vmag, False)
            vp[:, :Nk] = c.v
            flat = torch.zeros(Bt * H * self.npad_k * 64)
            flat[pv_offsets(Bt, H, self.npad_k, self.npad_k).reshape(-1)] = vp.reshape(-1)
            self.bufs["vtp"] = Buf(flat.to(BF), device)
            kp = _pad_fill(gen, (Bt, self.npad_k, C), fill, kmag, True)
            kp[:, :Nk] = kd
            if shared:
                qp = _pad_fill(gen, (Bt, self.npad_q, C), fill, qmag, True)
                qp[:, :Nq] = qd
                m = torch.cat((qp, kp), -1).reshape(Bt * self.npad_k, 2 * C)
                self.bufs["qk"] = Buf(frag_pack(m.to(BF), BF), device)
                self.q_cols = self.k_cols = 2 * C
                self.q_col0, self.k_col0 = 0, C
            else:
                self.bufs["k"] = Buf(frag_pack(kp.reshape(Bt * self.npad_k, C).to(BF), BF), device)
                self.q_cols = self.k_cols = C
                self.q_col0 = self.k_col0 = 0
                if c.form != "e":
                    qp = _pad_fill(gen, (Bt, self.npad_q, C), fill, qmag, True)
                    qp[:, :Nq] = qd
                    self.bufs["q"] = Buf(frag_pack(qp.reshape(Bt * self.npad_q, C).to(BF), BF), device)
            if c.form == "e":
                G, R, D, Rp = 2, c.R, C, c.Rp
                xs = _pad_fill(gen, (G, Rp, D), fill, 2.0, True)
                xs[:, :R] = c.x
                self.bufs["x"] = Buf(torch.stack([frag_pack(xs[g].to(BF), BF) for g in range(G)]), device)
                self.bufs["x"].stride = Rp * D
                self.bufs["w"] = Buf(torch.stack([frag_pack(c.W[g].to(BF), BF) for g in range(G)]), device)
                self.bufs["w"].stride = D * D
                for name, t in (("stats", c.stats), ("ln_s", c.ln_s), ("bias", c.bias), ("pos", c.pos)):
                    self.bufs[name] = Buf(t.contiguous(), device)
                cos, sin = rope_tables("cpu")
                self.bufs["cos"], self.bufs["sin"] = Buf(cos, device), Buf(sin, device)
        rows = c.out_rows
        self.ldo = C + 8
        n_out = frag_numel(rows, C, self.out_dtype) if self.out_packed else rows * self.ldo
        self.bufs["out"] = Buf(torch.full((n_out,), math.nan, dtype=self.out_dtype), device)
        self.inputs0 = {n: b.full.clone() for n, b in self.bufs.items() if n != "out"}

    # ---- where the defined output lives
    def out_index(self, o_group_rows=None):
        """flat offsets [Bt, Nq, C] of the defined output elements inside the out payload"""
        c = self.case
        rows = torch.cat([c.out_row(b, o_group_rows) + torch.arange(c.Nq) for b in range(c.Bt)])
        if self.out_packed:
            return frag_offsets(c.out_rows, c.C, self.out_dtype)[rows].view(c.Bt, c.Nq, c.C)
        return (rows[:, None] * self.ldo + torch.arange(c.C)[None]).view(c.Bt, c.Nq, c.C)

    def output(self):
        """the defined region [Bt, Nq, heads, 64] (float64, on the CPU)"""
        c = self.case
        flat = self.bufs["out"].t.cpu()
        return flat[self.out_index().reshape(-1)].double().view(c.Bt, c.Nq, c.heads, 64)

    def raw_output(self):
        return self.bufs["out"].t.cpu().clone()

    def untouched(self):
        """True iff every out element outside the defined region still holds its NaN pre-fill (the columns beyond heads * 64 of a
        row-major output, the rows [o_group * Nq, o_group_rows) of a group, the padding of a fragment-order output), every guard
        band is intact and no input buffer changed"""
        flat = self.bufs["out"].t.cpu()
        mask = torch.ones(flat.numel(), dtype=torch.bool)
        mask[self.out_index().reshape(-1)] = False
        ok = bool(torch.isnan(flat[mask].float()).all())
        ok = ok and all(b.guards_intact() for b in self.bufs.values())
        for n, ref in self.inputs0.items():
            a, b_ = self.bufs[n].full.cpu(), ref.cpu()
            ok = ok and a.dtype == b_.dtype and torch.equal(a.view(torch.uint8), b_.view(torch.uint8))
        return ok

    # ---- the launch, as engine.py makes it
    def launch(self, ops, scale=None):
        c, bufs = self.case, self.bufs
        scale = c.scale if scale is None else scale
        out = bufs["out"].t
        if self.out_packed:
            out = ops.PackedAct(c.out_rows, c.C, self.out_dtype, self.device, data=bufs["out"].t)
        kw = dict(B=c.Bt, heads=c.heads, Nq=c.Nq, Nk=c.Nk, scale=scale)
        if c.form in ROW_FORMS:
            if c.form == "a":
                qk = bufs["qk"].t.view(-1, 2 * c.C)
                q, k = qk, qk[:, c.C:]
            else:
                q, k = bufs["q"].t, bufs["k"].t
            mode = c.prec if c.prec in ("f32x3", "f16x3") else "fp32"
            prev = ops.get_product_mode()
            ops.set_product_mode(mode)
            try:
                ops.attention(q, self.sq, self.ldq, k, self.sk, self.ldk, bufs["vt"].t, self.vt_ld, out, self.ldo, **kw)
            finally:
                ops.set_product_mode(prev)
            return
        if c.grouped:
            kw.update(o_group=c.o_group, o_group_rows=c.Rp)
        kbuf = bufs["qk"] if "qk" in bufs else bufs["k"]
        if c.form == "e":
            D = c.C
            ops.attention_packed_qproj(bufs["x"], bufs["stats"], bufs["w"], bufs["ln_s"], bufs["bias"], bufs["pos"], bufs["cos"], bufs["sin"],
                                       kbuf, self.k_cols, self.k_col0, self.npad_k, bufs["vtp"], out, self.ldo, eps=1e-6,
                                       stats_group_stride=c.R * (D // 32) * 2, vec_group_stride=D, **kw)
            return
        qbuf = bufs["qk"] if "qk" in bufs else bufs["q"]
        ops.attention_packed(qbuf, self.q_cols, self.q_col0, self.npad_q, kbuf, self.k_cols, self.k_col0, self.npad_k, bufs["vtp"], out,
                             self.ldo, **kw)


def form_key(entry, shared_qk, k_col0, o_group, out_dtype, out_packed, prec):
    """what test_forms_are_the_models reduces an engine launch to"""
    return (entry, bool(shared_qk), bool(k_col0), bool(o_group), str(out_dtype).replace("torch.", ""), bool(out_packed), prec)


def covered_keys():
    """the form keys the matrix runs: every form in every precision it accepts and every output kind"""
    keys = set()
    for form in FORMS:
        for prec in PRECISIONS[form]:
            for dt, packed in KINDS:
                entry = "attention" if form in ROW_FORMS else "attention_packed_qproj" if form == "e" else "attention_packed"
                shared = form in ("a", "b", "db")
                keys.add(form_key(entry, shared, shared, form in ("db", "dc", "e"), dt, packed, prec))
    return keys


# ----------------------------------------------------------------------------- attention_packed_kernel, restated in torch fp32
MUTANTS = ("l_not_rescaled", "o_not_rescaled", "merge_own_max", "mask_dropped", "mask_off_by_one", "k_col0_ignored",
           "group_rows_formula", "head_mod")


def _exp2(x):
    return torch.exp2(x.float())


def _softmax_pv_emul(q, k, v, Nk, scale, mut):
    """one (image, head): q [Nq, 64], k / v [npad_k, 64] fp32 tensors holding bf16 values, pads as the buffers hold them.
    Tiles go to waves by tile & 3, base-2 online softmax per wave with the scale inside an fma, the tile maximum taken on the raw
    scores, P rounded to bf16 for the product while l sums the unrounded P, the four (m, l, O) states merged against their common
    maximum."""
    f32 = torch.float32
    sl2 = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    ntiles = (Nk + 63) // 64
    Nq = q.shape[0]
    ms, ls, os_ = [], [], []
    for w in range(4):
        m = torch.full((Nq,), -math.inf, dtype=f32)
        l = torch.zeros(Nq, dtype=f32)
        o = torch.zeros(Nq, 64, dtype=f32)
        for tile in range(w, ntiles, 4):
            kb = tile * 64
            s = q @ k[kb:kb + 64].T                                         # bf16 products are exact in fp32; accumulation in fp32
            if kb + 64 > Nk and mut != "mask_dropped":
                key = kb + torch.arange(64)
                dead = key > Nk if mut == "mask_off_by_one" else key >= Nk
                s = torch.where(dead[None], torch.full_like(s, -math.inf), s)
            mx = s.max(1).values
            m_new = torch.maximum(m, mx * sl2)
            alpha = _exp2(m - m_new)
            p = _exp2((s.double() * sl2.double() - m_new.double()[:, None]).float())      # fma: one rounding
            psum = p.view(Nq, 4, 4, 4).sum(-1).sum(-1).sum(-1)
            l = (l if mut == "l_not_rescaled" else l * alpha) + psum
            m = m_new
            if mut != "o_not_rescaled":
                o = o * alpha[:, None]
            o = o + bf(p) @ v[kb:kb + 64]
        ms.append(m), ls.append(l), os_.append(o)
    M = torch.stack(ms).max(0).values
    L = torch.zeros(Nq, dtype=f32)
    acc = torch.zeros(Nq, 64, dtype=f32)
    for w in range(4):
        sc = _exp2(ms[w] - M)
        if mut == "merge_own_max":
            sc = torch.where(torch.isinf(ms[w]), torch.zeros_like(sc), torch.ones_like(sc))
        L = L + ls[w] * sc
        acc = acc + os_[w] * sc[:, None]
    return acc * (1.0 / L)[:, None]


def emulate(lay, mut=None):
    """the packed launch of Layout `lay` (built on the CPU), read from its buffers through the unpackers; returns the out payload as
    the kernel would leave it (fp32 / bf16, row-major or fragment order, NaN where nothing is written)"""
    c = lay.case
    assert c.form in PACKED_FORMS and mut in (None,) + MUTANTS
    Bt, H, C = c.Bt, c.heads, c.C
    kbuf = lay.bufs["qk"] if "qk" in lay.bufs else lay.bufs["k"]
    kd = frag_unpack(kbuf.t, Bt * lay.npad_k, lay.k_cols, BF).float().view(Bt, lay.npad_k, lay.k_cols)
    if c.form == "e":
        qd = c.q.reshape(Bt, c.Nq, C)                                      # the projection, rounded to bf16 as attn_qproj does
        q_col0 = 0
    else:
        qbuf = lay.bufs["qk"] if "qk" in lay.bufs else lay.bufs["q"]
        qd = frag_unpack(qbuf.t, Bt * lay.npad_q, lay.q_cols, BF).float().view(Bt, lay.npad_q, lay.q_cols)
        q_col0 = lay.q_col0
    vd = lay.bufs["vtp"].t[pv_offsets(Bt, H, lay.npad_k, lay.npad_k).reshape(-1)].float().view(Bt, lay.npad_k, H, 64)
    k_col0 = 0 if mut == "k_col0_ignored" else lay.k_col0
    out = lay.bufs["out"].t.clone()
    idx = lay.out_index(c.o_group * c.Nq if mut == "group_rows_formula" else None)
    for b in range(Bt):
        for h in range(H):
            hh = h % (H - 1) if mut == "head_mod" else h
            o = _softmax_pv_emul(qd[b, :c.Nq, q_col0 + hh * 64:q_col0 + hh * 64 + 64], kd[b, :, k_col0 + hh * 64:k_col0 + hh * 64 + 64],
                                 vd[b, :, hh], c.Nk, c.scale, mut)
            out[idx[b, :, h * 64:(h + 1) * 64].reshape(-1)] = o.to(out.dtype).reshape(-1)
    return out


def read_payload(lay, payload):
    c = lay.case
    return payload[lay.out_index().reshape(-1)].double().view(c.Bt, c.Nq, c.heads, 64)
