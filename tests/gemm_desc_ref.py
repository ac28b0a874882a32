"""A float64 reference of sp3_gemm_desc (include/spann3r_hip.h), driven by the fields tests/golden/gemm_plan_table.jsonl stores.

Case(fields, seed) lays every buffer of one descriptor out by the header's layout rules (no allocation: `Case.bufs` holds name ->
Spec with the extent in elements, which tests/test_gemm_desc_ref_cpu.py checks for every census row), `materialize(device)` allocates
and fills them, `desc()` is the sp3_gemm_desc of the launch and `expected()` what every output must hold.  The formulas are the ones
of test_ops_gpu.py / test_gemm_lean_gpu.py / test_head_levels_gpu.py, gathered: products in float64 on the operands AS THE KERNEL
SEES THEM (bf16-rounded where it holds bf16, fp16 planes recombined for w_packed = 2), compared with an fp32-accumulate tolerance.

Builder rules
  - every buffer sits between two guard bands; outputs are filled with SENT, so a write beyond the layout's extent or into the pad
    columns of a row-major output (ldc > N) is seen; row-major inputs carry NaN in their pad columns (lda / ldw / ldr > extent), in
    three rows past M and in the guards, so a load outside the logical extent that reaches a result is seen.
  - fragment-order operands keep the zero padding the header prescribes.
  - W of the softmax loader (`w_slack`): the bank is allocated for ldw keys and the launch reads K of them.  The kernel loads the
    whole last k-block of W and relies on the PROBABILITIES past K being zero to cancel it, so NaN there fails by design of the test,
    not of the kernel: columns K..ldw hold a large finite value (3.0e3) instead.
  - strides and byte offsets (dropped by the table) are chosen non-minimal; the cross-attention k/v projection (second descriptor of
    a q/k/v pair, both sides in one launch) reads the other side's tokens and statistics through negative strides as engine.py does.
"""
import ctypes as C
import math

import torch

BF = torch.bfloat16
SENT = -24576.0          # exactly representable in bf16 and fp32; no kernel output of these operands comes near it
GUARD = 256              # elements in front of and behind every buffer
W_SLACK = 3.0e3
F32, BF16 = 0, 1
EPI_PLAIN, EPI_ROPE_VT, EPI_PIXSHUF, EPI_PARTIAL = 0, 1, 2, 3
LOAD_PLAIN, LOAD_CONV3X3, LOAD_SOFTMAX = 0, 1, 2
LN_EPS, SM_THRESH = 1e-6, 5e-4          # floats the table dropped: the model's values
ROPE_MAX_POS = 64


def bf(t):
    return t.to(BF).to(torch.float32)


# ----------------------------------------------------------------------------- fragment order (header: a_packed / w_packed)
def frag_geometry(dtype):
    """(KB, CH): k-block and per-lane chunk of a fragment-order operand of this dtype"""
    return (64, 16) if dtype == BF else (32, 8)


def frag_numel(rows, K, dtype):
    KB, _ = frag_geometry(dtype)
    return (rows + 15) // 16 * 16 * ((K + KB - 1) // KB * KB)


def frag_offsets(rows, K, dtype, device="cpu"):
    """element offset of (row, k) in a fragment-order [rows, K] operand, restated from the header text:
    [ceil(rows/16)][ceil(K/KB)][2 halves][64 lanes][CH/2], lane = 16*g + r holds row 16*nb + r, k = kb*KB + g*CH + e, e < CH/2 in the first half"""
    KB, CH = frag_geometry(dtype)
    nkb = (K + KB - 1) // KB
    r = torch.arange(rows, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    nb, rr, kb, g, e = r // 16, r % 16, k // KB, (k % KB) // CH, k % CH
    half, e2 = e // (CH // 2), e % (CH // 2)
    return (((nb * nkb + kb) * 2 + half) * 64 + 16 * g + rr) * (CH // 2) + e2


def frag_pack(x, dtype, Kalloc=None, slack=0.0):
    """dense [rows, K] -> flat fragment-order buffer (zero padded; columns K..Kalloc hold `slack`)"""
    rows, K = x.shape
    Kalloc = K if Kalloc is None else Kalloc
    out = torch.zeros(frag_numel(rows, Kalloc, dtype), dtype=dtype, device=x.device)
    if Kalloc > K:
        full = torch.full((rows, Kalloc), slack, dtype=dtype, device=x.device)
        full[:, :K] = x.to(dtype)
        x = full
    out[frag_offsets(rows, x.shape[1], dtype, x.device).reshape(-1)] = x.to(dtype).reshape(-1)
    return out


def frag_unpack(flat, rows, K, dtype):
    return flat[frag_offsets(rows, K, dtype, flat.device).reshape(-1)].reshape(rows, K)


def planes_pack(w):
    """fp32 [N, K] -> w_packed = 2: the blocks of the fp32 fragment order, but a block's first KB holds fp16(w) of every lane's 8 k
    ([64 lanes][8]) and its second KB fp16((w - h) * 2^11)"""
    flat = frag_pack(w, torch.float32)                                  # [blocks, 2 halves, 64 lanes, 4]
    blk = flat.view(-1, 2, 64, 4).permute(0, 2, 1, 3).reshape(-1, 64, 8)                       # a lane's 8 k
    hi = blk.to(torch.float16)
    lo = ((blk - hi.float()) * 2048.0).to(torch.float16)
    return torch.stack((hi, lo), 1).contiguous().view(torch.float32).reshape(-1)              # [blocks, 2 planes, 64 lanes, 8 halves]


def planes_unpack(flat, N, K):
    """the value the f16x3 product sees: h + l * 2^-11, as float64 [N, K]"""
    halves = flat.view(torch.float16).view(-1, 2, 64, 8).double()
    val = halves[:, 0] + halves[:, 1] / 2048.0                          # [blocks, lane, 8 k]
    nkb = (K + 31) // 32
    nb = (N + 15) // 16
    v = val.view(nb, nkb, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(nb * 16, nkb * 32)          # [nb, r, kb, g, e]
    return v[:N, :K]


def pv_offsets(B, heads, tokens, npad, device="cpu"):
    """offset of v[b, n, h, dd] in the PV-operand order [(b,h)][npad/32][4][64][8] written by the qkv_packed epilogue"""
    n = torch.arange(tokens, device=device)[:, None]
    dd = torch.arange(64, device=device)[None, :]
    u, kk = n // 32, n % 32
    w16 = kk % 16
    e, g = (w16 % 4) + 4 * (kk // 16), w16 // 4
    db, j = dd // 16, dd % 16
    per = ((u * 4 + db) * 64 + g * 16 + j) * 8 + e                      # [tokens, 64]
    bh = torch.arange(B * heads, device=device).view(B, 1, heads, 1) * (npad * 64)
    return bh + per.view(1, tokens, 1, 64)                              # [B, tokens, heads, 64]


# ----------------------------------------------------------------------------- reference pieces (checked one by one on the CPU)
def conv_rows(x, OH, OW, stride):
    """NHWC [B,H,W,C] -> the implicit-GEMM A [B*OH*OW, 9*C]: row = output pixel, k = (ky*3+kx)*C + ci, pad 1"""
    B, H, W, Cc = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cc, dtype=x.dtype, device=x.device)
    xp[:, 1:-1, 1:-1] = x
    oy = torch.arange(OH, device=x.device) * stride
    ox = torch.arange(OW, device=x.device) * stride
    taps = [xp[:, oy + ky][:, :, ox + kx] for ky in range(3) for kx in range(3)]             # 9 x [B,OH,OW,C]
    return torch.stack(taps, 3).reshape(B * OH * OW, 9 * Cc)


def pixshuf_scatter(y, B, H, W, ks, Cc):
    """GEMM rows [B*H*W, ks*ks*C] (n = (ky*ks+kx)*C + co) -> NHWC [B, ks*H, ks*W, C]"""
    return y.reshape(B, H, W, ks, ks, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, ks * H, ks * W, Cc)


def ln_fold_apply(prod, stats, ln_C, eps, s):
    """rstd * prod - rstd * mean * s from the producer's per-32-column (sum, sum of squares) partials [M, nt, 2]"""
    s1, s2 = stats[..., 0].double().sum(1), stats[..., 1].double().sum(1)
    mean = s1 / ln_C
    rstd = 1.0 / torch.sqrt((s2 / ln_C - mean * mean).clamp_min(0) + eps)
    return rstd[:, None] * prod - (rstd * mean)[:, None] * s.double()[None]


def rope_tables(device):
    half = 32
    inv = 1.0 / (100.0 ** (torch.arange(0, half, 2).float() / half))
    ang = torch.einsum("i,j->ij", torch.arange(ROPE_MAX_POS, dtype=torch.float32), inv)
    return ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)


def rope_cols_apply(y, pos, cos, sin):
    """2-D RoPE on columns of 64-wide heads: within a head, slab 0..31 turns with y, 32..63 with x; column c pairs with c ^ 16"""
    M, Nc = y.shape
    c = torch.arange(Nc, device=y.device)
    hc = c & 63
    axis, second, i0 = hc >> 5, ((hc >> 4) & 1).bool(), hc & 15
    p = pos.long()[:, axis]                                             # [M, Nc]
    cs, sn = cos.double()[p, i0[None]], sin.double()[p, i0[None]]
    partner = y[:, c ^ 16]
    return torch.where(second[None], y * cs + partner * sn, y * cs - partner * sn)


def softmax_keep(scores, thresh):
    """rows of softmax(scores), entries below thresh dropped: (kept probabilities, kept mass, row max, Z)"""
    m = scores.max(1, keepdim=True).values
    ex = torch.exp(scores - m)
    Z = ex.sum(1, keepdim=True)
    p = ex / Z
    p = torch.where(p < thresh, torch.zeros_like(p), p)
    return p, p.sum(1), m[:, 0], Z[:, 0]


def group_softmax_stats(x, width=32):
    """per `width`-column group (max, sum exp(x - max)) of finished rows [M, N] -> [M, ceil(N/width), 2]"""
    M, N = x.shape
    nt = (N + width - 1) // width
    pad = torch.full((M, nt * width), -math.inf, dtype=x.dtype, device=x.device)
    pad[:, :N] = x
    g = pad.view(M, nt, width)
    mx = g.max(-1).values
    return torch.stack((mx, torch.exp(g - mx[..., None]).sum(-1)), -1)


def upsample2x(r, OH, OW):
    """bilinear x2, align_corners, of NHWC [B,h,w,C], cropped to OH x OW (sp3_upsample2x)"""
    B, h, w, Cc = r.shape

    def taps(n_in, n_out):
        src = torch.arange(n_out, device=r.device, dtype=torch.float64) * ((n_in - 1) / (2 * n_in - 1) if n_in > 1 else 0.0)
        i0 = src.floor().long().clamp(0, n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0
    y0, y1, fy = taps(h, OH)
    x0, x1, fx = taps(w, OW)
    top = r[:, y0][:, :, x0] * (1 - fx)[None, None, :, None] + r[:, y0][:, :, x1] * fx[None, None, :, None]
    bot = r[:, y1][:, :, x0] * (1 - fx)[None, None, :, None] + r[:, y1][:, :, x1] * fx[None, None, :, None]
    return top * (1 - fy)[None, :, None, None] + bot * fy[None, :, None, None]


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ----------------------------------------------------------------------------- the builder
class Spec:
    def __init__(self, dtype, numel, out, fill):
        self.dtype, self.numel, self.out, self.fill = dtype, int(numel), out, fill
        self.t = None                # [GUARD + numel + GUARD] once materialised

    @property
    def body(self):
        return self.t[GUARD:GUARD + self.numel]

    def ptr(self, off=0):
        return self.t.data_ptr() + (GUARD + off) * self.t.element_size()

    def guards_intact(self):
        if not self.dtype.is_floating_point:
            return not bool(self.t[:GUARD].any() or self.t[GUARD + self.numel:].any())
        want = torch.full((GUARD,), self.fill, dtype=self.dtype, device=self.t.device)
        a, b = self.t[:GUARD], self.t[GUARD + self.numel:]
        if math.isnan(self.fill):
            return bool(torch.isnan(a).all() and torch.isnan(b).all())
        return torch.equal(a, want) and torch.equal(b, want)


def _grid(tokens):
    nh = int(math.isqrt(tokens))
    while tokens % nh:
        nh -= 1
    return nh, tokens // nh


class Case:
    """one descriptor of a census row"""

    def __init__(self, fields, seed=0, crossed=False, dyn=None):
        f = dict(fields)
        self.f, self.seed, self.crossed, self.dyn = f, int(seed), bool(crossed), dyn
        g = lambda k, dflt=0: f.get(k, dflt)
        self.M, self.N, self.K, self.batch = f["M"], f["N"], f["K"], max(g("batch", 1), 1)
        self.wdt = BF if g("wdtype") == BF16 else torch.float32
        self.adt = BF if g("a_bf16") else torch.float32
        self.loader, self.epi = g("loader"), g("epi")
        self.mode = g("f32x3") if self.wdt == torch.float32 else 0
        self.K1 = g("K1") if g("A2") else self.K
        self.ldw = g("ldw") or self.K
        self.splitk = max(g("splitk"), 1)
        self.odt = BF if (g("out_bf16") or (self.epi == EPI_ROPE_VT and self.wdt == BF)) else torch.float32
        # the extents the launch really uses when the count lives on the device (dyn_n): N of the score GEMM, K of the softmax loader
        self.Nx = dyn if (dyn is not None and self.loader != LOAD_SOFTMAX) else self.N
        self.Kx = dyn if (dyn is not None and self.loader == LOAD_SOFTMAX) else self.K
        assert not g("trace") and g("act") in (0, 1, 2)
        if g("ln_stats"):
            assert g("ln_C") == self.K == 32 * g("ln_nt") and g("ln_s")
        if self.loader == LOAD_SOFTMAX and g("a_packed"):
            raise NotImplementedError("softmax loader, probability form (fragment-order p~ with group scales)")
        if g("sm_stats_out") and g("out_packed"):
            raise NotImplementedError("score stage of the long-bank read (p~ with 64-key group statistics)")
        self.bufs = {}
        self._layout()

    # -- layout: extents by the header's rules, nothing allocated
    def _add(self, name, dtype, numel, out=False):
        self.bufs[name] = Spec(dtype, numel, out, SENT if out else math.nan)

    def _layout(self):
        f, M, N, K, G = self.f, self.M, self.N, self.K, self.batch
        g = lambda k, dflt=0: f.get(k, dflt)
        # A (+ A2)
        if self.loader == LOAD_CONV3X3:
            self.cB = M // (g("conv_OH") * g("conv_OW"))
            assert g("lda") == g("conv_C") and G == 1 and not g("a_packed")
            assert (g("conv_H") - 1) // g("conv_stride") + 1 == g("conv_OH") and (g("conv_W") - 1) // g("conv_stride") + 1 == g("conv_OW")
            self.strideA = self.cB * g("conv_H") * g("conv_W") * g("conv_C")
            self._add("A", self.adt, self.strideA)
        elif g("a_packed"):
            assert self.adt == self.wdt
            self.strideA = frag_numel(M, self.K1, self.adt) + frag_numel(1, self.K1, self.adt)
            self._add("A", self.adt, G * self.strideA)
            if g("A2"):
                self.strideA2 = frag_numel(M, K - self.K1, self.adt) + frag_numel(1, K - self.K1, self.adt)
                self._add("A2", self.adt, G * self.strideA2)
        else:
            self.lda = g("lda")
            assert self.lda >= (self.K1 if self.loader == LOAD_PLAIN else K)
            self.strideA = (M + 3) * self.lda
            self._add("A", self.adt, G * self.strideA)
            if g("A2"):
                self.lda2 = g("lda2")
                assert self.lda2 >= K - self.K1
                self.strideA2 = (M + 3) * self.lda2
                self._add("A2", self.adt, G * self.strideA2)
        # W
        wp = g("w_packed")
        if wp:
            self.strideW = frag_numel(N, self.ldw, self.wdt) + frag_numel(1, self.ldw, self.wdt)
        else:
            self.strideW = (N + 1) * self.ldw
        self._add("W", self.wdt, G * self.strideW)
        nb_ = N if self.epi != EPI_PIXSHUF else g("ps_C")
        self.sbias = (nb_ + 3) // 4 * 4 + 4
        if g("bias"):
            self._add("bias", torch.float32, G * self.sbias)
        if g("ln_stats"):
            self.sstats = M * g("ln_nt") * 2 + 8
            self._add("ln_stats", torch.float32, G * self.sstats)
            self._add("ln_s", torch.float32, G * self.sbias)
        rdt = BF if g("res_bf16") else torch.float32
        for i in (1, 2):
            if g("res%d" % i):
                if i == 2 and g("res2_up_H"):
                    self._add("res2", rdt, self.cB * g("res2_up_H") * g("res2_up_W") * N)
                else:
                    ld = g("ldr%d" % i)
                    assert ld >= N
                    self._add("res%d" % i, rdt, G * M * ld)          # header: [batch][M][ld]
        if self.loader == LOAD_SOFTMAX:
            assert g("sm_nt") == (K + 31) // 32 and G == 1
            self._add("sm_stats", torch.float32, M * g("sm_nt") * 2)
            if g("sm_zout"):
                self._add("sm_zout", torch.float32, M * 4, out=True)
        if g("dyn_n"):
            self._add("dyn_n", torch.int32, 4)
        # C
        if self.epi == EPI_ROPE_VT:
            rc, tok = g("rope_cols"), g("tokens")
            assert rc % 64 == 0 and N % 64 == 0 and M % tok == 0
            self.rB = M // tok
            if rc < N:
                assert g("heads") * 64 == N - rc and g("vt") and g("vt_ld") >= tok
                self.svt = self.rB * g("heads") * 64 * g("vt_ld") + 64
                self._add("vt", self.wdt, G * self.svt, out=True)
            if g("qkv_packed"):
                assert g("vt_ld") % 64 == 0
                self.strideC = frag_numel(self.rB * g("vt_ld"), rc, BF) + frag_numel(1, rc, BF)
            else:
                assert g("ldc") >= rc
                self.strideC = (M + 2) * g("ldc")
            self._add("C", self.wdt, G * self.strideC, out=True)
            self._add("pos", torch.int32, M * 2)
            self._add("rope_cos", torch.float32, ROPE_MAX_POS * 16)
            self._add("rope_sin", torch.float32, ROPE_MAX_POS * 16)
        elif self.epi == EPI_PIXSHUF:
            ks, pc = g("ps_k"), g("ps_C")
            assert N == ks * ks * pc and M % (g("ps_H") * g("ps_W")) == 0 and G == 1
            self.pB = M // (g("ps_H") * g("ps_W"))
            self.strideC = self.pB * ks * g("ps_H") * ks * g("ps_W") * pc
            self._add("C", self.odt, self.strideC, out=True)
        elif self.epi == EPI_PARTIAL:
            assert G == 1 and g("ldc") >= N
            self.strideC = self.splitk * M * g("ldc")
            self._add("C", torch.float32, self.strideC, out=True)
        elif g("out_packed"):
            self.strideC = frag_numel(M, N, self.odt) + frag_numel(1, N, self.odt)
            self._add("C", self.odt, G * self.strideC, out=True)
        else:
            assert g("ldc") >= N
            self.strideC = (M + 2) * g("ldc")
            self._add("C", self.odt, G * self.strideC, out=True)
        if g("c2"):
            assert N % 32 == 0
            self.sc2 = frag_numel(M, N, self.wdt) + frag_numel(1, N, self.wdt)
            self._add("c2", self.wdt, G * self.sc2, out=True)
        if g("stats_out"):
            self.sso = M * (N // 32) * 2 + 8
            self._add("stats_out", torch.float32, G * self.sso, out=True)
        if g("sm_stats_out"):
            assert G == 1
            self._add("sm_stats_out", torch.float32, M * ((N + 31) // 32) * 2, out=True)

    def nbytes(self):
        return sum((s.numel + 2 * GUARD) * torch.empty(0, dtype=s.dtype).element_size() for s in self.bufs.values())

    def slot(self, z):
        """storage slot of the tokens / statistics problem z reads (crossed: the other side's)"""
        return self.batch - 1 - z if self.crossed else z

    # -- allocation and content
    def materialize(self, device):
        f, M, N, K, G = self.f, self.M, self.N, self.K, self.batch
        g = lambda k, dflt=0: f.get(k, dflt)
        self.device = device
        gen = torch.Generator(device=device).manual_seed(1000 + self.seed)
        rnd = lambda *shape: torch.rand(*shape, generator=gen, device=device) * 2 - 1
        for s in self.bufs.values():
            s.t = torch.full((s.numel + 2 * GUARD,), s.fill if s.dtype.is_floating_point else 0, dtype=s.dtype, device=device)
        B = self.bufs
        self.A_eff, self.W_eff, self.x_ln = [], [], []
        round_a = (lambda t: bf(t)) if (self.wdt == BF or self.mode == 2) else (lambda t: t)
        for z in range(G):
            # ---- A: asymmetric content (a ramp down the rows), distinct per problem
            if self.loader == LOAD_CONV3X3:
                x = rnd(self.cB, g("conv_H"), g("conv_W"), g("conv_C"))
                x[..., 0] += torch.arange(g("conv_W"), device=device)[None, None, :] * 0.02
                x = x.to(self.adt)
                B["A"].body.copy_(x.reshape(-1))
                xe = x.float().clamp_min(0) if g("relu_in") else x.float()
                self.A_eff.append(conv_rows(round_a(xe), g("conv_OH"), g("conv_OW"), g("conv_stride")))
                continue
            ramp = torch.arange(M, device=device) / float(M)
            if self.loader == LOAD_SOFTMAX:
                a = rnd(M, K) * 2.0
                a[:, 0] += ramp
                a = self._clear_of_threshold(a)
            else:
                a = rnd(M, K) * (2.0 if g("ln_stats") else 1.0) + (0.2 if g("ln_stats") else 0.0)
                a[:, 0] += ramp * 3.0
            if g("ln_stats"):
                self.x_ln.append(a.clone())                         # the fp32 stream whose partials the producer wrote
            a = a.to(self.adt)
            sl = self.slot(z)
            parts = ((a[:, :self.K1], "A", self.strideA), (a[:, self.K1:], "A2", self.strideA2)) if g("A2") else ((a, "A", self.strideA),)
            for part, name, stride in parts:
                dst = B[name].body[sl * stride:(sl + 1) * stride]
                if g("a_packed"):
                    pk = frag_pack(part, self.adt)
                    dst[:pk.numel()].copy_(pk)
                else:
                    ld = self.lda if name == "A" else self.lda2
                    dst.view(M + 3, ld)[:M, :part.shape[1]].copy_(part)
                    if self.loader == LOAD_SOFTMAX and self.Kx < K:
                        dst.view(M + 3, ld)[:M, self.Kx:K] = math.nan        # scores past the extent on the device are never used
            ae = a.float().clamp_min(0) if g("relu_in") else a.float()
            self.A_eff.append(ae if self.loader == LOAD_SOFTMAX else round_a(ae))
        for z in range(G):
            # ---- W
            w = rnd(N, K) * (0.05 if self.loader != LOAD_SOFTMAX else 1.0)
            w[:, 1 % K] += torch.arange(N, device=device) * (0.02 / max(N / 1024.0, 1.0)) * (0.05 if self.loader != LOAD_SOFTMAX else 1.0)
            dst = B["W"].body[z * self.strideW:(z + 1) * self.strideW]
            if g("w_packed") == 2:
                pk = planes_pack(w)
                dst[:pk.numel()].copy_(pk)
                self.W_eff.append(planes_unpack(pk, N, K))
            elif g("w_packed"):
                w = w.to(self.wdt)
                slack = W_SLACK if self.loader == LOAD_SOFTMAX else 0.0
                pk = frag_pack(w, self.wdt, self.ldw, slack)
                dst[:pk.numel()].copy_(pk)
                self.W_eff.append(round_a(w.float()))
            else:
                w = w.to(self.wdt)
                dst.view(N + 1, self.ldw)[:N, :K].copy_(w)
                self.W_eff.append(round_a(w.float()))
        nb_ = N if self.epi != EPI_PIXSHUF else g("ps_C")
        self.bias = rnd(G, nb_) if g("bias") else None
        if g("bias"):
            B["bias"].body.view(G, self.sbias)[:, :nb_].copy_(self.bias)
        if g("ln_stats"):
            C_ = g("ln_C")
            self.ln_s = torch.stack([self.W_eff[z].sum(1).float() for z in range(G)])
            B["ln_s"].body.view(G, self.sbias)[:, :N].copy_(self.ln_s)
            self.ln_st = []
            for z in range(G):
                xd = self.x_ln[z].double().view(M, C_ // 32, 32)
                st = torch.stack((xd.sum(-1), (xd * xd).sum(-1)), -1).float()
                B["ln_stats"].body[self.slot(z) * self.sstats:][:st.numel()].copy_(st.reshape(-1))
                self.ln_st.append(st)
        rdt = BF if g("res_bf16") else torch.float32
        self.res = {}
        for i in (1, 2):
            if not g("res%d" % i):
                continue
            if i == 2 and g("res2_up_H"):
                r = (rnd(self.cB, g("res2_up_H"), g("res2_up_W"), N) * 2 + 0.3).to(rdt)
                B["res2"].body.copy_(r.reshape(-1))
                up = upsample2x(r.double(), g("conv_OH"), g("conv_OW"))
                self.res[2] = bf(up.float()).double().reshape(1, M, N)          # rounded to the map dtype as the stored map would be
                # the kernel interpolates in fp32 and then rounds: where the float64 value lies within the fp32 interpolation bound of a
                # bf16 rounding boundary its residual may be either neighbour.  res2_alt: what to add to expected() for the other
                # candidates (zero on every one-candidate element); res2_two: the share of two-candidate elements
                import conv_ref
                lo, hi, two = conv_ref.bf16_candidates(up, conv_ref.upsample_bound(r, g("conv_OH"), g("conv_OW")))
                self.res2_alt = [(c.double().reshape(1, M, N) - self.res[2]) for c in (lo, hi)]
                self.res2_two = float(two.float().mean())
            else:
                ld = g("ldr%d" % i)
                r = (rnd(G, M, N) * 2 + 0.3 * i).to(rdt)
                B["res%d" % i].body.view(G, M, ld)[:, :, :N].copy_(r)
                self.res[i] = r.double()
        if self.loader == LOAD_SOFTMAX:
            st = group_softmax_stats(self.A_eff[0][:, :self.Kx].double()).float()         # [M, ceil(Kx/32), 2], compact for the extent in use
            B["sm_stats"].body[:st.numel()].copy_(st.reshape(-1))
        if g("dyn_n"):
            B["dyn_n"].body.copy_(torch.tensor([self.dyn if self.dyn is not None else (N if self.loader != LOAD_SOFTMAX else K), 0, 0, 0], dtype=torch.int32))
        if self.epi == EPI_ROPE_VT:
            nh, nw = _grid(g("tokens"))
            ys, xs = torch.meshgrid(torch.arange(nh), torch.arange(nw), indexing="ij")
            self.pos = torch.stack((ys.reshape(-1), xs.reshape(-1)), -1).repeat(self.rB, 1).to(torch.int32).to(device)
            assert int(self.pos.max()) < ROPE_MAX_POS
            self.cos, self.sin = rope_tables(device)
            B["pos"].body.copy_(self.pos.reshape(-1))
            B["rope_cos"].body.copy_(self.cos.reshape(-1))
            B["rope_sin"].body.copy_(self.sin.reshape(-1))
        return self

    def _clear_of_threshold(self, a):
        """scores whose probability would sit within 0.2 % of the threshold are moved away from it (a flip there is not an error)"""
        for _ in range(3):
            p = torch.softmax(a[:, :self.Kx].double(), -1)
            near = ((p - SM_THRESH).abs() < 2e-3 * SM_THRESH)
            if not bool(near.any()):
                break
            a[:, :self.Kx] -= near.float() * 0.02
        return a

    # -- the descriptor
    def desc(self, lib):
        f, G, B = self.f, self.batch, self.bufs
        g = lambda k, dflt=0: f.get(k, dflt)
        ptrs = {n for n, t in lib.GemmDesc._fields_ if t is C.c_void_p}
        d = lib.GemmDesc()
        for k, v in f.items():
            if k not in ptrs:
                setattr(d, k, v)
        d.tile = -1
        es = lambda dt: torch.empty(0, dtype=dt).element_size()
        d.A = B["A"].ptr(self.strideA * (G - 1) if self.crossed else 0)
        d.strideA = -self.strideA if self.crossed else self.strideA
        if g("A2"):
            d.A2, d.sb_A2 = B["A2"].ptr(), self.strideA2 * es(self.adt)
        d.W, d.strideW = B["W"].ptr(), self.strideW
        d.C, d.strideC = B["C"].ptr(), self.strideC
        if g("bias"):
            d.bias, d.sb_bias = B["bias"].ptr(), self.sbias * 4
        if g("ln_stats"):
            d.ln_stats = B["ln_stats"].ptr(self.sstats * (G - 1) if self.crossed else 0)
            d.sb_ln_stats = (-self.sstats if self.crossed else self.sstats) * 4
            d.ln_s, d.sb_ln_s, d.ln_eps = B["ln_s"].ptr(), self.sbias * 4, LN_EPS
        for n in ("res1", "res2", "sm_stats", "sm_zout", "sm_stats_out", "dyn_n", "pos", "rope_cos", "rope_sin"):
            if g(n):
                src = self.rope_from.bufs if (n in ("pos", "rope_cos", "rope_sin") and getattr(self, "rope_from", None) is not None) else B
                setattr(d, n, src[n].ptr())
        if self.loader == LOAD_SOFTMAX:
            d.sm_thresh = SM_THRESH
        if g("vt"):
            d.vt, d.sb_vt = B["vt"].ptr(), self.svt * es(self.wdt)
        if g("c2"):
            d.c2, d.sb_c2 = B["c2"].ptr(), self.sc2 * es(self.wdt)
        if g("stats_out"):
            d.stats_out, d.sb_stats_out = B["stats_out"].ptr(), self.sso * 4
        return d

    # -- what the outputs must be: name -> [per problem float64 tensors]; 'C' already in its logical shape
    def expected(self):
        f, M, G = self.f, self.M, self.batch
        N, K = self.Nx, self.Kx
        g = lambda k, dflt=0: f.get(k, dflt)
        out = {"C": []}
        for z in range(G):
            A, W = self.A_eff[z].double()[:, :K], self.W_eff[z].double()[:N, :K]
            if self.loader == LOAD_SOFTMAX:
                p, mass, mx, Z = softmax_keep(A, SM_THRESH)
                pe = bf(p.float()).double() if self.wdt == BF else p
                y = (pe @ W.T) / mass[:, None]
                out["sm_zout"] = [torch.stack((mass, mx, 1.0 / Z), 1)]
            else:
                y = (A @ W.T) * float(g("alpha", 1.0))
            if self.epi == EPI_PARTIAL:
                KB = frag_geometry(self.wdt)[0]
                nkb = (K + KB - 1) // KB
                per = (nkb + self.splitk - 1) // self.splitk
                parts = [(A[:, s * per * KB:(s + 1) * per * KB] @ W[:, s * per * KB:(s + 1) * per * KB].T) * float(g("alpha", 1.0)) for s in range(self.splitk)]
                out["C"].append(torch.stack(parts))
                continue
            if g("ln_stats"):
                y = ln_fold_apply(y, self.ln_st[z], g("ln_C"), LN_EPS, self.ln_s[z][:N])
            if self.bias is not None:
                b = self.bias[z].double()
                y = y + (b.repeat(N // b.numel())[None] if self.epi == EPI_PIXSHUF else b[None, :N])
            if g("act") == 1:
                y = gelu(y)
            elif g("act") == 2:
                y = y.clamp_min(0)
            for i in (1, 2):
                if i in self.res:
                    y = y + self.res[i][z][:, :N]
            if self.epi == EPI_ROPE_VT:
                rc = g("rope_cols")
                qk = rope_cols_apply(y[:, :rc], self.pos, self.cos, self.sin)
                out["C"].append(qk)
                if rc < N:
                    out.setdefault("vt", []).append(y[:, rc:].reshape(self.rB, g("tokens"), g("heads"), 64))
            elif self.epi == EPI_PIXSHUF:
                out["C"].append(pixshuf_scatter(y, self.pB, g("ps_H"), g("ps_W"), g("ps_k"), g("ps_C")))
            else:
                out["C"].append(y)
        return out

    # -- what the launch left: same keys / shapes as expected(), plus the derived outputs checked against C itself
    def got(self):
        f, M, G, B = self.f, self.M, self.batch, self.bufs
        N = self.Nx
        g = lambda k, dflt=0: f.get(k, dflt)
        res = {"C": []}
        for z in range(G):
            c = B["C"].body[z * self.strideC:(z + 1) * self.strideC]
            if self.epi == EPI_ROPE_VT:
                rc, tok = g("rope_cols"), g("tokens")
                if g("qkv_packed"):
                    dense = frag_unpack(c, self.rB * g("vt_ld"), rc, BF).view(self.rB, g("vt_ld"), rc)
                    res["C"].append(dense[:, :tok].reshape(M, rc))
                else:
                    res["C"].append(c.view(M + 2, g("ldc"))[:M, :rc])
                if rc < self.N:
                    v = B["vt"].body[z * self.svt:(z + 1) * self.svt]
                    if g("qkv_packed"):
                        res.setdefault("vt", []).append(v[pv_offsets(self.rB, g("heads"), tok, g("vt_ld"), v.device)])
                    else:
                        res.setdefault("vt", []).append(v[:self.svt - 64].view(self.rB, g("heads"), 64, g("vt_ld"))[..., :tok].permute(0, 3, 1, 2))
            elif self.epi == EPI_PIXSHUF:
                res["C"].append(c.view(self.pB, g("ps_k") * g("ps_H"), g("ps_k") * g("ps_W"), g("ps_C")))
            elif self.epi == EPI_PARTIAL:
                res["C"].append(c.view(self.splitk, M, g("ldc"))[:, :, :N])
            elif g("out_packed"):
                res["C"].append(frag_unpack(c, M, N, self.odt))
            else:
                res["C"].append(c.view(M + 2, g("ldc"))[:M, :N])
            if g("c2"):
                res.setdefault("c2", []).append(frag_unpack(B["c2"].body[z * self.sc2:(z + 1) * self.sc2], M, N, self.wdt))
            if g("stats_out"):
                res.setdefault("stats_out", []).append(B["stats_out"].body[z * self.sso:][:M * (N // 32) * 2].view(M, N // 32, 2))
        if g("sm_stats_out"):
            nt = (N + 31) // 32
            res["sm_stats_out"] = [B["sm_stats_out"].body[:M * nt * 2].view(M, nt, 2)]
        if g("sm_zout"):
            res["sm_zout"] = [B["sm_zout"].body.view(M, 4)[:, :3]]
        return res

    def sentinel_faults(self):
        """names of outputs with a write where none may land: guard bands, pad columns / rows of row-major C, columns past a device-side extent"""
        bad = [n for n, s in self.bufs.items() if not s.guards_intact()]
        f, M, G, B = self.f, self.M, self.batch, self.bufs
        g = lambda k, dflt=0: f.get(k, dflt)
        row_major = (self.epi == EPI_PLAIN and not g("out_packed")) or (self.epi == EPI_ROPE_VT and not g("qkv_packed"))
        if row_major:
            ncol = g("rope_cols") if self.epi == EPI_ROPE_VT else self.Nx
            for z in range(G):
                c = B["C"].body[z * self.strideC:(z + 1) * self.strideC].view(M + 2, g("ldc"))
                if not (bool((c[:, ncol:] == SENT).all()) and bool((c[M:] == SENT).all())):
                    bad.append("C[%d] pad" % z)
        if self.epi == EPI_PARTIAL:
            c = B["C"].body.view(self.splitk, M, g("ldc"))
            if not bool((c[:, :, self.N:] == SENT).all()):
                bad.append("C pad")
        # padding INSIDE a layout: untouched or zero (the header prescribes zero padding for the consumers of a fragment-order operand)
        clean = lambda t: bool(((t == SENT) | (t == 0)).all())
        for z in range(G):
            packed = []
            if self.epi == EPI_PLAIN and g("out_packed"):
                packed.append(("C", B["C"].body[z * self.strideC:], M, M, self.N, self.odt))
            if g("c2"):
                packed.append(("c2", B["c2"].body[z * self.sc2:], M, M, self.N, self.wdt))
            if self.epi == EPI_ROPE_VT and g("qkv_packed"):
                packed.append(("C", B["C"].body[z * self.strideC:], self.rB * g("vt_ld"), None, g("rope_cols"), BF))
            for name, flat, rows, live_rows, cols, dt in packed:
                KB = frag_geometry(dt)[0]
                rp, cp = (rows + 15) // 16 * 16, (cols + KB - 1) // KB * KB
                full = frag_unpack(flat[:rp * cp], rp, cp, dt)
                if live_rows is None:                              # q / k rows padded per image to vt_ld tokens
                    pad = full[:rows].view(self.rB, g("vt_ld"), cp)[:, g("tokens"):]
                    ok = clean(pad) and clean(full[rows:]) and clean(full[:, cols:])
                else:
                    ok = clean(full[live_rows:]) and clean(full[:, (self.Nx if name == "C" else cols):])
                if not ok:
                    bad.append("%s[%d] padding inside the fragment order" % (name, z))
            if g("vt") and self.epi == EPI_ROPE_VT:
                v = B["vt"].body[z * self.svt:(z + 1) * self.svt - 64]
                if g("qkv_packed"):
                    live = torch.zeros(v.numel(), dtype=torch.bool, device=v.device)
                    live[pv_offsets(self.rB, g("heads"), g("tokens"), g("vt_ld"), v.device).reshape(-1)] = True
                    ok = clean(v[~live])
                else:
                    ok = clean(v.view(-1, g("vt_ld"))[:, g("tokens"):])
                if not ok:
                    bad.append("vt[%d] padding past the tokens" % z)
        if g("sm_stats_out"):
            used = M * ((self.Nx + 31) // 32) * 2
            if not bool((B["sm_stats_out"].body[used:] == SENT).all()):
                bad.append("sm_stats_out past the extent in use")
        for n in ("vt", "c2", "stats_out"):
            if g(n):
                stride, used = {"vt": (getattr(self, "svt", 0), 64), "c2": (getattr(self, "sc2", 0), frag_numel(1, self.N, self.wdt)),
                                "stats_out": (getattr(self, "sso", 0), 8)}[n]
                for z in range(G):
                    if not bool((B[n].body[(z + 1) * stride - used:(z + 1) * stride] == SENT).all()):
                        bad.append("%s[%d] slack" % (n, z))
        return bad


# ----------------------------------------------------------------------------- rows of the table
def row_cases(row, line, dyn=None):
    """the Cases of one census row.  The second descriptor of a lean q/k/v pair is the cross-attention k/v projection: crossed."""
    ds = row["descs"]
    pair = len(ds) == 2 and all(d.get("epi") == EPI_ROPE_VT and d.get("batch", 1) == 2 and d.get("ln_stats") for d in ds)
    cases = [Case(d, seed=line * 8 + i, crossed=(pair and i == 1 and d["N"] == 2 * d.get("rope_cols", 0)), dyn=dyn) for i, d in enumerate(ds)]
    if pair:
        cases[1].rope_from = cases[0]          # positions and RoPE tables are shared by the two descriptors of a q/k/v pair (same tokens)
    return cases


def dyn_extents(row):
    """the extents a dyn_n row runs at: the bound, a mid value (multiple of 4) and the smallest the instance accepts"""
    d = row["descs"][0]
    if not d.get("dyn_n"):
        return [None]
    bound = d["K"] if d.get("loader") == LOAD_SOFTMAX else d["N"]
    return [bound, (bound // 2 + 36) // 4 * 4, 4]


def tolerance(case, name):
    """max-norm relative bounds, against the UNROUNDED float64 reference, of the existing tests of the same family"""
    if case.loader == LOAD_SOFTMAX:
        return 6e-3 if case.wdt == BF else 2e-3                                        # test_two_launch_memory_read
    if name in ("C", "vt") and case.epi == EPI_ROPE_VT and case.wdt == BF:
        return 8e-3                                                                    # test_proj_rope_vt
    if name == "C" and case.odt == BF:
        return 4e-3                                                                    # test_lean_packed_fc1, test_lean_conv3x3_small_maps
    return 2e-5                                                                        # fp32 accumulate on rounded operands


ZOUT_BOUNDS = (("kept mass", 1e-5), ("row max", 1e-6), ("1/Z", 1e-5))      # test_two_launch_memory_read's columns; the mass is tighter here
                                                                          # because the builder keeps every probability clear of the threshold


def bf16_excess_map(got, ref, width=32):
    """a bf16-stored output against the unrounded reference, element by element: a correctly rounded store of an fp32-accumulated value
    lies within half a bf16 step of the reference plus 2e-5 of its 32-column group's largest value.  Returns |got - ref| / bound per
    element (pass: <= 1), so small elements are held as tightly as large ones."""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    n = ref.shape[1]
    nt = (n + width - 1) // width
    gmax = torch.nn.functional.pad(ref.abs(), (0, nt * width - n)).view(-1, nt, width).amax((0, 2))
    slack = 2e-5 * gmax.repeat_interleave(width)[:n][None]
    mag = (ref.abs() + slack).clamp_min(1e-38)
    half_step = torch.exp2(torch.floor(torch.log2(mag)) - 8)
    return (got - ref).abs() / (half_step + slack)


def bf16_excess(got, ref, width=32):
    """the worst element of bf16_excess_map"""
    return float(bf16_excess_map(got, ref, width).max())


def conv_bf16_excess(case, z, got, ref):
    """bf16_excess of a convolution output; with a half-resolution res2 every element takes the smaller error over the candidates of its
    upsampled residual (Case.res2_alt)"""
    ex = bf16_excess_map(got, ref)
    for alt in getattr(case, "res2_alt", ()):
        ex = torch.minimum(ex, bf16_excess_map(got, ref + alt[z]))
    return float(ex.max())


def block_errors(got, ref, width=32):
    """max |got - ref| / max |ref| per 32-column group of the last dim (ragged tail included) -> worst over the groups, and overall"""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    n = ref.shape[1]
    nt = (n + width - 1) // width
    padn = nt * width - n
    diff = torch.nn.functional.pad((got - ref).abs(), (0, padn)).view(-1, nt, width).amax((0, 2))
    mag = torch.nn.functional.pad(ref.abs(), (0, padn)).view(-1, nt, width).amax((0, 2))
    return float((diff / mag.clamp_min(1e-30)).max()), float(diff.max() / mag.max().clamp_min(1e-30))


def compare(case):
    """every output of a launched Case against expected(): list of failure strings (empty = pass), and the errors by output kind"""
    exp, got = case.expected(), case.got()
    fails, errs = [], {}

    def note(kind, v):
        errs[kind] = max(errs.get(kind, 0.0), v)
    for z in range(case.batch):
        cg = got["C"][z]
        for name in exp:
            if z >= len(exp[name]):
                continue
            e, o = exp[name][z], got[name][z]
            if torch.isnan(o.float()).any():
                fails.append("%s[%d]: NaN" % (name, z))
                continue
            if name == "sm_zout":                                 # three different quantities: each column by its own bound
                for j, (what, tol) in enumerate(ZOUT_BOUNDS):
                    e_ = float((o[:, j].double() - e[:, j]).abs().max() / e[:, j].abs().max())
                    note("sm_zout " + what, e_)
                    if not e_ < tol:
                        fails.append("sm_zout %s: %.3e (bound %.1e)" % (what, e_, tol))
                continue
            blk, allv = block_errors(o, e)
            tol = tolerance(case, name)
            note(name, blk)
            if not (blk < tol and allv < tol):
                fails.append("%s[%d]: per 32-column group %.3e, whole %.3e (bound %.1e)" % (name, z, blk, allv, tol))
            if o.dtype == BF and case.loader == LOAD_CONV3X3 and name == "C":
                # asserted.  Five small-map rows with a half-resolution res2 (table lines 21, 25, 45, 75, 183; tiles 40 / 41) used to sit
                # 7 .. 49 x outside this bound.  The cause was in this reference, not in the kernel: conv_sm_body adds r1 + r2 in fp32 and
                # rounds once at the store, but it interpolates the half-resolution residual in fp32 and rounds THAT to bf16 (bit-equal to
                # sp3_upsample2x_bf16 into memory), where the reference interpolated in float64 and rounded -- a fraction of a per cent of
                # the elements land on the other bf16 neighbour, a whole step of the residual (tests/test_conv_ref_cpu.py reproduces it).
                # Such elements now have two candidates: conv_bf16_excess.
                ex = conv_bf16_excess(case, z, o, e)
                note(name + " bf16 steps", ex)
                if not ex <= 1.0:
                    fails.append("%s[%d]: %.2f x the elementwise bf16 bound" % (name, z, ex))
            elif o.dtype == BF and case.loader != LOAD_SOFTMAX:
                note(name + " bf16 steps", bf16_excess(o, e))                     # reported (SP3_CENSUS_REPORT), not asserted
        # outputs derived from the finished C: the fragment-order copy bit for bit, the statistics from the stored values
        cf = cg.double()
        if "c2" in got and not torch.equal(got["c2"][z], cg.to(case.wdt)):
            fails.append("c2[%d] is not C in the MFMA dtype" % z)
        if "stats_out" in got:
            Mr, Nn = cf.shape
            want = torch.stack((cf.reshape(Mr, Nn // 32, 32).sum(-1), (cf * cf).reshape(Mr, Nn // 32, 32).sum(-1)), -1)
            for j, nm in enumerate(("sum", "sumsq")):             # per statistic and per 32-column group
                e_ = float(((got["stats_out"][z][..., j].double() - want[..., j]).abs().amax(0) / want[..., j].abs().amax(0).clamp_min(1e-30)).max())
                note("stats_out", e_)
                if not e_ < 1e-5:
                    fails.append("stats_out[%d] %s: %.3e" % (z, nm, e_))
        if "sm_stats_out" in got:
            want = group_softmax_stats(cf)
            so = got["sm_stats_out"][z].double()
            e0 = float(((so[..., 0] - want[..., 0]).abs().amax(0) / want[..., 0].abs().amax(0).clamp_min(1e-30)).max())
            e1 = float(((so[..., 1] - want[..., 1]).abs().amax(0) / want[..., 1].abs().amax(0).clamp_min(1e-30)).max())
            note("sm_stats_out", max(e0, e1))
            if not (e0 < 1e-6 and e1 < 1e-5):
                fails.append("sm_stats_out: max %.3e, sum exp %.3e" % (e0, e1))
    if hasattr(case, "res2_two"):
        errs["res2_up two-candidate share"] = case.res2_two
        if not case.res2_two <= 0.01:
            fails.append("res2_up: %.4f of the elements have two candidates (cap 1 %%)" % case.res2_two)
    fails += ["sentinel: " + s for s in case.sentinel_faults()]
    return fails, errs
