/*
 * spann3r_hip.h -- C-ABI of libspann3r_hip.so: the MI355X (gfx950) hot-path kernels of
 * Spann3R's per-frame forward.
 *
 * The reference is Python on PyTorch; its ONLY native FFI is the `curope` extension
 * (`rope_2d`, croco/models/curope/curope.cpp:49-69).  Everything else on the hot path is an
 * ATen op reached through nn.Module.forward.  This header therefore declares
 *   (1) `sp3_rope_2d`   -- the drop-in for the curope FFI, and
 *   (2) one entry point per ATen-level operator the reference's hot path calls, each citing the
 *       reference call site(s) it replaces.
 * A maintainer binds these with ctypes; spann3r_amd/lib.py is that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`
 *   - `stream` is a hipStream_t passed as void* (use the caller's CURRENT stream; the reference's
 *     curope launches on stream 0, kernels.cu:102 -- a latent bug we do not reproduce)
 *   - return value: 0 on success, non-zero error code otherwise; `sp3_last_error()` gives the text
 *     (the Python binding raises RuntimeError, matching TORCH_CHECK -> RuntimeError)
 *   - activations are fp32 in memory; `wdtype` selects the MFMA arithmetic:
 *       SP3_F32  : v_mfma_f32_16x16x4_f32  (exact fp32; the <=1e-3 parity mode)
 *       SP3_BF16 : v_mfma_f32_16x16x32_bf16 (bf16 operands, fp32 accumulate; the bench mode)
 *   - no function allocates, frees or synchronises: all of them are hipGraph-capturable
 */
#ifndef SPANN3R_HIP_H
#define SPANN3R_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SP3_F32 = 0, SP3_BF16 = 1 };
/* sp3_attention's further operand codes: fp32 operands in memory, every product through three MFMAs of a two-way split */
enum { SP3_ATTN_F32X3 = 2, SP3_ATTN_F16X3 = 3 };
enum { SP3_ACT_NONE = 0, SP3_ACT_GELU = 1, SP3_ACT_RELU = 2 };
enum { SP3_EPI_PLAIN = 0, SP3_EPI_ROPE_VT = 1, SP3_EPI_PIXSHUF = 2, SP3_EPI_PARTIAL = 3 };
enum { SP3_LOAD_PLAIN = 0, SP3_LOAD_CONV3X3 = 1, SP3_LOAD_SOFTMAX = 2 };

const char* sp3_last_error(void);
int sp3_version(void);

/* Cache policy of the per-frame chain's once-read weight loads (process-wide):
 *   0  every load uses the default policy
 *   1  the library's table decides per kernel family and instance (the default)
 *   2  every family that has a streaming variant streams (non-temporal weight loads): lean 196-row GEMMs, small-map and wide
 *      3x3 convolutions, the q-projection attention
 * Results are bit-identical under every mode; only the cache behaviour of the weight loads changes.  The mode is read at launch
 * time (a captured graph keeps what it captured: set it before the first forward) and never changes what sp3_gemm_plan answers.
 * Initialised from the environment variable SP3_W_STREAM (0 / 1 / 2).  sp3_weight_stream_set returns 0, or 1 for an unknown mode. */
int sp3_weight_stream_set(int mode);
int sp3_weight_stream_get(void);

/* ------------------------------------------------------------------------------------------
 * sp3_gemm : C = epilogue( alpha * A[M,K] . W[N,K]^T )
 * Replaces every nn.Linear / 1x1 Conv2d / 3x3 Conv2d / ConvTranspose2d(k==stride) / einsum on the
 * path: croco/models/blocks.py:74-77,97,110,154-156,167 ; dust3r/model.py:190-191 ;
 * spann3r/model.py:154,174,301,309 ; croco/models/dpt_block.py:33-75,95-113,180-188,318-324,
 * 356-410 ; dust3r/patch_embed.py:24 (after sp3_im2col_patch).
 * A is fp32 [M, lda]; W is [N, K] in `wdtype`; bias fp32 [N].
 * loader CONV3X3: A is an NHWC fp32 map [batchless B*H*W, Cin]; row m = output pixel, K = 9*Cin
 *                 ordered (tap, ci); pad 1; stride conv_stride.
 * epilogue ROPE_VT (fused qkv / kv / q projection of an attention layer): columns
 *   [0, rope_cols) get bias then 2-D RoPE (tables + per-row int32 (y,x) positions) and are stored
 *   row-major to C (ldc) in `wdtype`; columns >= rope_cols are V: stored transposed per head to
 *   vt[((b*heads + h)*64 + d) * vt_ld + n] in `wdtype` (head_dim is 64 on this path).
 * epilogue PIXSHUF: N = ks*ks*Cout, ConvTranspose2d(k=s=ks) scatter into NHWC [B, ks*H, ks*W, Cout].
 * epilogue PARTIAL: K is split over `splitk` workgroups (grid.z); slice z stores its raw fp32 partial sums to
 *   C + z*M*ldc (no bias/activation); sp3_reduce_ln finishes the op (bias + residual + LayerNorm(s)).
 * a_bf16: A (and A2) hold bf16 instead of fp32 (bf16 mode keeps GEMM inputs in bf16: same numerics as converting
 *   on load, half the L2 traffic).  Requires wdtype == SP3_BF16.
 */
typedef struct sp3_gemm_desc {
  const float* A;
  const float* A2;        /* optional second A source for k >= K1 (torch.cat(..., dim=-1) without the copy:
                             spann3r/model.py:300); K1 % 64 == 0; A2 row stride lda2 */
  const void* W;
  void* C;
  const float* bias;
  const float* res1;      /* optional residuals, added after activation: C += res1 (+ res2) */
  const float* res2;
  int32_t M, N, K;
  int32_t batch;          /* grid.y; strides below in elements */
  int32_t K1;             /* k < K1 reads A, k >= K1 reads A2 (set K1 = K when A2 is null) */
  int64_t lda, lda2, ldw, ldc, ldr1, ldr2;   /* ldw: W row stride (>= K) */
  int64_t strideA, strideW, strideC;
  float alpha;
  int32_t wdtype;         /* SP3_F32 | SP3_BF16 : dtype of W and of the MFMA */
  int32_t act;            /* SP3_ACT_* applied after bias */
  int32_t out_bf16;       /* plain epilogue: store C as bf16 instead of fp32 */
  int32_t relu_in;        /* apply ReLU to A on load (ResidualConvUnit pre-activation) */
  int32_t loader;         /* SP3_LOAD_* */
  int32_t conv_H, conv_W, conv_C, conv_OH, conv_OW, conv_stride;
  int32_t epi;            /* SP3_EPI_* */
  const float* rope_cos;  /* [max_pos, 16] */
  const float* rope_sin;
  const int32_t* pos;     /* [M, 2] (y, x) */
  int32_t rope_cols;
  void* vt;
  int32_t tokens;         /* rows per image (N tokens): b = m / tokens, n = m % tokens */
  int32_t heads;
  int64_t vt_ld;
  int32_t ps_k, ps_H, ps_W, ps_C;
  int32_t tile;           /* -1 auto (sp3_gemm_plan tells which); 30..: lean small-M instances (sp3_gemm_plan); the general tiles, all there are:
                             0: 32x32 (K over 4 waves); 1: 64x64; 2: 64x128; 3: 64x64 (K over 4 waves) -- operands from a register ring;
                             5 / 6: 128x128 / 128x64 with both operands staged through LDS (fragment-order A and W in the MFMA
                             dtype, whole k-blocks); 13: 112x64, weights in a register ring, loader waves stage A (bf16 only);
                             20 / 21 / 22 / 24 / 25: 256x128 / 128x128 / 128x64 / 64x32 / 32x32 with the LDS ring pipelined (operands
                             as for 5 / 6).  Any other number below 30 is an error. */
  int32_t a_bf16;
  int32_t splitk;         /* >= 1; > 1 only with SP3_EPI_PARTIAL */
  int32_t a_packed;       /* A is in MFMA-fragment order [ceil(M/16)][ceil(K/KB)][2 halves][64 lanes][CH/2] (see w_packed); written
                             that way by the producing kernel (out_packed options), plain loader only */
  /* --- LayerNorm folded into the GEMM (DESIGN.md "LN fold"): for y = LayerNorm(x; gamma, beta) . W^T + b,
   *   y = rstd * (x . (gamma (.) W)^T) - rstd * mean * s + (b + beta . W^T),  s_n = sum_k (gamma (.) W)_nk.
   * CONSUMER side: A is the raw stream x (packed), W is gamma (.) W, bias is the folded bias, ln_s = s, and the row
   * statistics come from ln_stats[M][ln_nt][2] = per-32-column partial (sum, sum of squares) of x written by the
   * PRODUCER of x; mean/rstd are finished per output tile.  PRODUCER side (plain epilogue): stats_out receives those
   * partials of the rows this launch finalises (N % 32 == 0) and c2 a second, fragment-order copy of C in the MFMA
   * dtype (the consumers' A operand).  Replaces the norm1/norm2/norm3/norm_y/value_norm launches
   * (croco/models/blocks.py:128-129,187-190, spann3r/model.py:308). */
  const float* ln_stats;
  const float* ln_s;
  int32_t ln_nt;          /* number of 32-column groups of x = C_x / 32 */
  int32_t ln_C;           /* C_x */
  float ln_eps;
  float* stats_out;       /* [M][N/32][2] or null */
  void* c2;               /* packed copy of C (dims M x N) in the MFMA dtype, or null */
  int32_t qkv_packed;     /* ROPE_VT epilogue, bf16: q/k stored in fragment order (rows = b*vt_ld + n, K-dim = rope_cols) and
                             V in PV-operand order [(b,h)][vt_ld/32][4][64][8] -- the layouts sp3_attention_packed reads */
  int32_t out_packed;     /* plain epilogue: store C in fragment order (it is the next GEMM's packed A; dims M x N) */
  int32_t w_packed;       /* W is in MFMA-fragment order [ceil(N/16)][ceil(K/KB)][2 halves][64 lanes][CH/2], zero padded; KB/CH =
                             64/16 (bf16) or 32/8 (fp32); lane = 16*g + r holds row 16*nb + r, k = kb*KB + g*CH + e: e < CH/2 in the first 1 KB
                             half of the 2 KB block, the rest in the second (every wave access is one contiguous KB).
                             2 (fp32 W, product mode f16x3 only): same blocks, but a lane's 32 bytes hold the fp16 planes of its 8 k --
                             first half h = fp16(w), second half l = fp16((w - h) * 2^11), the split the kernel would take per use.  Accepted only with
                             wdtype fp32, f32x3 == 4, not the softmax loader and a resolved tile 0..2: anything else is an error (sp3_gemm_plan: -1) */
  /* --- grouped launches (batch > 1, grid.y): `batch` independent problems of one shape in one launch, e.g. the two
   *   sides of a DUSt3R decoder layer (different weights, dust3r/model.py:196-198).  A / W / C advance by strideA /
   *   strideW / strideC ELEMENTS per batch index (C in its own dtype, any epilogue, also the packed layouts), res1 /
   *   res2 are [batch][M][ld], and the operands below advance by these BYTE offsets.  Offsets may be negative (the
   *   cross-attention k/v projection of side z reads the tokens and statistics of side 1-z).  rope tables / pos are
   *   shared. */
  int64_t sb_A2, sb_bias, sb_ln_stats, sb_ln_s, sb_stats_out, sb_c2, sb_vt;
  /* --- diagnostics: if non-null, the first 8 workgroups of a role-loop launch (tile 13) store shader-clock stamps of
   *   their own timeline: trace[wg*64 + 0] = entry, [1] = loop done, [2] = epilogue done, [8 + i/4] = loader passed the
   *   barrier of k-block i (i % 4 == 0), [32 + i/4] = consumer wave 0 finished k-block i.  tools/trace_gemm.py prints it. */
  int64_t* trace;
  /* --- the spatial-memory read as two launches (spann3r/model.py:159-183: softmax over the bank, probabilities below
   *   attn_thresh dropped, renormalised, times V):
   *   launch 1, the score GEMM (plain loader/epilogue): sm_stats_out[M][ceil(N/32)][2] receives, per row and 32-column
   *     group of the finished C, (max, sum exp(x - max)) -- the softmax statistics leave with the scores.
   *   launch 2, loader SP3_LOAD_SOFTMAX (16x64 tile, K over 4 waves): A is the fp32 score matrix [M, lda] (K = bank tokens, any multiple
   *     of 4); each lane merges sm_stats[M][sm_nt][2] of its rows to (m, Z) and turns the scores it loads into
   *     p = exp(a - m) / Z, p < sm_thresh -> 0, on their way into the MFMA; C = (p . W^T) / sum(kept p) (+ bias, res);
   *     sm_zout[M][4] receives (sum(kept p), m, 1/Z, -) per row.  No probability matrix exists in memory.
   *     sp3_colsum_softmax finishes the column sums (mem_attn) from the scores and sm_zout. */
  float* sm_stats_out;
  const float* sm_stats;
  int32_t sm_nt;
  float sm_thresh;
  float* sm_zout;
  /* --- fp32 operands (wdtype SP3_F32, A fp32), register-ring tiles 0-3: products through three bf16 MFMAs per k-block
   *   (hi.hi + hi.lo + lo.hi of a bf16 split of both operands: 16 mantissa bits per product, fp32 accumulate) instead of the
   *   fp32 MFMA -- 2-3x the matrix rate, the "f32x3" precision mode of the model.  Ignored for bf16 operands. */
  int32_t f32x3;
  /* --- dtype of the residual maps res1 / res2 (their pointer type says fp32): 1 = they hold bf16.  Only the lean small-map
   *   convolutions (tiles 40 / 41) read bf16 residuals, and only next to a bf16 map and output (res_bf16 == out_bf16 == a_bf16);
   *   sp3_gemm_plan answers -1 for any other combination and the general tiles refuse res_bf16 != 0, so a descriptor whose
   *   residual dtype differs from its output dtype is never routed to a kernel that would reinterpret the bytes. */
  int32_t res_bf16;
  /* --- the growing extent of the spatial-memory read as DEVICE state (round 6): if non-null, the score GEMM of the read (tile 43:
   *   sm_stats_out set) takes its column count N from dyn_n[0] and its P.V GEMM (tile 44: loader SP3_LOAD_SOFTMAX) its contraction
   *   length K (and sm_nt = ceil(K / 32)) -- the bank's current token count, spann3r/model.py:80-95 grows it by a frame per step.
   *   The descriptor's N / K then only bound what the launch can serve (grid size, argument checks; dyn_n[0] <= that bound,
   *   dyn_n[0] % 4 == 0), so ONE captured hipGraph serves every bank length up to it.  Lean instances only: the general tiles
   *   refuse a descriptor with dyn_n set. */
  const int32_t* dyn_n;
  /* --- res2 as a HALF-resolution map (lean small-map convolutions, tiles 40 / 41, bf16 maps only): res2_up_H > 0 says res2 is the NHWC map
   *   [B, res2_up_H, res2_up_W, N] and the residual added is its bilinear x2 (align_corners, the arithmetic of sp3_upsample2x), cropped to
   *   conv_OH x conv_OW (<= 2 res2_up_H x 2 res2_up_W) and rounded to the map dtype as the stored upsampled map would have been:
   *   FeatureFusionBlock's interpolate -> next block's `output + res` (croco/models/dpt_block.py:205-218) without the upsampled map in
   *   memory.  sp3_gemm_plan answers -1 for any other kernel family.
   *   Rounding: the bilinear x2 is computed in fp32 (csrc/common.h up2x_taps / up2x_mix: the one arithmetic of every upsample kernel) and
   *   rounded to the map dtype BEFORE it is added, so the residual is bit-equal to what sp3_upsample2x_bf16 would have stored; r1 + r2
   *   are then added in fp32 and the sum is rounded once, at the store.  Against a float64 interpolation rounded to bf16 a fraction of a
   *   per cent of the residual's elements therefore sit on the other bf16 neighbour (tests/gemm_desc_ref.py takes either). */
  int32_t res2_up_H, res2_up_W;
} sp3_gemm_desc;
int sp3_gemm(const sp3_gemm_desc* desc_host, void* stream);
/* Launch planning.  Which kernel instance a descriptor runs on is decided in the library only (csrc/gemm.hip gemm_plan): hosts pass
 * tile < 0 and ask sp3_gemm_plan / sp3_gemm_plan_n when they need the answer (a profile label, an operand layout to prepare).
 *
 * sp3_gemm_n: n (1..4) independent problems that depend on the same inputs, in ONE launch where the library has a kernel for the
 * group; sp3_gemm is its n = 1 case.
 *  - every descriptor a small-map convolution (tiles 40 / 41, which may be mixed): one level launch -- a 1-D grid in which problem i
 *    owns a contiguous range of workgroups, the one with the longest contraction first.  (The level kernel holds tile 41 for bf16
 *    maps only: an fp32 map on tile 41 goes out on its own, before the level.)
 *  - n = 2, both on one lean q/k/v instance (ROPE_VT, tiles 30 / 31 / 50..): one launch of that instance, e.g. a decoder layer's
 *    self-attention q/k/v projection (N = 2304) and its cross-attention k/v projection (N = 1536), which both read the previous
 *    layer's tokens (dust3r/model.py:196-198, croco/models/blocks.py:187-189).
 *    The two descriptors describe the same tokens: equal M, tokens, heads, vt_ld and ln_eps, and the SAME pos / rope_cos / rope_sin
 *    pointers (the launch carries one set).  Planning reads no pointer values, so sp3_gemm_plan_n answers the pair's tile whatever
 *    the pointers are; sp3_gemm_n refuses a pair that breaks this rule before anything is launched.
 *  - otherwise differently shaped groups of ONE general kernel instance (grid.y = sum of the batches; same dtypes, loader and product
 *    mode; no split-K, no softmax loader).  A pair's second descriptor with tile < 0 runs on the first one's tile.  With more than
 *    two, every descriptor must resolve to the first one's tile by itself -- grouping never moves a member of a level to another
 *    instance -- and a group that disagrees is refused.
 * sp3_gemm_plan_n: tiles[i] = the tile sp3_gemm_n(descs, n) runs descs[i] on; nonzero for a group it refuses. */
int sp3_gemm_n(const sp3_gemm_desc* const* descs, int n, void* stream);
int sp3_gemm_plan_n(const sp3_gemm_desc* const* descs, int n, int* tiles);
/* The tile sp3_gemm runs `desc` on when desc->tile < 0 (desc->tile itself is ignored), or < 0 for an invalid descriptor.  Tiles
 * 30.. are the LEAN small-M instances (csrc/gemm_sm.hip): the per-frame step's 196-row weight-streaming Linears
 * (croco/models/blocks.py:73-79,94-112,149-169 at batch 1) on bf16 fragment-order operands, with shape, tile and epilogue fixed at
 * compile time -- 30 / 31: q/k/v projections (K = 1024 / 768, ROPE_VT epilogue with qkv_packed), 32 / 33: fc1 + GELU into
 * fragment order (K = 1024 / 768), 34..38: output projections onto the fp32 residual stream (K = 1024, 4096, 768, 3072, 1792).
 * They serve M <= 256, batch <= 2, bias set, alpha = 1, no split-K / second residual / split A; anything else runs on the general
 * tiles above.  40 / 41: loader CONV3X3 on maps of <= 256 / <= 2048 output pixels (NHWC map, residuals and output all fp32 or all bf16 --
 * a_bf16 = out_bf16 = res_bf16 --, bf16 fragment-order weights, K = 9 Cin a multiple of 64, plain epilogue with bias / ReLU / two residuals): the DPT heads' small-map convolutions
 * (croco/models/dpt_block.py:33-75,95-113) in ONE launch instead of split-K partials + sp3_reduce_ln.  SP3_LEAN_GEMM=0 in the environment switches them off (A/B runs). */
int sp3_gemm_plan(const sp3_gemm_desc* desc_host);

/* ------------------------------------------------------------------------------------------
 * sp3_layernorm : nn.LayerNorm over the last dim (croco/models/blocks.py:128-129,187-190 eps 1e-6;
 * dust3r/model.py:153,204; spann3r/model.py:154,174,308 -- norm_q/k/v eps 1e-5).
 * x fp32 [rows, ldx] -> out [rows, ldo] (fp32, or bf16 if out_bf16). C % 4 == 0, C <= 4096.
 */
int sp3_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                  void* out, int64_t ldo, int out_bf16, int rows, int C, void* stream);
/* Same, output in fragment order (see sp3_gemm_desc.a_packed). */
int sp3_layernorm_packed(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                         void* out, int out_bf16, int rows, int C, void* stream);
/* fp32 row-major output (as sp3_layernorm) AND a bf16 fragment-order copy for GEMM consumers in the same launch: rows are taken
 * in groups of group_rows (one image / one decoder side) and group g starts at packed row g * group_rows_pad (a multiple of 16),
 * so every group is an a_packed operand of its own.  enc_norm / dec_norm (dust3r/model.py:153,204), whose outputs are both
 * API-visible (fp32) and the A operands of decoder_embed / the key MLPs (dust3r/model.py:190-191, spann3r/model.py:299-303). */
int sp3_layernorm_dual(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, float* out, int64_t ldo,
                       void* out_packed_bf16, int rows, int C, int group_rows, int group_rows_pad, void* stream);
/* Same, but stores the result TRANSPOSED: out[c * ldo + row] (used to append LN_v(value) columns
 * to the [1024, capacity] V^T bank of the spatial memory). */
int sp3_layernorm_t(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                    void* out, int64_t ldo, int out_bf16, int rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * sp3_reduce_ln : finishes a split-K GEMM and fuses what the reference does next on the residual stream:
 *   x = sum_s partial[s] + bias (+ res);  x_out = x (fp32, optional);
 *   out1 = LayerNorm(x; g1,b1) (optional), out2 = LayerNorm(x; g2,b2) (optional)  -- fp32 or bf16.
 * Replaces `x = x + drop_path(proj/fc2(...))` followed by the next norm1/norm2/norm3/norm_y/enc_norm/dec_norm
 * (croco/models/blocks.py:128-129,187-190; dust3r/model.py:153,204).  One wave per row; C % 4 == 0, C <= 4096.
 */
typedef struct sp3_reduce_ln_desc {
  const float* partial;   /* [splits][rows][C] fp32, split stride in elements */
  int64_t split_stride;
  const float* bias;      /* [C] or null */
  const float* res;       /* [rows, ldres] or null */
  int64_t ldres;
  float* x_out;           /* [rows, ldx] or null (may alias res) */
  int64_t ldx;
  const float* g1; const float* b1; void* out1; int64_t ld1; int32_t out1_bf16;
  const float* g2; const float* b2; void* out2; int64_t ld2; int32_t out2_bf16;
  float eps;
  int32_t splits, rows, C;
  int32_t out1_packed, out2_packed;   /* store the LayerNorm output in fragment order (GEMM a_packed operand) */
  int32_t act;            /* SP3_ACT_NONE | SP3_ACT_RELU, applied to sum + bias BEFORE the residuals (sp3_gemm's order) */
  const float* res2;      /* second residual [rows, ldres2] or null: x = act(sum + bias) + res + res2 */
  int64_t ldres2;
} sp3_reduce_ln_desc;
int sp3_reduce_ln(const sp3_reduce_ln_desc* desc_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * sp3_rope_2d : drop-in for curope.rope_2d (curope.cpp:49-69, kernels.cu:17-108).
 * tokens [B,N,H,D] modified in place; element (b,n,h,d) at tokens + b*sB + n*sN + h*sH + d
 * (the reference only requires stride(3)==1 && stride(2)==D, kernels.cu:91; sH generalises it);
 * positions int64 [B,N,2] contiguous; D % 4 == 0; dtype SP3_F32 | SP3_BF16; fwd = +1 / -1.
 */
int sp3_rope_2d(void* tokens, int dtype, int B, int N, int H, int D, int64_t sB, int64_t sN, int64_t sH,
                const int64_t* positions, float base, float fwd, void* stream);

/* ------------------------------------------------------------------------------------------
 * sp3_attention : softmax(q k^T * scale) v per head, head_dim 64
 * (croco/models/blocks.py:105-109 and 162-166).  q [B,Nq,heads,64] / k [B,Nk,heads,64] with row
 * strides ldq/ldk and batch strides sq/sk (elements, `dtype`), already RoPE'd; vt as written by
 * the ROPE_VT epilogue; out fp32 (or bf16 if out_bf16) [B*Nq, ldo] with head h at columns [64h, 64h+64).
 * dtype: SP3_F32 | SP3_BF16 (operands in that type) |
 *   SP3_ATTN_F32X3 = fp32 operands with every product through three bf16 MFMAs of a (hi, lo) split (the "f32x3" precision of
 *                    the model: 16 mantissa bits per product, fp32 softmax and accumulation) |
 *   SP3_ATTN_F16X3 = fp32 operands with every product through three fp16 MFMAs of a split x = h + l * 2^-11 (the "f16x3" precision:
 *                    22 operand bits, every product exact in fp32; operands must stay below fp16's 65504).
 * Pads: q rows beyond Nq and k rows beyond Nk inside the allocation are never read and may hold anything.  vt columns
 * [Nk, Nk rounded up to 64) are read and multiplied by probabilities that are exactly zero: they may hold anything FINITE
 * (0 * NaN and 0 * inf are NaN); columns beyond that up to vt_ld are never read.  Any scale, of either sign, is served.
 */
int sp3_attention(const void* q, int64_t sq, int64_t ldq, const void* k, int64_t sk, int64_t ldk,
                  const void* vt, int64_t vt_ld, void* out, int64_t ldo, int out_bf16,
                  int B, int heads, int Nq, int Nk, float scale, int dtype, void* stream);
/* out_packed != 0: out is stored in fragment order as a [B*Nq, heads*64] GEMM operand (ldo ignored) */
int sp3_attention_ex(const void* q, int64_t sq, int64_t ldq, const void* k, int64_t sk, int64_t ldk,
                     const void* vt, int64_t vt_ld, void* out, int64_t ldo, int out_bf16, int out_packed,
                     int B, int heads, int Nq, int Nk, float scale, int dtype, void* stream);

/* bf16 attention on the fragment-order q/k and PV-order V written by the qkv_packed ROPE_VT epilogue: every operand load
 * is one contiguous wave read, the next key tile is prefetched during the softmax.  qp/kp: packed [B*npad_q|npad_k, q_cols|k_cols]
 * matrices, head h of q at columns q_col0 + 64h (k: k_col0 + 64h); vtp as described at qkv_packed (vt_ld = npad_k).
 * out: fp32/bf16 row-major [B*Nq, ldo] or fragment order (out_packed).  o_group > 0: every o_group consecutive images form
 * one problem of a grouped launch whose output rows start at a multiple of o_group_rows (image b -> row
 * (b / o_group) * o_group_rows + (b % o_group) * Nq), so each problem's packed rows stay 16-aligned; 0: rows b * Nq.
 * Pads: q rows [Nq, npad_q) and k rows [Nk, npad_k) of an image may hold anything, NaN included -- a padded query's results are
 * dropped, a padded key is taken out of the softmax by a select.  V of keys [Nk, Nk rounded up to 64) is multiplied by
 * probabilities that are exactly zero and may hold anything FINITE (0 * NaN is NaN); V beyond that is never read.  Output rows
 * other than the B * Nq defined ones (the rows [o_group * Nq, o_group_rows) of a group among them) are not written.
 * scale > 0 is required: the kernel takes the tile maximum of the raw scores before it scales them. */
int sp3_attention_packed(const void* qp, int q_cols, int q_col0, int npad_q, const void* kp, int k_cols, int k_col0, int npad_k,
                         const void* vtp, void* out, int64_t ldo, int out_bf16, int out_packed,
                         int B, int heads, int Nq, int Nk, float scale, int o_group, int o_group_rows, void* stream);

/* Host only, launches nothing: the query blocks of 16 rows that one workgroup of sp3_attention_packed(B, heads, Nq) takes (1 or 2; 0 for
 * a shape the launch would refuse).  A workgroup reads its head's whole K and V^T once for all its blocks; the grid is
 * ceil(Nq / (16 QB)) x heads x B workgroups.  A query block's result does not depend on the count that computed it, bit for bit. */
int sp3_attention_packed_qb(int B, int heads, int Nq);

/* sp3_attention_packed with the QUERY PROJECTION inside the launch (round 6): a decoder layer's cross-attention
 * (croco/models/blocks.py:149-169) reads q = RoPE2D(projq(norm2(x))) of its own side; instead of a 196 x 768 x 768 GEMM launch in front
 * of the attention launch, every attention workgroup (16 query rows x one head) computes its [16 x 64] q tile from the fragment-order
 * bf16 copy of x, the producer's LayerNorm partials (folded norm2: ln_s = column sums of gamma (.) Wq, bias = bq + Wq beta) and the
 * fragment-order weight.  Images come in groups (the two decoder sides of a grouped launch): image b belongs to group b / o_group;
 * its rows are (b % o_group) * Nq + token inside the group's x / statistics / positions; the *_group_stride fields step from group
 * to group (elements of bf16, floats).  k / v / out arguments as sp3_attention_packed, pads and scale > 0 included; rows of
 * x_packed / ln_stats / pos beyond a group's o_group * Nq are never read.  D = 768 (12 heads), Nq < 512. */
typedef struct sp3_attn_qproj_desc {
  const void* x_packed; int64_t x_group_stride;
  const float* ln_stats; int64_t stats_group_stride;   /* [rows][D / 32][2] */
  const void* w_packed; int64_t w_group_stride;         /* [D][D] fragment order */
  const float* ln_s; const float* bias; int64_t vec_group_stride;
  const int32_t* pos; const float* rope_cos; const float* rope_sin;   /* [rows of one group][2] (y, x); tables [max_pos][16] */
  float ln_eps; int32_t D;
  const void* kp; int32_t k_cols, k_col0, npad_k; const void* vtp;
  void* out; int64_t ldo; int32_t out_bf16, out_packed;
  int32_t B, heads, Nq, Nk; float scale; int32_t o_group, o_group_rows;
} sp3_attn_qproj_desc;
int sp3_attention_packed_qproj(const sp3_attn_qproj_desc* desc_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spatial-memory kernels (spann3r/model.py:97-210).
 * The bank (spann3r_amd/model.py SpatialMemory) keeps, next to the reference's mem_k / mem_v / mem_attn / mem_count, the
 * two operands of a read already normalised and in sp3_gemm's fragment order (w_packed): K' = gamma_q (.) LN_k(mem_k)
 * [cap, 1024] and LN_v(mem_v)^T [1024, cap], plus s_bank / b_bank [cap] that fold LN_q into the S GEMM.
 * sp3_bank_write   : one launch per stored frame (:80-95 plus the bank-side LayerNorms of :154,174): raw copies, K', V^T,
 *   s_bank[t] = alpha * sum_c K'[t,c] (of the rounded operand), b_bank[t] = alpha * sum_c beta_q[c] LN_k(k)[t,c].
 * sp3_softmax_thresh: rows of S fp32 [rows, ld]: softmax over the first M columns; if thresh > 0, p < thresh -> 0 and
 *   renormalise (:160,170-172).  Outputs (either may be null): P fp32 [rows, ld] (columns [M, Mpad) written as 0) and
 *   P_packed = the probabilities as sp3_gemm's a_packed operand [rows, K] with K = M rounded up to one k-block (64 bf16 /
 *   32 fp32, zero filled), stride_packed elements per batch entry.  batch in grid.y via strideS.
 * sp3_colsum_accum : mem_attn[j] += sum_r P[r, j]  (:180-181) from the row-major fp32 P;
 * sp3_colsum_packed: the same from the fragment-order copy (one writer per column, fixed order: deterministic).
 * sp3_pack_stats   : fragment-order copy + per-32-column (sum, sum of squares) partials of a row-major fp32 matrix (what
 *   a producer GEMM's c2 / stats_out write), for callers that hand memory_read a plain tensor.
 * sp3_cos_sim      : score[t] = mean_p cos(k[p,:], wm[t,p,:]) for t < T (:102-112); k fp32 [P,C],
 *   wm fp32 [T,P,C] contiguous; scratch fp32 [T*P] holds the per-patch cosines (one wave per (t,p) pair, then one
 *   block per t averages them). Deterministic reduction order.
 * sp3_mem_append   : count[0..M) += 1; count[M..M+P) = 0; attn[M..M+P) = 0  (:84-90).
 * sp3_prune_select : w = attn/count, w[count < protect] = 1e8; sel[0..top_k) = indices of the top_k
 *   weights, sorted by weight descending, ties by index ascending (:187-193). M <= 16384.
 * sp3_gather_rows  : dst[i, :] = src[sel[i], :] (row gather of a [*, C] matrix, elem_size bytes/elem).
 * sp3_gather_cols  : dst[c, i] = src[c, sel[i]] for c < C (a row-major V^T), zero-fills [n_sel, n_fill).
 * sp3_gather_packed_rows / _cols : the same two gathers on fragment-order matrices ([*, C] rows = tokens; [C, cap] with
 *   k = token; the column gather zero-fills tokens [n_sel, n_fill)).
 * sp3_gather_1d    : dst[i] = src[sel[i]] fp32.
 */
typedef struct sp3_bank_write_desc {
  const float* feat_k;    /* [P, C] fp32: the frame's memory key   (feat_k1) */
  const float* feat_v;    /* [P, C] fp32: the frame's memory value (cur_v + feat_k1) */
  float* k_raw;           /* [cap, C] fp32 = reference mem_k; rows [M, M+P) are written */
  float* v_raw;           /* [cap, C] fp32 = reference mem_v */
  void* k_hat;            /* fragment-order [cap, C] in wdtype: gamma_q (.) LN_k(mem_k) */
  void* v_hat_t;          /* fragment-order [C, cap] in wdtype: LN_v(mem_v)^T */
  float* s_bank;          /* [cap] */
  float* b_bank;          /* [cap] */
  const float *gamma_k, *beta_k, *gamma_v, *beta_v, *gamma_q, *beta_q;   /* norm_k / norm_v / norm_q, fp32 [C] */
  float eps;              /* 1e-5 (spann3r/model.py:245-247) */
  float alpha;            /* 1 / sqrt(C): the S GEMM's scale, folded into s_bank / b_bank */
  int32_t M, P, C, cap;   /* cap % 64 == 0, C % 256 == 0 */
  int32_t wdtype;         /* SP3_F32 | SP3_BF16 */
  const int32_t* state;   /* round 6: if non-null, the first row M is read from state[0] on the device (sp3_bank_state_set) and the M
                           * field is ignored: one captured launch serves every fill level; rows >= cap are not written */
} sp3_bank_write_desc;
int sp3_bank_write(const sp3_bank_write_desc* desc_host, void* stream);
int sp3_softmax_thresh(const float* S, float* P, int64_t ld, int64_t strideS, int rows, int M, int Mpad,
                       float thresh, int batch, void* P_packed, int64_t stride_packed, int packed_bf16, void* stream);
/* the packed-only form of sp3_softmax_thresh for long banks, two streaming launches (row statistics; then one contiguous kilobyte of
 * fragment-order probabilities per wave store): same arithmetic with v_exp_f32; rowstat_ws: batch * rows * 4 floats */
int sp3_softmax_pack(const float* S, int64_t ld, int64_t strideS, int rows, int M, float thresh, int batch, void* P_packed,
                     int64_t stride_packed, int packed_bf16, float* rowstat_ws, void* stream);
int sp3_colsum_accum(const float* P, int64_t ld, int rows, int M, float* mem_attn, void* stream);
int sp3_colsum_packed(const void* P_packed, int packed_bf16, int rows, int M, float* mem_attn, void* stream);
/* the column sums of the two-launch read (sp3_gemm, loader SP3_LOAD_SOFTMAX): mem_attn[j] += sum_r [p >= thresh] p / Z'_r,
 * p = exp(S[r, j] - m_r) / Z_r with rowz[r] = (Z', m, 1/Z, -) = that launch's sm_zout; fixed summation order.  append_P > 0
 * also does sp3_mem_append(mem_count, mem_attn, M, append_P) (the frame that was read against is committed in the same launch). */
int sp3_colsum_softmax(const float* S, int64_t ld, int rows, int M, const float* rowz, float thresh, float* mem_attn,
                       float* mem_count, int append_P, void* stream);
int sp3_pack_stats(const float* x, int64_t ldx, int rows, int C, void* packed, int packed_bf16, float* stats, void* stream);
int sp3_gather_packed_rows(const void* src, void* dst, const int32_t* sel, int n_sel, int C, int elem_size, void* stream);
int sp3_gather_packed_cols(const void* src, void* dst, const int32_t* sel, int n_sel, int n_fill, int C, int cap,
                           int elem_size, void* stream);
int sp3_cos_sim(const float* k, const float* wm, int T, int P, int C, float* scratch, float* score, void* stream);
/* Device-resident fill state of a bank (round 6): state[0] = M (tokens stored), state[1] = wm (frames of working memory,
 * spann3r/model.py:120-143).  The host owns the policy (commit / skip / prune are its decisions, as in the reference) and pushes the
 * values after every change; the kernels of a step read them from the device, so the step's hipGraph does not depend on them.
 * sp3_cos_sim_state = sp3_cos_sim against the last state[1] frames of k_raw [cap, C] (rows [M - wm P, M)), wm <= Tmax: launched
 * for Tmax frames, surplus workgroups exit; score[t] for t >= wm is left untouched. */
int sp3_bank_state_set(int32_t* state, int M, int wm, void* stream);
/* The long-bank read without a score matrix (round 6; spann3r/model.py:159-183 at attn_thresh = 0, > 256 query rows).  Stage 1 =
 * sp3_gemm with sm_stats_out AND a fragment-order bf16 output (lean tile 45): C = p~ = exp(s - m_g) per 64-key group g of a row,
 * [M rows][ldc = bank capacity], sm_stats_out[ldc / 64][M rounded up to 256] = (m_g, sum_g p~) as float2.  sp3_prob_merge turns the
 * statistics into scale[g][row] = exp(m_g - m_row) / Z_row (same [ldc / 64][rows_pad] layout, fp32).  Stage 2 = sp3_gemm with loader
 * SP3_LOAD_SOFTMAX in its probability form (lean tile 46: A = p~ a_packed bf16, sm_stats = scale, PARTIAL epilogue, splitk a multiple of
 * 8, ldw = the capacity): partial[s] = sum over the groups of slice s of scale[g] * (p~_g . V_hat_g); sp3_reduce_ln adds the slices and
 * q.  sp3_colsum_prob: mem_attn[key] += sum_rows p~[row, key] * scale[key / 64][row] (:180-181).  M = bank tokens (N of stage 1, K of
 * stage 2), or dyn_n[0] if dyn_n is set (then M only sizes the launch). */
int sp3_prob_merge(const float* stats, float* scale, int rows, int M, int cap, const int32_t* dyn_n, void* stream);
int sp3_colsum_prob(const void* P_packed, const float* scale, int rows, int M, int cap, const int32_t* dyn_n, float* mem_attn, void* stream);
int sp3_cos_sim_state(const float* k, const float* k_raw, int Tmax, int P, int C, const int32_t* state, float* scratch, float* score,
                      void* stream);
int sp3_mem_append(float* count, float* attn, int M, int P, void* stream);
int sp3_prune_select(const float* attn, const float* count, int M, float protect, int top_k,
                     int32_t* sel, void* stream);
int sp3_gather_rows(const void* src, void* dst, const int32_t* sel, int n_sel, int C, int elem_size, void* stream);
int sp3_gather_cols(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const int32_t* sel, int n_sel,
                    int n_fill, int C, int elem_size, void* stream);
int sp3_gather_1d(const float* src, float* dst, const int32_t* sel, int n_sel, void* stream);

/* ------------------------------------------------------------------------------------------
 * DPT-head helpers (all maps NHWC fp32).
 * sp3_im2col_patch : non-overlapping p x p patches -> rows [B*(H/p)*(W/p), C*p*p], k = (c, py, px)
 *   so the Conv2d weight [E, C, p, p] is used unchanged as W[E, C*p*p] (dust3r/patch_embed.py:24,
 *   spann3r/model.py:317). Source element (b,c,y,x) at img + b*sb + c*sc + y*sy + x*sx.
 * sp3_upsample2x   : F.interpolate(scale_factor=2, mode='bilinear', align_corners=True)
 *   (croco/models/dpt_block.py:214-216, 253-258) on [B,H,W,C] -> [B,2H,2W,C]; optional crop of the
 *   output to [outH, outW] (dust3r/heads/dpt_head.py:57).
 * sp3_head_final   : head.4 1x1 conv (128->4) + postprocess (dust3r/heads/postprocess.py:22-58):
 *   pts3d = xyz/max(|xyz|,1e-8) * expm1(|xyz|), conf = 1 + exp(c).  feat [pixels, C] fp32,
 *   w fp32 [4, C], b fp32 [4] -> pts [pixels,3], conf [pixels], raw [pixels,4] (optional).
 */
/* sp3_conv3x3_tile : Conv2d(3x3, stride 1, padding 1) on an NHWC map [B,H,W,Cin] -> [B,H,W,Cout] as an LDS-tiled
 *   implicit GEMM (bf16 MFMA, fp32 accumulation): out = act(conv(relu_in ? relu(x) : x) + bias) + res1 + res2.
 *   x fp32 or bf16 (in_bf16); w_packed = the [Cout, 9*Cin] weight (k = (ky*3+kx)*Cin + ci) as bf16 in sp3_gemm's
 *   w_packed fragment order; bias fp32[Cout] / res1 / res2 fp32 NHWC maps of the output shape, all optional;
 *   out fp32 or bf16 (out_bf16).  Cin, Cout multiples of 64; act is SP3_ACT_NONE or SP3_ACT_RELU.
 *   Replaces the Conv2d calls of ResidualConvUnit_custom (croco/models/dpt_block.py:120-142), scratch.layer_rn
 *   (:180-188) and the head convs (:318-324) in bf16 mode; fp32 mode and stride 2 use sp3_gemm's LOAD_CONV3X3.
 *   out_bf16 (0 / 1): the output map is bf16; res_bf16 (0 / 1): the residual maps res1 / res2 are bf16 too (else fp32).
 *   tile_px chooses the workgroup's tile: 0 = by size, 1 = 8 x 8 pixels x 64 channels, 2 = 8 rows x 16 pixels x 64 channels, 3 = 8 x 16
 *   pixels x 32 channels (2 and 3 need Cin % 128 == 0: the halo is staged 128 channels at a time; half the weight stream per flop).
 *   By size: the 64-channel wide tile once its grid has >= 256 workgroups, the 32-channel one from 80 (batch-1 56 x 56 maps:
 *   112 -> 224 workgroups), else 8 x 8.  All tiles give the same sums up to fp32 addition order.
 */
int sp3_conv3x3_tile(const void* x, int in_bf16, const void* w_packed, const float* bias, const float* res1,
                     const float* res2, void* out, int out_bf16, int res_bf16, int tile_px, int B, int H, int W,
                     int Cin, int Cout, int relu_in, int act, void* stream);
int sp3_im2col_patch(const float* img, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int B, int C, int H, int W,
                     int p, void* out, int out_bf16, int out_packed, void* stream);
int sp3_upsample2x(const float* in, float* out, int B, int H, int W, int C, int outH, int outW, void* stream);
/* the same on bf16 NHWC maps (bf16 mode of the DPT heads keeps its feature maps in bf16; interpolation arithmetic in fp32) */
int sp3_upsample2x_bf16(const void* in, void* out, int B, int H, int W, int C, int outH, int outW, void* stream);
int sp3_head_final(const float* feat, const float* w, const float* b, int64_t pixels, int C, float* pts,
                   float* conf, float* raw, void* stream);
/* the same with the feature map stored as bf16 (outputs stay fp32: the API's pointmaps / confidences) */
int sp3_head_final_bf16(const void* feat, const float* w, const float* b, int64_t pixels, int C, float* pts, float* conf,
                        float* raw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline: one decoded RGB frame (uint8 HWC, row stride src_row_stride bytes) -> the normalised
 * float image the model consumes.  Replaces PIL Image.crop + Image.resize(LANCZOS) (dust3r/datasets/utils/cropping.py:54-111),
 * ImgNorm (dust3r/utils/image.py:23) and transpose_to_landscape (dust3r/datasets/base/base_stereo_view_dataset.py:215-220):
 *   crop window [crop_t, +H1) x [crop_l, +W1)  ->  Pillow's 8-bit LANCZOS resample to W2 x H2 (horizontal pass into `tmp`
 *   [H1, W2, 3] uint8, then vertical; bounds [n, 2] = (first tap, taps) and coef [n, ksize] = 22-bit fixed-point weights per
 *   output index, computed by the host: spann3r_amd/preprocess.py)  ->  crop [crop2_t, +outH) x [crop2_l, +outW)  ->
 *   (u/255 - 0.5)/0.5  ->  out fp32 [3, outH, outW], or [3, outW, outH] if `transpose` (portrait rectified to landscape).
 * Bit-exact with Pillow for the uint8 stage. */
int sp3_preprocess_image(const uint8_t* src, int64_t src_row_stride, int crop_l, int crop_t, int H1, int W1,
                         const int32_t* hbounds, const int32_t* hcoef, int hksize, int W2,
                         const int32_t* vbounds, const int32_t* vcoef, int vksize, int H2,
                         int crop2_l, int crop2_t, int outW, int outH, int transpose, uint8_t* tmp, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training criterion: ConfLoss_t(Regr3D_t(L21, norm_mode='avg_dis', fix_first), alpha).compute_frame_loss
 * (spann3r/loss.py:20-84,129-285; dust3r/losses.py:52-56) forward and backward on stacked buffers:
 *   P [E, B, HW, 3] predicted pointmaps and Cf [E, B, HW] confidences, one slab per loss entry in the reference's order
 *   L0, L1, R1, L2, R2, ..., R_{n-1} (E = 2 (n-1); L_i = preds_all[i][0], R_i = preds_all[i-1][1]);
 *   G [n, B, HW, 3] ground-truth points (world), V [n, B, HW] validity (bytes), pose0 [B, 16] camera pose of view 1 (affine).
 * forward: out7 (device) = factor loss, loss, conf_loss_1, conf_loss2, conf_mean, pts3d_1, pts3d_2 (the reference's details);
 *   ent_out (device, nullable) [E, 2] = (mean error, conf loss) per entry; ws = device scratch of sp3_conf_loss_ws_bytes(n, B)
 *   bytes that the backward reads.  backward: dP, dC = gradients of grad_scale2[0] * loss + grad_scale2[1] * factor loss
 *   (grad_scale2: 2 floats on the device).  Sums in double, fixed order: deterministic. */
int64_t sp3_conf_loss_ws_bytes(int n, int B);
int sp3_conf_loss_forward(const float* P, const float* Cf, const float* G, const uint8_t* V, const float* pose0, int n, int B, int HW,
                          float alpha, int fix_first, void* ws, float* out7, float* ent_out, void* stream);
int sp3_conf_loss_backward(const float* P, const float* Cf, const float* G, const uint8_t* V, const float* pose0, int n, int B, int HW,
                           float alpha, int fix_first, const void* ws, const float* grad_scale2, float* dP, float* dC, void* stream);
/* Regr3D_t_ScaleShiftInv(L21, gt_scale) forward (spann3r/loss.py:292-368; the validation criterion of spann3r/training.py:39,152):
 * same stacked buffers as sp3_conf_loss_forward (no confidences); the joint median-depth shift and median-centre / median-norm
 * scale (torch.nanmedian: lower middle element) are radix selections on the device.  out (device, 6 + E floats): loss (the SUM over
 * the E entries of the mean Euclidean error), factor loss, mean gt_shift_z, pred_shift_z, gt_scale, pred_scale, then the mean error of
 * every entry.  ws: sp3_ssi_loss_ws_bytes(n, B, HW) bytes of device scratch. */
int64_t sp3_ssi_loss_ws_bytes(int n, int B, int HW);
int sp3_ssi_loss_forward(const float* P, const float* G, const uint8_t* V, const float* pose0, int n, int B, int HW, int fix_first,
                         int gt_scale, void* ws, float* out, void* stream);
/* The per-sample medians of Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True).get_all_pts3d_t (the configuration of the
 * reference's eval.py:55): the same selection without the avg_dis normalisation in front of it.  stats (device) fp32 [B, 4] =
 * gt_shift_z, pred_shift_z, gt_scale, pred_scale (clipped to [1e-3, 1e3]).  Same buffers and scratch as sp3_ssi_loss_forward. */
int sp3_ssi_align_stats(const float* P, const float* G, const uint8_t* V, const float* pose0, int n, int B, int HW, void* ws, float* stats,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Pieces of the BACKWARD of the spatial-memory read in its training form (attn_thresh = 0, mem_dropout; forward:
 * spann3r/model.py:145-183), between the four sp3_gemm launches of spann3r_amd/train.py:
 * sp3_transpose     : dst[c * ld_dst + r] = src[r * ld_src + c]  (sp3_gemm computes A[M,K] . W[N,K]^T only)
 * sp3_mul           : out = a (.) b  (the dropout mask on the probabilities, :168)
 * sp3_softmax_bwd   : dS = alpha * A (.) (dA - rowsum(dA (.) A)), dA = dAd (.) mask (mask nullable), rows x T, row stride ld
 * sp3_layernorm_bwd : dx = LayerNorm backward of dy w.r.t. x (+ dx_add, nullable: the residual path), dgamma / dbeta [C]
 *                     (accumulate != 0: added to their current contents); scratch: ceil(rows / 4) * 2 * C floats.  Column sums in a
 *                     fixed order: deterministic. */
int sp3_transpose(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int rows, int cols, void* stream);
int sp3_transpose_batched(const float* src, int64_t ld_src, int64_t stride_src, float* dst, int64_t ld_dst, int64_t stride_dst, int rows,
                          int cols, int batch, void* stream);       /* `batch` matrices, element strides between them */
/* same, and columns [rows, pad_to) of every destination row are written as zeros (pad_to <= ld_dst, pad_to - rows < 32): the
 * contraction pad of the next GEMM without a separate fill launch */
int sp3_transpose_pad(const float* src, int64_t ld_src, int64_t stride_src, float* dst, int64_t ld_dst, int64_t stride_dst, int rows,
                      int cols, int batch, int pad_to, void* stream);
/* exact-erf GELU (nn.GELU, croco/models/blocks.py:73-79) of the train-mode blocks and its backward dx = dy * gelu'(x) */
int sp3_gelu(const float* x, float* y, int64_t n, void* stream);
int sp3_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* train-mode DPT head pieces (croco/models/dpt_block.py:120-218, dust3r/heads/postprocess.py:10-58), NHWC fp32:
 * sp3_im2col3x3 / sp3_col2im3x3 : the 3x3, pad 1, stride 1|2 convolution as a GEMM over col [B*OH*OW, 9*C] (k = (ky*3+kx)*C + c) and the
 *   adjoint gather that turns d col back into d x;  sp3_relu / sp3_relu_bwd;  sp3_upsample2x_bwd : adjoint of sp3_upsample2x;
 * sp3_postprocess(_bwd) : raw [M, 4] -> pts3d [M, 3] = xyz / |xyz| * expm1(|xyz|), conf [M] = 1 + exp(c), and its backward. */
int sp3_im2col3x3(const float* x, float* col, int B, int H, int W, int C, int stride, void* stream);
int sp3_col2im3x3(const float* dcol, float* dx, int B, int H, int W, int C, int stride, void* stream);
int sp3_relu(const float* x, float* y, int64_t n, void* stream);
int sp3_relu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
int sp3_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, int outH, int outW, void* stream);
int sp3_postprocess(const float* raw, float* pts, float* conf, int64_t M, void* stream);
int sp3_postprocess_bwd(const float* raw, const float* dpts, const float* dconf, float* draw, int64_t M, void* stream);
/* torch.optim.AdamW update of one parameter tensor (spann3r/training.py:327; decoupled weight decay, bias correction for `step` >= 1);
 * the gradient is multiplied by grad_scale first (1 / accum_iter, or the clip coefficient of clip_grad_norm_, croco/utils/misc.py:274). */
int sp3_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
              int step, float grad_scale, void* stream);
int sp3_mul(const float* a, const float* b, float* out, int64_t n, void* stream);
/* bf16 training step (spann3r/training.py:170-259 under bf16 autocast): fp32 row-major [rows, cols] (row stride ld) -> the GEMM's bf16
 * fragment order, as [rows, cols] (dst, nullable) and / or as its transpose [cols, rows] (dstT, nullable) in one pass; pads are written
 * as zeros.  With both forms every product of a Linear's backward (dX = dY . W, dW = dY^T . X) is an sp3_gemm A . W^T launch on packed
 * bf16 operands: the ATen calls they replace are the matmuls autograd derives for nn.Linear (croco/models/blocks.py:73-112). */
int sp3_pack_bf16(const float* src, int64_t ld, int rows, int cols, void* dst, void* dstT, void* stream);
/* sp3_pack_bf16 of the 3x3 / pad 1 im2col matrix [(b, oy, ox), (ky*3 + kx)*C + c] of an NHWC fp32 map x [B, H, W, C] (stride 1 or 2; the layout
 * of sp3_im2col3x3), gathered inside the pack launch: the operand of a 3x3 convolution's bf16 GEMMs (croco/models/dpt_block.py:120-218) without
 * writing and re-reading the 9x larger column matrix. */
int sp3_pack_bf16_conv3x3(const float* x, int B, int H, int W, int C, int stride, int act, void* dst, void* dstT, void* stream);
/* sp3_pack_bf16 with the producer's activation applied to every element as it is loaded (act: 0 none, 1 exact-erf GELU = sp3_gelu, 2 ReLU =
 * sp3_relu; also the `act` of sp3_pack_bf16_conv3x3): Mlp's act(fc1(x)) -> fc2 (croco/models/blocks.py:73-79) and the ReLU -> convolution pairs of
 * the DPT head (dpt_block.py:120-142) without the activation launch and its fp32 output */
int sp3_pack_bf16_act(const float* src, int64_t ld, int rows, int cols, void* dst, void* dstT, int act, void* stream);
/* sp3_pack_bf16, and colsum[j] (+)= sum_r src[r, j] (the bias gradient of the Linear whose dY is being packed; rows <= 8192): the pack
 * launch leaves the column sums of its 64-row tiles in partial_ws (ceil(rows / 64) * ceil(cols / 64) * 64 floats), a second small launch
 * adds them in a fixed order: deterministic, and no second pass over src. */
int sp3_pack_bf16_colsum(const float* src, int64_t ld, int rows, int cols, void* dst, void* dstT, float* colsum, int accumulate,
                         float* partial_ws, void* stream);
/* torch.nn.utils.clip_grad_norm_ (croco/utils/misc.py:262-288, called with clip_grad = 1.0 by spann3r/training.py:227-228) on flat
 * gradient buckets, without a host round trip: sp3_sumsq_partial writes sp3_sumsq_blocks(n) partial sums of squares of one bucket
 * (fixed order: deterministic), sp3_clip_coef reduces `count` partials of all buckets to out[0] = extra_scale * min(1, max_norm /
 * (norm + 1e-6)) and out[1] = norm (of the gradients times |extra_scale|; max_norm <= 0: no clipping). */
int64_t sp3_sumsq_blocks(int64_t n);
/* out[j] (+)= sum_r x[r, j] for a tall fp32 matrix (the bias gradient of a Linear / convolution: autograd's dY.sum(0)), two deterministic
 * stages; scratch: sp3_colsum_rows_ws(rows, N) floats */
int64_t sp3_colsum_rows_ws(int rows, int N);
int sp3_colsum_rows(const float* x, int64_t ld, int rows, int N, float* out, int accumulate, float* scratch, void* stream);
int sp3_sumsq_partial(const float* g, int64_t n, double* partial, void* stream);
int sp3_clip_coef(const double* partial, int count, float max_norm, float extra_scale, float* out, int* step_counter, void* stream);
   /* step_counter (nullable): incremented by one -- the optimizer's step count kept on the device so that a captured step replays */
/* torch.optim.AdamW (spann3r/training.py:327) over one flat bucket of n elements (n % 1024 == 0): p, g, m, v share the element layout;
 * chunk_table holds (weight_decay, lr_scale) per 1024-element chunk (lr_scale < 0: chunk untouched -- parameters without a gradient
 * on any rank); the gradient is multiplied by grad_scale * grad_scale_dev[0] (device scalar, nullable: sp3_clip_coef's out[0]). */
int sp3_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* chunk_table, float lr, float beta1, float beta2,
                   float eps, int step, const float* grad_scale_dev, float grad_scale, const int* step_dev, const float* lr_dev, void* stream);
   /* step_dev / lr_dev (nullable): the step count / learning rate are read from device memory instead (hipGraph replay of the step) */
int sp3_softmax_bwd(const float* A, const float* dAd, const float* mask, float* dS, int64_t ld, int rows, int T, float alpha, void* stream);
/* same, and dS[:, T .. Tpad) = 0 (Tpad <= ld) */
int sp3_softmax_bwd_pad(const float* A, const float* dAd, const float* mask, float* dS, int64_t ld, int rows, int T, int Tpad, float alpha,
                        void* stream);
/* Multi-head attention in training (croco/models/blocks.py:100-108 Attention.forward, :160-166 CrossAttention.forward): the
 * reshape / permute(0, 2, 1, 3) / RoPE2D between the projections and the per-head products, and their backward, for up to three
 * tensors (q, k, v / dq, dk, dv) in ONE launch.  A part reads element (b, n, h, d) at src + b*s_b + n*s_n + h*s_h + d, rotates the
 * token by RoPE2D (pos != NULL: int64 [B*N, 2] (y, x) positions; fwd = +1: croco/models/pos_embed.py:96-157 forward, fwd = -1: its
 * transpose = the backward), and writes it to dst + b*d_b + n*d_n + h*d_h + d (dst nullable) and to the per-head transpose
 * dstT [B*H][hd][ldT] (nullable; pad columns zero), which is the W operand of the A . W^T GEMMs contracted over tokens.
 * hd <= 64, hd % 4 == 0; every stride a multiple of 4 elements, pointers 16-byte aligned. */
typedef struct sp3_head_part {
  const float* src;
  int64_t s_b, s_n, s_h;
  float* dst;
  int64_t d_b, d_n, d_h;
  float* dstT;
  const int64_t* pos;
  int32_t N;
  float fwd;
  int64_t ldT;          /* row length of dstT; columns [N, ldT) are zeroed; 0: N rounded up to 8; at most N rounded up to 64 */
} sp3_head_part;
int sp3_head_shuffle(const sp3_head_part* parts, int nparts, int B, int H, int hd, float rope_base, const float* cos_tab,
                     const float* sin_tab, int tab_len, void* stream);
   /* cos_tab / sin_tab (nullable): cos / sin of position * rope_base^(-f / (hd/4)) as [tab_len][hd / 4] fp32; positions outside the table
    * (or no table) are computed in the kernel */
/* Attention of the train-mode blocks (croco/models/blocks.py:100-108, :160-166: softmax(q k^T * scale) v per head, head_dim 64) as
 * flash-style kernels with a backward -- what torch's autograd derives for those lines, without materialising the attention matrix.
 *   forward : sp3_attention's kernel on fp32 operands (q, k already rotated; vt = per-head V^T [B*heads][64][vt_ld], zero padded to a
 *             multiple of 64 keys), also leaving lse[b*heads + h][query] = (max_j s_j, 1 / sum_j exp(s_j - max)) for the backward
 *             (two floats: one folded log-sum-exp would round a large maximum into the recomputed probabilities);
 *   backward: dq, dk, dv from (q, k, v, d out, lse) with the probabilities recomputed; two launches (16 queries / 16 keys per
 *             workgroup); the per-head transposes qT, doT [B*heads][64][ldTq] and kT [..][ldTk] (sp3_head_shuffle) feed the products
 *             contracted over tokens; lse is the forward's [B*heads][Nq][2]; D is a [B*heads][Nq] scratch: rowsum(P (.) dP) of the recomputed, rounded P and dP, so that the
 *             rows of dS sum to zero as in the unfused softmax backward (rowsum(d out (.) out) leaks a common-mode term in fp32).
 * bf16_products: 0 = exact fp32 MFMA, 1 = operands rounded to bf16 into one bf16 MFMA per product (fp32 accumulation, bf16 training).
 * Element (b, n, h, d) of q / k / v / dout / dq / dk / dv is at p + b*s + n*ld + h*64 + d (strides in elements, multiples of 4). */
int sp3_attention_train_fwd(const float* q, int64_t sq, int64_t ldq, const float* k, int64_t sk, int64_t ldk, const float* vt, int64_t vt_ld,
                            float* out, int64_t ldo, float* lse, int B, int heads, int Nq, int Nk, float scale, int bf16_products, void* stream);
typedef struct sp3_attn_bwd_desc {
  const float *q, *k, *v, *dout;
  int64_t sq, ldq, sk, ldk, sv, ldv, sdo, lddo;
  const float *qT, *kT, *doT;
  int64_t ldTq, ldTk;
  const float* lse;
  float* D;
  float *dq, *dk, *dv;
  int64_t sdq, lddq, sdk, lddk, sdv, lddv;
  int32_t B, heads, Nq, Nk;
  float scale;
  int32_t bf16_products;
} sp3_attn_bwd_desc;
int sp3_attention_train_bwd(const sp3_attn_bwd_desc* d, void* stream);
int sp3_layernorm_bwd(const float* x, int64_t ldx, const float* gamma, const float* dy, int64_t ldy, const float* dx_add, int64_t ld_add,
                      float* dx, int64_t ld_dx, float* dgamma, float* dbeta, int accumulate, float* scratch, int rows, int C, float eps,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-forward geometry (demo.py:147-215).
 * sp3_focal_weiszfeld : estimate_focal_knowing_depth(pts3d, pp, focal_mode='weiszfeld') (dust3r/post_process.py:38-60):
 *   pts3d fp32 [B, H, W, 3], principal point (ppx, ppy); closed-form L2 start, `iters` (reference: 10) rounds of inverse-distance
 *   re-weighting, clipped to [focal_min, focal_max] (already multiplied by the reference's focal_base); focal [B] on the device.
 * sp3_conf_filter : the confident part of a cloud, pixel order kept (demo.py:205-211: conf_sig = (conf - 1) / conf > thresh,
 *   boolean indexing of points and colours): conf [n], pts / rgb [n, 3] (rgb nullable) -> out_pts / out_rgb [total, 3];
 *   scratch: ceil(n / 1024) ints; total: device int64. */
int sp3_focal_weiszfeld(const float* pts3d, int B, int H, int W, float ppx, float ppy, int iters, float focal_min, float focal_max,
                        float* focal, void* stream);
int sp3_conf_filter(const float* conf, const float* pts, const float* rgb, int64_t n, float thresh, int* scratch, int64_t* total,
                    float* out_pts, float* out_rgb, void* stream);

/* Camera poses from pointmaps (demo.py:170-186 calls cv2.solvePnPRansac(points, pixel grid, K, 0) per frame).  OpenCV's pipeline
 * (calib3d/src/solvepnp.cpp, ptsetreg.cpp, epnp.cpp, calibration.cpp; restated for the tests in oracle/pnp_oracle.py) is run by
 * spann3r_amd/postprocess.py::estimate_poses: the 5-point EPnP hypotheses and the 12x12 / 6x6 solves on the host, everything that
 * is O(H*W) here, one workgroup per frame (and hypothesis), double-precision sums in a fixed order.
 * Poses are Rt[12] = row-major R (9) | t (3), world -> camera.  cv_mode != 0 selects OpenCV's consensus test: projection in double,
 * no depth-sign test, (float)err^2 <= (float)thresh^2; cv_mode == 0 is the stricter test of earlier rounds (err < thresh, z > 0).
 * sp3_pnp_score    : counts[F][n_hyp] = consensus of hypothesis Rt[F][n_hyp][12] over the finite points of frame f.
 * sp3_pnp_dlt_accum: out41[F][41] = the four symmetric 4x4 blocks (10 unique entries each: S, Sx, Sy, Sr) of the calibrated DLT
 *   normal matrix [[S, 0, -Sx], [0, S, -Sy], [-Sx, -Sy, Sr]] (cvFindExtrinsicCameraParams2's L^T L) over the finite points (Rt == null)
 *   or over the consensus set of Rt[F][12], and the number of points used; norm4[F][4] = a centroid (3) and scale applied to the
 *   object points first ((0, 0, 0, 1) reproduces OpenCV's un-normalised system).
 * sp3_pnp_gn_accum : out29[F][29] = normal equations of the reprojection error (pixels) at pose Rt[F][12] (DOUBLE: the pose under
 *   refinement): H (21 unique, row-major
 *   upper triangle, parameters (omega, delta) of Xc' = Xc + omega x Xc + delta), g (6), squared error, point count -- over the
 *   consensus set of Rt_mask[F][12] if given (a FIXED set, as solvePnPRansac refines it), else over the inliers of Rt itself. */
int sp3_pnp_dlt_accum(const float* pts, int F, int H, int W, float focal, float cx, float cy, const float* norm4, const float* Rt,
                      float thresh, int cv_mode, double* out41, void* stream);
int sp3_pnp_gn_accum(const float* pts, int F, int H, int W, float focal, float cx, float cy, const double* Rt, const float* Rt_mask,
                     float thresh, double* out29, void* stream);
int sp3_pnp_score(const float* pts, int F, int H, int W, float focal, float cx, float cy, const float* Rt, int n_hyp, float thresh,
                  int cv_mode, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reconstruction metrics (eval.py:189-231, spann3r/tools/eval_recon.py; spann3r_amd/evaluate.py drives these).
 * Clouds are fp32 [n, 3]; indices are int32 (n < 2^31).  No entry point allocates or synchronises; `ws` is caller-provided
 * device scratch of the matching sp3_*_ws_bytes(), 16-byte aligned.
 *
 * sp3_nn_grid: a uniform cell grid over the reference cloud, chosen by the host: origin = the cloud's minimum corner, cell edge h,
 *   inv_h = 1 / h, dims nx * ny * nz (<= 2^24 cells); cell of x = clamp(floor((x - ox) * inv_h), 0, nx - 1), id = (cz * ny + cy) * nx + cx.
 *   slack: an upper bound of the fp32 rounding of cell assignment and wall positions, taken off every stopping bound.
 *   csrc/cell_grid.h is the one statement of the grid's rule (cell of x, ring walk, stopping bound, workspace head), shared by
 *   sp3_nn_query, sp3_knn_query and sp3_mesh_dist_query; spann3r_amd/cell_grid.py is the host half (h, dims, slack, cell_start).
 * sp3_nn_cell_ids     : ids[n] = cell id of every point (also used for the queries, clamped into the grid).
 * sp3_nn_pack_records : recs[i] = (x, y, z, bit pattern of s) of point s = order[i] (order null: s = i): 16-byte records.
 * sp3_nn_query : exact nearest neighbour of q[nq] among the m records sorted by cell id, cell_start[cells + 1] = first record of each
 *   cell.  q_order (nullable): a permutation of the queries (sorted by home cell) that decides which lanes run together; results are
 *   written in caller order.  Rings r = 0..max_ring around the home cell; a query is finished when its best distance is within the
 *   distance to the nearest wall of the visited block that still has cells behind it.  Queries left open go through the brute-force
 *   kernel.  dist > max_dist (+inf: no gate) gives idx -1, dist +inf.  After the call the first 32 bytes of ws hold
 *   { int32 fallback queries, 3 x int32 pad, uint64 cells visited, uint64 points visited }.
 * sp3_nn_brute : the same result by the LDS-tiled brute-force kernel alone, for every query; recs in any order.
 * sp3_knn_query: k <= 32 nearest neighbours, ascending: dist / idx [nq, k]; missing entries (m < k, or beyond max_dist) are +inf / -1.
 *   A grid of one cell makes it a brute-force scan.
 * sp3_knn_normals : per point, the unit eigenvector of the smallest eigenvalue of the covariance (fp64, about the mean) of the
 *   points nbr[i][0..k) (entries < 0 skipped); fewer than 3 neighbours: (0, 0, 1).  Sign unconstrained.
 * sp3_transform_points : out = R src + t in fp64, rounded to fp32; Rt12 (HOST) = row-major R (9) | t (3).
 * sp3_icp_accum : over the pairs (p_i, q = tgt[idx_i]) with idx_i >= 0, in fp64 and a fixed order:
 *   out17 = { count, sum p (3), sum q (3), sum p q^T (9, row-major), sum |p - q|^2 }.
 * sp3_sum_count_f32 : out2 = { sum x_i, #(x_i < thresh) } in fp64, fixed order.
 * sp3_normal_dot : out_i = |na[idx_i] . nb[i]| (gather_a != 0) or |na[i] . nb[idx_i]|; idx_i < 0 gives 0. */
typedef struct {
  float ox, oy, oz, h, inv_h, slack;
  int nx, ny, nz;
} sp3_nn_grid;
int sp3_nn_cell_ids(const float* pts, int64_t n, const sp3_nn_grid* g, int* ids, void* stream);
int sp3_nn_pack_records(const float* pts, const int64_t* order, int64_t n, float* recs, void* stream);
int64_t sp3_nn_query_ws_bytes(int64_t nq);
int sp3_nn_query(const float* q, const int64_t* q_order, int64_t nq, const float* recs, const int* cell_start, int64_t m,
                 const sp3_nn_grid* g, int max_ring, float max_dist, void* ws, float* dist, int* idx, void* stream);
int sp3_nn_brute(const float* q, int64_t nq, const float* recs, int64_t m, float max_dist, void* ws, float* dist, int* idx, void* stream);
int sp3_knn_query(const float* q, const int64_t* q_order, int64_t nq, const float* recs, const int* cell_start, int64_t m,
                  const sp3_nn_grid* g, int k, float max_dist, float* dist, int* idx, void* stream);
int sp3_knn_normals(const float* pts, const int* nbr, int64_t n, int k, float* normals, void* stream);
int sp3_transform_points(const float* src, int64_t n, const double* Rt12, float* out, void* stream);
int64_t sp3_icp_accum_ws_bytes(int64_t n);
int sp3_icp_accum(const float* p, const float* tgt, const int* idx, int64_t n, void* ws, double* out17, void* stream);
int64_t sp3_sum_count_ws_bytes(int64_t n);
int sp3_sum_count_f32(const float* x, int64_t n, float thresh, void* ws, double* out2, void* stream);
int sp3_normal_dot(const float* na, const float* nb, const int* idx, int64_t n, int gather_a, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Headless point-cloud rendering (demo.py:221-225, spann3r/tools/vis.py; spann3r_amd/vis.py drives these).
 *
 * sp3_render_cam: a pinhole camera in the OpenCV convention of the rest of the package (+z forward, pixel centres at integer
 *   coordinates): world-to-camera R (row-major) and t, intrinsics, image size, z_near >= 0 and the square point size (1..8).
 * Projection rule: Xc = R X + t in fp32, every multiply and add rounded on its own, summed left to right.  A point is culled when
 *   it or Xc is not finite or Xc.z <= z_near.  Otherwise u = fx Xc.x / Xc.z + cx, v = fy Xc.y / Xc.z + cy, its pixel is
 *   (floor(u + 0.5), floor(v + 0.5)) and its footprint the point_size x point_size square of pixels whose top-left corner is
 *   pixel - (point_size - 1) / 2 (integer division), clipped to the image.
 * The z-buffer: one uint64 key per pixel, (bit pattern of fp32 Xc.z) << 32 | global point index; all-ones = empty.
 * sp3_render_clear   : every key = all-ones.
 * sp3_render_splat   : one point per lane; point i (global index index_base + i) does an agent-scope 64-bit unsigned atomic min of its
 *   key on every pixel of its footprint: the nearest point wins, at equal depth the lowest index, whatever the arrival order.
 *   conf (nullable, fp32 [n]): only points with (c - 1) / c > conf_thresh are drawn (the reference's mask, demo.py:213).
 *   index_base + n must stay below 2^32 - 1.  n = 0 is a no-op.
 * sp3_render_resolve : per pixel, index_out = low 32 bits of the key (-1: empty), depth_out = the fp32 of its high bits (+inf: empty),
 *   rgb_out uint8 [H, W, 3] = the low three bytes of rgba[index] (background, packed the same way, when empty).  depth_out and
 *   index_out may be null.
 * sp3_pack_rgba8     : rgba[i] = r | g << 8 | b << 16 | 255 << 24 of img fp32 [n, 3], channel = clamp(floor(c * 255 + 0.5), 0, 255).
 * sp3_colorize_hsv   : out uint8 [n, 3] = trunc(255 * hsv_to_rgb(1 - x)), x fp32 [n, 3] in [0, 1]; matplotlib.colors.hsv_to_rgb's
 *   formula in fp32, every operation rounded on its own.
 * sp3_colorize_lut   : out uint8 [n, 4] = lut[clamp(trunc(x * 256), 0, 255)], lut uint8 [256, 4]; lut and out 4-byte aligned. */
typedef struct {
  float R[9];
  float t[3];
  float fx, fy, cx, cy;
  int width, height;
  float z_near;
  int point_size;
} sp3_render_cam;
int sp3_render_clear(uint64_t* keys, int64_t pixels, void* stream);
int sp3_render_splat(const float* pts, const float* conf, float conf_thresh, int64_t n, int64_t index_base, const sp3_render_cam* cam,
                     uint64_t* keys, void* stream);
int sp3_render_resolve(const uint64_t* keys, const uint32_t* rgba, const sp3_render_cam* cam, uint32_t background, uint8_t* rgb_out,
                       float* depth_out, int32_t* index_out, void* stream);
int sp3_pack_rgba8(const float* img, int64_t n, uint32_t* rgba, void* stream);
int sp3_colorize_hsv(const float* x, int64_t n, uint8_t* out, void* stream);
int sp3_colorize_lut(const float* x, int64_t n, const uint8_t* lut, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pointmap meshes (app.py:68-105 pts3d_to_trimesh, :38-47 cat_meshes, :132-167; spann3r_amd/mesh.py and vis.py drive these).
 * No entry point allocates, frees or synchronises; `ws` is caller-provided device scratch of the matching sp3_*_ws_bytes(),
 * 16-byte aligned.  Vertex, pixel and face indices are int32: 4 t h w < 2^31.
 *
 * Validity of pixel p: (valid null or valid[p] != 0) and (conf null or (conf[p] - 1) / conf[p] > conf_thresh, sp3_render_splat's test;
 *   a NaN confidence is invalid) and (pts null or the three coordinates of pts[p] finite).  valid and conf exclude each other.
 * sp3_mesh_faces : the face list of t pointmaps of h x w pixels, vertex index of pixel (f, y, x) = (f h + y) w + x.  A cell is the
 *   2 x 2 pixel square with top-left pixel (y, x), y < h - 1, x < w - 1, corners tl, tr, bl, br.  Candidates, in output order: frame
 *   after frame; per frame four blocks, (tl, tr, bl), (bl, tr, tl), (tr, bl, br), (br, bl, tr); per block the cells row-major.  With
 *   both_windings = 0 only the first and third block exist.  A candidate is kept when its three vertices are valid; the kept ones are
 *   written densely in candidate order: faces int32 [F, 3], colour_px int32 [F] = tl for the first two blocks, br for the last two
 *   (the pixel whose colour the reference gives the face).  faces / colour_px need room for every candidate: 4 (or 2) t (h-1)(w-1).
 *   counts int32 [1 + blocks per frame * t]: counts[0] = F, counts[1 + f * blocks + b] = faces kept of block b of frame f.
 *   Compaction is three launches -- counts per 256-cell tile, one single-workgroup exclusive scan, scatter -- behind one launch
 *   that writes the validity bytes; no workgroup waits on another.  t = 0 is a no-op.
 * sp3_mesh_compact_vertices : keeps vertex i of pts fp32 [n, 3] when a face references it (faces non-null, int32 [nfaces, 3];
 *   valid / conf must be null) or, for a cloud (faces null), when pixel i is valid by the rule above, pts included.  Kept vertices
 *   are written densely in index order: out_pos fp32 [V, 3] = M (scale * x), where scale * x rounds per coordinate and row r of the
 *   row-major 4x4 transform16 (HOST pointer, null = identity; the fourth row is ignored) gives ((m0 x + m1 y) + m2 z) + m3, every
 *   operation rounded on its own; out_rgba[V] = rgba[i] (both null: no colours).  faces are rewritten in place to rows of out_pos
 *   (an index outside 0..n-1 becomes -1).  count[0] = V; minmax fp32 [6] = per-axis min (3) and max (3) of out_pos (+inf / -inf when
 *   V = 0).  A mesh keeps a non-finite vertex only if a face references it: sp3_mesh_faces with pts given emits no such face.
 *   n = 0 is a no-op.
 * sp3_render_tris : draws triangles into the key buffer of sp3_render_splat, one triangle per lane.  Face i = vertices
 *   faces[3i..3i+2] of pts fp32 [nverts, 3]; its key index is index_base + colour_px[i] (colour_px null: + faces[3i]); a face with a
 *   vertex or colour index outside 0..nverts-1 is skipped.  index_base + nverts must stay below 2^32 - 1.  nfaces_dev (nullable,
 *   device int32): only the first min(nfaces, *nfaces_dev) faces are drawn.  point_size is not used.  The rule:
 *   - every vertex is projected as sp3_render_splat projects a point (same fp32 operations, same order, each rounded on its own);
 *     the triangle is culled if any vertex is culled by that rule;
 *   - X = floor(16 u + 0.5), Y = floor(16 v + 0.5) in fp32 (1/16 pixel); culled if any |X| or |Y| exceeds 2^20 or is not finite;
 *   - A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) in int64; A = 0 draws nothing; A < 0: vertices 1 and 2 swap and A = -A (both
 *     orientations are drawn);
 *   - the box = pixels (px, py) with 16 px in [min X, max X] and 16 py in [min Y, max Y], clipped to the image; an empty box draws
 *     nothing; a box of more than max_bbox_px (> 0) pixels culls the triangle (counted in *culled_big, a nullable device uint64
 *     that the caller zeroes) -- the bound on every lane's loop, and the rule that a sheet stretched across a depth edge is no surface;
 *   - for the directed edge a -> b, E(px, py) = (Xb - Xa)(16 py - Ya) - (Yb - Ya)(16 px - Xa) in int64: E0 of 1 -> 2, E1 of 2 -> 0,
 *     E2 of 0 -> 1, so E0 + E1 + E2 = A.  A pixel is covered when every Ei > 0, or Ei = 0 on a top-left edge: one with Yb < Ya, or
 *     Yb = Ya and Xb > Xa.  A pixel centre on an edge shared by two triangles is thus drawn by exactly one of them;
 *   - depth = fp32(A) / ((fp32(E0) / z0' + fp32(E1) / z1') + fp32(E2) / z2') with /z' = multiplication by the rounded 1.0f / Xc.z of
 *     that vertex: perspective-correct, every operation rounded on its own; a pixel whose depth is not finite is skipped;
 *   - key = (bit pattern of depth) << 32 | index, agent-scope 64-bit unsigned atomic min: nearest wins, then the lowest index,
 *     whatever the arrival order, among points and triangles alike; sp3_render_resolve reads the buffer unchanged.
 *   nfaces = 0 is a no-op. */
int64_t sp3_mesh_faces_ws_bytes(int t, int h, int w);
int sp3_mesh_faces(const uint8_t* valid, const float* conf, float conf_thresh, const float* pts, int t, int h, int w, int both_windings,
                   void* ws, int32_t* faces, int32_t* colour_px, int32_t* counts, void* stream);
int64_t sp3_mesh_vertices_ws_bytes(int64_t n);
int sp3_mesh_compact_vertices(const float* pts, const uint32_t* rgba, int64_t n, int32_t* faces, int64_t nfaces, const uint8_t* valid,
                              const float* conf, float conf_thresh, float scale, const float* transform16, void* ws, float* out_pos,
                              uint32_t* out_rgba, int32_t* count, float* minmax, void* stream);
int sp3_render_tris(const float* pts, int64_t nverts, const int32_t* faces, const int32_t* colour_px, int64_t nfaces,
                    const int32_t* nfaces_dev, int64_t index_base, const sp3_render_cam* cam, int max_bbox_px, uint64_t* keys,
                    uint64_t* culled_big, void* stream);

/* ------------------------------------------------------------------------------------------
 * RGB-D views (dust3r/datasets/base/base_stereo_view_dataset.py:63-119,143-194,215-220; dust3r/datasets/utils/cropping.py:54-112;
 * dust3r/utils/geometry.py:165-217; the sanitising of spann3r/datasets/seven_scenes.py:123-126; spann3r_amd/views.py drives this).
 * The depth side of a whole sequence in ONE launch: raw depth maps -> `depthmap`, `pts3d` (world) and `valid_mask` of every view,
 * all views landscape and of one common size.  The entry point neither allocates nor synchronises.
 *
 * Per view a descriptor (below).  For output pixel (x, y) of the view's own orientation, 0 <= x < w, 0 <= y < h:
 *   index   : xr = x + l2, yr = y + t2 (second crop, in the resized W2 x H2 image), then nearest-neighbour resize from the W1 x H1
 *             window of the first crop by OpenCV's INTER_NEAREST rule for a given dsize:  ifx = 1.0 / ((double)W2 / W1),
 *             sx = min((int)floor(xr * ifx), W1 - 1), every operation in double; the same rule for y.  The raw value is read at
 *             column crop_l + sx, row crop_t + sy; no intermediate image exists.  (This is not floor(xr * W1 / W2): the two differ
 *             e.g. for W1 = 36, W2 = 20 at xr = 15.)  Parity unpinned vs cv2: cv2 is not in the build image, the rule is restated.
 *   sanitise: raw (uint16 or fp32) converted to fp32; raw == raw_invalid (when use_raw_invalid) -> 0; z = raw / depth_div, an fp32
 *             DIVISION; z not finite -> 0; z > max_depth -> 0; z < min_depth -> 0.
 *   unproject: x_cam = fp32(((double)x - cu) * z / fu), y_cam = fp32(((double)y - cv) * z / fv), every operation in double and ONE
 *             rounding to fp32 (what numpy does for an int64 grid and fp32 scalars); z_cam = z.
 *   world   : X_i = ((R_i0 x_cam + R_i1 y_cam) + R_i2 z_cam) + t_i in fp32, every operation rounded on its own; R | t = the 3x4
 *             cam2world matrix, row-major in `pose`.
 *   mask    : z > 0 and the three world coordinates finite.
 *   store   : at [y, x] of the view's [h, w] maps, or at [x, y] of [w, h] maps when `transpose` (a portrait view rectified to
 *             landscape): depth fp32 [n, out_h, out_w], pts fp32 [n, out_h, out_w, 3], mask uint8 [n, out_h, out_w] (0 / 1), and, when
 *             xcam is non-null, the camera-frame point fp32 [n, out_h, out_w, 3].  (out_h, out_w) = (h, w), or (w, h) if transposed.
 * descs_host and descs_dev hold the same n descriptors; the host copy is only read for the geometry checks of the call (every
 * window inside its source, every view of the common output size).  n = 0 is a no-op. */
typedef struct sp3_view_desc {
  const void* src;          /* device: raw depth, row-major */
  int64_t row_stride;       /* in elements */
  int32_t dtype;            /* 0 = uint16, 1 = fp32 */
  int32_t src_w, src_h;
  int32_t crop_l, crop_t, W1, H1;
  int32_t W2, H2;
  int32_t l2, t2;
  int32_t w, h;
  int32_t transpose;
  float fu, fv, cu, cv;
  float pose[12];
  int32_t use_raw_invalid;
  float raw_invalid, depth_div, min_depth, max_depth;
} sp3_view_desc;
int sp3_view_depth(const sp3_view_desc* descs_host, const sp3_view_desc* descs_dev, int n, int out_h, int out_w, float* depth,
                   float* pts, uint8_t* mask, float* xcam, void* stream);
/* sp3_eval_align : the alignment of the reference's eval.py:128-168 and the masked clouds of :189-191.  pred fp32 [m, B, HW, 3]
 * (camera of view 0), gt fp32 [n, B, HW, 3] (world), pose0 fp32 [B, 16] (cam2world of view 0), stats fp32 [B, 4] = gt_shift_z,
 * pred_shift_z, gt_scale, pred_scale (sp3_ssi_align_stats), all on the device.  Per point, in double from the fp32 inputs and
 * rounded to fp32 once:
 *   pred: (x, y, z - pred_shift_z) * (gt_scale / pred_scale);   gt: pose0^-1 applied, then z - gt_shift_z
 *   -- with to_world = 0 that is what Regr3D_t_ScaleShiftInv(norm_mode=False, gt_scale=True).get_all_pts3d_t returns;
 *   to_world = 1: z + gt_shift_z, then pose0 applied: both stacks in the world of the ground truth (eval.py:152-156).
 * pred_out / gt_out have the shapes of pred / gt.  With mask non-null (uint8 [n, HW]; needs B = 1 and m = n): images fp32
 * [n, HW, 3] = (img + 1) / 2 of img fp32 [n, 3, HW], and the points p with mask[p] > 0 in row-major order over (frame, row, column)
 * -- the order matters, ICP and the k-NN normals break ties by index -- written densely: cloud_pred, cloud_gt, cloud_rgb fp32
 * [count, 3] (room for n HW points each), cloud_src int32 [count] = p, count int32 [1].  ws: sp3_eval_align_ws_bytes(n HW) bytes of
 * device scratch, 4-byte aligned.  The compaction is the tile count / single-workgroup scan / scatter of the pointmap meshes. */
int64_t sp3_eval_align_ws_bytes(int64_t npts);
int sp3_eval_align(const float* pred, int m, const float* gt, int n, int B, int HW, const float* pose0, const float* stats, int to_world,
                   float* pred_out, float* gt_out, const uint8_t* mask, const float* img, void* ws, float* images, float* cloud_pred,
                   float* cloud_gt, float* cloud_rgb, int32_t* cloud_src, int32_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * TSDF fusion (spann3r_amd/fusion.py drives these; csrc/fusion.hip).  One welded surface per reconstruction: a truncated signed
 * distance volume integrated from depth maps or world pointmaps, and the indexed triangle mesh of its zero level by marching
 * tetrahedra.  There is no reference implementation of either stage (the reference's eval.py:241 ends in the comment
 * "Get depth from pcd and run TSDFusion"); the rules below are the contract and tests/fusion_ref.py restates them in numpy.
 * No entry point allocates, frees or synchronises.  Every fp32 operation is rounded on its own and sums run left to right.
 *
 * Volume: nx x ny x nz voxels, voxel (i, j, k) at linear index (k ny + j) nx + i; its centre is (origin.x + fp32(i) * voxel,
 *   origin.y + fp32(j) * voxel, origin.z + fp32(k) * voxel): one rounded multiply, one rounded add.  origin3 is a HOST pointer to
 *   three finite fp32; voxel and trunc are finite and > 0.  State: tsdf fp32 [n] (initial 1), weight fp32 [n] (initial 0), rgb fp32
 *   [n, 3] in [0, 1] (nullable: no colours).  Vertex and face indices are int32: 7 n < 2^31 (sp3_tsdf_extract, whose face counter
 *   can reach 12 per cell: 12 n < 2^31).  n = 0 is a no-op.
 *
 * sp3_tsdf_integrate: T frames into the volume in ONE launch.  frames_host and frames_dev hold the same T descriptors; the host
 *   copy is only read for the checks of the call.  A frame has either depth (fp32, camera z) or pts (fp32 world points, 3 per pixel)
 *   -- exactly one -- and nullable valid, pixel_weight and rgba maps; pixel (px, py) of every map of a frame is element
 *   p = py * row_stride + px (pts: 3 p .. 3 p + 2).  With rgb non-null every frame needs rgba (packed as sp3_pack_rgba8 packs);
 *   with rgb null rgba is ignored.  M = w2c, the 3 x 4 world-to-camera matrix, row-major.
 *   One lane owns one voxel, loads its state once, walks the frames in table order and stores the state once.  Per frame, for the
 *   voxel centre (x, y, z):
 *     Xc_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 (sp3_view_depth's world step);  skip unless Xc.z > 0;
 *     u = fu * Xc.x / Xc.z + cu, v = fv * Xc.y / Xc.z + cv (multiply, divide, add);  px = floor(u + 0.5), py = floor(v + 0.5);
 *     skip unless 0 <= px < w and 0 <= py < h (compared in fp32, a NaN fails);  skip if valid[p] == 0;
 *     d = depth[p], or from pts[p] = (X, Y, Z): d = ((M_20 X + M_21 Y) + M_22 Z) + M_23;  skip if d is not finite or d <= 0;
 *     s = d - Xc.z;  skip if s < -trunc;  f = min(1, s / trunc) (a division);
 *     a = pixel_weight[p], or 1;  skip unless a > 0 and finite;
 *     W' = weight + a;  tsdf = (weight * tsdf + a * f) / W';  with colours, per channel c of rgba: rgb_c = (weight * rgb_c + a * q) / W',
 *     q = fp32(byte c) / 255;  weight = W'.
 *   No atomics, no workgroup waits on another.  The state between two frames is the fp32 state a call would store, so two calls with
 *   frames A then B give the bits of one call with A followed by B.  T = 0 is a no-op.
 *
 * sp3_tsdf_extract: marching tetrahedra.  Inside means tsdf < 0 (0 is outside).  Voxel v is observed when weight[v] >= min_weight
 *   (min_weight > 0).  Corner code of a cube: c = dx + 2 dy + 4 dz.
 *   Cells: cell v is the cube of the voxels v + (dx, dy, dz), for i < nx - 1, j < ny - 1, k < nz - 1; it is live when all 8 are
 *     observed.  Every cell is cut into the 6 tetrahedra of the Kuhn triangulation around the diagonal 0-7, in this order and vertex
 *     order (corner codes; each has det(v1 - v0, v2 - v0, v3 - v0) > 0):
 *       T0 = (0, 1, 3, 7), T1 = (0, 5, 1, 7), T2 = (0, 3, 2, 7), T3 = (0, 2, 6, 7), T4 = (0, 4, 5, 7), T5 = (0, 6, 4, 7).
 *   Vertices: a tetrahedron edge joins two voxels whose offsets differ by one of 7 steps; it belongs to its endpoint a with the
 *     lower linear index, in slot 0..6 = +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z.  Slot s of voxel a carries a vertex when the other
 *     endpoint b lies in the volume, a and b are both observed and exactly one of them is inside (so a vertex on an edge that no
 *     live cell uses may be emitted; sp3_mesh_compact_vertices drops it).  The vertex: t = tsdf_a / (tsdf_a - tsdf_b), per coordinate
 *     p = p_a + t * (p_b - p_a) with p_a, p_b the voxel centres by the rule above; colour per channel c = rgb_a + t * (rgb_b - rgb_a),
 *     packed as sp3_pack_rgba8 packs (rgb null: 0xffffffff).  Vertices are written densely in (owner index, slot) order: vertices
 *     fp32 [V, 3], rgba uint32 [V] (nullable).
 *   Faces: per live cell in index order, per tetrahedron T0..T5, with m the vertices (positions 0..3 of the tetrahedron) that are
 *     inside.  "(a, b, c, d) even" means the permutation has an even number of inversions.  P_xy = the vertex on the edge between
 *     tetrahedron vertices x and y.
 *       none or all inside: nothing.
 *       one inside (lone = it) or one outside (lone = it): the other three in increasing position (a, b, c); swap b and c unless
 *         (lone, a, b, c) is even; swap them once more if the lone vertex is the outside one; one triangle (P_lone,a, P_lone,b, P_lone,c).
 *       two inside (m < n) and two outside (q < r): swap q and r unless (m, n, q, r) is even; two triangles (P_mq, P_mr, P_nr) and
 *         (P_mq, P_nr, P_nq).
 *     With linear interpolation every triangle's normal ((p1 - p0) x (p2 - p0)) then points to the positive (outside) side.  The cut
 *     is the same in every cell, so faces of neighbouring cells match and the surface is closed wherever the cells are live; all
 *     cells that share an edge share its one vertex: the mesh is welded by construction.  faces int32 [F, 3] are written densely in
 *     (cell index, tetrahedron, triangle) order and hold rows of `vertices`.
 *   counts int32 [2] = V, F, the true totals.  Nothing is written at or beyond row max_vertices of vertices / rgba or row max_faces
 *     of faces (a face within capacity may name a vertex beyond it): the caller compares, allocates and calls again.
 *   Both compactions are the tile count / single-workgroup scan / scatter of csrc/scan.h (6 launches in all).  ws: device scratch of
 *     sp3_tsdf_extract_ws_bytes(), 16-byte aligned: a 7-bit edge mask and one exclusive vertex offset per voxel (5 n bytes), and
 *     the two tile tables; a face finds a vertex as offset[owner] + popcount(mask[owner] below its slot). */
typedef struct sp3_tsdf_frame {
  const float* depth;          /* device fp32 [h, row_stride], camera z; or null */
  const float* pts;            /* device fp32 [h, row_stride, 3], world points; or null */
  const uint8_t* valid;        /* nullable */
  const float* pixel_weight;   /* nullable */
  const uint32_t* rgba;        /* nullable (required when the volume has colours) */
  int64_t row_stride;          /* in pixels, common to the maps of the frame */
  int32_t w, h;
  float fu, fv, cu, cv;
  float w2c[12];
} sp3_tsdf_frame;
int sp3_tsdf_integrate(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, int nx, int ny, int nz,
                       const float* origin3, float voxel, float trunc, float* tsdf, float* weight, float* rgb, void* stream);
int64_t sp3_tsdf_extract_ws_bytes(int nx, int ny, int nz);
int sp3_tsdf_extract(const float* tsdf, const float* weight, const float* rgb, int nx, int ny, int nz, const float* origin3, float voxel,
                     float min_weight, void* ws, int64_t max_vertices, int64_t max_faces, float* vertices, uint32_t* rgba, int32_t* faces,
                     int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * TSDF ray-casting and frame-to-model tracking (spann3r_amd/fusion.py drives these; csrc/raycast.hip): the zero level of a volume
 * of "TSDF fusion" seen from cameras with no meshing, and the KinectFusion step that registers a frame to the model before it is
 * integrated.  Neither stage has a reference implementation; the rules below are the contract and tests/raycast_ref.py restates
 * them in numpy.  No entry point allocates, frees or synchronises.
 *
 * sp3_tsdf_raycast: T views of one volume in ONE launch.  views_host and views_dev hold the same T descriptors; the host copy is
 *   only read for the checks of the call.  The volume is given as to sp3_tsdf_integrate (tsdf, weight, nullable rgb; read only).
 *   A view writes depth (required) and the nullable vertex, normal and rgba maps; pixel (px, py) of every map is element
 *   p = py * row_stride + px (vertex, normal: 3 p .. 3 p + 2); nothing is written at columns >= w of a row.  rgba non-null while
 *   rgb is null is an error.  c2w = the row-major 3 x 4 camera-to-world matrix: R its 3 x 3 part, eye its last column.
 *   0 <= near <= far, far may be +inf; fu, fv not 0; min_weight > 0; step (metric) > 0 and finite.  T <= 65535.
 *   cap = ceil(2 (nx + ny + nz) * voxel / step), computed by the callee in double from the fp32 voxel and step, is a hard bound on
 *   the samples of a ray (cap > 2^24 is an error): no input makes a lane loop without end.  T = 0 and n = 0 are no-ops.
 *   Every fp32 operation is rounded on its own, sums run left to right, division and square root are IEEE; min / max of two
 *   numbers are comparisons (b < a ? b : a).  One lane owns one pixel (px, py):
 *   Ray:  xn = (fp32(px) - cu) / fu, yn = (fp32(py) - cv) / fv;  dir_r = (R_r0 xn + R_r1 yn) + R_r2;
 *     len = sqrt((dx^2 + dy^2) + dz^2), dl = step / len.  The ray parameter lambda is camera z; the point at lambda is
 *     eye_r + dir_r * lambda (one multiply, one add).
 *   Box:  the voxel-centre lattice, lo_a = origin_a, hi_a = origin_a + fp32(n_a - 1) * voxel.  Per axis a = x, y, z: if dir_a == 0
 *     the axis constrains nothing when lo_a <= eye_a <= hi_a and the ray misses otherwise; else q1 = (lo_a - eye_a) / dir_a,
 *     q2 = (hi_a - eye_a) / dir_a, enter = max(enter, min(q1, q2)), exit = min(exit, max(q1, q2)), from -inf and +inf.
 *     lambda0 = max(enter, near), lambda1 = min(exit, far); the ray misses unless lambda0 <= lambda1 (a NaN fails).
 *   Samples:  lambda_i = lambda0 + fp32(i) * dl for i = 0, 1, .. while lambda_i <= lambda1 and i < cap; each recomputed from i.
 *   Cell of a point p:  g_a = (p_a - origin_a) / voxel, i_a = floor(g_a);  valid when 0 <= i_a <= n_a - 2 on every axis (compared in
 *     fp32, a NaN fails) and all eight corners (i + dx, j + dy, k + dz) have weight >= min_weight.  t_a = g_a - fp32(i_a).  Value:
 *     trilinear in lerp form a + t (b - a): along x on the four x-edges, then along y, then along z.
 *   March, with state (prev_valid = false, f_prev):  an invalid sample clears prev_valid.  A valid sample with value f:
 *     prev_valid and f_prev >= 0 and f < 0: a hit, lambda* = lambda_{i-1} + dl * (f_prev / (f_prev - f)), stop;
 *     prev_valid and f_prev < 0 and f >= 0: a back face, stop, a miss;  otherwise f_prev = f, prev_valid = true.
 *   At a hit:  p* = eye + dir * lambda*; its cell is evaluated again by the same rule and an invalid cell makes the pixel a miss.
 *     Gradient of the same interpolant: d/dx = the four x-edge differences (v1jk - v0jk) lerped along y, then z; d/dy = the four
 *     y-edge differences lerped along x, then z; d/dz = the four z-edge differences lerped along x, then y.
 *     normal = grad / sqrt((gx^2 + gy^2) + gz^2); a zero or non-finite length makes the pixel a miss.  The normal points to the
 *     positive (outside) side, as the faces of sp3_tsdf_extract do.  Colour: per channel the same trilinear lerps of rgb, packed as
 *     sp3_pack_rgba8 packs.
 *   Outputs:  hit: depth = lambda*, vertex = p*, normal, rgba;  miss: depth 0, vertex and normal 0, rgba 0.
 *   A workgroup is a 16 x 16 pixel block of one view (a wave: an 8 x 8 tile); no atomics, no workgroup waits on another.
 *
 * sp3_tsdf_track_accum: the normal equations of projective point-to-plane registration of ONE frame against the ray-cast maps of
 *   the model, in fp64 and a fixed order (per-workgroup partials in ws, a last launch adds them in index order; the scheme of
 *   sp3_icp_accum).  pts fp32 [n, 3] = the frame's world points, valid uint8 [n] (nullable), T12 = the correction under refinement
 *   and w2c12 = the world-to-camera matrix of the model view, both DEVICE double [12], row-major R (9) | t (3) as sp3_pnp_gn_accum
 *   takes its pose; vertex, normal, depth = the model view's maps of sp3_tsdf_raycast with w, h, row_stride, fu, fv, cu, cv.
 *   Per point p with valid != 0, in double from the fp32 inputs:  y = R p + t, skip a non-finite p;  yc = M y, skip unless yc.z > 0;
 *     u = fu yc.x / yc.z + cu, v = fv yc.y / yc.z + cv;  px = floor(u + 0.5), py = floor(v + 0.5), skip unless 0 <= px < w and
 *     0 <= py < h;  skip if depth there is 0;  q, nrm = vertex, normal there;  d = y - q, skip unless d.d <= dist_max^2;
 *     r = nrm.d,  J = (y x nrm, nrm): the parameters are (omega, delta) of y' = y + omega x y + delta, the left perturbation of
 *     sp3_pnp_gn_accum.  There is no normal-compatibility gate: the frame has no normals of its own.
 *   out29 = J^T J (21: upper triangle, row-major), J^T r (6), sum r^2, the number of pairs.  n = 0 gives zeros.
 *   ws: device scratch of sp3_tsdf_track_accum_ws_bytes(n). */
typedef struct sp3_tsdf_view {
  float* depth;                /* device fp32 [h, row_stride], camera z of the hit, 0 = miss */
  float* vertex;               /* device fp32 [h, row_stride, 3], world; nullable */
  float* normal;               /* device fp32 [h, row_stride, 3], unit, outward; nullable */
  uint32_t* rgba;              /* nullable (needs a volume with colours) */
  int64_t row_stride;          /* in pixels, common to the maps of the view */
  int32_t w, h;
  float fu, fv, cu, cv;
  float c2w[12];
  float near, far;
} sp3_tsdf_view;
int sp3_tsdf_raycast(const sp3_tsdf_view* views_host, const sp3_tsdf_view* views_dev, int T, int nx, int ny, int nz, const float* origin3,
                     float voxel, const float* tsdf, const float* weight, const float* rgb, float min_weight, float step, void* stream);
int64_t sp3_tsdf_track_accum_ws_bytes(int64_t n);
int sp3_tsdf_track_accum(const float* pts, const uint8_t* valid, int64_t n, const double* T12, const float* vertex, const float* normal,
                         const float* depth, int w, int h, int64_t row_stride, float fu, float fv, float cu, float cv, const double* w2c12,
                         float dist_max, void* ws, double* out29, void* stream);

/* ------------------------------------------------------------------------------------------
 * Brick TSDF volume (spann3r_amd/fusion.py BrickTSDFVolume drives these; csrc/bricks.hip): the volume of "TSDF fusion" on two
 * levels, so that a session can fuse inside a generous virtual box without holding its voxels: a table of 8 x 8 x 8-voxel bricks,
 * allocated where depth measurements land, and a pool that holds only those bricks.  There is no reference implementation;
 * tests/bricks_ref.py restates mark, alloc, integrate and to_dense in numpy, and the dense kernels above are the anchor of the
 * integration and of the ray-caster.  No entry point allocates, frees or synchronises.  Every fp32 operation is rounded on its own
 * and sums run left to right.  No atomics; no workgroup waits on another.
 *
 * Layout: the virtual grid is nx x ny x nz voxels, every dimension a multiple of 8 (anything else is an error); voxel centres follow
 *   the dense rule, origin_a + fp32(i_a) * voxel.  The brick grid is bx = nx / 8, by = ny / 8, bz = nz / 8; brick (I, J, K) has
 *   linear index (K by + J) bx + I.  table int32 [bx by bz]: -1 = absent, otherwise a pool slot.  slot_brick int32 [capacity]: the
 *   linear brick index of a slot.  Pool: tsdf fp32 [capacity, 512], weight fp32 [capacity, 512], rgb fp32 [capacity, 512, 3]
 *   (nullable: no colours); voxel (i, j, k) lives in the brick (i >> 3, j >> 3, k >> 3) at place (k & 7) 64 + (j & 7) 8 + (i & 7).
 *   count: DEVICE int32 [1], the slots in use.  The voxels of an absent brick read as tsdf 1, weight 0, rgb 0: that is "the
 *   densified volume" below.  bx by bz + capacity + 256 must stay below 2^31 (int32 brick indices, slots, the scan's tile table and
 *   `need`), a side below 2^20 voxels; pool indices are 64-bit.
 *
 * sp3_tsdf_brick_mark: T frames (T <= 65535) in ONE launch, a lane owns a pixel.  The frames are sp3_tsdf_frame as
 *   sp3_tsdf_integrate takes them (rgba is ignored); c2w_dev is a device fp32 [T, 12] array of row-major 3 x 4 camera-to-world
 *   matrices (R | eye), read for frames with depth only (required when there is one).  A pixel (px, py) counts when it passes the
 *   pixel tests of the integrate rule: valid[p] != 0, d finite and > 0 (d = depth[p], or from pts[p] by the frame's w2c as there),
 *   pixel_weight[p] > 0 and finite.  Its point P: for a pts frame the point itself; for a depth frame
 *     xn = (fp32(px) - cu) / fu, yn = (fp32(py) - cv) / fv, Xc = (xn * d, yn * d, d), P_r = ((R_r0 Xc.x + R_r1 Xc.y) + R_r2 Xc.z) + eye_r.
 *   A non-finite P is skipped.  band is metric, > 0 and at most 8 voxel.  Per axis a:
 *     lo_a = floor(((P_a - band) - origin_a) / voxel),  hi_a = floor(((P_a + band) - origin_a) / voxel) + 1  (in fp32);
 *     the pixel is skipped unless hi_a >= 0 and lo_a <= n_a - 1 on every axis (a NaN fails); then lo_a and hi_a are clamped to
 *     [0, n_a - 1] and flags[brick] = 1 for every brick of lo_a >> 3 .. hi_a >> 3 on each axis (at most 4 per axis, 3 when band
 *     stays below 7 voxels).  flags is uint8 [bx by bz]; the writes are plain stores of the same value, so the result does not depend
 *     on order.  mark never clears a flag.  T = 0 is a no-op.
 *
 * sp3_tsdf_brick_alloc: order-preserving, all or nothing.  A brick is new when its flag is set and its table entry is -1.  With
 *   need = count + the number of new bricks:  need <= capacity: every new brick, in linear brick order, gets slot count + its
 *   exclusive rank among the new bricks; table and slot_brick are filled, the 512 voxels of the slot are set to tsdf 1, weight 0,
 *   rgb 0, all flags are cleared and count = need.  need > capacity: nothing is written to flags, table, slot_brick, the pool or
 *   count, so the caller grows the pool (copying the slots in use) and calls alloc again without marking again.  In both cases
 *   counts2 int32 [2] = (count after the call, need).  It is the tile count / single-workgroup scan / scatter of csrc/scan.h plus
 *   the slot initialisation and one single-lane launch that alone changes count (5 launches).  ws: device scratch of
 *   sp3_tsdf_brick_alloc_ws_bytes(), 16-byte aligned.
 *
 * sp3_tsdf_brick_integrate: T frames into the slots 0 .. n_bricks - 1 in ONE launch; n_bricks is the count the host read from
 *   counts2 (that one read-back per call is accepted).  A workgroup owns a brick and a lane a voxel: it loads its state once, walks
 *   the frames in table order and stores once.  The per-frame rule is the text of sp3_tsdf_integrate, word for word, on the voxel's
 *   centre by the dense rule: an allocated voxel ends with the bits sp3_tsdf_integrate gives the same voxel of the same grid after
 *   the same frames.  (A brick allocated by a later call starts from tsdf 1, weight 0 then: what earlier frames would have
 *   contributed to it is not there.)  T = 0 and n_bricks = 0 are no-ops.
 *
 * sp3_tsdf_brick_raycast: the rule of sp3_tsdf_raycast on the densified volume of the virtual grid: the same sp3_tsdf_view table,
 *   cap (from the virtual dims), workgroup shape and outputs; a corner in an absent brick is unobserved.  One freedom is added: a
 *   lane may pass over samples it can prove invalid without evaluating them -- every sample is recomputed from its index, so later
 *   samples do not change, and an invalid sample only clears prev_valid.  The proof used: corner 0 of a sample's cell lies in an
 *   absent brick, and so does corner 0 of a later sample; the lattice coordinates of corner 0 are monotone in the sample index
 *   (every rounded operation of the sample rule is monotone), so every sample in between has its corner 0 in that brick as well.
 *   The brick table is the only skip structure; nothing approximate decides a skip.
 *
 * sp3_tsdf_brick_to_dense: the densified volume of a box of voxels: lo3, size3 HOST int32 [3] with 0 <= lo_a, lo_a + size_a <= n_a
 *   and 7 sx sy sz < 2^31; out_tsdf, out_weight fp32 [sz, sy, sx], out_rgb fp32 [sz, sy, sx, 3] (nullable; needs a pool with
 *   colours).  A lane owns a voxel of the box: allocated voxels are copied, absent ones set to (1, 0, 0).  This is how a brick volume
 *   reaches sp3_tsdf_extract.
 *
 * Errors, by the usual codes: a dimension that is not a multiple of 8; band outside (0, 8 voxel]; capacity or bx by bz over the
 *   index limit; a frame with both or neither of depth and pts; a frame without rgba while the pool has colours (integrate); rgba
 *   views on a pool without colours. */
int sp3_tsdf_brick_mark(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, const float* c2w_dev, int T, int nx, int ny,
                        int nz, const float* origin3, float voxel, float band, uint8_t* flags, void* stream);
int64_t sp3_tsdf_brick_alloc_ws_bytes(int nx, int ny, int nz);
int sp3_tsdf_brick_alloc(uint8_t* flags, int nx, int ny, int nz, int32_t* table, int32_t* slot_brick, int32_t* count, int64_t capacity,
                         float* tsdf, float* weight, float* rgb, void* ws, int32_t* counts2, void* stream);
int sp3_tsdf_brick_integrate(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, int nx, int ny, int nz,
                             const float* origin3, float voxel, float trunc, const int32_t* slot_brick, int n_bricks, float* tsdf,
                             float* weight, float* rgb, void* stream);
int sp3_tsdf_brick_raycast(const sp3_tsdf_view* views_host, const sp3_tsdf_view* views_dev, int T, int nx, int ny, int nz,
                           const float* origin3, float voxel, const int32_t* table, const float* tsdf, const float* weight, const float* rgb,
                           float min_weight, float step, void* stream);
int sp3_tsdf_brick_to_dense(int nx, int ny, int nz, const int32_t* table, const float* tsdf, const float* weight, const float* rgb,
                            const int32_t* lo3, const int32_t* size3, float* out_tsdf, float* out_weight, float* out_rgb, void* stream);

/* ------------------------------------------------------------------------------------------
 * Brick mesh extraction (spann3r_amd/fusion.py BrickTSDFVolume.extract_raw drives it; csrc/brick_mesh.hip): marching tetrahedra on
 * the pool of "Brick TSDF volume" itself.  Work and scratch follow the allocated bricks: there is no dense intermediate and the
 * extent of the virtual grid does not enter.  tests/brick_mesh_ref.py restates it in numpy.  The call does not allocate, free or
 * synchronise; its only read-back is the caller's read of counts.  No atomics; no workgroup waits on another.
 *
 * sp3_tsdf_brick_extract: the rule of sp3_tsdf_extract ("TSDF fusion" above) on the densified volume of the WHOLE virtual grid --
 *   absent voxels read tsdf 1, weight 0, so they are unobserved.  Taken from there word for word: observed (weight >= min_weight,
 *   min_weight > 0) and inside (tsdf < 0); the corner code and the 6 Kuhn tetrahedra T0..T5; the 7 edge slots and their owner (the
 *   endpoint with the lower coordinates); when a slot carries a vertex (the other endpoint lies in the grid, both are observed,
 *   exactly one is inside -- whether or not a live cell uses the edge); t, the vertex formula and the colour formula (rgb null:
 *   0xffffffff; rgba nullable); the face cases and their orientation; counts int32 [2] = the true V and F; nothing is written at or
 *   beyond row max_vertices of vertices / rgba or row max_faces of faces (a face within capacity may name a vertex beyond it).
 *   Two points differ:
 *   Positions: voxel centres are the virtual grid's, origin_a + fp32(i_a) * voxel with i_a the index in the virtual grid -- the
 *     centre sp3_tsdf_brick_integrate used, not the shifted origin a box of sp3_tsdf_brick_to_dense would give the dense kernel.
 *   Order: by pool slot.  Vertices are written densely in (slot, place in the brick, edge slot) order, place = (k & 7) 64 +
 *     (j & 7) 8 + (i & 7) as in the pool; faces in (slot of the brick of the cell's corner 0, place of corner 0, tetrahedron,
 *     triangle) order.  Only a cell whose corner 0 lies in an allocated brick can be live and only an allocated voxel can own a
 *     vertex, so the work set is the slots 0 .. n_bricks - 1 (n_bricks: the count the host read from counts2 of
 *     sp3_tsdf_brick_alloc) and nothing else.  The output is deterministic: the same pool gives the same bits every call.
 *   table, slot_brick and the pool are those of "Brick TSDF volume"; a table entry >= n_bricks counts as absent.  Vertex and face
 *   indices are int32: 12 * 512 * n_bricks < 2^31, anything more is an error (checked before anything is launched).
 *   n_bricks = 0 writes counts = (0, 0) and launches nothing else.
 *   The launch structure is sp3_tsdf_extract's with a 256-voxel half brick as the scan tile (5 launches: one count of vertices and
 *   faces, two single-workgroup scans, two scatters).  A workgroup looks up the 7 `+` neighbours of its brick once (outside the
 *   grid or absent: unobserved) and stages the observed and inside bits of the 9 x 9 x 5 halo of its half brick in LDS; the edge
 *   mask, a cell's inside byte and its liveness come from there.  ws: device scratch of sp3_tsdf_brick_extract_ws_bytes(n_bricks),
 *   16-byte aligned: a 7-bit edge mask and one exclusive vertex offset per ALLOCATED voxel (5 * 512 * n_bricks bytes) and the two
 *   tile tables; a face finds a vertex as offset[owner] + popcount(mask[owner] below its slot), the owner through
 *   table -> slot -> slot * 512 + place. */
int64_t sp3_tsdf_brick_extract_ws_bytes(int n_bricks);
int sp3_tsdf_brick_extract(int nx, int ny, int nz, const float* origin3, float voxel, const int32_t* table, const int32_t* slot_brick,
                           int n_bricks, const float* tsdf, const float* weight, const float* rgb, float min_weight, void* ws,
                           int64_t max_vertices, int64_t max_faces, float* vertices, uint32_t* rgba, int32_t* faces, int32_t* counts,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh components (spann3r_amd/mesh.py components / filter_components drive these; csrc/mesh_components.hip): the connected pieces
 * of an indexed triangle mesh, so that the specks of a fused surface can be dropped on the device.  tests/mesh_components_ref.py
 * restates the rule in numpy.  No entry point allocates, frees or synchronises; `ws` is caller-provided device scratch of the
 * matching sp3_*_ws_bytes(), 16-byte aligned.  Indices are int32: nverts, nfaces and ncomponents must stay below 2^31 - 1 (checked
 * before anything is launched).  All outputs are integers and functions of the graph alone: two runs give the same bits, and a
 * permuted face list gives the same vertex_component and the face_component permuted alike.
 *
 * The rule.  Vertices 0..V-1, faces int32 [F, 3].  A face is VALID when its three indices lie in 0..V-1; an invalid face is never
 *   dereferenced and counts nowhere but in info[1].  Two vertices are connected when a valid face names both -- vertex connectivity,
 *   so two fans that touch in one vertex are ONE component.  (Open3D's cluster_connected_triangles joins triangles across shared
 *   EDGES only and would report those fans as two clusters; on a mesh where every contact is along an edge the two agree.  Parity
 *   with it is unpinned: Open3D is not available to test against.)  A COMPONENT is a connectivity class with at least one valid
 *   face; a vertex that no valid face names belongs to none.  Components are numbered 0..C-1 by ascending smallest vertex index.
 *   A degenerate face (a == b) and a duplicated face are valid and count.
 * sp3_mesh_components :
 *   vertex_component int32 [V] = the component of the vertex, -1 for a vertex no valid face names;
 *   face_component int32 [F] = the component of the face's vertices, -1 for an invalid face;
 *   component_faces, component_vertices int32 [C] = valid faces and vertices per component; nothing is written at or beyond entry
 *     max_components of either (both may be null when max_components = 0);
 *   info int32 [2] = (C, the number of invalid faces): the true C, whatever the capacity.
 *   F = 0 or V = 0: C = 0, every vertex -1, every face -1 and invalid when V = 0.
 *   Labelling is a lock-free union-find with the root as the smallest index.  parent[v] = v at the start (a launch of its own);
 *   per valid face one lane hooks (a, b) and (a, c): find both roots, atomicCAS(&parent[hi], hi, lo) with hi the larger root and lo
 *   the smaller, on failure continue from the value the CAS returned; a later launch flattens, label[v] = find(v).  (Two vertices
 *   whose parent entries are equal hang under one vertex already: that hook ends there.)  Invariants:
 *   - parent[v] <= v always and an entry only ever decreases; every write to parent after the first launch is an agent-scope
 *     atomicCAS or atomicMin (the latter shortcuts a hooked vertex to the root just found).  Every chain walk therefore strictly
 *     descends and ends after at most v steps, a failed CAS restarts from a strictly smaller index, no input makes a lane loop
 *     without end, and no lane ever waits for another lane's store.  Trees only merge, and the root of a tree is its smallest vertex.
 *   - invalid faces are dropped before any walk starts: an index outside 0..V-1 never starts or extends a walk.
 *   - the L2s of the XCDs are not coherent and a CU's L1 is never refreshed: inside the hooking launch parent is read with
 *     agent-scope atomic loads, and the result does not depend on their freshness -- a load returns a value the entry held at some
 *     time, the vertex itself or a smaller vertex of its tree; a stale self-pointer only makes the next CAS fail, and the CAS
 *     returns the true value.  Launch boundaries are the only other hand-offs.
 *   - faces and vertices per root are counted with integer atomicAdd (deterministic), aggregated in the wave first because a
 *     typical mesh has nearly all faces in ONE component: peel by the first active lane's label, ballot the lanes that share it,
 *     one add of the popcount; at most 64 rounds.
 *   - dense ids: roots with a non-zero face count are flagged, counted per 256-vertex tile, scanned (one workgroup) and scattered.
 *   8 launches.  ws: four int32 per vertex (parent, the two counts, root -> id) and the tile table.
 * sp3_mesh_select_faces : face i is kept when c = face_component[i] lies in 0..ncomponents-1 and keep[c] != 0 (keep: device
 *   uint8 [ncomponents]); the kept rows of faces are written densely, in their original order and with their indices unchanged, to
 *   out_faces (room for nfaces rows); count[0] = the number kept.  Count per 256-face tile, scan, scatter.  The vertices then go
 *   through sp3_mesh_compact_vertices(faces = out_faces), which rewrites the indices and drops what nothing references.
 *   nfaces = 0 or ncomponents = 0 writes count = 0 and nothing else. */
int64_t sp3_mesh_components_ws_bytes(int64_t nverts);
int sp3_mesh_components(const int32_t* faces, int64_t nfaces, int64_t nverts, void* ws, int64_t max_components,
                        int32_t* vertex_component, int32_t* face_component, int32_t* component_faces, int32_t* component_vertices,
                        int32_t* info, void* stream);
int64_t sp3_mesh_select_faces_ws_bytes(int64_t nfaces);
int sp3_mesh_select_faces(const int32_t* faces, const int32_t* face_component, int64_t nfaces, const uint8_t* keep, int64_t ncomponents,
                          void* ws, int32_t* out_faces, int32_t* count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification (spann3r_amd/mesh.py cluster_vertices / simplify drive these; csrc/mesh_simplify.hip): vertex clustering on
 * a uniform grid, so that a fused surface has the triangle count its user chose and the overlapping per-frame sheets of
 * sp3_mesh_faces become one welded vertex set.  tests/mesh_simplify_ref.py restates the rule in numpy; Open3D's
 * simplify_vertex_clustering is not available to test against, so that restatement is the anchor (parity unpinned).  No entry point
 * allocates, frees or synchronises; `ws` is caller-provided device scratch of the matching sp3_*_ws_bytes(), 16-byte aligned.
 * Indices are int32: nverts and nfaces must stay below 2^31 - 1, and a table has 2^table_log2 slots, 1 <= table_log2 <= 31, MORE
 * slots than items (all checked before anything is launched).  Every output is a function of the input alone: the sums are
 * integers, so two runs give the same bits, whatever the order of the atomics, the table size or the hash function.
 *
 * The rule.  vertices fp32 [V, 3], rgba uint32 [V] (nullable), faces int32 [F, 3], origin3 HOST fp32 [3], cell > 0 and finite,
 *   inv = fp32(1) / cell computed on the host.
 *   1. Cell of a vertex.  Per axis u = (p - o) * inv, two separately rounded fp32 operations (no contraction: the file is compiled
 *      under `#pragma clang fp contract(off)`); i = floorf(u).  A vertex is USABLE when all three u are finite and |i| < 2^30; an
 *      unusable vertex belongs to no cluster (vertex_cluster = -1).  r = u - i, one rounded fp32 subtraction, and
 *      q = min((int)(r * 65536.0f), 65535), in 0..65535.  (u - i is exact unless -0.5 < u < 0, where 1 - |u| may round, for
 *      |u| <= 2^-25 up to r = 1; the min keeps q in range there.)
 *   2. Cluster.  The usable vertices that share (ix, iy, iz).  Clusters are numbered 0..C-1 by ascending smallest member vertex
 *      index, the convention of sp3_mesh_components.
 *   3. Representative.  Per axis pos = (float)((double)o + ((double)i + (double)Sq / (double)n / 65536.0) * (double)cell): Sq the
 *      unsigned 64-bit sum of the members' q, n the member count, every fp64 operation rounded on its own (no FMA), left to right as
 *      written.  Colour per byte, alpha included: (2 Sc + n) / (2 n) in integers (round half up), Sc in 64 bits.
 *   4. Faces.  A face is VALID when its three indices lie in 0..V-1 and name usable vertices; an invalid face is never dereferenced
 *      beyond the index check.  A valid face is remapped to cluster ids and dropped as COLLAPSED when two of its ids are equal.
 *      With dedup the survivors are grouped by their triple rotated so that the smallest id comes first -- rotation keeps the
 *      winding, so a face and its mirror image are two different faces -- and of each group the face with the lowest original index
 *      is kept.  Kept faces are written densely, in original order and in their original rotation.
 *   5. sp3_mesh_compact_vertices(faces = the kept faces) then drops the clusters no kept face names, renumbers and gives the bounds.
 *
 * The table.  Both groupings use the same lock-free open-addressing table of int32 slots.  A slot holds an ITEM index (a vertex, a
 *   face), not a key; the key of a slot is recomputed from the item it holds: for a vertex the cell of that vertex, for a face the
 *   rotated cluster triple read from the remapped-face buffer an earlier launch wrote.  So any V and C work without packing a key
 *   into 64 bits.  Insert: probe linearly from hash(key), wrapping at the end; read the slot with an agent-scope atomic load; if it
 *   is EMPTY, agent-scope atomicCAS(slot, EMPTY, me); if the slot then or already holds g with key(g) == key(me), atomicMin(slot, me)
 *   and stop (the atomicMin is skipped when g < me: the slot only decreases, so it is below me already); otherwise go on to the next
 *   slot.  Invariants:
 *   - a claimed slot never changes its key, and a slot's value only ever decreases, within one key;
 *   - a lane inserts only at the first EMPTY slot of its probe sequence, so one key owns exactly one slot, which ends at the
 *     smallest item of the key;
 *   - the table holds more slots than items, so every probe ends at a match or at an EMPTY slot (the loops are bounded by the
 *     table size all the same);
 *   - no lane waits for another lane's store, and a stale read only costs a failed CAS, which returns the true value (a stale item
 *     is one the slot held earlier: same key, not smaller than the current one);
 *   - the keys are immutable during the launch that hashes them.
 *   The L2s of the XCDs are not coherent and a CU's L1 is never refreshed: inside an insert launch only the atomics carry
 *   information, and launch boundaries are the only other hand-offs.  After the insert launch, in launches of their own, each item
 *   finds its slot again with plain loads; a vertex is its cluster's leader, and a face is kept, when the slot holds its own index;
 *   leader and kept flags are counted per 256-item tile, scanned (one workgroup) and scattered, which gives the dense ids and the
 *   dense face list in original order.
 *
 * sp3_mesh_cluster : positions fp32 [C, 3] and out_rgba [C] (null exactly when rgba is null) need room for nverts rows; only the
 *   first C are written.  vertex_cluster int32 [V].  info int32 [1] = C.  Members add q, the four colour bytes and 1 to their
 *   cluster's unsigned 64-bit sums with agent-scope atomic adds (one add per lane and sum; no aggregation in the wave).  7 launches.
 *   ws: the table, two int32 per vertex (leader -> id, id -> leader), the tile table and 64 bytes of sums per vertex of capacity
 *   (only the first C are touched).  nverts = 0 writes info = 0 and nothing else.
 * sp3_mesh_cluster_faces : vertex_cluster int32 [nverts] as sp3_mesh_cluster wrote it (any entry < 0: unusable).  out_faces int32
 *   needs room for nfaces rows; info int32 [4] = (kept, invalid, collapsed, duplicate), kept + invalid + collapsed + duplicate =
 *   nfaces.  dedup = 0: every survivor is kept, no table is used and table_log2 is ignored (pass 0 to the ws function too).
 *   6 launches (5 without dedup).  ws: the table, the remapped faces (12 bytes a face), one flag byte a face and the tile table.
 *   nfaces = 0 writes info = 0 and nothing else; nverts = 0 makes every face invalid. */
int64_t sp3_mesh_cluster_ws_bytes(int64_t nverts, int table_log2);
int sp3_mesh_cluster(const float* vertices, const uint32_t* rgba, int64_t nverts, const float* origin3, float cell, int table_log2,
                     void* ws, float* positions, uint32_t* out_rgba, int32_t* vertex_cluster, int32_t* info, void* stream);
int64_t sp3_mesh_cluster_faces_ws_bytes(int64_t nfaces, int table_log2);
int sp3_mesh_cluster_faces(const int32_t* faces, int64_t nfaces, const int32_t* vertex_cluster, int64_t nverts, int dedup, int table_log2,
                           void* ws, int32_t* out_faces, int32_t* info, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh surface sampling and normals (spann3r_amd/mesh.py face_frames / sample_surface / vertex_normals and
 * spann3r_amd/evaluate.py evaluate_meshes drive these; csrc/mesh_sample.hip): points drawn from the SURFACE of a mesh by area, each
 * with its face's exact normal, and area-weighted vertex normals -- so that a fused surface is scored on what it is and not on
 * where its tessellation put the vertices, and a viewer can light it.  tests/mesh_sample_ref.py restates the rule in numpy;
 * Open3D's sample_points_uniformly / compute_vertex_normals and trimesh's sample_surface are not available to test against, so that
 * restatement is the anchor (parity unpinned).  No entry point allocates, frees or synchronises; `ws` is caller-provided device
 * scratch of the matching sp3_*_ws_bytes(), 8-byte aligned like cum and info.  Indices are int32: nverts and nfaces must stay below
 * 2^31 - 1 (checked before anything is launched).  Every output is a function of the input alone: dmax is an integer maximum
 * over the bits of non-negative doubles, the prefix sum and the vertex sums are integers, the random numbers are a function of
 * (seed, sample index) -- two runs give the same bits, whatever the order of the atomics.  Every fp64 operation below is rounded
 * on its own, in the order written (no FMA: the file is compiled under `#pragma clang fp contract(off)`).
 *
 * The rule.  vertices fp32 [V, 3], rgba uint32 [V] (nullable), faces int32 [F, 3].
 *   1. Face frame.  A face is VALID when its three indices lie in 0..V-1; an invalid face is never dereferenced beyond that check.
 *      For a valid face with corners A, B, C converted to fp64: e1 = B - A, e2 = C - A,
 *      n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), d = sqrt(nx nx + ny ny + nz nz), summed left to right: twice
 *      the area.  An invalid face, or one whose d is not finite (a NaN or infinite corner), has d = 0 and n = 0.  The unit face
 *      normal is (float)(n / d) per component, (0, 0, 0) when d == 0.  dmax is the maximum d over all faces: the fp64 bits of
 *      non-negative finite doubles, read as unsigned 64-bit integers, order as the doubles do, so one agent-scope 64-bit atomicMax
 *      gives it exactly.
 *   2. Sampling weight.  w_f = (uint64) floor(d_f / dmax * 4294967296.0), 0 when d_f == 0; w_f <= 2^32.  cum is the INCLUSIVE
 *      prefix sum of w in face order, unsigned 64-bit; its total W stays below 2^63.  A face with w_f = 0 is never drawn: an
 *      invalid or degenerate one, and also a face below 2^-32 of the largest one.  The total area is reported as
 *      (double)W / 4294967296.0 * dmax / 2: the QUANTISED area, short of the sum of d / 2 by less than F dmax 2^-33.
 *   3. Random numbers, counter-based and stateless: h(c) = splitmix64 of z = seed + (c + 1) * 0x9E3779B97F4A7C15 modulo 2^64:
 *      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) * 0x94D049BB133111EB, h = z ^ (z >> 31).
 *   4. Sample k uses the counters 3k, 3k + 1, 3k + 2.  Face: t = umulhi64(h(3k), W), face = the smallest f with cum[f] > t (an
 *      upper-bound search; t < W, so it exists).  The draws are independent and identically distributed, as Open3D and trimesh
 *      draw theirs: no stratification.  Barycentric coordinates: a = h(3k + 1) >> 40 and b = h(3k + 2) >> 40, 24-bit integers;
 *      if a + b > 2^24 then a = 2^24 - a and b = 2^24 - b.  Point per axis: (float)((double)A + (a / 2^24 * e1 + b / 2^24 * e2)):
 *      two products, one sum, one sum, one narrowing.  Colour per byte, alpha included:
 *      (cA (2^24 - a - b) + cB a + cC b + 2^23) >> 24 in integers.  The normal of the sample is the unit face normal.
 *   5. Vertex normals, area-weighted.  Per valid face and component q = llrint(n_c / dmax * 1073741824.0), round half to even,
 *      |q| <= 2^30; q is added to each of the face's three vertices with agent-scope 64-bit integer atomic adds (two's complement
 *      on unsigned 64-bit; one add per lane and sum, no aggregation in the wave).  normal = (float)(S_c / sqrt(Sx Sx + Sy Sy + Sz Sz))
 *      with S converted to fp64, (0, 0, 0) when all three sums are 0 -- a vertex no valid face names, among others.
 *
 * sp3_mesh_face_frames : face_normals fp32 [F, 3] (nullable), cum uint64 [F], info uint64 [2] = (W, the bits of dmax).  5 launches:
 *   clear info; frames (d, the normal, the atomicMax; the bits of d wait in cum); weights and the scan inside every 256-face
 *   tile; one workgroup's scan of the tile totals; add-back.  ws: one uint64 per tile.  nfaces = 0 writes info = 0 and nothing else.
 * sp3_mesh_sample : reads cum and info (as sp3_mesh_face_frames wrote them for the SAME vertices and faces) from the device, so
 *   there is no host round trip between the two calls.  points, normals fp32 [N, 3], out_rgba uint32 [N] (null exactly when rgba
 *   is null), face_index int32 [N].  One launch, one lane per sample; nsamples = 0 launches nothing.  W == 0 with nsamples > 0 must
 *   not be launched (a launch then writes nothing): the caller reads info once, which also gives the area.  nsamples < 2^40.
 * sp3_mesh_vertex_normals : info from sp3_mesh_face_frames of the same mesh; normals fp32 [V, 3].  3 launches (clear, accumulate,
 *   finalise).  ws: 24 bytes of sums per vertex.  nverts = 0 launches nothing; nfaces = 0 gives zeros. */
int64_t sp3_mesh_face_frames_ws_bytes(int64_t nfaces);
int sp3_mesh_face_frames(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, void* ws, float* face_normals,
                         uint64_t* cum, uint64_t* info, void* stream);
int sp3_mesh_sample(const float* vertices, const uint32_t* rgba, int64_t nverts, const int32_t* faces, int64_t nfaces, const uint64_t* cum,
                    const uint64_t* info, int64_t nsamples, uint64_t seed, float* points, float* normals, uint32_t* out_rgba,
                    int32_t* face_index, void* stream);
int64_t sp3_mesh_vertex_normals_ws_bytes(int64_t nverts);
int sp3_mesh_vertex_normals(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const uint64_t* info, void* ws,
                            float* normals, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh distance (spann3r_amd/mesh.py TriangleGrid / point_mesh_distance and spann3r_amd/evaluate.py evaluate_meshes(exact=True)
 * drive these; csrc/mesh_distance.hip): the exact unsigned distance from a point to the SURFACE of a triangle mesh, with the closest
 * point, the face it lies on and the Voronoi region of that face -- so that a surface is scored against a surface and not against
 * the nearest of its samples.  tests/mesh_distance_ref.py restates the rule in numpy and is itself checked against a second
 * formulation in exact rationals; Open3D's RaycastingScene.compute_closest_points and trimesh's ProximityQuery are not available
 * to test against (parity unpinned).  No entry point allocates, frees or synchronises; `ws` is caller-provided device scratch of
 * sp3_mesh_dist_query_ws_bytes(nq), 16-byte aligned.  Indices are int32: nverts, nfaces and npairs stay below 2^31 - 1.  Every fp64
 * operation below is rounded on its own, in the order written (no FMA: the file is compiled under `#pragma clang fp contract(off)`);
 * dot(u, v) = (ux vx + uy vy) + uz vz.
 *
 * The rule.  vertices fp32 [V, 3], faces int32 [F, 3], a query p fp32 [3].
 *   1. A face is USABLE when its three indices lie in 0..V-1 and the d of sp3_mesh_face_frames (rule 1 of "Mesh surface sampling and
 *      normals": the length of the fp64 cross product of its two edges) is finite and > 0 -- which a NaN or infinite coordinate never
 *      gives.  A face that is not usable is never dereferenced beyond that test and never wins.
 *   2. Closest point c of a usable face (A, B, C) to p, everything converted to fp64 (Ericson, Real-Time Collision Detection 5.1.5):
 *      ab = B - A, ac = C - A, ap = p - A, bp = p - B, cp = p - C; d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp),
 *      d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4 (two products,
 *      one difference), e = d4 - d3, g = d5 - d6.  The FIRST of these tests that holds decides:
 *        region 0 (A)      : d1 <= 0 and d2 <= 0                  c = A
 *        region 1 (B)      : d3 >= 0 and d4 <= d3                 c = B
 *        region 2 (edge AB): vc <= 0 and d1 >= 0 and d3 <= 0      t = d1 / (d1 - d3), c = A + t ab
 *        region 3 (C)      : d6 >= 0 and d5 <= d6                 c = C
 *        region 4 (edge AC): vb <= 0 and d2 >= 0 and d6 <= 0      t = d2 / (d2 - d6), c = A + t ac
 *        region 5 (edge BC): va <= 0 and e >= 0 and g >= 0        t = e / (e + g), c = B + t (C - B)
 *        region 6 (inside) : otherwise                            den = 1 / ((va + vb) + vc), s = vb den, t = vc den,
 *                                                                 c = A + (ab s + ac t)
 *      per axis.  d2(p, face) = (dx dx + dy dy) + dz dz of p - c.  (A comparison with a NaN is false: a NaN query ends in region 6
 *      with d2 = NaN, which never wins.)
 *   3. The result of a query is the minimum over the usable faces of the pair (d2, face index), compared lexicographically,
 *      starting from (+inf, none) with a strict <: among equal d2 the smallest index wins, and a d2 that is NaN or +inf never
 *      does.  It is a pure function of the inputs, whatever the grid, the order of the visits or the number of times a face is
 *      evaluated.  Outputs: dist fp32 = (float)sqrt(d2); closest fp32 [3], the fp64 c rounded once; face int32; region uint8
 *      (0..6).  No winner (no usable face, a non-finite query): +inf, the query itself, -1, 255.
 *
 * The grid of face references is an sp3_nn_grid as it is (origin, h, inv_h, slack, dims; its cell-of-x rule).
 * sp3_mesh_tri_cell_count : counts int64 [F] = the number of cells the face is registered in: the cells cell(min - slack) ..
 *   cell(max + slack) per axis of its fp32 bounding box (0 for a face that is not usable).  Registration is CONSERVATIVE: cell(x) --
 *   an fp32 subtraction, product, floor and clamp -- is monotone in x, every point of the face has each coordinate between the
 *   face's min and max, so under the very assignment the queries use it falls in a registered cell, whatever the rounding of the
 *   inflation does (the slack only adds cells).  No tighter plane test is made.
 * sp3_mesh_tri_cell_fill : offsets int64 [F] = the EXCLUSIVE prefix sum of counts (the host's), npairs their total; writes
 *   (pair_cell, pair_face) int32 [npairs], a face's pairs in z, y, x order from offsets[f]; nothing is written at or past npairs.
 *   The host sorts the pairs by cell (stable) and builds cell_start[cells + 1].
 * sp3_mesh_dist_query : one lane per query, taken in q_order (nullable; sorted by home cell, clamped into the grid), results in
 *   caller order.  Rings r = 0..max_ring around the home cell.  A face no cell of the visited block holds has, on one axis, all its
 *   cells beyond one wall of the block, so it lies wholly behind that wall: the query is finished when sqrt of its best d2 is within
 *   the distance to the nearest wall of the block that still has cells behind it, less the slack -- the walk and the bound of
 *   csrc/cell_grid.h, the same code sp3_nn_query runs.  Queries
 *   left open go through the brute-force kernels.  pair_face [npairs] sorted by cell; indices read from it, from cell_start and from
 *   faces are range-checked before use.  After the call the first 32 bytes of ws hold { int32 fallback queries, 3 x int32 pad,
 *   uint64 cells visited, uint64 faces evaluated } (by the grid kernel).  nq = 0 launches nothing.
 * sp3_mesh_dist_brute : the same result for every query with the faces staged through LDS in tiles of 512 (usability decided by
 *   the loader), the face list split over workgroups; joined by a 64-bit integer atomicMin over the bits of d2, then, in a second pass
 *   over the same tiles, an atomicMin of the face index among the faces with exactly that d2; a last launch recomputes the closest
 *   point of the winner.  The fallback of sp3_mesh_dist_query, the route of a one-cell grid, and the on-device cross-check. */
int sp3_mesh_tri_cell_count(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const sp3_nn_grid* g, int64_t* counts,
                            void* stream);
int sp3_mesh_tri_cell_fill(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const sp3_nn_grid* g, const int64_t* offsets,
                           int64_t npairs, int32_t* pair_cell, int32_t* pair_face, void* stream);
int64_t sp3_mesh_dist_query_ws_bytes(int64_t nq);
int sp3_mesh_dist_query(const float* q, const int64_t* q_order, int64_t nq, const float* vertices, int64_t nverts, const int32_t* faces,
                        int64_t nfaces, const int32_t* pair_face, int64_t npairs, const int32_t* cell_start, const sp3_nn_grid* g, int max_ring,
                        void* ws, float* dist, float* closest, int32_t* face, uint8_t* region, void* stream);
int sp3_mesh_dist_brute(const float* q, int64_t nq, const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, void* ws,
                        float* dist, float* closest, int32_t* face, uint8_t* region, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh rays (spann3r_amd/mesh.py ray_mesh_intersect / render_depth_maps and spann3r_amd/evaluate.py evaluate_depth drive these;
 * csrc/mesh_ray.hip): what a ray hits first on a triangle mesh -- the other geometric question next to "Mesh distance" -- and, from
 * it, depth maps of a mesh seen from T cameras (spann3r/tools/render_dtu.py:54-80 render_depth_maps obtains them through pyrender and
 * an OpenGL context; parity with pyrender is unpinned, it is not available to test against).  tests/mesh_ray_ref.py restates the
 * rule in numpy and is itself checked against Moeller-Trumbore in exact rationals.  No entry point allocates, frees or synchronises;
 * `ws` is caller-provided device scratch of sp3_mesh_ray_ws_bytes(nq) (32 bytes for sp3_mesh_ray_views), 16-byte aligned.  Indices
 * are int32: nverts, nfaces and npairs stay below 2^31 - 1.  Every fp64 operation below is rounded on its own, in the order written
 * (no FMA: the file is compiled under `#pragma clang fp contract(off)`).
 *
 * The rule.  vertices fp32 [V, 3], faces int32 [F, 3].
 *   1. A RAY is o fp32 [3], d fp32 [3] (not normalised) and a range t_min <= t <= t_max with 0 <= t_min, doubles; o and d are
 *      converted to fp64.  A ray with a non-finite component of o or d, or with d = 0, hits nothing.
 *   2. A face is USABLE as in rule 1 of "Mesh distance" (indices in 0..V-1, the fp64 cross product of its edges finite and > 0); a
 *      face that is not usable is never hit.
 *   3. Intersection with a usable face (A, B, C) (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013), in fp64:
 *      kz = the axis of the largest |d|, the lowest axis among equals; kx = kz + 1, ky = kx + 1, cyclic; kx and ky are swapped when
 *      d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Per vertex P = vertex - o, X = P[kx] - Sx P[kz],
 *      Y = P[ky] - Sy P[kz], Z = Sz P[kz].  U = Xc Yb - Yc Xb, V = Xa Yc - Ya Xc, W = Xb Ya - Yb Xa (two products, one difference).
 *      A miss when one of U, V, W is < 0 and one is > 0.  det = (U + V) + W; a miss when det == 0.  T = (U Za + V Zb) + W Zc,
 *      t = T / det, a zero t stored as +0.  A hit when t_min <= t <= t_max (a comparison with a NaN is false).
 *      Watertight: the transformed vertex depends on the vertex and the ray only, and without FMA x y - z w = -(z w - x y) exactly, so
 *      the edge function of an edge two faces share is for one the exact negative of the other's; a zero counts as inside for both.
 *      No ray passes between two faces that share an edge; rule 4 decides which of them takes it.
 *      SIDE: det > 0 exactly when the ray's origin lies on the side from which A, B, C appear counter-clockwise (the side the normal
 *      (B - A) x (C - A) points to): side 0, the front.  det < 0: side 1, the back.  (Pinned on one triangle seen from both sides.)
 *      cull: 0 keeps every hit, 1 ("back") drops the hits with side 1, 2 ("front") those with side 0, before the minimum.
 *   4. The result of a ray is the minimum over the hits of the pair (t, face index), compared lexicographically, starting from
 *      (+inf, none) with a strict <: among equal t the smallest index wins, and a t that is NaN or +inf never does.  It is a pure
 *      function of the inputs, whatever the grid, the order of the visits or the number of times a face is evaluated.  Outputs:
 *      t fp32 = the fp64 t rounded once; face int32; bary fp32 [3] = U / det, V / det, W / det, the weights of A, B, C;
 *      point fp32 [3] = o + t d per axis, one fp64 product and one fp64 sum, rounded once; side uint8.  A miss: +inf, -1,
 *      (0, 0, 0), o itself, 255.
 *
 * sp3_mesh_ray_query : one lane per ray, taken in q_order (nullable; a permutation of the rays, sorted by the cell of the origin),
 *   results in caller order, over the grid of face references of sp3_mesh_tri_cell_count / _fill as it is (pair_face sorted by
 *   cell, cell_start [cells + 1]; npairs >= 1).  The ray is clipped in fp64 against the box [origin - slack, wall(n) + slack] per axis
 *   (wall(i) = fmaf(i, h, origin), as csrc/cell_grid.h computes it); an axis with d = 0 is a test of o against the two planes, never a
 *   division.  A ray that misses the box, or whose clipped range is empty, evaluates nothing.  It starts at max(t_min, entry) in the
 *   cell that the grid's own cell rule gives the entry point rounded to fp32 (clamped into the grid).  In every cell every referenced
 *   face is evaluated and any hit kept, wherever it lies.  The exit parameter of the cell along an axis is (wall - o) / d with the
 *   wall taken from the integer cell index at every step (no running sum: no drift); a cell on the rim of the grid has no wall on its
 *   outer side and reaches to the box's exit.  The walk steps along the axis of the smallest exit (on a tie the lowest such axis: a
 *   cell more is harmless) and ends when best t <= exit - 2 slack / |d[kz]|, when the exit is not before min(t_max, the box's exit),
 *   or when no wall is left: at most nx + ny + nz cells, so there is no fallback list.
 *   WHY NO HIT IS MISSED.  U, V, W of one sign make t a convex combination of Za, Zb, Zc, so the point o + t d of a hit lies in the
 *   face's fp32 bounding box (to fp64 rounding).  Registration covers cell(min - slack) .. cell(max + slack) under the monotone fp32
 *   cell rule, whose borders differ from the real-valued walls of the walk by less than half the slack (the subtraction, the product with
 *   the rounded inv_h and the fmaf of a wall with the rounded h are under three fp32 ulps of the box's largest coordinate plus its
 *   extent together; the host's slack, spann3r_amd/cell_grid.py make_grid, is 1e-6 of that: over eight).  The fp64 cell intervals of the walk tile
 *   [start, exit] without a gap, each from the same integer-indexed walls, so the real-valued cell that holds the point of a hit with
 *   t below the exit has been visited, and it or a neighbour within the slack of the point -- registered too -- is the cell the walk
 *   was in.  The stopping margin is two slacks of travel along the dominant axis, a larger margin than registration's, and only
 *   delays the stop; an entry cell that the fp32 rounding of the entry point puts one cell ahead skips less than half a slack of the
 *   ray, which the registered neighbours cover, and one cell behind only adds a cell.  On an axis with d = 0 the fp32 cell of o is
 *   exactly the cell registration gives that coordinate.
 *   After the call the first 32 bytes of ws hold { int32 0, 3 x int32 pad, uint64 cells visited, uint64 faces evaluated }.
 * sp3_mesh_ray_brute : the same result for every ray with the faces staged through LDS in tiles of 512 (usability decided by the
 *   loader), the face list split over workgroups; joined by a 64-bit integer atomicMin over the bits of the non-negative t, then, in
 *   a second pass over the same tiles, an atomicMin of the face index among the faces with exactly that t; a last launch recomputes
 *   bary, point and side of the winner.  The route of a one-cell grid and the on-device cross-check.
 * sp3_mesh_ray_views : the walk of sp3_mesh_ray_query (every face per ray when npairs == 0) for the rays of T cameras in ONE launch;
 *   views_host and views_dev hold the same T descriptors, the host copy is validated and sizes the launch, the device copy is read,
 *   never written, through scalar loads (a wave owns an 8 x 8 pixel tile of one view).  Pixel (u, v), centres at integer coordinates:
 *   x = ((u + pixel_offset) - cu) / fu, y = ((v + pixel_offset) - cv) / fv in fp64 from the fp32 fields; d_i = fp32((R_i0 x + R_i1 y)
 *   + R_i2), R_ij = c2w[4 i + j]; o_i = c2w[4 i + 3]; t_min = near, t_max = far, no culling.  The camera-frame direction has z = 1, so
 *   t IS camera z.  depth[v * row_stride + u] = t, 0 for a miss (render_dtu.py's convention and sp3_tsdf_raycast's); face (nullable)
 *   int32 and bary (nullable) fp32 [.., 3] likewise.  By construction equal to sp3_mesh_ray_query on the same rays, bit for bit.
 *   T = 0 launches nothing; ws as above. */
typedef struct {
  float* depth;        /* [h, row_stride] */
  int32_t* face;       /* [h, row_stride] or null */
  float* bary;         /* [h, row_stride, 3] or null */
  int64_t row_stride;  /* elements between rows, >= w */
  int32_t w, h;
  float fu, fv, cu, cv;
  float c2w[12];       /* camera-to-world, row-major 3 x 4 */
  float near, far;     /* 0 <= near <= far (+inf allowed), camera z */
} sp3_mesh_ray_view;
int64_t sp3_mesh_ray_ws_bytes(int64_t nq);
int sp3_mesh_ray_query(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                       int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                       const int32_t* cell_start, const sp3_nn_grid* g, double t_min, double t_max, int cull, void* ws, float* t,
                       int32_t* face, float* bary, float* point, uint8_t* side, void* stream);
int sp3_mesh_ray_brute(const float* origins, const float* directions, int64_t nq, const float* vertices, int64_t nverts,
                       const int32_t* faces, int64_t nfaces, double t_min, double t_max, int cull, void* ws, float* t, int32_t* face,
                       float* bary, float* point, uint8_t* side, void* stream);
int sp3_mesh_ray_views(const sp3_mesh_ray_view* views_host, const sp3_mesh_ray_view* views_dev, int T, float pixel_offset,
                       const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                       const int32_t* cell_start, const sp3_nn_grid* g, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh BVH (spann3r_amd/mesh.py TriangleBVH and the bvh= keyword of point_mesh_distance / ray_mesh_intersect / render_depth_maps,
 * spann3r_amd/evaluate.py evaluate_meshes(exact=True, accel="bvh") and evaluate_depth(bvh=...) drive these; csrc/mesh_bvh.hip): a
 * bounding-volume hierarchy over the faces of a mesh that answers the questions of "Mesh distance" and "Mesh rays" BY THEIR OWN
 * RULES at any range -- a query far from the surface, or a mesh whose faces differ wildly in size, costs a walk of the tree's depth
 * where the uniform grid hands over to the brute-force kernels or grows its cells.  The faces of a leaf are evaluated by the very
 * functions the grid and the brute-force kernels call (csrc/tri_dist.h, csrc/tri_ray.h) and the result is the same lexicographic
 * minimum (rules 3 of "Mesh distance" and 4 of "Mesh rays"), so every output equals theirs bit for bit; tests/mesh_bvh_ref.py restates
 * the structure and both walks in numpy.  No entry point allocates, frees or synchronises; `ws` is 32 bytes of caller-provided device
 * scratch, 16-byte aligned.  Indices are int32: nverts and nfaces stay below 2^31 - 1.
 *
 * The structure.  LEAF = 4 faces per leaf node, ARITY = 4 children per node (named constants of csrc/mesh_bvh.hip and
 * spann3r_amd/cell_grid.py).
 *   1. KEYS.  A usable face (rule 1 of "Mesh distance") gets the 63-bit Morton key (x in bit 0, y in bit 1, z in bit 2 of every
 *      triple) of the fp32 centre 0.5f min + 0.5f max of its fp32 bounding box, each axis quantised to 21 bits against the box of
 *      the mesh's finite vertices: clamp(floor((c - lo) * scale), 0, 2^21 - 1), scale = fp32(2^21 / (hi - lo)), 0 for an axis of no
 *      extent; a usable key is capped at 2^63 - 2 and a face that is not usable gets 2^63 - 1 (63 ones).  The host sorts the keys
 *      (stable); `order` int32 [usable] is the usable faces in that order.  The key decides the QUALITY of the tree only: any
 *      permutation of the usable faces gives a valid tree and the same results.
 *   2. LEVELS.  Leaf node k holds order[k LEAF .. (k + 1) LEAF); node k of level l + 1 holds nodes k ARITY .. (k + 1) ARITY of
 *      level l; levels are added until one holds a single node, the root: size(0) = ceil(usable / LEAF), size(l + 1) =
 *      ceil(size(l) / ARITY), at most 16 levels.  Level l is stored at level_off[l] .. level_off[l + 1] of node_lo / node_hi fp32
 *      [nodes, 3].  There are no child pointers, and a node exists iff its index is below its level's size: existence is decided
 *      from counts, never from box values.  A node's box is the exact fp32 min / max of the vertices of the faces below it -- min
 *      and max are exact and order-free, so the boxes have the same bits every run.
 *   3. slack = 1e-6 (the largest |coordinate| of the box of the finite vertices + its largest extent): make_grid's without h.
 * sp3_mesh_bvh_keys : keys int64 [n] of n faces, or -- faces null, n = nverts -- of n points (a non-finite point: 2^63 - 1); box =
 *   6 floats ON THE HOST, lo then hi.  The point form gives the order queries are served in: neighbours descend together.
 * sp3_mesh_bvh_build : one launch for the leaf level and one per level above it (at most 16), each reading only what an earlier
 *   launch wrote.  No atomics, counters or flags.  The descriptor is validated by every entry point: 1 <= usable <= nfaces, leaves =
 *   ceil(usable / LEAF), 1 <= levels <= 16, level_off[0] = 0, every level the ceiling quotient of the one below, the last of size 1.
 *
 * The walk: one lane per query, depth first, the stack in LDS laid out [entry][lane], (ARITY - 1) (levels - 1) + 1 entries of 4
 * bytes (a popped node pushes at most ARITY nodes of the level below; 46 entries at 16 levels), no scratch memory.  A node is
 * tested when it is pushed and again when it is popped; the children of a node are pushed farthest first, so the nearest is
 * popped first.  Every node is pushed at most once, so the walk ends.  An entry is the node's index within its level under a
 * marker bit at 30 - 2 level (LEAF = ARITY = 4): level l holds at most max(2^(29 - 2 l), 1) nodes for nfaces < 2^31 - 1, so the index
 * stays below the marker up to the root of a 16-level tree (level 15, index 0: the word 1), and a descriptor with a larger level
 * is refused.  Indices read from order, faces and q_order are range-checked; an entry of q_order outside 0 .. nq - 1 is skipped.
 * sp3_mesh_bvh_dist_query : per axis g = max(max(lo - p, p - hi) - slack, 0) in fp64 from the node's fp32 box; lb = ((gx gx + gy gy)
 *   + gz gz) (1 - 2^-30); a node is skipped iff lb > best d2 -- strictly, so a node that may hold an equal d2 with a smaller face
 *   index is visited.  WHY NO FACE IS MISSED: the true distance to a box never exceeds the true distance to a face inside it; the
 *   evaluated d2 of rule 2 differs from the true one by rounding (3.4e-13 relative measured against exact rationals in
 *   tests/test_mesh_distance_cpu.py, larger for points within that of the surface, which the slack -- 1e-6 of the scene -- covers),
 *   and the factor sits three orders above that; it only delays pruning.  This is an argument, not a proof: tests/test_mesh_bvh_cpu.py
 *   checks the property lb(face's own box) <= evaluated d2 on thousands of pairs, slivers and near-contact included.  A non-finite
 *   query never enters the tree: rule 3's no-winner outputs.  Outputs as sp3_mesh_dist_query; q_order nullable.
 * sp3_mesh_bvh_ray_query : the ray is clipped in fp64 against the node's box pushed out by the slack, starting from [t_min, t_max],
 *   with the slab test sp3_mesh_ray_query applies to the grid's box (an axis with d = 0 is a test of o, never a division).  A node is
 *   skipped iff the clipped range is empty or its entry is > best t (strictly); children nearest entry first.
 *   WHY NO HIT IS MISSED.  As for the grid: U, V, W of one sign make t a convex combination of Za, Zb, Zc, so the point o + t d of a
 *   hit lies in the face's fp32 bounding box to fp64 rounding -- a few 1e-16 of the distances involved, against a slack of 1e-6 of
 *   the scene.  The box of every ancestor contains the face's box exactly (min and max do not round).  So t lies in the clipped
 *   range of the face's leaf and of every node above it, the entry of each of them is <= t, and none is skipped while best > t or
 *   (best == t and the face's index is smaller): the face is evaluated.  Outputs as sp3_mesh_ray_query; q_order nullable.
 * sp3_mesh_bvh_ray_views : the same walk for the rays of T cameras in ONE launch: the descriptors, the pixel rule and the outputs of
 *   sp3_mesh_ray_views (a wave owns an 8 x 8 tile of one view; the device copy of the table is only read, through scalar loads).
 * After a query the first 32 bytes of ws hold { int32 0, 3 x int32 pad, uint64 nodes visited, uint64 faces evaluated }.  nq = 0 and
 * T = 0 launch nothing. */
#define SP3_BVH_MAX_LEVELS 16
typedef struct {
  int32_t usable;                             /* entries of order: the usable faces */
  int32_t leaves;                             /* ceil(usable / LEAF) */
  int32_t levels;                             /* 1 .. SP3_BVH_MAX_LEVELS, the leaf level included */
  int32_t level_off[SP3_BVH_MAX_LEVELS + 1];  /* level l: nodes level_off[l] .. level_off[l + 1] - 1; entries past `levels` unused */
  float slack;
} sp3_mesh_bvh;
int sp3_mesh_bvh_keys(const float* vertices, int64_t nverts, const int32_t* faces, int64_t n, const float* box, int64_t* keys, void* stream);
int sp3_mesh_bvh_build(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const sp3_mesh_bvh* b,
                       float* node_lo, float* node_hi, void* stream);
int sp3_mesh_bvh_dist_query(const float* q, const int64_t* q_order, int64_t nq, const float* vertices, int64_t nverts, const int32_t* faces,
                            int64_t nfaces, const int32_t* order, const float* node_lo, const float* node_hi, const sp3_mesh_bvh* b, void* ws,
                            float* dist, float* closest, int32_t* face, uint8_t* region, void* stream);
int sp3_mesh_bvh_ray_query(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                           int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                           const float* node_hi, const sp3_mesh_bvh* b, double t_min, double t_max, int cull, void* ws, float* t, int32_t* face,
                           float* bary, float* point, uint8_t* side, void* stream);
int sp3_mesh_bvh_ray_views(const sp3_mesh_ray_view* views_host, const sp3_mesh_ray_view* views_dev, int T, float pixel_offset,
                           const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order,
                           const float* node_lo, const float* node_hi, const sp3_mesh_bvh* b, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh visibility (spann3r_amd/mesh.py ray_mesh_occluded / point_visibility / vertex_visibility / cull_to_views and
 * spann3r_amd/evaluate.py evaluate_meshes(cull_views=...) drive these; csrc/ray_kernels.h holds the two front ends, csrc/mesh_ray.hip
 * and csrc/mesh_bvh.hip their entry points over the grid and over the tree, csrc/mesh_visibility.hip the face classes): which part of
 * a mesh a set of cameras can see -- the cull_mesh step that NICE-SLAM-style evaluations apply to both meshes before accuracy and
 * completion.  tests/mesh_visibility_ref.py restates the rule in numpy; Open3D, trimesh and the NICE-SLAM script are not available
 * to test against, so that restatement and the closest-hit kernels of "Mesh rays" are the anchors (parity unpinned).  No entry
 * point allocates, frees or synchronises; `ws` is 32 bytes of caller-provided device scratch, 16-byte aligned, whose head counts
 * cells / nodes visited and faces evaluated as after sp3_mesh_ray_query.  Every fp64 operation below is rounded on its own, in the
 * order written (no FMA).
 *
 * The rule.
 *   1. OCCLUSION.  A ray (o, d, t_min, t_max, cull) of "Mesh rays" is OCCLUDED iff some usable face is a hit by rule 3 there: exactly
 *      `face >= 0` of sp3_mesh_ray_query.  Whether a hit exists does not depend on which one a walk meets first, so the walks stop at
 *      the first accepted hit (the grid's leaves its cell loop; the tree's sets its best key to -inf, below every node's entry, so
 *      every later pop and push fails the test it already makes) and the answer is a pure function of the inputs whatever the
 *      structure.  A miss walks exactly the path of the closest-hit walk.  A ray with a non-finite component or d = 0 is not
 *      occluded; an empty range (t_min > t_max) occludes nothing.
 *   2. VISIBILITY of a point p fp32 [3] from a view (w, h, fu, fv, cu, cv, near, far, c2w[12], w2c[12]; w2c is the fp64 inverse of
 *      the pose rounded to fp32, fusion.camera_tables').  In fp64 from the fp32 fields:
 *        x = ((W00 p0 + W01 p1) + W02 p2) + W03, y and z likewise from rows 1 and 2 of w2c;
 *        IN RANGE: z > 0 and near <= z <= far;
 *        u = (x / z) fu + cu, v = (y / z) fv + cv;
 *        IN THE IMAGE: 0 <= (u - pixel_offset) + 0.5 < w and 0 <= (v - pixel_offset) + 0.5 < h (a pixel covers half a unit either
 *        side of its centre, the pixel rule of sp3_mesh_ray_views);
 *        the SHADOW RAY: o = the translation of c2w (as sp3_mesh_ray_views takes it), d_k = fp32((double)p_k - (double)o_k),
 *        t_min = near / z, t_max = 1.0 - (double)bias, bias fp32 in [0, 1);
 *      visible(p, view) = in range, in the image and the shadow ray not occluded.  A non-finite p is visible from nowhere.  Surfaces
 *      in front of the near plane do not occlude (as they are not rendered by sp3_mesh_ray_views).  bias is a relative depth
 *      tolerance: it drops the hit of a vertex on its own faces (t = 1 to the fp32 rounding of d); a convention, default 1e-3.
 *   3. count int32 [N] = the number of views that see the point; mask uint8 [T, N] (nullable) = visible(p, view).
 *   4. CULLING.  A vertex is SEEN iff count >= min_views.  The class of a face is -1 when one of its indices lies outside 0..V-1
 *      (count is then never read for it), else 1 (keep) when -- mode 0, "any" -- one of its vertices is seen or -- mode 1, "all" --
 *      all three are, else 0.  sp3_mesh_select_faces(face_component = the classes, ncomponents = 2, keep = {0, 1}) keeps the faces of
 *      class 1 in their order and rotation, and sp3_mesh_compact_vertices drops the vertices nothing names.
 *
 * sp3_mesh_ray_occluded / sp3_mesh_bvh_ray_occluded : the arguments, host checks and workspace head of sp3_mesh_ray_query /
 *   sp3_mesh_bvh_ray_query with one uint8 per ray (1: occluded) in place of the five outputs: one lane per ray in q_order, one byte
 *   stored per ray and nothing else.
 * sp3_mesh_point_views / sp3_mesh_bvh_point_views : one lane per (point, view) pair, the view in blockIdx.y (its descriptor is
 *   wave-uniform and read through scalar loads), the points in q_order (nullable; the structure's own query order: the lanes of a
 *   wave shoot from one origin at neighbouring targets).  The projection tests run first: a pair outside the frustum walks nothing.
 *   A visible pair does one integer atomicAdd on count[p] (order-free: the same bits every run; the caller zeroes count) and every
 *   pair stores mask[view * N + p] when mask is given.  views_host and views_dev hold the same T descriptors; the host copy is
 *   validated as sp3_mesh_ray_views validates (1 <= w, h <= 2^24, finite intrinsics with non-zero focals, 0 <= near <= far,
 *   T <= 65535), the device copy is only read.  bias must lie in [0, 1) and pixel_offset be finite.  The grid form takes
 *   npairs = 0 (a grid of one cell: every face per ray).  T = 0 or N = 0 launches nothing.
 * sp3_mesh_vis_face_class : cls int32 [F] of rule 4 from count int32 [V]; one lane per face.  F = 0 launches nothing. */
typedef struct {
  int32_t w, h;
  float fu, fv, cu, cv;
  float near, far;     /* 0 <= near <= far (+inf allowed), camera z */
  float c2w[12];       /* camera-to-world, row-major 3 x 4: the origin of the shadow rays */
  float w2c[12];       /* world-to-camera, row-major 3 x 4: the projection */
} sp3_mesh_vis_view;
int sp3_mesh_ray_occluded(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                          int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                          const int32_t* cell_start, const sp3_nn_grid* g, double t_min, double t_max, int cull, void* ws,
                          uint8_t* occluded, void* stream);
int sp3_mesh_bvh_ray_occluded(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                              int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                              const float* node_hi, const sp3_mesh_bvh* b, double t_min, double t_max, int cull, void* ws,
                              uint8_t* occluded, void* stream);
int sp3_mesh_point_views(const sp3_mesh_vis_view* views_host, const sp3_mesh_vis_view* views_dev, int T, float pixel_offset, float bias,
                         int cull, const float* points, const int64_t* q_order, int64_t npoints, const float* vertices, int64_t nverts,
                         const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs, const int32_t* cell_start,
                         const sp3_nn_grid* g, void* ws, int32_t* count, uint8_t* mask, void* stream);
int sp3_mesh_bvh_point_views(const sp3_mesh_vis_view* views_host, const sp3_mesh_vis_view* views_dev, int T, float pixel_offset,
                             float bias, int cull, const float* points, const int64_t* q_order, int64_t npoints, const float* vertices,
                             int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                             const float* node_hi, const sp3_mesh_bvh* b, void* ws, int32_t* count, uint8_t* mask, void* stream);
int sp3_mesh_vis_face_class(const int32_t* faces, int64_t nfaces, int64_t nverts, const int32_t* count, int min_views, int mode,
                            int32_t* cls, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh topology and smoothing (spann3r_amd/mesh.py MeshTopology / topology / smooth drive these; csrc/mesh_topology.hip): the table
 * of unique undirected edges of an indexed triangle mesh with their face incidences, the vertex adjacency derived from it, a
 * manifold report, and Taubin's lambda|mu low-pass on top.  tests/mesh_topology_ref.py restates the rule in numpy; Open3D's
 * filter_smooth_taubin is not available to test against (parity unpinned: the defaults 0.5 / -0.53 are its defaults).  No entry
 * point allocates, frees or synchronises; `ws` is caller-provided device scratch of the matching sp3_*_ws_bytes(), 16-byte aligned.
 * The two sorts between the entry points are the caller's (torch.sort(stable=True), as for TriangleGrid and TriangleBVH).  Every
 * output is a pure function of the inputs: integer work, and fp64 sums in one fixed order.
 *
 * The rule.  Vertices 0..V-1, faces int32 [F, 3], V < 2^31 - 1, 3 F < 2^31.
 *   Usable faces.  A face is USABLE when its three indices lie in 0..V-1 and are pairwise distinct (narrower than "Mesh components",
 *     which accepts a == b: a self-edge has no meaning here).  An unusable face is never dereferenced.
 *   Half-edges.  Usable face f has half-edges h = 3 f + c, c = 0, 1, 2, from a = face[c] to b = face[(c + 1) % 3]; lo = min(a, b),
 *     hi = max(a, b); the half-edge is FORWARD when a < b.
 *   Edge table.  The unique pairs (lo, hi) are the edges, numbered 0..E-1 in ascending (lo, hi) order.  Edge e has uses (its
 *     half-edges), fwd (those that are forward) and the list of its half-edges in ascending h,
 *     half_edges[edge_first[e] : edge_first[e + 1]]; its faces are h / 3.  edge_first[E] = 3 x the usable faces.
 *   Edge class.  0 boundary: uses == 1.  1 interior: uses == 2 and fwd == 1.  2 inconsistent: uses == 2 and fwd is 0 or 2 (two faces
 *     with the same winding along the edge; a duplicated face gives three).  3 non-manifold: uses > 2.
 *   Vertex adjacency.  CSR: vertex_offsets int32 [V + 1], vertex_neighbors int32 [2 E]; row v holds the distinct vertices that share
 *     an edge with v, ASCENDING.  vertex_boundary uint8 [V] = 1 iff v is an endpoint of a class-0 edge.
 *   info int32 [16], ZERO on entry of sp3_mesh_edge_keys: [0] E, [1..4] the edges of class 0..3, [5] usable faces, [6] unusable faces,
 *     [7] vertices with a non-empty row, [8] vertices with vertex_boundary = 1.  The report of mesh.py is one read of it:
 *     euler = info[7] - E + info[5]; closed = (E > 0 and info[2] == E).
 *   One smoothing pass with factor c (a double).  Vertex v with k > 0 neighbours n_0 < .. < n_{k-1} (its row) that is not fixed:
 *     per component, in fp64, every operation rounded on its own (`#pragma clang fp contract(off)`, as csrc/tri_dist.h),
 *       s = p[n_0];  s = s + p[n_1];  ..;  m = s / k;  out = fp32(p[v] + c * (m - p[v])).
 *     A vertex with k = 0 or a fixed one (fixed uint8 [V], nullable: nothing fixed) copies its bits.  Positions between passes are
 *     fp32 in ping-pong buffers: a pass never reads what it writes (out == positions is refused).  NaN and infinity propagate as
 *     IEEE says; there are no special cases.  mesh.smooth: each of `iterations` rounds is pass(lam), then pass(mu) unless mu == 0.
 * sp3_mesh_edge_keys : one lane per face writes keys int64 [3 F], keys[3 f + c] = ((lo << 31 | hi) << 1) | backward -- 63 bits -- or,
 *   for an unusable face, three copies of 2^63 - 1, which lies above every real key; info[5] and info[6] are counted (integer adds
 *   of wave popcounts).  The caller sorts the keys (stable) with the half-edge index as payload: equal pairs become one run, within
 *   a run the forward entries come first, and equal keys keep ascending h.
 * sp3_mesh_edge_table : keys / order int64 [nkeys] are the sorted keys and their payload (nkeys = 3 F).  Writes edges int32 [E, 2],
 *   edge_first int32 [E + 1], edge_uses, edge_fwd int32 [E], edge_class uint8 [E], half_edges int32 [3 x usable], vertex_boundary
 *   uint8 [V] and info[0..4], [7], [8]; every table has room for nkeys entries (edge_first: nkeys + 1), since E is not known to the
 *   host.  With E = 0 nothing but vertex_boundary (zeros) and info is written.  Why each step is order-free:
 *   - run heads (a real key whose key >> 1 differs from its predecessor's) are flagged, counted per 256-element tile, scanned by one
 *     workgroup and scattered to offsets[tile] + rank: the head writes its pair and edge_first[e]; the last real element writes
 *     edge_first[e + 1].  An element's edge is offsets[tile] + (heads of its tile up to and including itself) - 1, whether its
 *     run began in its own tile or any number of tiles and scan chunks earlier: no lane walks a run.
 *   - a later launch has one lane per edge: uses from edge_first, fwd by a binary search for the first backward entry of the run
 *     (the sort put the forward ones first), the class, the class counts (integer adds of wave popcounts) and the flags of its two
 *     vertices.  Several lanes may store to one flag; all store 1, and nothing reads a flag before the next launch.
 *   - the sort leaves a run as two ascending lists of h, forward then backward.  A further launch, one lane per element, merges
 *     them: an element's place is its place in its own list plus the entries of the other list below it (binary search), so that
 *     the half-edges of an edge ascend.
 *   - launch boundaries are the only hand-offs; no lane waits for another lane's store.  8 launches.
 * sp3_mesh_adjacency_keys : one lane per edge writes keys int64 [2 E], (lo << 32) | hi and (hi << 32) | lo; 2 E < 2^31.  The caller
 *   sorts them (they are distinct).
 * sp3_mesh_adjacency_rows : lane i writes vertex_neighbors[i] = the low word of sorted key i and, for i <= V, vertex_offsets[i] =
 *   the number of keys below i << 32 (binary search): rows ascend because the keys do.
 * sp3_mesh_smooth_pass : one lane per vertex reads its two offsets and gathers its row in order; a row is never split over lanes,
 *   which would change the order of the sum.  vertex_neighbors may be null when every row is empty. */
int sp3_mesh_edge_keys(const int32_t* faces, int64_t nfaces, int64_t nverts, int64_t* keys, int32_t* info, void* stream);
int64_t sp3_mesh_edge_table_ws_bytes(int64_t nkeys, int64_t nverts);
int sp3_mesh_edge_table(const int64_t* keys, const int64_t* order, int64_t nkeys, int64_t nverts, void* ws, int32_t* edges,
                        int32_t* edge_first, int32_t* edge_uses, int32_t* edge_fwd, uint8_t* edge_class, int32_t* half_edges,
                        uint8_t* vertex_boundary, int32_t* info, void* stream);
int sp3_mesh_adjacency_keys(const int32_t* edges, int64_t nedges, int64_t* keys, void* stream);
int sp3_mesh_adjacency_rows(const int64_t* keys, int64_t nkeys, int64_t nverts, int32_t* vertex_offsets, int32_t* vertex_neighbors,
                            void* stream);
int sp3_mesh_smooth_pass(const float* positions, int64_t nverts, const int32_t* vertex_offsets, const int32_t* vertex_neighbors,
                         const uint8_t* fixed, double factor, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh boundary loops and hole filling (spann3r_amd/mesh.py BoundaryLoops / boundary_loops / fill_holes drive these;
 * csrc/mesh_boundary.hip): the boundary edges of an edge table ("Mesh topology and smoothing") as ordered loops, and a fan over
 * every loop of at most max_edges edges.  tests/mesh_boundary_ref.py restates the rule in numpy.  Unpinned: Open3D `fill_holes` /
 * MeshLab are absent, nothing upstream fixes these numbers.  No entry point allocates, frees or synchronises; `ws` is
 * caller-provided device scratch of the matching sp3_*_ws_bytes(), 16-byte aligned.  Integer work except the fp64 centroid sums;
 * every output is a pure function of the inputs.
 *
 * The rule.  A mesh (vertices fp32 [V, 3], optional packed colours int32 [V], faces int32 [F, 3]) and the edge table of its faces.
 *   Boundary elements.  The class-0 edges in ascending edge number are the elements j = 0..B-1, B = info[1] of the edge table (the
 *     host has read it).  Element j has edge[j] = e, its one half-edge h[j] = half_edges[edge_first[e]], src[j] = faces[h / 3][h % 3]
 *     and dst[j] = faces[h / 3][(h % 3 + 1) % 3]: the edge in the direction its face walks it.
 *   Regular vertices, the successor.  A vertex is REGULAR when exactly one element leaves it (it is that element's src) and exactly
 *     one enters it (dst).  next[j] = the element that leaves dst[j] if dst[j] is regular, else -1.  Bow-ties (two fans meeting in
 *     one vertex), vertices on non-manifold edges and flipped windings are irregular; a chain ends there on purpose: nothing is
 *     sorted by angle, nothing is guessed.
 *   Cycles and chains.  next is injective on its domain -- next[j] = k makes dst[j] regular, so j is the only element entering
 *     src[k] -- hence the elements fall into disjoint closed cycles and open simple chains; a chain never runs into a cycle.  A
 *     closed cycle has at least 3 elements: a 1-cycle would be an edge from a vertex to itself (no usable face has one), a 2-cycle
 *     two opposite half-edges on one vertex pair, which is one edge with two uses and so not of class 0.
 *   Loops.  A closed cycle is a LOOP, its HEAD its smallest j; loops are numbered 0..L-1 by ascending head.  loop[j] = the number
 *     of j's loop, rank[j] = the next-steps from the head to j; both -1 on an open chain.  CSR: loop_first int32 [L + 1],
 *     loop_members int32 [loop_first[L]]; row l lists the loop's elements in walk order from the head.
 *   info int32 [16], ZERO on entry of sp3_mesh_boundary_link: [0] B, [1] L, [2] elements on open chains, [3] irregular vertices (with
 *     an element and not regular), [4] the longest loop (0 without one), [5] loop_first[L] = B - [2].
 *   Filling with max_edges = n >= 3.  Every loop of length len <= n is filled, in loop order.  len == 3: one face (dst[m0], src[m0],
 *     src[m2]) over its members m0, m1, m2 -- the boundary walk reversed, so the face is wound like its three neighbours -- and no
 *     vertex.  len > 3: one new vertex c and len faces (dst[m], src[m], c) in member order.  New vertices follow V in loop order, new
 *     faces follow F in (loop, rank) order; nothing that exists is rewritten.  Position of c per component, in fp64, every operation
 *     rounded on its own (`#pragma clang fp contract(off)`, as sp3_mesh_smooth_pass):
 *       s = p[src[m0]];  s = s + p[src[m1]];  ..;  c = fp32(s / len).
 *     Colour of c, where there are colours, per byte channel in integers: (2 * sum + len) / (2 * len) (the mean, rounded half up).
 *     Open chains and loops longer than n are never filled: that is how the observed rim of a fused surface stays open.
 * sp3_mesh_boundary_elements : flags the class-0 edges, counts them per 256-element tile, scans, scatters (scan.h): writes edge /
 *   half_edge / src / dst int32 [B], and per vertex vertex_out / vertex_in int32 [V] (the elements leaving / entering; integer
 *   atomicAdds, order-free) and vertex_leave int32 [V] (an element that leaves it, -1 without one).  Several lanes may store to
 *   vertex_leave[v] at an irregular vertex, with different values; the slot is only ever read where the counts say 1 and 1, where
 *   one lane stored, and never before the next launch.  nboundary must be the table's info[1]; an element whose half-edge or
 *   vertices are out of range (a table of another mesh) gets src = dst = -1 and links to nothing.  6 launches.
 * sp3_mesh_boundary_link : one lane per element writes next; one lane per vertex counts the irregular ones into info[3].
 * sp3_mesh_boundary_rounds : R = ceil(log2(max(B, 2))).
 * sp3_mesh_boundary_rank : list ranking by pointer doubling.  state int32 [B, 4] per element: (ptr, label, steps, 0); after round k
 *   ptr is the element 2^k steps ahead (-1: the chain ended within them), label the smallest element of the window of 2^k
 *   elements that starts at j, steps the next-steps from j to the FIRST place the label stands at.  Round k reads one buffer and
 *   writes the other (state and ws take turns so that round R - 1 lands in state): a round never reads what it writes.
 *   new = (ptr[ptr], min label of the two windows, its steps (+ 2^k when it comes from the far window)); on EQUAL labels the near
 *   window's steps stay -- once 2^k exceeds the length of a loop the window covers the head more than once, and rank needs the
 *   first time.  After R rounds ptr == -1 exactly on open chains (no chain is longer than B <= 2^R) and label is the head on a
 *   loop.  1 + R launches.
 * sp3_mesh_boundary_loops : heads (label == j, ptr != -1) are flagged, counted, scanned (info[1] = L) and numbered; a loop's length
 *   is steps + 1 of its head's successor next[head] -- no atomics, no walk; the lengths are scanned into loop_first (a grid of B + 1 lanes,
 *   since L is not known to the host; info[5]); every element then writes loop, rank = (len - steps) % len and itself to
 *   loop_members[loop_first[loop] + rank].  loop_first has room for B + 1 entries, loop_members for B.  7 launches.  The caller reads
 *   info once afterwards and sizes the CSR.
 * sp3_mesh_fill_count : one lane per loop decides len <= max_edges; two scans give vertex_at / face_at int32 [L] (the loop's new
 *   vertex and first new face, counted from V and F; -1: none) and fill_info int32 [16], ZERO on entry: [0] vertices added, [1] faces
 *   added, [2] loops filled.  4 launches.  The caller reads the totals and allocates.
 * sp3_mesh_fill_emit : out_positions fp32 [V + added, 3], out_rgba int32 [V + added] (null with rgba null) and out_faces int32
 *   [F + added, 3] already hold the mesh in front; one lane per loop with a centre adds its row in order (at most max_edges
 *   members: the only sequential walk there is), one lane per member of a loop writes its face.  The caller's arrays are only read. */
int64_t sp3_mesh_boundary_elements_ws_bytes(int64_t nedges);
int sp3_mesh_boundary_elements(const int32_t* faces, int64_t nfaces, int64_t nverts, const uint8_t* edge_class, const int32_t* edge_first,
                               const int32_t* half_edges, int64_t nedges, int64_t nboundary, void* ws, int32_t* edge, int32_t* half_edge,
                               int32_t* src, int32_t* dst, int32_t* vertex_out, int32_t* vertex_in, int32_t* vertex_leave, void* stream);
int sp3_mesh_boundary_link(const int32_t* dst, int64_t nboundary, const int32_t* vertex_out, const int32_t* vertex_in,
                           const int32_t* vertex_leave, int64_t nverts, int32_t* next, int32_t* info, void* stream);
int sp3_mesh_boundary_rounds(int64_t nboundary);
int64_t sp3_mesh_boundary_rank_ws_bytes(int64_t nboundary);
int sp3_mesh_boundary_rank(const int32_t* next, int64_t nboundary, void* ws, int32_t* state, void* stream);
int64_t sp3_mesh_boundary_loops_ws_bytes(int64_t nboundary);
int sp3_mesh_boundary_loops(const int32_t* next, const int32_t* state, int64_t nboundary, void* ws, int32_t* loop, int32_t* rank, int32_t* loop_first,
                            int32_t* loop_members, int32_t* info, void* stream);
int64_t sp3_mesh_fill_count_ws_bytes(int64_t nloops);
int sp3_mesh_fill_count(const int32_t* loop_first, int64_t nloops, int64_t max_edges, void* ws, int32_t* vertex_at, int32_t* face_at,
                        int32_t* info, void* stream);
int sp3_mesh_fill_emit(const float* positions, const int32_t* rgba, int64_t nverts, int64_t nfaces, const int32_t* src, const int32_t* dst,
                       const int32_t* loop, const int32_t* rank, const int32_t* loop_first, const int32_t* loop_members, int64_t nloops,
                       int64_t nmembers, const int32_t* vertex_at, const int32_t* face_at, int64_t vertices_added, int64_t faces_added,
                       float* out_positions, int32_t* out_rgba, int32_t* out_faces, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-view consistency (spann3r_amd/multiview.py drives these; csrc/multiview.hip).  Every frame of a reconstruction has a
 * pointmap in one world frame and a confidence; a flying pixel at a depth discontinuity survives a per-frame confidence test
 * although other cameras look straight through it.  Here every pixel's point is looked up in every OTHER frame: it is counted as
 * seen, in agreement, in front of or behind what that frame measured there, and its confidence is clipped where it floats in front
 * of a more confident measurement.  The rule is that of DUSt3R's BasePCOptimizer.clean_pointcloud (dust3r/cloud_opt/base_opt.py),
 * with these differences: the pixel is floor(u + 0.5) instead of torch.round (they differ only at exact halves); the projection is
 * fu * xc / zc + cu instead of a matrix product followed by a division; the depth of frame j at a pixel is the camera z of j's own
 * pointmap there, not an optimised depth map; there is a `valid` mask, which that method lacks.  Parity with that method is
 * UNPINNED (dust3r.cloud_opt cannot be imported where this is built); tests/multiview_ref.py restates the rule below in numpy and
 * the kernel is checked against that bit for bit.  No entry point allocates device memory, frees or synchronises.  Every fp32
 * operation is rounded on its own (`#pragma clang fp contract(off)`) and sums run left to right as written.
 *
 * Frames are sp3_tsdf_frame descriptors exactly as sp3_tsdf_integrate takes them (frames_host and frames_dev hold the same T
 *   descriptors; the host copy is only read for the checks).  Every frame must have pts; a frame with depth is refused.
 *   pixel_weight carries the confidence (nullable), valid is nullable, rgba is ignored.  Frames may differ in w, h and row_stride.
 * Lookup of a world point X = (x, y, z) in frame j (descriptor fr, m = fr.w2c), the steps of sp3_tsdf_integrate in its order:
 *     zc = ((m8 x + m9 y) + m10 z) + m11;  skip unless zc > 0;  xc (m0..m3) and yc (m4..m7) likewise;
 *     u = fu * xc / zc + cu, v = fv * yc / zc + cv;  px = floor(u + 0.5), py = floor(v + 0.5);
 *     skip unless 0 <= px < w and 0 <= py < h (compared in fp32, a NaN fails);  p = py * row_stride + px;  skip if valid[p] == 0;
 *     d = ((m8 X' + m9 Y') + m10 Z') + m11 of pts[p] = (X', Y', Z');  skip unless d is finite and > 0.
 *   A lookup that is not skipped is SEEN.
 * Classes, with lo = (1.0f - tol) * d and hi = (1.0f + tol) * d:  FRONT: zc < lo (the point floats in front of what j measured
 *   there, a free-space violation);  BEHIND: not front and zc > hi (occluded in j, which says nothing);  AGREE: otherwise;
 *   STRONGER: front, both frames have pixel_weight, and conf_i[q] < conf_j[p] (a NaN on either side fails).
 * Counts of pixel q of frame i, X = pts_i[q]: all four 0 if valid_i[q] == 0; otherwise every j != i is visited in table order (a
 *   non-finite X is skipped by every lookup on its own).  counts[q] = (seen, agree, front, stronger) as int32; behind is
 *   seen - agree - front.  They are integers of a pure per-pair predicate: the same bits on every run.
 * Cleaning: pixel q of frame i is BAD iff some j is front for it and conf_i[q] < c_j[p], with conf_i the ORIGINAL confidence of
 *   frame i and c_j the state of frame j.  Parallel order: c_j is j's original confidence, so bad == (stronger > 0).  Sequence order
 *   (that method's in-place loop): frames are processed i = 0 .. T - 1; c_j is the cleaned confidence of j when j < i and the
 *   original when j > i.  (The original conf_i suffices: before its first clip a pixel holds its original value, and a clip is
 *   idempotent.)  conf_out[q] = (conf < max_bad_conf ? conf : max_bad_conf) for a bad pixel and the input bits otherwise; a NaN
 *   confidence is never bad and passes through.
 *
 * out_host / out_dev: T descriptors sp3_multiview_out, one per frame: counts int32 [h, row_stride, 4] (nullable, 16-byte aligned),
 *   conf_out fp32 [h, row_stride] (nullable), max_bad_conf (not NaN).  Only pixels inside w x h are written.
 * sp3_multiview_counts: ONE launch over all (frame, 16 x 16 pixel block): a lane owns a pixel, a wave an 8 x 8 tile; the descriptor
 *   tables are read by scalar loads only.  Writes counts and, where conf_out is set, the parallel-order cleaning.  0 <= tol < 1;
 *   with any conf_out set every frame needs pixel_weight.  T <= 65535.  T = 0 is a no-op; T = 1 writes zeros and passes the
 *   confidence through.
 * sp3_multiview_clean: the sequence order as T launches of the same kernel; launch i covers frame i only, reads out[j].conf_out
 *   for j < i (written by the earlier launches) and frames[j].pixel_weight for j > i; the launch boundaries are the only hand-offs.
 *   Every conf_out must be non-null.  counts, where set, are the counts against the ORIGINAL confidences, those of the counts call.
 * Both refuse a conf_out that equals a pixel_weight or another conf_out (pointer equality); that the buffers do not overlap in any
 *   other way is the caller's contract. */
typedef struct sp3_multiview_out {
  int32_t* counts;             /* device int32 [h, row_stride, 4]: seen, agree, front, stronger; nullable */
  float* conf_out;             /* device fp32 [h, row_stride]; nullable */
  float max_bad_conf;
} sp3_multiview_out;
int sp3_multiview_counts(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, float tol,
                         const sp3_multiview_out* out_host, const sp3_multiview_out* out_dev, void* stream);
int sp3_multiview_clean(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, float tol,
                        const sp3_multiview_out* out_host, const sp3_multiview_out* out_dev, void* stream);

/* ---- Global alignment (csrc/align.hip; spann3r_amd/align.py) --------------------------------------------------------------
 * A pair graph gives, for every ordered pair e = (i_e, j_e), two pointmaps in i's camera frame and two confidences.  Global
 * alignment looks for ONE set of camera poses, focals and depth maps that explains all pairs at once: the loss below is the
 * confidence-weighted distance between the E pairwise pointmaps, each moved by its own similarity, and the N unprojected depth
 * maps.  It follows PointCloudOptimizer.forward (dust3r/cloud_opt/optimizer.py) with dist = "l1".  Parity with that class is
 * UNPINNED (dust3r.cloud_opt cannot be imported where this is built); tests/align_ref.py restates the rule below in numpy, and a
 * float64 torch statement of the reference's formulas, from its parametrisation down, is the second anchor.  The kernel sees only
 * GEOMETRIC parameters: a log, an exp or a quaternion on the device would not round like numpy, so the parametrisation stays in
 * torch (spann3r_amd/align.py).  No entry point allocates device memory, frees or synchronises.  Every fp32 operation is rounded
 * on its own (`#pragma clang fp contract(off)`), dot products run left to right as written, division and square root are IEEE.
 *
 * Image n (sp3_align_image): depth d fp32 [h, row_stride] (the positive depth itself), c2w = C (row-major 3 x 4), f, (cx, cy),
 *   grad_depth fp32 [h, row_stride] (output, nullable).  Edge e (sp3_align_edge): img = (i_e, j_e); per side s the pointmap
 *   pts[s] fp32 [h, row_stride[s], 3] and the weight[s] fp32 [h, row_stride[s]] of image img[s] (the already transformed
 *   confidence, e.g. log conf); M (row-major 3 x 4, already s_e [R_e | t_e]); a = (axy, axy, az).
 * Items: an item is (e, s); the items of image n are those with img[s] == n, listed as CSR item_first[N + 1], item_edge[2 E],
 *   item_side[2 E].  Every (e, s) must be listed exactly once, under its image.
 * Pixel (u, v) of image n, integer pixel centres, all fp32:
 *     ux = u - cx, vy = v - cy;  rx = ux / f, ry = vy / f;  xc = (d ux) / f, yc = (d vy) / f;  hx = xc / f, hy = yc / f, df = d / f;
 *     X_r = ((C_r0 xc + C_r1 yc) + C_r2 d) + C_r3.
 *   For every item of n, in CSR order, with P, W the item's pointmap and weight at (u, v):
 *     q = a (.) P;  Y_r = ((M_r0 qx + M_r1 qy) + M_r2 qz) + M_r3;  r = X - Y;  rho = sqrt((r0^2 + r1^2) + r2^2);  term = W rho;
 *     g = (W / rho) r, and g = 0 where rho == 0 (torch.norm's backward);  gc_c = (g0 C_0c + g1 C_1c) + g2 C_2c (c = 0..2);
 *     gm_c = (g0 M_0c + g1 M_1c) + g2 M_2c.
 * Loss: L = S_0 / A_0 + S_1 / A_1;  S_s = the fp64 sum of the fp32 terms of side s;  A_s = the pixel count of side s over all
 *   edges (total_area_i / total_area_j of the reference).
 * Outputs, all gradients of L:
 *   grad_depth[u, v] = the fp32 sum over the items of n, in order, of ((gc_0 rx + gc_1 ry) + gc_2) / (float)A_s; stored once.
 *   img_sums fp64 [N, 15]: 0..11 dL/dC (g_r * (xc, yc, d, 1)_c at 4 r + c), 12 dL/df (-(gc_0 hx + gc_1 hy)), 13 / 14
 *     dL/dcx, dL/dcy (-(gc_0 df), -(gc_1 df)).  The products g_r * x_c are taken in fp64 (exact), the rest in fp32 and converted;
 *     every addend is then multiplied by 1.0 / A_s in fp64.
 *   edge_sums fp64 [E, 15], over both items of the edge: 0..11 dL/dM (-(g_r * (qx, qy, qz, 1)_c)), 12..14 dL/da per component
 *     (-(gm_c * P_c)); products in fp64, times 1.0 / A_s.  (a has two free values: dL/daxy = [12] + [13].)
 *   loss3 fp64 [3]: S_0, S_1, L = S_0 * (1 / A_0) + S_1 * (1 / A_1).
 *   All fp64 sums run in a fixed order: in the wave, the four waves in order, one row per (image | edge-side, 16 x 16 block) in ws,
 *   then a second launch adds the rows in index order (the scheme of sp3_icp_accum).  No floating-point atomics: the same bits on
 *   every run.  A non-finite P, W or d propagates; nothing is masked.
 * sp3_align_loss_grad: ONE launch over all (image, 16 x 16 block) plus the finishing launch; a lane owns a pixel, a wave an 8 x 8
 *   tile.  Tables are given as host and device copies; every index, stride and size is checked on the host copies before anything
 *   is launched: N in 1..4096, E in 1..65536, T = blocks of the largest image <= 65536, f != 0, image indices, sides, the CSR.
 *   ws: sp3_align_loss_grad_ws_bytes(N, E, wmax, hmax) bytes, 8-byte aligned.
 * sp3_align_moments: for B triples (src, dst, w) of [n_b, 3] / [n_b] fp32 the 17 fp64 sums of a weighted similarity registration,
 *   out fp64 [B, 17]: 0 sum w;  1..3 sum w p;  4..6 sum w q;  7..15 sum w p q^T (3 r + c: p_r q_c);  16 sum w |p|^2 (p = src, q = dst;
 *   every product in fp64, (w p_r) first).  Same reduction scheme, one slab of min(ceil(n_b / 256), 1024) rows per triple.
 *   B in 1..65535, n_b in 1..2^31 / 3.  ws: sp3_align_moments_ws_bytes(B, max n_b). */
typedef struct sp3_align_image {
  const float* depth;          /* device fp32 [h, row_stride] */
  float* grad_depth;           /* device fp32 [h, row_stride]; nullable */
  int64_t row_stride;
  int32_t w, h;
  float f, cx, cy;
  float c2w[12];
} sp3_align_image;
typedef struct sp3_align_edge {
  const float* pts[2];         /* device fp32 [h, row_stride[s], 3] of image img[s] */
  const float* weight[2];      /* device fp32 [h, row_stride[s]] */
  int64_t row_stride[2];
  int32_t img[2];              /* (i_e, j_e) */
  float M[12];
  float a[3];
} sp3_align_edge;
typedef struct sp3_align_triple {
  const float* src;            /* device fp32 [n, 3] */
  const float* dst;            /* device fp32 [n, 3] */
  const float* w;              /* device fp32 [n] */
  int64_t n;
} sp3_align_triple;
int64_t sp3_align_loss_grad_ws_bytes(int N, int E, int wmax, int hmax);
int sp3_align_loss_grad(const sp3_align_image* imgs_host, const sp3_align_image* imgs_dev, int N, const sp3_align_edge* edges_host,
                        const sp3_align_edge* edges_dev, int E, const int* item_first_host, const int* item_edge_host,
                        const int* item_side_host, const int* item_first_dev, const int* item_edge_dev, const int* item_side_dev,
                        void* ws, double* img_sums, double* edge_sums, double* loss3, void* stream);
int64_t sp3_align_moments_ws_bytes(int B, int64_t nmax);
int sp3_align_moments(const sp3_align_triple* tr_host, const sp3_align_triple* tr_dev, int B, void* ws, double* out, void* stream);

/* small utilities */
/* n (1..8) contiguous device-to-device copies in one launch; every copy 16-byte aligned and a multiple of 16 bytes.
 * (The sequence loop's per-frame bookkeeping -- torch .clone() / slice assignments around spann3r/model.py:523-531.) */
int sp3_copy_multi(int n, const void* const* src, void* const* dst, const int64_t* bytes, void* stream);
int sp3_copy2d_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int cols, void* stream);
int sp3_fill_f32(float* p, float v, int64_t n, void* stream);
int sp3_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
/* Measurement aid (bench.py): a one-wave kernel that spins `cycles` shader clocks and stores its own duration in ticks of
 * the constant 100 MHz counter: a kernel of known length to calibrate the cost of a HIP-event bracket against. */
int sp3_spin(int64_t cycles, int64_t* ticks_100mhz, void* stream);

#ifdef __cplusplus
}
#endif
#endif
