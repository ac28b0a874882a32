// Global alignment of a pair graph (include/spann3r_hip.h, "Global alignment"; spann3r_amd/align.py drives these): the
// confidence-weighted distance between E transformed pairwise pointmaps and N unprojected depth maps, with its gradient for every
// pixel's depth, every camera and every pair, in ONE launch that stores nothing per edge.
//
// k_align: a lane owns pixel (u, v) of image n (n from blockIdx.z), a wave an 8 x 8 tile and a workgroup a 16 x 16 block, as in
// k_multiview.  The loop over the items (edge, side) of the image is workgroup-uniform: its bounds and the descriptors of both tables
// arrive by scalar loads of read-only tables.  The pixel's unprojection, its depth gradient (fp32) and the 15 + 2 running sums of
// its image (fp64) stay in registers over the whole loop; the 15 sums of an item are reduced at once: in the wave by four DPP steps
// inside a row of 16 and two ds_bpermute steps across rows (wave_sum_f64), the four waves through LDS in wave order (two buffers,
// so one barrier per item), one row of the partial slab per (edge, side, block).
// k_align_finish adds the rows in index order.  No atomics; a lane outside its image takes part in every reduction with zeros.
//
// k_moments: the 17 weighted registration sums of B point-set triples, by the slab scheme of csrc/slab.h with one slab per triple.
//
// Every fp32 operation is rounded on its own (no contraction into FMAs): the file-level pragma below.
#include "common.h"
#include "slab.h"
#include "tsdf.h"
#include <math.h>

#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int ALIGN_MAX_N = 4096, ALIGN_MAX_E = 65536, ALIGN_MAX_TILES = 65536, MOMENTS_MAX_B = 65535;
constexpr int NI = 17, NE = 15;      // sums per (image, block): 15 + the two S_side; per (edge, side, block)

// One lane's fp64 value from the lane a DPP control names (both halves move as 32-bit DPP movs: full-rate VALU, no LDS crossbar).
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// The sum over the 64 lanes, in every lane, in a fixed order; all 64 lanes must be active.  The four steps inside a row of 16 go
// through DPP: quad_perm [1,0,3,2] and [2,3,0,1] (lane ^ 1, lane ^ 2), then row_half_mirror and row_mirror, which pair a lane with
// 7 - l and 15 - l -- the lanes of the other quad / other half, all of which hold the same partial sum by then.  Only the last two
// steps (lane ^ 16, lane ^ 32) cross rows and go through ds_bpermute: 60 instead of 180 crossbar operations for 15 sums.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

__global__ __launch_bounds__(RC_TILE * RC_TILE) void k_align(const sp3_align_image* __restrict__ imgs, const sp3_align_edge* __restrict__ edges,
                                                            const int* __restrict__ item_first, const int* __restrict__ item_edge,
                                                            const int* __restrict__ item_side, int N, int E, float Af0, float Af1, double invA0,
                                                            double invA1, double* __restrict__ ws) {
  __shared__ double sh[2][4][NE];
  __shared__ double shi[4][NI];
  const int n = (int)blockIdx.z;      // (workgroup-uniform, as the item loop below: descriptor fields arrive by scalar loads)
  const sp3_align_image& im = imgs[n];
  if ((int)blockIdx.x * RC_TILE >= im.w || (int)blockIdx.y * RC_TILE >= im.h) return;      // the whole workgroup lies outside
  const int tiles = (int)(gridDim.x * gridDim.y), slot = (int)(blockIdx.y * gridDim.x + blockIdx.x);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
  const int v = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool in = u < im.w && v < im.h;      // a lane outside reads pixel (0, 0) and adds zeros
  const int64_t q = in ? (int64_t)v * im.row_stride + u : 0;
  const float* C = im.c2w;
  const float f = im.f;
  const float d = im.depth[q];
  const float ux = (float)u - im.cx, vy = (float)v - im.cy;
  const float rx = ux / f, ry = vy / f;                    // dX_cam / dd = (rx, ry, 1)
  const float xc = (d * ux) / f, yc = (d * vy) / f;        // X_cam = (xc, yc, d)
  const float hx = xc / f, hy = yc / f, df_ = d / f;
  const float X0 = ((C[0] * xc + C[1] * yc) + C[2] * d) + C[3];
  const float X1 = ((C[4] * xc + C[5] * yc) + C[6] * d) + C[7];
  const float X2 = ((C[8] * xc + C[9] * yc) + C[10] * d) + C[11];
  float gd = 0.f;
  double acc[NI];
#pragma unroll
  for (int c = 0; c < NI; ++c) acc[c] = 0.0;
  const int k0 = item_first[n], k1 = item_first[n + 1];
  for (int k = k0; k < k1; ++k) {
    const int e = item_edge[k], s = item_side[k];
    const sp3_align_edge& ed = edges[e];
    // (both sides' pointers and strides are loaded, the side is chosen among scalars: an index by s would make the load a vector one)
    const float* pts = s ? ed.pts[1] : ed.pts[0];
    const float* wgt = s ? ed.weight[1] : ed.weight[0];
    const int64_t rs = s ? ed.row_stride[1] : ed.row_stride[0];
    const int64_t p = in ? (int64_t)v * rs + u : 0;
    const float* P = pts + 3 * p;
    const float Px = P[0], Py = P[1], Pz = P[2], W = wgt[p];
    const float* M = ed.M;
    const float qx = ed.a[0] * Px, qy = ed.a[1] * Py, qz = ed.a[2] * Pz;
    const float Y0 = ((M[0] * qx + M[1] * qy) + M[2] * qz) + M[3];
    const float Y1 = ((M[4] * qx + M[5] * qy) + M[6] * qz) + M[7];
    const float Y2 = ((M[8] * qx + M[9] * qy) + M[10] * qz) + M[11];
    const float r0 = X0 - Y0, r1 = X1 - Y1, r2 = X2 - Y2;
    const float rho = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
    const float term = W * rho;
    const float kk = W / rho;
    const bool zero = rho == 0.f;      // (torch.norm's backward: a zero gradient at a zero residual; a NaN is not zero)
    const float g0 = zero ? 0.f : kk * r0, g1 = zero ? 0.f : kk * r1, g2 = zero ? 0.f : kk * r2;
    const float gcx = (g0 * C[0] + g1 * C[4]) + g2 * C[8];      // the gradient in the camera frame
    const float gcy = (g0 * C[1] + g1 * C[5]) + g2 * C[9];
    const float gcz = (g0 * C[2] + g1 * C[6]) + g2 * C[10];
    const float Af = s ? Af1 : Af0;
    const double iA = s ? invA1 : invA0;
    gd += ((gcx * rx + gcy * ry) + gcz) / Af;
    const float gf = -(gcx * hx + gcy * hy), gpx = -(gcx * df_), gpy = -(gcy * df_);
    const float gm0 = (g0 * M[0] + g1 * M[4]) + g2 * M[8];
    const float gm1 = (g0 * M[1] + g1 * M[5]) + g2 * M[9];
    const float gm2 = (g0 * M[2] + g1 * M[6]) + g2 * M[10];
    const double G[3] = {(double)g0, (double)g1, (double)g2};
    const double xh[4] = {(double)xc, (double)yc, (double)d, 1.0}, qh[4] = {(double)qx, (double)qy, (double)qz, 1.0};
    double ev[NE];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[4 * r + c] += in ? (G[r] * xh[c]) * iA : 0.0;
        ev[4 * r + c] = in ? -(G[r] * qh[c]) * iA : 0.0;
      }
    }
    acc[12] += in ? (double)gf * iA : 0.0;
    acc[13] += in ? (double)gpx * iA : 0.0;
    acc[14] += in ? (double)gpy * iA : 0.0;
    acc[15] += in && s == 0 ? (double)term : 0.0;
    acc[16] += in && s == 1 ? (double)term : 0.0;
    ev[12] = in ? -((double)gm0 * (double)Px) * iA : 0.0;
    ev[13] = in ? -((double)gm1 * (double)Py) * iA : 0.0;
    ev[14] = in ? -((double)gm2 * (double)Pz) * iA : 0.0;
#pragma unroll
    for (int c = 0; c < NE; ++c) ev[c] = wave_sum_f64(ev[c]);
    const int b = (k - k0) & 1;
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < NE; ++c) sh[b][wave][c] = ev[c];
    }
    __syncthreads();      // (the next item writes the other buffer; this one is written again only behind the next barrier)
    if (threadIdx.x < NE) {
      const int c = threadIdx.x;
      ws[(int64_t)N * tiles * NI + (((int64_t)e * 2 + s) * tiles + slot) * NE + c] = ((sh[b][0][c] + sh[b][1][c]) + sh[b][2][c]) + sh[b][3][c];
    }
  }
  if (in && im.grad_depth != nullptr) im.grad_depth[q] = gd;
#pragma unroll
  for (int c = 0; c < NI; ++c) acc[c] = wave_sum_f64(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NI; ++c) shi[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < NI) {
    const int c = threadIdx.x;
    ws[((int64_t)n * tiles + slot) * NI + c] = ((shi[0][c] + shi[1][c]) + shi[2][c]) + shi[3][c];
  }
}

// blocks 0 .. N-1: the 15 sums of image n; N .. N+E-1: the 15 sums of edge e (side 0's rows, then side 1's); N+E: S_0, S_1, L.
// Only the rows of blocks inside the image were written, and only those are read, in (ty, tx) order.
__global__ __launch_bounds__(64) void k_align_finish(const sp3_align_image* __restrict__ imgs, const sp3_align_edge* __restrict__ edges, int N, int E,
                                                    int gx, int gy, double invA0, double invA1, const double* __restrict__ ws,
                                                    double* __restrict__ img_sums, double* __restrict__ edge_sums, double* __restrict__ loss3) {
  const int b = (int)blockIdx.x, c = (int)threadIdx.x, tiles = gx * gy;
  if (b < N) {
    if (c >= 15) return;
    const int tx = (imgs[b].w + RC_TILE - 1) / RC_TILE, ty = (imgs[b].h + RC_TILE - 1) / RC_TILE;
    double s = 0.0;
    for (int y = 0; y < ty; ++y)
      for (int x = 0; x < tx; ++x) s += ws[((int64_t)b * tiles + y * gx + x) * NI + c];
    img_sums[(int64_t)b * 15 + c] = s;
  } else if (b < N + E) {
    if (c >= NE) return;
    const int e = b - N;
    double s = 0.0;
    for (int side = 0; side < 2; ++side) {
      const sp3_align_image& im = imgs[edges[e].img[side]];
      const int tx = (im.w + RC_TILE - 1) / RC_TILE, ty = (im.h + RC_TILE - 1) / RC_TILE;
      for (int y = 0; y < ty; ++y)
        for (int x = 0; x < tx; ++x) s += ws[(int64_t)N * tiles * NI + (((int64_t)e * 2 + side) * tiles + y * gx + x) * NE + c];
    }
    edge_sums[(int64_t)e * NE + c] = s;
  } else {
    __shared__ double S[2];
    if (c < 2) {
      double s = 0.0;
      for (int n = 0; n < N; ++n) {
        const int tx = (imgs[n].w + RC_TILE - 1) / RC_TILE, ty = (imgs[n].h + RC_TILE - 1) / RC_TILE;
        for (int y = 0; y < ty; ++y)
          for (int x = 0; x < tx; ++x) s += ws[((int64_t)n * tiles + y * gx + x) * NI + 15 + c];
      }
      S[c] = s;
      loss3[c] = s;
    }
    __syncthreads();
    if (c == 0) loss3[2] = S[0] * invA0 + S[1] * invA1;
  }
}

__device__ __forceinline__ int moments_blocks(int64_t n) { return (int)((n + 255) / 256 < SLAB_BLOCKS ? (n + 255) / 256 : SLAB_BLOCKS); }

__global__ __launch_bounds__(256) void k_moments(const sp3_align_triple* __restrict__ tr, double* __restrict__ ws) {
  const sp3_align_triple& t = tr[blockIdx.y];
  const int nb = moments_blocks(t.n);
  if ((int)blockIdx.x >= nb) return;
  double v[17];
#pragma unroll
  for (int e = 0; e < 17; ++e) v[e] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)nb * 256) {
    const double w = t.w[i], px = t.src[3 * i], py = t.src[3 * i + 1], pz = t.src[3 * i + 2];
    const double qx = t.dst[3 * i], qy = t.dst[3 * i + 1], qz = t.dst[3 * i + 2];
    const double wx = w * px, wy = w * py, wz = w * pz;
    v[0] += w;
    v[1] += wx; v[2] += wy; v[3] += wz;
    v[4] += w * qx; v[5] += w * qy; v[6] += w * qz;
    v[7] += wx * qx; v[8] += wx * qy; v[9] += wx * qz;
    v[10] += wy * qx; v[11] += wy * qy; v[12] += wy * qz;
    v[13] += wz * qx; v[14] += wz * qy; v[15] += wz * qz;
    v[16] += (wx * px + wy * py) + wz * pz;
  }
  block_slab<17>(v, ws + (int64_t)blockIdx.y * gridDim.x * 17);
}

__global__ __launch_bounds__(64) void k_moments_finish(const sp3_align_triple* __restrict__ tr, int gx, const double* __restrict__ ws,
                                                      double* __restrict__ out) {
  if (threadIdx.x >= 17) return;
  const int b = (int)blockIdx.x, nb = moments_blocks(tr[b].n);
  double s = 0.0;
  for (int x = 0; x < nb; ++x) s += ws[((int64_t)b * gx + x) * 17 + threadIdx.x];
  out[(int64_t)b * 17 + threadIdx.x] = s;
}

int host_blocks(int64_t n) { return slab_blocks(n); }

// the checks of sp3_align_loss_grad on the host copies -> the grid of the largest image and the two areas
int check_align(const sp3_align_image* imgs, int N, const sp3_align_edge* edges, int E, const int* item_first, const int* item_edge,
                const int* item_side, int& gx, int& gy, double (&A)[2]) {
  const char* what = "sp3_align_loss_grad";
  SP3_CHECK(N >= 1 && N <= ALIGN_MAX_N, "%s: N %d must lie in 1..%d", what, N, ALIGN_MAX_N);
  SP3_CHECK(E >= 1 && E <= ALIGN_MAX_E, "%s: E %d must lie in 1..%d", what, E, ALIGN_MAX_E);
  SP3_CHECK(imgs != nullptr && edges != nullptr && item_first != nullptr && item_edge != nullptr && item_side != nullptr, "%s: null table", what);
  int wmax = 0, hmax = 0;
  for (int n = 0; n < N; ++n) {
    const sp3_align_image& im = imgs[n];
    SP3_CHECK(im.depth != nullptr, "%s: image %d: null depth", what, n);
    SP3_CHECK(im.w >= 1 && im.h >= 1 && im.row_stride >= im.w && (int64_t)im.h * im.row_stride < ((int64_t)1 << 31),
              "%s: image %d: bad geometry w %d h %d row_stride %lld", what, n, im.w, im.h, (long long)im.row_stride);
    SP3_CHECK(im.f != 0.f, "%s: image %d: f == 0", what, n);
    wmax = im.w > wmax ? im.w : wmax;
    hmax = im.h > hmax ? im.h : hmax;
  }
  gx = (wmax + RC_TILE - 1) / RC_TILE;
  gy = (hmax + RC_TILE - 1) / RC_TILE;
  SP3_CHECK((int64_t)gx * gy <= ALIGN_MAX_TILES, "%s: T %lld blocks per image must stay within %d", what, (long long)gx * gy, ALIGN_MAX_TILES);
  A[0] = A[1] = 0.0;
  for (int e = 0; e < E; ++e) {
    const sp3_align_edge& ed = edges[e];
    for (int s = 0; s < 2; ++s) {
      SP3_CHECK(ed.img[s] >= 0 && ed.img[s] < N, "%s: edge %d: image index %d outside 0..%d", what, e, ed.img[s], N - 1);
      const sp3_align_image& im = imgs[ed.img[s]];
      SP3_CHECK(ed.pts[s] != nullptr && ed.weight[s] != nullptr, "%s: edge %d side %d: null pts / weight", what, e, s);
      SP3_CHECK(ed.row_stride[s] >= im.w && (int64_t)im.h * ed.row_stride[s] < ((int64_t)1 << 31),
                "%s: edge %d side %d: row_stride %lld below the width %d of image %d or too large", what, e, s, (long long)ed.row_stride[s], im.w,
                ed.img[s]);
      A[s] += (double)im.w * (double)im.h;
    }
  }
  SP3_CHECK(item_first[0] == 0 && item_first[N] == 2 * E, "%s: item_first must run from 0 to 2 E = %d (got %d .. %d)", what, 2 * E, item_first[0],
            item_first[N]);
  for (int n = 0; n < N; ++n)
    SP3_CHECK(item_first[n] <= item_first[n + 1], "%s: item_first decreases at image %d", what, n);
  std::vector<char> seen((size_t)2 * E, 0);
  for (int n = 0; n < N; ++n) {
    for (int k = item_first[n]; k < item_first[n + 1]; ++k) {
      const int e = item_edge[k], s = item_side[k];
      SP3_CHECK(e >= 0 && e < E, "%s: item %d: edge index %d outside 0..%d", what, k, e, E - 1);
      SP3_CHECK(s == 0 || s == 1, "%s: item %d: side %d is neither 0 nor 1", what, k, s);
      SP3_CHECK(edges[e].img[s] == n, "%s: item %d (edge %d side %d) is listed under image %d but belongs to image %d", what, k, e, s, n,
                edges[e].img[s]);
      SP3_CHECK(!seen[2 * e + s], "%s: (edge %d, side %d) is listed twice", what, e, s);
      seen[2 * e + s] = 1;
    }
  }      // (2 E items, none twice: each (edge, side) exactly once)
  return 0;
}

int64_t align_ws_doubles(int N, int E, int gx, int gy) { return (int64_t)gx * gy * ((int64_t)N * NI + (int64_t)E * 2 * NE); }

}  // namespace

extern "C" int64_t sp3_align_loss_grad_ws_bytes(int N, int E, int wmax, int hmax) {
  if (N < 1 || E < 1 || wmax < 1 || hmax < 1) return 0;
  return align_ws_doubles(N, E, (wmax + RC_TILE - 1) / RC_TILE, (hmax + RC_TILE - 1) / RC_TILE) * 8;
}

extern "C" int sp3_align_loss_grad(const sp3_align_image* imgs_host, const sp3_align_image* imgs_dev, int N, const sp3_align_edge* edges_host,
                                   const sp3_align_edge* edges_dev, int E, const int* item_first_host, const int* item_edge_host,
                                   const int* item_side_host, const int* item_first_dev, const int* item_edge_dev, const int* item_side_dev,
                                   void* ws, double* img_sums, double* edge_sums, double* loss3, void* stream) {
  int gx, gy;
  double A[2];
  if (check_align(imgs_host, N, edges_host, E, item_first_host, item_edge_host, item_side_host, gx, gy, A)) return 1;
  SP3_CHECK(ws != nullptr && img_sums != nullptr && edge_sums != nullptr && loss3 != nullptr, "sp3_align_loss_grad: null ws / output");
  SP3_CHECK(imgs_dev != nullptr && edges_dev != nullptr && item_first_dev != nullptr && item_edge_dev != nullptr && item_side_dev != nullptr,
            "sp3_align_loss_grad: null device copy of a table");      // (last: nothing launches without it)
  hipStream_t st = (hipStream_t)stream;
  const double iA0 = 1.0 / A[0], iA1 = 1.0 / A[1];
  hipLaunchKernelGGL(k_align, dim3(gx, gy, N), dim3(RC_TILE * RC_TILE), 0, st, imgs_dev, edges_dev, item_first_dev, item_edge_dev, item_side_dev, N, E,
                     (float)A[0], (float)A[1], iA0, iA1, (double*)ws);
  hipLaunchKernelGGL(k_align_finish, dim3(N + E + 1), dim3(64), 0, st, imgs_dev, edges_dev, N, E, gx, gy, iA0, iA1, (const double*)ws, img_sums,
                     edge_sums, loss3);
  SP3_LAUNCH_CHECK("sp3_align_loss_grad");
  return 0;
}

extern "C" int64_t sp3_align_moments_ws_bytes(int B, int64_t nmax) {
  if (B < 1 || nmax < 1) return 0;
  return (int64_t)B * host_blocks(nmax) * 17 * 8;
}

extern "C" int sp3_align_moments(const sp3_align_triple* tr_host, const sp3_align_triple* tr_dev, int B, void* ws, double* out, void* stream) {
  SP3_CHECK(B >= 1 && B <= MOMENTS_MAX_B, "sp3_align_moments: B %d must lie in 1..%d", B, MOMENTS_MAX_B);
  SP3_CHECK(tr_host != nullptr, "sp3_align_moments: null table");
  int64_t nmax = 0;
  for (int b = 0; b < B; ++b) {
    const sp3_align_triple& t = tr_host[b];
    SP3_CHECK(t.src != nullptr && t.dst != nullptr && t.w != nullptr, "sp3_align_moments: triple %d: null pointer", b);
    SP3_CHECK(t.n >= 1 && t.n <= ((int64_t)1 << 31) / 3, "sp3_align_moments: triple %d: n = %lld out of range", b, (long long)t.n);
    nmax = t.n > nmax ? t.n : nmax;
  }
  SP3_CHECK(ws != nullptr && out != nullptr, "sp3_align_moments: null ws / output");
  SP3_CHECK(tr_dev != nullptr, "sp3_align_moments: null device copy of the table");      // (last: nothing launches without it)
  const int gx = host_blocks(nmax);
  hipLaunchKernelGGL(k_moments, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, tr_dev, (double*)ws);
  hipLaunchKernelGGL(k_moments_finish, dim3(B), dim3(64), 0, (hipStream_t)stream, tr_dev, gx, (const double*)ws, out);
  SP3_LAUNCH_CHECK("sp3_align_moments");
  return 0;
}
