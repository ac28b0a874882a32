// Reconstruction metrics on the device (reference: eval.py:189-231, spann3r/tools/eval_recon.py): exact nearest-neighbour
// search between two point clouds, k-NN / PCA normals, and the correspondence sums of point-to-point ICP.
//
//   * The reference cloud is binned into a uniform cell grid (host picks origin / edge h / dims, spann3r_amd/cell_grid.py);
//     its points are stored sorted by cell as 16-byte records (x, y, z, original index) with a cell-start table.
//   * A query walks the cells around its home cell ring by ring until its best (k-th best) distance is within the bound of
//     the walked block: csrc/cell_grid.h states the walk, the bound and its slack, and why the result is exact.
//   * Queries still open after `max_ring` rings go to an LDS-tiled brute-force kernel, the reference cloud split over workgroups
//     and joined by a 64-bit integer atomicMin of (distance bits, index): order-free, so results are bit-reproducible.
//   * Distances are direct differences.  dist2 uses the _rn intrinsics, which this compiler defines as plain operators: the sum is
//     contracted into two FMAs, so d2 is within eval_ref.dist_bound but NOT bit-equal to a numpy fp32 restatement (unfusing moves bits).
//   * Sums (ICP correspondences, metric means) are fp64 per workgroup into partial slabs, finished by a second kernel in a
//     fixed order: no float atomics.
#include "cell_grid.h"
#include "slab.h"

namespace {

constexpr int KNN_MAX = 32;
constexpr int KNN_BLOCK = 128;
constexpr int BRUTE_TILE = 1024;

struct Rec { float x, y, z; int i; };   // 16 bytes: one global_load_dwordx4 / ds_read_b128 per point
static_assert(sizeof(Rec) == 16, "record size");

__device__ __forceinline__ Rec ld_rec(const float4* p) {
  const float4 v = *p;
  Rec r; r.x = v.x; r.y = v.y; r.z = v.z; r.i = __float_as_int(v.w);
  return r;
}

// (ax-bx)^2 + (ay-by)^2 + (az-bz)^2; the differences are rounded on their own, the sum compiles to a product and two FMAs (above)
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__global__ __launch_bounds__(256) void cell_ids_kernel(const float* __restrict__ pts, int64_t n, sp3_nn_grid g, int* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Cell c = cell_of(g, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
  ids[i] = cell_id(g, c.x, c.y, c.z);
}

__global__ __launch_bounds__(256) void pack_records_kernel(const float* __restrict__ pts, const int64_t* __restrict__ order, int64_t n,
                                                           float4* __restrict__ recs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t s = order ? order[i] : i;
  recs[i] = make_float4(pts[3 * s], pts[3 * s + 1], pts[3 * s + 2], __int_as_float((int)s));
}

// ---- exact 1-NN, one lane per query (queries sorted by home cell: the lanes of a wave walk the same cells)
__global__ __launch_bounds__(256) void nn_grid_kernel(const float* __restrict__ q, const int64_t* __restrict__ order, int64_t nq,
                                                      const float4* __restrict__ recs, const int* __restrict__ cell_start, sp3_nn_grid g,
                                                      int max_ring, float max_dist, float* __restrict__ dist, int* __restrict__ idx,
                                                      GridHead* head, unsigned long long* __restrict__ fb_key, int* __restrict__ fb_list) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int cells = 0, points = 0;
  if (t < nq) {
    const int64_t qi = order ? order[t] : t;
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    float best = INFINITY;
    int bi = -1;
    const auto scan = [&](int s, int e) {
      points += e - s;
      for (int j = s; j < e; ++j) {
        const Rec p = ld_rec(recs + j);
        const float d2 = dist2(qx, qy, qz, p.x, p.y, p.z);
        if (d2 < best) { best = d2; bi = p.i; }
      }
    };
    // settled: everything unvisited is farther than the best, or farther than max_dist (then the best decides alone)
    if (walk_rings(g, cell_start, qx, qy, qz, max_ring, cells, scan, [&](float b) { return best <= b * b || b >= max_dist; })) {
      const float d = __fsqrt_rn(best);
      const bool hit = bi >= 0 && d <= max_dist;
      dist[qi] = hit ? d : INFINITY;
      idx[qi] = hit ? bi : -1;
    } else {
      head->open_slot(qi, fb_list, fb_key);
    }
  }
  head->count(cells, points);
}

// ---- brute force: a workgroup holds 256 queries in registers and streams its chunk of the reference cloud through LDS.
// slots: the fallback list or every query (cell_grid.h Slots).  key[slot] = min (d2 bits << 32 | index).
__global__ __launch_bounds__(256) void nn_brute_kernel(const float* __restrict__ q, Slots slots, const float4* __restrict__ recs, int64_t m,
                                                       int64_t chunk, unsigned long long* __restrict__ key) {
  __shared__ float4 tile[BRUTE_TILE];
  const int64_t nq = slots.size();
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(r0 + chunk, m);
  for (int64_t qb = (int64_t)blockIdx.x * 256; qb < nq; qb += (int64_t)gridDim.x * 256) {
    const int64_t slot = qb + threadIdx.x;
    const int64_t qi = slot < nq ? slots.query(slot) : -1;
    const bool active = qi >= 0;
    const float qx = active ? q[3 * qi] : 0.f, qy = active ? q[3 * qi + 1] : 0.f, qz = active ? q[3 * qi + 2] : 0.f;
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int64_t t0 = r0; t0 < r1; t0 += BRUTE_TILE) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < BRUTE_TILE / 256; ++k) {
        const int64_t j = t0 + threadIdx.x + k * 256;
        if (j < r1) tile[threadIdx.x + k * 256] = recs[j];
      }
      __syncthreads();
      const int cnt = (int)min((int64_t)BRUTE_TILE, r1 - t0);
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) {
        const Rec p = ld_rec(tile + j);   // same address in every lane: an LDS broadcast
        const float d2 = dist2(qx, qy, qz, p.x, p.y, p.z);
        if (d2 < best || (d2 == best && p.i < bi)) { best = d2; bi = p.i; }
      }
    }
    if (active && r0 < r1)
      atomicMin(&key[slot], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bi);   // d2 >= 0: bit order = value order
  }
}

__global__ __launch_bounds__(256) void fill_u64_kernel(unsigned long long* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = ~0ull;
}

__global__ __launch_bounds__(256) void nn_brute_finish_kernel(Slots slots, const unsigned long long* __restrict__ key, float max_dist,
                                                              float* __restrict__ dist, int* __restrict__ idx) {
  const int64_t nq = slots.size();
  for (int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x; slot < nq; slot += (int64_t)gridDim.x * 256) {
    const unsigned long long k = key[slot];
    const int64_t qi = slots.query(slot);
    if (qi < 0) continue;
    const float d = __fsqrt_rn(__uint_as_float((unsigned)(k >> 32)));
    const bool hit = k != ~0ull && d <= max_dist;
    dist[qi] = hit ? d : INFINITY;
    idx[qi] = hit ? (int)(unsigned)(k & 0xffffffffu) : -1;
  }
}

// ---- k-NN (k <= 32): same rings, the stopping test on the k-th best.  The per-lane candidate list (ascending) lives in LDS,
// [slot][lane] so that the lanes of a wave hit consecutive banks.
__global__ __launch_bounds__(KNN_BLOCK) void knn_grid_kernel(const float* __restrict__ q, const int64_t* __restrict__ order, int64_t nq,
                                                             const float4* __restrict__ recs, const int* __restrict__ cell_start, sp3_nn_grid g,
                                                             int k, float max_dist, float* __restrict__ dist, int* __restrict__ idx) {
  __shared__ float kd[KNN_MAX][KNN_BLOCK];
  __shared__ int ki[KNN_MAX][KNN_BLOCK];
  const int l = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * KNN_BLOCK + l;
  if (t >= nq) return;
  const int64_t qi = order ? order[t] : t;
  const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
  for (int j = 0; j < k; ++j) { kd[j][l] = INFINITY; ki[j][l] = -1; }
  float kth = INFINITY;
  int cells = 0;
  const auto scan = [&](int s, int e) {
    for (int j = s; j < e; ++j) {
      const Rec p = ld_rec(recs + j);
      const float d2 = dist2(qx, qy, qz, p.x, p.y, p.z);
      if (d2 < kth) {
        int u = k - 1;
        while (u > 0 && kd[u - 1][l] > d2) { kd[u][l] = kd[u - 1][l]; ki[u][l] = ki[u - 1][l]; --u; }
        kd[u][l] = d2; ki[u][l] = p.i;
        kth = kd[k - 1][l];
      }
    }
  };
  // no ring budget: the block of ring max(dims) - 1 covers the whole grid
  walk_rings(g, cell_start, qx, qy, qz, max(g.nx, max(g.ny, g.nz)) - 1, cells, scan, [&](float b) { return kth <= b * b; });
  for (int j = 0; j < k; ++j) {
    const float d = __fsqrt_rn(kd[j][l]);
    const bool hit = ki[j][l] >= 0 && d <= max_dist;
    dist[qi * k + j] = hit ? d : INFINITY;
    idx[qi * k + j] = hit ? ki[j][l] : -1;
  }
}

// ---- normals: covariance of the k neighbours about their mean (fp64 on centred values), unit eigenvector of the smallest
// eigenvalue of the symmetric 3x3 (closed-form eigenvalues, eigenvector = the best-conditioned cross product of two rows of A - lambda I)
__global__ __launch_bounds__(256) void knn_normals_kernel(const float* __restrict__ pts, const int* __restrict__ nbr, int64_t n, int k,
                                                          float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* nb = nbr + i * k;
  double mx = 0, my = 0, mz = 0;
  int cnt = 0;
  for (int j = 0; j < k; ++j) {
    const int64_t s = nb[j];
    if (s < 0) continue;
    mx += pts[3 * s]; my += pts[3 * s + 1]; mz += pts[3 * s + 2];
    ++cnt;
  }
  double nx = 0, ny = 0, nz = 1;
  if (cnt >= 3) {
    mx /= cnt; my /= cnt; mz /= cnt;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
    for (int j = 0; j < k; ++j) {
      const int64_t s = nb[j];
      if (s < 0) continue;
      const double x = pts[3 * s] - mx, y = pts[3 * s + 1] - my, z = pts[3 * s + 2] - mz;
      a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
    }
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double qm = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - qm, b11 = a11 - qm, b22 = a22 - qm;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    if (p > 0.0) {
      const double det = b00 * (b11 * b22 - a12 * a12) - a01 * (a01 * b22 - a12 * a02) + a02 * (a01 * a12 - b11 * a02);
      double r = det / (2.0 * p * p * p);
      r = fmin(fmax(r, -1.0), 1.0);
      const double lam = qm + 2.0 * p * cos(acos(r) / 3.0 + 2.0943951023931954923);   // the smallest eigenvalue
      const double r0x = a00 - lam, r0y = a01, r0z = a02, r1x = a01, r1y = a11 - lam, r1z = a12, r2x = a02, r2y = a12, r2z = a22 - lam;
      const double c0x = r0y * r1z - r0z * r1y, c0y = r0z * r1x - r0x * r1z, c0z = r0x * r1y - r0y * r1x;
      const double c1x = r0y * r2z - r0z * r2y, c1y = r0z * r2x - r0x * r2z, c1z = r0x * r2y - r0y * r2x;
      const double c2x = r1y * r2z - r1z * r2y, c2y = r1z * r2x - r1x * r2z, c2z = r1x * r2y - r1y * r2x;
      const double n0 = c0x * c0x + c0y * c0y + c0z * c0z, n1 = c1x * c1x + c1y * c1y + c1z * c1z, n2 = c2x * c2x + c2y * c2y + c2z * c2z;
      double vx = c0x, vy = c0y, vz = c0z, vn = n0;
      if (n1 > vn) { vx = c1x; vy = c1y; vz = c1z; vn = n1; }
      if (n2 > vn) { vx = c2x; vy = c2y; vz = c2z; vn = n2; }
      if (vn > 0.0) { const double s = 1.0 / sqrt(vn); nx = vx * s; ny = vy * s; nz = vz * s; }
    }
  }
  out[3 * i] = (float)nx; out[3 * i + 1] = (float)ny; out[3 * i + 2] = (float)nz;
}

struct Rigid { double m[12]; };   // row-major R (9) | t (3)

__global__ __launch_bounds__(256) void transform_points_kernel(const float* __restrict__ src, int64_t n, Rigid T, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  out[3 * i] = (float)(T.m[0] * x + T.m[1] * y + T.m[2] * z + T.m[9]);
  out[3 * i + 1] = (float)(T.m[3] * x + T.m[4] * y + T.m[5] * z + T.m[10]);
  out[3 * i + 2] = (float)(T.m[6] * x + T.m[7] * y + T.m[8] * z + T.m[11]);
}

// (p_i, q = tgt[idx_i]) for idx_i >= 0: count, sum p (3), sum q (3), sum p q^T (9, row-major), sum |p - q|^2
__global__ __launch_bounds__(256) void icp_accum_kernel(const float* __restrict__ p, const float* __restrict__ tgt, const int* __restrict__ idx,
                                                        int64_t n, double* __restrict__ slab) {
  double v[17];
#pragma unroll
  for (int e = 0; e < 17; ++e) v[e] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t j = idx[i];
    if (j < 0) continue;
    const double px = p[3 * i], py = p[3 * i + 1], pz = p[3 * i + 2], qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
    v[0] += 1.0;
    v[1] += px; v[2] += py; v[3] += pz;
    v[4] += qx; v[5] += qy; v[6] += qz;
    v[7] += px * qx; v[8] += px * qy; v[9] += px * qz;
    v[10] += py * qx; v[11] += py * qy; v[12] += py * qz;
    v[13] += pz * qx; v[14] += pz * qy; v[15] += pz * qz;
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    v[16] += dx * dx + dy * dy + dz * dz;
  }
  block_slab<17>(v, slab);
}

// sum x, count (x < thresh)
__global__ __launch_bounds__(256) void sum_count_kernel(const float* __restrict__ x, int64_t n, float thresh, double* __restrict__ slab) {
  double v[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = x[i];
    v[0] += (double)a;
    v[1] += a < thresh ? 1.0 : 0.0;
  }
  block_slab<2>(v, slab);
}

// out_i = | na[ia] . nb[ib] |, (ia, ib) = (idx_i, i) if gather_a else (i, idx_i)
__global__ __launch_bounds__(256) void normal_dot_kernel(const float* __restrict__ na, const float* __restrict__ nb, const int* __restrict__ idx,
                                                         int64_t n, int gather_a, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t j = idx[i];
  if (j < 0) { out[i] = 0.f; return; }
  const int64_t ia = gather_a ? j : i, ib = gather_a ? i : j;
  out[i] = fabsf((float)((double)na[3 * ia] * nb[3 * ib] + (double)na[3 * ia + 1] * nb[3 * ib + 1] + (double)na[3 * ia + 2] * nb[3 * ib + 2]));
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// the brute-force stage over `slots` queries (list / count nullable: every query)
int launch_brute(const float* q, const int* list, const int* count, int64_t nq, const float4* recs, int64_t m, float max_dist,
                 unsigned long long* key, float* dist, int* idx, hipStream_t st) {
  const Slots slots = {list, count, nq};
  const BruteLaunch l = size_brute(nq, m, 8192, BRUTE_TILE);
  nn_brute_kernel<<<dim3(l.qblocks, l.chunks), 256, 0, st>>>(q, slots, recs, m, l.chunk, key);
  nn_brute_finish_kernel<<<l.qblocks, 256, 0, st>>>(slots, key, max_dist, dist, idx);
  return 0;
}

}  // namespace

extern "C" {

int sp3_nn_cell_ids(const float* pts, int64_t n, const sp3_nn_grid* g, int* ids, void* stream) {
  SP3_CHECK(pts && ids && n >= 1 && n <= N_MAX, "sp3_nn_cell_ids: null pointer or n = %lld out of range", (long long)n);
  if (check_grid(g, "sp3_nn_cell_ids")) return 1;
  cell_ids_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(pts, n, *g, ids);
  SP3_LAUNCH_CHECK("sp3_nn_cell_ids");
  return 0;
}

int sp3_nn_pack_records(const float* pts, const int64_t* order, int64_t n, float* recs, void* stream) {
  SP3_CHECK(pts && recs && n >= 1 && n <= N_MAX, "sp3_nn_pack_records: null pointer or n = %lld out of range", (long long)n);
  SP3_CHECK(((uintptr_t)recs & 15) == 0, "sp3_nn_pack_records: records must be 16-byte aligned");
  pack_records_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(pts, order, n, (float4*)recs);
  SP3_LAUNCH_CHECK("sp3_nn_pack_records");
  return 0;
}

int64_t sp3_nn_query_ws_bytes(int64_t nq) { return nq < 0 ? 0 : 32 + nq * 8 + (nq + 3) / 4 * 16; }

int sp3_nn_query(const float* q, const int64_t* q_order, int64_t nq, const float* recs, const int* cell_start, int64_t m,
                 const sp3_nn_grid* g, int max_ring, float max_dist, void* ws, float* dist, int* idx, void* stream) {
  SP3_CHECK(q && recs && cell_start && ws && dist && idx, "sp3_nn_query: null pointer");
  SP3_CHECK(nq >= 1 && nq <= N_MAX && m >= 1 && m <= N_MAX, "sp3_nn_query: nq = %lld, m = %lld out of range", (long long)nq, (long long)m);
  SP3_CHECK(max_ring >= 0 && max_dist >= 0.f, "sp3_nn_query: max_ring / max_dist must be non-negative");
  SP3_CHECK((((uintptr_t)recs | (uintptr_t)ws) & 15) == 0, "sp3_nn_query: records and workspace must be 16-byte aligned");
  if (check_grid(g, "sp3_nn_query")) return 1;
  hipStream_t st = (hipStream_t)stream;
  GridHead* head = (GridHead*)ws;
  unsigned long long* key = (unsigned long long*)((char*)ws + 32);
  int* list = (int*)((char*)ws + 32 + nq * 8);
  if (hipMemsetAsync(ws, 0, 32, st) != hipSuccess) { sp3_set_error("sp3_nn_query: hipMemsetAsync failed"); return 2; }
  nn_grid_kernel<<<blocks256(nq), 256, 0, st>>>(q, q_order, nq, (const float4*)recs, cell_start, *g, max_ring, max_dist, dist, idx, head, key, list);
  launch_brute(q, list, &head->fb_count, nq, (const float4*)recs, m, max_dist, key, dist, idx, st);
  SP3_LAUNCH_CHECK("sp3_nn_query");
  return 0;
}

int sp3_nn_brute(const float* q, int64_t nq, const float* recs, int64_t m, float max_dist, void* ws, float* dist, int* idx, void* stream) {
  SP3_CHECK(q && recs && ws && dist && idx, "sp3_nn_brute: null pointer");
  SP3_CHECK(nq >= 1 && nq <= N_MAX && m >= 1 && m <= N_MAX, "sp3_nn_brute: nq = %lld, m = %lld out of range", (long long)nq, (long long)m);
  SP3_CHECK(max_dist >= 0.f, "sp3_nn_brute: max_dist must be non-negative");
  SP3_CHECK((((uintptr_t)recs | (uintptr_t)ws) & 15) == 0, "sp3_nn_brute: records and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* key = (unsigned long long*)((char*)ws + 32);
  fill_u64_kernel<<<blocks256(nq), 256, 0, st>>>(key, nq);
  launch_brute(q, nullptr, nullptr, nq, (const float4*)recs, m, max_dist, key, dist, idx, st);
  SP3_LAUNCH_CHECK("sp3_nn_brute");
  return 0;
}

int sp3_knn_query(const float* q, const int64_t* q_order, int64_t nq, const float* recs, const int* cell_start, int64_t m,
                  const sp3_nn_grid* g, int k, float max_dist, float* dist, int* idx, void* stream) {
  SP3_CHECK(q && recs && cell_start && dist && idx, "sp3_knn_query: null pointer");
  SP3_CHECK(nq >= 1 && nq <= N_MAX && m >= 1 && m <= N_MAX && nq * (int64_t)k <= N_MAX * 16, "sp3_knn_query: nq = %lld, m = %lld out of range",
            (long long)nq, (long long)m);
  SP3_CHECK(k >= 1 && k <= KNN_MAX, "sp3_knn_query: k = %d, must be 1..%d", k, KNN_MAX);
  SP3_CHECK(max_dist >= 0.f, "sp3_knn_query: max_dist must be non-negative");
  SP3_CHECK(((uintptr_t)recs & 15) == 0, "sp3_knn_query: records must be 16-byte aligned");
  if (check_grid(g, "sp3_knn_query")) return 1;
  knn_grid_kernel<<<(unsigned)((nq + KNN_BLOCK - 1) / KNN_BLOCK), KNN_BLOCK, 0, (hipStream_t)stream>>>(q, q_order, nq, (const float4*)recs, cell_start, *g,
                                                                                                    k, max_dist, dist, idx);
  SP3_LAUNCH_CHECK("sp3_knn_query");
  return 0;
}

int sp3_knn_normals(const float* pts, const int* nbr, int64_t n, int k, float* normals, void* stream) {
  SP3_CHECK(pts && nbr && normals && n >= 1 && n <= N_MAX, "sp3_knn_normals: null pointer or n = %lld out of range", (long long)n);
  SP3_CHECK(k >= 1 && k <= KNN_MAX, "sp3_knn_normals: k = %d, must be 1..%d", k, KNN_MAX);
  knn_normals_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(pts, nbr, n, k, normals);
  SP3_LAUNCH_CHECK("sp3_knn_normals");
  return 0;
}

int sp3_transform_points(const float* src, int64_t n, const double* Rt12, float* out, void* stream) {
  SP3_CHECK(src && Rt12 && out && n >= 1 && n <= N_MAX, "sp3_transform_points: null pointer or n = %lld out of range", (long long)n);
  Rigid T;
  for (int i = 0; i < 12; ++i) T.m[i] = Rt12[i];
  transform_points_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(src, n, T, out);
  SP3_LAUNCH_CHECK("sp3_transform_points");
  return 0;
}

int64_t sp3_icp_accum_ws_bytes(int64_t n) { return (int64_t)slab_blocks(n) * 17 * 8; }

int sp3_icp_accum(const float* p, const float* tgt, const int* idx, int64_t n, void* ws, double* out17, void* stream) {
  SP3_CHECK(p && tgt && idx && ws && out17 && n >= 1 && n <= N_MAX, "sp3_icp_accum: null pointer or n = %lld out of range", (long long)n);
  const int nb = slab_blocks(n);
  icp_accum_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(p, tgt, idx, n, (double*)ws);
  slab_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)ws, nb, 17, out17);
  SP3_LAUNCH_CHECK("sp3_icp_accum");
  return 0;
}

int64_t sp3_sum_count_ws_bytes(int64_t n) { return (int64_t)slab_blocks(n) * 2 * 8; }

int sp3_sum_count_f32(const float* x, int64_t n, float thresh, void* ws, double* out2, void* stream) {
  SP3_CHECK(x && ws && out2 && n >= 1, "sp3_sum_count_f32: null pointer or n = %lld out of range", (long long)n);
  const int nb = slab_blocks(n);
  sum_count_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(x, n, thresh, (double*)ws);
  slab_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)ws, nb, 2, out2);
  SP3_LAUNCH_CHECK("sp3_sum_count_f32");
  return 0;
}

int sp3_normal_dot(const float* na, const float* nb, const int* idx, int64_t n, int gather_a, float* out, void* stream) {
  SP3_CHECK(na && nb && idx && out && n >= 1 && n <= N_MAX, "sp3_normal_dot: null pointer or n = %lld out of range", (long long)n);
  normal_dot_kernel<<<blocks256(n), 256, 0, (hipStream_t)stream>>>(na, nb, idx, n, gather_a, out);
  SP3_LAUNCH_CHECK("sp3_normal_dot");
  return 0;
}

}  // extern "C"
