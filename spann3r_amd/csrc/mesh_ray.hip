// Ray queries on a triangle mesh (include/spann3r_hip.h "Mesh rays"; spann3r_amd/mesh.py ray_mesh_intersect / render_depth_maps and
// spann3r_amd/evaluate.py evaluate_depth drive these; tests/mesh_ray_ref.py restates the rule).
//
//   * The rule of one (ray, face) pair is Woop, Benthin and Wald's watertight test in fp64, every operation rounded on its own
//     (csrc/tri_ray.h states it once, for this file and csrc/mesh_bvh.hip; the file-level pragma below covers the rest) and in the
//     order the header fixes.  The result of a ray is the lexicographic minimum of (t, face index)
//     over the hits: a pure function of the inputs, so a face may be evaluated in any order, any number of times, by any kernel.
//   * The grid of face references is mesh.TriangleGrid's as it is (csrc/mesh_distance.hip registers the faces).  A ray is clipped
//     against the grid's box pushed out by the slack and walks the cells it crosses one by one; the exit parameter of a cell is
//     recomputed from the integer cell index at every step (wall = fmaf(i, h, origin), as ring_bound computes it), so nothing drifts.
//     The walk ends when the best t lies before the exit of the current cell less a margin, when it leaves the grid or passes t_max:
//     at most nx + ny + nz cells, so there is no fallback list.  The header says why no hit is missed.
//   * The hot loops keep (t, face) only; bary, point and side of the winner are recomputed once at the end.
//   * The brute-force kernel stages faces through LDS in tiles, the face list split over workgroups, and joins by the two order-free
//     passes of csrc/mesh_distance.hip: an integer atomicMin over the bits of the non-negative t, then an atomicMin of the face index
//     among the faces with exactly that t.
//   * sp3_mesh_ray_views makes its rays from a read-only table of cameras (a wave owns an 8 x 8 pixel tile of one view, blockIdx.z:
//     the descriptor arrives by scalar loads) and runs the same walk.
//   * Every loop is bounded by the grid dims, npairs or nfaces; nothing waits on another lane's store; what an atomic wrote is read
//     by a LATER launch only.
#include "cell_grid.h"
#include "tri_ray.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int TB = 256;
constexpr int TILE = 512;                      // faces per LDS tile of the brute-force kernel: 512 * 40 bytes
constexpr int VIEW_TILE = 16;                  // a workgroup of sp3_mesh_ray_views: 16 x 16 pixels, four 8 x 8 wave tiles

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TB - 1) / TB); }

// ------------------------------------------------------------------------------------------------ the walk
struct MeshRef {
  const float* __restrict__ verts;
  const int* __restrict__ faces;
  const int* __restrict__ pair_face;
  const int* __restrict__ cell_start;
  int nverts, nfaces, npairs;
};

// The winning face (-1: none) of the ray (o, d) in [t_min, t_max] by the walk of the header; cells / evals count what it did.
__device__ __forceinline__ int walk_ray(const sp3_nn_grid& g, const MeshRef& m, const Ray& r, float ox, float oy, float oz, float dx, float dy,
                                        float dz, double t_min, double t_max, int cull, int& cells, int& evals) {
  const double o[3] = {(double)ox, (double)oy, (double)oz}, d[3] = {(double)dx, (double)dy, (double)dz};
  const float org[3] = {g.ox, g.oy, g.oz};
  const int n[3] = {g.nx, g.ny, g.nz};
  const double slack = (double)g.slack;
  // the slab test against the box [origin - slack, wall(n) + slack] (clip_box, csrc/tri_ray.h)
  double lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { lo[k] = (double)org[k] - slack; hi[k] = (double)fmaf((float)n[k], g.h, org[k]) + slack; }
  double t0 = t_min, t1 = t_max;
  if (!clip_box(o, d, lo, hi, t0, t1)) return -1;
  // the entry cell, clamped into the grid by the cell rule itself
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double m0 = t0 * d[k];
    c[k] = cell_axis((float)(o[k] + m0), org[k], g.inv_h, n[k]);
  }
  const double margin = 2.0 * slack * fabs(r.Sz);      // two slacks of travel along the ray's largest axis, in ray parameter
  double best = INFINITY;
  int bf = -1;
  const int max_steps = g.nx + g.ny + g.nz;
  for (int step = 0; step < max_steps; ++step) {
    const int id = cell_id(g, c[0], c[1], c[2]);
    const int s = max(m.cell_start[id], 0), e = min(m.cell_start[id + 1], m.npairs);
    ++cells;
    for (int j = s; j < e; ++j) {
      const int f = m.pair_face[j];
      float v[9];
      if (!((unsigned)f < (unsigned)m.nfaces && load_face(m.verts, m.nverts, m.faces, f, v))) continue;      // (the pairs hold usable faces only)
      ++evals;
      Hit h;
      if (intersect(r, v, t_min, t_max, cull, h) && (h.t < best || (h.t == best && f < bf))) { best = h.t; bf = f; }
    }
    // the exit of this cell per axis, from the integer index; a cell on the rim of the grid reaches to the box's own exit
    double te = INFINITY;
    int ax = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (d[k] == 0.0) continue;
      const int iw = d[k] > 0.0 ? c[k] + 1 : c[k];
      if (iw <= 0 || iw >= n[k]) continue;
      const double tk = ((double)fmaf((float)iw, g.h, org[k]) - o[k]) / d[k];
      if (tk < te) { te = tk; ax = k; }
    }
    if (ax < 0 || !(te < t1)) break;      // the ray leaves the grid, or passes t_max, inside this cell
    if (best <= te - margin) break;       // everything unvisited lies at a larger t
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k == ax) c[k] += d[k] > 0.0 ? 1 : -1;
  }
  return bf;
}

// every face against the ray, for a grid of one cell (no references): usability decided here
__device__ __forceinline__ int scan_all(const MeshRef& m, const Ray& r, double t_min, double t_max, int cull, int& evals) {
  double best = INFINITY;
  int bf = -1;
  for (int f = 0; f < m.nfaces; ++f) {
    float v[9];
    if (!(load_face(m.verts, m.nverts, m.faces, f, v) && has_area(v))) continue;
    ++evals;
    Hit h;
    if (intersect(r, v, t_min, t_max, cull, h) && h.t < best) { best = h.t; bf = f; }      // ascending f: the smallest index among equals
  }
  return bf;
}

// ---- one lane per ray (rays sorted by the cell of their origin: the lanes of a wave start in the same cells)
__global__ __launch_bounds__(TB) void k_mr_grid(const float* __restrict__ org, const float* __restrict__ dir, const int64_t* __restrict__ order,
                                                 int64_t nq, MeshRef m, sp3_nn_grid g, double t_min, double t_max, int cull, RayOut out,
                                                 GridHead* head) {
  const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
  int cells = 0, evals = 0;
  if (t < nq) {
    const int64_t qi = order ? order[t] : t;
    const float ox = org[3 * qi], oy = org[3 * qi + 1], oz = org[3 * qi + 2], dx = dir[3 * qi], dy = dir[3 * qi + 1], dz = dir[3 * qi + 2];
    const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
    const int bf = r.ok ? walk_ray(g, m, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, cells, evals) : -1;
    store(out, qi, result_of(m.verts, m.nverts, m.faces, m.nfaces, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, bf));
  }
  head->count(cells, evals);
}

// ---- brute force: a workgroup holds 256 rays in registers and streams its chunk of the faces through LDS.
// PASS 0: key[slot] = min over the hits of the bits of t.  PASS 1: fkey[slot] = min face index with t == key[slot].
template <int PASS>
__global__ __launch_bounds__(TB) void k_mr_brute(const float* __restrict__ org, const float* __restrict__ dir, Slots slots,
                                                  const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t nfaces,
                                                  int64_t chunk, double t_min, double t_max, int cull, u64* key, int* fkey) {
  __shared__ float tv[TILE * 9];
  __shared__ int tf[TILE];      // the face index, -1 for a face that is not usable
  const int64_t nq = slots.size();
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(r0 + chunk, nfaces);
  for (int64_t qb = (int64_t)blockIdx.x * TB; qb < nq; qb += (int64_t)gridDim.x * TB) {
    const int64_t slot = qb + threadIdx.x;
    const int64_t qi = slot < nq ? slots.query(slot) : -1;
    Ray r = make_ray(0.f, 0.f, 0.f, 0.f, 0.f, 1.f);
    if (qi >= 0) r = make_ray(org[3 * qi], org[3 * qi + 1], org[3 * qi + 2], dir[3 * qi], dir[3 * qi + 1], dir[3 * qi + 2]);
    const bool active = qi >= 0 && r.ok;
    const double target = (PASS == 1 && active) ? __longlong_as_double((long long)key[slot]) : 0.0;      // NaN (all ones): nothing equals it
    double best = INFINITY;
    int bf = NO_FACE;
    for (int64_t t0 = r0; t0 < r1; t0 += TILE) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < TILE / TB; ++k) {
        const int i = threadIdx.x + k * TB;
        const int64_t f = t0 + i;
        if (f < r1) {
          float v[9];
          const bool ok = load_face(verts, nverts, faces, f, v) && has_area(v);
          tf[i] = ok ? (int)f : -1;
          if (ok) {
#pragma unroll
            for (int c = 0; c < 9; ++c) tv[i * 9 + c] = v[c];
          }
        }
      }
      __syncthreads();
      const int cnt = (int)min((int64_t)TILE, r1 - t0);
      for (int j = 0; j < cnt; ++j) {
        const int f = tf[j];      // the same address in every lane: an LDS broadcast, and a uniform branch
        if (f < 0) continue;
        Hit h;
        if (!intersect(r, tv + j * 9, t_min, t_max, cull, h)) continue;
        if (PASS == 0) {
          if (h.t < best) best = h.t;
        } else {
          if (h.t == target && f < bf) bf = f;
        }
      }
    }
    if (active && r0 < r1) {
      if (PASS == 0) {
        if (best < INFINITY) atomicMin(&key[slot], (u64)__double_as_longlong(best));      // t >= +0: bit order = value order
      } else {
        if (bf != NO_FACE) atomicMin(&fkey[slot], bf);
      }
    }
  }
}

__global__ __launch_bounds__(TB) void k_mr_fill_keys(u64* __restrict__ key, int* __restrict__ fkey, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n) { key[i] = ~0ull; fkey[i] = NO_FACE; }
}

__global__ __launch_bounds__(TB) void k_mr_brute_finish(const float* __restrict__ org, const float* __restrict__ dir, int64_t nq,
                                                         const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces,
                                                         double t_min, double t_max, int cull, const int* __restrict__ fkey, RayOut out) {
  for (int64_t qi = (int64_t)blockIdx.x * TB + threadIdx.x; qi < nq; qi += (int64_t)gridDim.x * TB) {
    const float ox = org[3 * qi], oy = org[3 * qi + 1], oz = org[3 * qi + 2], dx = dir[3 * qi], dy = dir[3 * qi + 1], dz = dir[3 * qi + 2];
    const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
    store(out, qi, result_of(verts, nverts, faces, nfaces, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, fkey[qi]));
  }
}

// ---- T cameras in one launch: a lane owns a pixel, a wave an 8 x 8 tile, a workgroup 16 x 16 pixels of view blockIdx.z
__global__ __launch_bounds__(VIEW_TILE * VIEW_TILE) void k_mr_views(const sp3_mesh_ray_view* __restrict__ views, float pixel_offset, MeshRef m,
                                                                    sp3_nn_grid g, GridHead* head) {
  const sp3_mesh_ray_view& vw = views[blockIdx.z];      // (wave-uniform: the descriptor fields arrive by scalar loads)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * VIEW_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * VIEW_TILE + (wave >> 1) * 8 + (lane >> 3);
  int cells = 0, evals = 0;
  if (px < vw.w && py < vw.h) {
    float oo[3], dd[3];
    pixel_ray(vw, px, py, pixel_offset, oo, dd);
    const float ox = oo[0], oy = oo[1], oz = oo[2];
    const double t_min = (double)vw.near, t_max = (double)vw.far;
    const Ray r = make_ray(ox, oy, oz, dd[0], dd[1], dd[2]);
    int bf = -1;
    if (r.ok) bf = m.npairs > 0 ? walk_ray(g, m, r, ox, oy, oz, dd[0], dd[1], dd[2], t_min, t_max, CULL_NONE, cells, evals)
                                : scan_all(m, r, t_min, t_max, CULL_NONE, evals);
    const Result o = result_of(m.verts, m.nverts, m.faces, m.nfaces, r, ox, oy, oz, dd[0], dd[1], dd[2], t_min, t_max, CULL_NONE, bf);
    store_pixel(vw, px, py, o);
  }
  head->count(cells, evals);
}

inline bool sizes_ok(int64_t nverts, int64_t nfaces) { return nverts >= 0 && nverts < N_MAX && nfaces >= 1 && nfaces < N_MAX; }
inline bool range_ok(double t_min, double t_max) { return t_min >= 0.0 && t_min <= t_max; }      // (false for a NaN)
inline int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

int check_mesh_args(const char* what, int64_t nverts, int64_t nfaces, int64_t nq, double t_min, double t_max, int cull) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "%s: nverts %lld or nfaces %lld out of range (1 face at least; both below 2^31 - 1)", what, (long long)nverts,
            (long long)nfaces);
  SP3_CHECK(nq >= 0 && nq <= N_MAX, "%s: nq = %lld out of range", what, (long long)nq);
  SP3_CHECK(range_ok(t_min, t_max), "%s: 0 <= t_min <= t_max, got %g and %g", what, t_min, t_max);
  SP3_CHECK(cull >= CULL_NONE && cull <= CULL_FRONT, "%s: cull %d must be 0 (none), 1 (back) or 2 (front)", what, cull);
  return 0;
}

}  // namespace

extern "C" int64_t sp3_mesh_ray_ws_bytes(int64_t nq) { return nq < 0 || nq > N_MAX ? 0 : 32 + round4(nq) * 12; }

extern "C" int sp3_mesh_ray_query(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                                  int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                                  const int32_t* cell_start, const sp3_nn_grid* g, double t_min, double t_max, int cull, void* ws, float* t,
                                  int32_t* face, float* bary, float* point, uint8_t* side, void* stream) {
  if (check_mesh_args("sp3_mesh_ray_query", nverts, nfaces, nq, t_min, t_max, cull)) return 1;
  SP3_CHECK(npairs >= 1 && npairs < N_MAX, "sp3_mesh_ray_query: npairs = %lld out of range (a grid of one cell holds none: sp3_mesh_ray_brute)",
            (long long)npairs);
  if (check_grid(g, "sp3_mesh_ray_query")) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(origins && directions && faces && pair_face && cell_start && ws && t && face && bary && point && side && (nverts == 0 || vertices),
            "sp3_mesh_ray_query: null pointer");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_ray_query: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, 32, st) != hipSuccess) { sp3_set_error("sp3_mesh_ray_query: hipMemsetAsync failed"); return 2; }
  const MeshRef m = {vertices, (const int*)faces, (const int*)pair_face, (const int*)cell_start, (int)nverts, (int)nfaces, (int)npairs};
  const RayOut out = {t, (int*)face, bary, point, side};
  k_mr_grid<<<blocks_for(nq), TB, 0, st>>>(origins, directions, q_order, nq, m, *g, t_min, t_max, cull, out, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_query");
  return 0;
}

extern "C" int sp3_mesh_ray_brute(const float* origins, const float* directions, int64_t nq, const float* vertices, int64_t nverts,
                                  const int32_t* faces, int64_t nfaces, double t_min, double t_max, int cull, void* ws, float* t, int32_t* face,
                                  float* bary, float* point, uint8_t* side, void* stream) {
  if (check_mesh_args("sp3_mesh_ray_brute", nverts, nfaces, nq, t_min, t_max, cull)) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(origins && directions && faces && ws && t && face && bary && point && side && (nverts == 0 || vertices),
            "sp3_mesh_ray_brute: null pointer");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_ray_brute: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, 32, st) != hipSuccess) { sp3_set_error("sp3_mesh_ray_brute: hipMemsetAsync failed"); return 2; }
  u64* key = (u64*)((char*)ws + 32);
  int* fkey = (int*)((char*)ws + 32 + round4(nq) * 8);
  const Slots slots = {nullptr, nullptr, nq};
  const BruteLaunch l = size_brute(nq, nfaces, 4096, TILE);
  const dim3 grid(l.qblocks, l.chunks);
  const RayOut out = {t, (int*)face, bary, point, side};
  k_mr_fill_keys<<<blocks_for(nq), TB, 0, st>>>(key, fkey, nq);
  k_mr_brute<0><<<grid, TB, 0, st>>>(origins, directions, slots, vertices, (int)nverts, (const int*)faces, nfaces, l.chunk, t_min, t_max, cull, key, fkey);
  k_mr_brute<1><<<grid, TB, 0, st>>>(origins, directions, slots, vertices, (int)nverts, (const int*)faces, nfaces, l.chunk, t_min, t_max, cull, key, fkey);
  k_mr_brute_finish<<<l.qblocks, TB, 0, st>>>(origins, directions, nq, vertices, (int)nverts, (const int*)faces, (int)nfaces, t_min, t_max, cull,
                                              fkey, out);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_brute");
  return 0;
}

extern "C" int sp3_mesh_ray_views(const sp3_mesh_ray_view* views_host, const sp3_mesh_ray_view* views_dev, int T, float pixel_offset,
                                  const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face,
                                  int64_t npairs, const int32_t* cell_start, const sp3_nn_grid* g, void* ws, void* stream) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "sp3_mesh_ray_views: nverts %lld or nfaces %lld out of range (1 face at least; both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  SP3_CHECK(npairs >= 0 && npairs < N_MAX, "sp3_mesh_ray_views: npairs = %lld out of range", (long long)npairs);
  SP3_CHECK(T >= 0 && T <= 65535, "sp3_mesh_ray_views: T %d must be in 0 .. 65535", T);
  SP3_CHECK(isfinite(pixel_offset), "sp3_mesh_ray_views: pixel_offset is not finite");
  if (check_grid(g, "sp3_mesh_ray_views")) return 1;
  if (T == 0) return 0;
  SP3_CHECK(views_host && views_dev && faces && ws && (nverts == 0 || vertices) && (npairs == 0 || (pair_face && cell_start)),
            "sp3_mesh_ray_views: null pointer");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_ray_views: the workspace must be 16-byte aligned");
  int wmax = 0, hmax = 0;
  for (int i = 0; i < T; ++i) {
    const sp3_mesh_ray_view& v = views_host[i];
    SP3_CHECK(v.w >= 1 && v.h >= 1 && v.w <= (1 << 24) && v.h <= (1 << 24) && v.row_stride >= v.w && (int64_t)v.h * v.row_stride < N_MAX / 3,
              "sp3_mesh_ray_views: view %d: bad geometry: %d x %d, row stride %lld", i, v.w, v.h, (long long)v.row_stride);
    SP3_CHECK(v.depth != nullptr, "sp3_mesh_ray_views: view %d: null depth map", i);
    SP3_CHECK(isfinite(v.fu) && isfinite(v.fv) && isfinite(v.cu) && isfinite(v.cv) && v.fu != 0.f && v.fv != 0.f,
              "sp3_mesh_ray_views: view %d: intrinsics must be finite with non-zero focal lengths", i);
    SP3_CHECK(range_ok((double)v.near, (double)v.far), "sp3_mesh_ray_views: view %d: 0 <= near <= far, got %g and %g", i, (double)v.near,
              (double)v.far);
    wmax = v.w > wmax ? v.w : wmax;
    hmax = v.h > hmax ? v.h : hmax;
  }
  const dim3 grid((wmax + VIEW_TILE - 1) / VIEW_TILE, (hmax + VIEW_TILE - 1) / VIEW_TILE, T);
  SP3_CHECK(grid.y <= 65535, "sp3_mesh_ray_views: %d rows of pixels are more than one launch covers", hmax);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, 32, st) != hipSuccess) { sp3_set_error("sp3_mesh_ray_views: hipMemsetAsync failed"); return 2; }
  const MeshRef m = {vertices, (const int*)faces, (const int*)pair_face, (const int*)cell_start, (int)nverts, (int)nfaces, (int)npairs};
  k_mr_views<<<grid, VIEW_TILE * VIEW_TILE, 0, st>>>(views_dev, pixel_offset, m, *g, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_views");
  return 0;
}
