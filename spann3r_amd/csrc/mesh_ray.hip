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
//   * Brute force is the face sweep of csrc/face_sweep.h (LDS tiles, the two order-free passes, the workspace carving) with the rule
//     "key = t of the hit, a missed face does not count"; the finish kernel here turns the winning face into the five outputs.
//   * The kernels that serve rays are the two front ends of csrc/ray_kernels.h -- one lane per given ray, and one lane per pixel of a
//     read-only table of cameras (sp3_mesh_ray_views) -- instantiated with the walk of this file; csrc/mesh_bvh.hip instantiates
//     them with the tree's.  The host checks of the ray entry points and of the table of views are that header's too; the size
//     checks and the workspace head (begin_query) are csrc/cell_grid.h's.
//   * "Mesh visibility" (sp3_mesh_ray_occluded, sp3_mesh_point_views) asks the same walk whether ANY face is a hit: walk_ray<true> and
//     scan_all<true> return at the first accepted one; the <false> instantiations are the code they were.  Their front ends are
//     csrc/ray_kernels.h's too.
//   * Every loop is bounded by the grid dims, npairs or nfaces; nothing waits on another lane's store; what an atomic wrote is read
//     by a LATER launch only.
#include "face_sweep.h"
#include "ray_kernels.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ the walk
struct MeshRef {
  const float* __restrict__ verts;
  const int* __restrict__ faces;
  const int* __restrict__ pair_face;
  const int* __restrict__ cell_start;
  int nverts, nfaces, npairs;
};

// The winning face (-1: none) of the ray (o, d) in [t_min, t_max] by the walk of the header; cells / evals count what it did.
// ANY ("Mesh visibility"): the first accepted hit ends the walk and is returned, whichever it is.
template <bool ANY>
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
      if (ANY) {
        if (intersect(r, v, t_min, t_max, cull, h)) return f;
      } else if (intersect(r, v, t_min, t_max, cull, h) && (h.t < best || (h.t == best && f < bf))) { best = h.t; bf = f; }
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
template <bool ANY>
__device__ __forceinline__ int scan_all(const MeshRef& m, const Ray& r, double t_min, double t_max, int cull, int& evals) {
  double best = INFINITY;
  int bf = -1;
  for (int f = 0; f < m.nfaces; ++f) {
    float v[9];
    if (!(load_face(m.verts, m.nverts, m.faces, f, v) && has_area(v))) continue;
    ++evals;
    Hit h;
    if (ANY) {
      if (intersect(r, v, t_min, t_max, cull, h)) return f;
    } else if (intersect(r, v, t_min, t_max, cull, h) && h.t < best) { best = h.t; bf = f; }      // ascending f: the smallest index among equals
  }
  return bf;
}

// ---- the Walker of csrc/ray_kernels.h: the cells along the ray.  VIEWS: a grid of one cell holds no references (sp3_mesh_ray_views
// takes one; sp3_mesh_ray_query refuses it) and every face is scanned instead.  Nothing to prepare, no LDS.
template <bool VIEWS>
struct GridWalker {
  MeshRef m;
  sp3_nn_grid g;
  __device__ __forceinline__ void prepare(unsigned*) {}
  template <bool ANY = false>
  __device__ __forceinline__ int walk(const Ray& r, float ox, float oy, float oz, float dx, float dy, float dz, double t_min, double t_max, int cull,
                                      int& cells, int& evals) const {
    if (VIEWS && m.npairs <= 0) return scan_all<ANY>(m, r, t_min, t_max, cull, evals);
    return walk_ray<ANY>(g, m, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, cells, evals);
  }
};

// ---- brute force (csrc/face_sweep.h): the key of a face is the t of its hit, and a face the ray misses does not count
struct RayRule {
  const float* __restrict__ org;
  const float* __restrict__ dir;
  double t_min, t_max;
  int cull;
  Ray r;
  __device__ __forceinline__ bool load(int64_t qi) {
    r = make_ray(0.f, 0.f, 0.f, 0.f, 0.f, 1.f);
    if (qi >= 0) r = make_ray(org[3 * qi], org[3 * qi + 1], org[3 * qi + 2], dir[3 * qi], dir[3 * qi + 1], dir[3 * qi + 2]);
    return qi >= 0 && r.ok;
  }
  template <typename Take>
  __device__ __forceinline__ void eval(const float* v, Take take) const {
    Hit h;
    if (intersect(r, v, t_min, t_max, cull, h)) take(h.t);
  }
};

__global__ __launch_bounds__(TB) void k_mr_brute_finish(const float* __restrict__ org, const float* __restrict__ dir, int64_t nq,
                                                         const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces,
                                                         double t_min, double t_max, int cull, const int* __restrict__ fkey, RayOut out) {
  for (int64_t qi = (int64_t)blockIdx.x * TB + threadIdx.x; qi < nq; qi += (int64_t)gridDim.x * TB) {
    const float ox = org[3 * qi], oy = org[3 * qi + 1], oz = org[3 * qi + 2], dx = dir[3 * qi], dy = dir[3 * qi + 1], dz = dir[3 * qi + 2];
    const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
    store(out, qi, result_of(verts, nverts, faces, nfaces, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, fkey[qi]));
  }
}

inline MeshRef mesh_ref(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                        const int32_t* cell_start) {
  return {vertices, (const int*)faces, (const int*)pair_face, (const int*)cell_start, (int)nverts, (int)nfaces, (int)npairs};
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
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_ray_query")) return e;
  const GridWalker<false> w = {mesh_ref(vertices, nverts, faces, nfaces, pair_face, npairs, cell_start), *g};
  const RayOut out = {t, (int*)face, bary, point, side};
  k_ray_query<<<blocks_for(nq), TB, 0, st>>>(origins, directions, q_order, nq, w, t_min, t_max, cull, out, (GridHead*)ws);
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
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_ray_brute")) return e;
  const SweepWs w = carve(ws, nq);      // (key and fkey; no fallback list)
  const RayOut out = {t, (int*)face, bary, point, side};
  k_fill_keys<<<blocks_for(nq), TB, 0, st>>>(w.key, w.fkey, nq);
  const RayRule rule = {origins, directions, t_min, t_max, cull};
  const BruteLaunch l = sweep_faces(rule, Slots{nullptr, nullptr, nq}, vertices, (int)nverts, (const int*)faces, nfaces, w, st);
  k_mr_brute_finish<<<l.qblocks, TB, 0, st>>>(origins, directions, nq, vertices, (int)nverts, (const int*)faces, (int)nfaces, t_min, t_max, cull,
                                              w.fkey, out);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_brute");
  return 0;
}

extern "C" int sp3_mesh_ray_views(const sp3_mesh_ray_view* views_host, const sp3_mesh_ray_view* views_dev, int T, float pixel_offset,
                                  const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face,
                                  int64_t npairs, const int32_t* cell_start, const sp3_nn_grid* g, void* ws, void* stream) {
  if (check_mesh_sizes("sp3_mesh_ray_views", nverts, nfaces)) return 1;
  SP3_CHECK(npairs >= 0 && npairs < N_MAX, "sp3_mesh_ray_views: npairs = %lld out of range", (long long)npairs);
  if (check_view_args("sp3_mesh_ray_views", T, pixel_offset) || check_grid(g, "sp3_mesh_ray_views")) return 1;
  if (T == 0) return 0;
  SP3_CHECK(views_host && views_dev && faces && ws && (nverts == 0 || vertices) && (npairs == 0 || (pair_face && cell_start)),
            "sp3_mesh_ray_views: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_ray_views")) return e;
  dim3 grid;
  if (check_views("sp3_mesh_ray_views", views_host, T, grid)) return 1;
  const GridWalker<true> w = {mesh_ref(vertices, nverts, faces, nfaces, pair_face, npairs, cell_start), *g};
  k_ray_views<<<grid, TB, 0, st>>>(views_dev, pixel_offset, w, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_views");
  return 0;
}

// ---- "Mesh visibility" over the grid
extern "C" int sp3_mesh_ray_occluded(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                                     int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                                     const int32_t* cell_start, const sp3_nn_grid* g, double t_min, double t_max, int cull, void* ws,
                                     uint8_t* occluded, void* stream) {
  if (check_mesh_args("sp3_mesh_ray_occluded", nverts, nfaces, nq, t_min, t_max, cull)) return 1;
  SP3_CHECK(npairs >= 1 && npairs < N_MAX, "sp3_mesh_ray_occluded: npairs = %lld out of range (a grid of one cell holds none: sp3_mesh_ray_brute)",
            (long long)npairs);
  if (check_grid(g, "sp3_mesh_ray_occluded")) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(origins && directions && faces && pair_face && cell_start && ws && occluded && (nverts == 0 || vertices),
            "sp3_mesh_ray_occluded: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_ray_occluded")) return e;
  const GridWalker<false> w = {mesh_ref(vertices, nverts, faces, nfaces, pair_face, npairs, cell_start), *g};
  k_ray_occluded<<<blocks_for(nq), TB, 0, st>>>(origins, directions, q_order, nq, w, t_min, t_max, cull, occluded, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_ray_occluded");
  return 0;
}

extern "C" int sp3_mesh_point_views(const sp3_mesh_vis_view* views_host, const sp3_mesh_vis_view* views_dev, int T, float pixel_offset,
                                    float bias, int cull, const float* points, const int64_t* q_order, int64_t npoints, const float* vertices,
                                    int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* pair_face, int64_t npairs,
                                    const int32_t* cell_start, const sp3_nn_grid* g, void* ws, int32_t* count, uint8_t* mask, void* stream) {
  if (check_vis_args("sp3_mesh_point_views", T, pixel_offset, bias, cull, nverts, nfaces, npoints)) return 1;
  SP3_CHECK(npairs >= 0 && npairs < N_MAX, "sp3_mesh_point_views: npairs = %lld out of range", (long long)npairs);
  if (check_grid(g, "sp3_mesh_point_views")) return 1;
  if (T == 0 || npoints == 0) return 0;
  SP3_CHECK(views_host && views_dev && points && count && faces && ws && (nverts == 0 || vertices) && (npairs == 0 || (pair_face && cell_start)),
            "sp3_mesh_point_views: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_point_views")) return e;
  if (check_vis_views("sp3_mesh_point_views", views_host, T)) return 1;
  const GridWalker<true> w = {mesh_ref(vertices, nverts, faces, nfaces, pair_face, npairs, cell_start), *g};
  k_point_views<<<point_views_grid(npoints, T), TB, 0, st>>>(views_dev, pixel_offset, bias, cull, points, q_order, npoints, w, (int*)count, mask,
                                                             (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_point_views");
  return 0;
}
