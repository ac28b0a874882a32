// The two front ends of "Mesh rays" (include/spann3r_hip.h), per translation unit: one lane per given ray, and one lane per pixel
// of a table of cameras; with the host checks their entry points share.  csrc/mesh_ray.hip (the cell grid) and csrc/mesh_bvh.hip
// (the tree) instantiate them with a Walker, a struct passed by value that says which faces a ray looks at:
//     void prepare(unsigned* lds)      once per workgroup, every lane: `lds` is the launch's dynamic LDS (the grid asks for none)
//     int walk(const Ray&, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, int& steps, int& evals)      -> the winning face, -1: none
//     int walk<true>(the same)          the occlusion mode ("Mesh visibility"): stops at the first accepted hit -> some face hit, -1: none
//     m                                 the mesh: verts, nverts, faces, nfaces
// The two front ends of "Mesh visibility" follow them: one lane per given ray that stores whether it is occluded, and one lane per
// (point, view) pair of a table of cameras.
// Everything a ray reports comes from csrc/tri_ray.h (make_ray, result_of, store, pixel_ray, store_pixel) and the lane's query
// from query_of (csrc/cell_grid.h), so the structures cannot differ in anything but the faces they visit.
#pragma once
#include "cell_grid.h"
#include "tri_ray.h"

namespace {

constexpr int VIEW_TILE = 16;                  // a workgroup of k_ray_views: 16 x 16 pixels, four 8 x 8 wave tiles
static_assert(TB == VIEW_TILE * VIEW_TILE, "one workgroup size, and one stack stride, for both front ends");

// ---- one lane per ray, in the given order (sorted by the structure's own key: the lanes of a wave visit the same cells or nodes)
template <typename Walker>
__global__ __launch_bounds__(TB) void k_ray_query(const float* __restrict__ org, const float* __restrict__ dir, const int64_t* __restrict__ order,
                                                   int64_t nq, Walker w, double t_min, double t_max, int cull, RayOut out, GridHead* head) {
  extern __shared__ unsigned s_dyn[];
  w.prepare(s_dyn);
  int steps = 0, evals = 0;
  const int64_t qi = query_of(order, (int64_t)blockIdx.x * TB + threadIdx.x, nq);
  if (qi >= 0) {
    const float ox = org[3 * qi], oy = org[3 * qi + 1], oz = org[3 * qi + 2], dx = dir[3 * qi], dy = dir[3 * qi + 1], dz = dir[3 * qi + 2];
    const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
    const int bf = r.ok ? w.walk(r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, steps, evals) : -1;
    store(out, qi, result_of(w.m.verts, w.m.nverts, w.m.faces, w.m.nfaces, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, bf));
  }
  head->count(steps, evals);
}

// ---- T cameras in one launch: a lane owns a pixel, a wave an 8 x 8 tile, a workgroup 16 x 16 pixels of view blockIdx.z
template <typename Walker>
__global__ __launch_bounds__(TB) void k_ray_views(const sp3_mesh_ray_view* __restrict__ views, float pixel_offset, Walker w, GridHead* head) {
  extern __shared__ unsigned s_dyn[];
  w.prepare(s_dyn);
  const sp3_mesh_ray_view& vw = views[blockIdx.z];      // (wave-uniform: the descriptor fields arrive by scalar loads)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * VIEW_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * VIEW_TILE + (wave >> 1) * 8 + (lane >> 3);
  int steps = 0, evals = 0;
  if (px < vw.w && py < vw.h) {
    float oo[3], dd[3];
    pixel_ray(vw, px, py, pixel_offset, oo, dd);
    const double t_min = (double)vw.near, t_max = (double)vw.far;
    const Ray r = make_ray(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2]);
    const int bf = r.ok ? w.walk(r, oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], t_min, t_max, CULL_NONE, steps, evals) : -1;
    store_pixel(vw, px, py, result_of(w.m.verts, w.m.nverts, w.m.faces, w.m.nfaces, r, oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], t_min, t_max,
                                      CULL_NONE, bf));
  }
  head->count(steps, evals);
}

// ---- "Mesh visibility": one lane per given ray, as k_ray_query, but only whether SOME face is a hit: walk<true> stops at the first
// accepted one.  One byte stored per ray.
template <typename Walker>
__global__ __launch_bounds__(TB) void k_ray_occluded(const float* __restrict__ org, const float* __restrict__ dir, const int64_t* __restrict__ order,
                                                      int64_t nq, Walker w, double t_min, double t_max, int cull, uint8_t* __restrict__ occluded,
                                                      GridHead* head) {
  extern __shared__ unsigned s_dyn[];
  w.prepare(s_dyn);
  int steps = 0, evals = 0;
  const int64_t qi = query_of(order, (int64_t)blockIdx.x * TB + threadIdx.x, nq);
  if (qi >= 0) {
    const float ox = org[3 * qi], oy = org[3 * qi + 1], oz = org[3 * qi + 2], dx = dir[3 * qi], dy = dir[3 * qi + 1], dz = dir[3 * qi + 2];
    const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
    const int f = r.ok ? w.template walk<true>(r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, steps, evals) : -1;
    occluded[qi] = f >= 0 ? 1 : 0;
  }
  head->count(steps, evals);
}

// ---- one lane per (point, view) pair, the view in blockIdx.y (wave-uniform: its fields arrive by scalar loads), the points in the
// order of the structure's own key: the lanes of a wave shoot from one origin at neighbouring targets.  The projection tests of the
// header's rule 2 run first; a pair outside the frustum walks nothing.
template <typename Walker>
__global__ __launch_bounds__(TB) void k_point_views(const sp3_mesh_vis_view* __restrict__ views, float pixel_offset, float bias, int cull,
                                                     const float* __restrict__ pts, const int64_t* __restrict__ order, int64_t np, Walker w,
                                                     int* __restrict__ count, uint8_t* __restrict__ mask, GridHead* head) {
#pragma clang fp contract(off)
  extern __shared__ unsigned s_dyn[];
  w.prepare(s_dyn);
  const sp3_mesh_vis_view& vw = views[blockIdx.y];
  int steps = 0, evals = 0;
  const int64_t qi = query_of(order, (int64_t)blockIdx.x * TB + threadIdx.x, np);
  if (qi >= 0) {
    const float p0 = pts[3 * qi], p1 = pts[3 * qi + 1], p2 = pts[3 * qi + 2];
    const double q0 = (double)p0, q1 = (double)p1, q2 = (double)p2;
    bool vis = false;
    if (is_finite(fabs(q0)) && is_finite(fabs(q1)) && is_finite(fabs(q2))) {
      double c[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double a = (double)vw.w2c[4 * i] * q0, b = (double)vw.w2c[4 * i + 1] * q1, e = (double)vw.w2c[4 * i + 2] * q2;
        c[i] = ((a + b) + e) + (double)vw.w2c[4 * i + 3];
      }
      const double z = c[2];
      if (z > 0.0 && (double)vw.near <= z && z <= (double)vw.far) {
        const double u = (c[0] / z) * (double)vw.fu + (double)vw.cu, v = (c[1] / z) * (double)vw.fv + (double)vw.cv;
        const double su = (u - (double)pixel_offset) + 0.5, sv = (v - (double)pixel_offset) + 0.5;
        if (su >= 0.0 && su < (double)vw.w && sv >= 0.0 && sv < (double)vw.h) {
          const float ox = vw.c2w[3], oy = vw.c2w[7], oz = vw.c2w[11];
          const float dx = (float)(q0 - (double)ox), dy = (float)(q1 - (double)oy), dz = (float)(q2 - (double)oz);
          const double t_min = (double)vw.near / z, t_max = 1.0 - (double)bias;
          const Ray r = make_ray(ox, oy, oz, dx, dy, dz);
          const int f = r.ok ? w.template walk<true>(r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, steps, evals) : -1;
          vis = f < 0;
        }
      }
    }
    if (vis) atomicAdd(&count[qi], 1);
    if (mask != nullptr) mask[(int64_t)blockIdx.y * np + qi] = vis ? 1 : 0;
  }
  head->count(steps, evals);
}

// ------------------------------------------------------------------------------------------------ host
inline bool range_ok(double t_min, double t_max) { return t_min >= 0.0 && t_min <= t_max; }      // (false for a NaN)

// what every ray entry point that takes rays asks of its scalars
inline int check_mesh_args(const char* what, int64_t nverts, int64_t nfaces, int64_t nq, double t_min, double t_max, int cull) {
  if (check_query_args(what, nverts, nfaces, nq)) return 1;
  SP3_CHECK(range_ok(t_min, t_max), "%s: 0 <= t_min <= t_max, got %g and %g", what, t_min, t_max);
  SP3_CHECK(cull >= CULL_NONE && cull <= CULL_FRONT, "%s: cull %d must be 0 (none), 1 (back) or 2 (front)", what, cull);
  return 0;
}

// the count of views and the pixel offset, checked before the structure is looked at
inline int check_view_args(const char* what, int T, float pixel_offset) {
  SP3_CHECK(T >= 0 && T <= 65535, "%s: T %d must be in 0 .. 65535", what, T);
  SP3_CHECK(isfinite(pixel_offset), "%s: pixel_offset is not finite", what);
  return 0;
}

// the host copy of the table of T >= 1 views, entry by entry -> the launch grid that covers the largest of them
inline int check_views(const char* what, const sp3_mesh_ray_view* views_host, int T, dim3& grid) {
  int wmax = 0, hmax = 0;
  for (int i = 0; i < T; ++i) {
    const sp3_mesh_ray_view& v = views_host[i];
    SP3_CHECK(v.w >= 1 && v.h >= 1 && v.w <= (1 << 24) && v.h <= (1 << 24) && v.row_stride >= v.w && (int64_t)v.h * v.row_stride < N_MAX / 3,
              "%s: view %d: bad geometry: %d x %d, row stride %lld", what, i, v.w, v.h, (long long)v.row_stride);
    SP3_CHECK(v.depth != nullptr, "%s: view %d: null depth map", what, i);
    SP3_CHECK(isfinite(v.fu) && isfinite(v.fv) && isfinite(v.cu) && isfinite(v.cv) && v.fu != 0.f && v.fv != 0.f,
              "%s: view %d: intrinsics must be finite with non-zero focal lengths", what, i);
    SP3_CHECK(range_ok((double)v.near, (double)v.far), "%s: view %d: 0 <= near <= far, got %g and %g", what, i, (double)v.near, (double)v.far);
    wmax = v.w > wmax ? v.w : wmax;
    hmax = v.h > hmax ? v.h : hmax;
  }
  grid = dim3((wmax + VIEW_TILE - 1) / VIEW_TILE, (hmax + VIEW_TILE - 1) / VIEW_TILE, T);
  SP3_CHECK(grid.y <= 65535, "%s: %d rows of pixels are more than one launch covers", what, hmax);
  return 0;
}

// what the point-visibility entry points ask of their scalars, before the structure is looked at
inline int check_vis_args(const char* what, int T, float pixel_offset, float bias, int cull, int64_t nverts, int64_t nfaces, int64_t np) {
  if (check_query_args(what, nverts, nfaces, np) || check_view_args(what, T, pixel_offset)) return 1;
  SP3_CHECK(bias >= 0.f && bias < 1.f, "%s: bias %g must lie in [0, 1)", what, (double)bias);
  SP3_CHECK(cull >= CULL_NONE && cull <= CULL_FRONT, "%s: cull %d must be 0 (none), 1 (back) or 2 (front)", what, cull);
  return 0;
}

// the host copy of the table of T >= 1 visibility views, entry by entry, as check_views checks the views of a depth render
inline int check_vis_views(const char* what, const sp3_mesh_vis_view* views_host, int T) {
  for (int i = 0; i < T; ++i) {
    const sp3_mesh_vis_view& v = views_host[i];
    SP3_CHECK(v.w >= 1 && v.h >= 1 && v.w <= (1 << 24) && v.h <= (1 << 24), "%s: view %d: bad geometry: %d x %d", what, i, v.w, v.h);
    SP3_CHECK(isfinite(v.fu) && isfinite(v.fv) && isfinite(v.cu) && isfinite(v.cv) && v.fu != 0.f && v.fv != 0.f,
              "%s: view %d: intrinsics must be finite with non-zero focal lengths", what, i);
    SP3_CHECK(range_ok((double)v.near, (double)v.far), "%s: view %d: 0 <= near <= far, got %g and %g", what, i, (double)v.near, (double)v.far);
  }
  return 0;
}

// the launch of k_point_views: x covers the points, y the views
inline dim3 point_views_grid(int64_t np, int T) { return dim3(blocks_for(np), (unsigned)T, 1); }

}  // namespace
