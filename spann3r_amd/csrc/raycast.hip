// TSDF ray-casting and frame-to-model tracking (include/spann3r_hip.h, "TSDF ray-casting and frame-to-model tracking";
// spann3r_amd/fusion.py drives these): per camera the depth, world vertex, unit normal and colour of the zero level of a volume of
// csrc/fusion.hip with no meshing, and the normal equations of projective point-to-plane registration of one frame against such maps.
//
// sp3_tsdf_raycast is ONE launch for all views of a call: a lane owns a pixel, a wave an 8 x 8 pixel tile, a workgroup a 16 x 16
// block of one view (blockIdx.z), so the view descriptor is read through a wave-uniform index of a read-only table (scalar loads)
// and the rays of a wave walk neighbouring cells: its 8 gathers per sample fall into few cache lines.  The march is bounded by a
// sample count the host computes; no atomics, no LDS, no workgroup waits on another.
//
// sp3_tsdf_track_accum is the fp64 fixed-order sum of csrc/slab.h over the points of the frame: 29 running sums per thread.
//
// The march of a pixel is raycast_pixel (csrc/tsdf.h), shared with the brick volume (csrc/bricks.hip); this file supplies the dense
// volume's cell gather.
//
// Every fp32 operation of the ray-caster is rounded on its own (no contraction into FMAs): the file-level pragma below (csrc/tsdf.h
// sets the same for its own text) is what the compiler honours under its default -ffp-contract=fast-honor-pragmas.
// tests/raycast_ref.py restates it operation for operation.
#include "common.h"
#include "slab.h"
#include "tsdf.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

// the dense volume as raycast_pixel's Vol
struct DenseVol {
  const RcVol& g;
  const float* __restrict__ tsdf;
  const float* __restrict__ weight;

  struct Cell {
    int64_t base;      // linear index of corner 0
    float tx, ty, tz;
    float v[8];        // tsdf of corner code c = dx + 2 dy + 4 dz
  };

  __device__ __forceinline__ int64_t corner(const Cell& c, int e) const {
    return c.base + (e & 1) + (int64_t)g.nx * (((e >> 1) & 1) + (int64_t)g.ny * (e >> 2));
  }

  // The cell of point (px, py, pz) by the header's rule; INVALID: outside the lattice or a corner below min_weight.
  __device__ __forceinline__ int load(float px, float py, float pz, Cell& c) const {
    const float gx = (px - g.ox) / g.voxel, gy = (py - g.oy) / g.voxel, gz = (pz - g.oz) / g.voxel;
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    if (!(fx >= 0.f && fx <= (float)(g.nx - 2) && fy >= 0.f && fy <= (float)(g.ny - 2) && fz >= 0.f && fz <= (float)(g.nz - 2)))
      return CELL_INVALID;
    c.base = ((int64_t)(int)fz * g.ny + (int)fy) * g.nx + (int)fx;      // (every corner index stays inside the volume: i <= n - 2 per axis)
    c.tx = gx - fx;
    c.ty = gy - fy;
    c.tz = gz - fz;
    bool seen = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t q = corner(c, e);
      seen = seen && weight[q] >= g.min_weight;
      c.v[e] = tsdf[q];
    }
    return seen ? CELL_VALID : CELL_INVALID;
  }

  __device__ __forceinline__ int skip(const Ray&, int i, const Cell&) const { return i; }      // (load never says ABSENT)
};

template <bool RGB>
__global__ __launch_bounds__(RC_TILE * RC_TILE) void k_tsdf_raycast(const sp3_tsdf_view* __restrict__ views, RcVol g,
                                                                   const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                   const float* __restrict__ rgb) {
  const sp3_tsdf_view& vw = views[blockIdx.z];      // (wave-uniform: the descriptor fields arrive by scalar loads)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (px >= vw.w || py >= vw.h) return;
  raycast_pixel<RGB>(vw, px, py, DenseVol{g, tsdf, weight}, rgb);
}

// ------------------------------------------------------------------------------------------------ tracking
struct TrackView {
  const float *vertex, *normal, *depth;
  int64_t row_stride;
  int w, h;
  double fu, fv, cu, cv, dist2_max;
};

__global__ __launch_bounds__(256) void k_tsdf_track_accum(const float* __restrict__ pts, const uint8_t* __restrict__ valid, int64_t n,
                                                          const double* __restrict__ T12, const double* __restrict__ w2c12, TrackView mv,
                                                          double* __restrict__ slab) {
  double s[29];
#pragma unroll
  for (int e = 0; e < 29; ++e) s[e] = 0.0;
  double R[12], M[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    R[e] = T12[e];
    M[e] = w2c12[e];
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (valid != nullptr && valid[i] == 0) continue;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    const double yx = R[0] * x + R[1] * y + R[2] * z + R[9], yy = R[3] * x + R[4] * y + R[5] * z + R[10],
                 yz = R[6] * x + R[7] * y + R[8] * z + R[11];
    const double cz = M[6] * yx + M[7] * yy + M[8] * yz + M[11];
    if (!(cz > 0.0)) continue;
    const double cx = M[0] * yx + M[1] * yy + M[2] * yz + M[9], cy = M[3] * yx + M[4] * yy + M[5] * yz + M[10];
    const double fpx = floor(mv.fu * cx / cz + mv.cu + 0.5), fpy = floor(mv.fv * cy / cz + mv.cv + 0.5);
    if (!(fpx >= 0.0 && fpx < (double)mv.w && fpy >= 0.0 && fpy < (double)mv.h)) continue;      // (a NaN fails)
    const int64_t p = (int64_t)fpy * mv.row_stride + (int64_t)fpx;
    if (mv.depth[p] == 0.f) continue;
    const double qx = mv.vertex[3 * p], qy = mv.vertex[3 * p + 1], qz = mv.vertex[3 * p + 2];
    const double nx = mv.normal[3 * p], ny = mv.normal[3 * p + 1], nz = mv.normal[3 * p + 2];
    const double ddx = yx - qx, ddy = yy - qy, ddz = yz - qz;
    if (!(ddx * ddx + ddy * ddy + ddz * ddz <= mv.dist2_max)) continue;
    const double r = nx * ddx + ny * ddy + nz * ddz;
    const double J[6] = {yy * nz - yz * ny, yz * nx - yx * nz, yx * ny - yy * nx, nx, ny, nz};
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) s[e++] += J[a] * J[b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) s[21 + a] += J[a] * r;
    s[27] += r * r;
    s[28] += 1.0;
  }
  block_slab<29>(s, slab);
}

int check_rc_volume(const char* what, int nx, int ny, int nz, float voxel) {
  SP3_CHECK(nx >= 0 && ny >= 0 && nz >= 0, "%s: dims %d x %d x %d must be >= 0", what, nx, ny, nz);
  const int64_t lim = 0x7fffffffLL / 7;
  SP3_CHECK((int64_t)nx * ny <= lim && (int64_t)nx * ny * nz <= lim,
            "%s: dims %d x %d x %d over the index limit: 7 nx ny nz must stay below 2^31 (the volume of sp3_tsdf_integrate)", what, nx, ny, nz);
  SP3_CHECK(isfinite(voxel) && voxel > 0.f, "%s: voxel %g must be finite and > 0", what, (double)voxel);
  return 0;
}

}  // namespace

extern "C" int sp3_tsdf_raycast(const sp3_tsdf_view* views_host, const sp3_tsdf_view* views_dev, int T, int nx, int ny, int nz,
                                const float* origin3, float voxel, const float* tsdf, const float* weight, const float* rgb, float min_weight,
                                float step, void* stream) {
  if (check_rc_volume("sp3_tsdf_raycast", nx, ny, nz, voxel)) return 1;
  SP3_CHECK(T >= 0 && T <= 65535, "sp3_tsdf_raycast: T %d must be in 0 .. 65535", T);
  RcVol g;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.bx = g.by = g.bz = 0;
  g.voxel = voxel;
  if (check_march("sp3_tsdf_raycast", min_weight, step, g)) return 1;
  if (T == 0) return 0;
  int wmax, hmax;
  if (check_views("sp3_tsdf_raycast", views_host, views_dev, T, rgb != nullptr, wmax, hmax)) return 1;
  if ((int64_t)nx * ny * nz == 0) return 0;
  SP3_CHECK(origin3 != nullptr && tsdf != nullptr && weight != nullptr, "sp3_tsdf_raycast: null origin/tsdf/weight");
  SP3_CHECK(isfinite(origin3[0]) && isfinite(origin3[1]) && isfinite(origin3[2]), "sp3_tsdf_raycast: origin is not finite");
  g.ox = origin3[0]; g.oy = origin3[1]; g.oz = origin3[2];
  dim3 grid;
  if (view_grid("sp3_tsdf_raycast", wmax, hmax, T, grid)) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (rgb != nullptr)
    hipLaunchKernelGGL(k_tsdf_raycast<true>, grid, dim3(RC_TILE * RC_TILE), 0, st, views_dev, g, tsdf, weight, rgb);
  else
    hipLaunchKernelGGL(k_tsdf_raycast<false>, grid, dim3(RC_TILE * RC_TILE), 0, st, views_dev, g, tsdf, weight, rgb);
  SP3_LAUNCH_CHECK("sp3_tsdf_raycast");
  return 0;
}

extern "C" int64_t sp3_tsdf_track_accum_ws_bytes(int64_t n) { return (int64_t)slab_blocks(n) * 29 * 8; }

extern "C" int sp3_tsdf_track_accum(const float* pts, const uint8_t* valid, int64_t n, const double* T12, const float* vertex, const float* normal,
                                    const float* depth, int w, int h, int64_t row_stride, float fu, float fv, float cu, float cv,
                                    const double* w2c12, float dist_max, void* ws, double* out29, void* stream) {
  SP3_CHECK(n >= 0 && n <= 0x7fffffffLL, "sp3_tsdf_track_accum: n = %lld out of range", (long long)n);
  SP3_CHECK(w >= 1 && h >= 1 && w <= (1 << 24) && h <= (1 << 24) && row_stride >= w && (int64_t)h * row_stride < 0x7fffffffLL,
            "sp3_tsdf_track_accum: bad geometry: %d x %d, row stride %lld", w, h, (long long)row_stride);
  SP3_CHECK(isfinite(fu) && isfinite(fv) && isfinite(cu) && isfinite(cv), "sp3_tsdf_track_accum: intrinsics are not finite");
  SP3_CHECK(dist_max >= 0.f, "sp3_tsdf_track_accum: dist_max %g must be >= 0", (double)dist_max);
  SP3_CHECK(T12 != nullptr && vertex != nullptr && normal != nullptr && depth != nullptr && w2c12 != nullptr && ws != nullptr && out29 != nullptr &&
                (n == 0 || pts != nullptr),
            "sp3_tsdf_track_accum: null pts/T12/vertex/normal/depth/w2c12/ws/out29");
  TrackView mv;
  mv.vertex = vertex; mv.normal = normal; mv.depth = depth;
  mv.row_stride = row_stride; mv.w = w; mv.h = h;
  mv.fu = fu; mv.fv = fv; mv.cu = cu; mv.cv = cv;
  mv.dist2_max = (double)dist_max * (double)dist_max;
  const int nb = slab_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tsdf_track_accum, dim3(nb), dim3(256), 0, st, pts, valid, n, T12, w2c12, mv, (double*)ws);
  hipLaunchKernelGGL(slab_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nb, 29, out29);
  SP3_LAUNCH_CHECK("sp3_tsdf_track_accum");
  return 0;
}
