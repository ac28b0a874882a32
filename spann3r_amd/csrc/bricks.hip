// Brick TSDF volume (include/spann3r_hip.h, "Brick TSDF volume"; spann3r_amd/fusion.py BrickTSDFVolume drives these): the volume
// of csrc/fusion.hip on two levels.  A table of 8 x 8 x 8-voxel bricks over a virtual grid names a slot of a pool for every brick a
// measurement came near; only those bricks hold voxels.
//
// sp3_tsdf_brick_mark: a lane owns a pixel and flags the bricks its band box touches (plain byte stores of 1).
// sp3_tsdf_brick_alloc: the new bricks get slots in linear brick order by the tile count / single-workgroup scan / scatter of
//   csrc/scan.h; every kernel of the chain computes need = count + new itself and writes nothing when it exceeds the capacity.
// sp3_tsdf_brick_integrate: a workgroup owns a brick (512 lanes, a wave an 8 x 8 slab of one z), a lane a voxel; the per-frame
//   rule is integrate_voxel (csrc/tsdf.h), the one k_tsdf_integrate (csrc/fusion.hip) calls.
// sp3_tsdf_brick_raycast: the march of raycast_pixel (csrc/tsdf.h), the one k_tsdf_raycast (csrc/raycast.hip) calls, with the cell
//   gathered through the table.  A sample whose corner 0 lies in an absent brick is invalid; the lane then looks for a later sample
//   whose corner 0 lies in the SAME brick.  The coordinates of corner 0 are monotone in the sample index (every rounded operation
//   of the sample rule is monotone), so all samples in between lie in that brick too and are invalid: they are passed over without
//   being evaluated.  The jump is a guess from the ray's slope; the proof is the check of the sample it lands on.
// sp3_tsdf_brick_to_dense: a lane owns a voxel of the box.
//
// The shared rules keep both volumes' bits: csrc/tsdf.h switches contraction off for its own text and nothing is built with
// fast-math, so every fp32 operation is one IEEE operation wherever it is inlined.  Compiled for gfx950, the integrate kernels of
// both volumes came out of the move with the same instructions (profiles/tsdf_shared.txt).
//
// Every fp32 operation is rounded on its own (no contraction into FMAs): the file-level pragma below is what the compiler honours
// under its default -ffp-contract=fast-honor-pragmas.  No atomics, no workgroup waits on another.
#include "common.h"
#include "scan.h"
#include "tsdf.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

#define BRK 8                // voxels per brick side
#define BRK_VOX 512          // voxels per brick = lanes of an integrate workgroup
#define INIT_BLOCKS 1024     // workgroups of the slot initialisation (they stride over the new slots)

struct BVol {
  int nx, ny, nz, bx, by, bz;
  float ox, oy, oz, voxel, trunc;
};

__device__ __forceinline__ int64_t brick_index(const BVol& g, int I, int J, int K) { return ((int64_t)K * g.by + J) * g.bx + I; }

// ------------------------------------------------------------------------------------------------ mark
__global__ __launch_bounds__(MB) void k_brick_mark(const sp3_tsdf_frame* __restrict__ frames, const float* __restrict__ c2w, BVol g, float band,
                                                   uint8_t* __restrict__ flags) {
  const sp3_tsdf_frame& fr = frames[blockIdx.y];      // (wave-uniform: the descriptor fields arrive by scalar loads)
  const int64_t q = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (q >= (int64_t)fr.w * fr.h) return;
  const int py = (int)(q / fr.w), px = (int)(q - (int64_t)py * fr.w);
  const int64_t p = (int64_t)py * fr.row_stride + px;
  if (fr.valid != nullptr && fr.valid[p] == 0) return;
  float P[3], d;
  if (fr.depth != nullptr) {
    d = fr.depth[p];
    if (!isfinite(d) || d <= 0.f) return;
    const float* m = c2w + 12 * (int64_t)blockIdx.y;
    const float xn = ((float)px - fr.cu) / fr.fu, yn = ((float)py - fr.cv) / fr.fv;
    const float X = xn * d, Y = yn * d;
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r] = ((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * d) + m[4 * r + 3];
  } else {
    const float* m = fr.w2c;
    P[0] = fr.pts[3 * p];
    P[1] = fr.pts[3 * p + 1];
    P[2] = fr.pts[3 * p + 2];
    d = ((m[8] * P[0] + m[9] * P[1]) + m[10] * P[2]) + m[11];
    if (!isfinite(d) || d <= 0.f) return;
  }
  const float a = fr.pixel_weight != nullptr ? fr.pixel_weight[p] : 1.0f;
  if (!(a > 0.f) || !isfinite(a)) return;
  if (!(isfinite(P[0]) && isfinite(P[1]) && isfinite(P[2]))) return;
  const float o3[3] = {g.ox, g.oy, g.oz};
  const int n3[3] = {g.nx, g.ny, g.nz};
  int b0[3], b1[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    float lo = floorf(((P[ax] - band) - o3[ax]) / g.voxel), hi = floorf(((P[ax] + band) - o3[ax]) / g.voxel) + 1.0f;
    const float last = (float)(n3[ax] - 1);
    if (!(hi >= 0.f && lo <= last)) return;      // the box misses the grid (a NaN fails)
    lo = lo < 0.f ? 0.f : lo;
    hi = hi > last ? last : hi;
    b0[ax] = (int)lo >> 3;      // (0 <= lo <= hi <= n - 1: every brick index below stays inside the table)
    b1[ax] = (int)hi >> 3;
  }
  for (int K = b0[2]; K <= b1[2]; ++K)
    for (int J = b0[1]; J <= b1[1]; ++J)
      for (int I = b0[0]; I <= b1[0]; ++I) flags[brick_index(g, I, J, K)] = 1;
}

// ------------------------------------------------------------------------------------------------ alloc
__global__ __launch_bounds__(MB) void k_brick_new_count(const uint8_t* __restrict__ flags, const int* __restrict__ table, int64_t nb,
                                                        int* __restrict__ tile) {
  const int64_t b = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool fresh = b < nb && flags[b] != 0 && table[b] < 0;
  int total;
  block_rank(fresh, total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// tile[ntiles] = the number of new bricks (k_tile_scan); need = count + that
__global__ __launch_bounds__(MB) void k_brick_new_scatter(uint8_t* __restrict__ flags, int* __restrict__ table, int* __restrict__ slot_brick,
                                                          const int* __restrict__ count, const int* __restrict__ tile, int ntiles, int64_t nb,
                                                          int64_t capacity) {
  const int64_t b = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool fresh = b < nb && flags[b] != 0 && table[b] < 0;
  int total;
  const int rank = block_rank(fresh, total);
  const int64_t old = count[0], need = old + tile[ntiles];
  if (b >= nb || need > capacity) return;
  flags[b] = 0;
  if (fresh) {
    const int64_t slot = old + tile[blockIdx.x] + rank;      // (< need <= capacity)
    table[b] = (int)slot;
    slot_brick[slot] = (int)b;
  }
}

__global__ __launch_bounds__(MB) void k_brick_slot_init(const int* __restrict__ count, const int* __restrict__ tile, int ntiles, int64_t capacity,
                                                        float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb) {
  const int64_t old = count[0], need = old + tile[ntiles];
  if (need > capacity) return;
  for (int64_t s = old + blockIdx.x; s < need; s += gridDim.x) {
    for (int t = threadIdx.x; t < BRK_VOX; t += MB) {
      const int64_t v = s * BRK_VOX + t;
      tsdf[v] = 1.0f;
      weight[v] = 0.0f;
      if (rgb != nullptr) {
        rgb[3 * v] = 0.0f;
        rgb[3 * v + 1] = 0.0f;
        rgb[3 * v + 2] = 0.0f;
      }
    }
  }
}

// the one launch that changes `count`; everything before it read the old value
__global__ void k_brick_alloc_finish(int* __restrict__ count, const int* __restrict__ tile, int ntiles, int64_t capacity, int* __restrict__ counts2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t need = (int64_t)count[0] + tile[ntiles];      // (capacity + bricks < 2^31: no overflow)
  if (need <= capacity) count[0] = (int)need;
  counts2[0] = count[0];
  counts2[1] = (int)need;
}

// ------------------------------------------------------------------------------------------------ integrate
template <bool RGB>
__global__ __launch_bounds__(BRK_VOX) void k_brick_integrate(const sp3_tsdf_frame* __restrict__ frames, int T, BVol g,
                                                            const int* __restrict__ slot_brick, float* __restrict__ tsdf,
                                                            float* __restrict__ weight, float* __restrict__ rgb) {
  const int brick = slot_brick[blockIdx.x];      // (wave-uniform)
  const int I = brick % g.bx, J = (brick / g.bx) % g.by, K = brick / (g.bx * g.by);
  const int t = threadIdx.x;
  const int i = I * BRK + (t & 7), j = J * BRK + ((t >> 3) & 7), k = K * BRK + (t >> 6);
  const int64_t v = (int64_t)blockIdx.x * BRK_VOX + t;
  const float x = g.ox + (float)i * g.voxel, y = g.oy + (float)j * g.voxel, z = g.oz + (float)k * g.voxel;
  float D = tsdf[v], W = weight[v];
  float cr = 0.f, cg = 0.f, cb = 0.f;
  if (RGB) {
    cr = rgb[3 * v];
    cg = rgb[3 * v + 1];
    cb = rgb[3 * v + 2];
  }
  integrate_voxel<RGB>(frames, T, x, y, z, g.trunc, D, W, cr, cg, cb);
  tsdf[v] = D;
  weight[v] = W;
  if (RGB) {
    rgb[3 * v] = cr;
    rgb[3 * v + 1] = cg;
    rgb[3 * v + 2] = cb;
  }
}

// ------------------------------------------------------------------------------------------------ ray-casting
// lattice coordinates of corner 0 of the cell of a point, by the header's rule; false outside the lattice (a NaN fails)
__device__ __forceinline__ bool cell_floor(const RcVol& g, float px, float py, float pz, float& gx, float& gy, float& gz, float& fx, float& fy,
                                           float& fz) {
  gx = (px - g.ox) / g.voxel;
  gy = (py - g.oy) / g.voxel;
  gz = (pz - g.oz) / g.voxel;
  fx = floorf(gx);
  fy = floorf(gy);
  fz = floorf(gz);
  return fx >= 0.f && fx <= (float)(g.nx - 2) && fy >= 0.f && fy <= (float)(g.ny - 2) && fz >= 0.f && fz <= (float)(g.nz - 2);
}

// the brick volume as raycast_pixel's Vol (csrc/tsdf.h)
struct BrickVol {
  const RcVol& g;
  const int* __restrict__ table;
  const float* __restrict__ tsdf;
  const float* __restrict__ weight;

  struct Cell {
    int64_t q[8];      // pool index of corner code c = dx + 2 dy + 4 dz
    float tx, ty, tz;
    float v[8];
    int bI, bJ, bK;    // the brick of corner 0
  };

  __device__ __forceinline__ int64_t corner(const Cell& c, int e) const { return c.q[e]; }

  // The cell of point (px, py, pz) on the densified volume: a corner in an absent brick has weight 0 < min_weight.
  __device__ __forceinline__ int load(float px, float py, float pz, Cell& c) const {
    float gx, gy, gz, fx, fy, fz;
    if (!cell_floor(g, px, py, pz, gx, gy, gz, fx, fy, fz)) return CELL_INVALID;
    const int i = (int)fx, j = (int)fy, k = (int)fz;
    c.bI = i >> 3;
    c.bJ = j >> 3;
    c.bK = k >> 3;
    const int s0 = table[((int64_t)c.bK * g.by + c.bJ) * g.bx + c.bI];
    if (s0 < 0) return CELL_ABSENT;
    c.tx = gx - fx;
    c.ty = gy - fy;
    c.tz = gz - fz;
    const bool inner = (i & 7) < 7 && (j & 7) < 7 && (k & 7) < 7;      // all eight corners in the brick of corner 0
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ci = i + (e & 1), cj = j + ((e >> 1) & 1), ck = k + (e >> 2);      // (<= n - 1 per axis: inside the table)
      int s = s0;
      if (!inner) {
        const int cI = ci >> 3, cJ = cj >> 3, cK = ck >> 3;
        if (cI != c.bI || cJ != c.bJ || cK != c.bK) s = table[((int64_t)cK * g.by + cJ) * g.bx + cI];
      }
      if (s < 0) return CELL_INVALID;
      const int64_t q = (int64_t)s * BRK_VOX + (((ck & 7) << 6) | ((cj & 7) << 3) | (ci & 7));
      if (!(weight[q] >= g.min_weight)) return CELL_INVALID;
      c.q[e] = q;
      c.v[e] = tsdf[q];
    }
    return CELL_VALID;
  }

  // Sample i's corner 0 lies in the absent brick (c.bI, c.bJ, c.bK).  -> the largest index found (>= i) whose sample is inside the
  // march (index < cap, lambda <= lambda1) and has its corner 0 in the same brick; every sample from i to it is then invalid (see the
  // head of the file).  The guess comes from the slope; only the check decides.
  __device__ __forceinline__ int skip(const Ray& r, int i, const Cell& c) const {
    const float lam = r.lam0 + (float)i * r.dl;
    float gx, gy, gz, fx, fy, fz;
    cell_floor(g, r.ex + r.dx * lam, r.ey + r.dy * lam, r.ez + r.dz * lam, gx, gy, gz, fx, fy, fz);
    const float lo3[3] = {(float)(c.bI * BRK), (float)(c.bJ * BRK), (float)(c.bK * BRK)};
    const float g3[3] = {gx, gy, gz}, d3[3] = {r.dx, r.dy, r.dz};
    float room = 64.0f;      // samples; a brick's diagonal is under 56 samples at the smallest step (a quarter voxel)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float per = d3[a] * r.dl / g.voxel;      // lattice units per sample
      if (per > 0.f) {
        const float q = (lo3[a] + (float)BRK - g3[a]) / per;
        room = q < room ? q : room;
      } else if (per < 0.f) {
        const float q = (lo3[a] - g3[a]) / per;
        room = q < room ? q : room;
      }
    }
    int n = room > 0.f ? (int)room : 0;
    if (n > g.cap - 1 - i) n = g.cap - 1 - i;
    bool first = true;
    while (n > 0) {
      const float l2 = r.lam0 + (float)(i + n) * r.dl;
      if (l2 <= r.lam1) {
        cell_floor(g, r.ex + r.dx * l2, r.ey + r.dy * l2, r.ez + r.dz * l2, gx, gy, gz, fx, fy, fz);
        if (fx >= lo3[0] && fx < lo3[0] + (float)BRK && fy >= lo3[1] && fy < lo3[1] + (float)BRK && fz >= lo3[2] && fz < lo3[2] + (float)BRK)
          return i + n;
      }
      n = first ? n - 1 : n >> 1;
      first = false;
    }
    return i;
  }
};

template <bool RGB>
__global__ __launch_bounds__(RC_TILE * RC_TILE) void k_brick_raycast(const sp3_tsdf_view* __restrict__ views, RcVol g,
                                                                    const int* __restrict__ table, const float* __restrict__ tsdf,
                                                                    const float* __restrict__ weight, const float* __restrict__ rgb) {
  const sp3_tsdf_view& vw = views[blockIdx.z];      // (wave-uniform: the descriptor fields arrive by scalar loads)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (px >= vw.w || py >= vw.h) return;
  raycast_pixel<RGB>(vw, px, py, BrickVol{g, table, tsdf, weight}, rgb);
}

// ------------------------------------------------------------------------------------------------ to_dense
struct Box {
  int lx, ly, lz, sx, sy, sz;
};

__global__ __launch_bounds__(MB) void k_brick_to_dense(BVol g, const int* __restrict__ table, const float* __restrict__ tsdf,
                                                       const float* __restrict__ weight, const float* __restrict__ rgb, Box b, int64_t n,
                                                       float* __restrict__ out_tsdf, float* __restrict__ out_weight, float* __restrict__ out_rgb) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v >= n) return;
  const int i = b.lx + (int)(v % b.sx), j = b.ly + (int)((v / b.sx) % b.sy), k = b.lz + (int)(v / ((int64_t)b.sx * b.sy));
  const int s = table[brick_index(g, i >> 3, j >> 3, k >> 3)];      // (the box lies inside the grid: checked by the host)
  float D = 1.0f, W = 0.0f, cr = 0.f, cg = 0.f, cb = 0.f;
  if (s >= 0) {
    const int64_t q = (int64_t)s * BRK_VOX + (((k & 7) << 6) | ((j & 7) << 3) | (i & 7));
    D = tsdf[q];
    W = weight[q];
    if (rgb != nullptr && out_rgb != nullptr) {
      cr = rgb[3 * q];
      cg = rgb[3 * q + 1];
      cb = rgb[3 * q + 2];
    }
  }
  out_tsdf[v] = D;
  out_weight[v] = W;
  if (out_rgb != nullptr) {
    out_rgb[3 * v] = cr;
    out_rgb[3 * v + 1] = cg;
    out_rgb[3 * v + 2] = cb;
  }
}

// ------------------------------------------------------------------------------------------------ host checks
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// the virtual grid: multiples of 8, bricks + capacity below 2^31 (int32 brick indices, slots, tile tables and `need`)
int check_grid(const char* what, int nx, int ny, int nz, float voxel, int64_t capacity, BVol& g) {
  SP3_CHECK(nx >= 0 && ny >= 0 && nz >= 0, "%s: dims %d x %d x %d must be >= 0", what, nx, ny, nz);
  SP3_CHECK(nx % BRK == 0 && ny % BRK == 0 && nz % BRK == 0, "%s: dims %d x %d x %d must be multiples of 8 (whole bricks)", what, nx, ny, nz);
  SP3_CHECK(nx <= (1 << 20) && ny <= (1 << 20) && nz <= (1 << 20), "%s: dims %d x %d x %d: a side must stay below 2^20 voxels", what, nx, ny, nz);
  const int64_t bxy = (int64_t)(nx / BRK) * (ny / BRK);
  SP3_CHECK(capacity >= 0 && capacity <= 0x7fffffffLL, "%s: capacity %lld out of range", what, (long long)capacity);
  SP3_CHECK(bxy <= 0x7fffffffLL && bxy * (nz / BRK) + capacity + MB <= 0x7fffffffLL,
            "%s: dims %d x %d x %d with capacity %lld over the index limit: bricks + capacity must stay below 2^31 (int32 brick indices and slots)",
            what, nx, ny, nz, (long long)capacity);
  SP3_CHECK(isfinite(voxel) && voxel > 0.f, "%s: voxel %g must be finite and > 0", what, (double)voxel);
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.bx = nx / BRK; g.by = ny / BRK; g.bz = nz / BRK;
  g.voxel = voxel;
  g.ox = g.oy = g.oz = 0.f;
  g.trunc = 0.f;
  return 0;
}

int check_origin(const char* what, const float* origin3, BVol& g) {
  SP3_CHECK(origin3 != nullptr, "%s: null origin", what);
  SP3_CHECK(isfinite(origin3[0]) && isfinite(origin3[1]) && isfinite(origin3[2]), "%s: origin is not finite", what);
  g.ox = origin3[0]; g.oy = origin3[1]; g.oz = origin3[2];
  return 0;
}

}  // namespace

extern "C" int sp3_tsdf_brick_mark(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, const float* c2w_dev, int T, int nx,
                                   int ny, int nz, const float* origin3, float voxel, float band, uint8_t* flags, void* stream) {
  BVol g;
  if (check_grid("sp3_tsdf_brick_mark", nx, ny, nz, voxel, 0, g)) return 1;
  SP3_CHECK(T >= 0 && T <= 65535, "sp3_tsdf_brick_mark: T %d must be in 0 .. 65535", T);
  SP3_CHECK(isfinite(band) && band > 0.f && band <= 8.0f * voxel, "sp3_tsdf_brick_mark: band %g must lie in (0, 8 voxels = %g]", (double)band,
            (double)(8.0f * voxel));
  if (T == 0 || (int64_t)nx * ny * nz == 0) return 0;
  SP3_CHECK(frames_host != nullptr && frames_dev != nullptr && flags != nullptr, "sp3_tsdf_brick_mark: null frames/flags");
  if (check_origin("sp3_tsdf_brick_mark", origin3, g)) return 1;
  int64_t max_pixels = 0;
  if (check_frames("sp3_tsdf_brick_mark", frames_host, T, false, &max_pixels)) return 1;
  for (int f = 0; f < T; ++f)
    SP3_CHECK(frames_host[f].depth == nullptr || c2w_dev != nullptr, "sp3_tsdf_brick_mark: frame %d has depth: the camera-to-world array is required", f);
  const dim3 grid((unsigned)((max_pixels + MB - 1) / MB), (unsigned)T);
  hipLaunchKernelGGL(k_brick_mark, grid, dim3(MB), 0, (hipStream_t)stream, frames_dev, c2w_dev, g, band, flags);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_mark");
  return 0;
}

extern "C" int64_t sp3_tsdf_brick_alloc_ws_bytes(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 16;
  const int64_t nb = (int64_t)(nx / BRK) * (ny / BRK) * (nz / BRK);
  return align16(((nb + MB - 1) / MB + 1) * 4) + 16;
}

extern "C" int sp3_tsdf_brick_alloc(uint8_t* flags, int nx, int ny, int nz, int32_t* table, int32_t* slot_brick, int32_t* count,
                                    int64_t capacity, float* tsdf, float* weight, float* rgb, void* ws, int32_t* counts2, void* stream) {
  BVol g;
  if (check_grid("sp3_tsdf_brick_alloc", nx, ny, nz, 1.0f, capacity, g)) return 1;
  SP3_CHECK(count != nullptr && counts2 != nullptr && ws != nullptr, "sp3_tsdf_brick_alloc: null count/counts/ws");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_tsdf_brick_alloc: ws must be 16-byte aligned");
  const int64_t nb = (int64_t)g.bx * g.by * g.bz;
  SP3_CHECK(nb == 0 || (flags != nullptr && table != nullptr), "sp3_tsdf_brick_alloc: null flags/table");
  SP3_CHECK(capacity == 0 || (slot_brick != nullptr && tsdf != nullptr && weight != nullptr), "sp3_tsdf_brick_alloc: null slot_brick/tsdf/weight");
  hipStream_t st = (hipStream_t)stream;
  const int ntiles = (int)((nb + MB - 1) / MB), per = (ntiles + SCAN_T - 1) / SCAN_T;
  int* tile = (int*)ws;
  int* info = (int*)((char*)ws + align16(((int64_t)ntiles + 1) * 4));
  if (ntiles > 0) hipLaunchKernelGGL(k_brick_new_count, dim3(ntiles), dim3(MB), 0, st, (const uint8_t*)flags, (const int*)table, nb, tile);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, tile, ntiles, per, info, 0, 0);
  if (ntiles > 0) {
    hipLaunchKernelGGL(k_brick_new_scatter, dim3(ntiles), dim3(MB), 0, st, flags, (int*)table, (int*)slot_brick, (const int*)count, (const int*)tile,
                       ntiles, nb, capacity);
    const unsigned ib = (unsigned)(capacity < INIT_BLOCKS ? capacity : INIT_BLOCKS);
    if (ib > 0)
      hipLaunchKernelGGL(k_brick_slot_init, dim3(ib), dim3(MB), 0, st, (const int*)count, (const int*)tile, ntiles, capacity, tsdf, weight, rgb);
  }
  hipLaunchKernelGGL(k_brick_alloc_finish, dim3(1), dim3(64), 0, st, (int*)count, (const int*)tile, ntiles, capacity, (int*)counts2);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_alloc");
  return 0;
}

extern "C" int sp3_tsdf_brick_integrate(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, int nx, int ny, int nz,
                                        const float* origin3, float voxel, float trunc, const int32_t* slot_brick, int n_bricks, float* tsdf,
                                        float* weight, float* rgb, void* stream) {
  BVol g;
  if (check_grid("sp3_tsdf_brick_integrate", nx, ny, nz, voxel, 0, g)) return 1;
  SP3_CHECK(T >= 0, "sp3_tsdf_brick_integrate: T %d must be >= 0", T);
  SP3_CHECK(n_bricks >= 0 && (int64_t)n_bricks <= (int64_t)g.bx * g.by * g.bz, "sp3_tsdf_brick_integrate: n_bricks %d must lie in 0 .. %lld (the bricks of the grid)",
            n_bricks, (long long)((int64_t)g.bx * g.by * g.bz));
  SP3_CHECK(isfinite(trunc) && trunc > 0.f, "sp3_tsdf_brick_integrate: trunc %g must be finite and > 0", (double)trunc);
  if (T == 0 || n_bricks == 0) return 0;
  SP3_CHECK(frames_host != nullptr && frames_dev != nullptr && slot_brick != nullptr && tsdf != nullptr && weight != nullptr,
            "sp3_tsdf_brick_integrate: null frames/slot_brick/tsdf/weight");
  if (check_origin("sp3_tsdf_brick_integrate", origin3, g)) return 1;
  if (check_frames("sp3_tsdf_brick_integrate", frames_host, T, rgb != nullptr, nullptr)) return 1;
  g.trunc = trunc;
  hipStream_t st = (hipStream_t)stream;
  if (rgb != nullptr)
    hipLaunchKernelGGL(k_brick_integrate<true>, dim3((unsigned)n_bricks), dim3(BRK_VOX), 0, st, frames_dev, T, g, (const int*)slot_brick, tsdf, weight, rgb);
  else
    hipLaunchKernelGGL(k_brick_integrate<false>, dim3((unsigned)n_bricks), dim3(BRK_VOX), 0, st, frames_dev, T, g, (const int*)slot_brick, tsdf, weight, rgb);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_integrate");
  return 0;
}

extern "C" int sp3_tsdf_brick_raycast(const sp3_tsdf_view* views_host, const sp3_tsdf_view* views_dev, int T, int nx, int ny, int nz,
                                      const float* origin3, float voxel, const int32_t* table, const float* tsdf, const float* weight,
                                      const float* rgb, float min_weight, float step, void* stream) {
  BVol b;
  if (check_grid("sp3_tsdf_brick_raycast", nx, ny, nz, voxel, 0, b)) return 1;
  SP3_CHECK(T >= 0 && T <= 65535, "sp3_tsdf_brick_raycast: T %d must be in 0 .. 65535", T);
  RcVol g;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.bx = b.bx; g.by = b.by; g.bz = b.bz;
  g.voxel = voxel;
  if (check_march("sp3_tsdf_brick_raycast", min_weight, step, g)) return 1;
  if (T == 0) return 0;
  int wmax, hmax;
  if (check_views("sp3_tsdf_brick_raycast", views_host, views_dev, T, rgb != nullptr, wmax, hmax)) return 1;
  if ((int64_t)nx * ny * nz == 0) return 0;
  SP3_CHECK(table != nullptr, "sp3_tsdf_brick_raycast: null table");
  if (check_origin("sp3_tsdf_brick_raycast", origin3, b)) return 1;
  g.ox = b.ox; g.oy = b.oy; g.oz = b.oz;
  dim3 grid;
  if (view_grid("sp3_tsdf_brick_raycast", wmax, hmax, T, grid)) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (rgb != nullptr)
    hipLaunchKernelGGL(k_brick_raycast<true>, grid, dim3(RC_TILE * RC_TILE), 0, st, views_dev, g, (const int*)table, tsdf, weight, rgb);
  else
    hipLaunchKernelGGL(k_brick_raycast<false>, grid, dim3(RC_TILE * RC_TILE), 0, st, views_dev, g, (const int*)table, tsdf, weight, rgb);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_raycast");
  return 0;
}

extern "C" int sp3_tsdf_brick_to_dense(int nx, int ny, int nz, const int32_t* table, const float* tsdf, const float* weight, const float* rgb,
                                       const int32_t* lo3, const int32_t* size3, float* out_tsdf, float* out_weight, float* out_rgb,
                                       void* stream) {
  BVol g;
  if (check_grid("sp3_tsdf_brick_to_dense", nx, ny, nz, 1.0f, 0, g)) return 1;
  SP3_CHECK(lo3 != nullptr && size3 != nullptr, "sp3_tsdf_brick_to_dense: null box");
  const int dims[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a)
    SP3_CHECK(lo3[a] >= 0 && size3[a] >= 0 && (int64_t)lo3[a] + size3[a] <= dims[a], "sp3_tsdf_brick_to_dense: the box (lo %d, size %d) leaves the grid on axis %d (%d voxels)",
              lo3[a], size3[a], a, dims[a]);
  const int64_t sxy = (int64_t)size3[0] * size3[1];
  SP3_CHECK(sxy <= 0x7fffffffLL / 7 && sxy * size3[2] <= 0x7fffffffLL / 7, "sp3_tsdf_brick_to_dense: a box of %d x %d x %d is over the dense volume's index limit (7 n < 2^31)",
            size3[0], size3[1], size3[2]);
  const int64_t n = sxy * size3[2];
  if (n == 0) return 0;
  SP3_CHECK(table != nullptr && out_tsdf != nullptr && out_weight != nullptr, "sp3_tsdf_brick_to_dense: null table/out");
  SP3_CHECK(out_rgb == nullptr || rgb != nullptr, "sp3_tsdf_brick_to_dense: colours asked of a pool without colours");
  Box b;
  b.lx = lo3[0]; b.ly = lo3[1]; b.lz = lo3[2];
  b.sx = size3[0]; b.sy = size3[1]; b.sz = size3[2];
  hipLaunchKernelGGL(k_brick_to_dense, dim3((unsigned)((n + MB - 1) / MB)), dim3(MB), 0, (hipStream_t)stream, g, (const int*)table, tsdf, weight, rgb, b, n,
                     out_tsdf, out_weight, out_rgb);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_to_dense");
  return 0;
}
