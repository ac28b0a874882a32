// TSDF fusion (include/spann3r_hip.h, "TSDF fusion"; spann3r_amd/fusion.py drives these): a truncated signed distance volume
// integrated from depth maps or world pointmaps, and the welded, indexed triangle mesh of its zero level by marching tetrahedra.
//
// sp3_tsdf_integrate is ONE launch for all frames of a call: a lane owns a voxel, keeps its state in registers and walks the frame
// table in order, so the volume is read once and written once however many frames there are.  The frame descriptors are read
// through a wave-uniform index of a read-only table (scalar loads); a workgroup is a 16 x 4 x 4 brick of voxels, so that the lanes
// of a wave (a 16 x 4 slab of one z) read 64-byte runs of the volume and project to neighbouring pixels.  No atomics, no LDS.
//
// sp3_tsdf_extract is two order-preserving compactions in the multi-launch form of csrc/scan.h (count per 256-element tile, one
// single-workgroup scan, scatter): the surface vertices in (owner voxel, slot) order, then the faces in (cell, tetrahedron, triangle)
// order.  A face finds a vertex by offset[owner] + popcount(mask[owner] below its slot): one byte and one int32 of scratch per voxel.
// The 16 cases of a tetrahedron are generated at compile time from the rule in the header (make_cases, csrc/tets.h); no table is
// copied.
//
// The per-frame rule of a voxel is integrate_voxel (csrc/tsdf.h), shared with the brick volume (csrc/bricks.hip).
//
// Every fp32 operation of the projection, the running average and the interpolation is rounded on its own (no contraction into
// FMAs): the file-level pragma below (csrc/tsdf.h and csrc/tets.h set the same for their own text) is what the compiler honours
// under its default -ffp-contract=fast-honor-pragmas.
#include "common.h"
#include "scan.h"
#include "tets.h"
#include "tsdf.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

#define BRICK_X 16
#define BRICK_Y 4
#define BRICK_Z 4

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

struct Vol {
  int nx, ny, nz;
  float ox, oy, oz, voxel, trunc;
};

// ------------------------------------------------------------------------------------------------ integration
template <bool RGB>
__global__ __launch_bounds__(BRICK_X * BRICK_Y * BRICK_Z) void k_tsdf_integrate(const sp3_tsdf_frame* __restrict__ frames, int T, Vol g,
                                                                               float* __restrict__ tsdf, float* __restrict__ weight,
                                                                               float* __restrict__ rgb) {
  const int i = blockIdx.x * BRICK_X + (threadIdx.x & (BRICK_X - 1));
  const int j = blockIdx.y * BRICK_Y + ((threadIdx.x / BRICK_X) & (BRICK_Y - 1));
  const int k = blockIdx.z * BRICK_Z + threadIdx.x / (BRICK_X * BRICK_Y);
  if (i >= g.nx || j >= g.ny || k >= g.nz) return;
  const int64_t v = ((int64_t)k * g.ny + j) * g.nx + i;
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

// ------------------------------------------------------------------------------------------------ marching tetrahedra
// The Kuhn cut, the edge slots and the 16 cases of a tetrahedron: csrc/tets.h.
struct Grid {
  int nx, ny, nz;
  int64_t n;
  float ox, oy, oz, voxel, min_weight;
};

// the 7-bit mask of the edges voxel v owns that carry a vertex: the other endpoint exists, both are observed, the signs differ
__device__ __forceinline__ unsigned edge_mask(const float* __restrict__ tsdf, const float* __restrict__ weight, const Grid& g, int64_t v) {
  if (v >= g.n) return 0;
  if (!(weight[v] >= g.min_weight)) return 0;
  const int i = (int)(v % g.nx), j = (int)((v / g.nx) % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
  const bool in_a = tsdf[v] < 0.f;
  unsigned m = 0;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int c = SLOT_CODE[s], dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz) continue;
    const int64_t b = v + dx + (int64_t)g.nx * (dy + (int64_t)g.ny * dz);
    if (!(weight[b] >= g.min_weight)) continue;
    if ((tsdf[b] < 0.f) != in_a) m |= 1u << s;
  }
  return m;
}

__global__ __launch_bounds__(MB) void k_tsdf_edge_count(const float* __restrict__ tsdf, const float* __restrict__ weight, Grid g,
                                                        uint8_t* __restrict__ vmask, int* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const unsigned m = edge_mask(tsdf, weight, g, v);
  if (v < g.n) vmask[v] = (uint8_t)m;
  int total;
  block_excl_sum(__popc(m), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_tsdf_vertex_scatter(const float* __restrict__ tsdf, const float* __restrict__ rgb, Grid g,
                                                            const uint8_t* __restrict__ vmask, const int* __restrict__ offsets,
                                                            int* __restrict__ voff, int64_t max_vertices, float* __restrict__ vertices,
                                                            unsigned* __restrict__ rgba) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const unsigned m = v < g.n ? vmask[v] : 0u;
  int total;
  const int excl = block_excl_sum(__popc(m), total);
  if (v >= g.n) return;
  int64_t dst = (int64_t)offsets[blockIdx.x] + excl;
  voff[v] = (int)dst;
  if (m == 0) return;
  const int i = (int)(v % g.nx), j = (int)((v / g.nx) % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
  const float ta = tsdf[v];
  const float ax = g.ox + (float)i * g.voxel, ay = g.oy + (float)j * g.voxel, az = g.oz + (float)k * g.voxel;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    if (!((m >> s) & 1u)) continue;
    if (dst < max_vertices) {
      const int c = SLOT_CODE[s], dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      const int64_t b = v + dx + (int64_t)g.nx * (dy + (int64_t)g.ny * dz);
      const float t = ta / (ta - tsdf[b]);
      const float bx = g.ox + (float)(i + dx) * g.voxel, by = g.oy + (float)(j + dy) * g.voxel, bz = g.oz + (float)(k + dz) * g.voxel;
      vertices[3 * dst] = ax + t * (bx - ax);
      vertices[3 * dst + 1] = ay + t * (by - ay);
      vertices[3 * dst + 2] = az + t * (bz - az);
      if (rgba != nullptr) {
        unsigned word = 0xffffffffu;
        if (rgb != nullptr) {
          word = 255u << 24;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float ca = rgb[3 * v + ch], cb = rgb[3 * b + ch];
            word |= unorm8(ca + t * (cb - ca)) << (8 * ch);
          }
        }
        rgba[dst] = word;
      }
    }
    ++dst;
  }
}

// Cell v (its corner 0 is voxel v): the number of triangles, and with WRITE their indices from row `dst` on.
template <bool WRITE>
__device__ __forceinline__ int cell_faces(const float* __restrict__ tsdf, const float* __restrict__ weight, const Grid& g, int64_t v,
                                          const uint8_t* __restrict__ vmask, const int* __restrict__ voff, int64_t dst, int64_t max_faces,
                                          int* __restrict__ faces) {
  if (v >= g.n) return 0;
  const int i = (int)(v % g.nx), j = (int)((v / g.nx) % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
  if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return 0;
  unsigned inside = 0;
  bool live = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t b = v + (c & 1) + (int64_t)g.nx * (((c >> 1) & 1) + (int64_t)g.ny * (c >> 2));
    live = live && weight[b] >= g.min_weight;
    inside |= (tsdf[b] < 0.f ? 1u : 0u) << c;
  }
  if (!live || inside == 0u || inside == 255u) return 0;
  int n = 0;
  for (int t = 0; t < 6; ++t) {
    unsigned cs = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) cs |= ((inside >> TET[t][m]) & 1u) << m;
    const int nt = CASES.ntri[cs];
    if (WRITE) {
      for (int q = 0; q < nt; ++q) {
        if (dst + n + q >= max_faces) continue;
        for (int x = 0; x < 3; ++x) {
          const int ca = TET[t][CASES.e[cs][q][x][0]], cb = TET[t][CASES.e[cs][q][x][1]];
          const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
          const int64_t owner = v + (lo & 1) + (int64_t)g.nx * (((lo >> 1) & 1) + (int64_t)g.ny * (lo >> 2));
          const int slot = SLOT_OF[hi - lo];
          faces[3 * (dst + n + q) + x] = voff[owner] + __popc((unsigned)vmask[owner] & ((1u << slot) - 1u));
        }
      }
    }
    n += nt;
  }
  return n;
}

__global__ __launch_bounds__(MB) void k_tsdf_face_count(const float* __restrict__ tsdf, const float* __restrict__ weight, Grid g,
                                                        int* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const int n = cell_faces<false>(tsdf, weight, g, v, nullptr, nullptr, 0, 0, nullptr);
  int total;
  block_excl_sum(n, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_tsdf_face_scatter(const float* __restrict__ tsdf, const float* __restrict__ weight, Grid g,
                                                          const uint8_t* __restrict__ vmask, const int* __restrict__ voff,
                                                          const int* __restrict__ offsets, int64_t max_faces, int* __restrict__ faces) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const int n = cell_faces<false>(tsdf, weight, g, v, nullptr, nullptr, 0, 0, nullptr);
  int total;
  const int excl = block_excl_sum(n, total);
  if (n == 0) return;
  cell_faces<true>(tsdf, weight, g, v, vmask, voff, (int64_t)offsets[blockIdx.x] + excl, max_faces, faces);
}

// n = nx ny nz with 7 n < 2^31 (and, for the face counter of the extraction, faces_too: 12 n < 2^31), without overflow on the way
int check_volume(const char* what, int nx, int ny, int nz, float voxel, bool faces_too) {
  SP3_CHECK(nx >= 0 && ny >= 0 && nz >= 0, "%s: dims %d x %d x %d must be >= 0", what, nx, ny, nz);
  const int64_t lim = 0x7fffffffLL / (faces_too ? 12 : 7);
  SP3_CHECK((int64_t)nx * ny <= lim && (int64_t)nx * ny * nz <= lim,
            "%s: dims %d x %d x %d over the index limit: %s nx ny nz must stay below 2^31 (int32 vertex and face indices)", what, nx, ny, nz,
            faces_too ? "12" : "7");
  SP3_CHECK(isfinite(voxel) && voxel > 0.f, "%s: voxel %g must be finite and > 0", what, (double)voxel);
  return 0;
}

}  // namespace

extern "C" int sp3_tsdf_integrate(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, int nx, int ny, int nz,
                                  const float* origin3, float voxel, float trunc, float* tsdf, float* weight, float* rgb, void* stream) {
  if (check_volume("sp3_tsdf_integrate", nx, ny, nz, voxel, false)) return 1;
  SP3_CHECK(T >= 0, "sp3_tsdf_integrate: T %d must be >= 0", T);
  SP3_CHECK(isfinite(trunc) && trunc > 0.f, "sp3_tsdf_integrate: trunc %g must be finite and > 0", (double)trunc);
  if (T == 0 || (int64_t)nx * ny * nz == 0) return 0;
  SP3_CHECK(frames_host != nullptr && frames_dev != nullptr && origin3 != nullptr && tsdf != nullptr && weight != nullptr,
            "sp3_tsdf_integrate: null frames/origin/tsdf/weight");
  SP3_CHECK(isfinite(origin3[0]) && isfinite(origin3[1]) && isfinite(origin3[2]), "sp3_tsdf_integrate: origin is not finite");
  if (check_frames("sp3_tsdf_integrate", frames_host, T, rgb != nullptr, nullptr)) return 1;
  Vol g;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.ox = origin3[0]; g.oy = origin3[1]; g.oz = origin3[2];
  g.voxel = voxel; g.trunc = trunc;
  const dim3 grid((unsigned)((nx + BRICK_X - 1) / BRICK_X), (unsigned)((ny + BRICK_Y - 1) / BRICK_Y), (unsigned)((nz + BRICK_Z - 1) / BRICK_Z));
  SP3_CHECK(grid.y <= 65535u && grid.z <= 65535u, "sp3_tsdf_integrate: dims %d x %d x %d: ny and nz must stay below 2^18", nx, ny, nz);
  hipStream_t st = (hipStream_t)stream;
  if (rgb != nullptr)
    hipLaunchKernelGGL(k_tsdf_integrate<true>, grid, dim3(BRICK_X * BRICK_Y * BRICK_Z), 0, st, frames_dev, T, g, tsdf, weight, rgb);
  else
    hipLaunchKernelGGL(k_tsdf_integrate<false>, grid, dim3(BRICK_X * BRICK_Y * BRICK_Z), 0, st, frames_dev, T, g, tsdf, weight, rgb);
  SP3_LAUNCH_CHECK("sp3_tsdf_integrate");
  return 0;
}

extern "C" int64_t sp3_tsdf_extract_ws_bytes(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || (int64_t)nx * ny > 0x7fffffffLL / 12 || (int64_t)nx * ny * nz > 0x7fffffffLL / 12) return 0;
  const int64_t n = (int64_t)nx * ny * nz, nb = (n + MB - 1) / MB;
  return align16(n) + align16(n * 4) + 2 * align16((nb + 1) * 4);
}

extern "C" int sp3_tsdf_extract(const float* tsdf, const float* weight, const float* rgb, int nx, int ny, int nz, const float* origin3,
                                float voxel, float min_weight, void* ws, int64_t max_vertices, int64_t max_faces, float* vertices,
                                uint32_t* rgba, int32_t* faces, int32_t* counts, void* stream) {
  if (check_volume("sp3_tsdf_extract", nx, ny, nz, voxel, true)) return 1;
  SP3_CHECK(min_weight > 0.f, "sp3_tsdf_extract: min_weight %g must be > 0", (double)min_weight);
  SP3_CHECK(max_vertices >= 0 && max_faces >= 0, "sp3_tsdf_extract: negative capacity");
  const int64_t n = (int64_t)nx * ny * nz;
  if (n == 0) return 0;
  SP3_CHECK(tsdf != nullptr && weight != nullptr && origin3 != nullptr && ws != nullptr && counts != nullptr,
            "sp3_tsdf_extract: null tsdf/weight/origin/ws/counts");
  SP3_CHECK((max_vertices == 0 || vertices != nullptr) && (max_faces == 0 || faces != nullptr), "sp3_tsdf_extract: null vertices/faces");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_tsdf_extract: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  Grid g;
  g.nx = nx; g.ny = ny; g.nz = nz; g.n = n;
  g.ox = origin3[0]; g.oy = origin3[1]; g.oz = origin3[2];
  g.voxel = voxel; g.min_weight = min_weight;
  const int nb = (int)blocks_for(n), per = (nb + SCAN_T - 1) / SCAN_T;
  uint8_t* vmask = (uint8_t*)ws;
  int* voff = (int*)((char*)ws + align16(n));
  int* vtile = (int*)((char*)voff + align16(n * 4));
  int* ftile = (int*)((char*)vtile + align16(((int64_t)nb + 1) * 4));
  hipLaunchKernelGGL(k_tsdf_edge_count, dim3(nb), dim3(MB), 0, st, tsdf, weight, g, vmask, vtile);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, vtile, nb, per, (int*)counts, 0, 0);
  hipLaunchKernelGGL(k_tsdf_vertex_scatter, dim3(nb), dim3(MB), 0, st, tsdf, rgb, g, (const uint8_t*)vmask, (const int*)vtile, voff,
                     max_vertices, vertices, (unsigned*)rgba);
  hipLaunchKernelGGL(k_tsdf_face_count, dim3(nb), dim3(MB), 0, st, tsdf, weight, g, ftile);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, ftile, nb, per, (int*)counts + 1, 0, 0);
  hipLaunchKernelGGL(k_tsdf_face_scatter, dim3(nb), dim3(MB), 0, st, tsdf, weight, g, (const uint8_t*)vmask, (const int*)voff,
                     (const int*)ftile, max_faces, (int*)faces);
  SP3_LAUNCH_CHECK("sp3_tsdf_extract");
  return 0;
}
