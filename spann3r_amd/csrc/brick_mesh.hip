// Marching tetrahedra on the brick pool itself (include/spann3r_hip.h, "Brick mesh extraction"; spann3r_amd/fusion.py
// BrickTSDFVolume.extract_raw drives it): the rule of sp3_tsdf_extract (csrc/fusion.hip, tables in csrc/tets.h) on the densified
// volume of the whole virtual grid, with work and scratch per allocated voxel and no dense intermediate.
//
// The launch structure is sp3_tsdf_extract's -- count, k_tile_scan, scatter (csrc/scan.h), for the vertices and for the faces --
// with a 256-voxel half brick as the scan tile: workgroup 2 slot + h owns the places 256 h .. 256 h + 255 of a slot (its z layers
// 4 h .. 4 h + 3), so a lane's pool index is 256 blockIdx.x + threadIdx.x, the brick's own loads coalesce, and the
// (slot, place, ...) order of the outputs is the (tile, lane, ...) order of the compaction.
//
// Staging: a workgroup reads slot_brick[slot], looks the 7 `+` neighbours up in the table (outside the grid or absent: -1) and
// stages two bits -- observed, inside -- of the 9 x 9 x 5 halo of its half brick in LDS, one byte each (405 bytes): the edge mask,
// a cell's inside byte and its liveness are functions of those bits alone, and both counts of a tile come from the one launch that
// stages it.  (The tsdf values themselves are only needed where a vertex is written; the vertex scatter gathers them, and the
// colours, from the pool: a few loads per surface voxel.)  A wave is an 8 x 8 slab of one z, its byte reads fall into 21 dwords of
// a layer and into the 21 of the next.
//
// Every fp32 operation is rounded on its own (no contraction into FMAs): the file-level pragma below.  Plain vector loads and
// stores; no atomics; no workgroup waits on another.
#include "common.h"
#include "scan.h"
#include "tets.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

#define BRK 8                // voxels per brick side
#define BRK_VOX 512          // voxels per brick
#define HALO_Z 5             // layers a half brick's cells reach
#define HALO_N (9 * 9 * HALO_Z)
#define F_OBS 1u
#define F_IN 2u

struct BGrid {
  int bx, by, bz, n_bricks;
  float ox, oy, oz, voxel, min_weight;
};

inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

struct Halo {
  unsigned char f[HALO_N];      // [zl][y][x]: F_OBS | F_IN of the voxel at local (x, y, 4 h + zl) of the brick, 0 where there is none
  int nslot[8];                 // slot of the brick at offset code c = dx + 2 dy + 4 dz from this one; -1: outside the grid or absent
};

__device__ __forceinline__ int halo_at(int x, int y, int zl) { return (zl * 9 + y) * 9 + x; }

// nslot (threads 0..7) of the brick of `slot`; a __syncthreads() must follow before it is read
__device__ __forceinline__ void stage_neighbours(const BGrid& g, const int* __restrict__ table, int brick, int slot, int* nslot) {
  const int c = threadIdx.x;
  if (c >= 8) return;
  const int I = brick % g.bx + (c & 1), J = (brick / g.bx) % g.by + ((c >> 1) & 1), K = brick / (g.bx * g.by) + (c >> 2);
  int s = slot;
  if (c != 0) {
    s = -1;
    if (I < g.bx && J < g.by && K < g.bz) s = table[((int64_t)K * g.by + J) * g.bx + I];
    if (s >= g.n_bricks) s = -1;      // (a slot the call does not cover has no row of the scratch)
  }
  nslot[c] = s;
}

// pool index of the voxel at local (x, y, z), each in 0..8, of the brick whose neighbours are nslot; -1 where there is no voxel
__device__ __forceinline__ int pool_index(const int* nslot, int x, int y, int z) {
  const int s = nslot[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
  return s < 0 ? -1 : s * BRK_VOX + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7));      // (512 n_bricks < 2^31 / 12)
}

__device__ __forceinline__ unsigned voxel_flags(const BGrid& g, const float* __restrict__ tsdf, const float* __restrict__ weight, int q) {
  if (q < 0) return 0u;
  return (weight[q] >= g.min_weight ? F_OBS : 0u) | (tsdf[q] < 0.f ? F_IN : 0u);
}

// The halo of tile blockIdx.x; every thread of the block calls it.  Lane t is the voxel at local (t & 7, (t >> 3) & 7, 4 h + (t >> 6)).
__device__ __forceinline__ void stage_halo(const BGrid& g, const int* __restrict__ table, const int* __restrict__ slot_brick,
                                           const float* __restrict__ tsdf, const float* __restrict__ weight, Halo& H) {
  const int slot = blockIdx.x >> 1, half = blockIdx.x & 1, t = threadIdx.x;
  stage_neighbours(g, table, slot_brick[slot], slot, H.nslot);
  H.f[halo_at(t & 7, (t >> 3) & 7, t >> 6)] = (unsigned char)voxel_flags(g, tsdf, weight, (int)blockIdx.x * MB + t);
  __syncthreads();
  if (t < HALO_N - MB) {      // the 149 entries beyond the tile's own voxels: the layer above it, then the faces y = 8 and x = 8
    int x, y, zl;
    if (t < 64) {
      x = t & 7; y = t >> 3; zl = 4;
    } else if (t < 104) {
      x = (t - 64) & 7; y = 8; zl = (t - 64) >> 3;
    } else {
      x = 8; y = (t - 104) % 9; zl = (t - 104) / 9;
    }
    H.f[halo_at(x, y, zl)] = (unsigned char)voxel_flags(g, tsdf, weight, pool_index(H.nslot, x, y, 4 * half + zl));
  }
  __syncthreads();
}

// the 7-bit mask of the edges the voxel at (x, y, zl) owns that carry a vertex: both ends observed, exactly one inside
__device__ __forceinline__ unsigned edge_mask(const Halo& H, int x, int y, int zl) {
  const unsigned a = H.f[halo_at(x, y, zl)];
  if (!(a & F_OBS)) return 0u;
  unsigned m = 0;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int c = SLOT_CODE[s];
    const unsigned b = H.f[halo_at(x + (c & 1), y + ((c >> 1) & 1), zl + (c >> 2))];
    if ((b & F_OBS) && ((a ^ b) & F_IN)) m |= 1u << s;
  }
  return m;
}

// the cell whose corner 0 is the voxel at (x, y, zl): its inside byte, or 0 when it is not live (0 and 255 give no face either way)
__device__ __forceinline__ unsigned cell_inside(const Halo& H, int x, int y, int zl) {
  unsigned inside = 0, obs = F_OBS;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const unsigned b = H.f[halo_at(x + (c & 1), y + ((c >> 1) & 1), zl + (c >> 2))];
    obs &= b;
    inside |= ((b >> 1) & 1u) << c;
  }
  return obs ? inside : 0u;
}

__device__ __forceinline__ unsigned tet_case(unsigned inside, int t) {
  unsigned cs = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m) cs |= ((inside >> TET[t][m]) & 1u) << m;
  return cs;
}

__device__ __forceinline__ int cell_face_count(unsigned inside) {
  if (inside == 0u || inside == 255u) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += CASES.ntri[tet_case(inside, t)];
  return n;
}

// ------------------------------------------------------------------------------------------------ count (vertices and faces)
__global__ __launch_bounds__(MB) void k_brick_mesh_count(BGrid g, const int* __restrict__ table, const int* __restrict__ slot_brick,
                                                         const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         uint8_t* __restrict__ vmask, int* __restrict__ vtile, int* __restrict__ ftile) {
  __shared__ Halo H;
  stage_halo(g, table, slot_brick, tsdf, weight, H);
  const int t = threadIdx.x, x = t & 7, y = (t >> 3) & 7, zl = t >> 6;
  const unsigned m = edge_mask(H, x, y, zl);
  vmask[(int64_t)blockIdx.x * MB + t] = (uint8_t)m;
  int total;
  block_excl_sum(__popc(m), total);
  if (t == 0) vtile[blockIdx.x] = total;
  __syncthreads();      // (block_excl_sum's scratch is used again)
  block_excl_sum(cell_face_count(cell_inside(H, x, y, zl)), total);
  if (t == 0) ftile[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------ vertex scatter
__global__ __launch_bounds__(MB) void k_brick_mesh_vertices(BGrid g, const int* __restrict__ table, const int* __restrict__ slot_brick,
                                                            const float* __restrict__ tsdf, const float* __restrict__ rgb,
                                                            const uint8_t* __restrict__ vmask, const int* __restrict__ vtile,
                                                            int* __restrict__ voff, int64_t max_vertices, float* __restrict__ vertices,
                                                            unsigned* __restrict__ rgba) {
  __shared__ int nslot[8];
  const int slot = blockIdx.x >> 1, half = blockIdx.x & 1, t = threadIdx.x;
  const int brick = slot_brick[slot];      // (wave-uniform)
  stage_neighbours(g, table, brick, slot, nslot);
  const int q = (int)blockIdx.x * MB + t;
  const unsigned m = vmask[q];
  int total;
  const int excl = block_excl_sum(__popc(m), total);      // (its barrier also publishes nslot)
  int64_t dst = (int64_t)vtile[blockIdx.x] + excl;
  voff[q] = (int)dst;
  if (m == 0) return;
  const int x = t & 7, y = (t >> 3) & 7, z = 4 * half + (t >> 6);
  const int i = (brick % g.bx) * BRK + x, j = ((brick / g.bx) % g.by) * BRK + y, k = (brick / (g.bx * g.by)) * BRK + z;
  const float ta = tsdf[q];
  const float ax = g.ox + (float)i * g.voxel, ay = g.oy + (float)j * g.voxel, az = g.oz + (float)k * g.voxel;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    if (!((m >> s) & 1u)) continue;
    if (dst < max_vertices) {
      const int c = SLOT_CODE[s], dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      const int b = pool_index(nslot, x + dx, y + dy, z + dz);      // (>= 0: the mask bit says b was observed)
      const float tt = ta / (ta - tsdf[b]);
      const float bx = g.ox + (float)(i + dx) * g.voxel, by = g.oy + (float)(j + dy) * g.voxel, bz = g.oz + (float)(k + dz) * g.voxel;
      vertices[3 * dst] = ax + tt * (bx - ax);
      vertices[3 * dst + 1] = ay + tt * (by - ay);
      vertices[3 * dst + 2] = az + tt * (bz - az);
      if (rgba != nullptr) {
        unsigned word = 0xffffffffu;
        if (rgb != nullptr) {
          word = 255u << 24;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float ca = rgb[3 * (int64_t)q + ch], cb = rgb[3 * (int64_t)b + ch];
            word |= unorm8(ca + tt * (cb - ca)) << (8 * ch);
          }
        }
        rgba[dst] = word;
      }
    }
    ++dst;
  }
}

// ------------------------------------------------------------------------------------------------ face scatter
__global__ __launch_bounds__(MB) void k_brick_mesh_faces(BGrid g, const int* __restrict__ table, const int* __restrict__ slot_brick,
                                                         const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                         const uint8_t* __restrict__ vmask, const int* __restrict__ voff,
                                                         const int* __restrict__ ftile, int64_t max_faces, int* __restrict__ faces) {
  __shared__ Halo H;
  stage_halo(g, table, slot_brick, tsdf, weight, H);
  const int t = threadIdx.x, x = t & 7, y = (t >> 3) & 7, zl = t >> 6, z = 4 * (int)(blockIdx.x & 1) + zl;
  const unsigned inside = cell_inside(H, x, y, zl);
  const int n = cell_face_count(inside);
  int total;
  const int excl = block_excl_sum(n, total);
  if (n == 0) return;
  int64_t dst = (int64_t)ftile[blockIdx.x] + excl;
  for (int tt = 0; tt < 6; ++tt) {
    const unsigned cs = tet_case(inside, tt);
    const int nt = CASES.ntri[cs];
    for (int qd = 0; qd < nt; ++qd, ++dst) {
      if (dst >= max_faces) continue;
      for (int e = 0; e < 3; ++e) {
        const int ca = TET[tt][CASES.e[cs][qd][e][0]], cb = TET[tt][CASES.e[cs][qd][e][1]];
        const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
        const int owner = pool_index(H.nslot, x + (lo & 1), y + ((lo >> 1) & 1), z + (lo >> 2));      // (>= 0: the cell is live)
        const int slot = SLOT_OF[hi - lo];
        faces[3 * dst + e] = voff[owner] + __popc((unsigned)vmask[owner] & ((1u << slot) - 1u));
      }
    }
  }
}

}  // namespace

// the limit of the int32 vertex and face indices: 12 * 512 * n_bricks < 2^31
#define BRICK_MESH_LIMIT (0x7fffffffLL / (12 * BRK_VOX))

extern "C" int64_t sp3_tsdf_brick_extract_ws_bytes(int n_bricks) {
  if (n_bricks <= 0 || n_bricks > BRICK_MESH_LIMIT) return 0;
  const int64_t n = (int64_t)n_bricks * BRK_VOX, nb = 2 * (int64_t)n_bricks;
  return align16(n) + align16(n * 4) + 2 * align16((nb + 1) * 4);
}

extern "C" int sp3_tsdf_brick_extract(int nx, int ny, int nz, const float* origin3, float voxel, const int32_t* table,
                                      const int32_t* slot_brick, int n_bricks, const float* tsdf, const float* weight, const float* rgb,
                                      float min_weight, void* ws, int64_t max_vertices, int64_t max_faces, float* vertices, uint32_t* rgba,
                                      int32_t* faces, int32_t* counts, void* stream) {
  const char* what = "sp3_tsdf_brick_extract";
  SP3_CHECK(nx >= 0 && ny >= 0 && nz >= 0, "%s: dims %d x %d x %d must be >= 0", what, nx, ny, nz);
  SP3_CHECK(nx % BRK == 0 && ny % BRK == 0 && nz % BRK == 0, "%s: dims %d x %d x %d must be multiples of 8 (whole bricks)", what, nx, ny, nz);
  SP3_CHECK(nx <= (1 << 20) && ny <= (1 << 20) && nz <= (1 << 20), "%s: dims %d x %d x %d: a side must stay below 2^20 voxels", what, nx, ny, nz);
  const int64_t bxy = (int64_t)(nx / BRK) * (ny / BRK);
  SP3_CHECK(bxy <= 0x7fffffffLL && bxy * (nz / BRK) + MB <= 0x7fffffffLL,
            "%s: dims %d x %d x %d over the index limit: the bricks of the grid must stay below 2^31 (int32 brick indices)", what, nx, ny, nz);
  SP3_CHECK(n_bricks >= 0, "%s: n_bricks %d must be >= 0", what, n_bricks);
  SP3_CHECK(n_bricks <= BRICK_MESH_LIMIT,
            "%s: n_bricks %d over the index limit: 12 * 512 * n_bricks must stay below 2^31 (int32 vertex and face indices)", what, n_bricks);
  SP3_CHECK((int64_t)n_bricks <= bxy * (nz / BRK), "%s: n_bricks %d must lie in 0 .. %lld (the bricks of the grid)", what, n_bricks,
            (long long)(bxy * (nz / BRK)));
  SP3_CHECK(isfinite(voxel) && voxel > 0.f, "%s: voxel %g must be finite and > 0", what, (double)voxel);
  SP3_CHECK(min_weight > 0.f, "%s: min_weight %g must be > 0", what, (double)min_weight);
  SP3_CHECK(max_vertices >= 0 && max_faces >= 0, "%s: negative capacity", what);
  SP3_CHECK(counts != nullptr, "%s: null counts", what);
  hipStream_t st = (hipStream_t)stream;
  if (n_bricks == 0) {
    SP3_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st) == hipSuccess, "%s: clearing counts failed", what);
    return 0;
  }
  SP3_CHECK(origin3 != nullptr && table != nullptr && slot_brick != nullptr && tsdf != nullptr && weight != nullptr && ws != nullptr,
            "%s: null origin/table/slot_brick/tsdf/weight/ws", what);
  SP3_CHECK(isfinite(origin3[0]) && isfinite(origin3[1]) && isfinite(origin3[2]), "%s: origin is not finite", what);
  SP3_CHECK((max_vertices == 0 || vertices != nullptr) && (max_faces == 0 || faces != nullptr), "%s: null vertices/faces", what);
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "%s: ws must be 16-byte aligned", what);
  BGrid g;
  g.bx = nx / BRK; g.by = ny / BRK; g.bz = nz / BRK; g.n_bricks = n_bricks;
  g.ox = origin3[0]; g.oy = origin3[1]; g.oz = origin3[2];
  g.voxel = voxel; g.min_weight = min_weight;
  const int64_t n = (int64_t)n_bricks * BRK_VOX;
  const int nb = 2 * n_bricks, per = (nb + SCAN_T - 1) / SCAN_T;
  uint8_t* vmask = (uint8_t*)ws;
  int* voff = (int*)((char*)ws + align16(n));
  int* vtile = (int*)((char*)voff + align16(n * 4));
  int* ftile = (int*)((char*)vtile + align16(((int64_t)nb + 1) * 4));
  const int* tb = (const int*)table;
  const int* sb = (const int*)slot_brick;
  hipLaunchKernelGGL(k_brick_mesh_count, dim3(nb), dim3(MB), 0, st, g, tb, sb, tsdf, weight, vmask, vtile, ftile);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, vtile, nb, per, (int*)counts, 0, 0);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, ftile, nb, per, (int*)counts + 1, 0, 0);
  hipLaunchKernelGGL(k_brick_mesh_vertices, dim3(nb), dim3(MB), 0, st, g, tb, sb, tsdf, rgb, (const uint8_t*)vmask, (const int*)vtile, voff,
                     max_vertices, vertices, (unsigned*)rgba);
  hipLaunchKernelGGL(k_brick_mesh_faces, dim3(nb), dim3(MB), 0, st, g, tb, sb, tsdf, weight, (const uint8_t*)vmask, (const int*)voff,
                     (const int*)ftile, max_faces, (int*)faces);
  SP3_LAUNCH_CHECK("sp3_tsdf_brick_extract");
  return 0;
}
