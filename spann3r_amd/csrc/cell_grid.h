// The uniform cell grid of the exact searches, shared by csrc/eval.hip (nearest points: sp3_nn_query, sp3_knn_query) and
// csrc/mesh_distance.hip (nearest faces: sp3_mesh_dist_query).  This is the one statement of the rule; include/spann3r_hip.h
// (sp3_nn_grid) describes what the host hands in.  Everything here is per translation unit (anonymous namespace).  The last section
// holds what the query entry points of the three searches over faces (csrc/mesh_distance.hip, csrc/mesh_ray.hip, csrc/mesh_bvh.hip)
// share whatever their structure: the workgroup size, the lane's query index, the size checks and the workspace head.
//   * The items (points, or the (cell, face) references of triangles) are stored sorted by cell id (z * ny + y) * nx + x with a
//     cell-start table, so the cells of one x-row are one contiguous range.
//   * A query walks the cells around its (clamped) home cell by Chebyshev ring r = 0, 1, ...  After ring r every unvisited item
//     lies beyond a wall of the visited block, so the distance from the query to the nearest wall that still has cells behind it
//     is a lower bound for everything unvisited (>= r*h for a query inside the box; sides with no cells behind them do not
//     count, which is what makes it hold for queries outside the box too).  The walk stops when the client's best is within
//     that bound, less a slack that covers the fp32 rounding of the cell assignment, or when the block covers the whole grid.
//   * Queries still open after `max_ring` rings take a slot of a fallback list in the workspace; the client's brute-force
//     kernels serve the listed slots (or every query), the items split into chunks over blockIdx.y.
//   * The bound has one rounding whatever contraction the including file is compiled with: a wall position is one explicit fmaf,
//     and nothing else in cell_axis or ring_bound is a product followed by a sum, so no pragma can fuse or unfuse anything.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int64_t N_MAX = 0x7fffffff;   // indices travel as int32
int check_grid(const sp3_nn_grid* g, const char* what) {
  SP3_CHECK(g != nullptr, "%s: null grid", what);
  SP3_CHECK(g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && (int64_t)g->nx * g->ny * g->nz <= ((int64_t)1 << 24), "%s: grid dims %d x %d x %d", what,
            g->nx, g->ny, g->nz);
  SP3_CHECK(g->h > 0.f && g->inv_h > 0.f && g->slack >= 0.f, "%s: grid h / inv_h / slack must be positive", what);
  return 0;
}

__device__ __forceinline__ int cell_axis(float x, float o, float inv_h, int n) {
  const float t = floorf((x - o) * inv_h);
  return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));   // NaN -> 0: always a valid cell
}

struct Cell { int x, y, z; };
__device__ __forceinline__ Cell cell_of(const sp3_nn_grid& g, float x, float y, float z) {
  return {cell_axis(x, g.ox, g.inv_h, g.nx), cell_axis(y, g.oy, g.inv_h, g.ny), cell_axis(z, g.oz, g.inv_h, g.nz)};
}
__device__ __forceinline__ int cell_id(const sp3_nn_grid& g, int x, int y, int z) { return (z * g.ny + y) * g.nx + x; }

// Lower bound of the distance from q to anything outside the cell block [c - r, c + r]^3 (clipped to the grid), less the slack;
// +inf when the block covers the whole grid.
__device__ __forceinline__ float ring_bound(const sp3_nn_grid& g, float qx, float qy, float qz, Cell c, int r) {
  const auto wall = [&](float o, int i) { return fmaf((float)i, g.h, o); };   // o + i * h, rounded once
  float b = INFINITY;
  if (c.x - r > 0) b = fminf(b, qx - wall(g.ox, c.x - r));
  if (c.x + r < g.nx - 1) b = fminf(b, wall(g.ox, c.x + r + 1) - qx);
  if (c.y - r > 0) b = fminf(b, qy - wall(g.oy, c.y - r));
  if (c.y + r < g.ny - 1) b = fminf(b, wall(g.oy, c.y + r + 1) - qy);
  if (c.z - r > 0) b = fminf(b, qz - wall(g.oz, c.z - r));
  if (c.z + r < g.nz - 1) b = fminf(b, wall(g.oz, c.z + r + 1) - qz);
  return b == INFINITY ? b : (b - g.slack) * 0.999999f;
}

// Visits the cells of Chebyshev ring r around c.  Cells of one x-row are contiguous in the sorted items, so a row that lies
// wholly in the ring is one range; an inner row contributes its two end cells.  scan(first, last) sees item ranges.
template <typename Scan>
__device__ __forceinline__ void visit_ring(const sp3_nn_grid& g, const int* __restrict__ cell_start, Cell c, int r, int& cells, Scan scan) {
  const int z0 = max(c.z - r, 0), z1 = min(c.z + r, g.nz - 1), y0 = max(c.y - r, 0), y1 = min(c.y + r, g.ny - 1);
  const int x0 = max(c.x - r, 0), x1 = min(c.x + r, g.nx - 1);
  for (int z = z0; z <= z1; ++z) {
    for (int y = y0; y <= y1; ++y) {
      const int base = cell_id(g, 0, y, z);
      if (abs(z - c.z) == r || abs(y - c.y) == r) {
        scan(cell_start[base + x0], cell_start[base + x1 + 1]);
        cells += x1 - x0 + 1;
      } else {
        if (c.x - r >= 0) { scan(cell_start[base + c.x - r], cell_start[base + c.x - r + 1]); ++cells; }
        if (c.x + r < g.nx) { scan(cell_start[base + c.x + r], cell_start[base + c.x + r + 1]); ++cells; }
      }
    }
  }
}

// The walk of one query: rings 0..max_ring around its home cell, scan(first, last) on every item range, and after each ring
// settled(b) on the bound b > 0: true when nothing b or farther away can change the answer.  -> false: open after max_ring rings.
template <typename Scan, typename Settled>
__device__ __forceinline__ bool walk_rings(const sp3_nn_grid& g, const int* __restrict__ cell_start, float qx, float qy, float qz, int max_ring,
                                           int& cells, Scan scan, Settled settled) {
  const Cell c = cell_of(g, qx, qy, qz);
  for (int r = 0; r <= max_ring; ++r) {
    visit_ring(g, cell_start, c, r, cells, scan);
    const float b = ring_bound(g, qx, qy, qz, c, r);
    if (b == INFINITY || (b > 0.f && settled(b))) return true;
  }
  return false;
}

// The first 32 bytes of a query workspace (zeroed by the host call): open queries handed to the brute-force stage, cells visited, items seen.
struct GridHead {
  int fb_count, pad[3];
  unsigned long long cells, items;
  // hands the open query qi to the brute-force stage -> its slot, the key of the slot reset
  __device__ __forceinline__ int open_slot(int64_t qi, int* __restrict__ fb_list, unsigned long long* __restrict__ fb_key) {
    const int slot = atomicAdd(&fb_count, 1);
    fb_list[slot] = (int)qi; fb_key[slot] = ~0ull;
    return slot;
  }
  // adds the lanes' counts, summed per wave first; every lane of the block calls it
  __device__ __forceinline__ void count(int cells_seen, int items_seen) {
    unsigned long long c = (unsigned long long)cells_seen, p = (unsigned long long)items_seen;
#pragma unroll
    for (int o = SP3_WAVE / 2; o > 0; o >>= 1) { c += __shfl_xor(c, o); p += __shfl_xor(p, o); }
    if ((threadIdx.x & (SP3_WAVE - 1)) == 0) { atomicAdd(&cells, c); atomicAdd(&items, p); }
  }
};
static_assert(sizeof(GridHead) == 32, "workspace head");

// The queries of a brute-force stage: the first *count entries of the fallback list (both on the device), or every query (list null).
struct Slots {
  const int *list, *count;
  int64_t nq_all;
  __device__ __forceinline__ int64_t size() const { return count ? min((int64_t)*count, nq_all) : nq_all; }
  // the query of a slot below size(); -1 for a list entry that is no query (nothing is then read or written for it)
  __device__ __forceinline__ int64_t query(int64_t slot) const {
    const int64_t qi = list ? (int64_t)list[slot] : slot;
    return qi >= 0 && qi < nq_all ? qi : -1;
  }
};
// Launch shape of a brute-force stage, 256 threads: x = query blocks (the kernels stride over the slots), y = 1..256 chunks of about
// `per_chunk` items, each a multiple of the LDS tile.
struct BruteLaunch { unsigned qblocks, chunks; int64_t chunk; };
inline BruteLaunch size_brute(int64_t nq, int64_t items, int per_chunk, int tile) {
  int64_t chunks = (items + per_chunk - 1) / per_chunk;
  chunks = chunks < 1 ? 1 : chunks > 256 ? 256 : chunks;
  BruteLaunch l;
  l.chunk = ((items + chunks - 1) / chunks + tile - 1) / tile * tile;
  l.chunks = (unsigned)((items + l.chunk - 1) / l.chunk);
  l.qblocks = (unsigned)((nq + 255) / 256 < 1024 ? (nq + 255) / 256 : 1024);
  return l;
}

// ---- what the entry points of the searches over faces (csrc/mesh_distance.hip, csrc/mesh_ray.hip, csrc/mesh_bvh.hip) share
typedef unsigned long long u64;
constexpr int TB = 256;                        // lanes per workgroup of every kernel of those files
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + TB - 1) / TB); }
inline int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

// The query lane i serves, for every one-lane-per-query kernel of the three files (the grid kernels took order[i] unchecked before
// this rule was shared; they now have the range check the tree kernels always had): -1 for a lane past the end and for an entry of
// `order` that is no query (nothing is read or written for it).
__device__ __forceinline__ int64_t query_of(const int64_t* __restrict__ order, int64_t i, int64_t nq) {
  if (i >= nq) return -1;
  const int64_t qi = order ? order[i] : i;
  return (uint64_t)qi < (uint64_t)nq ? qi : -1;
}

// vertex and face counts that travel as int32; the registration of faces in cells (sp3_mesh_tri_cell_count / _fill) takes an empty
// face list, a query needs one face at least
inline bool sizes_ok_or_empty(int64_t nverts, int64_t nfaces) { return nverts >= 0 && nverts < N_MAX && nfaces >= 0 && nfaces < N_MAX; }
inline bool sizes_ok(int64_t nverts, int64_t nfaces) { return sizes_ok_or_empty(nverts, nfaces) && nfaces >= 1; }
inline int check_mesh_sizes(const char* what, int64_t nverts, int64_t nfaces) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "%s: nverts %lld or nfaces %lld out of range (1 face at least; both below 2^31 - 1)", what, (long long)nverts,
            (long long)nfaces);
  return 0;
}
inline int check_query_args(const char* what, int64_t nverts, int64_t nfaces, int64_t nq) {
  if (check_mesh_sizes(what, nverts, nfaces)) return 1;
  SP3_CHECK(nq >= 0 && nq <= N_MAX, "%s: nq = %lld out of range", what, (long long)nq);
  return 0;
}
// the last host step before the first launch of a query: the workspace's alignment, and its head zeroed.  -> 0, or the entry point's return value
inline int begin_query(void* ws, hipStream_t st, const char* what) {
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  if (hipMemsetAsync(ws, 0, sizeof(GridHead), st) != hipSuccess) { sp3_set_error("%s: hipMemsetAsync failed", what); return 2; }
  return 0;
}

}  // namespace
