// Mesh simplification (include/spann3r_hip.h "Mesh simplification"; spann3r_amd/mesh.py cluster_vertices / simplify drive these):
// vertex clustering on a uniform grid.  sp3_mesh_cluster groups the usable vertices by their cell, numbers the clusters by their
// smallest vertex and gives every cluster one representative from INTEGER sums (16-bit fractions of the cell, colour bytes, a count):
// the sums do not depend on the order of the atomics, so the output is the same bits every run.  sp3_mesh_cluster_faces remaps the
// faces to cluster ids, drops the invalid and the collapsed ones and, with dedup, keeps of every group of equal rotated triples the
// face with the lowest index, densely and in original order.
//
// Both groupings use ONE lock-free open-addressing table (table_insert / table_find).  A slot holds an ITEM index (a vertex, a face),
// never a key; the key of a slot is recomputed from the item it holds (VertexKeys: the cell of the vertex, from the caller's
// positions; FaceKeys: the rotated cluster triple, from the remapped-face buffer an EARLIER launch wrote), so any V and C work
// without packing a key into 64 bits.  What keeps it correct and finite on this chip:
//  - a claimed slot never changes its key: it leaves EMPTY through one agent-scope atomicCAS(slot, EMPTY, me), and afterwards only
//    atomicMin with items of the SAME key writes it, so a slot's value only ever decreases, within one key;
//  - a lane inserts only at the first EMPTY slot of its probe sequence (linear from hash(key), wrapping): all lanes of one key walk
//    the same sequence past the same claimed slots of other keys, so one key owns exactly one slot, and that slot ends at the
//    minimum item of the key, whatever the arrival order;
//  - the table holds more slots than items (checked before anything is launched), so every probe ends at a match or at an EMPTY
//    slot; the probe loops are bounded by the table size all the same;
//  - no lane waits for another lane's store.  The L2s of the XCDs are not coherent and a CU's L1 is never refreshed: inside the
//    insert launch a slot is read with agent-scope atomic loads only, and freshness does not matter -- a stale EMPTY only costs a
//    failed CAS, which returns the true value; a stale item is one the slot held earlier, of the same key and not smaller than the
//    current one, so the key comparison is right and the atomicMin that follows (skipped only when the item read is already smaller
//    than the lane's own, which then holds for the current value too) lands on the true value;
//  - the keys are immutable during the launch that hashes them (caller's input, or the output of an earlier launch).
// Launch boundaries are the only other hand-offs, as everywhere among scan.h's users: finding the slot again, the sums, the flags,
// the scans and the scatters run in later launches, where the table is read-only and plain loads are right.
// The result does not depend on the table size or on the hash function: they decide where a key lives, never what is computed.
//
// Every fp32 and fp64 operation of the rule is rounded on its own (no contraction into FMAs): the file-level pragma below is what
// the compiler honours under its default -ffp-contract=fast-honor-pragmas.  The rule is written with plain operators for that
// reason: the __fmul_rn / __fsub_rn forms are inline functions of a header that precedes the pragma, and their results were
// contracted (u - floor(u) became fma(p - o, inv, -floor(u))).
#include "common.h"
#include "scan.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

constexpr int EMPTY = -1;
constexpr int FACE_INVALID = -1, FACE_COLLAPSED = -2;      // first entry of a remapped face that does not survive

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned hash3(int a, int b, int c) {
  unsigned h = (unsigned)a * 0x9E3779B1u ^ (unsigned)b * 0x85EBCA77u ^ (unsigned)c * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h;
}

struct Key3 {
  int x, y, z;
};
__device__ __forceinline__ bool same(const Key3& a, const Key3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// ------------------------------------------------------------------------------------------------ the rule of a vertex
struct Grid {
  float ox, oy, oz, cell, inv;
};

// one axis: u = (p - o) * inv in two rounded operations, i = floor(u), q = the 16-bit fraction of u - i (one rounded subtraction:
// exact unless -0.5 < u < 0, where it can round up to 1; the fraction is capped at 65535 for that case).
__device__ __forceinline__ bool axis_cell(float p, float o, float inv, int& i, unsigned& q) {
  const float u = (p - o) * inv;
  const float fi = floorf(u);
  if (!(fabsf(fi) < 1073741824.0f)) return false;      // NaN, inf or |i| >= 2^30
  i = (int)fi;
  const float r = u - fi;
  const int f = (int)(r * 65536.0f);
  q = (unsigned)min(f, 65535);
  return true;
}

struct Cell {
  Key3 i;
  unsigned qx, qy, qz;
  bool ok;
};
__device__ __forceinline__ Cell cell_of(const float* __restrict__ verts, int64_t v, const Grid& g) {
  Cell c;
  c.i.x = c.i.y = c.i.z = 0;
  c.qx = c.qy = c.qz = 0;
  const bool a = axis_cell(verts[3 * v], g.ox, g.inv, c.i.x, c.qx);
  const bool b = axis_cell(verts[3 * v + 1], g.oy, g.inv, c.i.y, c.qy);
  const bool d = axis_cell(verts[3 * v + 2], g.oz, g.inv, c.i.z, c.qz);
  c.ok = a && b && d;
  return c;
}

struct VertexKeys {      // an item is a USABLE vertex; its key is its cell
  const float* __restrict__ verts;
  Grid g;
  __device__ __forceinline__ Key3 key(int v) const { return cell_of(verts, v, g).i; }
};

struct FaceKeys {      // an item is a surviving face; its key is its cluster triple rotated so that the smallest id comes first
  const int* __restrict__ remapped;
  __device__ __forceinline__ Key3 key(int f) const {
    const int a = remapped[3 * (int64_t)f], b = remapped[3 * (int64_t)f + 1], c = remapped[3 * (int64_t)f + 2];
    if (a < b && a < c) return Key3{a, b, c};
    if (b < c) return Key3{b, c, a};
    return Key3{c, a, b};
  }
};

// ------------------------------------------------------------------------------------------------ the table
template <typename Keys> __device__ __forceinline__ void table_insert(int* table, unsigned mask, const Keys& keys, int me, const Key3& mine) {
  unsigned h = hash3(mine.x, mine.y, mine.z) & mask;
  for (unsigned n = 0; n <= mask; ++n, h = (h + 1) & mask) {
    int g = ld_agent(table + h);
    if (g == EMPTY) {
      int old = EMPTY;
      if (__hip_atomic_compare_exchange_strong(table + h, &old, me, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
      g = old;      // the true value: some lane claimed the slot first
    }
    if (same(keys.key(g), mine)) {
      if (me < g) __hip_atomic_fetch_min(table + h, me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}

// the item the slot of `mine` ended with (the smallest item of that key), in a launch after the inserts
template <typename Keys> __device__ __forceinline__ int table_find(const int* __restrict__ table, unsigned mask, const Keys& keys, int me,
                                                                    const Key3& mine) {
  unsigned h = hash3(mine.x, mine.y, mine.z) & mask;
  for (unsigned n = 0; n <= mask; ++n, h = (h + 1) & mask) {
    const int g = table[h];
    if (g == EMPTY) break;
    if (g == me || same(keys.key(g), mine)) return g;
  }
  return me;      // (not reached: every item was inserted)
}

__global__ __launch_bounds__(MB) void k_ms_fill(int* __restrict__ p, int64_t n, int value, int* __restrict__ info, int ninfo) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < n) p[i] = value;
  if (i < ninfo) info[i] = 0;
}

// ------------------------------------------------------------------------------------------------ vertices
__global__ __launch_bounds__(MB) void k_ms_vertex_insert(VertexKeys keys, int nverts, int* table, unsigned mask) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v >= nverts) return;
  const Cell c = cell_of(keys.verts, v, keys.g);
  if (c.ok) table_insert(table, mask, keys, (int)v, c.i);
}

// vertex_cluster[v] = the leader (smallest vertex) of v's cluster, -1 for an unusable vertex; counts[tile] = its leaders
__global__ __launch_bounds__(MB) void k_ms_vertex_leader(VertexKeys keys, int nverts, const int* __restrict__ table, unsigned mask,
                                                          int* __restrict__ vertex_cluster, int* __restrict__ counts) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  int leader = -1;
  if (v < nverts) {
    const Cell c = cell_of(keys.verts, v, keys.g);
    if (c.ok) leader = table_find(table, mask, keys, (int)v, c.i);
    vertex_cluster[v] = leader;
  }
  int total;
  block_rank(v < nverts && leader == (int)v, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

#define MS_SUMS 8      // per cluster: sum of qx, qy, qz, of the four colour bytes, and the member count

// leader -> dense id (id_of[leader]), id -> leader, and the cluster's sums cleared
__global__ __launch_bounds__(MB) void k_ms_leader_scatter(int nverts, const int* __restrict__ vertex_cluster, const int* __restrict__ offsets,
                                                           int* __restrict__ id_of, int* __restrict__ leader_of,
                                                           unsigned long long* __restrict__ sums) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool lead = v < nverts && vertex_cluster[v] == (int)v;
  int total;
  const int rank = block_rank(lead, total);
  if (!lead) return;
  const int id = offsets[blockIdx.x] + rank;
  id_of[v] = id;
  leader_of[id] = (int)v;
#pragma unroll
  for (int k = 0; k < MS_SUMS; ++k) sums[(int64_t)id * MS_SUMS + k] = 0ull;
}

__device__ __forceinline__ void add64(unsigned long long* p, unsigned long long x) {
  __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// vertex_cluster: leader -> dense id; the vertex's fractions, colour bytes and 1 go to its cluster's integer sums
__global__ __launch_bounds__(MB) void k_ms_vertex_accumulate(VertexKeys keys, const uint32_t* __restrict__ rgba, int nverts,
                                                              const int* __restrict__ id_of, int* __restrict__ vertex_cluster,
                                                              unsigned long long* __restrict__ sums) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v >= nverts) return;
  const int leader = vertex_cluster[v];
  if (leader < 0) return;
  const int id = id_of[leader];
  vertex_cluster[v] = id;
  const Cell c = cell_of(keys.verts, v, keys.g);
  unsigned long long* s = sums + (int64_t)id * MS_SUMS;
  add64(s, c.qx);
  add64(s + 1, c.qy);
  add64(s + 2, c.qz);
  if (rgba != nullptr) {
    const uint32_t p = rgba[v];
    add64(s + 3, p & 255u);
    add64(s + 4, (p >> 8) & 255u);
    add64(s + 5, (p >> 16) & 255u);
    add64(s + 6, p >> 24);
  }
  add64(s + 7, 1ull);
}

// pos = (float)(o + (i + sum_q / n / 65536) * cell) in fp64, every operation rounded on its own
__device__ __forceinline__ float representative(float o, int i, unsigned long long sq, double n, float cell) {
  const double frac = (double)sq / n / 65536.0;
  const double offset = ((double)i + frac) * (double)cell;
  return (float)((double)o + offset);
}

__global__ __launch_bounds__(MB) void k_ms_cluster_finalize(VertexKeys keys, const int* __restrict__ info, const int* __restrict__ leader_of,
                                                             const unsigned long long* __restrict__ sums, int has_rgba,
                                                             float* __restrict__ positions, uint32_t* __restrict__ out_rgba) {
  const int64_t id = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (id >= info[0]) return;
  const Key3 i = keys.key(leader_of[id]);
  const unsigned long long* s = sums + id * MS_SUMS;
  const unsigned long long n = s[7];
  const double dn = (double)n;
  positions[3 * id] = representative(keys.g.ox, i.x, s[0], dn, keys.g.cell);
  positions[3 * id + 1] = representative(keys.g.oy, i.y, s[1], dn, keys.g.cell);
  positions[3 * id + 2] = representative(keys.g.oz, i.z, s[2], dn, keys.g.cell);
  if (has_rgba) {
    uint32_t p = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) p |= (uint32_t)((2ull * s[3 + k] + n) / (2ull * n)) << (8 * k);      // round half up
    out_rgba[id] = p;
  }
}

// ------------------------------------------------------------------------------------------------ faces
// remapped[f] = the cluster triple of a valid face, (-1, ..) for an invalid one, (-2, ..) for a collapsed one; info[1], info[2] count
// the invalid and the collapsed.  An index is dereferenced only after the range check.
__global__ __launch_bounds__(MB) void k_ms_face_remap(const int* __restrict__ faces, int64_t nfaces, const int* __restrict__ vertex_cluster,
                                                       int nverts, int* __restrict__ remapped, int* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  bool invalid = false, collapsed = false;
  if (f < nfaces) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int ca = FACE_INVALID, cb = FACE_INVALID, cc = FACE_INVALID;
    if ((unsigned)a < (unsigned)nverts && (unsigned)b < (unsigned)nverts && (unsigned)c < (unsigned)nverts) {
      ca = vertex_cluster[a];
      cb = vertex_cluster[b];
      cc = vertex_cluster[c];
    }
    invalid = ca < 0 || cb < 0 || cc < 0;
    collapsed = !invalid && (ca == cb || cb == cc || ca == cc);
    remapped[3 * f] = invalid ? FACE_INVALID : collapsed ? FACE_COLLAPSED : ca;
    remapped[3 * f + 1] = cb;
    remapped[3 * f + 2] = cc;
  }
  const unsigned long long bi = __ballot(invalid), bc = __ballot(collapsed);
  if ((threadIdx.x & (SP3_WAVE - 1)) == 0) {
    if (bi != 0ull) __hip_atomic_fetch_add(info + 1, __popcll(bi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bc != 0ull) __hip_atomic_fetch_add(info + 2, __popcll(bc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(MB) void k_ms_face_insert(FaceKeys keys, int64_t nfaces, int* table, unsigned mask) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (f >= nfaces || keys.remapped[3 * f] < 0) return;
  table_insert(table, mask, keys, (int)f, keys.key((int)f));
}

// kept[f]: a surviving face that (with dedup) is the smallest of its key; counts[tile] = the kept; info[3] counts the duplicates
__global__ __launch_bounds__(MB) void k_ms_face_flag(FaceKeys keys, int64_t nfaces, const int* __restrict__ table, unsigned mask, int dedup,
                                                      uint8_t* __restrict__ kept, int* __restrict__ counts, int* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  bool keep = false, dup = false;
  if (f < nfaces) {
    keep = keys.remapped[3 * f] >= 0;
    if (keep && dedup) {
      keep = table_find(table, mask, keys, (int)f, keys.key((int)f)) == (int)f;
      dup = !keep;
    }
    kept[f] = keep;
  }
  const unsigned long long bd = __ballot(dup);
  if (bd != 0ull && (threadIdx.x & (SP3_WAVE - 1)) == 0)
    __hip_atomic_fetch_add(info + 3, __popcll(bd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int total;
  block_rank(keep, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_ms_face_scatter(const int* __restrict__ remapped, const uint8_t* __restrict__ kept, int64_t nfaces,
                                                         const int* __restrict__ offsets, int* __restrict__ out_faces) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool keep = f < nfaces && kept[f] != 0;
  int total;
  const int rank = block_rank(keep, total);
  if (!keep) return;
  const int64_t dst = (int64_t)offsets[blockIdx.x] + rank;
  out_faces[3 * dst] = remapped[3 * f];
  out_faces[3 * dst + 1] = remapped[3 * f + 1];
  out_faces[3 * dst + 2] = remapped[3 * f + 2];
}

const int64_t kIndexLimit = 0x7fffffffLL;      // int32 indices; 256-element tiles keep every grid below 2^23 blocks

inline bool table_fits(int table_log2, int64_t items) { return table_log2 >= 1 && table_log2 <= 31 && ((int64_t)1 << table_log2) > items; }

}  // namespace

extern "C" int64_t sp3_mesh_cluster_ws_bytes(int64_t nverts, int table_log2) {
  if (nverts <= 0 || nverts >= kIndexLimit || !table_fits(table_log2, nverts)) return 0;
  const int64_t nb = (nverts + MB - 1) / MB;
  return align16(((int64_t)4) << table_log2) + 2 * align16(nverts * 4) + align16((nb + 1) * 4) + nverts * MS_SUMS * 8;
}

extern "C" int sp3_mesh_cluster(const float* vertices, const uint32_t* rgba, int64_t nverts, const float* origin3, float cell, int table_log2,
                                void* ws, float* positions, uint32_t* out_rgba, int32_t* vertex_cluster, int32_t* info, void* stream) {
  SP3_CHECK(nverts >= 0 && nverts < kIndexLimit, "sp3_mesh_cluster: nverts %lld out of range (int32 indices: below 2^31 - 1)", (long long)nverts);
  SP3_CHECK(cell > 0.f && cell <= 3.402823466e38f, "sp3_mesh_cluster: cell %g must be positive and finite", (double)cell);
  SP3_CHECK(origin3 != nullptr && info != nullptr, "sp3_mesh_cluster: null origin3/info");
  SP3_CHECK(nverts == 0 || table_fits(table_log2, nverts),
            "sp3_mesh_cluster: table_log2 %d: the table must have 2^1 .. 2^31 slots and more slots than the %lld vertices", table_log2,
            (long long)nverts);
  SP3_CHECK(nverts == 0 || (vertices != nullptr && ws != nullptr && positions != nullptr && vertex_cluster != nullptr),
            "sp3_mesh_cluster: null vertices/ws/positions/vertex_cluster");
  SP3_CHECK((rgba == nullptr) == (out_rgba == nullptr) || nverts == 0, "sp3_mesh_cluster: rgba and out_rgba go together");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_cluster: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (nverts == 0) {
    hipLaunchKernelGGL(k_ms_fill, dim3(1), dim3(MB), 0, st, (int*)info, (int64_t)0, 0, (int*)info, 1);
    SP3_LAUNCH_CHECK("sp3_mesh_cluster");
    return 0;
  }
  const int nv = (int)nverts;
  const int nb = (int)blocks_for(nverts);
  const int64_t slots = (int64_t)1 << table_log2;
  const unsigned mask = (unsigned)(slots - 1);
  int* table = (int*)ws;
  int* id_of = (int*)((char*)table + align16(slots * 4));
  int* leader_of = (int*)((char*)id_of + align16(nverts * 4));
  int* offsets = (int*)((char*)leader_of + align16(nverts * 4));
  unsigned long long* sums = (unsigned long long*)((char*)offsets + align16(((int64_t)nb + 1) * 4));
  VertexKeys keys;
  keys.verts = vertices;
  keys.g = Grid{origin3[0], origin3[1], origin3[2], cell, 1.0f / cell};
  hipLaunchKernelGGL(k_ms_fill, dim3(blocks_for(slots)), dim3(MB), 0, st, table, slots, EMPTY, (int*)info, 1);
  hipLaunchKernelGGL(k_ms_vertex_insert, dim3(nb), dim3(MB), 0, st, keys, nv, table, mask);
  hipLaunchKernelGGL(k_ms_vertex_leader, dim3(nb), dim3(MB), 0, st, keys, nv, (const int*)table, mask, (int*)vertex_cluster, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info, 0, 0);
  hipLaunchKernelGGL(k_ms_leader_scatter, dim3(nb), dim3(MB), 0, st, nv, (const int*)vertex_cluster, (const int*)offsets, id_of, leader_of, sums);
  hipLaunchKernelGGL(k_ms_vertex_accumulate, dim3(nb), dim3(MB), 0, st, keys, rgba, nv, (const int*)id_of, (int*)vertex_cluster, sums);
  hipLaunchKernelGGL(k_ms_cluster_finalize, dim3(nb), dim3(MB), 0, st, keys, (const int*)info, (const int*)leader_of,
                     (const unsigned long long*)sums, rgba != nullptr ? 1 : 0, positions, out_rgba);
  SP3_LAUNCH_CHECK("sp3_mesh_cluster");
  return 0;
}

extern "C" int64_t sp3_mesh_cluster_faces_ws_bytes(int64_t nfaces, int table_log2) {
  if (nfaces <= 0 || nfaces >= kIndexLimit || (table_log2 != 0 && !table_fits(table_log2, nfaces))) return 0;
  const int64_t nb = (nfaces + MB - 1) / MB;
  return (table_log2 != 0 ? align16(((int64_t)4) << table_log2) : 0) + align16(nfaces * 12) + align16(nfaces) + align16((nb + 1) * 4);
}

extern "C" int sp3_mesh_cluster_faces(const int32_t* faces, int64_t nfaces, const int32_t* vertex_cluster, int64_t nverts, int dedup,
                                      int table_log2, void* ws, int32_t* out_faces, int32_t* info, void* stream) {
  SP3_CHECK(nverts >= 0 && nverts < kIndexLimit && nfaces >= 0 && nfaces < kIndexLimit,
            "sp3_mesh_cluster_faces: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)", (long long)nverts,
            (long long)nfaces);
  SP3_CHECK(info != nullptr, "sp3_mesh_cluster_faces: null info");
  SP3_CHECK(!dedup || nfaces == 0 || table_fits(table_log2, nfaces),
            "sp3_mesh_cluster_faces: table_log2 %d: the table must have 2^1 .. 2^31 slots and more slots than the %lld faces", table_log2,
            (long long)nfaces);
  SP3_CHECK(nfaces == 0 || (faces != nullptr && ws != nullptr && out_faces != nullptr && (nverts == 0 || vertex_cluster != nullptr)),
            "sp3_mesh_cluster_faces: null faces/ws/out_faces/vertex_cluster");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_cluster_faces: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (nfaces == 0) {
    hipLaunchKernelGGL(k_ms_fill, dim3(1), dim3(MB), 0, st, (int*)info, (int64_t)0, 0, (int*)info, 4);
    SP3_LAUNCH_CHECK("sp3_mesh_cluster_faces");
    return 0;
  }
  const int nb = (int)blocks_for(nfaces);
  const int64_t slots = dedup ? (int64_t)1 << table_log2 : 0;
  const unsigned mask = (unsigned)(slots - 1);
  int* table = (int*)ws;
  int* remapped = (int*)((char*)table + align16(slots * 4));
  uint8_t* kept = (uint8_t*)remapped + align16(nfaces * 12);
  int* offsets = (int*)(kept + align16(nfaces));
  FaceKeys keys;
  keys.remapped = remapped;
  hipLaunchKernelGGL(k_ms_fill, dim3(blocks_for(slots > 4 ? slots : 4)), dim3(MB), 0, st, table, slots, EMPTY, (int*)info, 4);
  hipLaunchKernelGGL(k_ms_face_remap, dim3(nb), dim3(MB), 0, st, (const int*)faces, nfaces, (const int*)vertex_cluster, (int)nverts, remapped,
                     (int*)info);
  if (dedup) hipLaunchKernelGGL(k_ms_face_insert, dim3(nb), dim3(MB), 0, st, keys, nfaces, table, mask);
  hipLaunchKernelGGL(k_ms_face_flag, dim3(nb), dim3(MB), 0, st, keys, nfaces, (const int*)table, mask, dedup ? 1 : 0, kept, offsets, (int*)info);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info, 0, 0);
  hipLaunchKernelGGL(k_ms_face_scatter, dim3(nb), dim3(MB), 0, st, (const int*)remapped, (const uint8_t*)kept, nfaces, (const int*)offsets,
                     out_faces);
  SP3_LAUNCH_CHECK("sp3_mesh_cluster_faces");
  return 0;
}
