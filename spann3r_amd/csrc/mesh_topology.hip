// Mesh topology and smoothing (include/spann3r_hip.h "Mesh topology and smoothing"; spann3r_amd/mesh.py MeshTopology / topology /
// smooth drive these): the table of unique undirected edges of an indexed triangle mesh with their half-edges and classes, the
// vertex adjacency derived from it, and one pass of the uniform-weight Laplacian that Taubin's filter alternates.
//
// Why every step is order-free on this chip:
//  - The two sorts (torch.sort on the host side of the launch boundaries) fix every order there is: an edge's number is the rank of
//    its (lo, hi) among the unique pairs, its half-edges are a run of the sorted keys, a vertex's row is a run of the sorted directed
//    keys.  What the kernels add are functions of a sorted array and of tables an EARLIER launch wrote: head flags, block_rank,
//    k_tile_scan, a scatter to offsets[tile] + rank (scan.h as it is), and binary searches inside a run.
//  - A run may cross any number of 256-element tiles and scan chunks.  No lane walks its run: an element finds its edge as
//    offsets[tile] + (heads of the tile up to and including itself) - 1, which is right whether the head lies in its tile or in an
//    earlier one, and the ends of the run come from edge_first, written by the launch before.
//  - Stores that several lanes aim at one address all carry the same value (the 1 of vertex_boundary and of the referenced flag),
//    and nothing reads them before the next launch.  The counts are integer atomicAdds of wave popcounts.
//  - Launch boundaries are the only hand-offs; no lane waits for another lane's store.
//  - The smoothing pass reads one buffer and writes the other; a lane owns a vertex and adds its neighbours in the row's order, in
//    fp64 with every operation rounded on its own, so the sum has one order whatever the launch shape.
#include "common.h"
#include "scan.h"

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

const int64_t kKeyNone = 0x7fffffffffffffffLL;      // above every real key: lo = hi = 2^31 - 1 is no vertex pair (V < 2^31 - 1)
const int64_t kIndexLimit = 0x7fffffffLL;

enum { INFO_EDGES = 0, INFO_CLASS0 = 1, INFO_USABLE = 5, INFO_UNUSABLE = 6, INFO_REFERENCED = 7, INFO_BOUNDARY_VERTICES = 8 };

__device__ __forceinline__ void count_add(int* counter, bool on) {      // every lane of the wave calls it
  const unsigned long long b = __ballot(on);
  if (b != 0ull && (threadIdx.x & (SP3_WAVE - 1)) == 0) __hip_atomic_fetch_add(counter, __popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t edge_key(int a, int b) {
  const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
  return (((lo << 31) | hi) << 1) | (int64_t)(a > b);
}

// one lane per face: three keys, or three sentinels for a face that is not usable
__global__ __launch_bounds__(MB) void k_edge_keys(const int* __restrict__ faces, int64_t nfaces, int nverts, int64_t* __restrict__ keys,
                                                  int* __restrict__ info) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool in = f < nfaces;
  bool ok = false;
  if (in) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    ok = (unsigned)a < (unsigned)nverts && (unsigned)b < (unsigned)nverts && (unsigned)c < (unsigned)nverts && a != b && b != c && a != c;
    keys[3 * f] = ok ? edge_key(a, b) : kKeyNone;
    keys[3 * f + 1] = ok ? edge_key(b, c) : kKeyNone;
    keys[3 * f + 2] = ok ? edge_key(c, a) : kKeyNone;
  }
  count_add(info + INFO_USABLE, ok);
  count_add(info + INFO_UNUSABLE, in && !ok);
}

// element i of the sorted keys starts a run: a real key whose pair differs from its predecessor's
__device__ __forceinline__ bool run_head(const int64_t* __restrict__ keys, int64_t n, int64_t i) {
  if (i >= n) return false;
  const int64_t k = keys[i];
  return k != kKeyNone && (i == 0 || (k >> 1) != (keys[i - 1] >> 1));
}

__global__ __launch_bounds__(MB) void k_edge_head_count(const int64_t* __restrict__ keys, int64_t n, int* __restrict__ counts) {
  int total;
  block_rank(run_head(keys, n, (int64_t)blockIdx.x * MB + threadIdx.x), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// heads write their pair and where their run starts; the last real element writes where the last run ends (edge_first[E])
__global__ __launch_bounds__(MB) void k_edge_scatter(const int64_t* __restrict__ keys, int64_t n, const int* __restrict__ offsets,
                                                     int* __restrict__ edges, int* __restrict__ edge_first) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool head = run_head(keys, n, i);
  int total;
  const int rank = block_rank(head, total);
  if (i >= n) return;
  const int64_t k = keys[i];
  if (k == kKeyNone) return;
  const int64_t e = (int64_t)offsets[blockIdx.x] + rank + (head ? 1 : 0) - 1;      // the run this element lies in
  if (head) {
    edges[2 * e] = (int)(k >> 32);
    edges[2 * e + 1] = (int)((k >> 1) & 0x7fffffff);
    edge_first[e] = (int)i;
  }
  if (i == n - 1 || keys[i + 1] == kKeyNone) edge_first[e + 1] = (int)(i + 1);
}

// first index in [lo, hi) of the sorted keys whose backward bit is set: the forward entries of a run come first
__device__ __forceinline__ int first_backward(const int64_t* __restrict__ keys, int lo, int hi) {
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (keys[mid] & 1) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// one lane per edge: uses, forward uses, class, the class counts and the flags of its two vertices
__global__ __launch_bounds__(MB) void k_edge_finish(const int64_t* __restrict__ keys, const int* __restrict__ edges, const int* __restrict__ edge_first,
                                                    int* __restrict__ info, int* __restrict__ edge_uses, int* __restrict__ edge_fwd,
                                                    uint8_t* __restrict__ edge_class, uint8_t* __restrict__ vertex_boundary,
                                                    uint8_t* __restrict__ referenced) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool in = e < info[INFO_EDGES];      // (written by the scan, a launch earlier)
  int cls = -1;
  if (in) {
    const int s = edge_first[e], t = edge_first[e + 1];
    const int uses = t - s, fwd = first_backward(keys, s, t) - s;
    cls = uses == 1 ? 0 : uses > 2 ? 3 : fwd == 1 ? 1 : 2;
    edge_uses[e] = uses;
    edge_fwd[e] = fwd;
    edge_class[e] = (uint8_t)cls;
    const int lo = edges[2 * e], hi = edges[2 * e + 1];
    referenced[lo] = 1;
    referenced[hi] = 1;
    if (cls == 0) {
      vertex_boundary[lo] = 1;
      vertex_boundary[hi] = 1;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) count_add(info + INFO_CLASS0 + c, cls == c);
}

// number of entries of the ascending int64 list p[lo, hi) below x
__device__ __forceinline__ int count_below(const int64_t* __restrict__ p, int lo, int hi, int64_t x) {
  const int first = lo;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (p[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo - first;
}

// one lane per sorted element: the half-edges of an edge in ascending h.  The stable sort left them as two ascending lists, forward
// then backward; an element's place is its place in its own list plus the entries of the other list below it.
__global__ __launch_bounds__(MB) void k_half_edges(const int64_t* __restrict__ keys, const int64_t* __restrict__ order, int64_t n,
                                                   const int* __restrict__ offsets, const int* __restrict__ edge_first,
                                                   const int* __restrict__ edge_fwd, int* __restrict__ half_edges) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool head = run_head(keys, n, i);
  int total;
  const int rank = block_rank(head, total);
  if (i >= n || keys[i] == kKeyNone) return;
  const int64_t e = (int64_t)offsets[blockIdx.x] + rank + (head ? 1 : 0) - 1;
  const int s = edge_first[e], t = edge_first[e + 1], b = s + edge_fwd[e];
  const int64_t h = order[i];
  const int dst = i < b ? (int)i + count_below(order, b, t, h) : s + ((int)i - b) + count_below(order, s, b, h);
  half_edges[dst] = (int)h;
}

__global__ __launch_bounds__(MB) void k_vertex_count(const uint8_t* __restrict__ vertex_boundary, const uint8_t* __restrict__ referenced, int nverts,
                                                     int* __restrict__ info) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool in = v < nverts;
  count_add(info + INFO_REFERENCED, in && referenced[v] != 0);
  count_add(info + INFO_BOUNDARY_VERTICES, in && vertex_boundary[v] != 0);
}

__global__ __launch_bounds__(MB) void k_fill_u8(uint8_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < n) p[i] = 0;
}

// one lane per edge: its two directed keys
__global__ __launch_bounds__(MB) void k_adj_keys(const int* __restrict__ edges, int64_t nedges, int64_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (e >= nedges) return;
  const int64_t lo = edges[2 * e], hi = edges[2 * e + 1];
  keys[2 * e] = (lo << 32) | hi;
  keys[2 * e + 1] = (hi << 32) | lo;
}

// lane i: the neighbour of sorted directed key i, and the row start of vertex i (the keys below i << 32)
__global__ __launch_bounds__(MB) void k_adj_rows(const int64_t* __restrict__ keys, int64_t nkeys, int nverts, int* __restrict__ vertex_offsets,
                                                  int* __restrict__ vertex_neighbors) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < nkeys) vertex_neighbors[i] = (int)(keys[i] & 0xffffffffLL);
  if (i <= nverts) vertex_offsets[i] = count_below(keys, 0, (int)nkeys, i << 32);
}

// one lane per vertex: out = fp32(p + c (mean of the row - p)), the row added in its order in fp64
__global__ __launch_bounds__(MB) void k_smooth_pass(const float* __restrict__ pos, int nverts, const int* __restrict__ vertex_offsets,
                                                     const int* __restrict__ vertex_neighbors, const uint8_t* __restrict__ fixed, double c,
                                                     float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v >= nverts) return;
  const float px = pos[3 * v], py = pos[3 * v + 1], pz = pos[3 * v + 2];
  const int s = vertex_offsets[v], t = vertex_offsets[v + 1];
  if (t == s || (fixed != nullptr && fixed[v] != 0)) {
    out[3 * v] = px;
    out[3 * v + 1] = py;
    out[3 * v + 2] = pz;
    return;
  }
  const float* q = pos + 3 * (int64_t)vertex_neighbors[s];
  double sx = (double)q[0], sy = (double)q[1], sz = (double)q[2];
  for (int j = s + 1; j < t; ++j) {
    q = pos + 3 * (int64_t)vertex_neighbors[j];
    sx = sx + (double)q[0];
    sy = sy + (double)q[1];
    sz = sz + (double)q[2];
  }
  const double k = (double)(t - s);
  const double x = (double)px, y = (double)py, z = (double)pz;
  const double mx = sx / k, my = sy / k, mz = sz / k;
  out[3 * v] = (float)(x + c * (mx - x));
  out[3 * v + 1] = (float)(y + c * (my - y));
  out[3 * v + 2] = (float)(z + c * (mz - z));
}

}  // namespace

extern "C" int sp3_mesh_edge_keys(const int32_t* faces, int64_t nfaces, int64_t nverts, int64_t* keys, int32_t* info, void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_edge_keys: nverts %lld must lie in 1 .. 2^31 - 2 (63-bit keys)", (long long)nverts);
  SP3_CHECK(nfaces > 0 && 3 * nfaces < kIndexLimit + 1, "sp3_mesh_edge_keys: nfaces %lld: 3 F must lie in 3 .. 2^31 - 1 (int32 half-edges)",
            (long long)nfaces);
  SP3_CHECK(faces != nullptr && keys != nullptr && info != nullptr, "sp3_mesh_edge_keys: null faces/keys/info");
  hipLaunchKernelGGL(k_edge_keys, dim3(blocks_for(nfaces)), dim3(MB), 0, (hipStream_t)stream, (const int*)faces, nfaces, (int)nverts, keys,
                     (int*)info);
  SP3_LAUNCH_CHECK("sp3_mesh_edge_keys");
  return 0;
}

extern "C" int64_t sp3_mesh_edge_table_ws_bytes(int64_t nkeys, int64_t nverts) {
  if (nkeys <= 0 || nkeys > kIndexLimit || nverts <= 0 || nverts >= kIndexLimit) return 0;
  return align16(((nkeys + MB - 1) / MB + 1) * 4) + align16(nverts);
}

extern "C" int sp3_mesh_edge_table(const int64_t* keys, const int64_t* order, int64_t nkeys, int64_t nverts, void* ws, int32_t* edges,
                                   int32_t* edge_first, int32_t* edge_uses, int32_t* edge_fwd, uint8_t* edge_class, int32_t* half_edges,
                                   uint8_t* vertex_boundary, int32_t* info, void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_edge_table: nverts %lld must lie in 1 .. 2^31 - 2", (long long)nverts);
  SP3_CHECK(nkeys > 0 && nkeys <= kIndexLimit, "sp3_mesh_edge_table: nkeys %lld must lie in 1 .. 2^31 - 1", (long long)nkeys);
  SP3_CHECK(keys != nullptr && order != nullptr && ws != nullptr && edges != nullptr && edge_first != nullptr && edge_uses != nullptr &&
                edge_fwd != nullptr && edge_class != nullptr && half_edges != nullptr && vertex_boundary != nullptr && info != nullptr,
            "sp3_mesh_edge_table: null argument");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_edge_table: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)blocks_for(nkeys), nv = (int)nverts;
  int* offsets = (int*)ws;
  uint8_t* referenced = (uint8_t*)ws + align16(((int64_t)nb + 1) * 4);
  hipLaunchKernelGGL(k_fill_u8, dim3(blocks_for(nverts)), dim3(MB), 0, st, vertex_boundary, nverts);
  hipLaunchKernelGGL(k_fill_u8, dim3(blocks_for(nverts)), dim3(MB), 0, st, referenced, nverts);
  hipLaunchKernelGGL(k_edge_head_count, dim3(nb), dim3(MB), 0, st, keys, nkeys, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info, 0, 0);
  hipLaunchKernelGGL(k_edge_scatter, dim3(nb), dim3(MB), 0, st, keys, nkeys, (const int*)offsets, (int*)edges, (int*)edge_first);
  hipLaunchKernelGGL(k_edge_finish, dim3(nb), dim3(MB), 0, st, keys, (const int*)edges, (const int*)edge_first, (int*)info, (int*)edge_uses,
                     (int*)edge_fwd, edge_class, vertex_boundary, referenced);
  hipLaunchKernelGGL(k_half_edges, dim3(nb), dim3(MB), 0, st, keys, order, nkeys, (const int*)offsets, (const int*)edge_first,
                     (const int*)edge_fwd, (int*)half_edges);
  hipLaunchKernelGGL(k_vertex_count, dim3(blocks_for(nverts)), dim3(MB), 0, st, (const uint8_t*)vertex_boundary, (const uint8_t*)referenced, nv,
                     (int*)info);
  SP3_LAUNCH_CHECK("sp3_mesh_edge_table");
  return 0;
}

extern "C" int sp3_mesh_adjacency_keys(const int32_t* edges, int64_t nedges, int64_t* keys, void* stream) {
  SP3_CHECK(nedges > 0 && 2 * nedges <= kIndexLimit, "sp3_mesh_adjacency_keys: nedges %lld: 2 E must lie in 2 .. 2^31 - 1 (int32 offsets)",
            (long long)nedges);
  SP3_CHECK(edges != nullptr && keys != nullptr, "sp3_mesh_adjacency_keys: null edges/keys");
  hipLaunchKernelGGL(k_adj_keys, dim3(blocks_for(nedges)), dim3(MB), 0, (hipStream_t)stream, (const int*)edges, nedges, keys);
  SP3_LAUNCH_CHECK("sp3_mesh_adjacency_keys");
  return 0;
}

extern "C" int sp3_mesh_adjacency_rows(const int64_t* keys, int64_t nkeys, int64_t nverts, int32_t* vertex_offsets, int32_t* vertex_neighbors,
                                       void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_adjacency_rows: nverts %lld must lie in 1 .. 2^31 - 2", (long long)nverts);
  SP3_CHECK(nkeys > 0 && nkeys <= kIndexLimit, "sp3_mesh_adjacency_rows: nkeys %lld must lie in 1 .. 2^31 - 1", (long long)nkeys);
  SP3_CHECK(keys != nullptr && vertex_offsets != nullptr && vertex_neighbors != nullptr, "sp3_mesh_adjacency_rows: null argument");
  const int64_t lanes = nkeys > nverts + 1 ? nkeys : nverts + 1;
  hipLaunchKernelGGL(k_adj_rows, dim3(blocks_for(lanes)), dim3(MB), 0, (hipStream_t)stream, keys, nkeys, (int)nverts, (int*)vertex_offsets,
                     (int*)vertex_neighbors);
  SP3_LAUNCH_CHECK("sp3_mesh_adjacency_rows");
  return 0;
}

extern "C" int sp3_mesh_smooth_pass(const float* positions, int64_t nverts, const int32_t* vertex_offsets, const int32_t* vertex_neighbors,
                                    const uint8_t* fixed, double factor, float* out, void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_smooth_pass: nverts %lld must lie in 1 .. 2^31 - 2", (long long)nverts);
  SP3_CHECK(positions != nullptr && vertex_offsets != nullptr && out != nullptr, "sp3_mesh_smooth_pass: null positions/vertex_offsets/out");
  SP3_CHECK(positions != out, "sp3_mesh_smooth_pass: a pass never reads what it writes: out must be another buffer");
  hipLaunchKernelGGL(k_smooth_pass, dim3(blocks_for(nverts)), dim3(MB), 0, (hipStream_t)stream, positions, (int)nverts,
                     (const int*)vertex_offsets, (const int*)vertex_neighbors, fixed, factor, out);
  SP3_LAUNCH_CHECK("sp3_mesh_smooth_pass");
  return 0;
}
