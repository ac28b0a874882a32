// Mesh boundary loops and hole filling (include/spann3r_hip.h "Mesh boundary loops and hole filling"; spann3r_amd/mesh.py
// BoundaryLoops / boundary_loops / fill_holes drive these): the boundary edges of a MeshTopology in order, their successor links,
// the closed cycles among them as numbered loops with a rank per element and a CSR of members, and a fan (or one triangle) over
// every loop of at most max_edges edges.
//
// Why every step is order-free on this chip:
//  - The edge table fixed every order there is: a boundary element's number is the rank of its edge among the class-0 edges
//    (scan.h as it is: flags per 256-element tile, one single-workgroup scan, a scatter to offsets[tile] + rank), a loop's number is
//    the rank of its head among the heads (the same three steps), a member's place is loop_first[loop] + rank.
//  - The per-vertex counts are integer atomicAdds.  Several lanes may store to vertex_leave[v] at a vertex that more than one
//    element leaves; the slot is only ever read where the counts say one out and one in, where exactly one lane stored.
//  - List ranking is pointer doubling between two buffers: round k reads the state of 2^k-element windows from one and writes
//    the state of 2^(k+1)-element windows to the other, one launch per round.  A round never reads what it writes.
//  - No lane walks a loop, except the one lane per FILLED loop that adds the positions of its row in order (at most max_edges
//    of them): the order of that fp64 sum is the rule.
//  - Launch boundaries are the only hand-offs; no lane waits for another lane's store.
#include "common.h"
#include "scan.h"

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
inline int64_t tiles(int64_t n) { return (n + MB - 1) / MB; }

const int64_t kIndexLimit = 0x7fffffffLL;

enum { INFO_B = 0, INFO_LOOPS = 1, INFO_OPEN = 2, INFO_IRREGULAR = 3, INFO_LONGEST = 4, INFO_MEMBERS = 5 };
enum { FILL_VERTICES = 0, FILL_FACES = 1, FILL_LOOPS = 2 };

__device__ __forceinline__ void count_add(int* counter, bool on) {      // every lane of the wave calls it
  const unsigned long long b = __ballot(on);
  if (b != 0ull && (threadIdx.x & (SP3_WAVE - 1)) == 0) __hip_atomic_fetch_add(counter, __popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(MB) void k_fill_i32(int* __restrict__ p, int64_t n, int v) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < n) p[i] = v;
}

// ------------------------------------------------------------------------------------------------ elements
__global__ __launch_bounds__(MB) void k_class0_count(const uint8_t* __restrict__ edge_class, int64_t nedges, int* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  int total;
  block_rank(e < nedges && edge_class[e] == 0, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// a class-0 edge becomes element offsets[tile] + rank: its half-edge, the two ends in the direction of its face, the counts of its
// ends and the slot of the vertex it leaves.  An element whose half-edge or vertices are out of range (a table that is not this
// mesh's) gets src = dst = -1 and touches no vertex.
__global__ __launch_bounds__(MB) void k_class0_scatter(const uint8_t* __restrict__ edge_class, const int* __restrict__ edge_first,
                                                        const int* __restrict__ half_edges, int64_t nedges, const int* __restrict__ faces,
                                                        int64_t nfaces, int nverts, int nboundary, const int* __restrict__ offsets,
                                                        int* __restrict__ edge, int* __restrict__ half_edge, int* __restrict__ src,
                                                        int* __restrict__ dst, int* __restrict__ vertex_out, int* __restrict__ vertex_in,
                                                        int* __restrict__ vertex_leave) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool on = e < nedges && edge_class[e] == 0;
  int total;
  const int rank = block_rank(on, total);
  if (!on) return;
  const int64_t j = (int64_t)offsets[blockIdx.x] + rank;
  if (j >= nboundary) return;
  const int h = half_edges[edge_first[e]];
  int a = -1, b = -1;
  if (h >= 0 && h / 3 < nfaces) {
    const int f = h / 3, c = h - 3 * f;
    a = faces[3 * (int64_t)f + c];
    b = faces[3 * (int64_t)f + (c + 1) % 3];
    if ((unsigned)a >= (unsigned)nverts || (unsigned)b >= (unsigned)nverts) a = b = -1;
  }
  edge[j] = (int)e;
  half_edge[j] = h;
  src[j] = a;
  dst[j] = b;
  if (a < 0) return;
  __hip_atomic_fetch_add(vertex_out + a, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(vertex_in + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  vertex_leave[a] = (int)j;      // (read only where vertex_out == 1: then this lane is the only one that stored here)
}

// ------------------------------------------------------------------------------------------------ link
__global__ __launch_bounds__(MB) void k_link(const int* __restrict__ dst, int nboundary, const int* __restrict__ vertex_out,
                                             const int* __restrict__ vertex_in, const int* __restrict__ vertex_leave, int nverts,
                                             int* __restrict__ next, int* __restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < nboundary) {
    const int d = dst[i];
    int n = -1;
    if (d >= 0 && vertex_out[d] == 1 && vertex_in[d] == 1) n = vertex_leave[d];
    next[i] = (unsigned)n < (unsigned)nboundary ? n : -1;
  }
  bool irregular = false;
  if (i < nverts) {
    const int o = vertex_out[i], n = vertex_in[i];
    irregular = (o | n) != 0 && !(o == 1 && n == 1);
  }
  count_add(info + INFO_IRREGULAR, irregular);
}

// ------------------------------------------------------------------------------------------------ rank
// state of element j after k rounds: x = the element 2^k steps ahead (-1: the chain ended within them), y = the smallest element
// among j and the (up to) 2^k - 1 after it, z = the steps from j to the FIRST place that element stands at, w = 0
__global__ __launch_bounds__(MB) void k_rank_init(const int* __restrict__ next, int nboundary, int4* __restrict__ state) {
  const int64_t j = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (j < nboundary) state[j] = make_int4(next[j], (int)j, 0, 0);
}

__global__ __launch_bounds__(MB) void k_rank_round(const int4* __restrict__ in, int nboundary, unsigned span, int4* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (j >= nboundary) return;
  int4 s = in[j];
  if (s.x >= 0) {
    const int4 t = in[s.x];
    // t's window starts `span` steps ahead.  On equal labels the window has wrapped around a loop: the first place, ours, stays.
    if (t.y < s.y) {
      s.y = t.y;
      s.z = (int)((unsigned)t.z + span);
    }
    s.x = t.x;
  }
  out[j] = s;
}

// ------------------------------------------------------------------------------------------------ loops
__device__ __forceinline__ bool is_head(const int4* __restrict__ state, int nboundary, int64_t j) {
  if (j >= nboundary) return false;
  const int4 s = state[j];
  return s.x >= 0 && s.y == (int)j;
}

__global__ __launch_bounds__(MB) void k_head_count(const int4* __restrict__ state, int nboundary, int* __restrict__ counts, int* __restrict__ info) {
  const int64_t j = (int64_t)blockIdx.x * MB + threadIdx.x;
  int total;
  block_rank(is_head(state, nboundary, j), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
  count_add(info + INFO_OPEN, j < nboundary && state[j].x < 0);
  if (j == 0) info[INFO_B] = nboundary;
}

// head j of loop l = offsets[tile] + rank: the length of its loop is one more than the steps its successor needs to come back
__global__ __launch_bounds__(MB) void k_head_scatter(const int4* __restrict__ state, const int* __restrict__ next, int nboundary,
                                                     const int* __restrict__ offsets, int* __restrict__ head_loop, int* __restrict__ loop_len, int* __restrict__ info) {
  const int64_t j = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool head = is_head(state, nboundary, j);
  int total;
  const int rank = block_rank(head, total);
  int len = 0;
  if (head) {
    const int l = offsets[blockIdx.x] + rank;
    len = state[next[j]].z + 1;      // (next, not the state's pointer: that one is 2^R steps ahead by now)
    if (l < nboundary) {
      head_loop[j] = l;
      loop_len[l] = len;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o));
  if (len > 0 && (threadIdx.x & (SP3_WAVE - 1)) == 0) __hip_atomic_fetch_max(info + INFO_LONGEST, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lanes 0..L of the capacity grid (L = info[INFO_LOOPS], written by the scan a launch earlier): the tile sums of the lengths
__global__ __launch_bounds__(MB) void k_len_count(const int* __restrict__ loop_len, const int* __restrict__ info, int* __restrict__ counts) {
  const int64_t l = (int64_t)blockIdx.x * MB + threadIdx.x;
  int total;
  block_excl_sum(l < info[INFO_LOOPS] ? loop_len[l] : 0, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_len_scatter(const int* __restrict__ loop_len, const int* __restrict__ info, const int* __restrict__ offsets,
                                                    int* __restrict__ loop_first) {
  const int64_t l = (int64_t)blockIdx.x * MB + threadIdx.x;
  const int nl = info[INFO_LOOPS];
  int total;
  const int below = block_excl_sum(l < nl ? loop_len[l] : 0, total);
  if (l <= nl) loop_first[l] = offsets[blockIdx.x] + below;
}

// one lane per element: its loop (its label's), its rank (the steps the head needs to reach it) and its place in the row
__global__ __launch_bounds__(MB) void k_members(const int4* __restrict__ state, int nboundary, const int* __restrict__ head_loop,
                                                const int* __restrict__ loop_first, int* __restrict__ loop, int* __restrict__ rank,
                                                int* __restrict__ loop_members) {
  const int64_t j = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (j >= nboundary) return;
  const int4 s = state[j];
  int l = -1, r = -1;
  if (s.x >= 0) {
    l = head_loop[s.y];
    const int first = loop_first[l], len = loop_first[l + 1] - first;
    r = s.z == 0 ? 0 : len - s.z;
    const int64_t at = (int64_t)first + r;
    if (r >= 0 && at < nboundary) loop_members[at] = (int)j;
  }
  loop[j] = l;
  rank[j] = r;
}

// ------------------------------------------------------------------------------------------------ fill
__device__ __forceinline__ void fill_sizes(const int* __restrict__ loop_first, int nloops, int max_edges, int64_t l, int& nv, int& nf) {
  nv = nf = 0;
  if (l >= nloops) return;
  const int len = loop_first[l + 1] - loop_first[l];
  if (len > max_edges) return;
  nv = len > 3 ? 1 : 0;
  nf = len > 3 ? len : 1;
}

__global__ __launch_bounds__(MB) void k_fill_count(const int* __restrict__ loop_first, int nloops, int max_edges, int* __restrict__ vcounts,
                                                   int* __restrict__ fcounts, int* __restrict__ info) {
  const int64_t l = (int64_t)blockIdx.x * MB + threadIdx.x;
  int nv, nf, tv, tf;
  fill_sizes(loop_first, nloops, max_edges, l, nv, nf);
  block_rank(nv != 0, tv);
  block_excl_sum(nf, tf);
  if (threadIdx.x == 0) {
    vcounts[blockIdx.x] = tv;
    fcounts[blockIdx.x] = tf;
  }
  count_add(info + FILL_LOOPS, nf != 0);
}

__global__ __launch_bounds__(MB) void k_fill_offsets(const int* __restrict__ loop_first, int nloops, int max_edges, const int* __restrict__ voffsets,
                                                     const int* __restrict__ foffsets, int* __restrict__ vertex_at, int* __restrict__ face_at) {
  const int64_t l = (int64_t)blockIdx.x * MB + threadIdx.x;
  int nv, nf, tv, tf;
  fill_sizes(loop_first, nloops, max_edges, l, nv, nf);
  const int bv = block_rank(nv != 0, tv);
  const int bf = block_excl_sum(nf, tf);
  if (l >= nloops) return;
  vertex_at[l] = nv != 0 ? voffsets[blockIdx.x] + bv : -1;      // -1: no centre (a triangle, or a loop that stays open)
  face_at[l] = nf != 0 ? foffsets[blockIdx.x] + bf : -1;        // -1: not filled
}

// one lane per loop with a centre: the mean of its row's source vertices, added in the row's order in fp64
__global__ __launch_bounds__(MB) void k_fill_centres(const float* __restrict__ pos, const int* __restrict__ rgba, int nverts,
                                                     const int* __restrict__ src, const int* __restrict__ loop_first,
                                                     const int* __restrict__ loop_members, int nloops, const int* __restrict__ vertex_at,
                                                     int nadded, float* __restrict__ out_pos, int* __restrict__ out_rgba) {
#pragma clang fp contract(off)
  const int64_t l = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (l >= nloops) return;
  const int at = vertex_at[l];
  if ((unsigned)at >= (unsigned)nadded) return;
  const int s = loop_first[l], t = loop_first[l + 1];
  const float* q = pos + 3 * (int64_t)src[loop_members[s]];
  double sx = (double)q[0], sy = (double)q[1], sz = (double)q[2];
  for (int i = s + 1; i < t; ++i) {
    q = pos + 3 * (int64_t)src[loop_members[i]];
    sx = sx + (double)q[0];
    sy = sy + (double)q[1];
    sz = sz + (double)q[2];
  }
  const double k = (double)(t - s);
  float* o = out_pos + 3 * ((int64_t)nverts + at);
  o[0] = (float)(sx / k);
  o[1] = (float)(sy / k);
  o[2] = (float)(sz / k);
  if (rgba == nullptr) return;
  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int i = s; i < t; ++i) {
    const unsigned c = (unsigned)rgba[src[loop_members[i]]];
    c0 += c & 255u;
    c1 += (c >> 8) & 255u;
    c2 += (c >> 16) & 255u;
    c3 += c >> 24;
  }
  const unsigned long long n = (unsigned long long)(t - s);
  const unsigned r0 = (unsigned)((2 * c0 + n) / (2 * n)), r1 = (unsigned)((2 * c1 + n) / (2 * n));
  const unsigned r2 = (unsigned)((2 * c2 + n) / (2 * n)), r3 = (unsigned)((2 * c3 + n) / (2 * n));
  out_rgba[(int64_t)nverts + at] = (int)(r0 | (r1 << 8) | (r2 << 16) | (r3 << 24));
}

// one lane per member of a loop: the face of its element, against the walk, to the centre; a 3-loop has one face, written by rank 0
__global__ __launch_bounds__(MB) void k_fill_faces(const int* __restrict__ src, const int* __restrict__ dst, const int* __restrict__ loop,
                                                   const int* __restrict__ rank, const int* __restrict__ loop_first,
                                                   const int* __restrict__ loop_members, int nmembers, int nverts, int64_t nfaces,
                                                   const int* __restrict__ vertex_at, const int* __restrict__ face_at, int nadded,
                                                   int* __restrict__ out_faces) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i >= nmembers) return;
  const int m = loop_members[i], l = loop[m], r = rank[m];
  const int at = face_at[l];
  if (at < 0) return;
  const int first = loop_first[l], len = loop_first[l + 1] - first;
  int a = dst[m], b = src[m], c, slot;
  if (len == 3) {
    if (r != 0) return;
    c = src[loop_members[first + 2]];
    slot = at;
  } else {
    c = nverts + vertex_at[l];
    slot = at + r;
  }
  if ((unsigned)slot >= (unsigned)nadded) return;
  int* o = out_faces + 3 * (nfaces + slot);
  o[0] = a;
  o[1] = b;
  o[2] = c;
}

}  // namespace

extern "C" int64_t sp3_mesh_boundary_elements_ws_bytes(int64_t nedges) {
  if (nedges <= 0 || nedges > kIndexLimit) return 0;
  return align16((tiles(nedges) + 2) * 4);
}

extern "C" int sp3_mesh_boundary_elements(const int32_t* faces, int64_t nfaces, int64_t nverts, const uint8_t* edge_class,
                                          const int32_t* edge_first, const int32_t* half_edges, int64_t nedges, int64_t nboundary, void* ws,
                                          int32_t* edge, int32_t* half_edge, int32_t* src, int32_t* dst, int32_t* vertex_out,
                                          int32_t* vertex_in, int32_t* vertex_leave, void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_boundary_elements: nverts %lld must lie in 1 .. 2^31 - 2", (long long)nverts);
  SP3_CHECK(nfaces > 0 && 3 * nfaces <= kIndexLimit, "sp3_mesh_boundary_elements: nfaces %lld: 3 F must lie in 3 .. 2^31 - 1", (long long)nfaces);
  SP3_CHECK(nedges > 0 && nedges <= 3 * nfaces, "sp3_mesh_boundary_elements: nedges %lld must lie in 1 .. 3 F", (long long)nedges);
  SP3_CHECK(nboundary > 0 && nboundary <= nedges, "sp3_mesh_boundary_elements: nboundary %lld must lie in 1 .. E = %lld", (long long)nboundary,
            (long long)nedges);
  SP3_CHECK(faces != nullptr && edge_class != nullptr && edge_first != nullptr && half_edges != nullptr && ws != nullptr && edge != nullptr &&
                half_edge != nullptr && src != nullptr && dst != nullptr && vertex_out != nullptr && vertex_in != nullptr && vertex_leave != nullptr,
            "sp3_mesh_boundary_elements: null argument");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_boundary_elements: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)tiles(nedges);
  int* offsets = (int*)ws;
  hipLaunchKernelGGL(k_fill_i32, dim3(blocks_for(nverts)), dim3(MB), 0, st, (int*)vertex_out, nverts, 0);
  hipLaunchKernelGGL(k_fill_i32, dim3(blocks_for(nverts)), dim3(MB), 0, st, (int*)vertex_in, nverts, 0);
  hipLaunchKernelGGL(k_fill_i32, dim3(blocks_for(nverts)), dim3(MB), 0, st, (int*)vertex_leave, nverts, -1);
  hipLaunchKernelGGL(k_class0_count, dim3(nb), dim3(MB), 0, st, edge_class, nedges, offsets);
  // (the scan's total goes to a spare word of ws: the host knows B already)
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, offsets + nb + 1, 0, 0);
  hipLaunchKernelGGL(k_class0_scatter, dim3(nb), dim3(MB), 0, st, edge_class, (const int*)edge_first, (const int*)half_edges, nedges,
                     (const int*)faces, nfaces, (int)nverts, (int)nboundary, (const int*)offsets, (int*)edge, (int*)half_edge, (int*)src,
                     (int*)dst, (int*)vertex_out, (int*)vertex_in, (int*)vertex_leave);
  SP3_LAUNCH_CHECK("sp3_mesh_boundary_elements");
  return 0;
}

extern "C" int sp3_mesh_boundary_link(const int32_t* dst, int64_t nboundary, const int32_t* vertex_out, const int32_t* vertex_in,
                                      const int32_t* vertex_leave, int64_t nverts, int32_t* next, int32_t* info, void* stream) {
  SP3_CHECK(nverts > 0 && nverts < kIndexLimit, "sp3_mesh_boundary_link: nverts %lld must lie in 1 .. 2^31 - 2", (long long)nverts);
  SP3_CHECK(nboundary > 0 && nboundary <= kIndexLimit, "sp3_mesh_boundary_link: nboundary %lld must lie in 1 .. 2^31 - 1", (long long)nboundary);
  SP3_CHECK(dst != nullptr && vertex_out != nullptr && vertex_in != nullptr && vertex_leave != nullptr && next != nullptr && info != nullptr,
            "sp3_mesh_boundary_link: null argument");
  const int64_t lanes = nboundary > nverts ? nboundary : nverts;
  hipLaunchKernelGGL(k_link, dim3(blocks_for(lanes)), dim3(MB), 0, (hipStream_t)stream, (const int*)dst, (int)nboundary, (const int*)vertex_out,
                     (const int*)vertex_in, (const int*)vertex_leave, (int)nverts, (int*)next, (int*)info);
  SP3_LAUNCH_CHECK("sp3_mesh_boundary_link");
  return 0;
}

extern "C" int sp3_mesh_boundary_rounds(int64_t nboundary) {      // ceil(log2(max(B, 2)))
  int r = 1;
  while (r < 31 && ((int64_t)1 << r) < nboundary) ++r;
  return r;
}

extern "C" int64_t sp3_mesh_boundary_rank_ws_bytes(int64_t nboundary) {
  if (nboundary <= 0 || nboundary > kIndexLimit) return 0;
  return 16 * nboundary;
}

extern "C" int sp3_mesh_boundary_rank(const int32_t* next, int64_t nboundary, void* ws, int32_t* state, void* stream) {
  SP3_CHECK(nboundary > 0 && nboundary <= kIndexLimit, "sp3_mesh_boundary_rank: nboundary %lld must lie in 1 .. 2^31 - 1", (long long)nboundary);
  SP3_CHECK(next != nullptr && ws != nullptr && state != nullptr, "sp3_mesh_boundary_rank: null next/ws/state");
  SP3_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)state & 15) == 0, "sp3_mesh_boundary_rank: ws and state must be 16-byte aligned");
  SP3_CHECK(ws != (void*)state, "sp3_mesh_boundary_rank: a round never reads what it writes: ws must be another buffer than state");
  hipStream_t st = (hipStream_t)stream;
  const int rounds = sp3_mesh_boundary_rounds(nboundary), nb = (int)nboundary;
  int4* buf[2] = {(int4*)state, (int4*)ws};      // round k writes buf[(rounds - 1 - k) & 1]: the last one lands in state
  hipLaunchKernelGGL(k_rank_init, dim3(blocks_for(nboundary)), dim3(MB), 0, st, (const int*)next, nb, buf[rounds & 1]);
  for (int k = 0; k < rounds; ++k)
    hipLaunchKernelGGL(k_rank_round, dim3(blocks_for(nboundary)), dim3(MB), 0, st, (const int4*)buf[(rounds - k) & 1], nb, 1u << k,
                       buf[(rounds - 1 - k) & 1]);
  SP3_LAUNCH_CHECK("sp3_mesh_boundary_rank");
  return 0;
}

extern "C" int64_t sp3_mesh_boundary_loops_ws_bytes(int64_t nboundary) {
  if (nboundary <= 0 || nboundary > kIndexLimit) return 0;
  // the head counts, the length counts (a capacity of B + 1 loop slots), head_loop [B], loop_len [B]
  return align16((tiles(nboundary) + 2) * 4) + align16((tiles(nboundary + 1) + 2) * 4) + 2 * align16(4 * nboundary);
}

extern "C" int sp3_mesh_boundary_loops(const int32_t* next, const int32_t* state, int64_t nboundary, void* ws, int32_t* loop, int32_t* rank, int32_t* loop_first,
                                       int32_t* loop_members, int32_t* info, void* stream) {
  SP3_CHECK(nboundary > 0 && nboundary <= kIndexLimit, "sp3_mesh_boundary_loops: nboundary %lld must lie in 1 .. 2^31 - 1", (long long)nboundary);
  SP3_CHECK(next != nullptr && state != nullptr && ws != nullptr && loop != nullptr && rank != nullptr && loop_first != nullptr && loop_members != nullptr &&
                info != nullptr,
            "sp3_mesh_boundary_loops: null argument");
  SP3_CHECK(((uintptr_t)ws & 15) == 0 && ((uintptr_t)state & 15) == 0, "sp3_mesh_boundary_loops: ws and state must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)nboundary, nb = (int)tiles(nboundary), nbl = (int)tiles(nboundary + 1);
  char* p = (char*)ws;
  int* hcounts = (int*)p;
  p += align16(((int64_t)nb + 2) * 4);
  int* lcounts = (int*)p;
  p += align16(((int64_t)nbl + 2) * 4);
  int* head_loop = (int*)p;
  p += align16(4 * nboundary);
  int* loop_len = (int*)p;
  const int4* s = (const int4*)state;
  hipLaunchKernelGGL(k_head_count, dim3(nb), dim3(MB), 0, st, s, n, hcounts, (int*)info);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, hcounts, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info + INFO_LOOPS, 0, 0);
  hipLaunchKernelGGL(k_head_scatter, dim3(nb), dim3(MB), 0, st, s, (const int*)next, n, (const int*)hcounts, head_loop, loop_len, (int*)info);
  hipLaunchKernelGGL(k_len_count, dim3(nbl), dim3(MB), 0, st, (const int*)loop_len, (const int*)info, lcounts);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, lcounts, nbl, (nbl + SCAN_T - 1) / SCAN_T, (int*)info + INFO_MEMBERS, 0, 0);
  hipLaunchKernelGGL(k_len_scatter, dim3(nbl), dim3(MB), 0, st, (const int*)loop_len, (const int*)info, (const int*)lcounts, (int*)loop_first);
  hipLaunchKernelGGL(k_members, dim3(nb), dim3(MB), 0, st, s, n, (const int*)head_loop, (const int*)loop_first, (int*)loop, (int*)rank,
                     (int*)loop_members);
  SP3_LAUNCH_CHECK("sp3_mesh_boundary_loops");
  return 0;
}

extern "C" int64_t sp3_mesh_fill_count_ws_bytes(int64_t nloops) {
  if (nloops <= 0 || nloops > kIndexLimit) return 0;
  return 2 * align16((tiles(nloops) + 2) * 4);
}

extern "C" int sp3_mesh_fill_count(const int32_t* loop_first, int64_t nloops, int64_t max_edges, void* ws, int32_t* vertex_at, int32_t* face_at,
                                   int32_t* info, void* stream) {
  SP3_CHECK(nloops > 0 && nloops <= kIndexLimit, "sp3_mesh_fill_count: nloops %lld must lie in 1 .. 2^31 - 1", (long long)nloops);
  SP3_CHECK(max_edges >= 3, "sp3_mesh_fill_count: max_edges %lld must be >= 3 (the shortest loop)", (long long)max_edges);
  SP3_CHECK(loop_first != nullptr && ws != nullptr && vertex_at != nullptr && face_at != nullptr && info != nullptr,
            "sp3_mesh_fill_count: null argument");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_fill_count: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nl = (int)nloops, nb = (int)tiles(nloops), cap = (int)(max_edges < kIndexLimit ? max_edges : kIndexLimit);
  int* vcounts = (int*)ws;
  int* fcounts = (int*)((char*)ws + align16(((int64_t)nb + 2) * 4));
  hipLaunchKernelGGL(k_fill_count, dim3(nb), dim3(MB), 0, st, (const int*)loop_first, nl, cap, vcounts, fcounts, (int*)info);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, vcounts, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info + FILL_VERTICES, 0, 0);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, fcounts, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)info + FILL_FACES, 0, 0);
  hipLaunchKernelGGL(k_fill_offsets, dim3(nb), dim3(MB), 0, st, (const int*)loop_first, nl, cap, (const int*)vcounts, (const int*)fcounts,
                     (int*)vertex_at, (int*)face_at);
  SP3_LAUNCH_CHECK("sp3_mesh_fill_count");
  return 0;
}

extern "C" int sp3_mesh_fill_emit(const float* positions, const int32_t* rgba, int64_t nverts, int64_t nfaces, const int32_t* src,
                                  const int32_t* dst, const int32_t* loop, const int32_t* rank, const int32_t* loop_first,
                                  const int32_t* loop_members, int64_t nloops, int64_t nmembers, const int32_t* vertex_at,
                                  const int32_t* face_at, int64_t vertices_added, int64_t faces_added, float* out_positions,
                                  int32_t* out_rgba, int32_t* out_faces, void* stream) {
  SP3_CHECK(nverts > 0 && nverts + vertices_added < kIndexLimit, "sp3_mesh_fill_emit: %lld + %lld vertices must lie in 1 .. 2^31 - 2",
            (long long)nverts, (long long)vertices_added);
  SP3_CHECK(nfaces > 0 && 3 * (nfaces + faces_added) <= kIndexLimit, "sp3_mesh_fill_emit: %lld + %lld faces: 3 F must stay below 2^31",
            (long long)nfaces, (long long)faces_added);
  SP3_CHECK(nloops > 0 && nloops <= kIndexLimit && nmembers >= 3 * nloops && nmembers <= kIndexLimit,
            "sp3_mesh_fill_emit: %lld loops with %lld members: a loop has at least 3", (long long)nloops, (long long)nmembers);
  SP3_CHECK(vertices_added >= 0 && faces_added > 0 && vertices_added <= nloops && faces_added <= nmembers,
            "sp3_mesh_fill_emit: %lld vertices and %lld faces to add do not fit %lld loops with %lld members", (long long)vertices_added,
            (long long)faces_added, (long long)nloops, (long long)nmembers);
  SP3_CHECK(positions != nullptr && src != nullptr && dst != nullptr && loop != nullptr && rank != nullptr && loop_first != nullptr &&
                loop_members != nullptr && vertex_at != nullptr && face_at != nullptr && out_positions != nullptr && out_faces != nullptr,
            "sp3_mesh_fill_emit: null argument");
  SP3_CHECK((rgba == nullptr) == (out_rgba == nullptr), "sp3_mesh_fill_emit: rgba and out_rgba go together");
  SP3_CHECK(positions != out_positions, "sp3_mesh_fill_emit: out_positions must be another buffer (the caller's vertices are only read)");
  hipStream_t st = (hipStream_t)stream;
  if (vertices_added > 0)
    hipLaunchKernelGGL(k_fill_centres, dim3(blocks_for(nloops)), dim3(MB), 0, st, positions, (const int*)rgba, (int)nverts, (const int*)src,
                       (const int*)loop_first, (const int*)loop_members, (int)nloops, (const int*)vertex_at, (int)vertices_added, out_positions,
                       (int*)out_rgba);
  hipLaunchKernelGGL(k_fill_faces, dim3(blocks_for(nmembers)), dim3(MB), 0, st, (const int*)src, (const int*)dst, (const int*)loop,
                     (const int*)rank, (const int*)loop_first, (const int*)loop_members, (int)nmembers, (int)nverts, nfaces,
                     (const int*)vertex_at, (const int*)face_at, (int)faces_added, (int*)out_faces);
  SP3_LAUNCH_CHECK("sp3_mesh_fill_emit");
  return 0;
}
