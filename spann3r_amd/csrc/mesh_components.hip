// Mesh components (include/spann3r_hip.h "Mesh components"; spann3r_amd/mesh.py components / filter_components drive these): the
// connected pieces of an indexed triangle mesh by vertex connectivity, numbered by their smallest vertex, with their face and vertex
// counts, and the order-preserving selection of the faces of the components a caller keeps.  Integer work only: every output is a
// function of the graph, whatever the order in which lanes, waves and workgroups run.
//
// Labelling is a lock-free union-find whose root is the smallest index of its tree.  What keeps it correct and finite on this chip:
//  - parent[v] <= v always, and an entry only ever decreases: k_cc_init stores v (its own launch), and after that every write to
//    `parent` is an agent-scope atomicCAS(&parent[hi], hi, lo) with lo < hi or an agent-scope atomicMin with a smaller vertex of the
//    same tree.  So every chain walk strictly descends and ends after at most v steps, a failed CAS restarts from a strictly smaller
//    index, no input makes a lane loop without end, and no lane ever waits for another lane's store.  Trees only ever merge, and a
//    root is linked only under a smaller vertex, so the root of a tree is its smallest vertex.
//  - Invalid faces (an index outside 0..V-1) are dropped before any walk starts: such an index never starts or extends a walk and is
//    never used as an address.
//  - The L2s of the XCDs are not coherent with each other and a CU's L1 is never refreshed by other CUs' stores.  Inside the hooking
//    launch `parent` is therefore read with agent-scope atomic loads only.  The result does not depend on their freshness either: any
//    value a load can return is one the entry held earlier, i.e. the vertex itself or one of its ancestors (smaller, same tree), so a
//    walk over stale values still descends inside the tree; a stale self-pointer only makes the next CAS fail, and the CAS returns
//    the true value.  Launch boundaries are the only other hand-offs, as everywhere among scan.h's users: flatten, the counts and
//    the relabelling run in later launches, where `parent` is read-only and plain loads are right.
//  - The face and vertex counts per root are integer atomicAdds (deterministic).  A typical mesh has nearly all its faces in ONE
//    component, so the adds are aggregated in the wave first: peel by the first active lane's label, ballot the lanes that share it,
//    one add of the popcount -- at most 64 rounds, one round for a wave of one label.
//  - Dense ids: roots with a non-zero face count are flagged, counted per 256-vertex tile, scanned (k_tile_scan) and scattered: the
//    ids ascend with the root, which is the smallest vertex of its component.
#include "common.h"
#include "scan.h"

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's tree as far as this lane can see it, p = a value loaded from parent[v]; every step goes to a smaller index, so at
// most v steps
__device__ __forceinline__ int find_agent(const int* parent, int v, int p) {
  while (p < v) {
    v = p;
    p = ld_agent(parent + v);
  }
  return v;
}

// the same over a `parent` nobody writes in this launch
__device__ __forceinline__ int find_plain(const int* __restrict__ parent, int v) {
  for (int p = parent[v]; p < v; p = parent[v]) v = p;
  return v;
}

// one union of u != v: afterwards they are in one tree.  ru + rv strictly decreases with every failed CAS.
__device__ __forceinline__ void hook(int* parent, int u, int v) {
  const int pu = ld_agent(parent + u), pv = ld_agent(parent + v);
  if (pu == pv) return;      // both hang under one vertex already (u != v, so these are no self-pointers): most hooks of a mesh end here
  int ru = find_agent(parent, u, pu), rv = find_agent(parent, v, pv);
  int linked = -1;
  while (ru != rv) {
    const int hi = max(ru, rv), lo = min(ru, rv);
    int old = hi;      // hi is linked only while it is a root; a failed exchange leaves its true parent in `old`
    if (__hip_atomic_compare_exchange_strong(parent + hi, &old, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      linked = hi;
      break;
    }
    ru = find_agent(parent, hi, old);                    // old < hi: hi's true parent
    rv = lo;
  }
  // shortcut for later walks from u and v: the smaller root is in the tree of both now, below what they pointed to
  const int r = min(ru, rv);
  if (r < pu && u != linked) __hip_atomic_fetch_min(parent + u, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r < pv && v != linked) __hip_atomic_fetch_min(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// counter[label] += the number of lanes of this wave with `on` and that label: one atomic per distinct label of the wave.
// Every lane of the wave calls it.
__device__ __forceinline__ void wave_count(bool on, int label, int* __restrict__ counter) {
  const int lane = threadIdx.x & (SP3_WAVE - 1);
  unsigned long long left = __ballot(on);
  while (left != 0ull) {      // (uniform in the wave; every round retires its leader, so at most 64 rounds)
    const int leader = __ffsll((long long)left) - 1;
    const int l = __shfl(label, leader);
    const unsigned long long same = __ballot(on && label == l) & left;
    if (lane == leader) __hip_atomic_fetch_add(counter + l, __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    left &= ~same;
  }
}

struct Face {
  bool in, ok;      // a face of the list; a valid one
  int a, b, c;
};
__device__ __forceinline__ Face load_face(const int* __restrict__ faces, int64_t nfaces, int nverts) {
  Face f;
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  f.in = i < nfaces;
  f.ok = false;
  f.a = f.b = f.c = 0;
  if (f.in) {
    f.a = faces[3 * i];
    f.b = faces[3 * i + 1];
    f.c = faces[3 * i + 2];
    f.ok = (unsigned)f.a < (unsigned)nverts && (unsigned)f.b < (unsigned)nverts && (unsigned)f.c < (unsigned)nverts;
  }
  return f;
}

__global__ __launch_bounds__(MB) void k_cc_init(int nverts, int* __restrict__ parent, int* __restrict__ nfac, int* __restrict__ nver,
                                                int* __restrict__ info) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v == 0) info[1] = 0;
  if (v >= nverts) return;
  parent[v] = (int)v;
  nfac[v] = 0;
  nver[v] = 0;
}

__global__ __launch_bounds__(MB) void k_cc_hook(const int* __restrict__ faces, int64_t nfaces, int nverts, int* parent, int* __restrict__ info) {
  const Face f = load_face(faces, nfaces, nverts);
  const unsigned long long bad = __ballot(f.in && !f.ok);
  if (bad != 0ull && (threadIdx.x & (SP3_WAVE - 1)) == 0)
    __hip_atomic_fetch_add(info + 1, __popcll(bad), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!f.ok) return;
  if (f.a != f.b) hook(parent, f.a, f.b);
  if (f.a != f.c) hook(parent, f.a, f.c);
}

// label[v] = the root of v; nver[root] counts its vertices
__global__ __launch_bounds__(MB) void k_cc_flatten(const int* __restrict__ parent, int nverts, int* __restrict__ label, int* __restrict__ nver) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool in = v < nverts;
  int r = 0;
  if (in) {
    r = find_plain(parent, (int)v);
    label[v] = r;
  }
  wave_count(in, r, nver);
}

// face_label[f] = the root of a valid face's vertices (-1: invalid); nfac[root] counts its faces
__global__ __launch_bounds__(MB) void k_cc_face_count(const int* __restrict__ faces, int64_t nfaces, int nverts, const int* __restrict__ label,
                                                      int* __restrict__ face_label, int* __restrict__ nfac) {
  const Face f = load_face(faces, nfaces, nverts);
  const int r = f.ok ? label[f.a] : -1;
  if (f.in) face_label[(int64_t)blockIdx.x * MB + threadIdx.x] = r;
  wave_count(f.ok, r, nfac);
}

__device__ __forceinline__ bool is_component_root(const int* __restrict__ label, const int* __restrict__ nfac, int nverts, int64_t v) {
  return v < nverts && label[v] == (int)v && nfac[v] > 0;
}

__global__ __launch_bounds__(MB) void k_cc_root_count(const int* __restrict__ label, const int* __restrict__ nfac, int nverts,
                                                      int* __restrict__ counts) {
  int total;
  block_rank(is_component_root(label, nfac, nverts, (int64_t)blockIdx.x * MB + threadIdx.x), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// root -> dense id (root_id[root]); the counts of the components within the capacity
__global__ __launch_bounds__(MB) void k_cc_root_scatter(const int* __restrict__ label, const int* __restrict__ nfac, const int* __restrict__ nver,
                                                        int nverts, const int* __restrict__ offsets, int64_t max_components,
                                                        int* __restrict__ root_id, int* __restrict__ component_faces,
                                                        int* __restrict__ component_vertices) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool root = is_component_root(label, nfac, nverts, v);
  int total;
  const int rank = block_rank(root, total);
  if (!root) return;
  const int id = offsets[blockIdx.x] + rank;
  root_id[v] = id;
  if (id < max_components) {
    component_faces[id] = nfac[v];
    component_vertices[id] = nver[v];
  }
}

// root labels -> dense ids, in place; a vertex whose tree has no face gets -1.  Lane i takes vertex i and face i.
__global__ __launch_bounds__(MB) void k_cc_relabel(int nverts, int64_t nfaces, const int* __restrict__ nfac, const int* __restrict__ root_id,
                                                   int* __restrict__ vertex_component, int* __restrict__ face_component) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < nverts) {
    const int r = vertex_component[i];
    vertex_component[i] = nfac[r] > 0 ? root_id[r] : -1;
  }
  if (i < nfaces) {
    const int r = face_component[i];
    if (r >= 0) face_component[i] = root_id[r];
  }
}

__global__ __launch_bounds__(MB) void k_cc_fill(int* __restrict__ p, int64_t n, int value) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < n) p[i] = value;
}

// ------------------------------------------------------------------------------------------------ selection
__device__ __forceinline__ bool face_kept(const int* __restrict__ face_component, const uint8_t* __restrict__ keep, int64_t nfaces,
                                          int ncomponents, int64_t i) {
  if (i >= nfaces) return false;
  const int c = face_component[i];
  return (unsigned)c < (unsigned)ncomponents && keep[c] != 0;
}

__global__ __launch_bounds__(MB) void k_cc_select_count(const int* __restrict__ face_component, const uint8_t* __restrict__ keep, int64_t nfaces,
                                                        int ncomponents, int* __restrict__ counts) {
  int total;
  block_rank(face_kept(face_component, keep, nfaces, ncomponents, (int64_t)blockIdx.x * MB + threadIdx.x), total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_cc_select_scatter(const int* __restrict__ faces, const int* __restrict__ face_component,
                                                          const uint8_t* __restrict__ keep, int64_t nfaces, int ncomponents,
                                                          const int* __restrict__ offsets, int* __restrict__ out_faces) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool kept = face_kept(face_component, keep, nfaces, ncomponents, i);
  int total;
  const int rank = block_rank(kept, total);
  if (!kept) return;
  const int64_t dst = (int64_t)offsets[blockIdx.x] + rank;
  out_faces[3 * dst] = faces[3 * i];
  out_faces[3 * dst + 1] = faces[3 * i + 1];
  out_faces[3 * dst + 2] = faces[3 * i + 2];
}

const int64_t kIndexLimit = 0x7fffffffLL;      // int32 indices; 256-element tiles keep every grid below 2^23 blocks

}  // namespace

extern "C" int64_t sp3_mesh_components_ws_bytes(int64_t nverts) {
  if (nverts <= 0 || nverts >= kIndexLimit) return 0;
  const int64_t nb = (nverts + MB - 1) / MB;
  return 4 * align16(nverts * 4) + align16((nb + 1) * 4);
}

extern "C" int sp3_mesh_components(const int32_t* faces, int64_t nfaces, int64_t nverts, void* ws, int64_t max_components,
                                   int32_t* vertex_component, int32_t* face_component, int32_t* component_faces,
                                   int32_t* component_vertices, int32_t* info, void* stream) {
  SP3_CHECK(nverts >= 0 && nverts < kIndexLimit && nfaces >= 0 && nfaces < kIndexLimit,
            "sp3_mesh_components: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)", (long long)nverts,
            (long long)nfaces);
  SP3_CHECK(max_components >= 0, "sp3_mesh_components: max_components %lld must be >= 0", (long long)max_components);
  SP3_CHECK(info != nullptr, "sp3_mesh_components: null info");
  SP3_CHECK(nfaces == 0 || (faces != nullptr && face_component != nullptr), "sp3_mesh_components: null faces/face_component");
  SP3_CHECK(nverts == 0 || (ws != nullptr && vertex_component != nullptr), "sp3_mesh_components: null ws/vertex_component");
  SP3_CHECK(max_components == 0 || nverts == 0 || nfaces == 0 || (component_faces != nullptr && component_vertices != nullptr),
            "sp3_mesh_components: null component_faces/component_vertices with max_components %lld", (long long)max_components);
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_components: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nv = (int)nverts;
  const int nbv = (int)((nverts + MB - 1) / MB);
  if (nverts == 0 || nfaces == 0) {      // no component: there is no face, or (V = 0) every face is invalid
    hipLaunchKernelGGL(k_cc_fill, dim3(1), dim3(MB), 0, st, (int*)info, (int64_t)2, 0);
    if (nfaces > 0) {
      hipLaunchKernelGGL(k_cc_fill, dim3(blocks_for(nfaces)), dim3(MB), 0, st, (int*)face_component, nfaces, -1);
      hipLaunchKernelGGL(k_cc_fill, dim3(1), dim3(MB), 0, st, (int*)info + 1, (int64_t)1, (int)nfaces);
    }
    if (nverts > 0) hipLaunchKernelGGL(k_cc_fill, dim3(nbv), dim3(MB), 0, st, (int*)vertex_component, nverts, -1);
    SP3_LAUNCH_CHECK("sp3_mesh_components");
    return 0;
  }
  int* parent = (int*)ws;
  int* nfac = (int*)((char*)parent + align16(nverts * 4));
  int* nver = (int*)((char*)nfac + align16(nverts * 4));
  int* root_id = (int*)((char*)nver + align16(nverts * 4));
  int* offsets = (int*)((char*)root_id + align16(nverts * 4));
  const unsigned nbf = blocks_for(nfaces);
  hipLaunchKernelGGL(k_cc_init, dim3(nbv), dim3(MB), 0, st, nv, parent, nfac, nver, (int*)info);
  hipLaunchKernelGGL(k_cc_hook, dim3(nbf), dim3(MB), 0, st, (const int*)faces, nfaces, nv, parent, (int*)info);
  hipLaunchKernelGGL(k_cc_flatten, dim3(nbv), dim3(MB), 0, st, (const int*)parent, nv, (int*)vertex_component, nver);
  hipLaunchKernelGGL(k_cc_face_count, dim3(nbf), dim3(MB), 0, st, (const int*)faces, nfaces, nv, (const int*)vertex_component,
                     (int*)face_component, nfac);
  hipLaunchKernelGGL(k_cc_root_count, dim3(nbv), dim3(MB), 0, st, (const int*)vertex_component, (const int*)nfac, nv, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nbv, (nbv + SCAN_T - 1) / SCAN_T, (int*)info, 0, 0);
  hipLaunchKernelGGL(k_cc_root_scatter, dim3(nbv), dim3(MB), 0, st, (const int*)vertex_component, (const int*)nfac, (const int*)nver, nv,
                     (const int*)offsets, max_components, root_id, (int*)component_faces, (int*)component_vertices);
  hipLaunchKernelGGL(k_cc_relabel, dim3(blocks_for(nverts > nfaces ? nverts : nfaces)), dim3(MB), 0, st, nv, nfaces, (const int*)nfac,
                     (const int*)root_id, (int*)vertex_component, (int*)face_component);
  SP3_LAUNCH_CHECK("sp3_mesh_components");
  return 0;
}

extern "C" int64_t sp3_mesh_select_faces_ws_bytes(int64_t nfaces) {
  if (nfaces <= 0 || nfaces >= kIndexLimit) return 0;
  return align16(((nfaces + MB - 1) / MB + 1) * 4);
}

extern "C" int sp3_mesh_select_faces(const int32_t* faces, const int32_t* face_component, int64_t nfaces, const uint8_t* keep,
                                     int64_t ncomponents, void* ws, int32_t* out_faces, int32_t* count, void* stream) {
  SP3_CHECK(nfaces >= 0 && nfaces < kIndexLimit && ncomponents >= 0 && ncomponents < kIndexLimit,
            "sp3_mesh_select_faces: nfaces %lld or ncomponents %lld out of range (both below 2^31 - 1)", (long long)nfaces,
            (long long)ncomponents);
  SP3_CHECK(count != nullptr, "sp3_mesh_select_faces: null count");
  hipStream_t st = (hipStream_t)stream;
  if (nfaces == 0 || ncomponents == 0) {      // nothing can be kept
    hipLaunchKernelGGL(k_cc_fill, dim3(1), dim3(MB), 0, st, (int*)count, (int64_t)1, 0);
    SP3_LAUNCH_CHECK("sp3_mesh_select_faces");
    return 0;
  }
  SP3_CHECK(faces != nullptr && face_component != nullptr && keep != nullptr && ws != nullptr && out_faces != nullptr,
            "sp3_mesh_select_faces: null faces/face_component/keep/ws/out_faces");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_select_faces: ws must be 16-byte aligned");
  const int nb = (int)blocks_for(nfaces);
  int* offsets = (int*)ws;
  hipLaunchKernelGGL(k_cc_select_count, dim3(nb), dim3(MB), 0, st, (const int*)face_component, keep, nfaces, (int)ncomponents, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)count, 0, 0);
  hipLaunchKernelGGL(k_cc_select_scatter, dim3(nb), dim3(MB), 0, st, (const int*)faces, (const int*)face_component, keep, nfaces,
                     (int)ncomponents, (const int*)offsets, (int*)out_faces);
  SP3_LAUNCH_CHECK("sp3_mesh_select_faces");
  return 0;
}
