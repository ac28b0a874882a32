// A bounding-volume hierarchy over the faces of a triangle mesh (include/spann3r_hip.h "Mesh BVH"; spann3r_amd/mesh.py TriangleBVH
// and the bvh= keyword of point_mesh_distance / ray_mesh_intersect / render_depth_maps drive these; tests/mesh_bvh_ref.py restates
// the structure and both walks).  It answers the two questions of "Mesh distance" and "Mesh rays" by their own rules -- the faces
// of a leaf are evaluated by the functions of csrc/tri_dist.h and csrc/tri_ray.h, the ones the grid and the brute-force kernels
// call -- so the results are theirs bit for bit; only which faces are looked at differs.
//
//   * The tree is implicit, complete and wide: the usable faces in the order of their Morton keys (the host sorts), LEAF of them per
//     leaf node, ARITY nodes of a level per node of the next, up to one root.  No child pointers: node k of level l is found by
//     index arithmetic and a table of level offsets, and it exists iff k is below the level's size -- decided from counts, never from
//     box values.  A node's box is the exact fp32 min / max of the vertices below it.
//   * The build is one launch for the leaf level and one per level above it; a launch boundary is the only hand-off.  No atomics,
//     no counters, no flags, nothing polls, nothing waits on another lane's store.
//   * A query is one lane and a depth-first walk.  Its stack lives in LDS, laid out [entry][lane] and sized by the host from the
//     level count: a popped node pushes at most ARITY children of the level below, so at most (ARITY - 1) (levels - 1) + 1 entries
//     are ever held.  An entry is 4 bytes: the node's index within its level under a marker bit whose position gives the level.
//     Every node is pushed at most once, so the walk ends.
//   * A node is skipped when its bound says that no face below it can win or tie: the bound is tested when the node is pushed and
//     again when it is popped (the best has usually improved in between), and children are taken nearest first.
//   * Indices read from `order`, `faces` and `q_order` are range-checked before use; the stack never grows past the size the host gave it.
//   * The kernels that serve rays are the two front ends of csrc/ray_kernels.h (which csrc/mesh_ray.hip instantiates with the grid's
//     walk) with the TreeWalker of this file; the distance kernel stays here, since unlike the grid's it has no fallback.  The lane's
//     query index (query_of), the size checks and the workspace head (begin_query) are csrc/cell_grid.h's; the checks of ray
//     arguments and of the table of views are csrc/ray_kernels.h's.  Nothing here sweeps every face: the two order-free passes of
//     the brute-force kernels live in csrc/face_sweep.h.
//   * "Mesh visibility" (sp3_mesh_bvh_ray_occluded, sp3_mesh_bvh_point_views) asks the ray walk whether ANY face is a hit:
//     walk_ray<true> drops best to -inf at the first accepted one, which ends the walk through the tests it already makes.
#include "cell_grid.h"
#include "ray_kernels.h"
#include "tri_dist.h"

#pragma clang fp contract(off)

namespace {

constexpr int LEAF = 4;                        // faces per leaf node
constexpr int ARITY = 4;                       // children per node
constexpr int MAX_LEVELS = SP3_BVH_MAX_LEVELS;

constexpr int log2_of(int x) { return x <= 1 ? 0 : 1 + log2_of(x / 2); }
constexpr int LEAF_BITS = log2_of(LEAF), ARITY_BITS = log2_of(ARITY);
static_assert((1 << LEAF_BITS) == LEAF && (1 << ARITY_BITS) == ARITY && LEAF >= 2 && ARITY >= 2, "LEAF and ARITY are powers of two");
// A stack entry: the node's index within its level under a marker bit at MARK_BIT(level).  F < 2^31 faces make at most
// 2^(31 - LEAF_BITS) leaves, so level l holds at most level_cap(l) = max(2^(31 - LEAF_BITS - ARITY_BITS l), 1) nodes and its indices
// stay below the marker; the marker of the tallest tree's root (level MAX_LEVELS - 1, index 0) is bit 0 at LEAF = ARITY = 4.
constexpr int TOP_BIT = 32 - LEAF_BITS;
constexpr int mark_bit(int level) { return TOP_BIT - ARITY_BITS * level; }
constexpr int64_t level_cap(int level) { return 31 - LEAF_BITS - ARITY_BITS * level > 0 ? (int64_t)1 << (31 - LEAF_BITS - ARITY_BITS * level) : 1; }
constexpr unsigned entry_bits(int level, int k) { return (1u << mark_bit(level)) | (unsigned)k; }
constexpr bool entries_fit(int level) {      // every level up to this one: the marker is a bit of the word and lies above every index
  return level < 0 || (mark_bit(level) >= 0 && mark_bit(level) <= 31 && level_cap(level) <= ((int64_t)1 << mark_bit(level)) && entries_fit(level - 1));
}
static_assert((31 - LEAF_BITS + ARITY_BITS - 1) / ARITY_BITS + 1 <= MAX_LEVELS, "the level table holds the tallest tree");
static_assert(level_cap(MAX_LEVELS - 1) == 1, "the last level of the table can only be a root");
static_assert(entries_fit(MAX_LEVELS - 1), "every level of the table has a marker bit above its indices");
static_assert(entry_bits(MAX_LEVELS - 1, 0) != 0u && entry_bits(0, (int)(level_cap(0) - 1)) < (1u << TOP_BIT) * 2u, "an entry is a non-zero 32-bit word");

// ------------------------------------------------------------------------------------------------ keys
// 21 bits -> every third bit of 63
__device__ __forceinline__ unsigned long long spread3(unsigned x) {
  unsigned long long v = x & 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

constexpr long long KEY_NONE = 0x7fffffffffffffffll;      // 63 ones: an item that is not usable; a usable one stays below it

struct KeyBox { float lo[3], scale[3]; };                 // scale = 2^21 / extent, 0 for an axis of no extent

// One lane per item: a face (faces != null: the centre 0.5 min + 0.5 max of its fp32 box) or a point (faces == null).
__global__ __launch_bounds__(TB) void k_bvh_keys(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t n, KeyBox kb,
                                                  long long* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  float c[3];
  bool ok;
  if (faces != nullptr) {
    float v[9];
    ok = load_face(verts, nverts, faces, i, v) && has_area(v);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
      c[k] = 0.5f * mn + 0.5f * mx;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = verts[3 * i + k];
    ok = fabsf(c[0]) <= 3.4028234e38f && fabsf(c[1]) <= 3.4028234e38f && fabsf(c[2]) <= 3.4028234e38f;
  }
  long long key = KEY_NONE;
  if (ok) {
    unsigned long long m = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float t = floorf((c[k] - kb.lo[k]) * kb.scale[k]);
      const unsigned qk = (unsigned)fminf(fmaxf(t, 0.f), 2097151.f);      // (NaN -> 0)
      m |= spread3(qk) << k;
    }
    key = min((long long)m, KEY_NONE - 1);
  }
  keys[i] = key;
}

// ------------------------------------------------------------------------------------------------ build
// One lane per leaf node: the min / max of the vertices of order[k LEAF .. (k + 1) LEAF).
__global__ __launch_bounds__(TB) void k_bvh_leaves(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces,
                                                    const int* __restrict__ order, int usable, int nleaves, float* __restrict__ node_lo,
                                                    float* __restrict__ node_hi) {
  const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (k >= nleaves) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < LEAF; ++i) {
    const int64_t at = k * LEAF + i;
    if (at >= usable) continue;
    const int f = order[at];
    float v[9];
    if (!((unsigned)f < (unsigned)nfaces && load_face(verts, nverts, faces, f, v))) continue;
#pragma unroll
    for (int c = 0; c < 9; ++c) { lo[c % 3] = fminf(lo[c % 3], v[c]); hi[c % 3] = fmaxf(hi[c % 3], v[c]); }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { node_lo[3 * k + c] = lo[c]; node_hi[3 * k + c] = hi[c]; }
}

// One lane per node of a level above the leaves: the min / max of its children, nodes k ARITY .. of the level below.
__global__ __launch_bounds__(TB) void k_bvh_level(const float* __restrict__ child_lo, const float* __restrict__ child_hi, int nchild,
                                                   float* __restrict__ node_lo, float* __restrict__ node_hi, int nnode) {
  const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (k >= nnode) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int i = 0; i < ARITY; ++i) {
    const int64_t ch = k * ARITY + i;
    if (ch >= nchild) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], child_lo[3 * ch + c]); hi[c] = fmaxf(hi[c], child_hi[3 * ch + c]); }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { node_lo[3 * k + c] = lo[c]; node_hi[3 * k + c] = hi[c]; }
}

// ------------------------------------------------------------------------------------------------ the walk
struct Tree {
  const float* __restrict__ verts;
  const int* __restrict__ faces;
  const int* __restrict__ order;
  const float* __restrict__ node_lo;
  const float* __restrict__ node_hi;
  int nverts, nfaces;
};

// the level table in LDS (every lane of the block calls it): read by a run-time level without a private array
__device__ __forceinline__ void stage_levels(const sp3_mesh_bvh& b, int* s_off) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int l = 0; l <= MAX_LEVELS; ++l) s_off[l] = b.level_off[l];
  }
  __syncthreads();
}

__device__ __forceinline__ unsigned entry_of(int level, int k) { return entry_bits(level, k); }

// Depth-first over the tree.  bound(node, key) -> false: nothing below the node can be a result; else key orders it among its
// siblings and the node is skipped iff key > best (strict: a node that may hold an equal result with a smaller face index is
// visited).  face(f, v) sees every face of a visited leaf and updates best.  stack: this lane's column, entries TB apart.
template <typename Bound, typename Face>
__device__ __forceinline__ void walk_tree(const Tree& t, const int* s_off, int levels, int usable, unsigned* stack, int cap, const double& best,
                                          int& nodes, int& evals, Bound bound, Face face) {
  int sp = 0;
  double key;
  if (cap >= 1 && bound(s_off[levels - 1], key) && !(key > best)) { stack[0] = entry_of(levels - 1, 0); sp = 1; }
  while (sp > 0) {
    const unsigned e = stack[--sp * TB];
    const int bit = 31 - __clz((int)e);
    const int l = (TOP_BIT - bit) / ARITY_BITS, k = (int)(e ^ (1u << bit));
    if (!(bound(s_off[l] + k, key) && !(key > best))) continue;
    ++nodes;
    if (l == 0) {
#pragma unroll
      for (int i = 0; i < LEAF; ++i) {
        const int64_t at = (int64_t)k * LEAF + i;
        if (at >= usable) continue;
        const int f = t.order[at];
        float v[9];
        if (!((unsigned)f < (unsigned)t.nfaces && load_face(t.verts, t.nverts, t.faces, f, v))) continue;      // (order holds usable faces only)
        ++evals;
        face(f, v);
      }
    } else {
      const int first = s_off[l - 1], nchild = s_off[l] - first;
      double ck[ARITY];
      unsigned ce[ARITY];
#pragma unroll
      for (int i = 0; i < ARITY; ++i) {
        const int64_t ch = (int64_t)k * ARITY + i;
        const bool ok = ch < nchild && bound(first + (int)ch, key) && !(key > best);
        ck[i] = ok ? key : INFINITY;
        ce[i] = ok ? entry_of(l - 1, (int)ch) : 0u;
      }
      // nearest first: an odd-even transposition sort, every index a constant
#pragma unroll
      for (int pass = 0; pass < ARITY; ++pass) {
#pragma unroll
        for (int i = pass & 1; i + 1 < ARITY; i += 2) {
          if (ck[i + 1] < ck[i]) {
            const double sk = ck[i]; ck[i] = ck[i + 1]; ck[i + 1] = sk;
            const unsigned se = ce[i]; ce[i] = ce[i + 1]; ce[i + 1] = se;
          }
        }
      }
#pragma unroll
      for (int i = ARITY - 1; i >= 0; --i) {
        if (ce[i] != 0u && sp < cap) { stack[sp * TB] = ce[i]; ++sp; }      // (sp < cap always holds: the header's count)
      }
    }
  }
}

// the squared distance from p to the box of `node` pushed out by the slack, less a margin that covers the rounding of an evaluated d2
__device__ __forceinline__ double box_dist2(const Tree& t, int node, double slack, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double p[3] = {px, py, pz};
  double g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double lo = (double)t.node_lo[3 * (int64_t)node + c], hi = (double)t.node_hi[3 * (int64_t)node + c];
    g[c] = fmax(fmax(lo - p[c], p[c] - hi) - slack, 0.0);
  }
  return ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) * (1.0 - 0x1p-30);
}

// the winning face (-1: none) of the query p
__device__ __forceinline__ int walk_dist(const Tree& t, const int* s_off, const sp3_mesh_bvh& b, unsigned* stack, int cap, float qx, float qy,
                                         float qz, int& nodes, int& evals) {
  const double px = (double)qx, py = (double)qy, pz = (double)qz, slack = (double)b.slack;
  if (!(is_finite(fabs(px)) && is_finite(fabs(py)) && is_finite(fabs(pz)))) return -1;      // never enters the tree
  double best = INFINITY;
  int bf = -1;
  walk_tree(t, s_off, b.levels, b.usable, stack, cap, best, nodes, evals,
            [&](int node, double& key) { key = box_dist2(t, node, slack, px, py, pz); return true; },
            [&](int f, const float (&v)[9]) {
              const double d2 = dist2_to_face(px, py, pz, v);
              if (d2 < best || (d2 == best && f < bf)) { best = d2; bf = f; }
            });
  return bf;
}

// the winning face (-1: none) of the ray (o, d) in [t_min, t_max].  ANY ("Mesh visibility"): the first accepted hit puts best
// below every node's entry (t0 >= t_min >= 0 > -inf), so every later pop and push fails the test walk_tree already makes: no new
// control flow, and a ray that hits nothing walks what the closest-hit walk walks.
template <bool ANY>
__device__ __forceinline__ int walk_ray(const Tree& t, const int* s_off, const sp3_mesh_bvh& b, unsigned* stack, int cap, const Ray& r, float ox,
                                        float oy, float oz, float dx, float dy, float dz, double t_min, double t_max, int cull, int& nodes,
                                        int& evals) {
  const double o[3] = {(double)ox, (double)oy, (double)oz}, d[3] = {(double)dx, (double)dy, (double)dz};
  const double slack = (double)b.slack;
  double best = INFINITY;
  int bf = -1;
  walk_tree(t, s_off, b.levels, b.usable, stack, cap, best, nodes, evals,
            [&](int node, double& key) {
              double lo[3], hi[3];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                lo[c] = (double)t.node_lo[3 * (int64_t)node + c] - slack;
                hi[c] = (double)t.node_hi[3 * (int64_t)node + c] + slack;
              }
              double t0 = t_min, t1 = t_max;
              const bool in = clip_box(o, d, lo, hi, t0, t1);
              key = t0;
              return in;
            },
            [&](int f, const float (&v)[9]) {
              Hit h;
              if (ANY) {
                if (intersect(r, v, t_min, t_max, cull, h)) { best = -INFINITY; bf = f; }      // (the rest of this leaf is still evaluated)
              } else if (intersect(r, v, t_min, t_max, cull, h) && (h.t < best || (h.t == best && f < bf))) { best = h.t; bf = f; }
            });
  return bf;
}

// ---- one lane per query, in the order of the queries' own Morton keys: the lanes of a wave descend through the same nodes
__global__ __launch_bounds__(TB) void k_bvh_dist(const float* __restrict__ q, const int64_t* __restrict__ qorder, int64_t nq, Tree t, sp3_mesh_bvh b,
                                                  int cap, float* __restrict__ dist, float* __restrict__ closest, int* __restrict__ face,
                                                  uint8_t* __restrict__ region, GridHead* head) {
  extern __shared__ unsigned s_stack[];
  __shared__ int s_off[MAX_LEVELS + 1];
  stage_levels(b, s_off);
  int nodes = 0, evals = 0;
  const int64_t qi = query_of(qorder, (int64_t)blockIdx.x * TB + threadIdx.x, nq);
  if (qi >= 0) {
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const int bf = walk_dist(t, s_off, b, s_stack + threadIdx.x, cap, qx, qy, qz, nodes, evals);
    write_result(t.verts, t.nverts, t.faces, t.nfaces, qi, qx, qy, qz, bf < 0 ? NO_FACE : bf, dist, closest, face, region);
  }
  head->count(nodes, evals);
}

// ---- the Walker of csrc/ray_kernels.h: the nodes a ray's slab test passes.  prepare: the level table in static LDS, this lane's
// column of the stack in the launch's dynamic LDS.
struct TreeWalker {
  Tree m;
  sp3_mesh_bvh b;
  int cap;
  const int* s_off;
  unsigned* stack;
  __device__ __forceinline__ void prepare(unsigned* lds) {
    __shared__ int off[MAX_LEVELS + 1];
    stage_levels(b, off);
    s_off = off;
    stack = lds + threadIdx.x;
  }
  template <bool ANY = false>
  __device__ __forceinline__ int walk(const Ray& r, float ox, float oy, float oz, float dx, float dy, float dz, double t_min, double t_max, int cull,
                                      int& nodes, int& evals) const {
    return walk_ray<ANY>(m, s_off, b, stack, cap, r, ox, oy, oz, dx, dy, dz, t_min, t_max, cull, nodes, evals);
  }
};

// ------------------------------------------------------------------------------------------------ host
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the level table the host built (spann3r_amd/cell_grid.py bvh_levels) against the counts it must follow from
int check_tree(const sp3_mesh_bvh* b, int64_t nfaces, const char* what) {
  SP3_CHECK(b != nullptr, "%s: null tree descriptor", what);
  SP3_CHECK(b->usable >= 1 && b->usable <= nfaces, "%s: %d usable faces of %lld", what, b->usable, (long long)nfaces);
  SP3_CHECK(b->levels >= 1 && b->levels <= MAX_LEVELS, "%s: %d levels (1 .. %d)", what, b->levels, MAX_LEVELS);
  SP3_CHECK(b->leaves == ceil_div(b->usable, LEAF), "%s: %d leaves for %d usable faces, %d per leaf", what, b->leaves, b->usable, LEAF);
  SP3_CHECK(b->slack >= 0.f && b->slack <= 3.4028234e38f, "%s: the slack must be finite and non-negative", what);
  SP3_CHECK(b->level_off[0] == 0, "%s: level offsets start at 0", what);
  int64_t size = b->leaves;
  for (int l = 0; l < b->levels; ++l) {
    SP3_CHECK((int64_t)b->level_off[l + 1] - b->level_off[l] == size, "%s: level %d holds %lld nodes, the table says %lld", what, l, (long long)size,
              (long long)b->level_off[l + 1] - b->level_off[l]);
    SP3_CHECK(size <= level_cap(l), "%s: level %d holds %lld nodes: more than the %lld a stack entry can name", what, l, (long long)size,
              (long long)level_cap(l));
    if (l + 1 < b->levels) {
      SP3_CHECK(size > 1, "%s: level %d is already the root, the table has %d levels", what, l, b->levels);
      size = ceil_div(size, ARITY);
    }
  }
  SP3_CHECK(size == 1, "%s: the last level holds %lld nodes, not 1", what, (long long)size);
  return 0;
}

inline int stack_cap(int levels) { return (ARITY - 1) * (levels - 1) + 1; }
inline size_t stack_bytes(int cap) { return (size_t)cap * TB * sizeof(unsigned); }
inline Tree tree_of(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                    const float* node_hi) {
  return {vertices, (const int*)faces, (const int*)order, node_lo, node_hi, (int)nverts, (int)nfaces};
}
inline TreeWalker walker_of(const Tree& t, const sp3_mesh_bvh* b) { return {t, *b, stack_cap(b->levels), nullptr, nullptr}; }

}  // namespace

extern "C" int sp3_mesh_bvh_keys(const float* vertices, int64_t nverts, const int32_t* faces, int64_t n, const float* box, int64_t* keys,
                                 void* stream) {
  SP3_CHECK(nverts >= 0 && nverts < N_MAX && n >= 0 && n < N_MAX, "sp3_mesh_bvh_keys: nverts %lld or n %lld out of range (both below 2^31 - 1)",
            (long long)nverts, (long long)n);
  SP3_CHECK(faces != nullptr || n == nverts, "sp3_mesh_bvh_keys: the point form keys every vertex: n %lld, nverts %lld", (long long)n,
            (long long)nverts);
  SP3_CHECK(box != nullptr, "sp3_mesh_bvh_keys: null box");
  KeyBox kb;
  for (int k = 0; k < 3; ++k) {
    const float lo = box[k], hi = box[3 + k];
    SP3_CHECK(isfinite(lo) && isfinite(hi) && lo <= hi, "sp3_mesh_bvh_keys: the box must be finite with lo <= hi");
    const float ext = hi - lo;
    kb.lo[k] = lo;
    kb.scale[k] = ext > 0.f && isfinite(2097152.f / ext) ? 2097152.f / ext : 0.f;
  }
  if (n == 0) return 0;
  SP3_CHECK(keys != nullptr && (nverts == 0 || vertices != nullptr), "sp3_mesh_bvh_keys: null vertices/keys");
  SP3_CHECK(((uintptr_t)keys & 7) == 0, "sp3_mesh_bvh_keys: keys must be 8-byte aligned");
  k_bvh_keys<<<blocks_for(n), TB, 0, (hipStream_t)stream>>>(vertices, (int)nverts, (const int*)faces, n, kb, (long long*)keys);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_keys");
  return 0;
}

extern "C" int sp3_mesh_bvh_build(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order,
                                  const sp3_mesh_bvh* b, float* node_lo, float* node_hi, void* stream) {
  if (check_mesh_sizes("sp3_mesh_bvh_build", nverts, nfaces)) return 1;
  if (check_tree(b, nfaces, "sp3_mesh_bvh_build")) return 1;
  SP3_CHECK(faces && order && node_lo && node_hi && (nverts == 0 || vertices), "sp3_mesh_bvh_build: null pointer");
  hipStream_t st = (hipStream_t)stream;
  k_bvh_leaves<<<blocks_for(b->leaves), TB, 0, st>>>(vertices, (int)nverts, (const int*)faces, (int)nfaces, (const int*)order, b->usable, b->leaves,
                                                     node_lo, node_hi);
  for (int l = 1; l < b->levels; ++l) {
    const int64_t c0 = b->level_off[l - 1], n0 = b->level_off[l], n1 = b->level_off[l + 1];
    k_bvh_level<<<blocks_for(n1 - n0), TB, 0, st>>>(node_lo + 3 * c0, node_hi + 3 * c0, (int)(n0 - c0), node_lo + 3 * n0, node_hi + 3 * n0,
                                                    (int)(n1 - n0));
  }
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_build");
  return 0;
}

extern "C" int sp3_mesh_bvh_dist_query(const float* q, const int64_t* q_order, int64_t nq, const float* vertices, int64_t nverts,
                                       const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo, const float* node_hi,
                                       const sp3_mesh_bvh* b, void* ws, float* dist, float* closest, int32_t* face, uint8_t* region, void* stream) {
  if (check_query_args("sp3_mesh_bvh_dist_query", nverts, nfaces, nq) || check_tree(b, nfaces, "sp3_mesh_bvh_dist_query")) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(q && faces && order && node_lo && node_hi && ws && dist && closest && face && region && (nverts == 0 || vertices),
            "sp3_mesh_bvh_dist_query: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_bvh_dist_query")) return e;
  const int cap = stack_cap(b->levels);
  k_bvh_dist<<<blocks_for(nq), TB, stack_bytes(cap), st>>>(q, q_order, nq, tree_of(vertices, nverts, faces, nfaces, order, node_lo, node_hi), *b, cap,
                                                          dist, closest, (int*)face, region, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_dist_query");
  return 0;
}

extern "C" int sp3_mesh_bvh_ray_query(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                                      int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                                      const float* node_hi, const sp3_mesh_bvh* b, double t_min, double t_max, int cull, void* ws, float* t,
                                      int32_t* face, float* bary, float* point, uint8_t* side, void* stream) {
  if (check_mesh_args("sp3_mesh_bvh_ray_query", nverts, nfaces, nq, t_min, t_max, cull) || check_tree(b, nfaces, "sp3_mesh_bvh_ray_query")) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(origins && directions && faces && order && node_lo && node_hi && ws && t && face && bary && point && side && (nverts == 0 || vertices),
            "sp3_mesh_bvh_ray_query: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_bvh_ray_query")) return e;
  const TreeWalker w = walker_of(tree_of(vertices, nverts, faces, nfaces, order, node_lo, node_hi), b);
  const RayOut out = {t, (int*)face, bary, point, side};
  k_ray_query<<<blocks_for(nq), TB, stack_bytes(w.cap), st>>>(origins, directions, q_order, nq, w, t_min, t_max, cull, out, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_ray_query");
  return 0;
}

extern "C" int sp3_mesh_bvh_ray_views(const sp3_mesh_ray_view* views_host, const sp3_mesh_ray_view* views_dev, int T, float pixel_offset,
                                      const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order,
                                      const float* node_lo, const float* node_hi, const sp3_mesh_bvh* b, void* ws, void* stream) {
  if (check_mesh_sizes("sp3_mesh_bvh_ray_views", nverts, nfaces) || check_view_args("sp3_mesh_bvh_ray_views", T, pixel_offset) ||
      check_tree(b, nfaces, "sp3_mesh_bvh_ray_views"))
    return 1;
  if (T == 0) return 0;
  SP3_CHECK(views_host && views_dev && faces && order && node_lo && node_hi && ws && (nverts == 0 || vertices), "sp3_mesh_bvh_ray_views: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_bvh_ray_views")) return e;
  dim3 grid;
  if (check_views("sp3_mesh_bvh_ray_views", views_host, T, grid)) return 1;
  const TreeWalker w = walker_of(tree_of(vertices, nverts, faces, nfaces, order, node_lo, node_hi), b);
  k_ray_views<<<grid, TB, stack_bytes(w.cap), st>>>(views_dev, pixel_offset, w, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_ray_views");
  return 0;
}

// ---- "Mesh visibility" over the tree
extern "C" int sp3_mesh_bvh_ray_occluded(const float* origins, const float* directions, const int64_t* q_order, int64_t nq, const float* vertices,
                                         int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order, const float* node_lo,
                                         const float* node_hi, const sp3_mesh_bvh* b, double t_min, double t_max, int cull, void* ws,
                                         uint8_t* occluded, void* stream) {
  if (check_mesh_args("sp3_mesh_bvh_ray_occluded", nverts, nfaces, nq, t_min, t_max, cull) || check_tree(b, nfaces, "sp3_mesh_bvh_ray_occluded"))
    return 1;
  if (nq == 0) return 0;
  SP3_CHECK(origins && directions && faces && order && node_lo && node_hi && ws && occluded && (nverts == 0 || vertices),
            "sp3_mesh_bvh_ray_occluded: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_bvh_ray_occluded")) return e;
  const TreeWalker w = walker_of(tree_of(vertices, nverts, faces, nfaces, order, node_lo, node_hi), b);
  k_ray_occluded<<<blocks_for(nq), TB, stack_bytes(w.cap), st>>>(origins, directions, q_order, nq, w, t_min, t_max, cull, occluded, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_ray_occluded");
  return 0;
}

extern "C" int sp3_mesh_bvh_point_views(const sp3_mesh_vis_view* views_host, const sp3_mesh_vis_view* views_dev, int T, float pixel_offset,
                                        float bias, int cull, const float* points, const int64_t* q_order, int64_t npoints,
                                        const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const int32_t* order,
                                        const float* node_lo, const float* node_hi, const sp3_mesh_bvh* b, void* ws, int32_t* count,
                                        uint8_t* mask, void* stream) {
  if (check_vis_args("sp3_mesh_bvh_point_views", T, pixel_offset, bias, cull, nverts, nfaces, npoints) ||
      check_tree(b, nfaces, "sp3_mesh_bvh_point_views"))
    return 1;
  if (T == 0 || npoints == 0) return 0;
  SP3_CHECK(views_host && views_dev && points && count && faces && order && node_lo && node_hi && ws && (nverts == 0 || vertices),
            "sp3_mesh_bvh_point_views: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_bvh_point_views")) return e;
  if (check_vis_views("sp3_mesh_bvh_point_views", views_host, T)) return 1;
  const TreeWalker w = walker_of(tree_of(vertices, nverts, faces, nfaces, order, node_lo, node_hi), b);
  k_point_views<<<point_views_grid(npoints, T), TB, stack_bytes(w.cap), st>>>(views_dev, pixel_offset, bias, cull, points, q_order, npoints, w,
                                                                             (int*)count, mask, (GridHead*)ws);
  SP3_LAUNCH_CHECK("sp3_mesh_bvh_point_views");
  return 0;
}
