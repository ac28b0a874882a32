// Exact point-to-triangle-mesh distance (include/spann3r_hip.h "Mesh distance"; spann3r_amd/mesh.py TriangleGrid /
// point_mesh_distance and spann3r_amd/evaluate.py evaluate_meshes(exact=True) drive these; tests/mesh_distance_ref.py restates the rule).
//
//   * The rule of one (query, face) pair is Ericson's closest point on a triangle by Voronoi region, in fp64, every operation rounded
//     on its own (csrc/tri_dist.h states it once, for this file and csrc/mesh_bvh.hip; the file-level pragma below covers the rest;
//     csrc/mesh_sample.hip has the history) and in the order the header fixes.  The result of
//     a query is the lexicographic minimum of (d2, face index) over the usable faces: a pure function of the inputs, so a face may be
//     evaluated in any order, any number of times, by either kernel.
//   * Faces are registered in every cell of an sp3_nn_grid their bounding box touches (sp3_mesh_tri_cell_count / _fill; the host
//     sorts the pairs by cell).  A query walks the cells around its home cell ring by ring, with the walk and the stopping bound of
//     csrc/cell_grid.h, which sp3_nn_query shares: a face that no cell of the visited block holds has, on one axis, every one of
//     its cells beyond a wall of the block, so it lies wholly behind that wall and the wall's distance bounds it.
//   * The hot loops keep (d2, face) only; the closest point and the region of the winner are recomputed once at the end.
//   * Brute force -- every query, or the ones the walk left open -- is the face sweep of csrc/face_sweep.h (LDS tiles, the two
//     order-free passes, the workspace carving) with the rule "key = d2, every usable face counts"; the finish kernel here turns the
//     winning face into the four outputs.
//   * The lane's query index (query_of), the size checks and the workspace head (begin_query) are csrc/cell_grid.h's, shared with
//     csrc/mesh_ray.hip and csrc/mesh_bvh.hip.
//   * Every loop is bounded by max_ring, the grid dims, npairs or nfaces; nothing waits on another lane's store; what an atomic wrote
//     is read by a LATER launch only.
#include "face_sweep.h"
#include "tri_dist.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ faces in the grid (csrc/cell_grid.h)
// the cells [x0, x1] x [y0, y1] x [z0, z1] of the face's bounding box pushed out by the slack; cell_axis is monotone in x, so every
// point of the face falls in one of them whatever the fp32 rounding of the box does
__device__ __forceinline__ void face_cells(const sp3_nn_grid& g, const float (&v)[9], int (&lo)[3], int (&hi)[3]) {
  const float o[3] = {g.ox, g.oy, g.oz};
  const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    lo[k] = cell_axis(mn - g.slack, o[k], g.inv_h, n[k]);
    hi[k] = max(cell_axis(mx + g.slack, o[k], g.inv_h, n[k]), lo[k]);
  }
}

__global__ __launch_bounds__(TB) void k_md_cell_count(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t nfaces,
                                                       sp3_nn_grid g, int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (f >= nfaces) return;
  float v[9];
  int64_t n = 0;
  if (load_face(verts, nverts, faces, f, v) && has_area(v)) {
    int lo[3], hi[3];
    face_cells(g, v, lo, hi);
    n = (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
  }
  counts[f] = n;
}

__global__ __launch_bounds__(TB) void k_md_cell_fill(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t nfaces,
                                                      sp3_nn_grid g, const int64_t* __restrict__ offsets, int64_t npairs,
                                                      int* __restrict__ pair_cell, int* __restrict__ pair_face) {
  const int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (f >= nfaces) return;
  float v[9];
  if (!(load_face(verts, nverts, faces, f, v) && has_area(v))) return;
  int lo[3], hi[3];
  face_cells(g, v, lo, hi);
  int64_t at = offsets[f];
  if (at < 0) return;
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        if (at >= npairs) return;      // offsets that do not belong to this grid: never past the arrays
        pair_cell[at] = cell_id(g, x, y, z);
        pair_face[at] = (int)f;
        ++at;
      }
}

// ---- one lane per query (queries sorted by home cell: the lanes of a wave walk the same cells)
__global__ __launch_bounds__(TB) void k_md_grid(const float* __restrict__ q, const int64_t* __restrict__ order, int64_t nq,
                                                 const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces,
                                                 const int* __restrict__ pair_face, int npairs, const int* __restrict__ cell_start, sp3_nn_grid g,
                                                 int max_ring, float* __restrict__ dist, float* __restrict__ closest, int* __restrict__ face,
                                                 uint8_t* __restrict__ region, GridHead* head, u64* __restrict__ fb_key, int* __restrict__ fb_face,
                                                 int* __restrict__ fb_list) {
  int cells = 0, evals = 0;
  const int64_t qi = query_of(order, (int64_t)blockIdx.x * TB + threadIdx.x, nq);
  if (qi >= 0) {
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const double px = (double)qx, py = (double)qy, pz = (double)qz;
    double best = INFINITY;
    int bf = -1;
    const auto scan = [&](int s, int e) {
      s = max(s, 0);
      e = min(e, npairs);
      for (int j = s; j < e; ++j) {
        const int f = pair_face[j];
        float v[9];
        if (!((unsigned)f < (unsigned)nfaces && load_face(verts, nverts, faces, f, v))) continue;      // (the pairs hold usable faces only)
        ++evals;
        const double d2 = dist2_to_face(px, py, pz, v);
        if (d2 < best || (d2 == best && f < bf)) { best = d2; bf = f; }
      }
    };
    // settled: everything unvisited lies behind a wall that is farther than the best
    if (walk_rings(g, cell_start, qx, qy, qz, max_ring, cells, scan, [&](float b) { return best <= (double)b * (double)b; })) {
      write_result(verts, nverts, faces, nfaces, qi, qx, qy, qz, bf < 0 ? NO_FACE : bf, dist, closest, face, region);
    } else {
      fb_face[head->open_slot(qi, fb_list, fb_key)] = NO_FACE;
    }
  }
  head->count(cells, evals);
}

// ---- brute force (csrc/face_sweep.h): the key of a face is its squared distance, and every usable face counts
struct DistRule {
  const float* __restrict__ q;
  double px, py, pz;
  __device__ __forceinline__ bool load(int64_t qi) {
    const bool active = qi >= 0;
    px = active ? (double)q[3 * qi] : 0.0; py = active ? (double)q[3 * qi + 1] : 0.0; pz = active ? (double)q[3 * qi + 2] : 0.0;
    return active;
  }
  template <typename Take>
  __device__ __forceinline__ void eval(const float* v, Take take) const { take(dist2_to_face(px, py, pz, v)); }
};

__global__ __launch_bounds__(TB) void k_md_brute_finish(const float* __restrict__ q, Slots slots, const float* __restrict__ verts, int nverts,
                                                         const int* __restrict__ faces, int nfaces, const int* __restrict__ fkey,
                                                         float* __restrict__ dist, float* __restrict__ closest, int* __restrict__ face,
                                                         uint8_t* __restrict__ region) {
  const int64_t nq = slots.size();
  for (int64_t slot = (int64_t)blockIdx.x * TB + threadIdx.x; slot < nq; slot += (int64_t)gridDim.x * TB) {
    const int64_t qi = slots.query(slot);
    if (qi < 0) continue;
    write_result(verts, nverts, faces, nfaces, qi, q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], fkey[slot], dist, closest, face, region);
  }
}

// the brute-force stage over the listed queries (list / count null: every query): the two passes and the finish
void launch_brute(const float* q, const int* list, const int* count, int64_t nq, const float* verts, int nverts, const int* faces, int64_t nfaces,
                  const SweepWs& w, float* dist, float* closest, int* face, uint8_t* region, hipStream_t st) {
  const Slots slots = {list, count, nq};
  const BruteLaunch l = sweep_faces(DistRule{q}, slots, verts, nverts, faces, nfaces, w, st);
  k_md_brute_finish<<<l.qblocks, TB, 0, st>>>(q, slots, verts, nverts, faces, (int)nfaces, w.fkey, dist, closest, face, region);
}

}  // namespace

extern "C" int sp3_mesh_tri_cell_count(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const sp3_nn_grid* g,
                                       int64_t* counts, void* stream) {
  SP3_CHECK(sizes_ok_or_empty(nverts, nfaces), "sp3_mesh_tri_cell_count: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  if (check_grid(g, "sp3_mesh_tri_cell_count")) return 1;
  if (nfaces == 0) return 0;
  SP3_CHECK(faces != nullptr && counts != nullptr && (nverts == 0 || vertices != nullptr), "sp3_mesh_tri_cell_count: null vertices/faces/counts");
  SP3_CHECK(((uintptr_t)counts & 7) == 0, "sp3_mesh_tri_cell_count: counts must be 8-byte aligned");
  k_md_cell_count<<<blocks_for(nfaces), TB, 0, (hipStream_t)stream>>>(vertices, (int)nverts, (const int*)faces, nfaces, *g, counts);
  SP3_LAUNCH_CHECK("sp3_mesh_tri_cell_count");
  return 0;
}

extern "C" int sp3_mesh_tri_cell_fill(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const sp3_nn_grid* g,
                                      const int64_t* offsets, int64_t npairs, int32_t* pair_cell, int32_t* pair_face, void* stream) {
  SP3_CHECK(sizes_ok_or_empty(nverts, nfaces), "sp3_mesh_tri_cell_fill: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  SP3_CHECK(npairs >= 0 && npairs < N_MAX, "sp3_mesh_tri_cell_fill: npairs %lld out of range (0 .. 2^31 - 2)", (long long)npairs);
  if (check_grid(g, "sp3_mesh_tri_cell_fill")) return 1;
  if (nfaces == 0 || npairs == 0) return 0;
  SP3_CHECK(faces != nullptr && offsets != nullptr && pair_cell != nullptr && pair_face != nullptr && (nverts == 0 || vertices != nullptr),
            "sp3_mesh_tri_cell_fill: null vertices/faces/offsets/pair_cell/pair_face");
  SP3_CHECK(((uintptr_t)offsets & 7) == 0, "sp3_mesh_tri_cell_fill: offsets must be 8-byte aligned");
  k_md_cell_fill<<<blocks_for(nfaces), TB, 0, (hipStream_t)stream>>>(vertices, (int)nverts, (const int*)faces, nfaces, *g, offsets, npairs,
                                                                     (int*)pair_cell, (int*)pair_face);
  SP3_LAUNCH_CHECK("sp3_mesh_tri_cell_fill");
  return 0;
}

extern "C" int64_t sp3_mesh_dist_query_ws_bytes(int64_t nq) { return nq < 0 || nq > N_MAX ? 0 : 32 + round4(nq) * 16; }

extern "C" int sp3_mesh_dist_query(const float* q, const int64_t* q_order, int64_t nq, const float* vertices, int64_t nverts, const int32_t* faces,
                                   int64_t nfaces, const int32_t* pair_face, int64_t npairs, const int32_t* cell_start, const sp3_nn_grid* g,
                                   int max_ring, void* ws, float* dist, float* closest, int32_t* face, uint8_t* region, void* stream) {
  if (check_mesh_sizes("sp3_mesh_dist_query", nverts, nfaces)) return 1;
  SP3_CHECK(nq >= 0 && nq <= N_MAX && npairs >= 0 && npairs < N_MAX, "sp3_mesh_dist_query: nq = %lld or npairs = %lld out of range", (long long)nq,
            (long long)npairs);
  SP3_CHECK(max_ring >= 0, "sp3_mesh_dist_query: max_ring must be non-negative");
  if (check_grid(g, "sp3_mesh_dist_query")) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(q && faces && cell_start && ws && dist && closest && face && region && (nverts == 0 || vertices) && (npairs == 0 || pair_face),
            "sp3_mesh_dist_query: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_dist_query")) return e;
  const SweepWs w = carve(ws, nq);
  k_md_grid<<<blocks_for(nq), TB, 0, st>>>(q, q_order, nq, vertices, (int)nverts, (const int*)faces, (int)nfaces, (const int*)pair_face, (int)npairs,
                                           (const int*)cell_start, *g, max_ring, dist, closest, (int*)face, region, w.head, w.key, w.fkey, w.list);
  launch_brute(q, w.list, &w.head->fb_count, nq, vertices, (int)nverts, (const int*)faces, nfaces, w, dist, closest, (int*)face, region, st);
  SP3_LAUNCH_CHECK("sp3_mesh_dist_query");
  return 0;
}

extern "C" int sp3_mesh_dist_brute(const float* q, int64_t nq, const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, void* ws,
                                   float* dist, float* closest, int32_t* face, uint8_t* region, void* stream) {
  if (check_query_args("sp3_mesh_dist_brute", nverts, nfaces, nq)) return 1;
  if (nq == 0) return 0;
  SP3_CHECK(q && faces && ws && dist && closest && face && region && (nverts == 0 || vertices), "sp3_mesh_dist_brute: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int e = begin_query(ws, st, "sp3_mesh_dist_brute")) return e;
  const SweepWs w = carve(ws, nq);
  k_fill_keys<<<blocks_for(nq), TB, 0, st>>>(w.key, w.fkey, nq);
  launch_brute(q, nullptr, nullptr, nq, vertices, (int)nverts, (const int*)faces, nfaces, w, dist, closest, (int*)face, region, st);
  SP3_LAUNCH_CHECK("sp3_mesh_dist_brute");
  return 0;
}
