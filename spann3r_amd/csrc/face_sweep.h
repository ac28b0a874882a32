// The brute-force sweep over the faces of a triangle mesh, per translation unit: the one statement of "every query against every
// face" for csrc/mesh_distance.hip (the nearest face of a point; also what a query the ring walk left open falls back to) and
// csrc/mesh_ray.hip (the first face a ray hits).
//   * A workgroup holds 256 queries in registers and streams its chunk of the faces through LDS in tiles of TILE faces (corners and
//     the usability verdict, one lane per face); the face list is split over blockIdx.y in chunks of about PER_CHUNK faces.
//   * The result of a query is the lexicographic minimum of (key, face index) over the faces its rule accepts, the key a
//     non-negative double (a squared distance, a ray parameter).  The pair does not fit one 64-bit atomic, so the join is two passes
//     over the same tiles: PASS 0, an integer atomicMin over the bits of the key (non-negative doubles order as their bits do);
//     PASS 1, an atomicMin of the face index among the faces that reach exactly that key -- the same inlined function on the same
//     inputs gives the same bits.  Both are order-free; what an atomic wrote is read by a LATER launch only.
//   * What differs between the questions is the Rule, a small struct passed by value:
//         bool load(int64_t qi)                        lane state from query qi (-1: no query) -> whether the lane takes part
//         void eval(const float* v, Take take) const   the staged face v[9]: take(key) if it counts
//     (eval hands its key to a callable, not back through a bool and a reference: the test of a ray stays one branch that way; with
//     the out-parameter the compiler kept two selects per face in the ray sweep, 2.6 % on 4096 rays x 0.93 M faces.)
//     The finish kernels, which turn the winning face into the outputs of a question, stay with the question.
#pragma once
#include "cell_grid.h"
#include "tri.h"

namespace {

constexpr int TILE = 512;                      // faces per LDS tile: 512 * 40 bytes
constexpr int PER_CHUNK = 4096;                // faces per workgroup, about (cell_grid.h size_brute)

// The workspace of a query call behind its 32-byte head: key and fkey per slot, then the fallback list (csrc/mesh_distance.hip
// alone; csrc/mesh_ray.hip has no fallback and its workspace ends after fkey).
struct SweepWs { GridHead* head; u64* key; int* fkey; int* list; };
inline SweepWs carve(void* ws, int64_t nq) {
  SweepWs w;
  w.head = (GridHead*)ws;
  w.key = (u64*)((char*)ws + 32);
  w.fkey = (int*)((char*)ws + 32 + round4(nq) * 8);
  w.list = w.fkey + round4(nq);
  return w;
}

// "no winner yet" in every slot (a sweep over all queries; the slots of a fallback list are reset as they are opened)
__global__ __launch_bounds__(TB) void k_fill_keys(u64* __restrict__ key, int* __restrict__ fkey, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n) { key[i] = ~0ull; fkey[i] = NO_FACE; }
}

// slots: the fallback list or every query (cell_grid.h Slots).
// PASS 0: key[slot] = min over the counted faces of the bits of their key.  PASS 1: fkey[slot] = min face index with key == key[slot].
template <int PASS, typename Rule>
__global__ __launch_bounds__(TB) void k_face_sweep(Rule rule, Slots slots, const float* __restrict__ verts, int nverts,
                                                    const int* __restrict__ faces, int64_t nfaces, int64_t chunk, u64* key, int* fkey) {
  __shared__ float tv[TILE * 9];
  __shared__ int tf[TILE];      // the face index, -1 for a face that is not usable
  const int64_t nq = slots.size();
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(r0 + chunk, nfaces);
  for (int64_t qb = (int64_t)blockIdx.x * TB; qb < nq; qb += (int64_t)gridDim.x * TB) {
    const int64_t slot = qb + threadIdx.x;
    const bool active = rule.load(slot < nq ? slots.query(slot) : -1);
    const double target = (PASS == 1 && active) ? __longlong_as_double((long long)key[slot]) : 0.0;      // NaN (all ones): nothing equals it
    double best = INFINITY;
    int bf = NO_FACE;
    for (int64_t t0 = r0; t0 < r1; t0 += TILE) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < TILE / TB; ++k) {
        const int i = threadIdx.x + k * TB;
        const int64_t f = t0 + i;
        if (f < r1) {
          float v[9];
          const bool ok = load_face(verts, nverts, faces, f, v) && has_area(v);
          tf[i] = ok ? (int)f : -1;
          if (ok) {
#pragma unroll
            for (int c = 0; c < 9; ++c) tv[i * 9 + c] = v[c];
          }
        }
      }
      __syncthreads();
      const int cnt = (int)min((int64_t)TILE, r1 - t0);
      for (int j = 0; j < cnt; ++j) {
        const int f = tf[j];      // the same address in every lane: an LDS broadcast, and a uniform branch
        if (f < 0) continue;
        rule.eval(tv + j * 9, [&](double k) {
          if (PASS == 0) {
            if (k < best) best = k;
          } else {
            if (k == target && f < bf) bf = f;
          }
        });
      }
    }
    if (active && r0 < r1) {
      if (PASS == 0) {
        if (best < INFINITY) atomicMin(&key[slot], (u64)__double_as_longlong(best));      // key >= +0: bit order = value order
      } else {
        if (bf != NO_FACE) atomicMin(&fkey[slot], bf);
      }
    }
  }
}

// both passes over the slots -> the launch shape, whose qblocks the caller's finish kernel takes
template <typename Rule>
inline BruteLaunch sweep_faces(const Rule& rule, const Slots& slots, const float* verts, int nverts, const int* faces, int64_t nfaces,
                               const SweepWs& w, hipStream_t st) {
  const BruteLaunch l = size_brute(slots.nq_all, nfaces, PER_CHUNK, TILE);
  const dim3 grid(l.qblocks, l.chunks);
  k_face_sweep<0><<<grid, TB, 0, st>>>(rule, slots, verts, nverts, faces, nfaces, l.chunk, w.key, w.fkey);
  k_face_sweep<1><<<grid, TB, 0, st>>>(rule, slots, verts, nverts, faces, nfaces, l.chunk, w.key, w.fkey);
  return l;
}

}  // namespace
