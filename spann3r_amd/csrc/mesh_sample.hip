// Mesh surface sampling and normals (include/spann3r_hip.h "Mesh surface sampling and normals"; spann3r_amd/mesh.py face_frames /
// sample_surface / vertex_normals drive these).  Everything rests on one per-face quantity, the cross product n of two edges in fp64
// and its length d (twice the area).  sp3_mesh_face_frames turns d into an INTEGER weight w = floor(d / dmax * 2^32) and scans it;
// sp3_mesh_sample draws faces from that prefix sum with a counter-based generator and places a point by 24-bit integer barycentric
// coordinates; sp3_mesh_vertex_normals adds llrint(n / dmax * 2^30) to the three vertices of every face in 64-bit integers.
// dmax is a maximum over the bits of non-negative doubles, the prefix sum and the vertex sums are integer: nothing depends on the
// order of the atomics or of the tiles, so every output is the same bits every run.
//
// One lane per face, per sample or per vertex.  Launch boundaries are the only hand-offs besides the agent-scope atomics (the
// atomicMax of dmax, the atomicAdds of the vertex sums); what an atomic wrote is read with plain loads in a LATER launch only.
//
// Every fp64 operation of the rule is rounded on its own (no contraction into FMAs): the file-level pragma below is what the
// compiler honours under its default -ffp-contract=fast-honor-pragmas, and the rule is written with plain operators for that reason
// (csrc/mesh_simplify.hip has the history).
#include "common.h"
#include "scan.h"
#include "tri.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }

const int64_t kIndexLimit = 0x7fffffffLL;      // int32 indices; 256-element tiles keep every grid below 2^23 blocks

// ------------------------------------------------------------------------------------------------ the rule of a face
struct Frame {
  EdgeCross e;      // (csrc/tri.h) all zero for an invalid face; nx, ny, nz, d zero for a non-finite one
  int abc[3];       // the face's three vertex indices
  bool valid;       // they lie in 0..V-1 (nothing is dereferenced otherwise)
};

__device__ __forceinline__ Frame frame_of(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t f) {
  Frame r = {};
  float v[9];
  r.valid = load_face(verts, nverts, faces, f, v, r.abc);
  if (!r.valid) return r;
  r.e = edge_cross(v);
  if (!is_finite(r.e.d)) r.e.nx = r.e.ny = r.e.nz = r.e.d = 0.0;
  return r;
}

// ------------------------------------------------------------------------------------------------ 64-bit variants of scan.h
// inclusive sum of `v` over the lanes up to this one and the block's total; every thread of the block calls it
__device__ __forceinline__ u64 block_incl_sum64(u64 v, u64& total) {
  __shared__ u64 wtot[MB / SP3_WAVE];
  const int lane = threadIdx.x & (SP3_WAVE - 1), wave = threadIdx.x / SP3_WAVE;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < SP3_WAVE; o <<= 1) {
    const u64 up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  if (lane == SP3_WAVE - 1) wtot[wave] = inc;
  __syncthreads();
  u64 base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < MB / SP3_WAVE; ++i) {
    if (i < wave) base += wtot[i];
    sum += wtot[i];
  }
  total = sum;
  return base + inc;
}

// totals[0..nb) -> exclusive offsets in place; info[0] = the grand total.  One workgroup; thread i owns `per` consecutive totals.
__global__ __launch_bounds__(SCAN_T) void k_sf_tile_scan64(u64* __restrict__ totals, int nb, int per, u64* __restrict__ info) {
  __shared__ u64 part[SCAN_T];
  const int i = threadIdx.x;
  const int lo = (int)min((int64_t)i * per, (int64_t)nb), hi = (int)min((int64_t)lo + per, (int64_t)nb);
  u64 s = 0;
  for (int j = lo; j < hi; ++j) s += totals[j];
  part[i] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {      // inclusive scan of the 1024 partial sums
    const u64 v = i >= d ? part[i - d] : 0ull;
    __syncthreads();
    part[i] += v;
    __syncthreads();
  }
  u64 run = part[i] - s;
  for (int j = lo; j < hi; ++j) {
    const u64 c = totals[j];
    totals[j] = run;
    run += c;
  }
  if (i == SCAN_T - 1) info[0] = part[i];
}

// ------------------------------------------------------------------------------------------------ face frames
__global__ __launch_bounds__(MB) void k_sf_clear(u64* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (i < n) p[i] = 0ull;
}

// cum[f] = the bits of d (a later launch turns them into weights), face_normals[f] = n / d, info[1] = max of the bits of d.  The bits
// of non-negative finite doubles order as the doubles do, so an integer maximum is the fp64 maximum, in any order.
__global__ __launch_bounds__(MB) void k_sf_frames(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t nfaces,
                                                   float* __restrict__ face_normals, u64* __restrict__ cum, u64* info) {
  __shared__ u64 wmax[MB / SP3_WAVE];
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  u64 bits = 0ull;
  if (f < nfaces) {
    const Frame r = frame_of(verts, nverts, faces, f);
    bits = (u64)__double_as_longlong(r.e.d);
    cum[f] = bits;
    if (face_normals != nullptr) {
      const bool pos = r.e.d > 0.0;
      face_normals[3 * f] = pos ? (float)(r.e.nx / r.e.d) : 0.f;
      face_normals[3 * f + 1] = pos ? (float)(r.e.ny / r.e.d) : 0.f;
      face_normals[3 * f + 2] = pos ? (float)(r.e.nz / r.e.d) : 0.f;
    }
  }
  u64 m = bits;
#pragma unroll
  for (int o = SP3_WAVE / 2; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(m, o);
    m = other > m ? other : m;
  }
  if ((threadIdx.x & (SP3_WAVE - 1)) == 0) wmax[threadIdx.x / SP3_WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < MB / SP3_WAVE; ++i) m = wmax[i] > m ? wmax[i] : m;
    // the maximum only grows: a block whose own maximum is not above what is already there has nothing to add (a stale read is a
    // smaller value and only costs an atomic that changes nothing)
    if (m > __hip_atomic_load(info + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      __hip_atomic_fetch_max(info + 1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ u64 weight_of(double d, double dmax) {
  return d > 0.0 ? (u64)floor(d / dmax * 4294967296.0) : 0ull;      // d <= dmax: at most 2^32
}

// cum[f]: the bits of d -> the inclusive sum of the weights inside the tile; totals[tile] = the tile's sum
__global__ __launch_bounds__(MB) void k_sf_weights(u64* __restrict__ cum, int64_t nfaces, const u64* __restrict__ info, u64* __restrict__ totals) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  const double dmax = __longlong_as_double((long long)info[1]);
  const u64 w = f < nfaces ? weight_of(__longlong_as_double((long long)cum[f]), dmax) : 0ull;
  u64 total;
  const u64 inc = block_incl_sum64(w, total);
  if (f < nfaces) cum[f] = inc;
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_sf_add_back(u64* __restrict__ cum, int64_t nfaces, const u64* __restrict__ offsets) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (f < nfaces) cum[f] += offsets[blockIdx.x];
}

// ------------------------------------------------------------------------------------------------ samples
__device__ __forceinline__ u64 hash_counter(u64 seed, u64 c) {
  u64 z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ float place(double a, double e1, double e2, double ua, double ub) {
  const double p1 = ua * e1;
  const double p2 = ub * e2;
  const double s = p1 + p2;
  return (float)(a + s);
}

__device__ __forceinline__ uint32_t mix_bytes(uint32_t ca, uint32_t cb, uint32_t cc, uint32_t wa, uint32_t a, uint32_t b) {
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {      // at most 255 * 2^24 + 2^23 < 2^32
    const uint32_t s = ((ca >> (8 * k)) & 255u) * wa + ((cb >> (8 * k)) & 255u) * a + ((cc >> (8 * k)) & 255u) * b + (1u << 23);
    out |= (s >> 24) << (8 * k);
  }
  return out;
}

// the smallest f in [lo, hi) with cum[f] > t; the caller guarantees cum[hi - 1] > t.  About log2 F dependent loads.  (A two-level form --
// the last entries of the 256-face tiles first, then inside the tile -- measured the same on the MI355X, 0.133 / 0.134 ms for 10^6
// samples of 0.93 M faces and 0.200 / 0.199 ms of 3.5 M (profiles/mesh_sample.txt), and was dropped: the first steps of the plain
// search touch the same few entries in every lane, which stay in cache just as a table of tile ends would.)
__device__ __forceinline__ int upper_bound(const u64* __restrict__ cum, int lo, int hi, u64 t) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(MB) void k_sf_sample(const float* __restrict__ verts, const uint32_t* __restrict__ rgba, int nverts,
                                                   const int* __restrict__ faces, int nfaces, const u64* __restrict__ cum,
                                                   const u64* __restrict__ info, int64_t nsamples, u64 seed, float* __restrict__ points,
                                                   float* __restrict__ normals, uint32_t* __restrict__ out_rgba, int* __restrict__ face_index) {
  const int64_t k = (int64_t)blockIdx.x * MB + threadIdx.x;
  const u64 W = info[0];
  if (k >= nsamples || W == 0ull) return;      // (W = 0: the caller was told not to launch; nothing is read or written)
  const u64 t = __umul64hi(hash_counter(seed, 3ull * (u64)k), W);      // t < W = cum[nfaces - 1]
  const int f = min(upper_bound(cum, 0, nfaces, t), nfaces - 1);      // (the min is not reached: t < cum[nfaces - 1])
  uint32_t a = (uint32_t)(hash_counter(seed, 3ull * (u64)k + 1ull) >> 40);
  uint32_t b = (uint32_t)(hash_counter(seed, 3ull * (u64)k + 2ull) >> 40);
  if (a + b > (1u << 24)) {
    a = (1u << 24) - a;
    b = (1u << 24) - b;
  }
  // a drawn face has a weight, so it is valid and finite when cum belongs to these faces; frame_of checks the indices all the same
  const Frame r = frame_of(verts, nverts, faces, f);
  const double ua = (double)a / 16777216.0, ub = (double)b / 16777216.0;
  points[3 * k] = place(r.e.ax, r.e.e1x, r.e.e2x, ua, ub);
  points[3 * k + 1] = place(r.e.ay, r.e.e1y, r.e.e2y, ua, ub);
  points[3 * k + 2] = place(r.e.az, r.e.e1z, r.e.e2z, ua, ub);
  const bool pos = r.e.d > 0.0;
  normals[3 * k] = pos ? (float)(r.e.nx / r.e.d) : 0.f;
  normals[3 * k + 1] = pos ? (float)(r.e.ny / r.e.d) : 0.f;
  normals[3 * k + 2] = pos ? (float)(r.e.nz / r.e.d) : 0.f;
  face_index[k] = f;
  if (out_rgba != nullptr) out_rgba[k] = r.valid ? mix_bytes(rgba[r.abc[0]], rgba[r.abc[1]], rgba[r.abc[2]], (1u << 24) - a - b, a, b) : 0u;
}

// ------------------------------------------------------------------------------------------------ vertex normals
__device__ __forceinline__ void add64(u64* p, long long x) {      // two's complement on unsigned 64-bit
  __hip_atomic_fetch_add(p, (u64)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one add per lane and sum (nearly every vertex has valence 6 - 8: nothing to aggregate in the wave)
__global__ __launch_bounds__(MB) void k_sf_vertex_accumulate(const float* __restrict__ verts, int nverts, const int* __restrict__ faces,
                                                              int64_t nfaces, const u64* __restrict__ info, u64* sums) {
  const int64_t f = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (f >= nfaces) return;
  const Frame r = frame_of(verts, nverts, faces, f);
  if (!(r.e.d > 0.0)) return;      // invalid, not finite or without area: q = 0
  const double dmax = __longlong_as_double((long long)info[1]);
  const long long qx = llrint(r.e.nx / dmax * 1073741824.0);
  const long long qy = llrint(r.e.ny / dmax * 1073741824.0);
  const long long qz = llrint(r.e.nz / dmax * 1073741824.0);
  const int (&v)[3] = r.abc;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    u64* s = sums + 3 * (int64_t)v[j];
    if (qx != 0) add64(s, qx);
    if (qy != 0) add64(s + 1, qy);
    if (qz != 0) add64(s + 2, qz);
  }
}

__global__ __launch_bounds__(MB) void k_sf_vertex_finalize(const u64* __restrict__ sums, int nverts, float* __restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (v >= nverts) return;
  const long long ix = (long long)sums[3 * v], iy = (long long)sums[3 * v + 1], iz = (long long)sums[3 * v + 2];
  float x = 0.f, y = 0.f, z = 0.f;
  if (ix != 0 || iy != 0 || iz != 0) {
    const double sx = (double)ix, sy = (double)iy, sz = (double)iz;
    const double len = sqrt(sx * sx + sy * sy + sz * sz);
    x = (float)(sx / len);
    y = (float)(sy / len);
    z = (float)(sz / len);
  }
  normals[3 * v] = x;
  normals[3 * v + 1] = y;
  normals[3 * v + 2] = z;
}

inline bool sizes_ok(int64_t nverts, int64_t nfaces) { return nverts >= 0 && nverts < kIndexLimit && nfaces >= 0 && nfaces < kIndexLimit; }

}  // namespace

extern "C" int64_t sp3_mesh_face_frames_ws_bytes(int64_t nfaces) {
  if (nfaces <= 0 || nfaces >= kIndexLimit) return 0;
  return ((nfaces + MB - 1) / MB) * 8;
}

extern "C" int sp3_mesh_face_frames(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, void* ws, float* face_normals,
                                    uint64_t* cum, uint64_t* info, void* stream) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "sp3_mesh_face_frames: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  SP3_CHECK(info != nullptr, "sp3_mesh_face_frames: null info");
  SP3_CHECK(nfaces == 0 || (faces != nullptr && ws != nullptr && cum != nullptr && (nverts == 0 || vertices != nullptr)),
            "sp3_mesh_face_frames: null vertices/faces/ws/cum");
  SP3_CHECK(((uintptr_t)ws & 7) == 0 && ((uintptr_t)cum & 7) == 0 && ((uintptr_t)info & 7) == 0,
            "sp3_mesh_face_frames: ws, cum and info must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sf_clear, dim3(1), dim3(MB), 0, st, (u64*)info, (int64_t)2);
  if (nfaces > 0) {
    const int nb = (int)blocks_for(nfaces);
    u64* totals = (u64*)ws;
    hipLaunchKernelGGL(k_sf_frames, dim3(nb), dim3(MB), 0, st, vertices, (int)nverts, (const int*)faces, nfaces, face_normals, (u64*)cum, (u64*)info);
    hipLaunchKernelGGL(k_sf_weights, dim3(nb), dim3(MB), 0, st, (u64*)cum, nfaces, (const u64*)info, totals);
    hipLaunchKernelGGL(k_sf_tile_scan64, dim3(1), dim3(SCAN_T), 0, st, totals, nb, (nb + SCAN_T - 1) / SCAN_T, (u64*)info);
    hipLaunchKernelGGL(k_sf_add_back, dim3(nb), dim3(MB), 0, st, (u64*)cum, nfaces, (const u64*)totals);
  }
  SP3_LAUNCH_CHECK("sp3_mesh_face_frames");
  return 0;
}

extern "C" int sp3_mesh_sample(const float* vertices, const uint32_t* rgba, int64_t nverts, const int32_t* faces, int64_t nfaces,
                               const uint64_t* cum, const uint64_t* info, int64_t nsamples, uint64_t seed, float* points, float* normals,
                               uint32_t* out_rgba, int32_t* face_index, void* stream) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "sp3_mesh_sample: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  SP3_CHECK(nsamples >= 0 && nsamples < ((int64_t)1 << 40), "sp3_mesh_sample: nsamples %lld out of range (0 .. 2^40 - 1)", (long long)nsamples);
  if (nsamples == 0) return 0;
  SP3_CHECK(nfaces > 0 && nverts > 0, "sp3_mesh_sample: %lld samples of a mesh of %lld faces over %lld vertices: no area to sample",
            (long long)nsamples, (long long)nfaces, (long long)nverts);
  SP3_CHECK(vertices != nullptr && faces != nullptr && cum != nullptr && info != nullptr && points != nullptr && normals != nullptr &&
                face_index != nullptr,
            "sp3_mesh_sample: null vertices/faces/cum/info/points/normals/face_index");
  SP3_CHECK((rgba == nullptr) == (out_rgba == nullptr), "sp3_mesh_sample: rgba and out_rgba go together");
  SP3_CHECK(((uintptr_t)cum & 7) == 0 && ((uintptr_t)info & 7) == 0, "sp3_mesh_sample: cum and info must be 8-byte aligned");
  hipLaunchKernelGGL(k_sf_sample, dim3(blocks_for(nsamples)), dim3(MB), 0, (hipStream_t)stream, vertices, rgba, (int)nverts, (const int*)faces,
                     (int)nfaces, (const u64*)cum, (const u64*)info, nsamples, (u64)seed, points, normals, out_rgba, (int*)face_index);
  SP3_LAUNCH_CHECK("sp3_mesh_sample");
  return 0;
}

extern "C" int64_t sp3_mesh_vertex_normals_ws_bytes(int64_t nverts) {
  if (nverts <= 0 || nverts >= kIndexLimit) return 0;
  return nverts * 24;
}

extern "C" int sp3_mesh_vertex_normals(const float* vertices, int64_t nverts, const int32_t* faces, int64_t nfaces, const uint64_t* info, void* ws,
                                       float* normals, void* stream) {
  SP3_CHECK(sizes_ok(nverts, nfaces), "sp3_mesh_vertex_normals: nverts %lld or nfaces %lld out of range (int32 indices: both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  if (nverts == 0) return 0;
  SP3_CHECK(vertices != nullptr && ws != nullptr && normals != nullptr && (nfaces == 0 || (faces != nullptr && info != nullptr)),
            "sp3_mesh_vertex_normals: null vertices/faces/info/ws/normals");
  SP3_CHECK(((uintptr_t)ws & 7) == 0 && ((uintptr_t)info & 7) == 0, "sp3_mesh_vertex_normals: ws and info must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  u64* sums = (u64*)ws;
  hipLaunchKernelGGL(k_sf_clear, dim3(blocks_for(3 * nverts)), dim3(MB), 0, st, sums, 3 * nverts);
  if (nfaces > 0)
    hipLaunchKernelGGL(k_sf_vertex_accumulate, dim3(blocks_for(nfaces)), dim3(MB), 0, st, vertices, (int)nverts, (const int*)faces, nfaces,
                       (const u64*)info, sums);
  hipLaunchKernelGGL(k_sf_vertex_finalize, dim3(blocks_for(nverts)), dim3(MB), 0, st, (const u64*)sums, (int)nverts, normals);
  SP3_LAUNCH_CHECK("sp3_mesh_vertex_normals");
  return 0;
}
