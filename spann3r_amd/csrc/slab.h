// Fixed-order fp64 sums over a launch (csrc/eval.hip, csrc/raycast.hip): every thread keeps NV running sums over a grid-stride
// loop, a workgroup of 256 reduces them (wave: xor shuffles; the four waves: LDS, in wave order) into its row of a partial slab,
// and slab_finish_kernel adds the rows in index order.  No float atomics, no workgroup waits on another: the result depends on the
// launch geometry alone, which slab_blocks fixes from n.
#pragma once
#include "common.h"

namespace {

constexpr int SLAB_BLOCKS = 1024;

// NV running sums per thread -> wave (shuffles) -> workgroup (LDS, fixed order) -> slab[block][NV]
template <int NV>
__device__ __forceinline__ void block_slab(double (&v)[NV], double* __restrict__ slab) {
  __shared__ double sh[4][NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[e] += __shfl_xor(v[e], o);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < NV; ++e) sh[w][e] = v[e];
  }
  __syncthreads();
  if (threadIdx.x < NV) slab[(int64_t)blockIdx.x * NV + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void slab_finish_kernel(const double* __restrict__ slab, int blocks, int nv, double* __restrict__ out) {
  if ((int)threadIdx.x >= nv) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += slab[(int64_t)b * nv + threadIdx.x];
  out[threadIdx.x] = s;
}

inline int slab_blocks(int64_t n) { return (int)(n <= 0 ? 1 : (n + 255) / 256 < SLAB_BLOCKS ? (n + 255) / 256 : SLAB_BLOCKS); }

}  // namespace
