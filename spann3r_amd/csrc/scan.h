// Order-preserving compaction in plain multi-launch form, shared by csrc/mesh.hip (faces, vertices), csrc/views.hip (the masked
// clouds of the evaluation) and csrc/fusion.hip (surface vertices and faces of a TSDF volume): one count per 256-element tile
// (block_rank, or block_excl_sum where an element gives several), one single-workgroup exclusive scan of the counts (k_tile_scan),
// one scatter to offsets[tile] + rank.  No workgroup waits on another; the launch boundaries are the only hand-offs.
// Integer work only.  Everything here is per translation unit (anonymous namespace).
#pragma once
#include "common.h"

#define MB 256              // threads of every tile kernel = elements of one scan tile
#define SCAN_T 1024         // threads of the single-workgroup scan

namespace {

// rank of this lane's flag among the block's flags (exclusive) and the block's total; every thread of the block calls it
__device__ __forceinline__ int block_rank(bool flag, int& total) {
  __shared__ int wsum[MB / SP3_WAVE];
  const unsigned long long b = __ballot(flag);
  const int lane = threadIdx.x & (SP3_WAVE - 1), wave = threadIdx.x / SP3_WAVE;
  const int below = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < MB / SP3_WAVE; ++i) {
    if (i < wave) base += wsum[i];
    sum += wsum[i];
  }
  total = sum;
  return base + below;
}

// the same for a small count per lane instead of a flag (csrc/fusion.hip: vertices per voxel, faces per cell): the exclusive sum of
// `v` over the lanes below this one and the block's total; every thread of the block calls it
__device__ __forceinline__ int block_excl_sum(int v, int& total) {
  __shared__ int wtot[MB / SP3_WAVE];
  const int lane = threadIdx.x & (SP3_WAVE - 1), wave = threadIdx.x / SP3_WAVE;
  int inc = v;
#pragma unroll
  for (int o = 1; o < SP3_WAVE; o <<= 1) {
    const int up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  if (lane == SP3_WAVE - 1) wtot[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < MB / SP3_WAVE; ++i) {
    if (i < wave) base += wtot[i];
    sum += wtot[i];
  }
  total = sum;
  return base + inc - v;
}

// counts[0..nb) -> exclusive offsets in place, counts[nb] = total; info[0] = total and, for nseg segments of tps tiles each,
// info[1 + s] = the sum of segment s.  One workgroup; thread i owns the `per` consecutive counts from i * per.
__global__ __launch_bounds__(SCAN_T) void k_tile_scan(int* __restrict__ counts, int nb, int per, int* __restrict__ info, int nseg, int tps) {
  __shared__ int part[SCAN_T];
  const int i = threadIdx.x;
  const int lo = min(i * per, nb), hi = min(lo + per, nb);
  int s = 0;
  for (int j = lo; j < hi; ++j) s += counts[j];
  part[i] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {      // inclusive scan of the 1024 partial sums
    const int v = i >= d ? part[i - d] : 0;
    __syncthreads();
    part[i] += v;
    __syncthreads();
  }
  int run = part[i] - s;
  for (int j = lo; j < hi; ++j) {
    const int c = counts[j];
    counts[j] = run;
    run += c;
  }
  if (i == SCAN_T - 1) {
    counts[nb] = part[i];
    info[0] = part[i];
  }
  __syncthreads();
  for (int sg = i; sg < nseg; sg += SCAN_T) info[1 + sg] = tps > 0 ? counts[(sg + 1) * tps] - counts[sg * tps] : 0;
}

}  // namespace
