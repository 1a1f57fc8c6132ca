// scan.h — the prefix-sum pieces radiuspairs.hip (int64 row starts) and voxelgrid.hip (uint32 voxel slots) share.  Both scan in
// two levels: per-block sums, ONE workgroup over those sums (scan_blocks below), then the rows of each block.
#pragma once
#include "common.h"

namespace prg {

constexpr int kScanThreads = 1024;   // threads of scan_blocks' one workgroup = block sums per round of its loop

// inclusive prefix sum over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_inclusive(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive scan of v[0..n) in place by ONE workgroup of kScanThreads, any n: 1024 elements per round with a running carry.
// kTotal: also write the grand total to v[n] — only for a buffer that has that entry.
template <typename T, bool kTotal>
__global__ __launch_bounds__(kScanThreads) void scan_blocks(T* __restrict__ v, int n) {
  __shared__ T wtot[kScanThreads / 64];
  __shared__ T carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int base = 0; base < n; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const T x = i < n ? v[i] : (T)0;
    const T inc = wave_inclusive(x, lane);
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    T woff = 0, all = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) {
      if (k < w) woff += wtot[k];
      all += wtot[k];
    }
    const T carry = carry_s;
    if (i < n) v[i] = carry + woff + inc - x;
    __syncthreads();
    if (threadIdx.x == 0) carry_s = carry + all;
    __syncthreads();
  }
  if (kTotal && threadIdx.x == 0) v[n] = carry_s;
}

}  // namespace prg
