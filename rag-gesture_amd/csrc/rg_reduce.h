// Fixed-order fp64 / i64 sums of the evaluation kernels (rg_fgd.hip, rg_motion.hip, rg_mesh.hip): the order of the additions
// depends on the launch shape alone, so a result's bits do not depend on what else runs.
#pragma once
#include "rg_common.h"

namespace {

// the lanes of a wave by xor butterfly: every lane gets the sum
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) { return wave_sum(v); }

// the lanes of a wave as wave_sum, then the waves in order from 0 (four waves: ((w0 + w1) + w2) + w3); red holds one value per
// wave, and every thread of the workgroup calls this (it holds two barriers, the first in front of the store into red)
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T s = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}
__device__ __forceinline__ double block_sum_f64(double v, double* red) { return block_sum(v, red); }
__device__ __forceinline__ long long block_sum_i64(long long v, long long* red) { return block_sum(v, red); }

// The greatest value held by a group of WIDTH adjacent lanes (a power of two up to 64, groups aligned to WIDTH) and the lowest
// index that comes with it, by xor butterfly: every lane of the group gets both.  The order (greater value first, then lower
// index) is total over distinct indices, so the result does not depend on which lane held which (value, index) pair.  Values
// must be numbers (the caller keeps NaN out); a lane with nothing to offer passes (-infinity, INT_MAX).
template <int WIDTH>
__device__ __forceinline__ void group_argmax_f64(double& v, int& i) {
#pragma unroll
  for (int m = WIDTH >> 1; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(i, m);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

}  // namespace
