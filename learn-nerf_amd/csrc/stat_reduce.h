// stat_reduce.h — the fixed-order fp64 reduction shared by csrc/view_stats.hip and csrc/image_metrics.hip.
//
// Launch 1: workgroups of 256 (four wave64s), at most 1024 of them, their count a function of the problem size only.
// Every thread sums its own terms in a fixed order, the 64 lanes of a wave meet in an xor butterfly (offsets 32, 16,
// ..., 1), lane 0 of each wave leaves its value in LDS and thread 0 adds the four in wave order and writes ONE partial.
// Launch 2: one workgroup of 256; thread t combines the partials 4t, 4t+1, 4t+2, 4t+3 (< n_parts) in that order, then
// the same butterfly and the same four-wave fold, and thread 0 adds the result to the caller's accumulator.
#pragma once
#include "common.h"

namespace lnrf {

constexpr int kStatBlock = 256;
constexpr int kStatMaxGrid = 1024;
constexpr int kStatPerFoldThread = kStatMaxGrid / kStatBlock;  // partials per thread of the fold launch

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the workgroup, valid in thread 0: butterfly per wave, then the four waves in order
__device__ __forceinline__ double block_sum_f64(double v, double* s_part) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// the body of launch 2: acc[0] += the n_parts <= kStatMaxGrid partials, by one workgroup of kStatBlock
__device__ __forceinline__ void fold_partials_f64(const double* __restrict__ parts, int n_parts,
                                                  double* __restrict__ acc, double* s_part) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kStatPerFoldThread; ++k) {
    const int b = (int)threadIdx.x * kStatPerFoldThread + k;
    if (b < n_parts) s += parts[b];
  }
  const double total = block_sum_f64(s, s_part);
  if (threadIdx.x == 0) acc[0] += total;
}

}  // namespace lnrf
