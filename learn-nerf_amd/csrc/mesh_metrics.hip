// mesh_metrics.hip — the parts of the mesh comparison (learn_nerf/mesh_metrics.py, scripts/eval_mesh.py) that are not
// the nearest-triangle query of csrc/raycast.hip: triangle areas, stratified surface sampling, and the statistics of the
// distances.  No allocation, copy, synchronisation or atomic in any entry point; results do not depend on the launch
// geometry; every output element is written.  tests/mesh_metrics_reference.py restates all three bit for bit.
//
// Area (fp32, every operation rounded once, contraction off): e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 with components
// a.y*b.z - a.z*b.y and cyclic, nn = (n.x*n.x + n.y*n.y) + n.z*n.z, area = 0.5 * sqrt(nn) with the correctly rounded
// sqrt (hipcc's default for fp32).
//
// Sampling.  cdf [n] is the caller's float64 running sum of the areas, non-decreasing, total = cdf[n - 1] > 0: the
// kernel's bits do not depend on how a prefix sum was scheduled.  Sample i of m: u0, u1, u2 = philox_uniform(seed,
// stream, 3i + 0 / 1 / 2); x = ((double(i) + double(u0)) / double(m)) * total; j = the first index with cdf[j] > x
// (binary search), and when there is none (x rounded up to the total) the first index with cdf[j] >= total.  Either way
// cdf[j] > cdf[j - 1] (or j = 0 with cdf[0] > 0): a triangle of zero area is never chosen.  If u1 + u2 > 1 (fp32 sum)
// then (u1, u2) = (1 - u1, 1 - u2); point = (v0 + u1 * e1) + u2 * e2 per component, contraction off.  The id is
// order[j], or j without an order.  Stratum i covers [i, i + 1) / m of the total area, so triangle j receives between
// m area_j / total - 2 and m area_j / total + 2 samples, and consecutive samples lie on consecutive triangles of the
// (Morton-sorted) order: spatially coherent queries for the other mesh's tree.
//
// Statistics: the scheme of stat_reduce.h (csrc/view_stats.hip).  Grid = min(ceil(m / 256), 1024); thread t of
// workgroup b takes the elements b * 256 + t, + grid * 256, ... in that order; per quantity an xor butterfly within a
// wave, the four waves in order, one partial per workgroup in scratch[q * grid + b]; a second launch of one workgroup
// folds the partials of each quantity into acc[q].  Quantities: 0 sum of sqrt(double(d2)) (fp64 sqrt, correctly
// rounded), 1 sum of double(d2), 2 sum of |double(cosine)|, 3 max of d2 (order-independent), 4 + k the number of
// elements with sqrt(double(d2)) <= tau_k, counted in doubles.  Launch 1 writes the partials of all 4 + 8 quantities.
#include <math.h>

#include "philox.h"
#include "stat_reduce.h"

namespace lnrf {

constexpr int kMmBlock = 256;
constexpr int kMmMaxGrid = 2048;  // grid-stride beyond
constexpr int64_t kMmMaxTris = (int64_t)1 << 28;
constexpr int64_t kMmMaxSamples = (int64_t)1 << 40;
constexpr int kDistMaxThresholds = 8;
constexpr int kDistQuantities = 4 + kDistMaxThresholds;

static inline int mm_grid(int64_t n) {
  const int64_t g = (n + kMmBlock - 1) / kMmBlock;
  return (int)(g < kMmMaxGrid ? g : kMmMaxGrid);
}

static inline int dist_grid(int64_t m) {
  const int64_t g = (m + kStatBlock - 1) / kStatBlock;
  return (int)(g < kStatMaxGrid ? g : kStatMaxGrid);
}

__global__ __launch_bounds__(kMmBlock) void tri_areas_kernel(const float* __restrict__ tris, int64_t n,
                                                             float* __restrict__ areas) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * kMmBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMmBlock) {
    const float* v = tris + 9 * i;
    const float ax = v[3] - v[0], ay = v[4] - v[1], az = v[5] - v[2];
    const float bx = v[6] - v[0], by = v[7] - v[1], bz = v[8] - v[2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float nn = (nx * nx + ny * ny) + nz * nz;
    areas[i] = 0.5f * sqrtf(nn);
  }
}

__global__ __launch_bounds__(kMmBlock) void sample_surface_kernel(const float* __restrict__ tris,
                                                                  const int32_t* __restrict__ order,
                                                                  const double* __restrict__ cdf, int64_t n, int64_t m,
                                                                  uint64_t seed, uint32_t stream,
                                                                  float* __restrict__ pts, int32_t* __restrict__ ids) {
#pragma clang fp contract(off)
  const double total = cdf[n - 1];
  for (int64_t i = (int64_t)blockIdx.x * kMmBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kMmBlock) {
    const float u0 = philox_uniform(seed, stream, 3 * (uint64_t)i);
    float u1 = philox_uniform(seed, stream, 3 * (uint64_t)i + 1);
    float u2 = philox_uniform(seed, stream, 3 * (uint64_t)i + 2);
    const double x = (((double)i + (double)u0) / (double)m) * total;
    int64_t lo = 0, hi = n;  // the first j with cdf[j] > x, n if there is none
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    if (lo == n) {  // x reached the total: the first j with cdf[j] >= total
      lo = 0, hi = n - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
      }
    }
    if (u1 + u2 > 1.0f) u1 = 1.0f - u1, u2 = 1.0f - u2;
    const float* v = tris + 9 * lo;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float e1 = v[3 + a] - v[a], e2 = v[6 + a] - v[a];
      pts[3 * i + a] = (v[a] + u1 * e1) + u2 * e2;
    }
    ids[i] = order ? order[lo] : (int32_t)lo;
  }
}

struct DistThresholds {
  double tau[kDistMaxThresholds];
};

__global__ __launch_bounds__(kStatBlock) void dist_stats_partial_kernel(const float* __restrict__ d2,
                                                                        const float* __restrict__ cosine, int64_t m,
                                                                        DistThresholds th, int n_th,
                                                                        double* __restrict__ parts) {
  __shared__ double s_part[kDistQuantities][kStatBlock / 64];
  double s_dist = 0.0, s_d2 = 0.0, s_cos = 0.0, count[kDistMaxThresholds];
  float mx = 0.0f;
#pragma unroll
  for (int k = 0; k < kDistMaxThresholds; ++k) count[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kStatBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kStatBlock) {
    const float v = d2[i];
    const double dist = sqrt((double)v);
    s_dist += dist;
    s_d2 += (double)v;
    if (cosine) s_cos += fabs((double)cosine[i]);
    mx = fmaxf(mx, v);
#pragma unroll
    for (int k = 0; k < kDistMaxThresholds; ++k)
      if (k < n_th && dist <= th.tau[k]) count[k] += 1.0;
  }
  double total[kDistQuantities];
  total[0] = block_sum_f64(s_dist, s_part[0]);
  total[1] = block_sum_f64(s_d2, s_part[1]);
  total[2] = block_sum_f64(s_cos, s_part[2]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if ((threadIdx.x & 63) == 0) s_part[3][threadIdx.x >> 6] = (double)mx;
  __syncthreads();
  total[3] = fmax(fmax(s_part[3][0], s_part[3][1]), fmax(s_part[3][2], s_part[3][3]));
#pragma unroll
  for (int k = 0; k < kDistMaxThresholds; ++k) total[4 + k] = block_sum_f64(count[k], s_part[4 + k]);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kDistQuantities; ++q) parts[(int64_t)q * gridDim.x + blockIdx.x] = total[q];
  }
}

__global__ __launch_bounds__(kStatBlock) void dist_stats_fold_kernel(const double* __restrict__ parts, int n_parts,
                                                                     int with_cosine, int n_th,
                                                                     double* __restrict__ acc) {
  __shared__ double s_part[kDistQuantities][kStatBlock / 64];
  for (int q = 0; q < 4 + n_th; ++q) {
    if (q == 3 || (q == 2 && !with_cosine)) continue;
    fold_partials_f64(parts + (int64_t)q * n_parts, n_parts, acc + q, s_part[q]);
  }
  double mx = 0.0;
  for (int b = (int)threadIdx.x; b < n_parts; b += kStatBlock) mx = fmax(mx, parts[(int64_t)3 * n_parts + b]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if ((threadIdx.x & 63) == 0) s_part[3][threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0)
    acc[3] = fmax(acc[3], fmax(fmax(s_part[3][0], s_part[3][1]), fmax(s_part[3][2], s_part[3][3])));
}

}  // namespace lnrf

using namespace lnrf;

extern "C" int lnrf_mesh_tri_areas(const float* tris, int64_t n, float* areas, lnrf_stream_t stream) {
  if (n < 0 || n > kMmMaxTris) {
    set_error("%s: %lld triangles: need 0 <= n <= 2^28", __func__, (long long)n);
    return LNRF_ERR_SHAPE;
  }
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris && areas, "null pointer");
  hipLaunchKernelGGL(tri_areas_kernel, dim3(mm_grid(n)), dim3(kMmBlock), 0, as_stream(stream), tris, n, areas);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_mesh_sample_surface(const float* tris, const int32_t* order, const double* cdf, int64_t n,
                                        int64_t m, uint64_t seed, uint32_t stream_id, float* pts, int32_t* ids,
                                        lnrf_stream_t stream) {
  if (n < 1 || n > kMmMaxTris || m < 0 || m >= kMmMaxSamples) {
    set_error("%s: %lld samples of %lld triangles: need 1 <= n <= 2^28 and 0 <= m < 2^40", __func__, (long long)m,
              (long long)n);
    return LNRF_ERR_SHAPE;
  }
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris && cdf && pts && ids, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)cdf & 7) == 0, "cdf must be 8-byte aligned");
  hipLaunchKernelGGL(sample_surface_kernel, dim3(mm_grid(m)), dim3(kMmBlock), 0, as_stream(stream), tris, order, cdf,
                     n, m, seed, stream_id, pts, ids);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int64_t lnrf_dist_stats_scratch_bytes(int64_t m) {
  if (m < 0) return -1;
  return (int64_t)dist_grid(m) * kDistQuantities * (int64_t)sizeof(double);
}

extern "C" int lnrf_dist_stats_f64(const float* d2, const float* cosine, int64_t m, const double* thresholds,
                                   int32_t n_thresholds, double* acc, void* scratch, int64_t scratch_bytes,
                                   lnrf_stream_t stream) {
  LNRF_CHECK_ARG(m >= 0, "negative element count");
  if (n_thresholds < 0 || n_thresholds > kDistMaxThresholds) {
    set_error("%s: %d thresholds: need between 0 and %d", __func__, n_thresholds, kDistMaxThresholds);
    return LNRF_ERR_SHAPE;
  }
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(d2 && acc && (thresholds || n_thresholds == 0), "null pointer");
  LNRF_CHECK_ARG(scratch && scratch_bytes >= lnrf_dist_stats_scratch_bytes(m) &&
                     (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "scratch too small or unaligned");
  DistThresholds th;
  for (int k = 0; k < kDistMaxThresholds; ++k) th.tau[k] = k < n_thresholds ? thresholds[k] : 0.0;
  const int grid = dist_grid(m);
  double* parts = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(dist_stats_partial_kernel, dim3(grid), dim3(kStatBlock), 0, as_stream(stream), d2, cosine, m, th,
                     (int)n_thresholds, parts);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(dist_stats_fold_kernel, dim3(1), dim3(kStatBlock), 0, as_stream(stream), parts, grid,
                     cosine ? 1 : 0, (int)n_thresholds, acc);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
