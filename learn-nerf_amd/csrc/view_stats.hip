// view_stats.hip — dataset diagnostics (scripts/cv_nerf.py, scripts/check_bbox.py): two whole-view reductions with a
// FIXED order, so that a tool which ranks views prints the same digits on every run.
//
// Both follow one scheme.  Launch 1: workgroups of 256 (four wave64s), grid = min(ceil(n / 256), 1024) — a function of
// the problem size only, never of the device.  Thread t of workgroup b accumulates the elements b*256 + t,
// + grid*256, ... in registers, the 64 lanes of a wave meet in an xor butterfly (offsets 32, 16, ..., 1), lane 0 of each
// wave leaves its value in LDS and thread 0 adds the four in wave order and writes ONE partial to scratch[b].
// Launch 2: one workgroup of 256; thread t combines the partials 4t, 4t+1, 4t+2, 4t+3 (< grid) in that order, then the
// same butterfly and the same four-wave fold, and thread 0 combines the result into the caller's accumulator.
// No atomics, no allocation, no synchronisation with the host; launch 1 writes every partial that launch 2 reads.
// The constants, the butterfly and the fp64 fold are in stat_reduce.h, which csrc/image_metrics.hip shares.
#include "ray_geom.h"
#include "stat_reduce.h"

namespace lnrf {

static inline int stat_grid(int64_t n) {
  const int64_t g = (n + kStatBlock - 1) / kStatBlock;
  return (int)(g < kStatMaxGrid ? g : kStatMaxGrid);
}

// ---------------------------------------------------------------------------------------
// sum_n sum_c (double(outputs[n,c]) - double(targets[n*stride + c]))^2: the numerator of train.py:141-142 in fp64.
__global__ __launch_bounds__(kStatBlock) void sq_err_partial_kernel(const float* __restrict__ outputs,
                                                                    const float* __restrict__ targets,
                                                                    int64_t target_stride, int64_t n,
                                                                    float* __restrict__ ray_err,
                                                                    double* __restrict__ parts) {
  __shared__ double s_part[kStatBlock / 64];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kStatBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kStatBlock) {
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double df = (double)outputs[i * 3 + c] - (double)targets[i * target_stride + c];
      e += df * df;
    }
    if (ray_err) ray_err[i] = (float)e;
    s += e;
  }
  const double total = block_sum_f64(s, s_part);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kStatBlock) void sq_err_fold_kernel(const double* __restrict__ parts, int n_parts,
                                                                 double* __restrict__ acc) {
  __shared__ double s_part[kStatBlock / 64];
  fold_partials_f64(parts, n_parts, acc, s_part);
}

// ---------------------------------------------------------------------------------------
// Pixels whose ray misses the scene box (scripts/check_bbox.py:31-46): count, channel sums, minima and maxima of the
// uint8 image over them.  Integers throughout: exact, and independent of the order of combination.
struct MissStats {
  unsigned long long count, sum[3];
  int mn[3], mx[3];
};

__device__ __forceinline__ MissStats miss_identity() {
  MissStats m;
  m.count = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    m.sum[c] = 0;
    m.mn[c] = 255;
    m.mx[c] = 0;
  }
  return m;
}

__device__ __forceinline__ void miss_combine(MissStats& a, const MissStats& b) {
  a.count += b.count;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.sum[c] += b.sum[c];
    a.mn[c] = min(a.mn[c], b.mn[c]);
    a.mx[c] = max(a.mx[c], b.mx[c]);
  }
}

__device__ __forceinline__ MissStats miss_shfl_xor(const MissStats& a, int off) {
  MissStats b;
  b.count = __shfl_xor(a.count, off, 64);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b.sum[c] = __shfl_xor(a.sum[c], off, 64);
    b.mn[c] = __shfl_xor(a.mn[c], off, 64);
    b.mx[c] = __shfl_xor(a.mx[c], off, 64);
  }
  return b;
}

// the workgroup's combination, valid in thread 0
__device__ __forceinline__ MissStats block_miss(MissStats m, MissStats* s_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) miss_combine(m, miss_shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = m;
  __syncthreads();
  MissStats total = s_part[0];
#pragma unroll
  for (int w = 1; w < kStatBlock / 64; ++w) miss_combine(total, s_part[w]);
  return total;
}

constexpr int kMissWords = 10;  // int64 words per partial and in `stats`: count, sum[3], min[3], max[3]

__device__ __forceinline__ void miss_store(const MissStats& m, long long* __restrict__ out) {
  out[0] = (long long)m.count;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[1 + c] = (long long)m.sum[c];
    out[4 + c] = m.mn[c];
    out[7 + c] = m.mx[c];
  }
}

__global__ __launch_bounds__(kStatBlock) void view_miss_partial_kernel(Camera cam, int width, int height,
                                                                       const uint8_t* __restrict__ image, BBox bb,
                                                                       float min_t_range, float eps,
                                                                       uint8_t* __restrict__ miss,
                                                                       long long* __restrict__ parts) {
  __shared__ MissStats s_part[kStatBlock / 64];
  const int64_t total = (int64_t)width * height;
  MissStats m = miss_identity();
  for (int64_t e = (int64_t)blockIdx.x * kStatBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kStatBlock) {
    const int py = (int)(e / width), px = (int)(e - (int64_t)py * width);
    float ray[6];
    camera_pixel_ray(cam, width, height, px, py, ray);
    const bool hit = ray_t_range(ray, bb.mn, bb.mx, min_t_range, eps).mask;
    if (miss) miss[e] = hit ? 0 : 1;
    if (!hit) {
      m.count += 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v = image[e * 3 + c];
        m.sum[c] += (unsigned long long)v;
        m.mn[c] = min(m.mn[c], v);
        m.mx[c] = max(m.mx[c], v);
      }
    }
  }
  const MissStats all = block_miss(m, s_part);
  if (threadIdx.x == 0) miss_store(all, parts + (int64_t)blockIdx.x * kMissWords);
}

__global__ __launch_bounds__(kStatBlock) void view_miss_fold_kernel(const long long* __restrict__ parts, int n_parts,
                                                                    long long* __restrict__ stats) {
  __shared__ MissStats s_part[kStatBlock / 64];
  MissStats m = miss_identity();
#pragma unroll
  for (int k = 0; k < kStatPerFoldThread; ++k) {
    const int b = (int)threadIdx.x * kStatPerFoldThread + k;
    if (b < n_parts) {
      const long long* p = parts + (int64_t)b * kMissWords;
      MissStats o;
      o.count = (unsigned long long)p[0];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        o.sum[c] = (unsigned long long)p[1 + c];
        o.mn[c] = (int)p[4 + c];
        o.mx[c] = (int)p[7 + c];
      }
      miss_combine(m, o);
    }
  }
  const MissStats all = block_miss(m, s_part);
  if (threadIdx.x == 0) {
    stats[0] += (long long)all.count;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      stats[1 + c] += (long long)all.sum[c];
      stats[4 + c] = min(stats[4 + c], (long long)all.mn[c]);
      stats[7 + c] = max(stats[7 + c], (long long)all.mx[c]);
    }
  }
}

}  // namespace lnrf

using namespace lnrf;

extern "C" int64_t lnrf_sq_err_scratch_bytes(int64_t n) {
  return n < 0 ? -1 : (int64_t)stat_grid(n) * (int64_t)sizeof(double);
}

extern "C" int lnrf_sq_err_f64(const float* outputs, const float* targets, int64_t target_stride, int64_t n,
                               float* ray_err, double* acc, void* scratch, int64_t scratch_bytes,
                               lnrf_stream_t stream) {
  LNRF_CHECK_ARG(n >= 0, "negative n");
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(outputs && targets && acc, "null pointer");
  LNRF_CHECK_ARG(target_stride >= 3, "target_stride < 3");
  LNRF_CHECK_ARG(scratch && scratch_bytes >= lnrf_sq_err_scratch_bytes(n) &&
                     (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "scratch too small or unaligned");
  const int grid = stat_grid(n);
  double* parts = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(sq_err_partial_kernel, dim3(grid), dim3(kStatBlock), 0, as_stream(stream), outputs, targets,
                     target_stride, n, ray_err, parts);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(sq_err_fold_kernel, dim3(1), dim3(kStatBlock), 0, as_stream(stream), parts, grid, acc);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

// LNRF_ERR_SHAPE unless 1 <= width, height and width * height <= INT32_MAX
static int check_view_shape(const char* fn, int32_t width, int32_t height) {
  if (width < 1 || height < 1 || (int64_t)width * height > INT32_MAX) {
    set_error("%s: a view of %d x %d pixels: need width, height >= 1 and width * height <= INT32_MAX", fn, width, height);
    return LNRF_ERR_SHAPE;
  }
  return LNRF_OK;
}

extern "C" int64_t lnrf_view_miss_scratch_bytes(int32_t width, int32_t height) {
  if (width < 1 || height < 1 || (int64_t)width * height > INT32_MAX) return -1;
  return (int64_t)stat_grid((int64_t)width * height) * kMissWords * (int64_t)sizeof(long long);
}

extern "C" int lnrf_view_miss_stats(const float* origin, const float* x_axis, const float* y_axis,
                                    const float* z_axis, float x_fov, float y_fov, int32_t width, int32_t height,
                                    const uint8_t* image, const float* bbox_min, const float* bbox_max,
                                    float min_t_range, float epsilon, uint8_t* miss, int64_t* stats, void* scratch,
                                    int64_t scratch_bytes, lnrf_stream_t stream) {
  if (int rc = check_view_shape(__func__, width, height)) return rc;
  LNRF_CHECK_ARG(origin && x_axis && y_axis && z_axis && bbox_min && bbox_max, "null camera / box");
  LNRF_CHECK_ARG(image && stats, "null image / stats");
  LNRF_CHECK_ARG(scratch && scratch_bytes >= lnrf_view_miss_scratch_bytes(width, height) &&
                     (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "scratch too small or unaligned");
  static_assert(sizeof(long long) == sizeof(int64_t), "stats words are 64-bit");
  const Camera cam = make_camera(origin, x_axis, y_axis, z_axis, x_fov, y_fov);
  BBox bb;
  for (int a = 0; a < 3; ++a) {
    bb.mn[a] = bbox_min[a];
    bb.mx[a] = bbox_max[a];
  }
  const int grid = stat_grid((int64_t)width * height);
  long long* parts = reinterpret_cast<long long*>(scratch);
  hipLaunchKernelGGL(view_miss_partial_kernel, dim3(grid), dim3(kStatBlock), 0, as_stream(stream), cam, (int)width,
                     (int)height, image, bb, min_t_range, epsilon, miss, parts);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(view_miss_fold_kernel, dim3(1), dim3(kStatBlock), 0, as_stream(stream), parts, grid,
                     reinterpret_cast<long long*>(stats));
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
