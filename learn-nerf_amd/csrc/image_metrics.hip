// image_metrics.hip — SSIM of two images (learn_nerf/metrics.py, scripts/eval_nerf.py): Wang et al. 2004 as the NeRF
// papers report it, in fp64 and with a FIXED order of summation, so that an evaluation prints the same digits on every run.
//
// Conventions.  a, b: fp32 [H, W, 3] in [0, 1], each channel on its own.  Window: 11 x 11 Gaussian, sigma 1.5,
// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1, applied separably (rows, then columns).  VALID region only:
// the map is [H - 10, W - 10, 3], nothing is padded.  mu_x, mu_y = filt(x), filt(y); s_xx = filt(x x) - mu_x^2, s_yy and
// s_xy likewise (population moments, negative variances are not clamped); C1 = 0.01^2, C2 = 0.03^2 (L = 1);
//   ssim = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)).
// The inputs are exact fp32 values; the taps, the products x x, y y, x y (exact in fp64), the moments, the ratio and the
// sum are all double.
//
// Passes.  A workgroup of 256 owns tiles of kSsimTH x kSsimTW = 16 x 32 map entries of ONE channel; the tiles are
// numbered (channel, tile row, tile column).  Per tile: (1) the (16 + 10) x (32 + 10) patch of both images is staged in
// LDS as fp32, zero where it leaves the image (such pixels only feed entries outside the map, which are never used);
// (2) the horizontal 11-tap pass writes the five moments of the 26 x 32 patch rows into five fp64 LDS planes; (3) thread
// t takes the entries (t / 32, t % 32) and (t / 32 + 8, t % 32), runs the vertical pass over the planes and the ratio,
// stores the entry if a map was asked for and adds it to its own sum.
// LDS: 2 * 26 * 42 * 4 = 8,736 B of patches + 5 * 26 * 33 * 8 = 34,320 B of planes + 32 B = 43,088 B static.  The plane
// pitch is 33 doubles, not 32: the 32 lanes that one ds_read_b64 group serves read 32 consecutive doubles of one plane
// row (64 distinct banks), and with the odd pitch rows r and r + 1 start two banks apart, so no mapping of lanes to
// rows puts a column's reads on one bank either.
//
// Reduction: the scheme of stat_reduce.h (csrc/view_stats.hip).  Grid = min(tiles, 1024), a function of the image size
// only; workgroup b takes the tiles b, b + grid, ... in that order and each thread sums its entries in that order, lower
// row first; xor butterfly within a wave, the four waves in order, ONE partial per workgroup in scratch; a second
// launch of one workgroup folds the partials into *acc.  No atomics, no allocation, no synchronisation with the host;
// launch 1 writes every partial that launch 2 reads.
#include <math.h>

#include "stat_reduce.h"

namespace lnrf {

constexpr int kSsimTaps = 11;
constexpr int kSsimHalo = kSsimTaps - 1;
constexpr int kSsimTH = 16, kSsimTW = 32;
constexpr int kSsimPatchH = kSsimTH + kSsimHalo, kSsimPatchW = kSsimTW + kSsimHalo;
constexpr int kSsimPitch = kSsimTW + 1;  // doubles per plane row
constexpr int kSsimPlanes = 5;           // x, y, x x, y y, x y
constexpr double kSsimC1 = 0.01 * 0.01, kSsimC2 = 0.03 * 0.03;
static_assert(kSsimTH * kSsimTW % kStatBlock == 0 && kStatBlock % kSsimTW == 0, "whole entries per thread");
static_assert(2 * kSsimPatchH * kSsimPatchW * sizeof(float) + kSsimPlanes * kSsimPatchH * kSsimPitch * sizeof(double) +
                      (kStatBlock / 64) * sizeof(double) < 64 * 1024, "static LDS stays under 64 KiB");

struct SsimTaps {
  double w[kSsimTaps];
};

static SsimTaps ssim_taps() {
  SsimTaps t;
  double sum = 0.0;
  for (int i = 0; i < kSsimTaps; ++i) {
    const double d = (double)(i - kSsimTaps / 2);
    t.w[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += t.w[i];
  }
  for (int i = 0; i < kSsimTaps; ++i) t.w[i] /= sum;
  return t;
}

struct SsimTiling {
  int tiles_x, tiles_y;
  int64_t tiles;  // 3 * tiles_y * tiles_x
};

static inline bool ssim_shape_ok(int32_t width, int32_t height) {
  return width >= kSsimTaps && height >= kSsimTaps && (int64_t)width * height <= INT32_MAX;
}

static inline SsimTiling ssim_tiling(int32_t width, int32_t height) {
  SsimTiling t;
  t.tiles_x = (width - kSsimHalo + kSsimTW - 1) / kSsimTW;
  t.tiles_y = (height - kSsimHalo + kSsimTH - 1) / kSsimTH;
  t.tiles = 3 * (int64_t)t.tiles_y * t.tiles_x;
  return t;
}

static inline int ssim_grid(const SsimTiling& t) { return (int)(t.tiles < kStatMaxGrid ? t.tiles : kStatMaxGrid); }

__global__ __launch_bounds__(kStatBlock) void ssim_partial_kernel(const float* __restrict__ a,
                                                                  const float* __restrict__ b, int width, int height,
                                                                  int tiles_x, int tiles_y, SsimTaps taps,
                                                                  double* __restrict__ ssim_map,
                                                                  double* __restrict__ parts) {
  __shared__ float s_a[kSsimPatchH * kSsimPatchW];
  __shared__ float s_b[kSsimPatchH * kSsimPatchW];
  __shared__ double s_h[kSsimPlanes][kSsimPatchH * kSsimPitch];
  __shared__ double s_part[kStatBlock / 64];
  const int tid = (int)threadIdx.x;
  const int map_w = width - kSsimHalo, map_h = height - kSsimHalo;
  const int per_channel = tiles_x * tiles_y;
  const int tiles = 3 * per_channel;
  double s = 0.0;
  for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
    const int ch = tile / per_channel, rem = tile - ch * per_channel;
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * kSsimTH, x0 = tx * kSsimTW;
    __syncthreads();  // the previous tile's patches and planes have been read
    for (int i = tid; i < kSsimPatchH * kSsimPatchW; i += kStatBlock) {
      const int y = y0 + i / kSsimPatchW, x = x0 + i % kSsimPatchW;
      const bool inside = y < height && x < width;
      const int64_t off = ((int64_t)y * width + x) * 3 + ch;
      s_a[i] = inside ? a[off] : 0.0f;
      s_b[i] = inside ? b[off] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kSsimPatchH * kSsimTW; i += kStatBlock) {
      const int pr = i / kSsimTW, c = i % kSsimTW;
      double m[kSsimPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kSsimTaps; ++k) {
        const double x = (double)s_a[pr * kSsimPatchW + c + k], y = (double)s_b[pr * kSsimPatchW + c + k];
        const double w = taps.w[k];
        m[0] = fma(w, x, m[0]);
        m[1] = fma(w, y, m[1]);
        m[2] = fma(w, x * x, m[2]);
        m[3] = fma(w, y * y, m[3]);
        m[4] = fma(w, x * y, m[4]);
      }
#pragma unroll
      for (int p = 0; p < kSsimPlanes; ++p) s_h[p][pr * kSsimPitch + c] = m[p];
    }
    __syncthreads();
    for (int e = tid; e < kSsimTH * kSsimTW; e += kStatBlock) {
      const int r = e / kSsimTW, c = e % kSsimTW;
      const int y = y0 + r, x = x0 + c;
      if (y >= map_h || x >= map_w) continue;
      double m[kSsimPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kSsimTaps; ++k) {
        const double w = taps.w[k];
#pragma unroll
        for (int p = 0; p < kSsimPlanes; ++p) m[p] = fma(w, s_h[p][(r + k) * kSsimPitch + c], m[p]);
      }
      const double mu_x = m[0], mu_y = m[1];
      const double s_xx = m[2] - mu_x * mu_x, s_yy = m[3] - mu_y * mu_y, s_xy = m[4] - mu_x * mu_y;
      const double num = (2.0 * mu_x * mu_y + kSsimC1) * (2.0 * s_xy + kSsimC2);
      const double den = (mu_x * mu_x + mu_y * mu_y + kSsimC1) * (s_xx + s_yy + kSsimC2);
      const double v = num / den;
      if (ssim_map) ssim_map[((int64_t)y * map_w + x) * 3 + ch] = v;
      s += v;
    }
  }
  const double total = block_sum_f64(s, s_part);
  if (tid == 0) parts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kStatBlock) void ssim_fold_kernel(const double* __restrict__ parts, int n_parts,
                                                               double* __restrict__ acc) {
  __shared__ double s_part[kStatBlock / 64];
  fold_partials_f64(parts, n_parts, acc, s_part);
}

}  // namespace lnrf

using namespace lnrf;

extern "C" int64_t lnrf_ssim_scratch_bytes(int32_t width, int32_t height) {
  if (!ssim_shape_ok(width, height)) return -1;
  return (int64_t)ssim_grid(ssim_tiling(width, height)) * (int64_t)sizeof(double);
}

extern "C" int lnrf_ssim_f64(const float* a, const float* b, int32_t width, int32_t height, double* ssim_map,
                             double* acc, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream) {
  if (!ssim_shape_ok(width, height)) {
    set_error("%s: images of %d x %d pixels: need width, height >= %d and width * height <= INT32_MAX", __func__, width,
              height, kSsimTaps);
    return LNRF_ERR_SHAPE;
  }
  LNRF_CHECK_ARG(a && b && acc, "null pointer");
  LNRF_CHECK_ARG(scratch && scratch_bytes >= lnrf_ssim_scratch_bytes(width, height) &&
                     (reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "scratch too small or unaligned");
  const SsimTiling t = ssim_tiling(width, height);
  const int grid = ssim_grid(t);
  double* parts = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(ssim_partial_kernel, dim3(grid), dim3(kStatBlock), 0, as_stream(stream), a, b, (int)width,
                     (int)height, t.tiles_x, t.tiles_y, ssim_taps(), ssim_map, parts);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_fold_kernel, dim3(1), dim3(kStatBlock), 0, as_stream(stream), parts, grid, acc);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
