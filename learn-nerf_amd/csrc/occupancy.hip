// occupancy.hip — occupancy grid of a trained model for the inference renderer: build the bitfield from corner
// densities, clip the rays' (t_min, t_max, mask) to the occupied cells, compact the live rays of a batch and scatter
// their rows back.  Additive: no counterpart in the reference, which evaluates every sample of every ray.
//
// Conventions (learn_nerf/occupancy.py and the NumPy restatement tests/occupancy_reference.py rely on them):
//   sigma     fp32 [(R+1)^3], the density at the cell-corner lattice in C order (mesh.density_grid at R + 1): cell
//             (i, j, k) has the corners (i + di, j + dj, k + dk), di, dj, dk in {0, 1}.
//   raw       a cell is raw-occupied iff some corner has NOT (sigma < sigma_thr), which is NOT (max of the 8 corners <
//             sigma_thr) with NaN and +inf corners occupying the cell; sigma_thr = 0 occupies every cell of a
//             non-negative density (and of any density short of a negative one at all 8 corners).
//   occupied  iff a raw-occupied cell lies within Chebyshev distance `dilate`.
//   bits      uint32 [ceil(R^3 / 32)]: cell idx = (i*R + j)*R + k is bit idx & 31 of word idx >> 5, the unused bits of
//             the last word are zero.  count: the number of occupied cells (integer partial sums per workgroup, folded
//             by one workgroup in a fixed order; no atomics).
//   clip      occ_geom.h (the per-ray walk and the derivation of its pad), one ray per lane.
//   compact   idx[0..count) = the indices of the non-zero mask bytes in ascending order, count as one int64: one
//             workgroup scans the mask in rounds of kScanBlock bytes, so the order is fixed by construction.
//   scatter   out[idx[i], :] = src[i, :], the inverse of lnrf_gather_rows; an index outside [0, n_out) is skipped,
//             rows of out that idx does not name are not touched, and idx must not name a row twice.
#include "common.h"
#include "occ_geom.h"

namespace lnrf {
namespace occ {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kScanBlock = 1024;

struct Layout {
  int64_t raw, partials, bytes;
};

static inline Layout occ_layout(int64_t res) {
  Layout l;
  l.raw = 0;                                             // uint8 [R^3]
  l.partials = (res * res * res + 255) & ~(int64_t)255;  // int64 [kMaxGrid]
  l.bytes = l.partials + (int64_t)kMaxGrid * 8;
  return l;
}

__global__ __launch_bounds__(kBlock) void occ_raw_kernel(const float* __restrict__ sigma, int res, float thr,
                                                         uint8_t* __restrict__ raw) {
  const int64_t r2 = (int64_t)res * res, n = r2 * res, p1 = res + 1, p2 = p1 * p1;
  for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kBlock) {
    const int64_t i = idx / r2, rem = idx - i * r2, j = rem / res, k = rem - j * res;
    const float* s = sigma + (i * p1 + j) * p1 + k;
    bool on = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) on |= !(s[(c >> 2) * p2 + ((c >> 1) & 1) * p1 + (c & 1)] < thr);
    raw[idx] = on ? 1 : 0;
  }
}

// one lane per cell: the wave's ballot is two words of the bitfield
__global__ __launch_bounds__(kBlock) void occ_pack_kernel(const uint8_t* __restrict__ raw, int res, int dilate,
                                                          uint32_t* __restrict__ bits, int64_t nwords,
                                                          int64_t* __restrict__ partials) {
  __shared__ int64_t red[kBlock / 64];
  const int64_t r2 = (int64_t)res * res, n = r2 * res;
  const int lane = threadIdx.x & 63;
  int64_t mine = 0;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < nwords * 32; base += (int64_t)gridDim.x * kBlock) {
    const int64_t idx = base + threadIdx.x;
    bool on = false;
    if (idx < n) {
      const int i = (int)(idx / r2), j = (int)((idx - i * r2) / res), k = (int)(idx - i * r2 - (int64_t)j * res);
      const int i0 = max(i - dilate, 0), i1 = min(i + dilate, res - 1);
      const int j0 = max(j - dilate, 0), j1 = min(j + dilate, res - 1);
      const int k0 = max(k - dilate, 0), k1 = min(k + dilate, res - 1);
      for (int ii = i0; ii <= i1 && !on; ++ii)
        for (int jj = j0; jj <= j1 && !on; ++jj) {
          const uint8_t* row = raw + (ii * r2 + (int64_t)jj * res);
          for (int kk = k0; kk <= k1; ++kk) on |= row[kk] != 0;
        }
    }
    const unsigned long long vote = __ballot(on);
    const int64_t word = idx >> 5;  // lane 0 and lane 32 each start a word
    if (lane == 0 && word < nwords) bits[word] = (uint32_t)vote;
    if (lane == 32 && word < nwords) bits[word] = (uint32_t)(vote >> 32);
    mine += on ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (lane == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int w = 0; w < kBlock / 64; ++w) s += red[w];
    partials[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void occ_count_fold_kernel(const int64_t* __restrict__ partials, int nblocks,
                                                                int64_t* __restrict__ count) {
  __shared__ int64_t red[kBlock];
  int64_t s = 0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) s += partials[b];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = red[0];
}

__global__ __launch_bounds__(kBlock) void occ_clip_rays_kernel(const float* __restrict__ rays, int64_t ray_stride,
                                                               int64_t n_rays, BBox bb, int res,
                                                               const uint32_t* __restrict__ bits, float min_t_range,
                                                               float eps, const float* t_min, const float* t_max,
                                                               const uint8_t* mask, float* t_min_out, float* t_max_out,
                                                               uint8_t* mask_out) {
  // the inputs may alias the outputs: every lane reads its ray's triple before it writes it
  for (int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x; n < n_rays; n += (int64_t)gridDim.x * kBlock) {
    const TRange r = occ_clip_ray(rays + n * ray_stride, bb.mn, bb.mx, res, bits, min_t_range, eps, t_min[n], t_max[n],
                                  mask[n] != 0);
    t_min_out[n] = r.t_min;
    t_max_out[n] = r.t_max;
    mask_out[n] = r.mask ? 1 : 0;
  }
}

__global__ __launch_bounds__(kScanBlock) void compact_mask_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                  int32_t* __restrict__ idx,
                                                                  int64_t* __restrict__ count) {
  __shared__ int lds[kScanBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += kScanBlock) {
    const int64_t e = base + threadIdx.x;
    const int v = (e < n && mask[e] != 0) ? 1 : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < kScanBlock / 64; ++i) {
      const int s = lds[i];
      before += i < w ? s : 0;
      total += s;
    }
    __syncthreads();  // lds is reused by the next round
    if (v) idx[carry + before + inc - 1] = (int32_t)e;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kBlock) void scatter_rows_kernel(const float* __restrict__ src, int row_floats,
                                                              const int32_t* __restrict__ idx, int64_t n,
                                                              float* __restrict__ out, int64_t n_out) {
  const int64_t total = n * row_floats;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t i = e / row_floats;
    const int f = (int)(e - i * row_floats);
    const int64_t r = idx[i];
    if (r >= 0 && r < n_out) out[r * row_floats + f] = src[e];
  }
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < 1 ? 1 : (blocks < kMaxGrid ? blocks : kMaxGrid));
}

static int check_res(const char* fn, int32_t res) {
  if (res < 1 || res > kMaxRes) {
    set_error("%s: resolution %d must lie in [1, %d]", fn, res, kMaxRes);
    return LNRF_ERR_SHAPE;
  }
  return LNRF_OK;
}

}  // namespace occ
}  // namespace lnrf

using namespace lnrf;

extern "C" int64_t lnrf_occ_scratch_bytes(int32_t resolution) {
  if (resolution < 1 || resolution > occ::kMaxRes) return -1;
  return occ::occ_layout(resolution).bytes;
}

extern "C" int lnrf_occ_build(const float* sigma, int32_t resolution, float sigma_thr, int32_t dilate, uint32_t* bits,
                              int64_t* count, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream) {
  const int rc = occ::check_res(__func__, resolution);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(sigma && bits && count && scratch, "null pointer");
  LNRF_CHECK_ARG(dilate >= 0, "dilate must be >= 0");
  LNRF_CHECK_ARG(!(sigma_thr != sigma_thr), "sigma_thr is NaN");
  const occ::Layout l = occ::occ_layout(resolution);
  LNRF_CHECK_ARG(scratch_bytes >= l.bytes && ((uintptr_t)scratch & 15) == 0, "scratch too small or unaligned");
  const int64_t n = (int64_t)resolution * resolution * resolution, nwords = (n + 31) / 32;
  uint8_t* raw = (uint8_t*)scratch + l.raw;
  int64_t* partials = (int64_t*)((char*)scratch + l.partials);
  const int reach = dilate < resolution - 1 ? dilate : resolution - 1;  // no two cells are further apart
  hipLaunchKernelGGL(occ::occ_raw_kernel, dim3(occ::grid_for(n)), dim3(occ::kBlock), 0, as_stream(stream), sigma,
                     (int)resolution, sigma_thr, raw);
  LNRF_LAUNCH_CHECK();
  const int blocks = occ::grid_for(nwords * 32);
  hipLaunchKernelGGL(occ::occ_pack_kernel, dim3(blocks), dim3(occ::kBlock), 0, as_stream(stream), raw,
                     (int)resolution, reach, bits, nwords, partials);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(occ::occ_count_fold_kernel, dim3(1), dim3(occ::kBlock), 0, as_stream(stream), partials, blocks,
                     count);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_occ_clip_rays(const float* rays, int64_t ray_stride, int64_t n_rays, const float* bbox_min,
                                  const float* bbox_max, const uint32_t* bits, int32_t resolution, float min_t_range,
                                  float epsilon, const float* t_min, const float* t_max, const uint8_t* mask,
                                  float* t_min_out, float* t_max_out, uint8_t* mask_out, lnrf_stream_t stream) {
  const int rc = occ::check_res(__func__, resolution);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(n_rays >= 0 && ray_stride >= 6, "bad sizes");
  LNRF_CHECK_ARG(bbox_min && bbox_max, "null bbox");
  BBox bb;
  for (int a = 0; a < 3; ++a) {
    bb.mn[a] = bbox_min[a];
    bb.mx[a] = bbox_max[a];
    // a positive finite cell edge on every axis
    LNRF_CHECK_ARG(bb.mx[a] > bb.mn[a] && std::isfinite(bb.mx[a] - bb.mn[a]), "the box needs max > min, both finite");
  }
  if (n_rays == 0) return LNRF_OK;
  LNRF_CHECK_ARG(rays && bits && t_min && t_max && mask && t_min_out && t_max_out && mask_out, "null pointer");
  hipLaunchKernelGGL(occ::occ_clip_rays_kernel, dim3(occ::grid_for(n_rays)), dim3(occ::kBlock), 0, as_stream(stream),
                     rays, ray_stride, n_rays, bb, (int)resolution, bits, min_t_range, epsilon, t_min, t_max, mask,
                     t_min_out, t_max_out, mask_out);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_compact_mask(const uint8_t* mask, int64_t n, int32_t* idx, int64_t* count, lnrf_stream_t stream) {
  LNRF_CHECK_ARG(n >= 0 && count, "bad sizes or null count");
  if (n > INT32_MAX) {
    set_error("%s: %lld entries do not fit in int32 indices", __func__, (long long)n);
    return LNRF_ERR_SHAPE;
  }
  LNRF_CHECK_ARG(n == 0 || (mask && idx), "null pointer");
  hipLaunchKernelGGL(occ::compact_mask_kernel, dim3(1), dim3(occ::kScanBlock), 0, as_stream(stream), mask, n, idx,
                     count);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_scatter_rows(const float* src, int32_t row_floats, const int32_t* idx, int64_t n, float* out,
                                 int64_t n_out, lnrf_stream_t stream) {
  LNRF_CHECK_ARG(n >= 0 && n_out >= 0 && row_floats >= 1, "bad sizes");
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(src && idx && out, "null pointer");
  hipLaunchKernelGGL(occ::scatter_rows_kernel, dim3(occ::grid_for(n * row_floats)), dim3(occ::kBlock), 0,
                     as_stream(stream), src, (int)row_floats, idx, n, out, n_out);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
