// texture.hip — the texture atlas of learn_nerf/texture.py: per-texel geometry, atlas coordinates of surface points,
// bilinear sampling, and the resolve and hole-filling passes that turn the baked state into an image.  Additive: no
// counterpart in the reference.  The layout, the no-bleed argument and every operation are tex_geom.h, whose header fixes
// the conventions; tests/texture_reference.py restates them in NumPy.  The bake itself (lnrf_tex_bake_views) walks the
// ray caster's tree and lives beside it in raycast.hip.
//
// Passes
//   texels   one lane per texel, a wave per tile of 8 x 8 texels (a tile lies in at most four cells, so a wave reads
//            the vertices of a few faces); outputs that are NULL are not written.
//   uv       one lane per surface point.
//   sample   one lane per sample; the four taps are element-granular gathers.
//   resolve  one lane per texel, linear: 16 B of state in, 4 B out.
//   fill     one lane per texel, linear, ping-pong between two images; the number of texels filled is counted per wave,
//            one integer atomic each, into a counter that the host reads after the last pass.
//
// No entry point allocates, copies or synchronises.
#include <limits.h>

#include "common.h"
#include "tex_geom.h"

static_assert(sizeof(lnrf_tex_view) == 64, "learn_nerf/texture.py packs lnrf_tex_view as 64 bytes");
static_assert(sizeof(lnrf_tex_atlas) == 16, "learn_nerf/_lib.py declares lnrf_tex_atlas as 16 bytes");

namespace lnrf {
namespace tex {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kTile = 8;        // a wave's tile is kTile^2 = 64 texels
static_assert(kTile * kTile == kWave, "one texel per lane");

__global__ __launch_bounds__(kBlock) void tex_texels_kernel(Atlas at, const float* __restrict__ tris,
                                                            int32_t* __restrict__ face, float* __restrict__ position,
                                                            float* __restrict__ normal, float* __restrict__ bary) {
  const int lane = threadIdx.x & (kWave - 1);
  const int tiles_x = (at.size + kTile - 1) / kTile;
  const int tiles = tiles_x * tiles_x;
  const int first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave));
  for (int tile = first; tile < tiles; tile += gridDim.x * (kBlock / kWave)) {
    const int x = (tile % tiles_x) * kTile + (lane & (kTile - 1)), y = (tile / tiles_x) * kTile + lane / kTile;
    if (x >= at.size || y >= at.size) continue;
    const int64_t o = (int64_t)y * at.size + x;
    int i, j;
    const int f = texel_face(at, x, y, &i, &j);
    float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f}, w[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0) {
      const Frame fr = face_frame(tris + 9 * (int64_t)f);
      float bb, bc;
      texel_bary(at.cell, f & 1, i, j, bb, bc);
      surface_point(fr, bb, bc, p);
      unit_normal(fr, n);
      bary_in_face_order(fr, bb, bc, w);
    }
    face[o] = f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (position) position[3 * o + k] = p[k];
      if (normal) normal[3 * o + k] = n[k];
      if (bary) bary[3 * o + k] = w[k];
    }
  }
}

__global__ __launch_bounds__(kBlock) void tex_uv_kernel(Atlas at, const float* __restrict__ tris,
                                                        const float* __restrict__ points,
                                                        const int32_t* __restrict__ ids, int64_t m,
                                                        float* __restrict__ uv) {
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < m; s += (int64_t)gridDim.x * kBlock) {
    const int f = ids[s];
    float out[2] = {NAN, NAN};
    if (f >= 0 && f < at.faces) {
      const float q[3] = {points[3 * s], points[3 * s + 1], points[3 * s + 2]};
      point_uv(at, f, face_frame(tris + 9 * (int64_t)f), q, out);
    }
    uv[2 * s] = out[0];
    uv[2 * s + 1] = out[1];
  }
}

template <class T>
__global__ __launch_bounds__(kBlock) void tex_sample_kernel(const T* __restrict__ texture, int height, int width,
                                                            const float* __restrict__ uv, int64_t m,
                                                            float* __restrict__ out) {
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < m; s += (int64_t)gridDim.x * kBlock) {
    int i0, i1, j0, j1;
    float tx, ty;
    tap_at(uv[2 * s] - 0.5f, width, i0, i1, tx);
    tap_at(uv[2 * s + 1] - 0.5f, height, j0, j1, ty);
    const T* r0 = texture + 3 * (int64_t)j0 * width;
    const T* r1 = texture + 3 * (int64_t)j1 * width;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      out[3 * s + k] = bilerp((float)r0[3 * i0 + k], (float)r0[3 * i1 + k], (float)r1[3 * i0 + k], (float)r1[3 * i1 + k],
                              tx, ty);
  }
}

__global__ __launch_bounds__(kBlock) void tex_resolve_kernel(int64_t n, const float4* __restrict__ state, uint8_t ur,
                                                             uint8_t ug, uint8_t ub, uint8_t* __restrict__ rgb,
                                                             uint8_t* __restrict__ seen) {
  for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < n; o += (int64_t)gridDim.x * kBlock) {
    const float4 st = state[o];
    const bool has = st.w > 0.0f;
    rgb[3 * o] = has ? resolve_channel(st.x, st.w) : ur;
    rgb[3 * o + 1] = has ? resolve_channel(st.y, st.w) : ug;
    rgb[3 * o + 2] = has ? resolve_channel(st.z, st.w) : ub;
    seen[o] = has ? 1 : 0;
  }
}

__global__ __launch_bounds__(kBlock) void tex_fill_kernel(Atlas at, const uint8_t* __restrict__ rgb_in,
                                                          const uint8_t* __restrict__ seen_in,
                                                          uint8_t* __restrict__ rgb_out, uint8_t* __restrict__ seen_out,
                                                          int32_t* __restrict__ filled) {
  const int64_t n = (int64_t)at.size * at.size;
  // the trip count is the same for every lane of a wave, so the ballot sees all 64
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t o = base + threadIdx.x;
    bool fill = false;
    if (o < n) {
      const int x = (int)(o % at.size), y = (int)(o / at.size);
      uint8_t c[3] = {rgb_in[3 * o], rgb_in[3 * o + 1], rgb_in[3 * o + 2]};
      uint8_t s = seen_in[o];
      int i, j;
      const int f = s == 0 ? texel_face(at, x, y, &i, &j) : -1;
      if (f >= 0) {
        const int nx[4] = {x - 1, x + 1, x, x}, ny[4] = {y, y, y - 1, y + 1};
        int sum[3] = {0, 0, 0}, count = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (nx[k] < 0 || nx[k] >= at.size || ny[k] < 0 || ny[k] >= at.size) continue;
          const int64_t q = (int64_t)ny[k] * at.size + nx[k];
          if (seen_in[q] == 0 || texel_face(at, nx[k], ny[k], &i, &j) != f) continue;
          sum[0] += rgb_in[3 * q];
          sum[1] += rgb_in[3 * q + 1];
          sum[2] += rgb_in[3 * q + 2];
          count += 1;
        }
        if (count > 0) {
          fill = true;
          s = 2;
#pragma unroll
          for (int k = 0; k < 3; ++k) c[k] = (uint8_t)((2 * sum[k] + count) / (2 * count));
        }
      }
      rgb_out[3 * o] = c[0];
      rgb_out[3 * o + 1] = c[1];
      rgb_out[3 * o + 2] = c[2];
      seen_out[o] = s;
    }
    const unsigned long long votes = __ballot(fill);
    if (votes != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(filled, (int32_t)__popcll(votes));
  }
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < 1 ? 1 : (blocks < kMaxGrid ? blocks : kMaxGrid));
}

static int check_atlas(const char* fn, const lnrf_tex_atlas* at) {
  if (atlas_ok(at)) return LNRF_OK;
  set_error("%s: the atlas needs faces >= 1, cells_per_row = ceil(sqrt(ceil(faces / 2))), %d <= cell <= %d and "
            "size = cells_per_row * cell <= %d",
            fn, kMinCell, kMaxCell, kMaxSize);
  return LNRF_ERR_SHAPE;
}

}  // namespace tex
}  // namespace lnrf

using namespace lnrf;

extern "C" int lnrf_tex_texels(const lnrf_tex_atlas* atlas, const float* tris, int32_t* face, float* position,
                               float* normal, float* bary, lnrf_stream_t stream) {
  const int rc = tex::check_atlas(__func__, atlas);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(tris && face, "null pointer");
  const int64_t tiles_x = (atlas->size + tex::kTile - 1) / tex::kTile;
  hipLaunchKernelGGL(tex::tex_texels_kernel, dim3(tex::grid_for(tiles_x * tiles_x * kWave)), dim3(tex::kBlock), 0,
                     as_stream(stream), *atlas, tris, face, position, normal, bary);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tex_uv(const lnrf_tex_atlas* atlas, const float* tris, const float* points, const int32_t* ids,
                           int64_t m, float* uv, lnrf_stream_t stream) {
  const int rc = tex::check_atlas(__func__, atlas);
  if (rc != LNRF_OK) return rc;
  if (m < 0) {
    set_error("%s: negative point count", __func__);
    return LNRF_ERR_SHAPE;
  }
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris && points && ids && uv, "null pointer");
  hipLaunchKernelGGL(tex::tex_uv_kernel, dim3(tex::grid_for(m)), dim3(tex::kBlock), 0, as_stream(stream), *atlas, tris,
                     points, ids, m, uv);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tex_sample(const void* texture, int32_t is_float, int64_t height, int64_t width, const float* uv,
                               int64_t m, float* out, lnrf_stream_t stream) {
  if (height < 1 || width < 1 || height > tex::kMaxSize || width > tex::kMaxSize || m < 0) {
    set_error("%s: a texture of %lld x %lld and %lld samples: sides in [1, %d], m >= 0", __func__, (long long)height,
              (long long)width, (long long)m, tex::kMaxSize);
    return LNRF_ERR_SHAPE;
  }
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(texture && uv && out, "null pointer");
  if (is_float)
    hipLaunchKernelGGL(tex::tex_sample_kernel<float>, dim3(tex::grid_for(m)), dim3(tex::kBlock), 0, as_stream(stream),
                       (const float*)texture, (int)height, (int)width, uv, m, out);
  else
    hipLaunchKernelGGL(tex::tex_sample_kernel<uint8_t>, dim3(tex::grid_for(m)), dim3(tex::kBlock), 0,
                       as_stream(stream), (const uint8_t*)texture, (int)height, (int)width, uv, m, out);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tex_resolve(const lnrf_tex_atlas* atlas, const float* state, int32_t unseen_r, int32_t unseen_g,
                                int32_t unseen_b, uint8_t* rgb, uint8_t* seen, lnrf_stream_t stream) {
  const int rc = tex::check_atlas(__func__, atlas);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(((unseen_r | unseen_g | unseen_b) & ~255) == 0, "the unseen colour must lie in [0, 255]");
  LNRF_CHECK_ARG(state && rgb && seen, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)state & 15) == 0, "state must be 16-byte aligned");
  const int64_t n = (int64_t)atlas->size * atlas->size;
  hipLaunchKernelGGL(tex::tex_resolve_kernel, dim3(tex::grid_for(n)), dim3(tex::kBlock), 0, as_stream(stream), n,
                     (const float4*)state, (uint8_t)unseen_r, (uint8_t)unseen_g, (uint8_t)unseen_b, rgb, seen);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tex_fill(const lnrf_tex_atlas* atlas, const uint8_t* rgb_in, const uint8_t* seen_in,
                             uint8_t* rgb_out, uint8_t* seen_out, int32_t* filled, lnrf_stream_t stream) {
  const int rc = tex::check_atlas(__func__, atlas);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(rgb_in && seen_in && rgb_out && seen_out && filled, "null pointer");
  LNRF_CHECK_ARG(rgb_in != rgb_out && seen_in != seen_out, "a pass reads one image and writes the other");
  const int64_t n = (int64_t)atlas->size * atlas->size;
  hipLaunchKernelGGL(tex::tex_fill_kernel, dim3(tex::grid_for(n)), dim3(tex::kBlock), 0, as_stream(stream), *atlas,
                     rgb_in, seen_in, rgb_out, seen_out, filled);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
