// tsdf_geom.h — the fp32 update of one voxel by one RGB-D view (lnrf_tsdf_integrate, tsdf.hip) and the colour of one
// mesh vertex (lnrf_tsdf_vertex_colors): one definition each, host and device, restated operation by operation in NumPy
// float32 by tests/tsdf_reference.py.  Every fp32 operation is rounded once (`#pragma clang fp contract(off)`), every
// division is the correctly rounded one (hipcc's default), and no operation is reassociated.
//
// Conventions
//   voxel     p = (xs[i], ys[j], zs[k]), linear index (i*ny + j)*nz + k; the coordinates are read, never computed.
//   view      lnrf_tsdf_view: origin; inv = the rows r0, r1, r2 of M^-1 for M with columns tan(x_fov/2) x_axis,
//             tan(y_fov/2) y_axis, camera_direction (inverted in float64 by the host, rounded to fp32); zaxis =
//             camera_direction; width W, height H (each >= 2); element offsets of the view's depth (uint16 [H, W]) and
//             colour (uint8 [H, W, 3], RGB) images in the launch's two packed buffers.
//   dot       dot(r, d) = fl(fl(fl(d.x*r.x) + fl(d.y*r.y)) + fl(d.z*r.z)).
//   update    d  = p - origin                       (per component)
//             a  = dot(r0, d), b = dot(r1, d), s = dot(r2, d), zc = dot(zaxis, d)
//             skip unless s > 0                     (a NaN skips)
//             u  = a / s, v = b / s
//             cf = fl(fl(fl(u + 1) * 0.5) * (float)(W - 1)) + 0.5,  rf likewise from v and H
//             skip unless 0 <= cf < (float)W and 0 <= rf < (float)H   (compared in float: NaN and +-inf skip)
//             pixel (row, col) = (floor(rf), floor(cf)): the nearest pixel of the linspace(-1, 1, .) ray convention
//             d16 = depth[depth_offset + row*W + col]
//             d16 == 0xFFFF: with carve, sum_t += 1 and n_obs += 1; next view
//             zd = fl(fl((float)d16 / 65535) * max_depth)
//             q  = fl(zd - zc) / trunc
//             q < -1: behind = 1
//             else:   sum_t += (q > 1 ? 1 : q), n_obs += 1, and when q <= 1: rgb_sum += rgb[pixel], n_col += 1
//   colour    of a vertex v in the padded index space of the marching-cubes volume: per axis lo_a = floor(v_a) - 1 and
//             hi_a = ceil(v_a) - 1 name the two grid points of the vertex's edge, f = v_a - floor(v_a) on the first axis
//             where that is not 0 (0 when the vertex is a grid point).  An endpoint has a colour when 0 <= index < n on
//             every axis and n_col > 0: mean_c = fl(fl((float)rgb_sum_c / (float)n_col) / 255).  Both coloured:
//             fl(m0 + fl(f * fl(m1 - m0))); one: that one; none: 0.5 grey, counted as missing.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/lnrf.h"

namespace lnrf {
namespace tsdf {

constexpr uint16_t kNoDepth = 0xFFFF;

struct VoxelState {
  float sum_t;
  int32_t n_obs;
  int32_t behind;
  int32_t r, g, b;
  int32_t n_col;
};

__host__ __device__ __forceinline__ float dot3(const float* __restrict__ r, float dx, float dy, float dz) {
#pragma clang fp contract(off)
  return (dx * r[0] + dy * r[1]) + dz * r[2];
}

// fl(fl(fl(u + 1) * 0.5) * (n - 1)) + 0.5: continuous pixel coordinate, pixel c covers [c, c + 1)
__host__ __device__ __forceinline__ float pixel_coord(float u, int n) {
#pragma clang fp contract(off)
  return ((u + 1.0f) * 0.5f) * (float)(n - 1) + 0.5f;
}

// One view's contribution to one voxel.  Reads depth / color only at the pixel that the voxel projects to, which lies
// inside the view's image.
__host__ __device__ __forceinline__ void update_voxel(VoxelState& st, float px, float py, float pz,
                                                      const lnrf_tsdf_view& view, const uint16_t* __restrict__ depth,
                                                      const uint8_t* __restrict__ color, float trunc, float max_depth,
                                                      bool carve) {
#pragma clang fp contract(off)
  const float dx = px - view.origin[0], dy = py - view.origin[1], dz = pz - view.origin[2];
  const float a = dot3(view.inv, dx, dy, dz);
  const float b = dot3(view.inv + 3, dx, dy, dz);
  const float s = dot3(view.inv + 6, dx, dy, dz);
  const float zc = dot3(view.zaxis, dx, dy, dz);
  if (!(s > 0.0f)) return;
  const float u = a / s, v = b / s;
  const float cf = pixel_coord(u, view.width), rf = pixel_coord(v, view.height);
  if (!(cf >= 0.0f && cf < (float)view.width && rf >= 0.0f && rf < (float)view.height)) return;
  const int64_t pixel = (int64_t)floorf(rf) * view.width + (int64_t)floorf(cf);
  const uint16_t d16 = depth[view.depth_offset + pixel];
  if (d16 == kNoDepth) {
    if (carve) {
      st.sum_t += 1.0f;
      st.n_obs += 1;
    }
    return;
  }
  const float zd = (float)d16 / 65535.0f * max_depth;
  const float q = (zd - zc) / trunc;
  if (q < -1.0f) {
    st.behind = 1;
    return;
  }
  st.sum_t += q > 1.0f ? 1.0f : q;
  st.n_obs += 1;
  if (q <= 1.0f) {
    const uint8_t* __restrict__ rgb = color + view.color_offset + 3 * pixel;
    st.r += rgb[0];
    st.g += rgb[1];
    st.b += rgb[2];
    st.n_col += 1;
  }
}

// The value of the marching-cubes volume at a grid point: -F, inside = positive.
__host__ __device__ __forceinline__ float volume_value(float sum_t, int32_t n_obs, uint8_t behind, bool unseen_inside) {
#pragma clang fp contract(off)
  if (n_obs > 0) return -(sum_t / (float)n_obs);
  return behind && unseen_inside ? 1.0f : -1.0f;
}

// Colour of one vertex (padded index space) -> true when neither endpoint has a colour (out = 0.5 grey).
__host__ __device__ __forceinline__ bool vertex_color(const float* __restrict__ vert, int nx, int ny, int nz,
                                                      const int32_t* __restrict__ rgb_sum,
                                                      const int32_t* __restrict__ n_col, float out[3]) {
#pragma clang fp contract(off)
  const int dims[3] = {nx, ny, nz};
  int64_t idx[2] = {0, 0};
  bool inside[2] = {true, true};
  float f = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = floorf(vert[a]), hi = ceilf(vert[a]);
    const float frac = vert[a] - lo;
    if (f == 0.0f && frac > 0.0f) f = frac;
    const float end[2] = {lo - 1.0f, hi - 1.0f};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      // compare in float: a NaN or a far-away vertex has no endpoint inside the grid
      const bool ok = end[e] >= 0.0f && end[e] <= (float)(dims[a] - 1);
      inside[e] = inside[e] && ok;
      idx[e] = idx[e] * dims[a] + (ok ? (int64_t)end[e] : 0);
    }
  }
  float mean[2][3];
  bool has[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int32_t n = inside[e] ? n_col[idx[e]] : 0;
    has[e] = n > 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      mean[e][c] = has[e] ? (float)rgb_sum[3 * idx[e] + c] / (float)n / 255.0f : 0.5f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[c] = has[0] && has[1] ? mean[0][c] + f * (mean[1][c] - mean[0][c]) : (has[0] ? mean[0][c] : mean[1][c]);
  return !(has[0] || has[1]);
}

}  // namespace tsdf
}  // namespace lnrf
