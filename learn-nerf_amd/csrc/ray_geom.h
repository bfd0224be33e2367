// ray_geom.h — the fp32 ray arithmetic shared by rays.hip (renderer kernels) and view_stats.hip (dataset
// diagnostics): ray / box slab test and the per-pixel direction of a pinhole view.  One definition, so that a mask
// computed by either file is the same bit for the same ray.
#pragma once
#include "common.h"

namespace lnrf {

// ---------------------------------------------------------------------------------------
// ray_t_range (render.py:346-389), computed per ray.
struct TRange {
  float t_min, t_max;
  bool mask;
};

__device__ __forceinline__ TRange ray_t_range(const float* __restrict__ ray, const float bmin[3],
                                              const float bmax[3], float min_t_range, float eps) {
  float lo = -INFINITY, hi = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float o = ray[a], d = ray[3 + a];
    const float den = d + eps;                 // render.py:371 (epsilon added, not sign-matched)
    const float t0 = (bmin[a] - o) / den;      // render.py:370-371
    const float t1 = (bmax[a] - o) / den;
    lo = fmaxf(lo, fminf(t0, t1));             // render.py:374-383
    hi = fminf(hi, fmaxf(t0, t1));             // render.py:384
  }
  const float min_t = fmaxf(0.0f, lo);         // render.py:383
  const float max_t = hi;
  const float max_c = fmaxf(max_t, min_t + min_t_range);  // render.py:385
  TRange r;
  r.mask = min_t < max_t;                      // render.py:388
  r.t_min = r.mask ? min_t : 0.0f;             // render.py:389 null_range
  r.t_max = r.mask ? max_c : min_t_range;
  return r;
}

struct BBox {
  float mn[3], mx[3];
};

// CameraView.bare_rays (dataset.py:52-78): pixel (px, py) in raster order ->
// direction = normalize(z + tan(x_fov/2) * lx[px] * x_axis + tan(y_fov/2) * ly[py] * y_axis),
// lx = linspace(-1, 1, W), ly = linspace(-1, 1, H) (end points inclusive); origin = camera origin.
struct Camera {
  float origin[3], x_axis[3], y_axis[3], z_axis[3];
  float tan_x, tan_y;
};

// (host) the kernel-side camera of a view given as host vectors and fields of view in radians
static inline Camera make_camera(const float* origin, const float* x_axis, const float* y_axis, const float* z_axis,
                                 float x_fov, float y_fov) {
  Camera cam;
  for (int a = 0; a < 3; ++a) {
    cam.origin[a] = origin[a];
    cam.x_axis[a] = x_axis[a];
    cam.y_axis[a] = y_axis[a];
    cam.z_axis[a] = z_axis[a];
  }
  cam.tan_x = tanf(x_fov * 0.5f);
  cam.tan_y = tanf(y_fov * 0.5f);
  return cam;
}

// ray[0..2] = origin, ray[3..5] = unit direction of pixel (px, py); a width / height of 1 sits at the -1 end
__device__ __forceinline__ void camera_pixel_ray(const Camera& cam, int width, int height, int px, int py,
                                                 float ray[6]) {
  const float lx = width > 1 ? -1.0f + 2.0f * (float)px / (float)(width - 1) : -1.0f;
  const float ly = height > 1 ? -1.0f + 2.0f * (float)py / (float)(height - 1) : -1.0f;
  float d[3];
  float nrm = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    d[a] = (cam.tan_x * lx) * cam.x_axis[a] + (cam.tan_y * ly) * cam.y_axis[a] + cam.z_axis[a];
    nrm += d[a] * d[a];
  }
  nrm = sqrtf(nrm);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ray[a] = cam.origin[a];
    ray[3 + a] = d[a] / nrm;
  }
}

}  // namespace lnrf
