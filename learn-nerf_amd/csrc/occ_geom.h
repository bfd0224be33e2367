// occ_geom.h — the fp32 walk of one ray through an occupancy grid (lnrf_occ_clip_rays, occupancy.hip): one definition,
// host and device, restated operation by operation in NumPy float32 by tests/occupancy_reference.py.
//
// Conventions
//   grid      R^3 cells over the scene box, cell edge h_a = fl(fl(bmax_a - bmin_a) / R) per axis; cell (i, j, k) has
//             linear index idx = (i*R + j)*R + k and is bit idx & 31 of word idx >> 5.
//   planes    plane p of axis a (p = 0..R) is crossed at
//                 t(a, p) = fl(fl(fl(bmin_a + fl(p * h_a)) - o_a) / den_a),   den_a = fl(d_a + eps),
//             the same d + eps as ray_t_range, recomputed from the integer p at every step (never t += dt), every
//             operation rounded once (`#pragma clang fp contract(off)`).
//   direction the sign of den_a: +1, -1, or 0 for den_a == 0 (the axis is never crossed).  d_a = 0.0 and -0.0 both
//             give den_a = eps > 0.
//   start     the cell of the point fl(o_a + fl(d_a * t_min)): c_a = clamp(floor(fl(fl(x_a - bmin_a) / h_a)), 0, R-1).
//   step      the axis with the smallest next crossing, the lowest axis on a tie (strict <, axes tried in order 0, 1,
//             2), so a ray through a cell edge or corner visits the cells x first, then y, then z.
//   end       the walk stops when the next crossing is not below t_max (a NaN stops it too), when the step leaves the
//             grid, or after 3R + 3 steps (a walk needs at most 3R - 2; at the cap the inputs are returned unclipped).
//   result    t_first = entry into the first occupied cell (t_min itself for the start cell), t_last = exit from the
//             last occupied cell visited, +inf when that exit is the end of the walk;
//                 t_min' = max(t_min, t_first - pad_first)
//                 t_max' = min(t_max, max(t_last + pad_last, t_min' + min_t_range))
//             mask' = mask & found; the null range (0, min_t_range) of ray_t_range when mask' is 0.  When the start
//             cell is occupied pad_first = 0 and t_min' = t_min bit for bit; when the last cell is occupied
//             t_max' = t_max bit for bit; a full grid therefore returns its inputs.
//
// pad.  With u = 2^-24 and A_a = |bmin_a| + |bmax_a| + |o_a| (a bound on every intermediate of the numerator), the
// numerator of t(a, p) carries at most u*A_a from each of its product, sum and difference and 2u*A_a from the two
// roundings of h_a (p * h_a <= the extent): 5u*A_a in all; the quotient adds a relative u.  Against the crossing of the
// exact plane bmin_a + p * (bmax_a - bmin_a) / R by the line of den_a,
//     |t(a, p) - t_exact| <= 5u * A_a / |den_a| + u * |t| (1 + O(u)).
// The samples lie on o + d*t, not o + den*t: at the same t the two differ by eps * t along the axis, i.e. the crossing
// moves by eps * |t| / |den_a|.  The walk uses, for the plane that gave t_first or t_last,
//     pad(a, t) = fl(fl(fl(8u * A_a) + fl(eps * |t|)) / |den_a|) + fl(4u * |t|))       (kPadAbs = 8u, kPadRel = 4u)
// whose constants leave 3u * A_a / |den_a| + 3u * |t| for the roundings of pad itself and of the two final sums.  The
// entry time of a cell is the largest of its three entry crossings, so it is at least the crossing that the walk
// reports minus that crossing's pad; the exit time is the smallest, so it is at most the reported one plus its pad.
// pad grows without bound as den_a -> 0: such a ray is then not clipped on that side, which is conservative.
#pragma once
#include <cmath>

#include "ray_geom.h"

namespace lnrf {
namespace occ {

constexpr int kMaxRes = 512;
constexpr float kPadAbs = 0x1p-21f;  // 8 * 2^-24
constexpr float kPadRel = 0x1p-22f;  // 4 * 2^-24

__host__ __device__ __forceinline__ float pick3(const float v[3], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

__host__ __device__ __forceinline__ float plane_t(float bmin, float h, float o, float den, int p) {
#pragma clang fp contract(off)
  return ((bmin + (float)p * h) - o) / den;
}

__host__ __device__ __forceinline__ float plane_pad(float amp, float den, float eps, float t) {
#pragma clang fp contract(off)
  const float at = fabsf(t);
  return (kPadAbs * amp + eps * at) / fabsf(den) + kPadRel * at;
}

__host__ __device__ __forceinline__ int start_cell(float o, float d, float t, float bmin, float h, int res) {
#pragma clang fp contract(off)
  const float x = o + d * t;
  const float c = floorf((x - bmin) / h);
  // compare in float: c may be far outside the int range (NaN goes to cell 0)
  return c >= (float)(res - 1) ? res - 1 : (c > 0.0f ? (int)c : 0);
}

// Clips (t_min, t_max, mask) of one ray to the occupied cells of `bits`.  Reads bits only at indices below res^3.
__host__ __device__ inline TRange occ_clip_ray(const float* __restrict__ ray, const float bmin[3], const float bmax[3],
                                               int res, const uint32_t* __restrict__ bits, float min_t_range,
                                               float eps, float t_min, float t_max, bool mask) {
#pragma clang fp contract(off)
  TRange out;
  out.mask = false;
  out.t_min = 0.0f;
  out.t_max = min_t_range;
  if (!mask) return out;
  float h[3], o[3], den[3], amp[3];
  int step[3], c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = ray[a];
    den[a] = ray[3 + a] + eps;
    h[a] = (bmax[a] - bmin[a]) / (float)res;
    amp[a] = (fabsf(bmin[a]) + fabsf(bmax[a])) + fabsf(o[a]);
    step[a] = den[a] > 0.0f ? 1 : (den[a] < 0.0f ? -1 : 0);
    c[a] = start_cell(o[a], ray[3 + a], t_min, bmin[a], h[a], res);
  }
  bool found = false;
  float t_first = 0.0f, pad_first = 0.0f, t_last = 0.0f, pad_last = 0.0f;
  float t_enter = t_min;
  int enter_axis = -1;
  const int cap = 3 * res + 3;
  int it = 0;
  for (; it < cap; ++it) {
    const int idx = (c[0] * res + c[1]) * res + c[2];
    const bool occupied = ((bits[idx >> 5] >> (idx & 31)) & 1u) != 0;
    float tn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      tn[a] = step[a] == 0 ? INFINITY : plane_t(bmin[a], h[a], o[a], den[a], c[a] + (step[a] > 0 ? 1 : 0));
    int axis = 0;
    float t_exit = tn[0];
    if (tn[1] < t_exit) {
      axis = 1;
      t_exit = tn[1];
    }
    if (tn[2] < t_exit) {
      axis = 2;
      t_exit = tn[2];
    }
    const int next = (axis == 0 ? c[0] + step[0] : (axis == 1 ? c[1] + step[1] : c[2] + step[2]));
    const bool leaves = !(t_exit < t_max) || next < 0 || next >= res;
    if (occupied) {
      if (!found) {
        found = true;
        t_first = t_enter;
        pad_first = enter_axis < 0 ? 0.0f : plane_pad(pick3(amp, enter_axis), pick3(den, enter_axis), eps, t_enter);
      }
      t_last = leaves ? INFINITY : t_exit;
      pad_last = leaves ? 0.0f : plane_pad(pick3(amp, axis), pick3(den, axis), eps, t_exit);
    }
    if (leaves) break;
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = a == axis ? next : c[a];
    t_enter = t_exit;
    enter_axis = axis;
  }
  if (it == cap) {  // not reachable by a finite ray; stay conservative
    out.mask = true;
    out.t_min = t_min;
    out.t_max = t_max;
    return out;
  }
  if (!found) return out;
  const float lo = fmaxf(t_min, t_first - pad_first);
  const float hi = fminf(t_max, fmaxf(t_last + pad_last, lo + min_t_range));
  out.mask = true;
  out.t_min = lo;
  out.t_max = hi;
  return out;
}

}  // namespace occ
}  // namespace lnrf
