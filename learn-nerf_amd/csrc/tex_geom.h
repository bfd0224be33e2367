// tex_geom.h — the texture atlas of learn_nerf/texture.py: which face a texel belongs to, the surface point, normal
// and barycentrics of a texel, and the atlas coordinates of a surface point.  One definition each, host and device
// (texture.hip, the bake kernel of raycast.hip and the host program of tests/test_texture_cpu.py call the same inline
// functions), restated operation by operation in NumPy float32 by tests/texture_reference.py.  Every fp32 operation is
// rounded once (`#pragma clang fp contract(off)`), every division and square root is the correctly rounded one
// (hipcc's default), and no operation is reassociated.
//
// Layout   The texture is a square of S x S texels, texel (x, y) centred at (x + 1/2, y + 1/2), row y = 0 at the top of
//          the image.  The F faces go two to a square cell of c x c texels, K = ceil(sqrt(ceil(F / 2))) cells per row,
//          S = K c, kMinCell <= c <= kMaxCell.  Face f: pair f / 2, cell (pair % K, pair / K), half f % 2.  In
//          cell-local texel indices (i, j) the texel belongs to the lower half (0) when i + j + 1 <= c, else to the
//          upper half (1).  Texels of cells beyond the last pair, and of the upper half of the last cell when F is odd,
//          have face -1.
// Corners  The vertex opposite the longest edge goes to the patch's right angle, so that an obtuse triangle is not
//          squashed: l_k = |v_(k+1)%3 - v_(k+2)%3|^2 as (dx*dx + dy*dy) + dz*dz of the fp32 differences (first minus
//          second as written), r = the lowest k with the largest l_k (a NaN never wins), and A = v_r, B = v_(r+1)%3,
//          C = v_(r+2)%3: the same winding.  In cell-local texel units
//            lower  A (1, 1)          B (c - 2, 1)    C (1, c - 2)      legs of c - 3
//            upper  A (c - 1, c - 1)  B (3, c - 1)    C (c - 1, 3)      legs of c - 4
//          and OBJ coordinates are u = x / S, v = 1 - y / S.
// No bleed A bilinear sampler (sample() below) at texel coordinate x reads the columns i0 = floor(x - 1/2) and, only
//          when x - 1/2 is no integer, i0 + 1; rows likewise.  Write x - 1/2 = a + fx, y - 1/2 = b + fy with integers
//          a, b and fractions in [0, 1); the texels read are (a + [fx > 0], b + [fy > 0]) at most.  Lower patch: any
//          point in or on its UV triangle has x, y >= 1 and x + y <= c - 1, so a, b >= 0 and a + b + fx + fy <= c - 2.
//          The largest index sum read is a + b + [fx > 0] + [fy > 0]; with both fractions 0 it is a + b <= c - 2, with
//          one positive a + b < c - 2 so a + b + 1 <= c - 2, with both positive a + b + 2 <= c - 1 (a + b <= c - 3):
//          always i + j + 1 <= c, the lower half.  Upper patch: x, y <= c - 1 and x + y >= c + 2, so a, b <= c - 2
//          (and a + 1 is read only when a < c - 1.5, i.e. stays <= c - 1), a + b = x + y - 1 - fx - fy > c - 1, i.e.
//          a + b >= c, and every texel read has i + j + 1 >= c + 1: the upper half.  Moving either patch one texel
//          towards the diagonal breaks this (x + y = c on the lower one reads i + j = c with weight 1/4 at
//          fx = fy = 1/2).  The upper legs need c - 4 >= 2: kMinCell = 6.  The argument is in exact arithmetic on the
//          UV; tex_uv rounds the global coordinate cell * c + local to fp32, which moves it by at most ulp(S) / 2 per
//          axis (2^-12 for S <= 8192), so a point on a hypotenuse can give a foreign texel a weight of about 2^-24.
// Texel    Every texel of a used half-cell gets geometry, the gutter included.  With (px, py) = (i + 1/2, j + 1/2):
//            lower  bB = (px - 1) / (c - 3),        bC = (py - 1) / (c - 3)
//            upper  bB = ((c - 1) - px) / (c - 4),  bC = ((c - 1) - py) / (c - 4)
//          clamp(bB, bC): a coordinate that is not > 0 becomes 0 (NaN too); then s = bB + bC, and if s > 1,
//          bB = bB / s, bC = bC / s.  bA = (1 - bB) - bC (reported, not used for the point).  Point
//          p = (A + bB * e1) + bC * e2 per component with e1 = B - A, e2 = C - A.  A gutter texel so holds the colour
//          of the nearest point of its own face in the UV plane, and no dilation across patches exists.
// Normal   n = e1 x e2 (components a.y*b.z - a.z*b.y and cyclic), nn = (n.x*n.x + n.y*n.y) + n.z*n.z; the face is
//          degenerate unless nn > 0 (zero area, or an area whose square underflows): it has the normal (0, 0, 0) and its
//          texels are never coloured.  Otherwise len = sqrt(nn), N = n / len per component.
// uv       of a surface point q of face f: w = q - A, bB = ((w x e2) . n) / nn, bC = ((e1 x w) . n) / nn (the
//          projection onto the face's plane, as the face case of lnrf_mesh_nearest), both 0 on a degenerate face,
//          clamp as above, local (x, y) = (1 + bB * (c - 3), 1 + bC * (c - 3)) or ((c - 1) - bB * (c - 4),
//          (c - 1) - bC * (c - 4)), global = (float)(cell * c) + local.
// sample   at the texel coordinate u: x = u - 1/2 (tap_at takes x), i0 = floor(x), t = x - i0,
//          i1 = i0 + (t > 0 ? 1 : 0), both indices clamped to [0, n - 1] (compared in float, so NaN lands on index 0
//          and +-inf on a border); value (a + tx * (b - a)) on the rows j0 and j1, then
//          top + ty * (bottom - top): four equal texels return that value exactly, and a texel of weight 0 is not read.
// View     lnrf_tex_view: origin; inv = the rows of M^-1 as in lnrf_tsdf_view; width, height >= 2; pixel_offset = the
//          view's first pixel in the launch's packed uint8 RGBA buffer.  For a point p: d = p - origin, a = dot(r0, d),
//          b = dot(r1, d), s = dot(r2, d) with dot(r, d) = (d.x*r.x + d.y*r.y) + d.z*r.z; behind unless s > 0;
//          xf = ((a / s + 1) * 0.5) * (W - 1), yf likewise with H: pixel centre (col, row) is at (col, row), the
//          linspace(-1, 1, .) grid of CameraView.bare_rays.  The footprint is inside iff 0 <= xf <= W - 1 and
//          0 <= yf <= H - 1 (NaN is outside); its pixels and weights are tap_at(xf), tap_at(yf).
// Bake     per texel of a non-degenerate face, for the views in order (state (sr, sg, sb, sw), fp32):
//            v = origin - p, dist = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z), skip unless dist > 0, l = v / dist,
//            cosv = (N.x*l.x + N.y*l.y) + N.z*l.z, skip unless cosv > cos_max;
//            project p; skip when behind or when the footprint is not inside;
//            skip unless the alpha of all (up to four) footprint pixels is >= 128;
//            skip when any triangle is hit by the ray from (p + offset * N) along l within (0, dist);
//            w = 1, then w = w * cosv `power` times; per channel value = the sample() lerps of the pixels' bytes as
//            floats (0 .. 255); s_c = s_c + w * value; sw = sw + w.
// Resolve  seen = sw > 0; x = (s_c / sw) / 255, clamped to [0, 1] (x > 0 ? x : 0, then x < 1 ? x : 1), byte =
//          (int)floor(255 * x + 0.5); an unseen texel gets the given colour.
// Fill     a texel with seen == 0 and a face >= 0 takes, from its neighbours (x-1, y), (x+1, y), (x, y-1), (x, y+1)
//          inside the texture that have seen != 0 and the same face, the channel means (2 * sum + n) / (2 * n) in
//          integers (round half up) and seen = 2; every other texel is copied.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/lnrf.h"

#if defined(__HIPCC__)
#define LNRF_HD __host__ __device__ __forceinline__
#else
#define LNRF_HD inline
#endif

namespace lnrf {
namespace tex {

constexpr int kMinCell = 6;
constexpr int kMaxCell = 256;
constexpr int kMaxSize = 1 << 15;  // S: texel coordinates stay exact integers in fp32 with room for the fraction

using Atlas = lnrf_tex_atlas;  // faces F, cells_per_row K, cell c, size S = K c

// the conventions of the layout: what the entry points check before they look at a pointer
inline bool atlas_ok(const Atlas* at) {
  if (!at || at->faces < 1 || at->cells_per_row < 1 || at->cell < kMinCell || at->cell > kMaxCell) return false;
  const int64_t pairs = ((int64_t)at->faces + 1) / 2, k = at->cells_per_row;
  return k * k >= pairs && (k - 1) * (k - 1) < pairs && k * at->cell <= kMaxSize && at->size == k * at->cell;
}

// face of texel (x, y) of the texture (-1: none), and its cell-local indices
LNRF_HD int texel_face(const Atlas& at, int x, int y, int* i, int* j) {
  const int cx = x / at.cell, cy = y / at.cell;
  *i = x - cx * at.cell;
  *j = y - cy * at.cell;
  const int64_t f = 2 * ((int64_t)cy * at.cells_per_row + cx) + (*i + *j + 1 <= at.cell ? 0 : 1);
  return f < at.faces ? (int)f : -1;
}

LNRF_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}

// the corner that goes to the right angle: opposite the longest edge, the lowest index among equals
LNRF_HD int right_angle(const float* __restrict__ v) {
#pragma clang fp contract(off)
  float l[3];
  for (int k = 0; k < 3; ++k) {
    const float* p = v + 3 * ((k + 1) % 3);
    const float* q = v + 3 * ((k + 2) % 3);
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    l[k] = (dx * dx + dy * dy) + dz * dz;
  }
  int r = 0;
  if (l[1] > l[r]) r = 1;
  if (l[2] > l[r]) r = 2;
  return r;
}

// A, the legs e1 = B - A and e2 = C - A, the normal and whether the face has one
struct Frame {
  float a[3], e1[3], e2[3], n[3], nn;
  int r;
  bool degenerate;
};

LNRF_HD Frame face_frame(const float* __restrict__ v) {
#pragma clang fp contract(off)
  Frame fr;
  fr.r = right_angle(v);
  const float* A = v + 3 * fr.r;
  const float* B = v + 3 * ((fr.r + 1) % 3);
  const float* C = v + 3 * ((fr.r + 2) % 3);
  for (int k = 0; k < 3; ++k) {
    fr.a[k] = A[k];
    fr.e1[k] = B[k] - A[k];
    fr.e2[k] = C[k] - A[k];
  }
  fr.n[0] = fr.e1[1] * fr.e2[2] - fr.e1[2] * fr.e2[1];
  fr.n[1] = fr.e1[2] * fr.e2[0] - fr.e1[0] * fr.e2[2];
  fr.n[2] = fr.e1[0] * fr.e2[1] - fr.e1[1] * fr.e2[0];
  fr.nn = dot3(fr.n[0], fr.n[1], fr.n[2], fr.n[0], fr.n[1], fr.n[2]);
  fr.degenerate = !(fr.nn > 0.0f);
  return fr;
}

// (0, 0, 0) for a degenerate face
LNRF_HD void unit_normal(const Frame& fr, float out[3]) {
#pragma clang fp contract(off)
  if (fr.degenerate) {
    out[0] = out[1] = out[2] = 0.0f;
    return;
  }
  const float len = sqrtf(fr.nn);
  out[0] = fr.n[0] / len;
  out[1] = fr.n[1] / len;
  out[2] = fr.n[2] / len;
}

LNRF_HD void clamp_bary(float& bb, float& bc) {
#pragma clang fp contract(off)
  bb = bb > 0.0f ? bb : 0.0f;
  bc = bc > 0.0f ? bc : 0.0f;
  const float s = bb + bc;
  if (s > 1.0f) {
    bb = bb / s;
    bc = bc / s;
  }
}

// clamped (bB, bC) of the centre of the cell-local texel (i, j) against the UV triangle of its half
LNRF_HD void texel_bary(int c, int half, int i, int j, float& bb, float& bc) {
#pragma clang fp contract(off)
  const float px = (float)i + 0.5f, py = (float)j + 0.5f;
  if (half == 0) {
    const float leg = (float)(c - 3);
    bb = (px - 1.0f) / leg;
    bc = (py - 1.0f) / leg;
  } else {
    const float leg = (float)(c - 4), far = (float)(c - 1);
    bb = (far - px) / leg;
    bc = (far - py) / leg;
  }
  clamp_bary(bb, bc);
}

LNRF_HD void surface_point(const Frame& fr, float bb, float bc, float p[3]) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) p[k] = (fr.a[k] + bb * fr.e1[k]) + bc * fr.e2[k];
}

// (bA, bB, bC) in the order of the face's own vertices
LNRF_HD void bary_in_face_order(const Frame& fr, float bb, float bc, float out[3]) {
#pragma clang fp contract(off)
  out[fr.r] = (1.0f - bb) - bc;
  out[(fr.r + 1) % 3] = bb;
  out[(fr.r + 2) % 3] = bc;
}

// atlas coordinates (texels) of the surface point q of face f
LNRF_HD void point_uv(const Atlas& at, int f, const Frame& fr, const float q[3], float uv[2]) {
#pragma clang fp contract(off)
  float bb = 0.0f, bc = 0.0f;
  if (!fr.degenerate) {
    const float wx = q[0] - fr.a[0], wy = q[1] - fr.a[1], wz = q[2] - fr.a[2];
    const float mx = wy * fr.e2[2] - wz * fr.e2[1], my = wz * fr.e2[0] - wx * fr.e2[2], mz = wx * fr.e2[1] - wy * fr.e2[0];
    const float lx = fr.e1[1] * wz - fr.e1[2] * wy, ly = fr.e1[2] * wx - fr.e1[0] * wz, lz = fr.e1[0] * wy - fr.e1[1] * wx;
    bb = dot3(mx, my, mz, fr.n[0], fr.n[1], fr.n[2]) / fr.nn;
    bc = dot3(lx, ly, lz, fr.n[0], fr.n[1], fr.n[2]) / fr.nn;
  }
  clamp_bary(bb, bc);
  const int pair = f / 2, c = at.cell;
  float x, y;
  if (f % 2 == 0) {
    const float leg = (float)(c - 3);
    x = 1.0f + bb * leg;
    y = 1.0f + bc * leg;
  } else {
    const float leg = (float)(c - 4), far = (float)(c - 1);
    x = far - bb * leg;
    y = far - bc * leg;
  }
  uv[0] = (float)((pair % at.cells_per_row) * c) + x;
  uv[1] = (float)((pair / at.cells_per_row) * c) + y;
}

// the two indices and the weight of a bilinear tap along an axis of n texels, at x in units where texel k is at k
LNRF_HD void tap_at(float x, int n, int& i0, int& i1, float& t) {
#pragma clang fp contract(off)
  const float fl = floorf(x), last = (float)(n - 1);
  t = x - fl;
  const float nx = t > 0.0f ? fl + 1.0f : fl;
  i0 = (int)(fl > 0.0f ? (fl < last ? fl : last) : 0.0f);
  i1 = (int)(nx > 0.0f ? (nx < last ? nx : last) : 0.0f);
}

LNRF_HD float bilerp(float c00, float c10, float c01, float c11, float tx, float ty) {
#pragma clang fp contract(off)
  const float top = c00 + tx * (c10 - c00);
  const float bottom = c01 + tx * (c11 - c01);
  return top + ty * (bottom - top);
}

// pixel-centre coordinates (xf, yf) of p in the view; false when p is behind the camera
LNRF_HD bool project(const lnrf_tex_view& view, const float p[3], float& xf, float& yf) {
#pragma clang fp contract(off)
  const float dx = p[0] - view.origin[0], dy = p[1] - view.origin[1], dz = p[2] - view.origin[2];
  const float a = (dx * view.inv[0] + dy * view.inv[1]) + dz * view.inv[2];
  const float b = (dx * view.inv[3] + dy * view.inv[4]) + dz * view.inv[5];
  const float s = (dx * view.inv[6] + dy * view.inv[7]) + dz * view.inv[8];
  if (!(s > 0.0f)) return false;
  xf = ((a / s + 1.0f) * 0.5f) * (float)(view.width - 1);
  yf = ((b / s + 1.0f) * 0.5f) * (float)(view.height - 1);
  return true;
}

LNRF_HD bool footprint_inside(const lnrf_tex_view& view, float xf, float yf) {
  return xf >= 0.0f && xf <= (float)(view.width - 1) && yf >= 0.0f && yf <= (float)(view.height - 1);
}

LNRF_HD uint8_t resolve_channel(float sum, float weight) {
#pragma clang fp contract(off)
  float x = (sum / weight) / 255.0f;
  x = x > 0.0f ? x : 0.0f;
  x = x < 1.0f ? x : 1.0f;
  return (uint8_t)(int)floorf(255.0f * x + 0.5f);
}

}  // namespace tex
}  // namespace lnrf
