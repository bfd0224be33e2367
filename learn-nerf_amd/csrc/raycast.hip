// raycast.hip — ray casting against a triangle mesh: the collider of the reference's simple_dataset/main.go (model3d's
// MeshToCollider and the first-hit / any-hit queries of render3d.RayCaster).  No allocation, copy, synchronisation or
// atomic in any entry point; every result depends on the triangles and the ray alone, not on the launch geometry and
// not on the leaf size.
//
// Conventions (learn_nerf/raycast.py and the NumPy restatement tests/raycast_reference.py rely on them):
//   test      Moeller-Trumbore in fp32, every operation rounded once (`#pragma clang fp contract(off)` in tri_test):
//             dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross components a.y*b.z - a.z*b.y and cyclic;
//             e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p, inv = 1 / det (IEEE), s = o - v0, u = (s . p) * inv,
//             q = s x e1, v = (d . q) * inv, t = (e2 . q) * inv; accepted iff det != 0 && u >= 0 && v >= 0 &&
//             u + v <= 1 && t > t_min && t < t_max.  A NaN anywhere rejects; both faces are hit.
//   closest   smallest accepted t and the original index of its triangle; among equal t the lowest original index;
//             +inf and -1 without one.  Every ray's outputs are written.
//   occluded  1 iff any triangle is accepted, else 0; the traversal stops at the first.
//   rays      [m, 2, 3] fp32 (origin, direction), the layout of CameraView.bare_rays; window [m, 2] fp32 (t_min, t_max)
//             or NULL for (0, +inf).
//
// Structure: 30-bit Morton codes of the triangle centroids (lnrf_rt_morton; the caller sorts by them, stable), leaves of
// leaf_size consecutive sorted triangles, L = the power of two >= ceil(n / leaf_size) leaves, and over them the implicit
// complete binary tree in heap order: node k in [1, 2L) has the children 2k and 2k + 1, leaf j is node L + j.  Bounds are
// fitted level by level (lnrf_rt_fit: one launch for the leaves, one per level above, no counters); a leaf beyond the
// last triangle is empty (lo > hi) and so is a node over empty leaves only.  nodes [2L, 8] fp32 = lo.xyz, 0, hi.xyz, 0.
// Traversal is depth-first without a stack: a node that is hit and is no leaf goes to 2k, everything else to the next
// subtree in pre-order, (k + 1) >> ctz(k + 1), which is 1 after the last one.  No private array, no scratch.
//
// Culling is conservative, with the fp32 margin it needs.  The pinned test can accept a ray that in exact arithmetic
// misses the triangle, so the boxes are widened per ray by mu = 2^-11 * rho, rho = |o - c|_1 + 3 * radius, c the centre
// of the mesh's box and radius the sum of its half extents: rho >= S + E for S = |o - v0| and E the longest edge of
// any triangle.  Claim: if the pinned test accepts triangle i at parameter t_c with |det| >= 2^-7 |e1| |e2|, the point
// o + t_c d lies within mu / 2 of the triangle, hence inside the widened box of every node that holds i, and the slab
// interval of such a node contains t_c.  With eps = 2^-24, a = |e1|, b = |e2| and |d| <= 1.001: each cross product is
// off by at most 3.5 eps times the product of the lengths and each dot product adds 3.01 eps of it, so det, s.p, d.q
// and e2.q are off by at most 7 eps times ab, Sb, Sa and Sab.  Divided by |det| = g ab with g >= 2^-7 (the exact
// determinant is within a factor 1 +- 7 eps / g of it) and scaled to lengths, u and v put the exact plane crossing
// within 14.2 eps (S + E) / g of a point of the triangle, t_c is within 14 eps (S + E) / g of the exact parameter, and
// rounding o - v0 and the edges moves the data by less than 4 eps (S + E): 32 eps (S + E) / g <= 2^-12 rho in all.  The
// slab test's own roundings (subtract, reciprocal, multiply: 4 eps relative) move a box plane by at most 8 eps rho,
// far inside the other half of mu.  The traversal prunes with "entry > best t", never ">=", so an equal t with a lower
// index is still reached.  Below the bound on det (a ray within about half a degree of the triangle's plane) the pinned
// test's own acceptance region has no bounded width and no margin can cover it: that is the stated limit of the claim.
// Triangles whose own shape breaks the bound for every ray, |e1 x e2| < 2^-6 |e1| |e2| (slivers, zero area), get the
// box (-inf, +inf): they are sorted to the end and tested by every ray, so for them the results equal a brute force
// unconditionally.
// Domain (checked by the Python layer before any launch): finite vertices and origins of magnitude <= 2^20, a mesh
// extent in [2^-20, 2^20], directions with | |d|^2 - 1 | <= 2^-9, windows without NaN.
// A direction component of exactly 0 has an infinite reciprocal: a plane distance times it is -inf or +inf (the axis
// then constrains nothing, or everything when the origin is outside the slab), and 0 * inf = NaN, the origin exactly
// on a plane, drops that axis' constraint.  A flat box (an axis-aligned triangle) is a slab of width 2 mu.
//
// Nearest triangle (lnrf_mesh_nearest; learn_nerf/mesh_metrics.py, tests/mesh_metrics_reference.py restates it bit for
// bit).  For a point p and a triangle a, b, c = v0, v1, v2, in fp32 with every operation rounded once (contraction
// off), dot and cross as above:
//   e1 = b - a, e2 = c - a, e3 = c - b, w = p - a, z = p - b;
//   seg(w, d): dd = d . d, wd = w . d, t = dd > 0 ? wd / dd (IEEE) : 0, then t = t > 0 ? t : 0, t = t < 1 ? t : 1,
//              r = w - t * d per component, value r . r;
//   d2 starts at +inf and takes, in this order and only where STRICTLY smaller, seg(w, e1) [edge a-b], seg(z, e3)
//   [b-c], seg(w, e2) [a-c], and the face: n = e1 x e2, nn = n . n; if nn > 0: u = ((w x e2) . n) / nn,
//   v = ((e1 x w) . n) / nn, and if u >= 0 && v >= 0 && u + v <= 1: r = (w - u * e1) - v * e2, value r . r.
//   Closest point (optional output): a + t * e1, b + t * e3, a + t * e2 or (a + u * e1) + v * e2 of the winner.
// A zero-length edge takes t = 0 and a zero normal skips the face, so a triangle collapsed to a segment or a point gives
// the distance to that segment or point and nothing divides 0 by 0: no NaN for any finite triangle of the domain.
// Every candidate is the distance to a point OF the triangle (t in [0, 1]; u, v >= 0, u + v <= 1), and every vector is
// relative (p - a, never an absolute position), which is what the margin below rests on.  nearest: the smallest d2
// and the original index of its triangle; among equal d2 the lowest original index.
// Box test: g.x = max(max((lo.x - p.x) - mu, (p.x - hi.x) - mu), 0), likewise y and z, D2 = (g.x^2 + g.y^2) + g.z^2;
// a node is skipped iff D2 > best d2 so far — strictly, so an equal d2 with a lower index is still reached; an empty
// node (lo > hi) is skipped; the box (-inf, +inf) of the slivers gives -inf - mu = -inf, g = 0, D2 = 0, never NaN: they
// are always tested.  mu = 2^-11 * rho with the rho of the ray code, rho = |p - c|_1 + 3 * radius >= S + E for S the
// distance from p to any vertex and E any edge.
// Claim: a triangle i whose pinned d2 is <= the running best is never inside a skipped node.  With eps = 2^-24:
// (1) The pinned value is not far BELOW the distance to the triangle's box.  The winning candidate is |r|^2 for
// r = w - t d (or (w - u e1) - v e2).  In exact arithmetic on the rounded t (u, v) that is p - q for a point q of the
// triangle (up to eps E, from fl(u + v) <= 1), and q lies in the box of every node that holds i, so per axis
// |p - q| >= the exact gap g* of that box.  The roundings: w and d are off by eps |w| and eps |d|, the product t d by
// another eps |d|, the difference by eps |r| — at most eps (|w| + 2 |d| + |r|) <= 4 eps (S + E) for a segment, twice
// that for the face; the squared norm adds 3.01 eps relative, i.e. 1.51 eps on the distance.  So
// sqrt(pinned d2) >= |g*| - 16 eps rho (tests/mesh_metrics_reference.py: LOWER_C, checked against float64 there).
// (2) The computed D is not far ABOVE |g*| - mu.  lo - p is off by eps |lo - p| <= eps rho, the subtraction of mu by
// as much again, so each computed gap is at most max(g* - mu + 2.01 eps rho, 0); lowering every positive component of
// a non-negative vector by m' lowers its norm by at least m' (the norm's slope along -(1, 1, 1) is sum g / |g| >= 1);
// the squared norm adds 1.51 eps rho.  So sqrt(D2) <= |g*| - mu + 3.6 eps rho wherever that is positive, else D2 = 0.
// (3) Hence D2 > pinned d2 needs mu < 19.6 eps rho, while mu = 2^-11 rho~ = 8192 eps rho~ with the fp32 rho~ within
// 5 eps of rho: the margin is about 400 times what the argument needs, as the ray code's is generous for its claim.
// Nothing here depends on the triangle's shape: the one-sided bound (1) holds for slivers and zero-area triangles too.
// Domain: that of the ray code — finite coordinates of magnitude <= 2^20 for vertices and points, a mesh extent in
// [2^-20, 2^20]; products of three differences stay below 2^87 and above the subnormals.
//
// Texture bake (lnrf_tex_bake_views; learn_nerf/texture.py): the any-hit query above, started per (texel, view) from
// inside the kernel instead of from a ray array; tex_geom.h fixes its arithmetic, the section further down the launch.
#include <cmath>
#include <limits.h>

#include "common.h"
#include "tex_geom.h"

namespace lnrf {
namespace rt {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kMaxLeaf = 64;
constexpr int64_t kMaxTris = (int64_t)1 << 28;
constexpr float kMargin = 0x1p-11f;
constexpr float kSliver2 = 0x1p-12f;  // (2^-6)^2
constexpr int32_t kSliverCode = 1 << 30;

struct Bvh {
  float cx, cy, cz, hx, hy, hz, radius;
  int n, leaf, leaves;
};

// |e1 x e2|^2 < 2^-12 |e1|^2 |e2|^2, or too small to tell: the triangle goes to the always-tested set
__device__ __forceinline__ bool is_sliver(const float* __restrict__ v) {
  const float ax = v[3] - v[0], ay = v[4] - v[1], az = v[5] - v[2];
  const float bx = v[6] - v[0], by = v[7] - v[1], bz = v[8] - v[2];
  const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const float n2 = nx * nx + ny * ny + nz * nz;
  const float a2 = ax * ax + ay * ay + az * az, b2 = bx * bx + by * by + bz * bz;
  return !(n2 > 0.0f) || !(n2 >= kSliver2 * (a2 * b2));
}

// the pinned test: contraction off, so every product and sum is rounded on its own
__device__ __forceinline__ bool tri_test(float ox, float oy, float oz, float dx, float dy, float dz,
                                         const float* __restrict__ v, float t_min, float t_max, float* t_out) {
#pragma clang fp contract(off)
  const float v0x = v[0], v0y = v[1], v0z = v[2];
  const float e1x = v[3] - v0x, e1y = v[4] - v0y, e1z = v[5] - v0z;
  const float e2x = v[6] - v0x, e2y = v[7] - v0y, e2z = v[8] - v0z;
  const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
  const float det = (e1x * px + e1y * py) + e1z * pz;
  const float inv = 1.0f / det;  // hipcc's default fp32 divide is correctly rounded
  const float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
  const float u = ((sx * px + sy * py) + sz * pz) * inv;
  const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  const float w = ((dx * qx + dy * qy) + dz * qz) * inv;
  const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
  *t_out = t;
  return det != 0.0f && u >= 0.0f && w >= 0.0f && u + w <= 1.0f && t > t_min && t < t_max;
}

struct Ray {
  float ox, oy, oz, dx, dy, dz, ix, iy, iz, mu;
};

__device__ __forceinline__ Ray load_ray(const Bvh& b, const float* __restrict__ r) {
  Ray ray;
  ray.ox = r[0], ray.oy = r[1], ray.oz = r[2], ray.dx = r[3], ray.dy = r[4], ray.dz = r[5];
  ray.ix = 1.0f / ray.dx, ray.iy = 1.0f / ray.dy, ray.iz = 1.0f / ray.dz;
  ray.mu = kMargin * (((fabsf(ray.ox - b.cx) + fabsf(ray.oy - b.cy)) + fabsf(ray.oz - b.cz)) + 3.0f * b.radius);
  return ray;
}

__device__ __forceinline__ void slab(float lo, float hi, float o, float inv, float& enter, float& exit) {
  const float t1 = (lo - o) * inv, t2 = (hi - o) * inv;
  if (t1 == t1 && t2 == t2) {  // 0 * inf: the origin on the plane of an axis the ray does not move along
    enter = fmaxf(enter, fminf(t1, t2));
    exit = fminf(exit, fmaxf(t1, t2));
  }
}

// may the ray meet, within [t_lo, t_hi], the node's box widened by the ray's margin?
__device__ __forceinline__ bool node_hit(const Ray& r, const float4 lo, const float4 hi, float t_lo, float t_hi) {
  if (!(lo.x <= hi.x)) return false;  // empty
  float enter = t_lo, exit = t_hi;
  slab(lo.x - r.mu, hi.x + r.mu, r.ox, r.ix, enter, exit);
  slab(lo.y - r.mu, hi.y + r.mu, r.oy, r.iy, enter, exit);
  slab(lo.z - r.mu, hi.z + r.mu, r.oz, r.iz, enter, exit);
  // an entry at +inf or an exit at -inf is beyond every fp32 t, also when t_hi is +inf
  return !(enter > exit) && enter != INFINITY && exit != -INFINITY;
}

// The stackless pre-order walk, shared by the ray queries and the nearest-triangle query: test(k) says whether node k
// may hold an answer; leaf(begin, end) gets the sorted-triangle range of every leaf that passes, and returns true to stop.
template <class Test, class Leaf>
__device__ __forceinline__ void walk(const Bvh& b, Test&& test, Leaf&& leaf) {
  int k = 1;
  do {
    const bool hit = test(k);
    if (hit && k < b.leaves) {
      k = 2 * k;
      continue;
    }
    if (hit) {
      const int begin = (k - b.leaves) * b.leaf;
      if (leaf(begin, min(begin + b.leaf, b.n))) return;
    }
    k += 1;
    k >>= __builtin_ctz(k);
  } while (k != 1);
}

// Walks the tree for one ray: leaf(begin, end) gets the sorted-triangle range of every leaf whose box the ray may meet
// within [t_min, t_hi()], and returns true to stop.
template <class Hi, class Leaf>
__device__ __forceinline__ void traverse(const Bvh& b, const float4* __restrict__ nodes, const Ray& r, float t_min,
                                         Hi&& t_hi, Leaf&& leaf) {
  walk(b, [&](int k) { return node_hit(r, nodes[2 * k], nodes[2 * k + 1], t_min, t_hi()); }, leaf);
}

// ---------------------------------------------------------------------------------------- nearest triangle ----

// the clamped segment a + t d, t in [0, 1], against the offset w = p - a: if it is strictly nearer than *best, takes over
__device__ __forceinline__ void seg_nearest(float wx, float wy, float wz, float dx, float dy, float dz, float& best,
                                            float& bt) {
#pragma clang fp contract(off)
  const float dd = (dx * dx + dy * dy) + dz * dz;
  const float wd = (wx * dx + wy * dy) + wz * dz;
  float t = 0.0f;
  if (dd > 0.0f) {
    t = wd / dd;  // correctly rounded
    t = t > 0.0f ? t : 0.0f;  // a NaN (inf / inf cannot occur in the domain) would become 0 as well
    t = t < 1.0f ? t : 1.0f;
  }
  const float rx = wx - t * dx, ry = wy - t * dy, rz = wz - t * dz;
  const float d2 = (rx * rx + ry * ry) + rz * rz;
  if (d2 < best) {
    best = d2;
    bt = t;
  }
}

// the pinned point-triangle distance of the file header: d2, and in (qx, qy, qz), if cp asks for it, the closest point
__device__ __forceinline__ float tri_nearest(float px, float py, float pz, const float* __restrict__ v, bool cp,
                                             float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
  const float ax = v[0], ay = v[1], az = v[2], bx = v[3], by = v[4], bz = v[5], cx = v[6], cy = v[7], cz = v[8];
  const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  const float e3x = cx - bx, e3y = cy - by, e3z = cz - bz;
  const float wx = px - ax, wy = py - ay, wz = pz - az;
  const float zx = px - bx, zy = py - by, zz = pz - bz;
  float best = INFINITY, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
  seg_nearest(wx, wy, wz, e1x, e1y, e1z, best, t0);  // a -> b
  float d2 = best;
  int which = 0;
  seg_nearest(zx, zy, zz, e3x, e3y, e3z, best, t1);  // b -> c
  if (best < d2) d2 = best, which = 1;
  seg_nearest(wx, wy, wz, e2x, e2y, e2z, best, t2);  // a -> c
  if (best < d2) d2 = best, which = 2;
  // the face: only where the normal is not 0 and the projection has barycentric coordinates inside
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float nn = (nx * nx + ny * ny) + nz * nz;
  float fu = 0.0f, fv = 0.0f;
  if (nn > 0.0f) {
    const float mx = wy * e2z - wz * e2y, my = wz * e2x - wx * e2z, mz = wx * e2y - wy * e2x;  // w x e2
    const float lx = e1y * wz - e1z * wy, ly = e1z * wx - e1x * wz, lz = e1x * wy - e1y * wx;  // e1 x w
    const float u = ((mx * nx + my * ny) + mz * nz) / nn;
    const float w = ((lx * nx + ly * ny) + lz * nz) / nn;
    if (u >= 0.0f && w >= 0.0f && u + w <= 1.0f) {
      const float rx = (wx - u * e1x) - w * e2x, ry = (wy - u * e1y) - w * e2y, rz = (wz - u * e1z) - w * e2z;
      const float f2 = (rx * rx + ry * ry) + rz * rz;
      if (f2 < d2) d2 = f2, which = 3, fu = u, fv = w;
    }
  }
  if (cp) {
    if (which == 0) qx = ax + t0 * e1x, qy = ay + t0 * e1y, qz = az + t0 * e1z;
    if (which == 1) qx = bx + t1 * e3x, qy = by + t1 * e3y, qz = bz + t1 * e3z;
    if (which == 2) qx = ax + t2 * e2x, qy = ay + t2 * e2y, qz = az + t2 * e2z;
    if (which == 3) qx = (ax + fu * e1x) + fv * e2x, qy = (ay + fu * e1y) + fv * e2y, qz = (az + fu * e1z) + fv * e2z;
  }
  return d2;
}

// squared distance from p to the node's box, each face moved outward by mu; 0 for the box (-inf, +inf) of the slivers
__device__ __forceinline__ float box_d2(float px, float py, float pz, float mu, const float4 lo, const float4 hi) {
#pragma clang fp contract(off)
  const float gx = fmaxf(fmaxf((lo.x - px) - mu, (px - hi.x) - mu), 0.0f);
  const float gy = fmaxf(fmaxf((lo.y - py) - mu, (py - hi.y) - mu), 0.0f);
  const float gz = fmaxf(fmaxf((lo.z - pz) - mu, (pz - hi.z) - mu), 0.0f);
  return (gx * gx + gy * gy) + gz * gz;
}

__global__ __launch_bounds__(kBlock) void rt_nearest_kernel(Bvh b, const float* __restrict__ tris,
                                                            const int32_t* __restrict__ order,
                                                            const float4* __restrict__ nodes,
                                                            const float* __restrict__ pts, int64_t m,
                                                            float* __restrict__ out_d2, int32_t* __restrict__ out_id,
                                                            float* __restrict__ out_point) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const float mu = kMargin * (((fabsf(px - b.cx) + fabsf(py - b.cy)) + fabsf(pz - b.cz)) + 3.0f * b.radius);
    float best = INFINITY, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int best_id = -1;
    walk(
        b,
        [&](int k) {
          const float4 lo = nodes[2 * k], hi = nodes[2 * k + 1];
          if (!(lo.x <= hi.x)) return false;  // empty
          return !(box_d2(px, py, pz, mu, lo, hi) > best);
        },
        [&](int begin, int end) {
          for (int j = begin; j < end; ++j) {
            float qx = 0.0f, qy = 0.0f, qz = 0.0f;
            const float d2 = tri_nearest(px, py, pz, tris + 9 * (int64_t)j, out_point != nullptr, qx, qy, qz);
            if (d2 <= best) {
              const int id = order[j];
              if (d2 < best || best_id < 0 || id < best_id) {
                best = d2;
                best_id = id;
                bx = qx, by = qy, bz = qz;
              }
            }
          }
          return false;
        });
    out_d2[i] = best;
    out_id[i] = best_id;
    if (out_point) out_point[3 * i] = bx, out_point[3 * i + 1] = by, out_point[3 * i + 2] = bz;
  }
}

__global__ __launch_bounds__(kBlock) void rt_morton_kernel(Bvh b, const float* __restrict__ tris,
                                                           int32_t* __restrict__ codes) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < b.n; i += gridDim.x * kBlock) {
    const float* v = tris + 9 * (int64_t)i;
    int32_t code = kSliverCode;
    if (!is_sliver(v)) {
      const float c[3] = {(v[0] + v[3] + v[6]) * (1.0f / 3.0f), (v[1] + v[4] + v[7]) * (1.0f / 3.0f),
                          (v[2] + v[5] + v[8]) * (1.0f / 3.0f)};
      const float lo[3] = {b.cx - b.hx, b.cy - b.hy, b.cz - b.hz}, h[3] = {b.hx, b.hy, b.hz};
      code = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float f = h[a] > 0.0f ? (c[a] - lo[a]) / (2.0f * h[a]) * 1024.0f : 0.0f;
        uint32_t q = f >= 1023.0f ? 1023u : (f > 0.0f ? (uint32_t)f : 0u);
        q = (q | (q << 16)) & 0x030000FFu;  // spread 10 bits to every third
        q = (q | (q << 8)) & 0x0300F00Fu;
        q = (q | (q << 4)) & 0x030C30C3u;
        q = (q | (q << 2)) & 0x09249249u;
        code |= (int32_t)(q << (2 - a));
      }
    }
    codes[i] = code;
  }
}

__global__ __launch_bounds__(kBlock) void rt_fit_leaves_kernel(Bvh b, const float* __restrict__ tris,
                                                               float4* __restrict__ nodes) {
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < b.leaves; j += gridDim.x * kBlock) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int begin = min((int64_t)j * b.leaf, (int64_t)b.n), end = min((int64_t)begin + b.leaf, (int64_t)b.n);
    for (int i = begin; i < end; ++i) {
      const float* v = tris + 9 * (int64_t)i;
      const bool sliver = is_sliver(v);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = sliver ? -INFINITY : fminf(lo[a], fminf(v[a], fminf(v[3 + a], v[6 + a])));
        hi[a] = sliver ? INFINITY : fmaxf(hi[a], fmaxf(v[a], fmaxf(v[3 + a], v[6 + a])));
      }
    }
    nodes[2 * ((int64_t)b.leaves + j)] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    nodes[2 * ((int64_t)b.leaves + j) + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    if (j == 0) {  // slot 0 is no node
      nodes[0] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
      nodes[1] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
    }
  }
}

// nodes [first, 2 * first): the union of the two children (an empty child changes nothing)
__global__ __launch_bounds__(kBlock) void rt_fit_level_kernel(int first, float4* __restrict__ nodes) {
  for (int k = first + blockIdx.x * kBlock + threadIdx.x; k < 2 * first; k += gridDim.x * kBlock) {
    const float4 la = nodes[4 * (int64_t)k], ha = nodes[4 * (int64_t)k + 1];
    const float4 lb = nodes[4 * (int64_t)k + 2], hb = nodes[4 * (int64_t)k + 3];
    nodes[2 * (int64_t)k] = make_float4(fminf(la.x, lb.x), fminf(la.y, lb.y), fminf(la.z, lb.z), 0.0f);
    nodes[2 * (int64_t)k + 1] = make_float4(fmaxf(ha.x, hb.x), fmaxf(ha.y, hb.y), fmaxf(ha.z, hb.z), 0.0f);
  }
}

__global__ __launch_bounds__(kBlock) void rt_closest_kernel(Bvh b, const float* __restrict__ tris,
                                                            const int32_t* __restrict__ order,
                                                            const float4* __restrict__ nodes,
                                                            const float* __restrict__ rays,
                                                            const float* __restrict__ window, int64_t m,
                                                            float* __restrict__ out_t, int32_t* __restrict__ out_id) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const Ray r = load_ray(b, rays + 6 * i);
    const float t_min = window ? window[2 * i] : 0.0f, t_max = window ? window[2 * i + 1] : INFINITY;
    float best = INFINITY;
    int best_id = -1;
    traverse(
        b, nodes, r, t_min, [&]() { return fminf(t_max, best); },
        [&](int begin, int end) {
          for (int j = begin; j < end; ++j) {
            float t;
            if (tri_test(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, tris + 9 * (int64_t)j, t_min, t_max, &t) && t <= best) {
              const int id = order[j];
              if (t < best || best_id < 0 || id < best_id) {
                best = t;
                best_id = id;
              }
            }
          }
          return false;
        });
    out_t[i] = best_id >= 0 ? best : INFINITY;
    out_id[i] = best_id;
  }
}

__global__ __launch_bounds__(kBlock) void rt_occluded_kernel(Bvh b, const float* __restrict__ tris,
                                                             const float4* __restrict__ nodes,
                                                             const float* __restrict__ rays,
                                                             const float* __restrict__ window, int64_t m,
                                                             uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const Ray r = load_ray(b, rays + 6 * i);
    const float t_min = window ? window[2 * i] : 0.0f, t_max = window ? window[2 * i + 1] : INFINITY;
    bool any = false;
    traverse(
        b, nodes, r, t_min, [&]() { return t_max; },
        [&](int begin, int end) {
          for (int j = begin; j < end && !any; ++j) {
            float t;
            any = tri_test(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, tris + 9 * (int64_t)j, t_min, t_max, &t);
          }
          return any;
        });
    out[i] = any ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------- texture bake ----
// lnrf_tex_bake_views (tex_geom.h "Bake" fixes every operation; learn_nerf/texture.py drives it).  One lane per texel,
// a wave per tile of 8 x 8 texels, so that a wave's lanes share one to four faces: their points project to neighbouring
// pixels and their shadow rays walk the same nodes.  The lane computes its point and normal once, loads its state once,
// walks the launch's views in order with the state in registers and stores it once; the descriptors are read at a
// wave-uniform index.  Per view the tests run cheapest first (facing, projection and footprint, alpha: arithmetic and
// four byte gathers) and only a (texel, view) pair that survives them starts a traversal.  No atomics, no scratch: a
// texel's result depends on the sequence of views alone, not on the launch geometry and not on how the views are split
// over launches (the state between two launches is exactly the registers' content).
constexpr int kTexTile = 8;
static_assert(kTexTile * kTexTile == kWave, "one texel per lane");

__global__ __launch_bounds__(kBlock) void tex_bake_views_kernel(Bvh b, const float* __restrict__ sorted_tris,
                                                                const float4* __restrict__ nodes, tex::Atlas at,
                                                                const float* __restrict__ tris,
                                                                const lnrf_tex_view* __restrict__ views, int n_views,
                                                                const uint8_t* __restrict__ rgba, float cos_max,
                                                                int power, float offset, float4* __restrict__ state) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1);
  const int tiles_x = (at.size + kTexTile - 1) / kTexTile;
  const int tiles = tiles_x * tiles_x;
  const int first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave));
  for (int tile = first; tile < tiles; tile += gridDim.x * (kBlock / kWave)) {
    const int x = (tile % tiles_x) * kTexTile + (lane & (kTexTile - 1)), y = (tile / tiles_x) * kTexTile + lane / kTexTile;
    if (x >= at.size || y >= at.size) continue;
    int ci, cj;
    const int f = tex::texel_face(at, x, y, &ci, &cj);
    if (f < 0) continue;
    const tex::Frame fr = tex::face_frame(tris + 9 * (int64_t)f);
    if (fr.degenerate) continue;
    float bb, bc, p[3], n[3];
    tex::texel_bary(at.cell, f & 1, ci, cj, bb, bc);
    tex::surface_point(fr, bb, bc, p);
    tex::unit_normal(fr, n);
    const float start[3] = {p[0] + offset * n[0], p[1] + offset * n[1], p[2] + offset * n[2]};
    const int64_t o = (int64_t)y * at.size + x;
    float4 st = state[o];
    for (int v = 0; v < n_views; ++v) {
      const lnrf_tex_view& view = views[v];
      const float vx = view.origin[0] - p[0], vy = view.origin[1] - p[1], vz = view.origin[2] - p[2];
      const float dist = sqrtf((vx * vx + vy * vy) + vz * vz);
      if (!(dist > 0.0f)) continue;
      const float lx = vx / dist, ly = vy / dist, lz = vz / dist;
      const float cosv = (n[0] * lx + n[1] * ly) + n[2] * lz;
      if (!(cosv > cos_max)) continue;
      float xf, yf;
      if (!tex::project(view, p, xf, yf) || !tex::footprint_inside(view, xf, yf)) continue;
      int i0, i1, j0, j1;
      float tx, ty;
      tex::tap_at(xf, view.width, i0, i1, tx);
      tex::tap_at(yf, view.height, j0, j1, ty);
      const uchar4* __restrict__ image = (const uchar4*)rgba + view.pixel_offset;
      const uchar4 c00 = image[(int64_t)j0 * view.width + i0], c10 = image[(int64_t)j0 * view.width + i1];
      const uchar4 c01 = image[(int64_t)j1 * view.width + i0], c11 = image[(int64_t)j1 * view.width + i1];
      if (c00.w < 128 || c10.w < 128 || c01.w < 128 || c11.w < 128) continue;
      Ray r;
      r.ox = start[0], r.oy = start[1], r.oz = start[2], r.dx = lx, r.dy = ly, r.dz = lz;
      r.ix = 1.0f / lx, r.iy = 1.0f / ly, r.iz = 1.0f / lz;
      r.mu = kMargin * (((fabsf(r.ox - b.cx) + fabsf(r.oy - b.cy)) + fabsf(r.oz - b.cz)) + 3.0f * b.radius);
      bool any = false;
      traverse(
          b, nodes, r, 0.0f, [&]() { return dist; },
          [&](int begin, int end) {
            for (int j = begin; j < end && !any; ++j) {
              float t;
              any = tri_test(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, sorted_tris + 9 * (int64_t)j, 0.0f, dist, &t);
            }
            return any;
          });
      if (any) continue;
      float w = 1.0f;
      for (int k = 0; k < power; ++k) w = w * cosv;
      st.x = st.x + w * tex::bilerp((float)c00.x, (float)c10.x, (float)c01.x, (float)c11.x, tx, ty);
      st.y = st.y + w * tex::bilerp((float)c00.y, (float)c10.y, (float)c01.y, (float)c11.y, tx, ty);
      st.z = st.z + w * tex::bilerp((float)c00.z, (float)c10.z, (float)c01.z, (float)c11.z, tx, ty);
      st.w = st.w + w;
    }
    state[o] = st;
  }
}

static int64_t leaves_for(int64_t n, int32_t leaf) {
  int64_t leaves = 1;
  while (leaves * leaf < n) leaves *= 2;
  return leaves;
}

static int check_bvh(const char* fn, const lnrf_rt_bvh* bvh, Bvh* b) {
  if (!bvh) {
    set_error("%s: null descriptor", fn);
    return LNRF_ERR_ARG;
  }
  bool finite = std::isfinite(bvh->radius) && bvh->radius > 0.0f;
  for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(bvh->center[a]) && bvh->half[a] >= 0.0f;
  if (!finite || !(bvh->half[0] + bvh->half[1] + bvh->half[2] <= bvh->radius * 1.001f)) {
    set_error("%s: the box needs a finite centre, half extents >= 0 and a radius > 0 that is at least their sum", fn);
    return LNRF_ERR_ARG;
  }
  if (bvh->n_tris < 1 || bvh->n_tris > kMaxTris || bvh->leaf_size < 1 || bvh->leaf_size > kMaxLeaf) {
    set_error("%s: %d triangles in leaves of %d: need 1 <= n <= 2^28 and a leaf size in [1, %d]", fn, bvh->n_tris,
              bvh->leaf_size, kMaxLeaf);
    return LNRF_ERR_SHAPE;
  }
  *b = Bvh{bvh->center[0], bvh->center[1], bvh->center[2], bvh->half[0], bvh->half[1], bvh->half[2], bvh->radius,
           bvh->n_tris,    bvh->leaf_size, (int)leaves_for(bvh->n_tris, bvh->leaf_size)};
  return LNRF_OK;
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
}

}  // namespace rt
}  // namespace lnrf

using namespace lnrf;

extern "C" int64_t lnrf_rt_node_count(int64_t n_tris, int32_t leaf_size) {
  if (n_tris < 1 || n_tris > rt::kMaxTris || leaf_size < 1 || leaf_size > rt::kMaxLeaf) return -1;
  return 2 * rt::leaves_for(n_tris, leaf_size);
}

extern "C" int lnrf_rt_morton(const lnrf_rt_bvh* bvh, const float* tris, int32_t* codes, lnrf_stream_t stream) {
  rt::Bvh b;
  const int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(tris && codes, "null pointer");
  hipLaunchKernelGGL(rt::rt_morton_kernel, dim3(rt::grid_for(b.n)), dim3(rt::kBlock), 0, as_stream(stream), b, tris,
                     codes);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_rt_fit(const lnrf_rt_bvh* bvh, const float* sorted_tris, float* nodes, lnrf_stream_t stream) {
  rt::Bvh b;
  const int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(sorted_tris && nodes, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)nodes & 15) == 0, "nodes must be 16-byte aligned");
  hipLaunchKernelGGL(rt::rt_fit_leaves_kernel, dim3(rt::grid_for(b.leaves)), dim3(rt::kBlock), 0, as_stream(stream), b,
                     sorted_tris, (float4*)nodes);
  LNRF_LAUNCH_CHECK();
  for (int first = b.leaves / 2; first >= 1; first /= 2) {
    hipLaunchKernelGGL(rt::rt_fit_level_kernel, dim3(rt::grid_for(first)), dim3(rt::kBlock), 0, as_stream(stream),
                       first, (float4*)nodes);
    LNRF_LAUNCH_CHECK();
  }
  return LNRF_OK;
}

static int check_query(const char* fn, const void* tris, const void* nodes, const void* rays, int64_t m) {
  if (m < 0) {
    set_error("%s: negative ray count", fn);
    return LNRF_ERR_ARG;
  }
  if (!tris || !nodes || (m > 0 && !rays)) {
    set_error("%s: null pointer", fn);
    return LNRF_ERR_ARG;
  }
  if ((uintptr_t)nodes & 15) {
    set_error("%s: nodes must be 16-byte aligned", fn);
    return LNRF_ERR_ARG;
  }
  return LNRF_OK;
}

extern "C" int lnrf_rt_closest(const lnrf_rt_bvh* bvh, const float* sorted_tris, const int32_t* order,
                               const float* nodes, const float* rays, const float* window, int64_t m, float* out_t,
                               int32_t* out_id, lnrf_stream_t stream) {
  rt::Bvh b;
  int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc == LNRF_OK) rc = check_query(__func__, sorted_tris, nodes, rays, m);
  if (rc != LNRF_OK) return rc;
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(order && out_t && out_id, "null pointer");
  hipLaunchKernelGGL(rt::rt_closest_kernel, dim3(rt::grid_for(m)), dim3(rt::kBlock), 0, as_stream(stream), b,
                     sorted_tris, order, (const float4*)nodes, rays, window, m, out_t, out_id);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_rt_occluded(const lnrf_rt_bvh* bvh, const float* sorted_tris, const float* nodes,
                                const float* rays, const float* window, int64_t m, uint8_t* out,
                                lnrf_stream_t stream) {
  rt::Bvh b;
  int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc == LNRF_OK) rc = check_query(__func__, sorted_tris, nodes, rays, m);
  if (rc != LNRF_OK) return rc;
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(out, "null pointer");
  hipLaunchKernelGGL(rt::rt_occluded_kernel, dim3(rt::grid_for(m)), dim3(rt::kBlock), 0, as_stream(stream), b,
                     sorted_tris, (const float4*)nodes, rays, window, m, out);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_mesh_nearest(const lnrf_rt_bvh* bvh, const float* sorted_tris, const int32_t* order,
                                 const float* nodes, const float* pts, int64_t m, float* out_d2, int32_t* out_id,
                                 float* out_point, lnrf_stream_t stream) {
  rt::Bvh b;
  int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc == LNRF_OK) rc = check_query(__func__, sorted_tris, nodes, pts, m);
  if (rc != LNRF_OK) return rc;
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(order && out_d2 && out_id, "null pointer");
  hipLaunchKernelGGL(rt::rt_nearest_kernel, dim3(rt::grid_for(m)), dim3(rt::kBlock), 0, as_stream(stream), b,
                     sorted_tris, order, (const float4*)nodes, pts, m, out_d2, out_id, out_point);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tex_bake_views(const lnrf_rt_bvh* bvh, const float* sorted_tris, const float* nodes,
                                   const lnrf_tex_atlas* atlas, const float* tris, const lnrf_tex_view* views,
                                   int64_t n_views, const uint8_t* rgba, float cos_max, int32_t power, float offset,
                                   float* state, lnrf_stream_t stream) {
  if (!tex::atlas_ok(atlas)) {
    set_error("%s: the atlas needs faces >= 1, cells_per_row = ceil(sqrt(ceil(faces / 2))), %d <= cell <= %d and "
              "size = cells_per_row * cell <= %d",
              __func__, tex::kMinCell, tex::kMaxCell, tex::kMaxSize);
    return LNRF_ERR_SHAPE;
  }
  if (n_views < 0 || n_views > INT32_MAX) {
    set_error("%s: n_views = %lld outside [0, INT32_MAX]", __func__, (long long)n_views);
    return LNRF_ERR_SHAPE;
  }
  rt::Bvh b;
  const int rc = rt::check_bvh(__func__, bvh, &b);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(std::isfinite(cos_max), "cos_max must be finite");
  LNRF_CHECK_ARG(power >= 0 && power <= 64, "power must lie in [0, 64]");
  LNRF_CHECK_ARG(offset >= 0.0f && std::isfinite(offset), "offset must be finite and not negative");
  LNRF_CHECK_ARG(sorted_tris && nodes && tris && state, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)nodes & 15) == 0 && ((uintptr_t)state & 15) == 0, "nodes and state must be 16-byte aligned");
  if (n_views == 0) return LNRF_OK;
  LNRF_CHECK_ARG(views && rgba, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)rgba & 3) == 0 && ((uintptr_t)views & 7) == 0, "rgba must be 4-byte, views 8-byte aligned");
  const int64_t tiles_x = (atlas->size + rt::kTexTile - 1) / rt::kTexTile;
  hipLaunchKernelGGL(rt::tex_bake_views_kernel, dim3(rt::grid_for(tiles_x * tiles_x * kWave)), dim3(rt::kBlock), 0,
                     as_stream(stream), b, sorted_tris, (const float4*)nodes, *atlas, tris, views, (int)n_views, rgba,
                     cos_max, (int)power, offset, (float4*)state);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
