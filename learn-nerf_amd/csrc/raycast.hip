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
#include <cmath>

#include "common.h"

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

// Walks the tree for one ray: leaf(begin, end) gets the sorted-triangle range of every leaf whose box the ray may meet
// within [t_min, t_hi()], and returns true to stop.
template <class Hi, class Leaf>
__device__ __forceinline__ void traverse(const Bvh& b, const float4* __restrict__ nodes, const Ray& r, float t_min,
                                         Hi&& t_hi, Leaf&& leaf) {
  int k = 1;
  do {
    const bool hit = node_hit(r, nodes[2 * k], nodes[2 * k + 1], t_min, t_hi());
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
