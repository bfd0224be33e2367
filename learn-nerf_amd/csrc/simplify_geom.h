// simplify_geom.h — the pinned arithmetic of the mesh simplifier (csrc/simplify.hip): the cell of a corner in fp32,
// the plane quadric of a triangle in fp64 and the placement of a cell's vertex in fp64.  One definition each, host and
// device, restated operation by operation in NumPy by tests/simplify_reference.py.  Every operation is rounded once
// (`#pragma clang fp contract(off)`), divisions and square roots are the correctly rounded ones (hipcc's default), and
// no operation is reassociated.
//
//   cell      per axis c_a = min(n_a - 1, (int)floorf(fl(fl(v_a - lo_a) * inv_h))), compared in float so that a huge
//             quotient cannot overflow the conversion; anything not above 0 (a corner below lo, a NaN) goes to cell 0.
//             key = (cx * ny + cy) * nz + cz.
//   quadric   of the triangle (a, b, c), every coordinate widened to fp64 first:
//             e1 = b - a, e2 = c - a
//             n  = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x)
//             w  = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z),   d = (n.x*a.x + n.y*a.y) + n.z*a.z
//             w > 0:  q = ((n.x*n.x)/w, (n.x*n.y)/w, (n.x*n.z)/w, (n.y*n.y)/w, (n.y*n.z)/w, (n.z*n.z)/w,
//                          (n.x*d)/w, (n.y*d)/w, (n.z*d)/w, (d*d)/w)        = (A upper triangle, b, c)
//             else    q = 0.   The error of x is x^T A x - 2 b^T x + c; its minimiser solves A x = b.
//   place     x0 = pos_sum / count (per component).  mean placement: x0.  quadric placement:
//             r = b - A x0, r_i = b_i - ((A_i0*x0.x + A_i1*x0.y) + A_i2*x0.z)
//             (lambda, V) = jacobi(A): kJacobiSweeps cyclic sweeps over the pairs (0,1), (0,2), (1,2); a pair with
//             a_pq != 0 is rotated by theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta*theta
//             + 1)) (sign(0) = +1), c = 1 / sqrt(t*t + 1), s = t*c:
//               a_pp -= t*a_pq, a_qq += t*a_pq, a_pq = 0, and with r the third index
//               (a_rp, a_rq) = (c*a_rp - s*a_rq, s*a_rp + c*a_rq);  columns p, q of V likewise.
//             lmax = max(lambda_0, lambda_1, lambda_2).  lmax > 0: for i = 0, 1, 2 in order, when lambda_i >
//             1e-3 * lmax:  g = ((V_0i*r.x + V_1i*r.y) + V_2i*r.z) / lambda_i,  x += V_.i * g  (x starts at x0).
//             Fallback to x0 when a coordinate of x is not finite or |x_a - centre_a| > h on some axis, centre_a =
//             lo_a + (c_a + 0.5) * h in fp64.  The result is rounded to fp32.
//   colour    floor(sum / count + 0.5) per channel = (2 sum + count) / (2 count) in integers.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/lnrf.h"

namespace lnrf {
namespace simp {

// Cyclic Jacobi sweeps of the 3x3 eigen-decomposition.  Chosen on the NumPy restatement (tests/test_simplify_cpu.py
// asserts it): over the cells of the test population the largest off-diagonal mass, relative to the Frobenius norm, is
// 3e-6 after 3 sweeps and 7e-24 after 4, so 4 sweeps meet the 1e-15 that is asked for; 6 keeps two sweeps (6 rotations)
// in hand for matrices the population does not hold.
constexpr int kJacobiSweeps = 6;
constexpr double kRankThreshold = 1e-3;  // Lindstrom 2000, section 4.3

struct Grid {
  float lox, loy, loz, inv_h;
  int nx, ny, nz;
};

__host__ __device__ __forceinline__ int cell_coord(float v, float lo, float inv_h, int n) {
#pragma clang fp contract(off)
  const float t = floorf((v - lo) * inv_h);
  return t >= (float)(n - 1) ? n - 1 : (t > 0.0f ? (int)t : 0);
}

__host__ __device__ __forceinline__ int32_t cell_key(const Grid& g, const float* __restrict__ p) {
  const int cx = cell_coord(p[0], g.lox, g.inv_h, g.nx), cy = cell_coord(p[1], g.loy, g.inv_h, g.ny),
            cz = cell_coord(p[2], g.loz, g.inv_h, g.nz);
  return (cx * g.ny + cy) * g.nz + cz;
}

// n = (b - a) x (c - a) in fp64
__host__ __device__ __forceinline__ void tri_normal(const double* a, const double* b, const double* c, double* n) {
#pragma clang fp contract(off)
  const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

// q[10] = the area-weighted plane quadric of the triangle, 0 for a triangle without area
__host__ __device__ __forceinline__ void tri_quadric(const float* __restrict__ tri, double* q) {
#pragma clang fp contract(off)
  const double a[3] = {(double)tri[0], (double)tri[1], (double)tri[2]};
  const double b[3] = {(double)tri[3], (double)tri[4], (double)tri[5]};
  const double c[3] = {(double)tri[6], (double)tri[7], (double)tri[8]};
  double n[3];
  tri_normal(a, b, c, n);
  const double w = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  const double d = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2];
  if (w > 0.0) {
    q[0] = (n[0] * n[0]) / w;
    q[1] = (n[0] * n[1]) / w;
    q[2] = (n[0] * n[2]) / w;
    q[3] = (n[1] * n[1]) / w;
    q[4] = (n[1] * n[2]) / w;
    q[5] = (n[2] * n[2]) / w;
    q[6] = (n[0] * d) / w;
    q[7] = (n[1] * d) / w;
    q[8] = (n[2] * d) / w;
    q[9] = (d * d) / w;
  } else {
#pragma unroll
    for (int i = 0; i < 10; ++i) q[i] = 0.0;
  }
}

// one Jacobi rotation of the pair (P, Q), R the third index; a symmetric (both triangles kept), v the eigenvectors
template <int P, int Q, int R>
__host__ __device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double denom = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / denom;
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = v[k][P], vkq = v[k][Q];
    v[k][P] = c * vkp - s * vkq;
    v[k][Q] = s * vkp + c * vkq;
  }
}

// x[3] = the vertex of one cell from its sums (px, py, pz, q0..q9) and corner count; returns 1 when the quadric
// placement fell back to the mean
__host__ __device__ __forceinline__ int place_vertex(const double* __restrict__ sums, int32_t count, bool quadric,
                                                     const double* centre, double h, double* x) {
#pragma clang fp contract(off)
  const double n = (double)count;
  const double x0[3] = {sums[0] / n, sums[1] / n, sums[2] / n};
  x[0] = x0[0], x[1] = x0[1], x[2] = x0[2];
  if (!quadric) return 0;
  const double* q = sums + 3;
  double a[3][3] = {{q[0], q[1], q[2]}, {q[1], q[3], q[4]}, {q[2], q[4], q[5]}};
  double r[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = q[6 + i] - ((a[i][0] * x0[0] + a[i][1] * x0[1]) + a[i][2] * x0[2]);
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1, 2>(a, v);
    jacobi_rotate<0, 2, 1>(a, v);
    jacobi_rotate<1, 2, 0>(a, v);
  }
  const double lam[3] = {a[0][0], a[1][1], a[2][2]};
  const double lmax = fmax(fmax(lam[0], lam[1]), lam[2]);
  if (!(lmax > 0.0)) return 0;  // A = 0 (only triangles without area): the mean, and not a fallback
  const double cut = kRankThreshold * lmax;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (lam[i] > cut) {
      const double g = ((v[0][i] * r[0] + v[1][i] * r[1]) + v[2][i] * r[2]) / lam[i];
      x[0] = x[0] + v[0][i] * g;
      x[1] = x[1] + v[1][i] * g;
      x[2] = x[2] + v[2][i] * g;
    }
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(x[k]) && fabs(x[k] - centre[k]) <= h;
  if (!ok) {
    x[0] = x0[0], x[1] = x0[1], x[2] = x0[2];
    return 1;
  }
  return 0;
}

}  // namespace simp
}  // namespace lnrf
