// pointcloud.hip — exact neighbour search over a point cloud on a uniform grid of cubic cells: the three KD-tree
// queries of the reference's point_cloud/main.go (tree.KNN for -sort-density :177-187, tree.Dist for the solid
// :111-118, tree.NearestNeighbor for the colours :123-125).  No allocation, copy, synchronisation or atomic in any entry
// point; every result depends on the points and the query alone, not on the launch geometry and not on the cell edge.
//
// Conventions (learn_nerf/point_cloud.py and the NumPy restatement tests/point_cloud_reference.py rely on them):
//   grid      lnrf_pc_grid: origin lo, cell edge h > 0, dimensions [gx, gy, gz], each in [1, 4096], at most 2^24 cells.
//             Cell (cx, cy, cz) has linear id (cx*gy + cy)*gz + cz (int32), so a run of cells along z is contiguous.
//   cell of   c_a = clamp(int(floor((p_a - lo_a) / h)), 0, g_a - 1), the subtraction and the division each rounded
//   a point   once in fp32.  Clamping puts a point on the upper face (or anywhere outside) into the last cell.
//   points    sorted by cell id (stable, by the caller): sorted_pts [n, 3] fp32, order [n] int32 = the original index
//             of each sorted point, cell_start [ncells + 1] int32 = first sorted point of each cell, [ncells] = n.
//   distance  dx = q.x - p.x, dy, dz likewise; d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded once (no FMA
//             contraction: `#pragma clang fp contract(off)` in dist2), so NumPy float32 gives the same bits.
//   knn       squared distance to the k-th nearest point, 1 <= k <= 32; a query that is one of the points counts
//             itself (distance 0); +inf when n < k.
//   nearest   smallest d2 and the original index of that point; among equal d2 the lowest original index; only
//             points with d2 <= max_radius*max_radius (one fp32 multiply; max_radius may be +inf) count, and a query
//             without one gets index -1 and +inf.  The query may lie anywhere, also outside the grid.
//
// Search: Chebyshev rings of cells around the query's (clamped) cell, ring r = the cells at Chebyshev distance exactly
// r, clipped to the grid and walked face by face; on the ring's x and y faces a column's whole z extent is one
// contiguous run of sorted points.  The search stops after ring r when the k-th best d2 is
// below the bound of that ring (strictly: a tie at the bound could hide a lower index), when the bound exceeds
// max_radius^2, or when the ring has covered the whole grid: max_a max(c_a, g_a - 1 - c_a) rings reach every cell.
//
// Ring bound, with the fp32 margin it needs.  A point not visited by rings 0..r differs from the query's cell by at
// least r + 1 on some axis a.  With t(x) = (x - lo_a) / h exact and T(x) its fp32 evaluation, T is monotone and
// |T - t| <= 2.01 * 2^-24 * |t|, and every point has t < g_a <= 4096, so t(p) and t(q) differ by more than
// r - 4.02 * 2^-24 * 4096 > r - 0.001 cells (a query clamped from outside the grid lies further still: the host sets
// g_a = floor(extent_a / h) + 1, so t(hi_a) >= g_a - 1).  The pinned d2 of such a point is at least
// ((r - 0.001) h)^2 (1 - 2^-24)^5.  The kernels use bound2 = fl(B*B) * (1 - 2^-20) with B = fl(fl(r - 0.01) * h) for
// r >= 1 and 0 for ring 0: the margin of 0.01 cells is ten times the error, and the factor covers the roundings of B,
// of its square and of d2 (r <= 4096, so 0.009 / r > 2e-6 against a few 2^-24).  A margin is therefore required and
// applied; it costs a further ring only when the k-th best d2 falls within 2 % of the bound.
//
// One thread per query; the caller passes the queries in cell order so that the lanes of a wave walk the same cells
// and their loads hit the same lines.  The k best are a sorted register array of KMAX = 1, 4, 8, 16 or 32 entries
// (the smallest that holds k) with a fully unrolled insertion, so no index is a runtime value.
#include <cmath>

#include "common.h"

namespace lnrf {
namespace pc {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kMaxDim = 4096;   // per axis: the ring bound's margin is proven for t < 4096
constexpr int64_t kMaxCells = (int64_t)1 << 24;
constexpr int kMaxK = 32;
constexpr float kRingMargin = 0.01f;
constexpr float kBoundScale = 1.0f - 0x1p-20f;

struct Grid {
  float lox, loy, loz, h;
  int gx, gy, gz;
};

__device__ __forceinline__ int cell_coord(float p, float lo, float h, int g) {
  const float t = floorf((p - lo) / h);  // hipcc's default fp32 divide is correctly rounded
  // compare in float: t may be far outside the int range (NaN goes to cell 0; the Python layer rejects it)
  return t >= (float)(g - 1) ? g - 1 : (t > 0.0f ? (int)t : 0);
}

// the pinned distance: contraction off, so every product and sum is rounded on its own (hipcc's __fmul_rn / __fadd_rn
// are plain operators that the default -ffp-contract=fast-honor-pragmas would still fuse)
__device__ __forceinline__ float dist2(float qx, float qy, float qz, const float* __restrict__ p) {
#pragma clang fp contract(off)
  const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// lower bound of the pinned d2 of every point outside rings 0..r
__device__ __forceinline__ float ring_bound2(int r, float h) {
#pragma clang fp contract(off)
  if (r < 1) return 0.0f;
  const float b = ((float)r - kRingMargin) * h;
  return (b * b) * kBoundScale;
}

// Visits every sorted-point run of ring r around cell (cx, cy, cz): f(begin, end).  Only cells inside the grid are
// walked, face by face, so a ring far beyond the grid on two axes costs what is left of it on the third: the two x
// faces (whole z runs of every column), the two y faces without the x faces' columns, and the end cells of the columns
// strictly inside.
template <class F>
__device__ __forceinline__ void for_ring(const Grid& g, const int32_t* __restrict__ cell_start, int cx, int cy, int cz,
                                         int r, F&& f) {
  if (r == 0) {
    const int c = (cx * g.gy + cy) * g.gz + cz;
    f(cell_start[c], cell_start[c + 1]);
    return;
  }
  const int y0 = max(cy - r, 0), y1 = min(cy + r, g.gy - 1);
  const int z0 = max(cz - r, 0), z1 = min(cz + r, g.gz - 1);
  const int xi0 = max(cx - r + 1, 0), xi1 = min(cx + r - 1, g.gx - 1);  // strictly inside the x faces
  const int yi0 = max(cy - r + 1, 0), yi1 = min(cy + r - 1, g.gy - 1);
  for (int side = 0; side < 2; ++side) {
    const int x = side ? cx + r : cx - r;
    if (x < 0 || x >= g.gx) continue;
    for (int y = y0; y <= y1; ++y) {
      const int col = (x * g.gy + y) * g.gz;
      f(cell_start[col + z0], cell_start[col + z1 + 1]);
    }
  }
  for (int side = 0; side < 2; ++side) {
    const int y = side ? cy + r : cy - r;
    if (y < 0 || y >= g.gy) continue;
    for (int x = xi0; x <= xi1; ++x) {
      const int col = (x * g.gy + y) * g.gz;
      f(cell_start[col + z0], cell_start[col + z1 + 1]);
    }
  }
  for (int side = 0; side < 2; ++side) {
    const int z = side ? cz + r : cz - r;
    if (z < 0 || z >= g.gz) continue;
    for (int x = xi0; x <= xi1; ++x) {
      for (int y = yi0; y <= yi1; ++y) {
        const int c = (x * g.gy + y) * g.gz + z;
        f(cell_start[c], cell_start[c + 1]);
      }
    }
  }
}

__device__ __forceinline__ int last_ring(const Grid& g, int cx, int cy, int cz) {
  return max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
}

__global__ __launch_bounds__(kBlock) void pc_cell_ids_kernel(Grid g, const float* __restrict__ pts, int64_t n,
                                                             int32_t* __restrict__ ids) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const float* p = pts + 3 * i;
    const int cx = cell_coord(p[0], g.lox, g.h, g.gx), cy = cell_coord(p[1], g.loy, g.h, g.gy),
              cz = cell_coord(p[2], g.loz, g.h, g.gz);
    ids[i] = (cx * g.gy + cy) * g.gz + cz;
  }
}

template <int KMAX>
__global__ __launch_bounds__(kBlock) void pc_knn_kernel(Grid g, const float* __restrict__ sorted_pts,
                                                        const int32_t* __restrict__ cell_start,
                                                        const float* __restrict__ queries, int64_t m, int k,
                                                        float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const float qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
    const int cx = cell_coord(qx, g.lox, g.h, g.gx), cy = cell_coord(qy, g.loy, g.h, g.gy),
              cz = cell_coord(qz, g.loz, g.h, g.gz);
    float best[KMAX];  // ascending; best[k - 1] is the k-th nearest so far
#pragma unroll
    for (int s = 0; s < KMAX; ++s) best[s] = INFINITY;
    float kth = INFINITY;
    const int rmax = last_ring(g, cx, cy, cz);
    for (int r = 0; r <= rmax; ++r) {
      for_ring(g, cell_start, cx, cy, cz, r, [&](int begin, int end) {
        for (int j = begin; j < end; ++j) {
          float d = dist2(qx, qy, qz, sorted_pts + 3 * (int64_t)j);
          if (d < kth) {
#pragma unroll
            for (int s = 0; s < KMAX; ++s) {
              const float lo = fminf(d, best[s]);
              d = fmaxf(d, best[s]);
              best[s] = lo;
            }
            kth = INFINITY;
#pragma unroll
            for (int s = 0; s < KMAX; ++s) kth = s == k - 1 ? best[s] : kth;
          }
        }
      });
      if (kth < ring_bound2(r, g.h)) break;
    }
    out[i] = kth;
  }
}

__global__ __launch_bounds__(kBlock) void pc_nearest_kernel(Grid g, const float* __restrict__ sorted_pts,
                                                            const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ cell_start,
                                                            const float* __restrict__ queries, int64_t m,
                                                            float max_radius, float* __restrict__ out_d2,
                                                            int32_t* __restrict__ out_idx) {
  const float r2 = max_radius * max_radius;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const float qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
    const int cx = cell_coord(qx, g.lox, g.h, g.gx), cy = cell_coord(qy, g.loy, g.h, g.gy),
              cz = cell_coord(qz, g.loz, g.h, g.gz);
    float best = INFINITY;
    int best_idx = -1;
    const int rmax = last_ring(g, cx, cy, cz);
    for (int r = 0; r <= rmax; ++r) {
      for_ring(g, cell_start, cx, cy, cz, r, [&](int begin, int end) {
        for (int j = begin; j < end; ++j) {
          const float d = dist2(qx, qy, qz, sorted_pts + 3 * (int64_t)j);
          if (d <= r2 && d <= best) {
            const int idx = order[j];
            if (d < best || idx < best_idx) {  // best_idx >= 0 whenever d == best is finite or best was set
              best = d;
              best_idx = idx;
            }
          }
        }
      });
      const float bound2 = ring_bound2(r, g.h);
      if ((best_idx >= 0 && best < bound2) || bound2 > r2) break;
    }
    out_d2[i] = best_idx >= 0 ? best : INFINITY;
    out_idx[i] = best_idx;
  }
}

static int check_grid(const char* fn, const lnrf_pc_grid* grid, Grid* g) {
  if (!grid) {
    set_error("%s: null grid", fn);
    return LNRF_ERR_ARG;
  }
  if (!(grid->h > 0.0f) || !std::isfinite(grid->h) || !std::isfinite(grid->lo[0]) || !std::isfinite(grid->lo[1]) ||
      !std::isfinite(grid->lo[2])) {
    set_error("%s: the grid needs a finite origin and a finite cell edge > 0", fn);
    return LNRF_ERR_ARG;
  }
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (grid->dims[a] < 1 || grid->dims[a] > kMaxDim) {
      set_error("%s: grid dimensions [%d, %d, %d] must each lie in [1, %d]", fn, grid->dims[0], grid->dims[1],
                grid->dims[2], kMaxDim);
      return LNRF_ERR_SHAPE;
    }
    cells *= grid->dims[a];
  }
  if (cells > kMaxCells) {
    set_error("%s: %lld cells exceed the cap of %lld", fn, (long long)cells, (long long)kMaxCells);
    return LNRF_ERR_SHAPE;
  }
  *g = Grid{grid->lo[0], grid->lo[1], grid->lo[2], grid->h, grid->dims[0], grid->dims[1], grid->dims[2]};
  return LNRF_OK;
}

static int check_count(const char* fn, const char* what, int64_t n) {
  if (n < 0) {
    set_error("%s: negative %s count", fn, what);
    return LNRF_ERR_ARG;
  }
  if (n > INT32_MAX) {
    set_error("%s: %lld %s do not fit in int32 indices", fn, (long long)n, what);
    return LNRF_ERR_SHAPE;
  }
  return LNRF_OK;
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
}

}  // namespace pc
}  // namespace lnrf

using namespace lnrf;

extern "C" int lnrf_pc_cell_ids(const lnrf_pc_grid* grid, const float* pts, int64_t n, int32_t* ids,
                                lnrf_stream_t stream) {
  pc::Grid g;
  int rc = pc::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = pc::check_count(__func__, "points", n);
  if (rc != LNRF_OK) return rc;
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(pts && ids, "null pointer");
  hipLaunchKernelGGL(pc::pc_cell_ids_kernel, dim3(pc::grid_for(n)), dim3(pc::kBlock), 0, as_stream(stream), g, pts, n,
                     ids);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_pc_knn_dist2(const lnrf_pc_grid* grid, const float* sorted_pts, const int32_t* cell_start,
                                 int64_t n, const float* queries, int64_t m, int32_t k, float* out_d2,
                                 lnrf_stream_t stream) {
  pc::Grid g;
  int rc = pc::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = pc::check_count(__func__, "points", n);
  if (rc == LNRF_OK) rc = pc::check_count(__func__, "queries", m);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(k >= 1, "k must be at least 1");
  if (k > pc::kMaxK) {
    set_error("%s: k = %d, at most %d neighbours are supported", __func__, k, pc::kMaxK);
    return LNRF_ERR_UNSUPPORTED;
  }
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(cell_start && queries && out_d2 && (sorted_pts || n == 0), "null pointer");
  const dim3 blocks(pc::grid_for(m)), threads(pc::kBlock);
#define LNRF_PC_KNN(KMAX)                                                                                       \
  hipLaunchKernelGGL(pc::pc_knn_kernel<KMAX>, blocks, threads, 0, as_stream(stream), g, sorted_pts, cell_start, \
                     queries, m, (int)k, out_d2)
  if (k == 1) LNRF_PC_KNN(1);
  else if (k <= 4) LNRF_PC_KNN(4);
  else if (k <= 8) LNRF_PC_KNN(8);
  else if (k <= 16) LNRF_PC_KNN(16);
  else LNRF_PC_KNN(32);
#undef LNRF_PC_KNN
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_pc_nearest(const lnrf_pc_grid* grid, const float* sorted_pts, const int32_t* order,
                               const int32_t* cell_start, int64_t n, const float* queries, int64_t m,
                               float max_radius, float* out_d2, int32_t* out_idx, lnrf_stream_t stream) {
  pc::Grid g;
  int rc = pc::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = pc::check_count(__func__, "points", n);
  if (rc == LNRF_OK) rc = pc::check_count(__func__, "queries", m);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(max_radius >= 0.0f, "max_radius must be >= 0 (NaN is not)");
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(cell_start && queries && out_d2 && out_idx && ((sorted_pts && order) || n == 0), "null pointer");
  hipLaunchKernelGGL(pc::pc_nearest_kernel, dim3(pc::grid_for(m)), dim3(pc::kBlock), 0, as_stream(stream), g,
                     sorted_pts, order, cell_start, queries, m, max_radius, out_d2, out_idx);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
