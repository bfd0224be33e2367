// simplify.hip — mesh simplification by vertex clustering with quadric error metrics (Lindstrom, "Out-of-core
// simplification of large polygonal models", SIGGRAPH 2000) on a grid of cubic cells; additive, no counterpart in the
// reference.  learn_nerf/simplify.py drives the passes; csrc/simplify_geom.h pins the arithmetic; the NumPy restatement
// is tests/simplify_reference.py.  No entry point allocates, copies or synchronises; the only atomics are integer adds.
//
// Everything is defined on triangle CORNERS: entry e = 3t + k is corner k of triangle t of tris [F, 3, 3], so an indexed
// mesh and its triangle soup give the same bits.
//
//   keys        lnrf_simp_cell_keys: the cell key of each corner (simplify_geom.h).
//   count       lnrf_simp_count_faces: the triangles whose three corners lie in three distinct cells (the survivors), by
//               a sum per workgroup and one integer atomic per workgroup.  The host's search for --target_faces runs it
//               once per grid it tries.
//   segments    the caller stable-sorts the 3F entries by key; a run of equal keys is one cell's segment, its entries in
//               ascending order: order [3F] int32 and seg_start [cells + 1] int32 (occupied cells only).
//   fold        lnrf_simp_accumulate.  Entry e of a segment contributes the vector
//                 u(e) = (corner position as 3 doubles, the 10 quadric coefficients of triangle t or zeros)
//               the quadric only when no EARLIER corner of t has the same key, so a triangle counts once per distinct
//               cell among its corners.  With u_0 .. u_{L-1} the segment's contributions in order and u_i = +0 for
//               i >= L, chunk m is the balanced tree over u_{16m} .. u_{16m+15}
//                 level 1: x_j = u_j + u_{j+8} (j < 8), level 2: y_j = x_j + x_{j+4}, level 3: z_j = y_j + y_{j+2},
//                 chunk = z_0 + z_1
//               (an xor butterfly over 16 lanes, offsets 8, 4, 2, 1) and the segment's sum is
//                 ((0 + chunk_0) + chunk_1) + ... + chunk_{ceil(L/16)-1},
//               per component, in fp64.  This order is a function of the segment alone.  Two launch shapes compute it:
//               a 16-lane group per cell, one chunk per step (short segments), or a wave per cell, four chunks per step
//               whose sums are added in chunk order (long segments; a further +0 chunk at the end is the identity,
//               because the running sum is never -0).  shape = 0 gives segments of at most kLongSegment entries to the
//               first and the others to the second, 1 and 2 force one shape for every segment: same bits.
//               The corner count is the segment length and the colour sums are integers: exact in any order.
//   place       lnrf_simp_place: one lane per occupied cell (simplify_geom.h).
//   flipped     lnrf_simp_flipped: output faces whose fp64 normal (from the fp32 output vertices) has a negative dot
//               product with the fp64 normal of their input triangle; integer atomics.
#include <cmath>

#include "common.h"
#include "simplify_geom.h"

namespace lnrf {
namespace simp {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;         // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kCountMaxGrid = 1024;    // the counting kernels end in one atomic per workgroup
constexpr int kFoldMaxGrid = 1 << 16;  // the fold's groups stride over the cells beyond this
constexpr int kChunk = 16;
constexpr int kLongSegment = 256;  // entries; above it a wave takes the segment
constexpr int kSums = 13;          // 3 position sums + 10 quadric coefficients

__global__ __launch_bounds__(kBlock) void cell_keys_kernel(Grid g, const float* __restrict__ pts, int64_t n,
                                                           int32_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    keys[i] = cell_key(g, pts + 3 * i);
}

// *count += the workgroup's sum of `mine`: a butterfly per wave, the four waves through LDS, one integer atomic per
// workgroup (thousands of waves adding to one address queue up behind each other)
__device__ __forceinline__ void block_count(unsigned long long mine, unsigned long long* __restrict__ count) {
  __shared__ unsigned long long s_part[kBlock / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    if (total) atomicAdd(count, total);
  }
}

__global__ __launch_bounds__(kBlock) void count_faces_kernel(Grid g, const float* __restrict__ tris, int64_t n,
                                                             unsigned long long* __restrict__ count) {
  unsigned long long mine = 0;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) {
    const float* p = tris + 9 * t;
    const int32_t k0 = cell_key(g, p), k1 = cell_key(g, p + 3), k2 = cell_key(g, p + 6);
    mine += (k0 != k1 && k1 != k2 && k0 != k2) ? 1u : 0u;
  }
  block_count(mine, count);
}

// u(e) of the header comment; zeros for an entry outside the segment or outside [0, 3F)
__device__ __forceinline__ void entry_terms(const float* __restrict__ tris, const int32_t* __restrict__ keys,
                                            const uint8_t* __restrict__ colors, int64_t n_entries, bool live, int32_t e,
                                            double* u, unsigned long long* rgb) {
#pragma unroll
  for (int i = 0; i < kSums; ++i) u[i] = 0.0;
  if (!live || e < 0 || (int64_t)e >= n_entries) return;
  const int32_t t = e / 3, k = e - 3 * t;
  const float* tri = tris + 9 * (int64_t)t;
  const int32_t* tk = keys + 3 * (int64_t)t;
  const int32_t k0 = tk[0], k1 = tk[1], k2 = tk[2];
  u[0] = (double)tri[3 * k], u[1] = (double)tri[3 * k + 1], u[2] = (double)tri[3 * k + 2];
  const bool first = k == 0 || (k == 1 && k1 != k0) || (k == 2 && k2 != k0 && k2 != k1);
  if (first) tri_quadric(tri, u + 3);
  if (colors) {
    const uint8_t* c = colors + 3 * (int64_t)e;
    rgb[0] += c[0], rgb[1] += c[1], rgb[2] += c[2];
  }
}

// GROUP lanes per cell (16: one chunk per step, 64: four); cells whose length is in (min_len, max_len] only
template <int GROUP>
__global__ __launch_bounds__(kBlock) void accumulate_kernel(const float* __restrict__ tris, int64_t n_entries,
                                                            const int32_t* __restrict__ keys,
                                                            const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ seg_start, int64_t n_cells,
                                                            const uint8_t* __restrict__ colors, int64_t min_len,
                                                            int64_t max_len, int32_t* __restrict__ counts,
                                                            double* __restrict__ sums,
                                                            long long* __restrict__ col_sums) {
  constexpr int kGroups = kBlock / GROUP;
  const int lane = threadIdx.x % GROUP;
  for (int64_t cell = (int64_t)blockIdx.x * kGroups + threadIdx.x / GROUP; cell < n_cells;
       cell += (int64_t)gridDim.x * kGroups) {
    int64_t s0 = seg_start[cell], s1 = seg_start[cell + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_entries ? n_entries : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_entries ? n_entries : s1);
    const int64_t len = s1 - s0;
    if (len <= min_len || len > max_len) continue;
    double acc[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
    unsigned long long rgb[3] = {0, 0, 0};
    for (int64_t base = s0; base < s1; base += GROUP) {
      const int64_t s = base + lane;
      const bool live = s < s1;
      double u[kSums];
      entry_terms(tris, keys, colors, n_entries, live, live ? order[s] : 0, u, rgb);
#pragma unroll
      for (int i = 0; i < kSums; ++i) {
        double x = u[i];
#pragma unroll
        for (int off = kChunk / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kChunk);
        if (GROUP == kChunk) {
          acc[i] += x;
        } else {
#pragma unroll
          for (int c = 0; c < GROUP / kChunk; ++c) acc[i] += __shfl(x, c * kChunk, GROUP);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int off = GROUP / 2; off > 0; off >>= 1) rgb[c] += __shfl_xor(rgb[c], off, GROUP);
    }
    if (lane == 0) {
      counts[cell] = (int32_t)len;
#pragma unroll
      for (int i = 0; i < kSums; ++i) sums[kSums * cell + i] = acc[i];
      if (col_sums) {
#pragma unroll
        for (int c = 0; c < 3; ++c) col_sums[3 * cell + c] = (long long)rgb[c];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void place_kernel(Grid g, double h, const int32_t* __restrict__ cell_keys,
                                                       const int32_t* __restrict__ counts,
                                                       const double* __restrict__ sums,
                                                       const long long* __restrict__ col_sums, int64_t n_cells,
                                                       int quadric, float* __restrict__ verts,
                                                       uint8_t* __restrict__ colors, uint8_t* __restrict__ fell_back) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * kBlock) {
    const int32_t count = counts[i] > 0 ? counts[i] : 1;  // an occupied cell has a corner; 1 keeps a bad input finite
    const int32_t key = cell_keys[i];
    const int cz = key % g.nz, cy = (key / g.nz) % g.ny, cx = key / (g.nz * g.ny);
    double centre[3], x[3], s[kSums];
    {
#pragma clang fp contract(off)
      centre[0] = (double)g.lox + ((double)cx + 0.5) * h;
      centre[1] = (double)g.loy + ((double)cy + 0.5) * h;
      centre[2] = (double)g.loz + ((double)cz + 0.5) * h;
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = sums[kSums * i + k];
    const int fb = place_vertex(s, count, quadric != 0, centre, h, x);
    verts[3 * i] = (float)x[0], verts[3 * i + 1] = (float)x[1], verts[3 * i + 2] = (float)x[2];
    fell_back[i] = (uint8_t)fb;
    if (colors) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long v = (2 * col_sums[3 * i + c] + count) / (2 * (long long)count);
        colors[3 * i + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void flipped_kernel(const float* __restrict__ tris, int64_t n_tris,
                                                         const int32_t* __restrict__ face_src,
                                                         const int32_t* __restrict__ faces, int64_t n_faces,
                                                         const float* __restrict__ verts, int64_t n_verts,
                                                         unsigned long long* __restrict__ count) {
  unsigned long long mine = 0;
  for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * kBlock) {
    const int32_t t = face_src[f], i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (t < 0 || t >= n_tris || i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) continue;
    double a[3], b[3], c[3], n_in[3], n_out[3];
    const float* tri = tris + 9 * (int64_t)t;
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = (double)tri[k], b[k] = (double)tri[3 + k], c[k] = (double)tri[6 + k];
    tri_normal(a, b, c, n_in);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)verts[3 * (int64_t)i0 + k];
      b[k] = (double)verts[3 * (int64_t)i1 + k];
      c[k] = (double)verts[3 * (int64_t)i2 + k];
    }
    tri_normal(a, b, c, n_out);
    double dot;
    {
#pragma clang fp contract(off)
      dot = (n_in[0] * n_out[0] + n_in[1] * n_out[1]) + n_in[2] * n_out[2];
    }
    mine += dot < 0.0 ? 1u : 0u;
  }
  block_count(mine, count);
}

static int check_grid(const char* fn, const lnrf_simp_grid* grid, Grid* g) {
  if (!grid) {
    set_error("%s: null grid", fn);
    return LNRF_ERR_ARG;
  }
  if (!(grid->inv_h > 0.0f) || !std::isfinite(grid->inv_h) || !std::isfinite(grid->lo[0]) ||
      !std::isfinite(grid->lo[1]) || !std::isfinite(grid->lo[2])) {
    set_error("%s: the grid needs a finite origin and a finite inverse cell edge > 0", fn);
    return LNRF_ERR_ARG;
  }
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (grid->dims[a] < 1) {
      set_error("%s: grid dimensions [%d, %d, %d] must each be at least 1", fn, grid->dims[0], grid->dims[1],
                grid->dims[2]);
      return LNRF_ERR_SHAPE;
    }
    cells *= grid->dims[a];  // at most 2^31 * 2^31 before the check below: no overflow
    if (cells > INT32_MAX) {
      set_error("%s: grid [%d, %d, %d] has 2^31 cells or more: the cell key is an int32", fn, grid->dims[0],
                grid->dims[1], grid->dims[2]);
      return LNRF_ERR_SHAPE;
    }
  }
  *g = Grid{grid->lo[0], grid->lo[1], grid->lo[2], grid->inv_h, grid->dims[0], grid->dims[1], grid->dims[2]};
  return LNRF_OK;
}

// 0 <= n and 3 n <= INT32_MAX when the count is of triangles (entries are int32)
static int check_count(const char* fn, const char* what, int64_t n, int64_t limit) {
  if (n < 0) {
    set_error("%s: negative %s count", fn, what);
    return LNRF_ERR_ARG;
  }
  if (n > limit) {
    set_error("%s: %lld %s do not fit in int32 indices", fn, (long long)n, what);
    return LNRF_ERR_SHAPE;
  }
  return LNRF_OK;
}

static inline int grid_for(int64_t n, int per_block, int cap) {
  const int64_t blocks = (n + per_block - 1) / per_block;
  return (int)(blocks < cap ? blocks : cap);
}

}  // namespace simp
}  // namespace lnrf

using namespace lnrf;

extern "C" int lnrf_simp_cell_keys(const lnrf_simp_grid* grid, const float* pts, int64_t n, int32_t* keys,
                                   lnrf_stream_t stream) {
  simp::Grid g;
  int rc = simp::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "points", n, INT32_MAX);
  if (rc != LNRF_OK) return rc;
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(pts && keys, "null pointer");
  hipLaunchKernelGGL(simp::cell_keys_kernel, dim3(simp::grid_for(n, simp::kBlock, simp::kMaxGrid)),
                     dim3(simp::kBlock), 0, as_stream(stream), g, pts, n, keys);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_simp_count_faces(const lnrf_simp_grid* grid, const float* tris, int64_t n_tris, int64_t* count,
                                     lnrf_stream_t stream) {
  simp::Grid g;
  int rc = simp::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "triangles", n_tris, INT32_MAX / 3);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(count, "null pointer");
  if (n_tris == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris, "null pointer");
  hipLaunchKernelGGL(simp::count_faces_kernel, dim3(simp::grid_for(n_tris, simp::kBlock, simp::kCountMaxGrid)),
                     dim3(simp::kBlock), 0, as_stream(stream), g, tris, n_tris,
                     reinterpret_cast<unsigned long long*>(count));
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int32_t lnrf_simp_long_segment(void) { return simp::kLongSegment; }

extern "C" int lnrf_simp_accumulate(const float* tris, int64_t n_tris, const int32_t* keys, const int32_t* order,
                                    const int32_t* seg_start, int64_t n_cells, const uint8_t* colors, int32_t shape,
                                    int32_t* counts, double* sums, int64_t* col_sums, lnrf_stream_t stream) {
  int rc = simp::check_count(__func__, "triangles", n_tris, INT32_MAX / 3);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "cells", n_cells, INT32_MAX);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(shape >= 0 && shape <= 2, "shape must be 0 (by length), 1 (16-lane groups) or 2 (waves)");
  LNRF_CHECK_ARG(n_cells <= 3 * n_tris, "more cells than corners");
  LNRF_CHECK_ARG((colors == nullptr) == (col_sums == nullptr), "colors and col_sums go together");
  if (n_cells == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris && keys && order && seg_start && counts && sums, "null pointer");
  const int64_t n_entries = 3 * n_tris, all = INT64_MAX;
  long long* cs = reinterpret_cast<long long*>(col_sums);
  if (shape != 2) {
    const int64_t max_len = shape == 0 ? simp::kLongSegment : all;
    hipLaunchKernelGGL(simp::accumulate_kernel<16>, dim3(simp::grid_for(n_cells, simp::kBlock / 16, simp::kFoldMaxGrid)),
                       dim3(simp::kBlock), 0, as_stream(stream), tris, n_entries, keys, order, seg_start, n_cells,
                       colors, (int64_t)0, max_len, counts, sums, cs);
    LNRF_LAUNCH_CHECK();
  }
  if (shape != 1) {
    const int64_t min_len = shape == 0 ? simp::kLongSegment : 0;
    const int cap = shape == 0 ? simp::kMaxGrid : simp::kFoldMaxGrid;  // by length: few segments are long
    hipLaunchKernelGGL(simp::accumulate_kernel<64>, dim3(simp::grid_for(n_cells, simp::kBlock / 64, cap)),
                       dim3(simp::kBlock), 0, as_stream(stream), tris, n_entries, keys, order, seg_start, n_cells,
                       colors, min_len, all, counts, sums, cs);
    LNRF_LAUNCH_CHECK();
  }
  return LNRF_OK;
}

extern "C" int lnrf_simp_place(const lnrf_simp_grid* grid, double h, const int32_t* cell_keys, const int32_t* counts,
                               const double* sums, const int64_t* col_sums, int64_t n_cells, int32_t placement,
                               float* verts, uint8_t* colors, uint8_t* fell_back, lnrf_stream_t stream) {
  simp::Grid g;
  int rc = simp::check_grid(__func__, grid, &g);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "cells", n_cells, INT32_MAX);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(h > 0.0 && std::isfinite(h), "the cell edge must be finite and > 0");
  LNRF_CHECK_ARG(placement == LNRF_SIMP_MEAN || placement == LNRF_SIMP_QUADRIC, "unknown placement");
  LNRF_CHECK_ARG((colors == nullptr) == (col_sums == nullptr), "colors and col_sums go together");
  if (n_cells == 0) return LNRF_OK;
  LNRF_CHECK_ARG(cell_keys && counts && sums && verts && fell_back, "null pointer");
  hipLaunchKernelGGL(simp::place_kernel, dim3(simp::grid_for(n_cells, simp::kBlock, simp::kMaxGrid)),
                     dim3(simp::kBlock), 0, as_stream(stream), g, h, cell_keys, counts, sums,
                     reinterpret_cast<const long long*>(col_sums), n_cells, (int)(placement == LNRF_SIMP_QUADRIC),
                     verts, colors, fell_back);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_simp_flipped(const float* tris, int64_t n_tris, const int32_t* face_src, const int32_t* faces,
                                 int64_t n_faces, const float* verts, int64_t n_verts, int64_t* count,
                                 lnrf_stream_t stream) {
  int rc = simp::check_count(__func__, "triangles", n_tris, INT32_MAX / 3);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "faces", n_faces, INT32_MAX / 3);
  if (rc == LNRF_OK) rc = simp::check_count(__func__, "vertices", n_verts, INT32_MAX);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(count, "null pointer");
  if (n_faces == 0) return LNRF_OK;
  LNRF_CHECK_ARG(tris && face_src && faces && verts, "null pointer");
  hipLaunchKernelGGL(simp::flipped_kernel, dim3(simp::grid_for(n_faces, simp::kBlock, simp::kCountMaxGrid)),
                     dim3(simp::kBlock), 0, as_stream(stream), tris, n_tris, face_src, faces, n_faces, verts, n_verts,
                     reinterpret_cast<unsigned long long*>(count));
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
