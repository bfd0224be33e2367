// tsdf.hip — truncated-signed-distance fusion of RGB-D views into a voxel grid (Curless & Levoy), the volume that
// marching cubes (mesh.hip) turns into a single-surface mesh, and that mesh's vertex colours.  Additive: no counterpart
// in the reference.  The per-voxel, per-view arithmetic and the vertex-colour rule are tsdf_geom.h, whose header fixes
// the conventions; learn_nerf/tsdf.py drives the passes and tests/tsdf_reference.py restates them in NumPy.
//
// State (caller-owned, zeroed before the first launch), one entry per voxel, linear index (i*ny + j)*nz + k:
//   sum_t f32, n_obs i32, behind u8, rgb_sum i32 [N, 3], n_col i32.
//
// Passes
//   integrate      one lane per voxel, one wave per tile of 4 x 4 x 4 voxels (lane = (li*4 + lj)*4 + lk), the waves of a
//                  workgroup and then the workgroups walking the tiles with k fastest (tile-stride beyond the grid
//                  cap).  The lane loads its voxel's state once, walks the launch's views in order with the state in
//                  registers, and stores it once.  The view descriptors are read at a wave-uniform index.  The depth
//                  and colour gathers are element-granular; a tile projects into a patch of a few pixels square, so
//                  the 64 addresses of a gather fall into a handful of cache lines.  With lanes along k instead (a
//                  wave = 64 voxels of one grid line, whose projection crosses up to 64 image rows) the same kernel
//                  took 5.5x as long at 256^3 and 3.4x at 512^3 (DESIGN.md section 4 "TSDF fusion"); the state is moved once
//                  per launch, the gathers once per view, so the tile wins although its state accesses come in runs
//                  of 4 voxels.  No atomics, no scratch: a voxel's result depends on the sequence of views alone, not
//                  on the launch geometry and not on how the views are split over launches (the state between two
//                  launches is exactly the registers' content).
//   volume         one lane per point of the padded volume [nx+2, ny+2, nz+2]: -1 on the padding layer, -F inside.
//   vertex_colors  one lane per vertex; the vertices without a colour are counted per wave, one integer atomic each.
//
// No entry point allocates, copies or synchronises; lnrf_tsdf_vertex_colors clears *n_missing with a memset node.
#include <limits.h>

#include "common.h"
#include "tsdf_geom.h"

static_assert(sizeof(lnrf_tsdf_view) == 88, "learn_nerf/tsdf.py packs lnrf_tsdf_view as 88 bytes");

namespace lnrf {
namespace tsdf {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxGrid = 256 * 8 * 4;  // 256 CUs x 8 workgroups x 4, grid-stride beyond
constexpr int kTile = 4;               // a wave's tile is kTile^3 = 64 voxels
static_assert(kTile * kTile * kTile == kWave, "one voxel per lane");

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(
    const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs, int nx, int ny, int nz,
    const lnrf_tsdf_view* __restrict__ views, int n_views, const uint16_t* __restrict__ depth,
    const uint8_t* __restrict__ color, float trunc, float max_depth, int carve, float* __restrict__ sum_t,
    int32_t* __restrict__ n_obs, uint8_t* __restrict__ behind, int32_t* __restrict__ rgb_sum,
    int32_t* __restrict__ n_col) {
  const int lane = threadIdx.x & (kWave - 1);
  const int li = lane / (kTile * kTile), lj = (lane / kTile) % kTile, lk = lane % kTile;
  const int tiles_j = (ny + kTile - 1) / kTile, tiles_k = (nz + kTile - 1) / kTile;
  const int64_t tiles = (int64_t)((nx + kTile - 1) / kTile) * tiles_j * tiles_k;
  // the wave's index, as a scalar: the tile arithmetic below is then wave-uniform
  const int64_t first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave));
  for (int64_t tile = first; tile < tiles; tile += (int64_t)gridDim.x * kWavesPerBlock) {
    const int tk = (int)(tile % tiles_k), tj = (int)((tile / tiles_k) % tiles_j), ti = (int)(tile / tiles_k / tiles_j);
    const int i = ti * kTile + li, j = tj * kTile + lj, k = tk * kTile + lk;
    if (i >= nx || j >= ny || k >= nz) continue;  // a tile that sticks out of the grid
    const int64_t cell = ((int64_t)i * ny + j) * nz + k;
    const float px = xs[i], py = ys[j], pz = zs[k];
    VoxelState st;
    st.sum_t = sum_t[cell];
    st.n_obs = n_obs[cell];
    st.behind = behind[cell];
    st.r = rgb_sum[3 * cell];
    st.g = rgb_sum[3 * cell + 1];
    st.b = rgb_sum[3 * cell + 2];
    st.n_col = n_col[cell];
    for (int v = 0; v < n_views; ++v) update_voxel(st, px, py, pz, views[v], depth, color, trunc, max_depth, carve != 0);
    sum_t[cell] = st.sum_t;
    n_obs[cell] = st.n_obs;
    behind[cell] = st.behind ? 1 : 0;
    rgb_sum[3 * cell] = st.r;
    rgb_sum[3 * cell + 1] = st.g;
    rgb_sum[3 * cell + 2] = st.b;
    n_col[cell] = st.n_col;
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_volume_kernel(const float* __restrict__ sum_t,
                                                             const int32_t* __restrict__ n_obs,
                                                             const uint8_t* __restrict__ behind, int nx, int ny, int nz,
                                                             int unseen_inside, float* __restrict__ out) {
  const int64_t py = ny + 2, pz = nz + 2, plane = py * pz, total = (int64_t)(nx + 2) * plane;
  for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += (int64_t)gridDim.x * kBlock) {
    const int i = (int)(o / plane) - 1, j = (int)((o % plane) / pz) - 1, k = (int)(o % pz) - 1;
    float value = -1.0f;
    if (i >= 0 && i < nx && j >= 0 && j < ny && k >= 0 && k < nz) {
      const int64_t cell = ((int64_t)i * ny + j) * nz + k;
      value = volume_value(sum_t[cell], n_obs[cell], behind[cell], unseen_inside != 0);
    }
    out[o] = value;
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_vertex_colors_kernel(const float* __restrict__ verts, int64_t n, int nx,
                                                                    int ny, int nz, const int32_t* __restrict__ rgb_sum,
                                                                    const int32_t* __restrict__ n_col,
                                                                    float* __restrict__ rgb_out,
                                                                    int32_t* __restrict__ n_missing) {
  // the trip count is the same for every lane of a wave, so the ballot sees all 64
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t v = base + threadIdx.x;
    bool missing = false;
    if (v < n) {
      const float vert[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
      float rgb[3];
      missing = vertex_color(vert, nx, ny, nz, rgb_sum, n_col, rgb);
      rgb_out[3 * v] = rgb[0];
      rgb_out[3 * v + 1] = rgb[1];
      rgb_out[3 * v + 2] = rgb[2];
    }
    const unsigned long long votes = __ballot(missing);
    if (votes != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(n_missing, (int32_t)__popcll(votes));
  }
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < 1 ? 1 : (blocks < kMaxGrid ? blocks : kMaxGrid));
}

// LNRF_OK and *cells, or LNRF_ERR_SHAPE for a grid outside the conventions
static int check_grid(const char* fn, int64_t nx, int64_t ny, int64_t nz, int64_t* cells) {
  // the padded volume has (nx+2)(ny+2)(nz+2) points, which must fit the int32 ids of marching cubes as well
  const bool ok = nx >= 1 && ny >= 1 && nz >= 1 && nx <= INT32_MAX - 2 && ny <= INT32_MAX - 2 && nz <= INT32_MAX - 2 &&
                  (nx + 2) * (ny + 2) <= INT32_MAX && (nx + 2) * (ny + 2) * (nz + 2) <= INT32_MAX;
  if (!ok) {
    set_error("%s: grid (%lld, %lld, %lld): every dimension must be >= 1 and the padded volume at most INT32_MAX points",
              fn, (long long)nx, (long long)ny, (long long)nz);
    return LNRF_ERR_SHAPE;
  }
  *cells = nx * ny * nz;
  return LNRF_OK;
}

}  // namespace tsdf
}  // namespace lnrf

using namespace lnrf;

extern "C" int lnrf_tsdf_integrate(const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                                   const lnrf_tsdf_view* views, int64_t n_views, const uint16_t* depth,
                                   const uint8_t* color, float trunc, float max_depth, int32_t carve, float* sum_t,
                                   int32_t* n_obs, uint8_t* behind, int32_t* rgb_sum, int32_t* n_col,
                                   lnrf_stream_t stream) {
  int64_t n = 0;
  const int rc = tsdf::check_grid(__func__, nx, ny, nz, &n);
  if (rc != LNRF_OK) return rc;
  if (n_views < 0 || n_views > INT32_MAX) {
    set_error("%s: n_views = %lld outside [0, INT32_MAX]", __func__, (long long)n_views);
    return LNRF_ERR_SHAPE;
  }
  LNRF_CHECK_ARG(trunc > 0.0f && std::isfinite(trunc), "trunc must be positive and finite");
  LNRF_CHECK_ARG(max_depth > 0.0f && std::isfinite(max_depth), "max_depth must be positive and finite");
  LNRF_CHECK_ARG(xs && ys && zs && sum_t && n_obs && behind && rgb_sum && n_col, "null pointer");
  if (n_views == 0) return LNRF_OK;
  LNRF_CHECK_ARG(views && depth && color, "null pointer");
  constexpr int64_t t = tsdf::kTile;
  const int64_t tiles = ((nx + t - 1) / t) * ((ny + t - 1) / t) * ((nz + t - 1) / t);  // one wave each
  hipLaunchKernelGGL(tsdf::tsdf_integrate_kernel, dim3(tsdf::grid_for(tiles * kWave)), dim3(tsdf::kBlock), 0,
                     as_stream(stream), xs, ys, zs, (int)nx, (int)ny, (int)nz, views, (int)n_views, depth, color, trunc,
                     max_depth, (int)carve, sum_t, n_obs, behind, rgb_sum, n_col);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tsdf_volume(const float* sum_t, const int32_t* n_obs, const uint8_t* behind, int64_t nx, int64_t ny,
                                int64_t nz, int32_t unseen_inside, float* out, lnrf_stream_t stream) {
  int64_t n = 0;
  const int rc = tsdf::check_grid(__func__, nx, ny, nz, &n);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(sum_t && n_obs && behind && out, "null pointer");
  const int64_t total = (nx + 2) * (ny + 2) * (nz + 2);
  hipLaunchKernelGGL(tsdf::tsdf_volume_kernel, dim3(tsdf::grid_for(total)), dim3(tsdf::kBlock), 0, as_stream(stream),
                     sum_t, n_obs, behind, (int)nx, (int)ny, (int)nz, (int)unseen_inside, out);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_tsdf_vertex_colors(const float* verts, int64_t n, int64_t nx, int64_t ny, int64_t nz,
                                       const int32_t* rgb_sum, const int32_t* n_col, float* rgb_out, int32_t* n_missing,
                                       lnrf_stream_t stream) {
  int64_t cells = 0;
  const int rc = tsdf::check_grid(__func__, nx, ny, nz, &cells);
  if (rc != LNRF_OK) return rc;
  if (n < 0 || n > INT32_MAX) {
    set_error("%s: %lld vertices outside [0, INT32_MAX]", __func__, (long long)n);
    return LNRF_ERR_SHAPE;
  }
  LNRF_CHECK_ARG(rgb_sum && n_col && n_missing, "null pointer");
  hipError_t e = hipMemsetAsync(n_missing, 0, sizeof(int32_t), as_stream(stream));
  if (e != hipSuccess) return hip_fail(e, __func__);
  if (n == 0) return LNRF_OK;
  LNRF_CHECK_ARG(verts && rgb_out, "null pointer");
  hipLaunchKernelGGL(tsdf::tsdf_vertex_colors_kernel, dim3(tsdf::grid_for(n)), dim3(tsdf::kBlock), 0, as_stream(stream),
                     verts, n, (int)nx, (int)ny, (int)nz, rgb_sum, n_col, rgb_out, n_missing);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
