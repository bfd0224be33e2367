// components.hip — connected components of a 3-D mask: labels, component sizes and a keep filter, for removing the
// floaters of a trained model from the mesh export's occupancy volume and from the occupancy grid.  Additive: no
// counterpart in the reference.
//
// Conventions (learn_nerf/components.py and the NumPy restatement tests/components_reference.py rely on them):
//   mask      uint8 [nx, ny, nz], non-zero = foreground; linear index (i*ny + j)*nz + k; every dimension >= 1 and
//             nx*ny*nz <= INT32_MAX (LNRF_ERR_UNSUPPORTED above).
//   connectivity  6 (cells sharing a face) or 26 (a face, an edge or a corner).
//   labels    int32 [N]: the smallest linear index of the cell's component, -1 for a background cell.  Unique: it does
//             not depend on launch order, workgroup placement or the number of rounds.
//   sizes     int32 [N]: the number of cells of the component at its root index (labels[r] == r), 0 elsewhere.
//   keep      uint8 [N]: 1 iff the cell is foreground, its component has >= min_cells cells and the component is not
//             after the cut (cut_size, cut_label) in the order (size descending, label ascending).
//
// Passes.  `parent` (scratch, int32 [N]) is a union-find forest over linear indices in which a parent is never above
// its child, parent[r] == r at a root and -1 at a background cell; `labels` holds, per cell, some ancestor of it.
//   local     one workgroup per 8^3 tile (tile-stride beyond 65536 tiles), one lane per cell: union-find over the
//             tile's cells in LDS (the local index (li*8 + lj)*8 + lk has the order of the linear index), then
//             labels = parent = the local root.
//   merge     one lane per cell, for each of the 13 (3 at connectivity 6) neighbours with a smaller index whose label
//             differs: unite the two trees with atomicMin on the larger root.  `labels` is not written in this launch
//             and is read with plain loads; `parent` is written by other workgroups and is read and written with
//             agent-scope atomics only.  Equal labels mean a common ancestor, so skipping that pair is safe.
//   flatten   labels[c] = parent[c] = the root reached from c.
// A merge round is merge + flatten and raises *changed when a parent was lowered or a bounded walk gave up.  The host
// runs rounds until one leaves *changed at 0 (learn_nerf/components.py); the argument that such a round is the fixed
// point, and that the fixed point is the convention above, is in DESIGN.md §4.
//
// Bounds.  Every walk follows strictly decreasing indices, so it ends after at most the chain's length; it is capped
// at kWalkCap steps anyway and a unite at kUniteCap attempts (each failed attempt lowers one of its two nodes).  A
// walk or unite that gives up raises *changed, which costs another round and never a wrong label.  No lane waits for
// another workgroup.
#include <limits.h>

#include "common.h"

namespace lnrf {
namespace cc {

constexpr int kTile = 8;                            // tile edge
constexpr int kTileCells = kTile * kTile * kTile;  // 512 lanes, 2 KiB of LDS
constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int kMaxTileGrid = 1 << 16;  // workgroups of the local pass, tile-stride beyond
constexpr int kWalkCap = 4096;
constexpr int kUniteCap = 64;

// the 13 neighbours that precede a cell in linear order; the first three share a face with it
__constant__ int8_t kBack[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},   {-1, -1, 0}, {-1, 1, 0},
                                    {-1, 0, -1}, {-1, 0, 1},  {0, -1, -1},  {0, -1, 1},  {-1, -1, -1},
                                    {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

template <int kScope>
__device__ __forceinline__ int load_at(int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope);
}

// the root above x, or the node reached after kWalkCap steps (gave_up)
template <int kScope>
__device__ __forceinline__ int find_root(int* parent, int x, bool& gave_up) {
  for (int step = 0; step < kWalkCap; ++step) {
    const int p = load_at<kScope>(parent + x);
    if (p == x) return x;
    x = p;
  }
  gave_up = true;
  return x;
}

// Joins the trees of a and b.  -> true when memory changed or the attempt was abandoned (another round is needed).
template <int kScope>
__device__ __forceinline__ bool unite(int* parent, int a, int b) {
  bool moved = false, gave_up = false;
  for (int attempt = 0; attempt < kUniteCap; ++attempt) {
    a = find_root<kScope>(parent, a, gave_up);
    b = find_root<kScope>(parent, b, gave_up);
    if (gave_up) return true;
    if (a == b) return moved;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, kScope);
    moved |= old > b;
    if (old == a) return true;  // a was still a root and now hangs below b
    a = old;                    // a had been given a parent < a meanwhile: that tree and b's remain to be joined
  }
  return true;
}

__global__ __launch_bounds__(kTileCells) void cc_local_kernel(const uint8_t* __restrict__ mask, int nx, int ny, int nz,
                                                              int64_t tiles, int tiles_y, int tiles_z, int faces_only,
                                                              int* __restrict__ labels, int* __restrict__ parent) {
  __shared__ int lds[kTileCells];
  const int t = threadIdx.x, li = t >> 6, lj = (t >> 3) & 7, lk = t & 7;
  const int64_t per_i = (int64_t)tiles_y * tiles_z;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // the same trip count for the whole workgroup
    const int ti = (int)(tile / per_i), tr = (int)(tile - ti * per_i);
    const int i = ti * kTile + li, j = (tr / tiles_z) * kTile + lj, k = (tr % tiles_z) * kTile + lk;
    const bool inside = i < nx && j < ny && k < nz;
    const int64_t cell = ((int64_t)i * ny + j) * nz + k;
    const bool fg = inside && mask[cell] != 0;
    lds[t] = fg ? t : -1;
    __syncthreads();
    if (fg) {
      const int count = faces_only ? 3 : 13;
      for (int n = 0; n < count; ++n) {
        const int a = li + kBack[n][0], b = lj + kBack[n][1], c = lk + kBack[n][2];
        if (a < 0 || b < 0 || c < 0 || b >= kTile || c >= kTile) continue;  // the merge pass joins across tiles
        const int other = (a * kTile + b) * kTile + c;
        if (load_at<__HIP_MEMORY_SCOPE_WORKGROUP>(lds + other) >= 0) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lds, t, other);
      }
    }
    __syncthreads();
    if (inside) {
      int root = -1;
      if (fg) {
        bool gave_up = false;  // an unfinished tile is finished by the merge rounds, which look at every pair
        const int r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(lds, t, gave_up);
        root = (int)(((int64_t)(i - li + (r >> 6)) * ny + (j - lj + ((r >> 3) & 7))) * nz + (k - lk + (r & 7)));
      }
      labels[cell] = root;
      parent[cell] = root;
    }
    __syncthreads();  // lds is reused by the next tile
  }
}

__global__ __launch_bounds__(kBlock) void cc_merge_kernel(const int* __restrict__ labels, int nx, int ny, int nz,
                                                          int faces_only, int* parent, int* changed) {
  const int64_t n = (int64_t)nx * ny * nz, plane = (int64_t)ny * nz;
  const int count = faces_only ? 3 : 13;
  bool raise = false;
  for (int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x; cell < n; cell += (int64_t)gridDim.x * kBlock) {
    const int mine = labels[cell];
    if (mine < 0) continue;
    const int i = (int)(cell / plane), j = (int)((cell - i * plane) / nz);
    const int k = (int)(cell - i * plane - (int64_t)j * nz);
    for (int nb = 0; nb < count; ++nb) {
      const int a = i + kBack[nb][0], b = j + kBack[nb][1], c = k + kBack[nb][2];
      if (a < 0 || b < 0 || c < 0 || b >= ny || c >= nz) continue;
      const int theirs = labels[(a * plane + (int64_t)b * nz) + c];
      if (theirs < 0 || theirs == mine) continue;
      raise |= unite<__HIP_MEMORY_SCOPE_AGENT>(parent, mine, theirs);
    }
  }
  if (raise) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(int64_t n, int* parent, int* __restrict__ labels,
                                                            int* changed) {
  bool raise = false;
  for (int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x; cell < n; cell += (int64_t)gridDim.x * kBlock) {
    if (labels[cell] < 0) continue;  // this lane's own entry: no other lane writes it
    const int root = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)cell, raise);
    // other lanes walk through parent[cell] in this launch; the minimum keeps it an ancestor whatever they see
    __hip_atomic_fetch_min(parent + cell, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    labels[cell] = root;
  }
  if (raise) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one integer add per distinct label of a wave: the lanes that share the first live lane's label leave together
__global__ __launch_bounds__(kBlock) void cc_sizes_kernel(const int* __restrict__ labels, int64_t n,
                                                          int* __restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t cell = base + threadIdx.x;
    const int label = cell < n ? labels[cell] : -1;
    bool live = label >= 0 && label < n;
    for (int pass = 0; pass < 64; ++pass) {  // every pass retires at least one live lane
      const unsigned long long todo = __ballot(live);
      if (todo == 0) break;
      const int first = __ffsll((long long)todo) - 1;
      const int key = __shfl(label, first, 64);
      const unsigned long long same = __ballot(live && label == key);
      if (lane == first) atomicAdd(sizes + key, __popcll(same));
      if (label == key) live = false;
    }
  }
}

__global__ __launch_bounds__(kBlock) void cc_keep_kernel(const int* __restrict__ labels,
                                                         const int* __restrict__ sizes, int64_t n, int min_cells,
                                                         int cut_size, int cut_label, uint8_t* __restrict__ keep) {
  for (int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x; cell < n; cell += (int64_t)gridDim.x * kBlock) {
    const int label = labels[cell];
    bool on = label >= 0 && label < n;
    if (on) {
      const int size = sizes[label];
      on = size >= min_cells && (size > cut_size || (size == cut_size && label <= cut_label));
    }
    keep[cell] = on ? 1 : 0;
  }
}

static inline int grid_for(int64_t n) {
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)(blocks < 1 ? 1 : (blocks < kMaxGrid ? blocks : kMaxGrid));
}

// LNRF_OK and *cells, or the error of a volume outside the conventions
static int check_volume(const char* fn, int64_t nx, int64_t ny, int64_t nz, int64_t* cells) {
  if (nx < 1 || ny < 1 || nz < 1) {
    set_error("%s: every dimension must be at least 1, got (%lld, %lld, %lld)", fn, (long long)nx, (long long)ny,
              (long long)nz);
    return LNRF_ERR_ARG;
  }
  if (nx > INT32_MAX || ny > INT32_MAX || nz > INT32_MAX || nx * ny > INT32_MAX || nx * ny * nz > INT32_MAX) {
    set_error("%s: (%lld, %lld, %lld) has more than INT32_MAX cells", fn, (long long)nx, (long long)ny, (long long)nz);
    return LNRF_ERR_UNSUPPORTED;
  }
  *cells = nx * ny * nz;
  return LNRF_OK;
}

static int check_connectivity(const char* fn, int32_t connectivity) {
  if (connectivity == 6 || connectivity == 26) return LNRF_OK;
  set_error("%s: connectivity must be 6 or 26, got %d", fn, connectivity);
  return LNRF_ERR_ARG;
}

}  // namespace cc
}  // namespace lnrf

using namespace lnrf;

extern "C" int32_t lnrf_cc_max_rounds(void) { return LNRF_CC_MAX_ROUNDS; }

extern "C" int64_t lnrf_cc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > INT32_MAX || ny > INT32_MAX || nz > INT32_MAX || nx * ny > INT32_MAX ||
      nx * ny * nz > INT32_MAX)
    return -1;
  return nx * ny * nz * 4;  // parent
}

extern "C" int lnrf_cc_local(const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity,
                             int32_t* labels, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream) {
  int64_t n = 0;
  int rc = cc::check_volume(__func__, nx, ny, nz, &n);
  if (rc == LNRF_OK) rc = cc::check_connectivity(__func__, connectivity);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(mask && labels && scratch, "null pointer");
  LNRF_CHECK_ARG(scratch_bytes >= n * 4 && ((uintptr_t)scratch & 3) == 0, "scratch too small or unaligned");
  const int64_t tx = (nx + cc::kTile - 1) / cc::kTile, ty = (ny + cc::kTile - 1) / cc::kTile,
                tz = (nz + cc::kTile - 1) / cc::kTile;  // tx*ty*tz <= N <= INT32_MAX
  const int64_t tiles = tx * ty * tz;
  hipLaunchKernelGGL(cc::cc_local_kernel, dim3((unsigned)(tiles < cc::kMaxTileGrid ? tiles : cc::kMaxTileGrid)),
                     dim3(cc::kTileCells), 0, as_stream(stream), mask, (int)nx, (int)ny, (int)nz, tiles, (int)ty,
                     (int)tz, connectivity == 6 ? 1 : 0, labels, (int*)scratch);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_cc_merge_round(int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int32_t round,
                                   int32_t* labels, int32_t* changed, void* scratch, int64_t scratch_bytes,
                                   lnrf_stream_t stream) {
  int64_t n = 0;
  int rc = cc::check_volume(__func__, nx, ny, nz, &n);
  if (rc == LNRF_OK) rc = cc::check_connectivity(__func__, connectivity);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(round >= 0, "round must be >= 0");
  if (round >= LNRF_CC_MAX_ROUNDS) {
    set_error("%s: no fixed point after %d rounds; the labels are not converged and must not be used", __func__,
              LNRF_CC_MAX_ROUNDS);
    return LNRF_ERR_UNSUPPORTED;
  }
  LNRF_CHECK_ARG(labels && changed && scratch, "null pointer");
  LNRF_CHECK_ARG(scratch_bytes >= n * 4 && ((uintptr_t)scratch & 3) == 0, "scratch too small or unaligned");
  hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), as_stream(stream));
  if (e != hipSuccess) return hip_fail(e, __func__);
  hipLaunchKernelGGL(cc::cc_merge_kernel, dim3(cc::grid_for(n)), dim3(cc::kBlock), 0, as_stream(stream), labels,
                     (int)nx, (int)ny, (int)nz, connectivity == 6 ? 1 : 0, (int*)scratch, changed);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc::cc_flatten_kernel, dim3(cc::grid_for(n)), dim3(cc::kBlock), 0, as_stream(stream), n,
                     (int*)scratch, labels, changed);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_cc_sizes(const int32_t* labels, int64_t n, int32_t* sizes, lnrf_stream_t stream) {
  LNRF_CHECK_ARG(n >= 1, "n must be >= 1");
  if (n > INT32_MAX) {
    set_error("%s: %lld cells do not fit in int32 labels", __func__, (long long)n);
    return LNRF_ERR_UNSUPPORTED;
  }
  LNRF_CHECK_ARG(labels && sizes, "null pointer");
  hipError_t e = hipMemsetAsync(sizes, 0, n * sizeof(int32_t), as_stream(stream));
  if (e != hipSuccess) return hip_fail(e, __func__);
  hipLaunchKernelGGL(cc::cc_sizes_kernel, dim3(cc::grid_for(n)), dim3(cc::kBlock), 0, as_stream(stream), labels, n,
                     sizes);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_cc_keep(const int32_t* labels, const int32_t* sizes, int64_t n, int32_t min_cells,
                            int32_t cut_size, int32_t cut_label, uint8_t* keep, lnrf_stream_t stream) {
  LNRF_CHECK_ARG(n >= 1, "n must be >= 1");
  if (n > INT32_MAX) {
    set_error("%s: %lld cells do not fit in int32 labels", __func__, (long long)n);
    return LNRF_ERR_UNSUPPORTED;
  }
  LNRF_CHECK_ARG(min_cells >= 1, "min_cells must be >= 1");
  LNRF_CHECK_ARG(cut_size >= 0, "cut_size must be >= 0 (0 = no cut)");
  LNRF_CHECK_ARG(labels && sizes && keep, "null pointer");
  hipLaunchKernelGGL(cc::cc_keep_kernel, dim3(cc::grid_for(n)), dim3(cc::kBlock), 0, as_stream(stream), labels, sizes,
                     n, (int)min_cells, (int)cut_size, (int)cut_label, keep);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}
