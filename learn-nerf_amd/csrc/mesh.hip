// mesh.hip — marching cubes over a density volume: the surface extraction of scripts/marching_cubes.py:62-66 (the
// reference calls skimage.measure.marching_cubes at occupancy 0.9).  Two device passes, a deterministic output order
// and no atomics.
//
// Conventions (learn_nerf/mesh.py and the NumPy restatement tests/mesh_reference.py rely on every one of them):
//   volume    fp32 [nx, ny, nz] in C order, nx, ny, nz >= 2; point (i,j,k) has linear index p = (i*ny + j)*nz + k
//             (int64).
//   inside    v > level, strictly; NaN is outside.  Inside means dense: the field is occupancy.
//   cell      (i,j,k) with i < nx-1, j < ny-1, k < nz-1 has corners (i+dx, j+dy, k+dz), corner number
//             c = dx + 2dy + 4dz; its case index is sum inside(c) << c.
//   edges     axis-major: for axis a = 0,1,2 and each corner c (ascending) with bit a clear, edge (c, c | 1<<a); so
//             edges 0-3 run along x, 4-7 along y and 8-11 along z.
//   vertices  one per crossing grid edge (inside differs at its two ends).  Point p owns its edges along +x, +y, +z;
//             vertices are ordered by (p, axis).  Coordinates are in index space: along the crossing axis a the
//             coordinate is float(p_a) + (level - v(p)) / (v(p + e_a) - v(p)), in fp32 and in exactly that order,
//             always from the lower-index end (no -ffast-math, and hipcc's default correctly rounded fp32 divide make
//             it IEEE, so NumPy float32 gives the same bits); the other two coordinates are the integers of p.
//   faces     ordered by linear cell index (= p of corner 0), then by table order; 0-based int32 vertex ids.  Every
//             face is outward: by the right-hand rule its normal points from inside to outside, so the signed volume
//             sum v0.(v1 x v2)/6 of a closed mesh is positive.
//
// Case table: generated at compile time from one rule (make_case_table).  On each of the 6 cube faces, walked
// counter-clockwise as seen from outside, the segment of every run of inside corners goes from the edge where the walk
// enters the run to the next crossing edge (where it leaves).  The decision depends on the face's four corners alone,
// so two cells that share a face put the same segments on it with opposite directions, and a volume padded with
// outside values always gives a closed, consistently oriented mesh.  Every crossing edge lies on two faces: it has one
// outgoing and one incoming segment, and the segments chain into closed loops, each started at its lowest edge, in
// the order of that edge, and fan-triangulated (l0, lk, lk+1).
//
// Passes (scratch layout: mc_layout):
//   count  mc_count_kernel: per point a 16-bit word, bit 0 inside, bits 1-3 crossing along x/y/z, bits 4-15 the
//          exclusive prefix of the vertex counts inside its tile of kTile points (< 3*kTile <= 4095); per tile the
//          vertex and triangle totals.  mc_scan_kernel (one workgroup): 64-bit exclusive offsets of the tiles and
//          the two totals, counts[0] = V, counts[1] = F (int64: the host decides whether they fit in int32 ids).
//   emit   mc_emit_kernel, given V and F read back: vertices at tile offset + prefix, faces at tile offset + block
//          scan of the triangle counts.  The topology (which vertices and triangles exist, and their ids) comes from
//          the scratch alone and the volume is read only for the interpolation; no write goes at or beyond V or F.
// Within a tile thread t handles points p0 + t + r*kBlock (r < kPer), so every load sweep is coalesced; the in-tile
// order stays linear because slice r's prefix is field r of one packed 64-bit workgroup scan.
#include "common.h"

namespace lnrf {
namespace mc {

// corners of each cube face, counter-clockwise as seen from outside the cube
constexpr int kFaceWalk[6][4] = {
    {0, 2, 3, 1},  // z = 0
    {0, 1, 5, 4},  // y = 0
    {0, 4, 6, 2},  // x = 0
    {4, 5, 7, 6},  // z = 1
    {2, 6, 7, 3},  // y = 1
    {1, 3, 7, 5},  // x = 1
};

constexpr int kMaxTri = 5;

// number of the cube edge between corners c0 and c1 (they differ in one bit a)
constexpr int edge_of(int c0, int c1) {
  const int lo = c0 < c1 ? c0 : c1, bit = c0 ^ c1;
  const int a = bit == 1 ? 0 : bit == 2 ? 1 : 2;
  return 4 * a + (((lo >> (a + 1)) << a) | (lo & ((1 << a) - 1)));
}

struct CaseTable {
  int8_t edges[256][16];  // triangles as edge triples, -1 terminated
  uint8_t ntri[256];
  int max_tri;
  bool closed;  // every edge had at most one outgoing segment and every chain came back to its first edge
};

constexpr CaseTable make_case_table() {
  CaseTable t{};
  t.max_tri = 0;
  t.closed = true;
  for (int cs = 0; cs < 256; ++cs) {
    int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (const auto& w : kFaceWalk) {
      bool cross[4] = {}, enter[4] = {};
      int edge[4] = {};
      for (int s = 0; s < 4; ++s) {
        const bool in0 = (cs >> w[s]) & 1, in1 = (cs >> w[(s + 1) & 3]) & 1;
        cross[s] = in0 != in1;
        enter[s] = !in0 && in1;
        edge[s] = edge_of(w[s], w[(s + 1) & 3]);
      }
      for (int s = 0; s < 4; ++s) {
        if (!enter[s]) continue;
        for (int d = 1; d < 4; ++d) {
          if (cross[(s + d) & 3]) {
            if (next[edge[s]] != -1) t.closed = false;
            next[edge[s]] = edge[(s + d) & 3];
            break;
          }
        }
      }
    }
    bool seen[12] = {};
    int n = 0, ntri = 0;
    for (int e0 = 0; e0 < 12; ++e0) {
      if (next[e0] < 0 || seen[e0]) continue;
      int loop[12] = {};
      int len = 0, e = e0;
      while (!seen[e] && next[e] >= 0) {
        seen[e] = true;
        loop[len++] = e;
        e = next[e];
      }
      if (e != e0) t.closed = false;
      for (int k = 1; k + 1 < len && n + 3 <= 15; ++k) {  // 15: keeps the -1 terminator (max_tri reports overflow)
        t.edges[cs][n++] = (int8_t)loop[0];
        t.edges[cs][n++] = (int8_t)loop[k];
        t.edges[cs][n++] = (int8_t)loop[k + 1];
      }
      ntri += len - 2;
    }
    for (; n < 16; ++n) t.edges[cs][n] = -1;
    t.ntri[cs] = (uint8_t)ntri;
    if (ntri > t.max_tri) t.max_tri = ntri;
  }
  return t;
}

constexpr CaseTable kHostTable = make_case_table();
static_assert(kHostTable.closed, "marching-cubes segments must chain into closed loops");
static_assert(kHostTable.max_tri <= kMaxTri, "marching-cubes case with more than 5 triangles");
static_assert(kHostTable.ntri[0] == 0 && kHostTable.ntri[255] == 0, "empty and full cells have no surface");

__constant__ CaseTable g_table = make_case_table();

constexpr int kBlock = 256;            // threads per workgroup (4 waves)
constexpr int kPer = 4;                // points per thread and tile: p0 + t + r*kBlock, r < kPer (coalesced)
constexpr int kTileLog2 = 10;
constexpr int kTile = 1 << kTileLog2;  // points per tile
constexpr int kScanBlock = 1024;       // the one workgroup of the tile scan
constexpr int kScanPer = 8;            // consecutive tiles per scan thread and round
constexpr int kMaxGrid = 2048;         // 256 CUs x 8 workgroups, grid-stride beyond
static_assert(kTile == kBlock * kPer, "tile size");
static_assert(3 * kTile <= 4096, "the tile-local vertex prefix must fit in 12 bits");
static_assert(kMaxTri * kBlock < 4096 && 3 * kBlock < 4096, "slice totals are scanned as 12-bit fields");
static_assert(kMaxTri * kTile < 65536, "tile triangle totals are scanned as a 16-bit field");
static_assert((int64_t)kScanBlock * kScanPer * kMaxTri * kTile < (1ll << 32), "round sums are 32-bit fields");

struct Dims {
  int64_t nx, ny, nz, syz, n;  // syz = ny*nz, n = nx*ny*nz
  int64_t di, dj, dk;          // (i, j, k) step of kBlock points in linear order
};

struct alignas(16) TileOff {
  long long v, f;  // exclusive offsets of the tile's first vertex and first face
};

struct Layout {
  int64_t packed, tile_counts, tile_offs, bytes, ntiles;
};

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

static inline Layout mc_layout(int64_t nx, int64_t ny, int64_t nz) {
  Layout l;
  const int64_t n = nx * ny * nz;
  l.ntiles = (n + kTile - 1) / kTile;
  l.packed = 0;                                          // uint16 [n]
  l.tile_counts = align256(2 * n);                       // int2 [ntiles]: (vertices, triangles) of the tile
  l.tile_offs = l.tile_counts + align256(8 * l.ntiles);  // TileOff [ntiles]
  l.bytes = l.tile_offs + 16 * l.ntiles;
  return l;
}

static inline Dims mc_dims(int64_t nx, int64_t ny, int64_t nz) {
  return Dims{nx, ny, nz, ny * nz, nx * ny * nz, kBlock / (ny * nz), (kBlock / nz) % ny, kBlock % nz};
}

// inside flags of the 8 corners of the cell at p (a corner beyond the volume counts as outside)
__device__ __forceinline__ int corner_mask(const float* __restrict__ vol, const Dims& d, int64_t p, bool ci, bool cj,
                                           bool ck, float level) {
  int m = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    if ((dx && !ci) || (dy && !cj) || (dz && !ck)) continue;
    const float v = vol[p + dx * d.syz + dy * d.nz + dz];
    m |= (v > level ? 1 : 0) << c;
  }
  return m;
}

// exclusive prefix of v over the workgroup in thread order, and the workgroup total.  Packed fields scan
// independently as long as no field's total overflows.
template <int kThreads, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T& total, T* lds) {
  constexpr int kWaves = kThreads / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const T s = lds[i];
    base += i < w ? s : T(0);
    total += s;
  }
  __syncthreads();  // lds is reused by the next tile
  return base + inc - v;
}

__device__ __forceinline__ void point_of(const Dims& d, int64_t p, int64_t& i, int64_t& j, int64_t& k) {
  i = p / d.syz;
  const int64_t r = p - i * d.syz;
  j = r / d.nz;
  k = r - j * d.nz;
}

// (i, j, k) of p + kBlock from those of p (dk < nz and dj < ny: one carry each at most)
__device__ __forceinline__ void step_point(const Dims& d, int64_t& i, int64_t& j, int64_t& k) {
  k += d.dk;
  if (k >= d.nz) {
    k -= d.nz;
    ++j;
  }
  j += d.dj;
  if (j >= d.ny) {
    j -= d.ny;
    ++i;
  }
  i += d.di;
}

__device__ __forceinline__ int field12(unsigned long long x, int r) { return (int)((x >> (12 * r)) & 0xFFF); }

// Thread t of a tile handles points p0 + t + r*kBlock: slice r of the tile is one coalesced sweep.  One 64-bit scan
// gives every slice's prefix (12-bit field r) and the tile's triangle total (bits 48-63).
__global__ __launch_bounds__(kBlock) void mc_count_kernel(const float* __restrict__ vol, Dims d, float level,
                                                          uint16_t* __restrict__ packed,
                                                          int2* __restrict__ tile_counts, int64_t ntiles) {
  __shared__ unsigned long long lds[kBlock / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t p0 = (tile << kTileLog2) + threadIdx.x;
    int64_t i, j, k;
    point_of(d, p0, i, j, k);
    int code[kPer];
    unsigned long long cnt = 0;
    int ntri = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      code[r] = 0;
      const int64_t p = p0 + r * kBlock;
      if (p < d.n) {
        const bool ci = i + 1 < d.nx, cj = j + 1 < d.ny, ck = k + 1 < d.nz;
        const int m = corner_mask(vol, d, p, ci, cj, ck, level);
        const int in0 = m & 1;
        const int cx = ci && ((m >> 1) & 1) != in0;
        const int cy = cj && ((m >> 2) & 1) != in0;
        const int cz = ck && ((m >> 4) & 1) != in0;
        code[r] = in0 | cx << 1 | cy << 2 | cz << 3;
        cnt |= (unsigned long long)(cx + cy + cz) << (12 * r);
        ntri += (ci && cj && ck) ? (int)g_table.ntri[m] : 0;
      }
      step_point(d, i, j, k);
    }
    cnt |= (unsigned long long)ntri << 48;
    unsigned long long total;
    const unsigned long long excl = block_excl_scan<kBlock>(cnt, total, lds);
    int before = 0;  // vertices of the slices in front of slice r
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int64_t p = p0 + r * kBlock;
      if (p < d.n) packed[p] = (uint16_t)(code[r] | (before + field12(excl, r)) << 4);
      before += field12(total, r);
    }
    if (threadIdx.x == 0) tile_counts[tile] = make_int2(before, (int)(total >> 48));
  }
}

// One workgroup, rounds of kScanBlock*kScanPer tiles: thread t reads kScanPer consecutive tiles (the round is one
// coalesced sweep), one scan of (vertices | faces << 32) per round, 64-bit carries across rounds.
__global__ __launch_bounds__(kScanBlock) void mc_scan_kernel(const int2* __restrict__ tile_counts, int64_t ntiles,
                                                             TileOff* __restrict__ tile_offs,
                                                             int64_t* __restrict__ counts) {
  __shared__ unsigned long long lds[kScanBlock / 64];
  long long carry_v = 0, carry_f = 0;
  for (int64_t base = 0; base < ntiles; base += (int64_t)kScanBlock * kScanPer) {
    const int64_t t0 = base + (int64_t)threadIdx.x * kScanPer;
    int2 c[kScanPer];
    if (t0 + kScanPer <= ntiles) {
      const int4* src = reinterpret_cast<const int4*>(tile_counts + t0);
#pragma unroll
      for (int q = 0; q < kScanPer / 2; ++q) {
        const int4 two = src[q];
        c[2 * q] = make_int2(two.x, two.y);
        c[2 * q + 1] = make_int2(two.z, two.w);
      }
    } else {
#pragma unroll
      for (int q = 0; q < kScanPer; ++q) c[q] = t0 + q < ntiles ? tile_counts[t0 + q] : make_int2(0, 0);
    }
    unsigned long long s = 0;
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) s += (unsigned long long)c[q].x | (unsigned long long)c[q].y << 32;
    unsigned long long total;
    const unsigned long long excl = block_excl_scan<kScanBlock>(s, total, lds);
    long long ov = carry_v + (long long)(excl & 0xFFFFFFFFull), of = carry_f + (long long)(excl >> 32);
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
      if (t0 + q < ntiles) tile_offs[t0 + q] = TileOff{ov, of};
      ov += c[q].x;
      of += c[q].y;
    }
    carry_v += (long long)(total & 0xFFFFFFFFull);
    carry_f += (long long)(total >> 32);
  }
  if (threadIdx.x == 0) {
    counts[0] = carry_v;
    counts[1] = carry_f;
  }
}

// id of the vertex on edge e of the cell whose corner 0 is point p
__device__ __forceinline__ long long edge_vertex(const uint16_t* __restrict__ packed,
                                                 const TileOff* __restrict__ tile_offs, const Dims& d, int64_t p,
                                                 int e) {
  const int a = e >> 2, r = e & 3;
  const int lo = ((r >> a) << (a + 1)) | (r & ((1 << a) - 1));  // the edge's corner with bit a clear
  const int64_t q = p + (lo & 1) * d.syz + ((lo >> 1) & 1) * d.nz + (lo >> 2);
  const uint32_t w = packed[q];
  return tile_offs[q >> kTileLog2].v + (long long)(w >> 4) + __popc((w >> 1) & ((1u << a) - 1));
}

// n_verts / n_faces: the counts of the count pass; no write goes at or beyond them whatever the scratch holds
__global__ __launch_bounds__(kBlock) void mc_emit_kernel(const float* __restrict__ vol, Dims d, float level,
                                                         const uint16_t* __restrict__ packed,
                                                         const TileOff* __restrict__ tile_offs, int64_t ntiles,
                                                         int64_t n_verts, int64_t n_faces, float* __restrict__ verts,
                                                         int32_t* __restrict__ faces) {
  __shared__ unsigned long long lds[kBlock / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const TileOff off = tile_offs[tile];
    const int64_t p0 = (tile << kTileLog2) + threadIdx.x;
    int64_t i, j, k;
    point_of(d, p0, i, j, k);
    int cases[kPer];
    unsigned long long cnt = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      cases[r] = 0;
      const int64_t p = p0 + r * kBlock;
      if (p < d.n) {
        const uint32_t w = packed[p];
        if (w & 0xEu) {
          long long vid = off.v + (long long)(w >> 4);
          const float v0 = vol[p];
          const float at[3] = {(float)i, (float)j, (float)k};
          const int64_t step[3] = {d.syz, d.nz, 1};
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            if (!(w & (2u << a))) continue;
            const float v1 = vol[p + step[a]];
            if (vid < n_verts) {
              float* out = verts + 3 * vid;
              out[0] = at[0];
              out[1] = at[1];
              out[2] = at[2];
              out[a] = at[a] + (level - v0) / (v1 - v0);
            }
            ++vid;
          }
        }
        if (i + 1 < d.nx && j + 1 < d.ny && k + 1 < d.nz) {
          int m = 0;
#pragma unroll
          for (int c = 0; c < 8; ++c)
            m |= (int)(packed[p + (c & 1) * d.syz + ((c >> 1) & 1) * d.nz + (c >> 2)] & 1u) << c;
          cases[r] = m;
          cnt |= (unsigned long long)g_table.ntri[m] << (12 * r);
        }
      }
      step_point(d, i, j, k);
    }
    unsigned long long total;
    const unsigned long long excl = block_excl_scan<kBlock>(cnt, total, lds);
    long long before = off.f;  // first face of slice r
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int m = cases[r];
      const int nt = g_table.ntri[m];  // case 0 for points without a cell
      long long fid = before + field12(excl, r);
      for (int t = 0; t < nt; ++t, ++fid) {
        if (fid >= n_faces) break;
#pragma unroll
        for (int q = 0; q < 3; ++q)
          faces[3 * fid + q] =
              (int32_t)edge_vertex(packed, tile_offs, d, p0 + r * kBlock, g_table.edges[m][3 * t + q]);
      }
      before += field12(total, r);
    }
  }
}

static int check_volume(const char* fn, int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 2 || ny < 2 || nz < 2) {
    set_error("%s: volume [%lld, %lld, %lld] needs every dimension >= 2", fn, (long long)nx, (long long)ny,
              (long long)nz);
    return LNRF_ERR_ARG;
  }
  return LNRF_OK;
}

static inline int grid_for(int64_t ntiles) { return (int)(ntiles < kMaxGrid ? ntiles : kMaxGrid); }

}  // namespace mc
}  // namespace lnrf

using namespace lnrf;

extern "C" int64_t lnrf_mc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 2 || ny < 2 || nz < 2) return -1;
  return mc::mc_layout(nx, ny, nz).bytes;
}

extern "C" int lnrf_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, void* scratch,
                             int64_t* counts, lnrf_stream_t stream) {
  const int rc = mc::check_volume(__func__, nx, ny, nz);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(vol && scratch && counts, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "scratch must be 16-byte aligned");
  const mc::Layout l = mc::mc_layout(nx, ny, nz);
  const mc::Dims d = mc::mc_dims(nx, ny, nz);
  char* s = (char*)scratch;
  hipLaunchKernelGGL(mc::mc_count_kernel, dim3(mc::grid_for(l.ntiles)), dim3(mc::kBlock), 0, as_stream(stream), vol,
                     d, level, (uint16_t*)(s + l.packed), (int2*)(s + l.tile_counts), l.ntiles);
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(mc::mc_scan_kernel, dim3(1), dim3(mc::kScanBlock), 0, as_stream(stream),
                     (const int2*)(s + l.tile_counts), l.ntiles, (mc::TileOff*)(s + l.tile_offs), counts);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, const void* scratch,
                            int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, lnrf_stream_t stream) {
  const int rc = mc::check_volume(__func__, nx, ny, nz);
  if (rc != LNRF_OK) return rc;
  LNRF_CHECK_ARG(vol && scratch, "null pointer");
  LNRF_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "scratch must be 16-byte aligned");
  LNRF_CHECK_ARG(n_verts >= 0 && n_faces >= 0, "negative count");
  LNRF_CHECK_ARG((verts || n_verts == 0) && (faces || n_faces == 0), "null output");
  if (n_verts > INT32_MAX || n_faces > INT32_MAX) {
    set_error("%s: %lld vertices / %lld faces do not fit in int32 ids", __func__, (long long)n_verts,
              (long long)n_faces);
    return LNRF_ERR_SHAPE;
  }
  if (n_verts == 0) return LNRF_OK;  // no crossing edge: no vertex, no face
  const mc::Layout l = mc::mc_layout(nx, ny, nz);
  const mc::Dims d = mc::mc_dims(nx, ny, nz);
  const char* s = (const char*)scratch;
  hipLaunchKernelGGL(mc::mc_emit_kernel, dim3(mc::grid_for(l.ntiles)), dim3(mc::kBlock), 0, as_stream(stream), vol,
                     d, level, (const uint16_t*)(s + l.packed), (const mc::TileOff*)(s + l.tile_offs), l.ntiles,
                     n_verts, n_faces, verts, faces);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_mc_case_table(int8_t* out) {
  LNRF_CHECK_ARG(out != nullptr, "null pointer");
  for (int c = 0; c < 256; ++c)
    for (int e = 0; e < 16; ++e) out[16 * c + e] = mc::kHostTable.edges[c][e];
  return LNRF_OK;
}
