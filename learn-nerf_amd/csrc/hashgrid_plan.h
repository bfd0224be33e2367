// hashgrid_plan.h — the host arithmetic of the hash-grid encoding (hashgrid.hip) and the cell geometry its kernels share:
// the descriptor mirror, where a point sits in a level's grid and what its 8 corners weigh, the two launch plans (work cut
// into eight XCD shares; buckets, splits, capacities and reduce workgroups), the decodes the kernels read them with, and
// the layout of the bucketed scatter's scratch block.  No HIP types: hashgrid.hip launches from these plans, and
// layout_host.cpp exports the same functions to the CPU tests (tests/test_hashgrid_plan.py), so there is one copy of each.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lnrf.h"

#if defined(__HIPCC__)
#define HG_HD __host__ __device__ __forceinline__
#else
#define HG_HD inline
#endif

namespace lnrf {

constexpr int kMaxLevels = 32;
constexpr int kXcds = 8;
constexpr int kStageEntries = 8192;   // forward: a staged table is 64 KiB of float2 in LDS
constexpr int kSliceEntries = 8192;   // fallback scatter: 64 KiB of float2
constexpr int kBucketEntries = 4096;  // bucketed scatter: 64 KiB of int64 x 2 features
constexpr int kMaxSlices = 256;       // bucketed levels: table <= 1M entries
constexpr int kBinChunk = 2048;       // samples per binning workgroup
constexpr int kTupleBytes = 12;       // scratch is sized for {rel, float, float} tuples (the 8-byte form uses less of it)

struct HashGridDesc {  // mirrors lnrf_hashgrid_desc
  int n_levels, feature_dim, smooth, pad_;
  float bbox_min[3], bbox_max[3];
  int grid_size[kMaxLevels];
  int table_size[kMaxLevels];         // entries (rows) of the level's table
  long long table_offset[kMaxLevels]; // first float of the level's table in the flat buffer
  int hashed[kMaxLevels];             // 1: XOR-prime hash, 0: dense x + G (y + G z)
};
static_assert(sizeof(HashGridDesc) == sizeof(lnrf_hashgrid_desc), "descriptor layout");

// ---- cell geometry ----------------------------------------------------------------------------------------------
struct Corner {
  unsigned base[3];  // floored cell
  float c[3];        // interpolation fraction (after smoothstep if smooth)
  float dc[3];       // d c[a] / d x[a] (0 outside the bounding box: the clip has zero slope there)
};

HG_HD Corner locate(const float x[3], const HashGridDesc& d, int G) {
  Corner r;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float frac = (x[a] - d.bbox_min[a]) / (d.bbox_max[a] - d.bbox_min[a]);   // instant_ngp.py:138-140
    frac = fminf(fmaxf(frac, 0.0f), 1.0f);
    const float fi = d.smooth ? 0.5f + (float)(G - 2) * frac : (float)(G - 1) * frac;  // :141-146
    float fl = floorf(fi);
    fl = fminf(fl, (float)(G - 2));                                           // :150
    float c = fi - fl;                                                        // :152
    const float extent = d.bbox_max[a] - d.bbox_min[a];
    const bool inside = x[a] > d.bbox_min[a] && x[a] < d.bbox_max[a];
    float slope = (d.smooth ? (float)(G - 2) : (float)(G - 1)) / extent;
    if (d.smooth) {
      slope *= 6.0f * c * (1.0f - c);                                         // d/dt of t^2 (3 - 2t)
      c = (c * c) * (3.0f - 2.0f * c);                                        // :153-154
    }
    r.base[a] = (unsigned)fl;                                                 // :156
    r.c[a] = c;
    r.dc[a] = inside ? slope : 0.0f;
  }
  return r;
}

// trilinear weight of corner (xo, yo, zo), instant_ngp.py:160-175: prod(o ? c : 1 - c); and its gradient d w / d x
HG_HD float corner_weight(const Corner& k, int xo, int yo, int zo) {
  return (xo ? k.c[0] : 1.0f - k.c[0]) * (yo ? k.c[1] : 1.0f - k.c[1]) * (zo ? k.c[2] : 1.0f - k.c[2]);
}
HG_HD void corner_weight_grad(const Corner& k, int xo, int yo, int zo, float g[3]) {
  const float wx = xo ? k.c[0] : 1.0f - k.c[0], wy = yo ? k.c[1] : 1.0f - k.c[1], wz = zo ? k.c[2] : 1.0f - k.c[2];
  g[0] = (xo ? k.dc[0] : -k.dc[0]) * wy * wz;
  g[1] = (yo ? k.dc[1] : -k.dc[1]) * wx * wz;
  g[2] = (zo ? k.dc[2] : -k.dc[2]) * wx * wy;
}

HG_HD unsigned entry_index(unsigned cx, unsigned cy, unsigned cz, int G, int T, int hashed) {
  if (hashed) {                                                                  // instant_ngp.py:219-223
    const unsigned hv = cx ^ (19349663u * cy) ^ (83492791u * cz);
    // power-of-two tables (the usual case): a mask instead of the ~35-instruction runtime modulo (uniform branch)
    return (T & (T - 1)) == 0 ? (hv & (unsigned)(T - 1)) : hv % (unsigned)T;
  }
  return cx + (unsigned)G * (cy + (unsigned)G * cz);                            // :199-201
}

struct LevelList { int n; int level[kMaxLevels]; };

// ---- forward: (level, sample chunk) -> workgroup, chosen per XCD --------------------------------------------------
// Workgroups are dealt to the eight XCDs round-robin (workgroup i runs on XCD i % 8) and every XCD has its own 4 MiB L2,
// so with a plain (chunk, level) grid every level's table is pulled from HBM into all eight L2s.  Here the work of all
// levels is laid out on a line (level after level, chunk after chunk, each chunk weighted by its level's cost) and cut
// into eight equal pieces: an XCD sweeps its piece in order, so a table is fetched by one XCD — two when a cut runs
// through the level — and the pieces end together.  Only speed depends on the dispatch order, not the result.
constexpr int kMaxXcdSegs = kMaxLevels + kXcds;
struct XcdPlan {
  int n_segs;
  int first_seg[kXcds + 1];     // segments of XCD x: first_seg[x] .. first_seg[x + 1] - 1
  int seg_level[kMaxXcdSegs];
  int seg_chunk0[kMaxXcdSegs];  // first 256-sample chunk of the segment
  int seg_chunks[kMaxXcdSegs];
};

// Relative cost of one sample of a level in the gather, measured alone at 786,432 samples (tools/
// hashgrid_level_probe.py): dense levels 12 us, hashed levels 17 us at 4 cells per entry, 27 us at 32, 31 us beyond
// (more and more of the 8 corners fall into different cache lines).
inline double gather_cost(const HashGridDesc& d, int l) {
  if (!d.hashed[l]) return 12.0;
  const double cells = (double)d.grid_size[l] * d.grid_size[l] * d.grid_size[l] / (double)d.table_size[l];
  return cells <= 4.0 ? 17.0 : (cells <= 32.0 ? 27.0 : 31.0);
}

// *grid = workgroups to launch, 0 if the plan does not cover every chunk of every level exactly once, in order
inline XcdPlan make_xcd_plan(const HashGridDesc& d, const LevelList& levels, int64_t m, unsigned* grid) {
  XcdPlan p;
  const int chunks = (int)((m + 255) / 256);
  double total = 0.0;
  for (int i = 0; i < levels.n; ++i) total += gather_cost(d, levels.level[i]) * chunks;
  const double share = total / kXcds;
  p.n_segs = 0;
  int xcd = 0, li = 0, next_chunk = 0, max_slots = 0, slots = 0;
  double filled = 0.0;
  p.first_seg[0] = 0;
  while (li < levels.n) {
    const double c = gather_cost(d, levels.level[li]);
    // chunks of this level that still fit into the XCD's share (the last XCD takes whatever is left)
    int take = chunks - next_chunk;
    if (xcd < kXcds - 1) {
      const int fit = (int)((share - filled) / c + 0.5);
      if (fit < take) take = fit;
    }
    if (take > 0) {
      p.seg_level[p.n_segs] = levels.level[li];
      p.seg_chunk0[p.n_segs] = next_chunk;
      p.seg_chunks[p.n_segs] = take;
      ++p.n_segs;
      next_chunk += take;
      filled += take * c;
      slots += take;
    }
    if (next_chunk >= chunks) {
      ++li;
      next_chunk = 0;
    } else {  // the XCD is full: the rest of the level goes to the next one
      if (slots > max_slots) max_slots = slots;
      ++xcd;
      p.first_seg[xcd] = p.n_segs;
      filled = 0.0;
      slots = 0;
    }
  }
  if (slots > max_slots) max_slots = slots;
  for (int x2 = xcd + 1; x2 <= kXcds; ++x2) p.first_seg[x2] = p.n_segs;
  *grid = (unsigned)max_slots * kXcds;
  bool ok = p.n_segs <= kMaxXcdSegs;
  for (int i = 0, s = 0; ok && i < levels.n; ++i) {
    int at = 0;
    while (s < p.n_segs && p.seg_level[s] == levels.level[i] && p.seg_chunk0[s] == at) at += p.seg_chunks[s++];
    ok = at == chunks;
  }
  if (!ok) *grid = 0;
  return p;
}

// Workgroup `block` of hashgrid_fwd_xcd_kernel: its segment and its 256-sample chunk within it (seg < 0: nothing), and
// from them the level and the first sample.  The two reads stay apart from the walk, so that the kernel can have its
// points on the way before it needs the level.
struct XcdWork { int seg, slot; };
HG_HD XcdWork xcd_work(const XcdPlan& plan, unsigned block) {
  const int xcd = block % kXcds;
  int slot = block / kXcds;
  int seg = plan.first_seg[xcd];
  const int seg_end = plan.first_seg[xcd + 1];
  while (seg < seg_end && slot >= plan.seg_chunks[seg]) slot -= plan.seg_chunks[seg++];
  if (seg >= seg_end) return {-1, 0};
  return {seg, slot};
}
HG_HD int xcd_level(const XcdPlan& plan, const XcdWork& w) { return plan.seg_level[w.seg]; }
HG_HD int64_t xcd_first_sample(const XcdPlan& plan, const XcdWork& w) {
  return ((int64_t)plan.seg_chunk0[w.seg] + w.slot) * 256;
}

// ---- bucketed scatter: buckets, capacities, reduce workgroups and the scratch block -------------------------------
struct BucketPlan {
  int n;                 // bucketed levels
  int level[kMaxLevels];
  int slices[kMaxLevels];
  int split[kMaxLevels];             // reduce workgroups per bucket
  int wg_off[kMaxLevels + 1];        // first reduce workgroup of the level
  long long tuple_off[kMaxLevels];   // first tuple of the level's buckets
  long long cursor_off[kMaxLevels];  // first cursor of the level
  long long cap[kMaxLevels];         // tuples per bucket of the level
};

// Every level whose table has at most kMaxSlices 4K-entry slices is bucketed (hashed or dense).
inline int bucket_slices(const HashGridDesc& d, int l) { return (d.table_size[l] + kBucketEntries - 1) / kBucketEntries; }
inline bool level_is_bucketed(const HashGridDesc& d, int l) { return bucket_slices(d, l) <= kMaxSlices; }
inline BucketPlan make_plan(const HashGridDesc& d, int64_t m) {
  BucketPlan p;
  p.n = 0;
  int64_t toff = 0, coff = 0;
  int wg = 0;
  for (int l = 0; l < d.n_levels; ++l) {
    if (!level_is_bucketed(d, l)) continue;
    const int slices = bucket_slices(d, l);
    // capacity: the hash spreads samples evenly (1.25x the mean); dense levels follow the scene geometry
    // (4x the mean).  Overflowing tuples fall back to atomics in the bin kernel.
    const double mean = (double)m * 8.0 / (double)slices;
    long long cap = (long long)(mean * (d.hashed[l] ? 1.25 : 4.0)) + 4096;
    if (cap > m * 8) cap = m * 8;
    // One workgroup streams about 1 tuple/ns, so buckets of more than ~64K tuples (few-slice levels) are
    // split; a split bucket is flushed with (contiguous) atomics, an unsplit one with plain stores.
    int split = mean <= 81920.0 ? 1 : (int)((mean + 65535.0) / 65536.0);
    if (split > 64) split = 64;
    p.level[p.n] = l;
    p.slices[p.n] = slices;
    p.split[p.n] = split;
    p.wg_off[p.n] = wg;
    p.cap[p.n] = cap;
    p.tuple_off[p.n] = toff;
    p.cursor_off[p.n] = coff;
    wg += slices * split;
    toff += (int64_t)slices * cap;
    coff += slices;
    ++p.n;
  }
  p.wg_off[p.n] = wg;
  return p;
}

// workgroup `block` of hashgrid_reduce_kernel: entry li of the plan and its level, bucket, which of plan.split[li] parts
struct ReduceWork { int li, level, bucket, part; };
HG_HD ReduceWork reduce_work(const BucketPlan& plan, int block) {
  int li = 0;
#pragma unroll 1
  for (int i = 1; i < plan.n; ++i)
    if (block >= plan.wg_off[i]) li = i;
  const int level = plan.level[li];
  const int split = plan.split[li];
  const int local = block - plan.wg_off[li];
  const int b = local / split;
  return {li, level, b, local - b * split};
}
// the tuples [lo, hi) of its bucket that workgroup w reads when the bucket's cursor stands at `count`: the parts tile what
// was stored, and what went beyond the capacity was not (the bin kernel added it to the table itself)
struct TupleRange { long long lo, hi; };
HG_HD TupleRange reduce_range(const BucketPlan& plan, const ReduceWork& w, long long count) {
  if (count > plan.cap[w.li]) count = plan.cap[w.li];
  return {count * w.part / plan.split[w.li], count * (w.part + 1) / plan.split[w.li]};
}

// The scratch block of a plan: one cursor (unsigned) per bucket, then kMaxLevels level maxima (unsigned), rounded up to
// 256 bytes, then the tuples.  cursor_bytes is what is zeroed before binning.
struct BucketScratch { int64_t cursor_bytes, level_max_off, tuple_off, total; };  // bytes
inline BucketScratch bucket_scratch(const BucketPlan& p) {
  const int last = p.n - 1;
  const int64_t cursors = p.n ? p.cursor_off[last] + p.slices[last] : 0;
  const int64_t tuples = p.n ? p.tuple_off[last] + p.slices[last] * p.cap[last] : 0;
  const int64_t cursor_bytes = (((cursors + kMaxLevels) * 4 + 255) / 256) * 256;
  return {cursor_bytes, cursors * 4, cursor_bytes, cursor_bytes + tuples * kTupleBytes};
}

}  // namespace lnrf

#undef HG_HD
