// hashgrid.hip — multiresolution hash-grid encoding of Instant-NGP as restated by the reference:
// HashTableEncoding.__call__ (learn_nerf/instant_ngp.py:134-208), hash_table_lookup (:211-224),
// MultiresHashTableEncoding (:92-118).  F = 2 features per entry, fp32 tables as in the reference.
//
// MI355X mapping: the gather is bound by L2 / Infinity-Cache / HBM random access, not by FLOPs.  The
// launch is LEVEL-MAJOR: blockIdx.y = level, so all CUs sweep the points of one level at a time and that
// level's table (<= 2 MiB at T = 2^18, 4 MiB at 2^19) stays resident in every XCD's 4 MiB L2 instead of
// 16 tables thrashing it.  The encoding is written feature-major ([L*F][M]) so that both the gather
// kernel's stores and the scatter kernel's gradient loads are fully coalesced; the tiny MLP reads it
// through the strided GEMM.  The cell geometry, the launch plans and their decodes are in hashgrid_plan.h.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "hashgrid_plan.h"

namespace lnrf {

// what the kernels need of one level, taken from the descriptor in one place (offset: first float of its table)
struct Level { int G, T, hashed; long long offset; };
__device__ __forceinline__ Level level_of(const HashGridDesc& d, int l) {
  return {d.grid_size[l], d.table_size[l], d.hashed[l], d.table_offset[l]};
}

// body(xo, yo, zo, idx) for the 8 corners of the cell, xo outermost (instant_ngp.py:160-175).  Fully unrolled and without
// an exit: a body may hold wave-wide operations (run_reserve), and may leave out the weight of a corner it skips.
template <class Body>
__device__ __forceinline__ void for_each_corner(const Corner& k, const Level& lv, Body&& body) {
#pragma unroll
  for (int xo = 0; xo < 2; ++xo)
#pragma unroll
    for (int yo = 0; yo < 2; ++yo)
#pragma unroll
      for (int zo = 0; zo < 2; ++zo)
        body(xo, yo, zo, entry_index(k.base[0] + xo, k.base[1] + yo, k.base[2] + zo, lv.G, lv.T, lv.hashed));
}

// weight of a corner for sample m: the trilinear weight, or (u != nullptr) its derivative along u: sum_a u_a dw/dx_a
__device__ __forceinline__ float sample_weight(const Corner& k, int xo, int yo, int zo, const float* __restrict__ u,
                                               int64_t m) {
  if (!u) return corner_weight(k, xo, yo, zo);
  float gw[3];
  corner_weight_grad(k, xo, yo, zo, gw);
  return gw[0] * u[m * 3] + gw[1] * u[m * 3 + 1] + gw[2] * u[m * 3 + 2];
}

// one sample of one level: 8 corners x 2 features
__device__ __forceinline__ void gather_sample(const HashGridDesc& d, int level, const Level& lv,
                                              const float2* __restrict__ tab, const float* __restrict__ x,
                                              const float* __restrict__ u, int64_t M, float* __restrict__ enc_t,
                                              int64_t m) {
  const float p[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
  const Corner k = locate(p, d, lv.G);
  float2 acc = make_float2(0.0f, 0.0f);
  for_each_corner(k, lv, [&](int xo, int yo, int zo, unsigned idx) {
    const float w = sample_weight(k, xo, yo, zo, u, m);
    const float2 v = tab[idx];
    acc.x += w * v.x;
    acc.y += w * v.y;
  });
  enc_t[(int64_t)(2 * level) * M + m] = acc.x;
  enc_t[(int64_t)(2 * level + 1) * M + m] = acc.y;
}

// enc_t[(2*level + f) * M + m]
// u == nullptr: the encoding.  u != nullptr ([M,3]): its directional derivative (d enc / d x) u.
// STAGE: the level's whole table (dense levels of at most kStageEntries entries, i.e. the 16^3 grids that every
// sample of the batch hits) is first copied into LDS with coalesced 16-byte loads and the 8 corner reads of every
// sample are LDS reads; the launch uses few, long-lived workgroups so that one copy serves thousands of samples.
template <bool STAGE>
__global__ void hashgrid_fwd_kernel(HashGridDesc d, LevelList ll, const float* __restrict__ tables,
                                    const float* __restrict__ x, const float* __restrict__ u, int64_t M,
                                    float* __restrict__ enc_t) {
  extern __shared__ __attribute__((aligned(16))) float lds_tab[];
  const int level = ll.level[blockIdx.y];
  const Level lv = level_of(d, level);
  const float2* __restrict__ tab = reinterpret_cast<const float2*>(tables + lv.offset);
  if (STAGE) {
    // table_offset is a multiple of 2 floats (F = 2), i.e. 8-byte aligned: copy as float2, fully coalesced
    float2* lt = reinterpret_cast<float2*>(lds_tab);
    for (int i = threadIdx.x; i < lv.T; i += blockDim.x) lt[i] = tab[i];
    __syncthreads();
    tab = lt;  // generic pointer into LDS: the gathers below become ds_read_b64
  }
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x)
    gather_sample(d, level, lv, tab, x, u, M, enc_t, m);
}

// The same gather with the (level, sample chunk) -> workgroup mapping chosen per XCD (XcdPlan, hashgrid_plan.h).
__global__ __launch_bounds__(256) void hashgrid_fwd_xcd_kernel(HashGridDesc d, XcdPlan plan,
                                                               const float* __restrict__ tables,
                                                               const float* __restrict__ x, const float* __restrict__ u,
                                                               int64_t M, float* __restrict__ enc_t) {
  const XcdWork w = xcd_work(plan, blockIdx.x);
  if (w.seg < 0) return;
  const int level = xcd_level(plan, w);
  const Level lv = level_of(d, level);
  const float2* __restrict__ tab = reinterpret_cast<const float2*>(tables + lv.offset);
  const int64_t m = xcd_first_sample(plan, w) + threadIdx.x;
  if (m < M) gather_sample(d, level, lv, tab, x, u, M, enc_t, m);
}

// g_x[m][a] = sum_levels sum_f g_enc_t[(2l+f)*M + m] * sum_corners (d w / d x_a) table[idx][f]
// (transpose of d enc / d x applied to g_enc; the analytic normal of the Ref-NeRF head on a hash grid)
__global__ void hashgrid_input_grad_kernel(HashGridDesc d, const float* __restrict__ tables,
                                           const float* __restrict__ x, int64_t M,
                                           const float* __restrict__ g_enc_t, float* __restrict__ g_x) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int level = 0; level < d.n_levels; ++level) {
      const Level lv = level_of(d, level);
      const float2* __restrict__ tab = reinterpret_cast<const float2*>(tables + lv.offset);
      const Corner k = locate(p, d, lv.G);
      const float g0 = g_enc_t[(int64_t)(2 * level) * M + m];
      const float g1 = g_enc_t[(int64_t)(2 * level + 1) * M + m];
      for_each_corner(k, lv, [&](int xo, int yo, int zo, unsigned idx) {
        float gw[3];
        corner_weight_grad(k, xo, yo, zo, gw);
        const float2 v = tab[idx];
        const float s = g0 * v.x + g1 * v.y;
        acc[0] += gw[0] * s;
        acc[1] += gw[1] * s;
        acc[2] += gw[2] * s;
      });
    }
    g_x[m * 3 + 0] = acc[0];
    g_x[m * 3 + 1] = acc[1];
    g_x[m * 3 + 2] = acc[2];
  }
}

// Scatter without scratch memory: g_tables[level][idx][f] += w * g_enc_t[(2*level+f)*M + m] with float atomics.
// blockIdx.y = 8K-entry slice of the table, blockIdx.z = level in `ll`.  A level of 2 to 64 slices, or a dense one of a
// single slice, is pre-reduced in LDS (thousands of samples share an entry of a dense level, so direct atomics contend):
// every workgroup scans its chunk of points, accumulates only the corners that fall into its slice and flushes the slice
// with contiguous atomics; the index arithmetic is recomputed once per slice (cheap next to the contended atomics it
// replaces).  A hashed level of one slice, and a level of more than 64 slices (launched as one), add straight to the table.
__host__ __device__ __forceinline__ int fallback_slices(int T) { return (T + kSliceEntries - 1) / kSliceEntries; }
__global__ void hashgrid_bwd_fallback_kernel(HashGridDesc d, LevelList ll, const float* __restrict__ x,
                                             const float* __restrict__ u, int64_t M,
                                             const float* __restrict__ g_enc_t, float* __restrict__ g_tables) {
  extern __shared__ __attribute__((aligned(16))) float lds_tab[];
  const int level = ll.level[blockIdx.z];
  const Level lv = level_of(d, level);
  const unsigned slice0 = blockIdx.y * (unsigned)kSliceEntries;
  if (slice0 >= (unsigned)lv.T) return;
  float* __restrict__ gtab = g_tables + lv.offset;
  const int slices = fallback_slices(lv.T);
  const bool in_lds = slices <= 64 && (slices > 1 || !lv.hashed);
  const int n = (lv.T - (int)slice0 < kSliceEntries ? lv.T - (int)slice0 : kSliceEntries) * 2;  // floats of my slice
  if (in_lds) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) lds_tab[i] = 0.0f;
    __syncthreads();
  }
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    const float p[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
    const Corner k = locate(p, d, lv.G);
    const float g0 = g_enc_t[(int64_t)(2 * level) * M + m];
    const float g1 = g_enc_t[(int64_t)(2 * level + 1) * M + m];
    for_each_corner(k, lv, [&](int xo, int yo, int zo, unsigned idx) {
      const unsigned rel = idx - slice0;
      if (in_lds && rel >= (unsigned)kSliceEntries) return;  // another workgroup's slice: its weight is not computed
      const float w = sample_weight(k, xo, yo, zo, u, m);
      if (in_lds) {
        atomicAdd(&lds_tab[2 * rel], w * g0);
        atomicAdd(&lds_tab[2 * rel + 1], w * g1);
      } else {
        atomicAdd(gtab + 2 * (int64_t)idx, w * g0);
        atomicAdd(gtab + 2 * (int64_t)idx + 1, w * g1);
      }
    });
  }
  if (in_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const float v = lds_tab[i];
      if (v != 0.0f) atomicAdd(gtab + 2 * (int64_t)slice0 + i, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Bucketed scatter.  LDS float atomics are slow on gfx950 (ds_add_f32: ~0.3 lanes/clk/CU, measured with
// tools/lds_atomic_bench.hip; ds_add_u64: ~5.6) and memory-side float atomics slower still, so the gradient
// table is reduced with 64-bit INTEGER LDS atomics on fixed-point values:
// Pass A bins the 8 (entry, w*g0, w*g1) contributions of every sample by 4K-entry table slice: a workgroup
// counts its chunk per slice in LDS, reserves room in each slice's global bucket with ONE atomic per
// (workgroup, slice), writes its tuples there and records the level's max |value|.
// Pass B gives every (level, slice) bucket to one workgroup (few-slice levels: several), which converts the
// values to fixed point with the power-of-two scale 2^(62 - lg - e) (level max < 2^e, fewer than 2^lg tuples
// in the bucket: the sum cannot overflow; resolution 2^-46 of the max for a 64K-tuple bucket), accumulates
// them with ds_add_u64 and adds the slice to the gradient table.  Integer accumulation is order-independent, so unsplit slices are bit-reproducible.
// Buckets are sized 1.25x the mean for hashed levels (the hash spreads samples evenly), 4x for dense levels;
// overflowing tuples fall back to global atomics.
struct BucketTuple {
  unsigned rel;  // entry index within the 4K-entry slice
  float v0, v1;
};
static_assert(sizeof(BucketTuple) == kTupleBytes, "the scratch block is sized for this tuple");
// Plain scatter (u == nullptr): the trilinear weights are <= 1, so every contribution is bounded by the level's
// max |d loss / d enc|, which the producer of the gradient rows hands in (lnrf_ngp_mlp_bwd).  The values are then
// quantised right away to 26-bit fixed point relative to that bound (2^-25 of the level maximum, about fp32's own
// resolution at the maximum) and a tuple is 8 bytes: {q0 : 26 | rel[0:6], q1 : 26 | rel[6:12]} — a third less tuple
// traffic than {rel, float, float}, integer sums in the reduce pass without any floating-point conversion.
struct PackedTuple {
  unsigned w0, w1;
};
constexpr int kQuantBits = 26;
__device__ __forceinline__ PackedTuple pack_tuple(unsigned rel, float v0, float v1, float scale) {
  // saturate (a caller-supplied bound that is too small must not wrap through the 26-bit field into the other sign)
  constexpr float kQmax = (float)((1 << (kQuantBits - 1)) - 1);
  const int q0 = __float2int_rn(fminf(fmaxf(v0 * scale, -kQmax), kQmax));
  const int q1 = __float2int_rn(fminf(fmaxf(v1 * scale, -kQmax), kQmax));
  PackedTuple t;
  t.w0 = ((unsigned)q0 & 0x03FFFFFFu) | ((rel & 63u) << 26);
  t.w1 = ((unsigned)q1 & 0x03FFFFFFu) | ((rel >> 6) << 26);
  return t;
}

// One slot per valid lane in counter[b] with one LDS atomic per RUN of equal b in neighbouring lanes
// (neighbouring lanes = neighbouring samples of a ray: on dense levels they share the slice, and same-address
// LDS atomics serialise at ~0.5 lanes/clk).  Must be called by the whole wave.  Returns the lane's offset.
__device__ __forceinline__ unsigned run_reserve(unsigned* counter, unsigned b, bool valid) {
  const int lane = threadIdx.x & 63;
  const unsigned bb = valid ? b : 0xFFFFFFFFu;
  const unsigned prev = __shfl_up(bb, 1, 64);
  const bool head = lane == 0 || bb != prev;
  const unsigned long long heads = __ballot(head);
  const int hl = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));  // head lane of my run
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int len = above ? __ffsll((long long)above) : 64 - lane;              // run length (head lanes)
  unsigned base = 0u;
  if (head && valid) base = atomicAdd(&counter[bb], (unsigned)len);
  base = __shfl(base, hl, 64);
  return base + (unsigned)(lane - hl);
}

template <bool QUANT>
__global__ void hashgrid_bin_kernel(HashGridDesc d, BucketPlan plan, const float* __restrict__ x,
                                    const float* __restrict__ u, int64_t M, const float* __restrict__ g_enc_t,
                                    BucketTuple* __restrict__ tuples, unsigned* __restrict__ cursors,
                                    unsigned* __restrict__ level_max, float* __restrict__ g_tables) {
  __shared__ unsigned s_count[kMaxSlices];
  __shared__ unsigned s_base[kMaxSlices];
  const int li = blockIdx.y;
  const int level = plan.level[li];
  const int S = plan.slices[li];
  const Level lv = level_of(d, level);
  BucketTuple* __restrict__ tup = tuples + plan.tuple_off[li];
  PackedTuple* __restrict__ ptup = reinterpret_cast<PackedTuple*>(tuples) + plan.tuple_off[li];
  float qscale = 0.0f;  // QUANT: 2^(25 - e) with the caller's bound < 2^e
  if (QUANT) {
    int e = 0;
    frexpf(__uint_as_float(level_max[plan.level[li]]), &e);
    qscale = ldexpf(1.0f, kQuantBits - 1 - e);
  }
  unsigned* __restrict__ cur = cursors + plan.cursor_off[li];
  const long long cap = plan.cap[li];
  for (int i = threadIdx.x; i < S; i += blockDim.x) s_count[i] = 0u;
  __syncthreads();
  const int64_t m0 = (int64_t)blockIdx.x * kBinChunk;
  constexpr int kIters = kBinChunk / 256;  // blockDim.x == 256; uniform trip count (run_reserve needs the whole wave)
  // pass 1: count per slice
  for (int it = 0; it < kIters; ++it) {
    const int64_t m = m0 + it * 256 + threadIdx.x;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    const float p[3] = {x[mm * 3 + 0], x[mm * 3 + 1], x[mm * 3 + 2]};
    const Corner k = locate(p, d, lv.G);
    // hashed levels spread a wave over many slices (little same-address contention): plain LDS atomics are
    // cheaper than the run detection; dense levels put whole runs of lanes into one slice.  The wave-uniform choice
    // stands outside the walk: inside its body the compiler branches on it per corner (about 80 instructions more).
    if (lv.hashed) {
      for_each_corner(k, lv, [&](int, int, int, unsigned idx) {
        if (valid) atomicAdd(&s_count[idx / kBucketEntries], 1u);
      });
    } else {
      for_each_corner(k, lv, [&](int, int, int, unsigned idx) { run_reserve(s_count, idx / kBucketEntries, valid); });
    }
  }
  __syncthreads();
  // reserve room in the global buckets; s_count becomes the running local offset
  for (int i = threadIdx.x; i < S; i += blockDim.x) {
    s_base[i] = s_count[i] ? atomicAdd(&cur[i], s_count[i]) : 0u;
    s_count[i] = 0u;
  }
  __syncthreads();
  // pass 2: write the tuples
  float vmax = 0.0f;
  for (int it = 0; it < kIters; ++it) {
    const int64_t m = m0 + it * 256 + threadIdx.x;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    const float p[3] = {x[mm * 3 + 0], x[mm * 3 + 1], x[mm * 3 + 2]};
    const Corner k = locate(p, d, lv.G);
    const float g0 = valid ? g_enc_t[(int64_t)(2 * level) * M + mm] : 0.0f;
    const float g1 = valid ? g_enc_t[(int64_t)(2 * level + 1) * M + mm] : 0.0f;
    for_each_corner(k, lv, [&](int xo, int yo, int zo, unsigned idx) {
      const float w = sample_weight(k, xo, yo, zo, u, mm);
      const unsigned b = idx / kBucketEntries;
      const unsigned off = lv.hashed ? (valid ? atomicAdd(&s_count[b], 1u) : 0u) : run_reserve(s_count, b, valid);
      if (valid) {
        const long long pos = (long long)s_base[b] + off;
        // NaN / Inf contributions cannot be carried in fixed point: they take the float atomics below, which propagate
        // them into the table as the reference's scatter-add would, and their tuple slot carries zeros
        const float v0 = w * g0, v1 = w * g1;
        const bool finite = fabsf(v0) <= 3.0e38f && fabsf(v1) <= 3.0e38f;
        const float t0 = finite ? v0 : 0.0f, t1 = finite ? v1 : 0.0f;
        if (!QUANT) vmax = fmaxf(vmax, fmaxf(fabsf(t0), fabsf(t1)));
        if (pos < cap) {
          if (QUANT) {
            ptup[(long long)b * cap + pos] = pack_tuple(idx - b * kBucketEntries, t0, t1, qscale);
          } else {
            BucketTuple t;
            t.rel = idx - b * kBucketEntries;
            t.v0 = t0;
            t.v1 = t1;
            tup[(long long)b * cap + pos] = t;
          }
        }
        if (pos >= cap || !finite) {  // bucket full (rare), or a non-finite value
          float* gt = g_tables + lv.offset + 2 * (int64_t)idx;
          atomicAdd(gt, v0);
          atomicAdd(gt + 1, v1);
        }
      }
    });
  }
  if (!QUANT) {
    // level max |value| (fixed-point scale of pass B): non-negative floats order like their bit patterns
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    if ((threadIdx.x & 63) == 0 && vmax > 0.0f) atomicMax(&level_max[plan.level[li]], __float_as_uint(vmax));
  }
}

// Pass B.  A bucket is split among plan.split[level] workgroups (few-slice levels would otherwise leave
// most of the chip idle; their partial slices are flushed with atomics); blockIdx.x -> (level, bucket, part).
// The tuple stream is read kReduceUnroll tuples per thread ahead of the LDS atomics that consume it.
constexpr int kReduceThreads = 512;
constexpr int kReduceUnroll = 4;
// The two steps of the tuple loop that depend on the tuple form: put a tuple into slot q of the prefetched ones (ok
// false: it is from past the end and has to add zeros), and what a loaded tuple adds to entry `rel` of the slice.
template <bool QUANT>
using TupleRaw = std::conditional_t<QUANT, uint2, BucketTuple>;
template <bool QUANT>
__device__ __forceinline__ void tuple_load(TupleRaw<QUANT>* t, int q, const TupleRaw<QUANT>& src, bool ok) {
  t[q] = src;
  if constexpr (!QUANT) {  // on t[q], as the loop would write it: on a reference to the slot it compiles to other code
    t[q].v0 = ok ? t[q].v0 : 0.0f;
    t[q].v1 = ok ? t[q].v1 : 0.0f;
  }
}
template <bool QUANT>
__device__ __forceinline__ void tuple_decode(const TupleRaw<QUANT>& t, bool ok, double scale, unsigned& rel,
                                             long long& q0, long long& q1) {
  if constexpr (QUANT) {
    // 8-byte tuples: 26-bit values (sign-extended) summed as they are — 2^38 of them fit a signed 64-bit sum
    rel = (t.x >> 26) | ((t.y >> 26) << 6);
    q0 = ok ? (long long)(((int)(t.x << 6)) >> 6) : 0ll;
    q1 = ok ? (long long)(((int)(t.y << 6)) >> 6) : 0ll;
  } else {
    rel = t.rel;
    q0 = __double2ll_rn((double)t.v0 * scale);
    q1 = __double2ll_rn((double)t.v1 * scale);
  }
}
template <bool QUANT>
__global__ __launch_bounds__(kReduceThreads) void hashgrid_reduce_kernel(
    HashGridDesc d, BucketPlan plan, const BucketTuple* __restrict__ tuples, const unsigned* __restrict__ cursors,
    const unsigned* __restrict__ level_max, float* __restrict__ g_tables) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lds_q[];
  const ReduceWork wk = reduce_work(plan, (int)blockIdx.x);
  const int li = wk.li, level = wk.level, b = wk.bucket;
  const int split = plan.split[li];
  const int T = d.table_size[level];
  for (int i = threadIdx.x; i < kBucketEntries * 2; i += kReduceThreads) lds_q[i] = 0ull;
  __syncthreads();
  const TupleRange range = reduce_range(plan, wk, cursors[plan.cursor_off[li] + b]);
  const long long lo = range.lo, hi = range.hi;
  // power-of-two scale: level max < 2^e and at most n = hi - lo < 2^lg terms per entry, so values scaled by
  // 2^(62 - lg - e) cannot overflow the signed 64-bit sum whatever the sample distribution is
  int e = 0;
  frexpf(__uint_as_float(level_max[plan.level[li]]), &e);
  const int lg = 64 - __clzll((hi - lo) | 1ll);
  const int fixed_bits = 62 - lg;  // 46 for a 64K-tuple bucket
  const double scale = ldexp(1.0, fixed_bits - e);
  const double inv_scale = QUANT ? ldexp(1.0, e - (kQuantBits - 1)) : ldexp(1.0, e - fixed_bits);
  const TupleRaw<QUANT>* __restrict__ tup =
      reinterpret_cast<const TupleRaw<QUANT>*>(tuples) + plan.tuple_off[li] + (long long)b * plan.cap[li];
  for (long long i0 = lo + threadIdx.x; i0 < hi; i0 += (long long)kReduceUnroll * kReduceThreads) {
    TupleRaw<QUANT> t[kReduceUnroll];
    bool ok[kReduceUnroll];
    // branch-free: out-of-range slots re-read the last tuple and add zeros (a guarded load makes the
    // compiler wait for every load separately)
#pragma unroll
    for (int q = 0; q < kReduceUnroll; ++q) {
      const long long i = i0 + (long long)q * kReduceThreads;
      ok[q] = i < hi;
      tuple_load<QUANT>(t, q, tup[ok[q] ? i : hi - 1], ok[q]);
    }
#pragma unroll
    for (int q = 0; q < kReduceUnroll; ++q) {
      unsigned rel;
      long long q0, q1;
      tuple_decode<QUANT>(t[q], ok[q], scale, rel, q0, q1);
      atomicAdd(&lds_q[2 * rel], (unsigned long long)q0);
      atomicAdd(&lds_q[2 * rel + 1], (unsigned long long)q1);
    }
  }
  __syncthreads();
  const long long slice0 = (long long)b * kBucketEntries;
  const int n = (int)((T - slice0 < kBucketEntries ? T - slice0 : kBucketEntries) * 2);
  float* __restrict__ gt = g_tables + d.table_offset[level] + 2 * slice0;
  for (int i = threadIdx.x; i < n; i += kReduceThreads) {
    const long long q = (long long)lds_q[i];
    if (q != 0) {
      const float v = (float)((double)q * inv_scale);
      if (split == 1) gt[i] += v;  // this workgroup is the only writer of the slice in this launch
      else atomicAdd(gt + i, v);
    }
  }
}

}  // namespace lnrf

using namespace lnrf;

static int check_desc(const lnrf_hashgrid_desc* d) {
  if (!d) { set_error("hashgrid: null descriptor"); return LNRF_ERR_ARG; }
  if (d->n_levels < 1 || d->n_levels > kMaxLevels) { set_error("hashgrid: n_levels out of range"); return LNRF_ERR_ARG; }
  if (d->feature_dim != 2) {
    set_error("hashgrid: only feature_dim == 2 is implemented (the reference default)");
    return LNRF_ERR_UNSUPPORTED;
  }
  for (int l = 0; l < d->n_levels; ++l)
    if (d->grid_size[l] < 2 || d->table_size[l] < 1) { set_error("hashgrid: bad level"); return LNRF_ERR_ARG; }
  return LNRF_OK;
}

// The checks every launching entry point starts with; *d = the descriptor.  m == 0 passes: the caller returns early.
static int check_args(const char* fn, const lnrf_hashgrid_desc* desc, bool pointers, int64_t m, HashGridDesc* d) {
  const int rc = check_desc(desc);
  if (rc) return rc;
  if (!pointers || m < 0) {
    set_error("%s: %s", fn, pointers ? "bad m" : "null pointer");
    return LNRF_ERR_ARG;
  }
  memcpy((void*)d, (const void*)desc, sizeof(*d));
  return LNRF_OK;
}

extern "C" int lnrf_hashgrid_fwd(const lnrf_hashgrid_desc* desc, const float* tables, const float* x, int64_t m,
                                 float* enc_t, lnrf_stream_t stream) {
  return lnrf_hashgrid_jvp(desc, tables, x, nullptr, m, enc_t, stream);
}

extern "C" int lnrf_hashgrid_jvp(const lnrf_hashgrid_desc* desc, const float* tables, const float* x,
                                 const float* u, int64_t m, float* enc_t, lnrf_stream_t stream) {
  HashGridDesc d;
  int rc = check_args(__func__, desc, tables && x && enc_t, m, &d);
  if (rc || m == 0) return rc;
  // dense levels whose table fits in 64 KiB of LDS are staged there (LDS gather); the others gather from L2 / HBM
  LevelList staged, direct;
  staged.n = direct.n = 0;
  for (int l = 0; l < d.n_levels; ++l) {
    if (!d.hashed[l] && d.table_size[l] <= kStageEntries && m >= 16384)
      staged.level[staged.n++] = l;
    else direct.level[direct.n++] = l;
  }
  if (direct.n > 0 && (m + 255) / 256 * direct.n <= (int64_t)1 << 28) {
    unsigned grid = 0;
    const XcdPlan plan = make_xcd_plan(d, direct, m, &grid);
    if (grid == 0) {
      set_error("hashgrid: inconsistent XCD plan");
      return LNRF_ERR_ARG;
    }
    hipLaunchKernelGGL(hashgrid_fwd_xcd_kernel, dim3(grid), dim3(256), 0, as_stream(stream), d, plan, tables, x, u, m,
                       enc_t);
    LNRF_LAUNCH_CHECK();
  } else if (direct.n > 0) {
    int64_t bx = (m + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(hashgrid_fwd_kernel<false>, dim3((unsigned)bx, (unsigned)direct.n), dim3(256), 0,
                       as_stream(stream), d, direct, tables, x, u, m, enc_t);
    LNRF_LAUNCH_CHECK();
  }
  if (staged.n > 0) {
    // one table copy (32 KiB for a 16^3 grid, read from L2) per 512-thread workgroup and >= 1024 samples; LDS is
    // sized to the largest staged table so that four such workgroups share a CU
    int max_rows = 0;
    for (int i = 0; i < staged.n; ++i)
      if (d.table_size[staged.level[i]] > max_rows) max_rows = d.table_size[staged.level[i]];
    int64_t bx = (m + 1023) / 1024;
    if (bx > 1024) bx = 1024;
    rc = set_max_dynamic_lds(hashgrid_fwd_kernel<true>, kStageEntries * 8);
    if (rc) return rc;
    hipLaunchKernelGGL(hashgrid_fwd_kernel<true>, dim3((unsigned)bx, (unsigned)staged.n), dim3(512), max_rows * 8,
                       as_stream(stream), d, staged, tables, x, u, m, enc_t);
    LNRF_LAUNCH_CHECK();
  }
  return LNRF_OK;
}

extern "C" int lnrf_hashgrid_input_grad(const lnrf_hashgrid_desc* desc, const float* tables, const float* x,
                                        int64_t m, const float* g_enc_t, float* g_x, lnrf_stream_t stream) {
  HashGridDesc d;
  const int rc = check_args(__func__, desc, tables && x && g_enc_t && g_x, m, &d);
  if (rc || m == 0) return rc;
  int64_t bx = (m + 255) / 256;
  if (bx > 8192) bx = 8192;
  hipLaunchKernelGGL(hashgrid_input_grad_kernel, dim3((unsigned)bx), dim3(256), 0, as_stream(stream), d, tables, x, m,
                     g_enc_t, g_x);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int64_t lnrf_hashgrid_bwd_scratch_bytes(const lnrf_hashgrid_desc* desc, int64_t m) {
  if (check_desc(desc)) return -1;
  HashGridDesc d;
  memcpy((void*)&d, (const void*)desc, sizeof(d));
  return bucket_scratch(make_plan(d, m)).total;
}

extern "C" int lnrf_hashgrid_bwd_dir(const lnrf_hashgrid_desc* desc, const float* x, const float* u, int64_t m,
                                     const float* g_enc_t, float* g_tables, lnrf_stream_t stream) {
  return lnrf_hashgrid_bwd_bucketed(desc, x, u, m, g_enc_t, nullptr, g_tables, nullptr, 0, stream);
}

extern "C" int lnrf_hashgrid_bwd_bucketed(const lnrf_hashgrid_desc* desc, const float* x, const float* u, int64_t m,
                                          const float* g_enc_t, const float* level_absmax, float* g_tables,
                                          void* scratch, int64_t scratch_bytes, lnrf_stream_t stream) {
  HashGridDesc d;
  const int rc = check_args(__func__, desc, x && g_enc_t && g_tables, m, &d);
  if (rc || m == 0) return rc;
  // bucketed path when the caller provides scratch memory; without it every level takes the fallback kernel
  const BucketPlan plan = make_plan(d, m);
  const BucketScratch sc = bucket_scratch(plan);
  const bool use_buckets = scratch && plan.n > 0 && scratch_bytes >= sc.total;
  if (use_buckets) {
    unsigned* cursors = reinterpret_cast<unsigned*>(scratch);
    unsigned* level_max = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(scratch) + sc.level_max_off);
    BucketTuple* tuples = reinterpret_cast<BucketTuple*>(reinterpret_cast<char*>(scratch) + sc.tuple_off);
    hipError_t e = hipMemsetAsync(cursors, 0, (size_t)sc.cursor_bytes, as_stream(stream));
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(bucket cursors)");
    const unsigned chunks = (unsigned)((m + kBinChunk - 1) / kBinChunk);
    // The caller hands in a bound of |g| per level (lnrf_ngp_mlp_bwd finds it while it writes the rows; weights <= 1):
    // quantised 8-byte tuples, 2^-25 of that bound per contribution.  This is the fused bf16 path's scatter.  WITHOUT a
    // bound (the exact-fp32 path, any other caller), or with directional-derivative weights (unbounded): 12-byte fp32
    // tuples, level maximum found while binning, 64-bit fixed point of 2^-46 of the maximum per contribution in the
    // reduce pass.
    const bool quant = u == nullptr && level_absmax != nullptr;
    if (quant) level_max = reinterpret_cast<unsigned*>(const_cast<float*>(level_absmax));  // read only from here on
    hipLaunchKernelGGL(quant ? hashgrid_bin_kernel<true> : hashgrid_bin_kernel<false>, dim3(chunks, (unsigned)plan.n),
                       dim3(256), 0, as_stream(stream), d, plan, x, u, m, g_enc_t, tuples, cursors, level_max, g_tables);
    LNRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(quant ? hashgrid_reduce_kernel<true> : hashgrid_reduce_kernel<false>,
                       dim3((unsigned)plan.wg_off[plan.n]), dim3(kReduceThreads), 64 * 1024, as_stream(stream), d, plan,
                       tuples, cursors, level_max, g_tables);
    LNRF_LAUNCH_CHECK();
  }
  // What is not bucketed: every level without scratch, tables of more than kMaxSlices bucket slices with it.  Levels of
  // 2 to 64 8K-slices are launched one workgroup row per slice, the others (one slice, or too many) as a single row.
  LevelList whole, sliced;
  whole.n = sliced.n = 0;
  int max_slices = 1;
  for (int l = 0; l < d.n_levels; ++l) {
    if (use_buckets && level_is_bucketed(d, l)) continue;
    const int slices = fallback_slices(d.table_size[l]);
    if (slices > 1 && slices <= 64) {
      sliced.level[sliced.n++] = l;
      if (slices > max_slices) max_slices = slices;
    } else {
      whole.level[whole.n++] = l;
    }
  }
  const int64_t max_bx = (m + 255) / 256;
  if (whole.n > 0) {
    const int64_t bx = max_bx < 1024 ? max_bx : 1024;
    hipLaunchKernelGGL(hashgrid_bwd_fallback_kernel, dim3((unsigned)bx, 1u, (unsigned)whole.n), dim3(256), 64 * 1024,
                       as_stream(stream), d, whole, x, u, m, g_enc_t, g_tables);
    LNRF_LAUNCH_CHECK();
  }
  if (sliced.n > 0) {
    int64_t bx = 1024 / max_slices;
    if (bx < 8) bx = 8;
    if (bx > max_bx) bx = max_bx;
    hipLaunchKernelGGL(hashgrid_bwd_fallback_kernel, dim3((unsigned)bx, (unsigned)max_slices, (unsigned)sliced.n),
                       dim3(256), 64 * 1024, as_stream(stream), d, sliced, x, u, m, g_enc_t, g_tables);
    LNRF_LAUNCH_CHECK();
  }
  return LNRF_OK;
}
