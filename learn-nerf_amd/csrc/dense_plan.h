// dense_plan.h — the dispatch decision of the generic dense path (dense.hip) as plain host arithmetic: which GEMM kernel a
// problem takes, its template flags, the reduction split and the grid; the split counts the scratch blocks are sized
// for; and the blockIdx -> tile map of gemm_big_kernel.  No HIP types: dense.hip launches from a GemmPlan, and
// layout_host.cpp exports the same functions to the CPU tests (tests/test_dense_plan.py), so there is one copy of the
// predicate.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

namespace lnrf {

// generic kernel: 64x64 output tile, 16-deep reduction chunk.  big kernel: 128x128, chunk 16 (fp32) / 32 (bf16).
constexpr int TI = 64, TJ = 64, RC = 16;
constexpr int BI = 128, BJ = 128;
constexpr int kBigKcF32 = 16, kBigKcBf16 = 32;
constexpr int kColSumRows = 512;  // rows per partial sum of the bias gradient

struct GemmPlan {
  int launch;     // 0: nothing to do (I == 0 or J == 0)
  int big;        // 1: gemm_big_kernel<bf16, a_fast_r, b_fast_r, b_aligned>, 0: gemm_f32_kernel<bf16>
  int bf16;
  int a_fast_r;   // big only: A contiguous in r (else in i)
  int b_fast_r;   // big only: B contiguous in r (else in j)
  int b_aligned;  // big only: B 16-byte aligned
  int kc;         // reduction depth per chunk
  int splits;     // splits asked for once the mode has had its say: 1, the caller's count, or gemm_auto_splits
  int nsplit;     // gridDim.z: splits of the reduction that are launched (none empty, never more than `splits`)
  int64_t lda, ldb;      // big only: stride of the non-contiguous dimension
  int64_t r_per_split;   // reduction depth per split, a multiple of kc
  unsigned gx, gy, gz;   // grid
};

// Split count of a split reduction whose caller leaves the choice open (weight gradient over m, lnrf_gemm_f32 mode 2 with
// splits = 0, lnrf_gemm_f32_det): ~2048 workgroups over the 64x64 tiles, at least 256 deep each, at most 512.
inline int gemm_auto_splits(int64_t I, int64_t J, int64_t R) {
  const int64_t tiles = ((I + TI - 1) / TI) * ((J + TJ - 1) / TJ);
  int64_t splits = (2048 + tiles - 1) / (tiles > 0 ? tiles : 1);
  if (splits > 512) splits = 512;
  const int64_t max_splits = (R + 255) / 256;
  if (splits > max_splits) splits = max_splits;
  return splits < 1 ? 1 : (int)splits;
}

// a_low / b_low: the low 4 bits of the operand addresses.  mode as lnrf_gemm_f32 (3: split partials).  splits: requested
// splits of the reduction; modes 0 and 1 never split, modes 2 and 3 choose with gemm_auto_splits when splits <= 0.
inline GemmPlan gemm_plan(int64_t sa_i, int64_t sa_r, int64_t sb_r, int64_t sb_j, int64_t I, int J, int64_t R,
                          unsigned a_low, unsigned b_low, bool bf16, int mode, int splits) {
  GemmPlan p{};
  p.bf16 = bf16;
  if (I == 0 || J == 0) return p;
  p.launch = 1;
  if (mode < 2) splits = 1;
  else if (splits <= 0) splits = gemm_auto_splits(I, J, R);
  p.splits = splits;
  // vectorised 128x128 kernel: both operands contiguous along one of their dimensions, 16-byte aligned rows,
  // extents along the contiguous dimensions multiples of 4, and enough work to fill 128-wide tiles
  const bool a_fast_r = sa_r == 1, a_fast_i = sa_i == 1 && !a_fast_r;
  const bool b_fast_r = sb_r == 1, b_fast_j = sb_j == 1;
  const int64_t lda = a_fast_r ? sa_i : sa_r, ldb = b_fast_r ? sb_j : sb_r;
  // A contiguous in i = X^T of the weight gradient: transposing LDS stores (swizzled bf16 image / 17-float rows in f32)
  const bool big = (a_fast_r || a_fast_i) && (b_fast_r || b_fast_j) && (a_low & 15u) == 0 &&
                   lda % 4 == 0 && ldb % 4 == 0 && (a_fast_r ? R % 4 == 0 : I % 4 == 0) &&
                   (b_fast_r ? R % 4 == 0 : J % 4 == 0) && I >= 64 && J >= 64 && R >= 32;
  if (big) {
    const int kc = bf16 ? kBigKcBf16 : kBigKcF32;
    int64_t per = (R + splits - 1) / splits;
    per = ((per + kc - 1) / kc) * kc;
    if (per % 4 != 0) per = ((per + 3) / 4) * 4;
    int nsplit = (int)((R + per - 1) / per);
    if (nsplit < 1) nsplit = 1;
    const int64_t ni = (I + BI - 1) / BI, njt = (J + BJ - 1) / BJ;
    p.big = 1;
    p.a_fast_r = a_fast_r;
    p.b_fast_r = !b_fast_j;
    p.b_aligned = (b_low & 15u) == 0;  // weights inside a flat parameter vector may start at any float
    p.kc = kc;
    p.nsplit = nsplit;
    p.lda = lda;
    p.ldb = ldb;
    p.r_per_split = per;
    p.gx = (unsigned)((ni >= 64 ? ((ni + 7) / 8) * 8 : ni) * njt);  // tile order: gemm_big_tile
    p.gy = 1u;
    p.gz = (unsigned)nsplit;
    return p;
  }
  int64_t per = (R + splits - 1) / splits;
  per = ((per + RC - 1) / RC) * RC;
  if (per < RC) per = RC;
  splits = (int)((R + per - 1) / per);
  if (splits < 1) splits = 1;
  p.kc = RC;
  p.nsplit = splits;
  p.r_per_split = per;
  p.gx = (unsigned)((I + TI - 1) / TI);
  p.gy = (unsigned)((J + TJ - 1) / TJ);
  p.gz = (unsigned)splits;
  return p;
}

// Scratch of lnrf_dense_bwd_weight_det: split partials of the kernel gradient (k = 0: none), then the bias partials.
inline int64_t dense_wgrad_scratch_bytes(int64_t m, int k, int n) {
  if (m < 0 || k < 0 || n < 1) return -1;
  const int64_t kernel_parts = k > 0 ? (int64_t)gemm_auto_splits(k, n, m) * k * n : 0;
  const int64_t bias_parts = (m + kColSumRows - 1) / kColSumRows * n;
  return (kernel_parts + bias_parts) * (int64_t)sizeof(float) + 256;
}
// Scratch of lnrf_gemm_f32_det.
inline int64_t gemm_det_scratch_bytes(int64_t I, int J, int64_t R) {
  if (I < 0 || J < 0 || R < 0) return -1;
  return (int64_t)gemm_auto_splits(I, J, R) * I * J * (int64_t)sizeof(float) + 256;
}

// blockIdx.x -> (row tile, column tile) of gemm_big_kernel; ni, nj = number of 128-row / 128-column tiles.
// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an L2), so
// the column tiles of one row tile are placed 8 blocks apart: the second one finds the A tile in its XCD's L2
// instead of re-reading it from HBM.  block = (8 nj) g + 8 jt + t  ->  row tile 8 g + t, column tile jt.
// (Few row tiles, e.g. the split-K weight gradient: plain order, or all the work would land on ni of the 8 XCDs.)
// A block of the padded grid lands on it >= ni or jt >= nj and leaves.
struct GemmTile {
  int64_t it;
  int jt;
};
DP_HD GemmTile gemm_big_tile(unsigned block, int64_t ni, int nj) {
  GemmTile t;
  if (ni >= 64) {
    const unsigned grp = block / (8u * nj), rem = block % (8u * nj);
    t.it = (int64_t)grp * 8 + (rem & 7u);
    t.jt = (int)(rem >> 3);
  } else {
    t.it = block % (unsigned)ni;
    t.jt = (int)(block / (unsigned)ni);
  }
  return t;
}

}  // namespace lnrf

#undef DP_HD
