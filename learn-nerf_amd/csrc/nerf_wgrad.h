// nerf_wgrad.h — everything about the split-K weight-gradient launch (nerf_wgrad_kernel + its slab fold) that is plain
// integer arithmetic: the operand-shape table, the problem record, which gradient-vector entry an accumulator register
// belongs to, and the problem list of every caller.  No HIP types: device code gets it through fused_chain.h, and
// layout_host.cpp builds it for the CPU so that tests/test_nerf_layout.py can check that every list gives every
// parameter exactly one owner (what makes the fold a plain read-modify-write and the step bit-reproducible).
#pragma once
#include "nerf_layout.h"

namespace lnrf {
using namespace nl;

// ---- slabs: the partial sums of one workgroup --------------------------------------------------------------------
// floats per (workgroup, wave): up to 9 accumulator tiles of 64 lanes x 16 + 4 bias rows
constexpr int kSlabMaxTiles = 9, kSlabMaxTO = 4;
constexpr int kSlabTileFloats = 64 * 16;
constexpr int kSlabWaveFloats = kSlabMaxTiles * kSlabTileFloats + kSlabMaxTO * 64;
constexpr int64_t kSlabBlockBytes = (int64_t)kWaves * kSlabWaveFloats * (int64_t)sizeof(float);
// the most workgroups one launch_nerf_wgrad call may use: every caller's slab region holds this many slabs
constexpr int kWgradMaxBlocks = 512;
constexpr int64_t kWgradSlabBytes = kWgradMaxBlocks * kSlabBlockBytes;

// ---- operand shapes ----------------------------------------------------------------------------------------------
// (name, id, NXF, NYF, WI, WO, SPI): X tensor of NXF k-step slots x dy tensor of NYF slots, on a WI x WO grid of waves,
// SPI steps per barrier (chosen so that every body keeps ~60 KB of loads in flight per workgroup); id is the value in
// WgradProblem::shape.  The body and both folds expand this one list, so they cannot disagree.  X_ELSE marks the row whose
// code a kernel also runs for a shape value outside the table (WgradList cannot produce one): a switch expands the list
// as LNRF_WGRAD_SHAPES(X, default: X).  The ids and the row order are those of the switches this table replaced, so
// that the kernels compile to the same code.
#define LNRF_WGRAD_SHAPES(X, X_ELSE)                                                                      \
  X(WG_HIDDEN, 0, 16, 16, 4, 2, 2)       /* h_{l-1} x dy_l, l = 1..8 */                                   \
  X(WG_Z_DY10M, 1, 16, 10, 4, 2, 2)      /* z x dy10m */                                                  \
  X(WG_XEMB, 2, 4, 16, 2, 4, 3)          /* x_emb x dy0, x_emb x dy5 */                                   \
  X(WG_DEMB_DY10M, 3, 2, 10, 1, 8, 5)    /* d_emb x dy10m */                                              \
  X(WG_DIR9, 5, 18, 8, 4, 2, 2)          /* Ref-NeRF Dense_9 */                                           \
  X(WG_ZD_DY10M, 6, 18, 10, 4, 2, 2)     /* [z | d_emb] x dy10m */                                        \
  X(WG_XEMB_DY0_DY5, 7, 4, 32, 2, 4, 2)  /* x_emb x [dy0 | dy5] */                                        \
  X_ELSE(WG_H128_DY3, 4, 8, 2, 4, 2, 6)  /* 128 hidden x 3 colours: h10 x dy11, Ref-NeRF Dense_10 */
// the shapes of the layer-stationary finish phase (wgrad_list_ls_finish): all nerf_ls_fold_kernel carries
#define LNRF_WGRAD_LS_SHAPES(X, X_ELSE) X(WG_XEMB_DY0_DY5) X(WG_ZD_DY10M) X_ELSE(WG_H128_DY3)

enum WgradShape : int {
#define X(name, id, nxf, nyf, wi, wo, spi) name = id,
  LNRF_WGRAD_SHAPES(X, X)
#undef X
};
template <WgradShape S>
struct WgShape;
#define X(name, id, nxf, nyf, wi, wo, spi)                                              \
  template <>                                                                           \
  struct WgShape<name> {                                                                \
    static constexpr int NXF = nxf, NYF = nyf, WI = wi, WO = wo, SPI = spi;             \
    static constexpr int TI = (nxf / 2 + wi - 1) / wi, TO = (nyf / 2 + wo - 1) / wo; /* accumulator tiles per wave */ \
  };
LNRF_WGRAD_SHAPES(X, X)
#undef X

// ---- problems  dW_l[in][out] += sum_m X_l[m][in] * dy_l[m][out] -----------------------------------------------------
enum { ROW_HIDDEN = 0, ROW_XEMB = 1, ROW_DEMB = 2, ROW_Z_DEMB = 3 };  // ROW_Z_DEMB: 16 slots of z, then 2 of d_emb
enum { COL_256 = 0, COL_DY10M = 1, COL_DY11 = 2, COL_EXPLICIT = 3, COL_DY0_DY5 = 4 };  // COL_DY0_DY5: tiles 0..7 dy0, 8..15 dy5
struct WgradProblem {
  WgradShape shape;
  int x_slot0;   // first X slot in the forward save buffer
  int y_slot0;   // first dy slot in the gradient dump
  int dense;     // Flax Dense index (COL_DY10M: Dense_10 with Dense_9 attached as column 128)
  int row_map;   // how X slots map to kernel rows
  int row_off;   // first kernel row of this block
  int col_map;
  int do_bias;
  int first_block, n_blocks;
  // COL_EXPLICIT (kernels outside NeRFModel's parameter layout, e.g. RefNERFModel's directional block): float offsets
  // of the kernel / bias in the gradient vector, kernel columns, and number of real kernel rows
  int w_off, b_off, out_dim, n_rows;
};
constexpr int kMaxProblems = 13;
struct WgradArgs {
  WgradProblem p[kMaxProblems];
  int n_problems;
};

// NeRFModel gradient-vector addressing for the shared weight-gradient body
struct NerfWgradEpi {
  static NL_HD void cols(const WgradProblem& pb, int ot, int colr, int& out_idx, int& out_dim, int64_t& w_off,
                         int64_t& b_off) {
    int dense_w = pb.dense;
    if (pb.col_map == COL_DY10M) {  // tiles 0..3 = Dense_10 outputs, tile 4 column 0 = Dense_9
      if (ot < 4) { out_idx = 32 * ot + colr; out_dim = 128; dense_w = 10; }
      else if (colr == 0 && pb.row_map != ROW_DEMB) { out_idx = 0; out_dim = 1; dense_w = 9; }
    } else if (pb.col_map == COL_DY0_DY5) {  // x_emb rows: Dense_0 (with its bias), then rows 256.. of Dense_5 (no bias)
      out_idx = 32 * (ot & 7) + colr; out_dim = 256;
      if (ot >= 8) {
        w_off = dense_w_off(5) + 256 * 256;
        b_off = -1;
        return;
      }
      dense_w = 0;
    } else if (pb.col_map == COL_DY11) {
      if (colr < 3) { out_idx = colr; out_dim = 3; }
    } else if (pb.col_map == COL_EXPLICIT) {
      if (32 * ot + colr < pb.out_dim) out_idx = 32 * ot + colr;
      out_dim = pb.out_dim;
      w_off = pb.w_off;
      b_off = pb.b_off;
      return;
    } else {
      out_idx = 32 * ot + colr; out_dim = 256;
    }
    w_off = dense_w_off(dense_w);
    b_off = dense_b_off(dense_w);
  }
  static NL_HD int row(const WgradProblem& pb, int f, int r16) {
    const int sh = (r16 >> 2) & 1, sj = 4 * (r16 >> 3) + (r16 & 3);  // slot (h, j) of that feature
    int in_idx;
    if (pb.row_map == ROW_HIDDEN) {
      in_idx = 16 * f + r16;
      if (pb.col_map == COL_EXPLICIT && in_idx >= pb.n_rows) in_idx = -1;
    } else if (pb.row_map == ROW_Z_DEMB) {
      if (f < 16) in_idx = 16 * f + r16;
      else {
        in_idx = demb_feat(f - 16, sh, sj);
        if (in_idx >= 0) in_idx += 256;
      }
    } else if (pb.row_map == ROW_XEMB) in_idx = xemb_feat(f, sh, sj);
    else in_idx = demb_feat(f, sh, sj);
    return in_idx >= 0 ? in_idx + pb.row_off : -1;
  }
  // rows of the kernel behind column tile `ot` (rows at or above it belong to no parameter): Dense_9 takes z only
  static NL_HD int row_limit(const WgradProblem& pb, int ot) {
    return pb.col_map == COL_DY10M && ot >= 4 ? 256 : 0x7FFFFFFF;
  }
};

// ---- who owns what ------------------------------------------------------------------------------------------------
// Every wave of a producing workgroup holds TI x TO accumulator tiles.  Tile j = a * TO + b of wave w is tile (it, ot)
// of the problem's grid of 32 x 32 tiles, or padding of the wave grid (real == false).  The bias row of out-tile ot is
// summed by the waves with wi == 0 in a == 0.
template <int NXF, int NYF, int WI, int WO>
constexpr int kWgradWaveTiles = ((NXF / 2 + WI - 1) / WI) * ((NYF / 2 + WO - 1) / WO);
struct WgradTile {
  bool real, bias;
  int it, ot, b;
};
template <int NXF, int NYF, int WI, int WO>
NL_HD WgradTile wgrad_tile(int w, int j) {
  constexpr int NI = NXF / 2, NO = NYF / 2, TO = (NO + WO - 1) / WO;
  static_assert(kWgradWaveTiles<NXF, NYF, WI, WO> <= kSlabMaxTiles && TO <= kSlabMaxTO, "slab layout");
  const int a = j / TO, b = j % TO;
  const int wi = w / WO, wo = w % WO;
  const int it = wi + WI * a, ot = wo + WO * b;
  return WgradTile{it < NI && ot < NO, wi == 0 && a == 0, it, ot, b};
}
// Where what lane (colr, hh) of the folding wave holds for tile (it, ot) goes in the gradient vector: register qq of the
// accumulator tile, and the bias sum.  false: nowhere (padding of the tile, or no such parameter).
template <class EPI, class PB>
struct WgradOwner {
  int out_idx = -1, out_dim = 1, row_lim;
  int64_t w_off = 0, b_off = 0;
  NL_HD WgradOwner(const PB& pb, int ot, int colr) {
    EPI::cols(pb, ot, colr, out_idx, out_dim, w_off, b_off);
    row_lim = EPI::row_limit(pb, ot);
  }
  NL_HD bool bias(int hh, int64_t& idx) const {
    idx = b_off + out_idx;
    return hh == 0 && out_idx >= 0 && b_off >= 0;
  }
  NL_HD bool weight(const PB& pb, int it, int hh, int qq, int64_t& idx) const {
    const int r = (qq & 3) + 8 * (qq >> 2) + 4 * hh;  // row in the 32-feature tile
    const int f = 2 * it + (r >> 4);                   // k-step slot within X
    const int in_idx = EPI::row(pb, f, r & 15);
    idx = w_off + (int64_t)in_idx * out_dim + out_idx;
    return out_idx >= 0 && in_idx >= 0 && in_idx < row_lim;
  }
};

// ---- problem lists (host) -----------------------------------------------------------------------------------------
// Problems in launch order (heaviest first, so that the small ones fill the tail of the launch), each on the workgroups
// [first_block, first_block + n_blocks).  A problem gets the workgroups it asks for, but at most one per 6 tiles.
// n_tiles is padded to whole workgroups (common.h padded_tiles), so it is at least 8 and the cap at least 2: no problem
// ends up with zero workgroups.
struct WgradList {
  WgradArgs args;
  int blocks = 0;  // workgroups of the launch so far
  int64_t cap;
  explicit WgradList(int64_t n_tiles) : cap((n_tiles + 5) / 6) { args.n_problems = 0; }

  WgradProblem& add(int want, WgradShape shape, int xs, int ys, int dense, int row_map, int row_off, int col_map,
                    int do_bias) {
    WgradProblem& p = args.p[args.n_problems++];
    p = WgradProblem{shape, xs, ys, dense, row_map, row_off, col_map, do_bias, blocks, (int)(want < cap ? want : cap),
                     0, 0, 0, 0};
    blocks += p.n_blocks;
    return p;
  }
  // Dense_l, l = 1..8: h_{l-1} x dy_l
  void hidden(int want, int l, int do_bias) {
    add(want, WG_HIDDEN, kSaveH + (l - 1) * 16, grad_dy_slot(l), l, ROW_HIDDEN, 0, COL_256, do_bias);
  }
  // x_emb x [dy0 | dy5]: Dense_0 (with its bias) and rows 256..315 of Dense_5; the two dumps are neighbours (nerf_layout.h)
  void xemb_dy0_dy5(int want, int do_bias) {
    add(want, WG_XEMB_DY0_DY5, kSaveXin, grad_dy_slot(0), 0, ROW_XEMB, 0, COL_DY0_DY5, do_bias);
  }
  // [z | d_emb] x dy10m: Dense_10 (all 280 rows) and Dense_9; neighbours in the save layout, so dy10m is read once
  void zd_dy10m(int want) { add(want, WG_ZD_DY10M, kSaveZ, kGradDy10m, 10, ROW_Z_DEMB, 0, COL_DY10M, 1); }
  // h10 x dy11: Dense_11
  void h10_dy11(int want) { add(want, WG_H128_DY3, kSaveH10, kGradDy11, 11, ROW_HIDDEN, 0, COL_DY11, 1); }
  // a kernel [n_rows][out_dim] at w_off with its bias at b_off, outside NeRFModel's parameter layout
  void explicit_at(int want, WgradShape shape, int xs, int ys, int out_dim, int n_rows, int w_off, int b_off) {
    WgradProblem& p = add(want, shape, xs, ys, 0, ROW_HIDDEN, 0, COL_EXPLICIT, 1);
    p.w_off = w_off; p.b_off = b_off; p.out_dim = out_dim; p.n_rows = n_rows;
  }
};

// lnrf_nerf_mlp_bwd_weights (the "split" backward): all 13 problems of one NeRFModel, workgroups proportional to bytes
// (kWgradMaxBlocks in all)
inline WgradList wgrad_list_split(int64_t n_tiles) {
  WgradList w(n_tiles);
  for (int l = 1; l <= 8; ++l) w.hidden(l <= 4 ? 48 : 47, l, 1);
  w.add(39, WG_Z_DY10M, kSaveZ, kGradDy10m, 10, ROW_HIDDEN, 0, COL_DY10M, 1);      // Dense_10 rows 0..255 and Dense_9
  w.add(30, WG_XEMB, kSaveXin, grad_dy_slot(0), 0, ROW_XEMB, 0, COL_256, 1);       // Dense_0
  w.add(30, WG_XEMB, kSaveXin, grad_dy_slot(5), 5, ROW_XEMB, 256, COL_256, 0);     // Dense_5 rows 256..315
  w.add(18, WG_DEMB_DY10M, kSaveDin, kGradDy10m, 10, ROW_DEMB, 256, COL_DY10M, 0);  // Dense_10 rows 256..279
  w.h10_dy11(15);
  return w;
}
// finish phase of the layer-stationary backward: what is not a pipeline stage.  Workgroups in proportion to the bytes a
// problem streams per tile (36, 28, 10 KiB); 256 = one per CU (384 = one and a half rounds is 10 % slower, 512 equal
// within the box-to-box spread).
inline WgradList wgrad_list_ls_finish(int64_t n_tiles) {
  WgradList w(n_tiles);
  w.xemb_dy0_dy5(256 * 36 / 74, 1);
  w.zd_dy10m(256 * 28 / 74);
  w.h10_dy11(256 * 10 / 74);
  return w;
}
// lnrf_refnerf_trunk_bwd: the pipeline does Dense_1..8, this is the rest of the trunk
inline WgradList wgrad_list_ref_trunk(int64_t n_tiles) {
  WgradList w(n_tiles);
  w.xemb_dy0_dy5(256, 1);
  return w;
}
// lnrf_refnerf_normal_bwd: the kernels of Dense_0..8 (the normal pass has no bias term); 256 workgroups = one per CU
// (two rounds of 512 cost twice the partial-sum traffic for the same streaming rate)
inline WgradList wgrad_list_ref_normal(int64_t n_tiles) {
  WgradList w(n_tiles);
  for (int l = 1; l <= 8; ++l) w.hidden(28, l, 0);
  w.xemb_dy0_dy5(32, 0);
  return w;
}
// lnrf_refnerf_dir_bwd: Dense_9 = [input fragments]^T dy9 (273 x 128 + bias), Dense_10 = relu(Dense_9)^T dy10
// (128 x 3 + bias); 256 workgroups = one per CU
inline WgradList wgrad_list_ref_dir(int64_t n_tiles) {
  WgradList w(n_tiles);
  w.explicit_at(200, WG_DIR9, kDirSaveXin, kDirGradDy9, kDirHidden, kDirIn, kDirW9, kDirB9);
  w.explicit_at(56, WG_H128_DY3, kDirSaveH, kDirGradDy10, 3, kDirHidden, kDirW10, kDirB10);
  return w;
}

}  // namespace lnrf
