// ngp_layout.h — everything about the fused InstantNGPModel MLP (ngp_mlp.hip) that is plain integer arithmetic: the
// per-layer tables, the pack walks of its weight streams, and the weight-gradient table of the persistent backward with
// its gradient-vector addressing.  No HIP types: device code includes it, and layout_host.cpp builds it for the CPU so
// that tests/test_ngp_layout.py can check that every weight is packed once and every gradient entry has one owner.
// The network is drawn at the top of ngp_mlp.hip; the vocabulary (fragment, k-step, tile, k slot <-> feature =
// hidden_feat) is that of nerf_layout.h.
#pragma once
#include "nerf_layout.h"

namespace lnrf {
using namespace nl;

constexpr int kNgpLayers = 5;
constexpr int kNgpHidden = 64, kNgpDensityDim = 16, kNgpDembDim = 24;
constexpr int kNgpStreamFrags = 48;  // 3 ring stages: forward (at most 26), transposed (20), padding
constexpr int kNgpBiasFloats = 256;
constexpr int kNgpPackBiasOff = kNgpStreamFrags * kFragBytes;
constexpr int kNgpPackBytes = kNgpPackBiasOff + kNgpBiasFloats * 4;
// split-precision blob: [hi, lo] per forward fragment, then the same fp32 bias block
constexpr int kNgpSplitMaxFrags = 2 * 26;
constexpr int kNgpSplitBiasOff = kNgpSplitMaxFrags * kFragBytes;
constexpr int kNgpSplitBytes = kNgpSplitBiasOff + kNgpBiasFloats * 4;

// ---- per-layer tables ------------------------------------------------------------------------------------------------
NL_HD constexpr int ngp_ne(int lf) { return lf <= 16 ? 1 : 2; }  // k-steps of encoding: the kernels exist for 1 and 2
// forward layer l with ne k-steps of encoding: k-steps, 32-row out tiles, first fragment
// (consumption order == stream order), first float of the bias block
NL_HD constexpr int ngp_fwd_nk(int l, int ne) { return l == 0 ? ne : (l == 2 ? 3 : 4); }
NL_HD constexpr int ngp_fwd_no(int l) { return (l == 1 || l == 4) ? 1 : 2; }
NL_HD constexpr int ngp_fwd_base(int l, int ne) {
  int b = 0;
  for (int i = 0; i < l; ++i) b += ngp_fwd_nk(i, ne) * ngp_fwd_no(i);
  return b;
}
NL_HD constexpr int ngp_fwd_count(int ne) { return ngp_fwd_base(kNgpLayers, ne); }
NL_HD constexpr int ngp_bias_base(int l) {
  int b = 0;
  for (int i = 0; i < l; ++i) b += 32 * ngp_fwd_no(i);
  return b;
}
NL_HD constexpr int ngp_out_dim(int l) { return l == 1 ? kNgpDensityDim : (l == 4 ? 3 : kNgpHidden); }
// backward step t applies Dense_{4-t}^T; its fragments follow the forward ones
NL_HD constexpr int ngp_bwd_nk(int t) { return (t == 0 || t == 3) ? 1 : 4; }
NL_HD constexpr int ngp_bwd_no(int t) { return (t == 2 || t == 4) ? 1 : 2; }
NL_HD constexpr int ngp_bwd_base(int t, int ne) {
  int b = ngp_fwd_count(ne);
  for (int i = 0; i < t; ++i) b += ngp_bwd_nk(i) * ngp_bwd_no(i);
  return b;
}
NL_HD constexpr int ngp_total_count(int ne) { return ngp_bwd_base(kNgpLayers, ne); }
static_assert(ngp_fwd_count(2) == 26 && ngp_total_count(2) == 46 && ngp_total_count(2) <= kNgpStreamFrags &&
                  ngp_bias_base(kNgpLayers) == kNgpBiasFloats, "stream and bias block sizes");

// ---- Flax parameter vector: Dense_l.kernel[in, out] row-major, then Dense_l.bias, from dense_offset --------------------
struct NgpOffsets { int64_t w[kNgpLayers], b[kNgpLayers]; };
NL_HD constexpr int ngp_in_dim(int l, int lf) {
  return l == 0 ? lf : (l == 2 ? kNgpDembDim + kNgpDensityDim : kNgpHidden);
}
NL_HD constexpr NgpOffsets ngp_offsets(int lf, int64_t dense_offset) {
  NgpOffsets o{};
  for (int l = 0; l < kNgpLayers; ++l) {
    o.w[l] = dense_offset;
    o.b[l] = o.w[l] + (int64_t)ngp_in_dim(l, lf) * ngp_out_dim(l);
    dense_offset = o.b[l] + ngp_out_dim(l);
  }
  return o;
}
NL_HD constexpr int ngp_dense_params(int lf) { return (int)ngp_offsets(lf, 0).b[kNgpLayers - 1] + ngp_out_dim(kNgpLayers - 1); }

// ---- input composition ---------------------------------------------------------------------------------------------------
// Fragment f (one k-step, 16 k slots in hidden_feat order) of the input of Dense_l feeds kernel rows [row0, row0 + rows).
// Dense_0: the lf encoding features.  Dense_2: d_emb (24 features in fragments 0 and 1), then `out` in fragment 2.
struct NgpXFrag { int row0, rows; };
NL_HD constexpr NgpXFrag ngp_xfrag(int l, int f, int lf) {
  if (l == 2 && f >= 2) return NgpXFrag{f == 2 ? kNgpDembDim : 0, f == 2 ? kNgpDensityDim : 0};
  const int left = (l == 0 ? lf : (l == 2 ? kNgpDembDim : kNgpHidden)) - 16 * f;
  return NgpXFrag{16 * f, left < 0 ? 0 : (left > 16 ? 16 : left)};
}

// ---- pack walks -----------------------------------------------------------------------------------------------------------
// Parameter feeding element (lane, j) of fragment g of the 48-fragment stream, or float i of the bias block; -1 = zero.
// The pack kernels and the host library call these and nothing else.  The forward walk answers -1 outside
// [0, ngp_fwd_count), the transposed one outside [ngp_fwd_count, ngp_total_count).
NL_HD constexpr int64_t ngp_fwd_stream_index(int g, int lane, int j, const NgpOffsets& off, int lf, int ne) {
  if (g >= ngp_fwd_count(ne)) return -1;
  const int r = lane & 31, hh = lane >> 5;
  int l = 0;
  for (int i = 1; i < kNgpLayers; ++i)
    if (g >= ngp_fwd_base(i, ne)) l = i;
  const int loc = g - ngp_fwd_base(l, ne), nk = ngp_fwd_nk(l, ne);
  const int o = loc / nk, ks = loc % nk;
  const int row = 32 * o + r, od = ngp_out_dim(l);  // A[row = output feature][k slot = input feature]
  const NgpXFrag x = ngp_xfrag(l, ks, lf);
  const int r16 = hidden_feat(0, hh, j);
  return (row < od && r16 < x.rows) ? off.w[l] + (int64_t)(x.row0 + r16) * od + row : -1;
}
// A[row = input feature of Dense_l][k slot = output feature of Dense_l], l = 4 - t.  Dense_2^T is restricted to the 16 rows
// fed by `out` (d_emb has no parameters upstream).
NL_HD constexpr int64_t ngp_bwd_stream_index(int g, int lane, int j, const NgpOffsets& off, int lf, int ne) {
  if (g < ngp_fwd_count(ne) || g >= ngp_total_count(ne)) return -1;
  const int r = lane & 31, hh = lane >> 5;
  int t = 0;
  for (int i = 1; i < kNgpLayers; ++i)
    if (g >= ngp_bwd_base(i, ne)) t = i;
  const int loc = g - ngp_bwd_base(t, ne), nk = ngp_bwd_nk(t);
  const int o = loc / nk, ks = loc % nk;
  const int l = 4 - t, od = ngp_out_dim(l);
  int row = 32 * o + r;
  if (l == 2) row = r < kNgpDensityDim ? kNgpDembDim + r : -1;
  else if (row >= ngp_in_dim(l, lf)) row = -1;
  const int k = hidden_feat(ks, hh, j);
  return (row >= 0 && k < od) ? off.w[l] + (int64_t)row * od + k : -1;
}
NL_HD constexpr int64_t ngp_bias_index(int i, const NgpOffsets& off) {
  int l = 0;
  for (int k = 1; k < kNgpLayers; ++k)
    if (i >= ngp_bias_base(k)) l = k;
  const int loc = i - ngp_bias_base(l);
  return loc < ngp_out_dim(l) ? off.b[l] + loc : -1;
}

// ---- weight gradients of the persistent backward -------------------------------------------------------------------------
// The 8 waves of a workgroup stage the X and dy fragments of a layer (nxf + nyf of them per wave), then the four waves of
// one half of the workgroup accumulate the layer's dW in accumulator slot `slot`.  A layer with NT = (nxf / 2) (nyf / 2)
// < 4 tiles of 32 x 32 is dealt to its four waves as NT tiles x 4 / NT k-parts of the group's 256 evaluations; every
// k-part has its own row in the partial-sum buffer.  A wave carries at most three tiles (five would not fit next to the
// chain's fragments).  The row order is the order of the problems in the kernel argument and of the reduce launch.
struct NgpWgradRow { int layer, slot, half, nxf, nyf; };
constexpr NgpWgradRow kNgpWgrad[kNgpLayers] = {
    {3, 0, 0, 4, 4}, {2, 0, 1, 4, 4}, {1, 1, 1, 4, 2}, {4, 1, 0, 4, 2}, {0, 2, 0, 2, 4}};
constexpr int kNgpWSlots = 3, kNgpMaxParts = 4;
constexpr int ngp_wgrad_problem(int layer) {  // row of Dense_layer
  int p = 0;
  for (int i = 1; i < kNgpLayers; ++i)
    if (kNgpWgrad[i].layer == layer) p = i;
  return p;
}
constexpr int ngp_wgrad_tiles(int p) { return (kNgpWgrad[p].nxf / 2) * (kNgpWgrad[p].nyf / 2); }
constexpr int ngp_wgrad_kparts(int p) { return 4 / ngp_wgrad_tiles(p); }
constexpr bool ngp_wgrad_table_ok() {  // every layer once, fragment counts of the layer tables, one slot per (half, layer)
  for (int p = 0; p < kNgpLayers; ++p) {
    const NgpWgradRow a = kNgpWgrad[p];
    bool ok = kNgpWgrad[ngp_wgrad_problem(p)].layer == p && a.slot < kNgpWSlots && 4 % ngp_wgrad_tiles(p) == 0 &&
              a.nyf == 2 * ngp_fwd_no(a.layer) && a.nxf == (ngp_fwd_nk(a.layer, 2) + 1) / 2 * 2;
    for (int q = 0; q < p; ++q) ok = ok && (kNgpWgrad[q].half != a.half || kNgpWgrad[q].slot != a.slot);
    if (!ok) return false;
  }
  return true;
}
static_assert(ngp_wgrad_table_ok(), "kNgpWgrad");

struct NgpWgradProblem {
  int out_dim;                      // columns of the Flax kernel (= valid dy features)
  unsigned w_lo, w_hi, b_lo, b_hi;  // float offsets of kernel / bias in the gradient vector (64-bit, split)
  int rb0, rb1, rb2, rb3;           // per X fragment: first kernel row ...
  int rv0, rv1, rv2, rv3;  // ... and how many of its 16 features are real (scalars: keeps the struct in SGPRs)
};
struct NgpWgradArgs { NgpWgradProblem p[kNgpLayers]; };
struct NgpPartsPlan { int lo[kNgpLayers], hi[kNgpLayers], parts[kNgpLayers]; };  // [lo, hi) relative to dense_offset
inline NgpWgradArgs ngp_wgrad_args(const NgpOffsets& off, int lf) {
  NgpWgradArgs a;
  for (int i = 0; i < kNgpLayers; ++i) {
    const int l = kNgpWgrad[i].layer;
    const NgpXFrag x0 = ngp_xfrag(l, 0, lf), x1 = ngp_xfrag(l, 1, lf), x2 = ngp_xfrag(l, 2, lf), x3 = ngp_xfrag(l, 3, lf);
    a.p[i] = NgpWgradProblem{ngp_out_dim(l), (unsigned)(off.w[l] & 0xFFFFFFFFll), (unsigned)(off.w[l] >> 32),
                             (unsigned)(off.b[l] & 0xFFFFFFFFll), (unsigned)(off.b[l] >> 32),
                             x0.row0, x1.row0, x2.row0, x3.row0, x0.rows, x1.rows, x2.rows, x3.rows};
  }
  return a;
}
inline NgpPartsPlan ngp_parts_plan(const NgpOffsets& off, int64_t dense_offset) {
  NgpPartsPlan plan;
  for (int i = 0; i < kNgpLayers; ++i) {
    const int l = kNgpWgrad[i].layer;
    plan.lo[i] = (int)(off.w[l] - dense_offset);
    plan.hi[i] = (int)(off.b[l] - dense_offset) + ngp_out_dim(l);
    plan.parts[i] = ngp_wgrad_kparts(i);
  }
  return plan;
}
// row of the 32-row dW tile that accumulator register qq of lane half hh holds: slot r & 15 of X fragment 2 it + (r >> 4)
NL_HD constexpr int ngp_acc_row(int qq, int hh) { return (qq & 3) + 8 * (qq >> 2) + 4 * hh; }
struct NgpWgradEpi {
  static NL_HD void cols(const NgpWgradProblem& pb, int ot, int colr, int& out_idx, int& out_dim, int64_t& w_off,
                         int64_t& b_off) {
    const int idx = 32 * ot + colr;
    out_idx = idx < pb.out_dim ? idx : -1;
    out_dim = pb.out_dim;
    w_off = (int64_t)(((uint64_t)pb.w_hi << 32) | pb.w_lo);
    b_off = (int64_t)(((uint64_t)pb.b_hi << 32) | pb.b_lo);
  }
  static NL_HD int row(const NgpWgradProblem& pb, int f, int r16) {
    const int base = f == 0 ? pb.rb0 : (f == 1 ? pb.rb1 : (f == 2 ? pb.rb2 : pb.rb3));
    const int nv = f == 0 ? pb.rv0 : (f == 1 ? pb.rv1 : (f == 2 ? pb.rv2 : pb.rv3));
    return r16 < nv ? base + r16 : -1;
  }
};

}  // namespace lnrf
