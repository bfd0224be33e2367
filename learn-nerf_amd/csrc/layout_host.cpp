// layout_host.cpp — host build of the index maps of the fused NeRF kernels (nerf_layout.h) and of the
// positional-encoding sincos (fast_math.h), so that tests/test_nerf_layout.py can run the exact packing /
// fragment logic on the CPU (no GPU needed) with an MFMA emulator; and of the weight-gradient problem lists and their
// gradient-vector addressing (nerf_wgrad.h); and of the tables and pack walks of the fused InstantNGPModel MLP (ngp_layout.h);
// and of the dispatch plan and tile map of the generic dense GEMM (dense_plan.h, tests/test_dense_plan.py); and of the
// cell geometry, launch plans and scratch layout of the hash grid (hashgrid_plan.h, tests/test_hashgrid_plan.py).
#include <stdint.h>
#include <string.h>

#include "dense_plan.h"
#include "fast_math.h"
#include "hashgrid_plan.h"
#include "nerf_wgrad.h"
#include "ngp_layout.h"

using namespace lnrf;

// ---- weight-gradient problem lists (nerf_wgrad.h).  which: 0 split backward, 1 layer-stationary finish phase,
// 2 Ref-NeRF trunk, 3 Ref-NeRF normal backward, 4 Ref-NeRF directional block
static WgradList wgrad_list_of(int which, int64_t n_tiles) {
  return which == 0 ? wgrad_list_split(n_tiles) : which == 1 ? wgrad_list_ls_finish(n_tiles)
       : which == 2 ? wgrad_list_ref_trunk(n_tiles) : which == 3 ? wgrad_list_ref_normal(n_tiles)
                                                                 : wgrad_list_ref_dir(n_tiles);
}
// Walks what the fold of the list's launch walks (problem, wave, accumulator tile, lane, register and bias sum) and adds 1
// to count[i] for every gradient-vector entry i it would add to; returns how many of them fall outside [0, n).
template <int NXF, int NYF, int WI, int WO>
static int64_t wgrad_count_owners(const WgradProblem& pb, int32_t* count, int64_t n) {
  int64_t outside = 0;
  int64_t i;
  auto hit = [&](bool owned) {
    if (!owned) return;
    if (i >= 0 && i < n) ++count[i];
    else ++outside;
  };
  for (int w = 0; w < kWaves; ++w)
    for (int j = 0; j < kWgradWaveTiles<NXF, NYF, WI, WO>; ++j) {
      const WgradTile tile = wgrad_tile<NXF, NYF, WI, WO>(w, j);
      if (!tile.real) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const int colr = lane & 31, hh = lane >> 5;
        const WgradOwner<NerfWgradEpi, WgradProblem> own(pb, tile.ot, colr);
        if (tile.bias && pb.do_bias) hit(own.bias(hh, i));
        for (int qq = 0; qq < 16; ++qq) hit(own.weight(pb, tile.it, hh, qq, i));
      }
    }
  return outside;
}

// What the end of ngp_mlp_kernel<NE, true> stores for problem P of kNgpWgrad (its `flush`: wave w4 of the layer's half, lane
// (colr, hh), bias sum and accumulator register qq): adds 1 to count[part * n + i] for every float i of row (workgroup,
// part) of the partial-sum buffer it writes; returns how many fall outside [0, n).
// KEEP IN STEP with `flush` in ngp_mlp.hip: this is a copy of its arithmetic (the table, the argument builder and
// NgpWgradEpi are shared); behind a shared function the persistent backward no longer compiles to the same code.
template <int P>
static int64_t ngp_count_owners(const NgpWgradProblem& pb, int64_t dense_off, int32_t* count, int64_t n) {
  constexpr int NO = kNgpWgrad[P].nyf / 2, NT = ngp_wgrad_tiles(P);
  int64_t outside = 0;
  auto hit = [&](int part, int64_t i) {
    if (i >= 0 && i < n) ++count[part * n + i];
    else ++outside;
  };
  for (int w4 = 0; w4 < 4; ++w4)
    for (int lane = 0; lane < 64; ++lane) {
      const int colr = lane & 31, hh = lane >> 5;
      const int tile_id = w4 % NT, part = w4 / NT;
      const int it = tile_id / NO, ot = tile_id % NO;
      int out_idx = -1, out_dim = 1;
      int64_t w_off = 0, b_off = 0;
      NgpWgradEpi::cols(pb, ot, colr, out_idx, out_dim, w_off, b_off);
      w_off -= dense_off;
      b_off -= dense_off;
      if (it == 0 && hh == 0 && out_idx >= 0) hit(part, b_off + out_idx);
      for (int qq = 0; qq < 16; ++qq) {
        const int r = ngp_acc_row(qq, hh);
        const int f = 2 * it + (r >> 4);
        const int in_idx = NgpWgradEpi::row(pb, f, r & 15);
        if (out_idx >= 0 && in_idx >= 0) hit(part, w_off + (int64_t)in_idx * out_dim + out_idx);
      }
    }
  return outside;
}
static bool ngp_enc_dim_ok(int enc_dim) { return enc_dim >= 1 && enc_dim <= 32; }
static HashGridDesc hashgrid_desc_of(const void* desc) {
  HashGridDesc d;
  memcpy(&d, desc, sizeof(d));
  return d;
}

extern "C" {
int lnrf_host_fwd_frags(void) { return kFwdFrags; }
int lnrf_host_bwd_frags(void) { return kBwdFrags; }
int lnrf_host_bias_floats(void) { return kBiasFloats; }
int lnrf_host_fwd_used(void) { return kFwdUsed; }
int lnrf_host_fwd_seq(int c) { return fwd_seq(c); }
int lnrf_host_fwd3_frags(void) { return kFwd3Frags; }
int lnrf_host_fwd3_used(void) { return kFwd3Used; }
int lnrf_host_fwd3_seq(int c) { return fwd3_seq(c); }
int lnrf_host_fwd3_base(int s) { return fwd3_base(s); }
int lnrf_host_bwd_seq(int c) { return bwd_seq(c); }
int lnrf_host_fwd_layer_info(int s, int what) {
  return what == 0 ? fwd_nk(s) : what == 1 ? fwd_no(s) : what == 2 ? fwd_base(s) : what == 3 ? fwd_bias_base(s)
                                                                                             : fwd_cons_base(s);
}
int lnrf_host_bwd_layer_info(int t, int what) {
  return what == 0 ? bwd_nk(t) : what == 1 ? bwd_no(t) : what == 2 ? bwd_base(t) : bwd_dense(t);
}
// parameter index (or -1) feeding element j of lane `lane` of stream fragment g: the pack walks of nerf_layout.h
int lnrf_host_fwd_weight_index(int g, int lane, int j) { return fwd_stream_index(g, lane, j, false); }
int lnrf_host_bwd_weight_index(int g, int lane, int j) { return bwd_stream_index(g, lane, j, false); }
int lnrf_host_fwd_bias_index(int i) { return bias_block_index(i, false); }
int lnrf_host_nrm_frags(void) { return kNrmFrags; }
int lnrf_host_nrm_weight_index(int g, int lane, int j) { return nrm_stream_index(g, lane, j); }
// The index array of a whole stream, out[(g * 64 + lane) * 8 + j] (bias blocks: out[i]); returns its length, -1 for an
// unknown stream.  stream 0 forward, 1 transposed, 2 split forward, 3 bias block (ref != 0: RefNERFModel's trunk-only
// form of these four), 4 normal pass, 5 / 6 / 7 directional forward / transposed / bias block.  out == NULL: length only.
int64_t lnrf_host_stream_indices(int stream, int ref, int32_t* out) {
  const int frags[8] = {kFwdFrags, kBwdFrags, kFwd3Frags, 0, kNrmFrags, kDirFwdFrags, kDirBwdFrags, 0};
  if (stream < 0 || stream > 7) return -1;
  if (stream == 3 || stream == 7) {
    const int n = stream == 3 ? kBiasFloats : kDirBiasFloats;
    for (int i = 0; out && i < n; ++i) out[i] = stream == 3 ? bias_block_index(i, ref != 0) : dir_bias_index(i);
    return n;
  }
  const int64_t n = (int64_t)frags[stream] * 512;
  for (int64_t e = 0; out && e < n; ++e) {
    const int g = (int)(e >> 9), lane = (int)((e >> 3) & 63), j = (int)(e & 7);
    out[e] = stream == 0 ? fwd_stream_index(g, lane, j, ref != 0) : stream == 1 ? bwd_stream_index(g, lane, j, ref != 0)
           : stream == 2 ? fwd3_stream_index(g, lane, j, ref != 0) : stream == 4 ? nrm_stream_index(g, lane, j)
           : stream == 5 ? dir_fwd_weight_index(g, lane, j) : dir_bwd_weight_index(g, lane, j);
  }
  return n;
}
// byte offsets of the regions of the packed blobs.  what 0..3 NeRFModel: forward, transposed, bias, size | 4, 5 its split
// blob: bias, size | 6..10 RefNERFModel behind the NeRFModel regions: normal pass, directional forward / transposed / bias,
// size | 11..16 its split blob: forward, bias, normal pass, directional forward, directional bias, size
int64_t lnrf_host_pack_offset(int what) {
  const int64_t v[17] = {kPackFwdOff, kPackBwdOff, kPackBiasOff, kPackBytes, kPack3BiasOff, kPack3Bytes,
                         kRefPackNrmOff, kRefPackDirFwdOff, kRefPackDirBwdOff, kRefPackDirBiasOff, kRefPackBytes,
                         kRef3FwdOff, kRef3BiasOff, kRef3NrmOff, kRef3DirOff, kRef3DirBiasOff, kRef3Bytes};
  return what >= 0 && what < 17 ? v[what] : -1;
}
int lnrf_host_xemb_feat(int ks, int h, int j) { return xemb_feat(ks, h, j); }
// slot orders of the save / gradient-dump tiles: what 0 x_emb, 1 h_l (arg = l), 2 z, 3 d_emb, 4 h10, 5 masks, 6 slots per tile
int lnrf_host_save_slot(int what, int arg) {
  return what == 0 ? kSaveXin : what == 1 ? kSaveH + 16 * arg : what == 2 ? kSaveZ : what == 3 ? kSaveDin
       : what == 4 ? kSaveH10 : what == 5 ? kSaveMask : kSaveSlots;
}
// what 0 dy11, 1 dy10m, 2 dy_l (arg = l), 3 slots per tile
int lnrf_host_grad_slot(int what, int arg) {
  return what == 0 ? kGradDy11 : what == 1 ? kGradDy10m : what == 2 ? grad_dy_slot(arg) : kGradSlots;
}
// Ref-NeRF directional block: what 0 input fragments, 1 relu(Dense_9), 2 its mask, 3 slots per tile of the save | 4 dy10,
// 5 dy9, 6 slots per tile of the gradient dump; -1 for anything else
int lnrf_host_dir_slot(int what) {
  const int v[7] = {kDirSaveXin, kDirSaveH, kDirSaveMask, kDirSaveSlots, kDirGradDy10, kDirGradDy9, kDirGradSlots};
  return what >= 0 && what < 7 ? v[what] : -1;
}
int lnrf_host_demb_feat(int ks, int h, int j) { return demb_feat(ks, h, j); }
int lnrf_host_hidden_feat(int ks, int h, int j) { return hidden_feat(ks, h, j); }
// what 0 bytes per fragment, 1 evaluations per tile, 2 tiles per workgroup (dumps are padded to whole workgroups)
int lnrf_host_dump_info(int what) { return what == 0 ? kFragBytes : what == 1 ? kTileCols : kWaves; }
// ReLU-mask slot (kSaveMask): bit of a lane's 128 that belongs to element j of fragment ks of the masked tensor, i.e. to
// accumulator register q = 8 (ks & 1) + j of out tile o = ks >> 1: bit 16 o + q; the lane's uint4 sits at lane * 16
int lnrf_host_mask_bit(int ks, int j) { return 16 * (ks >> 1) + 8 * (ks & 1) + j; }
int lnrf_host_dump_lane_off(int slot, int c, int hh) { return dump_lane_off(slot, c, hh); }
void lnrf_host_sincos_pe(float r, float* s, float* c) { lnrf::sincos_pe(r, s, c); }

// ---- weight-gradient problem lists: `which` as for wgrad_list_of ----
// what 0 slab capacity of a launch (workgroups), 1 / 2 accumulator tiles / bias rows a slab has room for per wave,
// 3 parameters of a NeRFModel, 4..7 kDirW9, kDirB9, kDirW10, kDirB10
int lnrf_host_wgrad_const(int what) {
  const int v[8] = {kWgradMaxBlocks, kSlabMaxTiles, kSlabMaxTO, kParamCount, kDirW9, kDirB9, kDirW10, kDirB10};
  return v[what];
}
// out[6 i ..]: first_block, n_blocks, TI * TO, TO, do_bias, 1 if nerf_ls_fold_kernel carries the shape; returns the
// number of problems, -1 for a shape outside the table
int lnrf_host_wgrad_list(int which, int64_t n_tiles, int32_t* out) {
  const WgradList list = wgrad_list_of(which, n_tiles);
  for (int i = 0; i < list.args.n_problems; ++i) {
    const WgradProblem& pb = list.args.p[i];
    int32_t* o = out + 6 * i;
    o[0] = pb.first_block; o[1] = pb.n_blocks; o[4] = pb.do_bias; o[5] = 0;
    switch (pb.shape) {
#define X(name, id, NXF, NYF, WI, WO, SPI) case name: o[2] = WgShape<name>::TI * WgShape<name>::TO; o[3] = WgShape<name>::TO; break;
      LNRF_WGRAD_SHAPES(X, X)
#undef X
      default: return -1;
    }
    switch (pb.shape) {
#define X(name) case name:
      LNRF_WGRAD_LS_SHAPES(X, X) o[5] = 1; break;
#undef X
      default: break;
    }
  }
  return list.args.n_problems;
}
// ---- fused InstantNGPModel MLP (ngp_layout.h); parameter indices are relative to the first Dense parameter ----
// The index array of a stream for enc_dim = L*F encoding features: stream 0 forward, 1 transposed (both over the 48
// fragments of the blob, out[(g * 64 + lane) * 8 + j], -1 outside their own fragments), 2 bias block (out[i]).  Returns
// its length, -1 for an unknown stream or enc_dim.  out == NULL: length only.
int64_t lnrf_host_ngp_stream_indices(int stream, int enc_dim, int32_t* out) {
  if (stream < 0 || stream > 2 || !ngp_enc_dim_ok(enc_dim)) return -1;
  const NgpOffsets off = ngp_offsets(enc_dim, 0);
  const int ne = ngp_ne(enc_dim);
  const int64_t n = stream == 2 ? kNgpBiasFloats : (int64_t)kNgpStreamFrags * 512;
  for (int64_t e = 0; out && e < n; ++e) {
    const int g = (int)(e >> 9), lane = (int)((e >> 3) & 63), j = (int)(e & 7);
    out[e] = (int32_t)(stream == 0 ? ngp_fwd_stream_index(g, lane, j, off, enc_dim, ne)
                     : stream == 1 ? ngp_bwd_stream_index(g, lane, j, off, enc_dim, ne) : ngp_bias_index((int)e, off));
  }
  return n;
}
// what 0 bias block of the blob, 1 its size, 2 bias block of the split blob, 3 its size (bytes), 4 / 5 fragments of the
// stream / fragment pairs of the split stream, 6 k-parts a partial-sum row is kept for
int64_t lnrf_host_ngp_pack_offset(int what) {
  const int64_t v[7] = {kNgpPackBiasOff, kNgpPackBytes, kNgpSplitBiasOff, kNgpSplitBytes, kNgpStreamFrags,
                        kNgpSplitMaxFrags / 2, kNgpMaxParts};
  return what >= 0 && what < 7 ? v[what] : -1;
}
// The weight-gradient stores of one workgroup of the persistent backward, through the production table, argument
// builder and addressing, with the Dense block at a non-zero dense_offset: count[part * n + i] (kNgpMaxParts planes of n)
// += 1 per store to float i of the row of k-part `part`; returns the stores outside [0, n), -1 for a bad enc_dim.
int64_t lnrf_host_ngp_wgrad_owners(int enc_dim, int32_t* count, int64_t n) {
  if (!ngp_enc_dim_ok(enc_dim)) return -1;
  const int64_t dense_off = 1001;
  const NgpWgradArgs a = ngp_wgrad_args(ngp_offsets(enc_dim, dense_off), enc_dim);
  return ngp_count_owners<0>(a.p[0], dense_off, count, n) + ngp_count_owners<1>(a.p[1], dense_off, count, n) +
         ngp_count_owners<2>(a.p[2], dense_off, count, n) + ngp_count_owners<3>(a.p[3], dense_off, count, n) +
         ngp_count_owners<4>(a.p[4], dense_off, count, n);
}
// out[4 i ..]: Dense layer, float range [lo, hi) relative to dense_offset and k-parts of problem i of the reduce launch;
// returns the Dense parameter count
int lnrf_host_ngp_parts_plan(int enc_dim, int32_t* out) {
  if (!ngp_enc_dim_ok(enc_dim)) return -1;
  const NgpPartsPlan pl = ngp_parts_plan(ngp_offsets(enc_dim, 1001), 1001);
  for (int i = 0; i < kNgpLayers; ++i) {
    int32_t* o = out + 4 * i;
    o[0] = kNgpWgrad[i].layer; o[1] = pl.lo[i]; o[2] = pl.hi[i]; o[3] = pl.parts[i];
  }
  return ngp_dense_params(enc_dim);
}
// ---- generic dense GEMM (dense_plan.h): the plan launch_gemm launches from.  out[0..14] = launch, big, bf16, a_fast_r,
// b_fast_r, b_aligned, kc, nsplit, lda, ldb, r_per_split, grid x / y / z, and GemmPlan::splits
void lnrf_host_gemm_plan(int64_t sa_i, int64_t sa_r, int64_t sb_r, int64_t sb_j, int64_t I, int32_t J, int64_t R,
                         uint32_t a_low, uint32_t b_low, int32_t bf16, int32_t mode, int32_t splits, int64_t* out) {
  const GemmPlan p = gemm_plan(sa_i, sa_r, sb_r, sb_j, I, J, R, a_low, b_low, bf16 != 0, mode, splits);
  const int64_t v[15] = {p.launch, p.big, p.bf16, p.a_fast_r, p.b_fast_r, p.b_aligned, p.kc, p.nsplit, p.lda, p.ldb,
                         p.r_per_split, p.gx, p.gy, p.gz, p.splits};
  for (int i = 0; i < 15; ++i) out[i] = v[i];
}
// tiles of blocks block0 .. block0 + count - 1 of gemm_big_kernel's grid for an I x J output: out[2 e] = row tile,
// out[2 e + 1] = column tile of block block0 + e
void lnrf_host_gemm_tile(int64_t I, int32_t J, uint32_t block0, int64_t count, int64_t* out) {
  for (int64_t e = 0; e < count; ++e) {
    const GemmTile t = gemm_big_tile(block0 + (uint32_t)e, (I + BI - 1) / BI, (J + BJ - 1) / BJ);
    out[2 * e] = t.it;
    out[2 * e + 1] = t.jt;
  }
}
// the scratch sizes behind lnrf_dense_bwd_weight_scratch_bytes / lnrf_gemm_f32_det_scratch_bytes
int64_t lnrf_host_dense_bwd_weight_scratch_bytes(int64_t m, int32_t k, int32_t n) { return dense_wgrad_scratch_bytes(m, k, n); }
int64_t lnrf_host_gemm_det_scratch_bytes(int64_t I, int32_t J, int64_t R) { return gemm_det_scratch_bytes(I, J, R); }
// ---- hash grid (hashgrid_plan.h); desc is a lnrf_hashgrid_desc ----
// the 8 corners of point x at `level` in the kernels' order (xo outermost): table entry, weight, d weight / d x
void lnrf_host_hashgrid_corners(const void* desc, int32_t level, const float* x, uint32_t* idx, float* w, float* dw) {
  const HashGridDesc d = hashgrid_desc_of(desc);
  const int G = d.grid_size[level];
  const Corner k = locate(x, d, G);
  for (int c = 0; c < 8; ++c) {
    const int xo = c >> 2, yo = (c >> 1) & 1, zo = c & 1;
    idx[c] = entry_index(k.base[0] + xo, k.base[1] + yo, k.base[2] + zo, G, d.table_size[level], d.hashed[level]);
    w[c] = corner_weight(k, xo, yo, zo);
    corner_weight_grad(k, xo, yo, zo, dw + 3 * c);
  }
}
// XCD plan of hashgrid_fwd_xcd_kernel for `n` levels and m samples.  Returns the grid (0: inconsistent plan);
// plan[0..8] = first_seg, then n_segs x (level, first chunk, chunks) from plan[9]; work[2 b], work[2 b + 1] = level (-1:
// nothing) and first sample of workgroup b.  plan / work == NULL: not written.
int64_t lnrf_host_hashgrid_xcd_plan(const void* desc, const int32_t* levels, int32_t n, int64_t m, int32_t* plan,
                                    int64_t* work) {
  const HashGridDesc d = hashgrid_desc_of(desc);
  LevelList ll;
  ll.n = n;
  for (int i = 0; i < n; ++i) ll.level[i] = levels[i];
  unsigned grid = 0;
  const XcdPlan p = make_xcd_plan(d, ll, m, &grid);
  for (int x = 0; plan && x <= kXcds; ++x) plan[x] = p.first_seg[x];
  for (int s = 0; plan && s < p.n_segs; ++s) {
    plan[9 + 3 * s] = p.seg_level[s]; plan[10 + 3 * s] = p.seg_chunk0[s]; plan[11 + 3 * s] = p.seg_chunks[s];
  }
  for (unsigned b = 0; work && b < grid; ++b) {
    const XcdWork w = xcd_work(p, b);
    work[2 * b] = w.seg < 0 ? -1 : xcd_level(p, w);
    work[2 * b + 1] = w.seg < 0 ? 0 : xcd_first_sample(p, w);
  }
  return grid;
}
// Bucket plan of the scatter for m samples.  Returns the bucketed levels n; levels[7 i ..] = level, slices, split, first
// reduce workgroup, first tuple, first cursor, capacity; scratch[0..4] = cursor bytes, byte offsets of the level maxima
// and of the tuples, total bytes, reduce workgroups.
int32_t lnrf_host_hashgrid_bucket_plan(const void* desc, int64_t m, int64_t* levels, int64_t* scratch) {
  const BucketPlan p = make_plan(hashgrid_desc_of(desc), m);
  for (int i = 0; i < p.n; ++i) {
    const int64_t v[7] = {p.level[i], p.slices[i], p.split[i], p.wg_off[i], p.tuple_off[i], p.cursor_off[i], p.cap[i]};
    for (int j = 0; j < 7; ++j) levels[7 * i + j] = v[j];
  }
  const BucketScratch s = bucket_scratch(p);
  scratch[0] = s.cursor_bytes; scratch[1] = s.level_max_off; scratch[2] = s.tuple_off; scratch[3] = s.total;
  scratch[4] = p.wg_off[p.n];
  return p.n;
}
// reduce workgroups block0 .. block0 + count - 1 of that plan, each for a bucket holding `tuples` tuples:
// out[6 e ..] = entry of the plan, its level, bucket, part, first and one-past-last tuple the workgroup reads
void lnrf_host_hashgrid_reduce_work(const void* desc, int64_t m, int32_t block0, int64_t count, int64_t tuples,
                                    int64_t* out) {
  const BucketPlan p = make_plan(hashgrid_desc_of(desc), m);
  for (int64_t e = 0; e < count; ++e) {
    const ReduceWork w = reduce_work(p, block0 + (int)e);
    const TupleRange r = reduce_range(p, w, tuples);
    const int64_t v[6] = {w.li, w.level, w.bucket, w.part, r.lo, r.hi};
    for (int j = 0; j < 6; ++j) out[6 * e + j] = v[j];
  }
}
int64_t lnrf_host_wgrad_owners(int which, int64_t n_tiles, int32_t* count, int64_t n) {
  const WgradList list = wgrad_list_of(which, n_tiles);
  int64_t outside = 0;
  for (int i = 0; i < list.args.n_problems; ++i) {
    const WgradProblem& pb = list.args.p[i];
    switch (pb.shape) {
#define X(name, id, NXF, NYF, WI, WO, SPI) case name: outside += wgrad_count_owners<NXF, NYF, WI, WO>(pb, count, n); break;
      LNRF_WGRAD_SHAPES(X, X)
#undef X
    }
  }
  return outside;
}
}
