// layout_host.cpp — host build of the index maps of the fused NeRF kernels (nerf_layout.h) and of the
// positional-encoding sincos (fast_math.h), so that tests/test_nerf_layout.py can run the exact packing /
// fragment logic on the CPU (no GPU needed) with an MFMA emulator; and of the weight-gradient problem lists and their
// gradient-vector addressing (nerf_wgrad.h).
#include <stdint.h>

#include "fast_math.h"
#include "nerf_wgrad.h"

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
