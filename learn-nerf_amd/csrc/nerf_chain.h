// nerf_chain.h — the pieces of the NeRFModel trunk (nerf_layout.h) shared by nerf_mlp.hip, nerf_bwd_ls.hip (layer-stationary
// backward) and refnerf_fused.hip: the positional encoding of x, the trunk layer of the forward / tangent chains, the masked
// step of the input-gradient chains, the input-gradient chain of one 32-evaluation tile and the launch of the
// weight-gradient problems of nerf_wgrad.h.
#pragma once
#include "fused_chain.h"

namespace lnrf {

// Positional encoding (model.py:65-77, fp32) of x into the 4 fragments of x_emb: a lane half holds kXPairs (coordinate,
// frequency) pairs, four per k-step, numbered pg = kXPairs * h + p = kXFreqs * coordinate + frequency over both halves;
// pair p = kXPairs is zero padding (the map of nerf_layout.h xemb_feat).  put(ks_, j, value) receives element j of
// fragment ks_: sin in 2 pp, cos in 2 pp + 1 of pair pp, and stores it as bf16 or as a hi / lo pair.
// The pair arithmetic is spelled out: behind a function shared with xemb_feat the kernels compile to different code.
template <class Put>
__device__ __forceinline__ void x_encode(const float (&px)[3], int h, Put put) {
  static_for<4>([&](auto ks_) {
    constexpr int ks = decltype(ks_)::value;
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int p = 4 * ks + pp;
      float s = 0.0f, co = 0.0f;
      if (p < kXPairs) {
        const int pg = kXPairs * h + p;
        const int cd = pg / kXFreqs, f = pg - kXFreqs * cd;
        const float v = cd == 0 ? px[0] : (cd == 1 ? px[1] : px[2]);
        sincos_pe(v * (float)(1 << f), &s, &co);
      }
      put(ks_, 2 * pp, s);
      put(ks_, 2 * pp + 1, co);
    }
  });
}

// One layer S of the trunk on the forward weight stream: B operand = x_emb for Dense_0, the previous layer's 16
// fragments after that (+ x_emb as k-steps 16..19 of Dense_5, model.py:52).  BIAS: accumulators start from the bias
// (forward) or from zero (tangent chain).  epi(o_, acc) per out tile.
template <int S, bool BIAS, class RING, class Epi>
__device__ __forceinline__ void trunk_layer(RING& ring, int h, const bf16x8 (&xe)[4], const bf16x8 (&in)[16], Epi epi) {
  chain_layer<fwd_cons_base(S), fwd_nk(S), fwd_no(S)>(
      ring,
      [&](auto o_) {
        if constexpr (BIAS) return bias_acc(fwd_bias_base(S) + 32 * decltype(o_)::value, h);
        else return zero_acc();
      },
      [&](auto k_) -> bf16x8 {
        constexpr int ks = decltype(k_)::value;
        if constexpr (S == 0) return xe[ks];
        else if constexpr (ks < 16) return in[ks];
        else return xe[ks - 16];
      },
      epi);
}
// ... in split precision (always with bias)
template <int S, class RING, class Epi>
__device__ __forceinline__ void trunk_layer_split(RING& ring, int h, const bf16x8 (&xe_hi)[4], const bf16x8 (&xe_lo)[4],
                                                  const bf16x8 (&inh)[16], const bf16x8 (&inl)[16], Epi epi) {
  chain_layer_split<fwd_cons_base(S), fwd_nk(S), fwd_no(S)>(
      ring, [&](auto o_) { return bias_acc(fwd_bias_base(S) + 32 * decltype(o_)::value, h); },
      [&](auto k_) -> bf16x8 {
        constexpr int ks = decltype(k_)::value;
        if constexpr (S == 0) return xe_hi[ks];
        else if constexpr (ks < 16) return inh[ks];
        else return xe_hi[ks - 16];
      },
      [&](auto k_) -> bf16x8 {
        constexpr int ks = decltype(k_)::value;
        if constexpr (S == 0) return xe_lo[ks];
        else if constexpr (ks < 16) return inl[ks];
        else return xe_lo[ks - 16];
      },
      epi);
}
// Epilogue of a masked step: out tile o of `acc` times the ReLU mask `mk` -> fragments 2 o, 2 o + 1 of `out`, dumped to
// slots slot0 + 2 o, + 1 of `gd`
template <int O>
__device__ __forceinline__ void masked_out_tile(const f32x16& acc, const uint4& mk, bf16x8 (&out)[16], const DumpAddr& gd,
                                                int slot0) {
  const unsigned mb = mask_word(mk, O);
  out[2 * O] = masked_frag<0>(acc, mb, 16 * (O & 1));
  out[2 * O + 1] = masked_frag<1>(acc, mb, 16 * (O & 1));
  gd.store(slot0 + 2 * O, frag_to_bits(out[2 * O]));
  gd.store(slot0 + 2 * O + 1, frag_to_bits(out[2 * O + 1]));
}
// One hidden step of an input-gradient chain (256 x 256 layer whose fragments start at consumption index C0):
// out = relu'(h_{L-1}) * (W_L^T in), dumped as dy_{L-1} / c_{L-1}
template <int C0, int L, class RING>
__device__ __forceinline__ void hidden_back(RING& ring, bf16x8 (&in)[16], bf16x8 (&out)[16], const uint4& mk,
                                            const DumpAddr& gd) {
  chain_layer<C0, 16, 8>(
      ring, [&](auto) { return zero_acc(); }, [&](auto k_) -> bf16x8 { return in[decltype(k_)::value]; },
      [&](auto o_, const f32x16& acc) { masked_out_tile<decltype(o_)::value>(acc, mk, out, gd, grad_dy_slot(L - 1)); });
}

struct BwdSeq {
  static constexpr int count = kBwdUsed;
  static constexpr int at(int c) { return bwd_seq(c); }
};
constexpr int kBwdStages = kBwdFrags / kStageFrags;  // 70

// Input-gradient chain of the tile owned by this wave (what jax.grad does through model.py:49-60 back to front).
// The pre-activation gradient fragments go to the gradient dump `gd` (layout: fused_chain.h dump_off) with non-temporal
// stores.  `ring` must be freshly constructed; the caller provides the workgroup barrier that separates two uses of the
// weight ring's LDS.
// HEAD_ONLY: stop after dy11, dy10m and dz: the head launch of the layer-stationary backward (nerf_bwd_ls.hip).
template <bool HEAD_ONLY = false, class RING>
__device__ __forceinline__ void bwd_chain_tile(RING& ring, const DumpAddr& gd, const char* __restrict__ save,
                                               int64_t save_tiles, const float* __restrict__ density,
                                               const float* __restrict__ rgb, const float* __restrict__ g_density,
                                               const float* __restrict__ g_rgb, int64_t M, int64_t tile, int lane) {
  const int c = lane & 31, h = lane >> 5;
  const int64_t m = tile * kTileCols + c;
  const bool valid = m < M;

  // head gradients (fp32): d/d(pre-tanh) and d/d(density logit)
  float gy11[3] = {0, 0, 0}, gy9 = 0.0f;
  if (valid && h == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float y = rgb[m * 3 + k];
      gy11[k] = g_rgb[m * 3 + k] * (1.0f - y * y);  // tanh'
    }
    gy9 = g_density[m] * -expm1f(-density[m]);  // softplus' = sigmoid = 1 - exp(-sp), no cancellation
  }
  // ReLU masks of h0..h7 and h10 (written by the forward), 16 bytes per lane and layer
  uint4 relu_mask[9];
#pragma unroll
  for (int i = HEAD_ONLY ? 8 : 0; i < 9; ++i)  // the head launch only applies relu'(h10)
    relu_mask[i] = *mask_at(save, kSaveMask + i, tile, save_tiles, kSaveTileSlots, lane);
  __syncthreads();
  ring.prologue();
  LNRF_TL_STAMP(ring);

  bf16x8 a0[16], a1[16];

  // dy11 fragment: k slot (h=0, j<3) = rgb channel
  bf16x8 dy11 = zero_frag();
  dy11[0] = (__bf16)gy11[0];
  dy11[1] = (__bf16)gy11[1];
  dy11[2] = (__bf16)gy11[2];
  gd.store(kGradDy11, frag_to_bits(dy11));
  gd.store(kGradDy11 + 1, frag_to_bits(zero_frag()));

  // T0: Dense_11^T -> dh10, masked by relu(h10)
  chain_layer<bwd_cons_base(0), bwd_nk(0), bwd_no(0)>(
      ring, [&](auto) { return zero_acc(); }, [&](auto) -> bf16x8 { return dy11; },
      [&](auto o_, const f32x16& acc) {
        masked_out_tile<decltype(o_)::value>(acc, relu_mask[8], a0, gd, kGradDy10m);
      });
  // logit-gradient fragment: slot (h=0, j=0)
  bf16x8 dlogit = zero_frag();
  dlogit[0] = (__bf16)gy9;
  gd.store(kGradDy10m + 8, frag_to_bits(dlogit));
  gd.store(kGradDy10m + 9, frag_to_bits(zero_frag()));

  // T1: [Dense_10 | Dense_9]^T (z rows) -> dz = dy8 (Dense_8 output is linear)
  chain_layer<bwd_cons_base(1), bwd_nk(1), bwd_no(1)>(
      ring, [&](auto) { return zero_acc(); },
      [&](auto k_) -> bf16x8 {
        constexpr int ks = decltype(k_)::value;
        if constexpr (ks < 8) return a0[ks];
        else return dlogit;
      },
      [&](auto o_, const f32x16& acc) {
        constexpr int o = decltype(o_)::value;
        a1[2 * o] = acc_to_frag<0, false>(acc);
        a1[2 * o + 1] = acc_to_frag<1, false>(acc);
        gd.store(grad_dy_slot(8) + 2 * o, frag_to_bits(a1[2 * o]));
        gd.store(grad_dy_slot(8) + 2 * o + 1, frag_to_bits(a1[2 * o + 1]));
      });

  if constexpr (HEAD_ONLY) return;
  // T2..T9: Dense_l^T for l = 8..1: dy_l (in) -> dh_{l-1}, masked by relu(h_{l-1}) -> dy_{l-1}
  static_assert(bwd_nk(2) == 16 && bwd_no(2) == 8, "hidden_back");
  static_for<8>([&](auto i_) {
    constexpr int TT = 2 + decltype(i_)::value, l = bwd_dense(TT);  // dense layer whose transpose is applied: 8..1
    if constexpr (TT % 2 == 0) hidden_back<bwd_cons_base(TT), l>(ring, a1, a0, relu_mask[l - 1], gd);
    else hidden_back<bwd_cons_base(TT), l>(ring, a0, a1, relu_mask[l - 1], gd);
  });
}

// launches nerf_wgrad_kernel (nerf_mlp.hip) on the workgroups of `list` (at most kWgradMaxBlocks): X operands from xbuf,
// dy operands from ybuf (both dumps of n_tiles tiles in the layout `lay` names, see fused_chain.h dump_off); `slabs` has
// room for kWgradSlabBytes
int launch_nerf_wgrad(const WgradList& list, const void* xbuf, const void* ybuf, int64_t n_tiles, float* grads,
                      hipStream_t stream, WgLayout lay, float* slabs, bool plain_loads = false,
                      bool fold = true);  // fold == false: the caller folds the slabs itself

// Layer-stationary backward of the eight 256 x 256 layers Dense_8 .. Dense_1 of ONE model (nerf_bwd_ls.hip): `scratch`
// (ls_scratch_bytes(m)) starts with the gradient dump, dy8 already written (slots grad_dy_slot(8)..); on return the
// launches that add dW_1..8 and db_1..8 to `grads` and leave dy7..dy0 in the dump are enqueued.  RefNERFModel's
// first-order trunk backward; ls_small_slabs: the kWgradSlabBytes of `scratch` for a weight-gradient launch behind it.
int64_t ls_scratch_bytes(int64_t m);
float* ls_small_slabs(void* scratch, int64_t m);
int launch_ls_pipeline(const void* packed, const void* save, void* scratch, int64_t m, float* grads, hipStream_t stream);

}  // namespace lnrf
