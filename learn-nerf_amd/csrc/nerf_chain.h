// nerf_chain.h — parts of the NeRFModel backward shared by nerf_mlp.hip (separate chain / weight-gradient launches),
// nerf_bwd_ls.hip (layer-stationary backward) and refnerf_fused.hip: the input-gradient chain of one 32-evaluation
// tile and the launch of the weight-gradient problems of nerf_wgrad.h.
#pragma once
#include "fused_chain.h"

namespace lnrf {

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
    relu_mask[i] = *reinterpret_cast<const uint4*>(save + dump_off(kSaveMask + i, tile, save_tiles, kSaveTileSlots) +
                                                   lane * 16);
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
        constexpr int o = decltype(o_)::value;
        const unsigned mb = (o >> 1) == 0 ? relu_mask[8].x : relu_mask[8].y;
        a0[2 * o] = masked_frag<0>(acc, mb, 16 * (o & 1));
        a0[2 * o + 1] = masked_frag<1>(acc, mb, 16 * (o & 1));
        gd.store(kGradDy10m + 2 * o, frag_to_bits(a0[2 * o]));
        gd.store(kGradDy10m + 2 * o + 1, frag_to_bits(a0[2 * o + 1]));
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
  auto back = [&](auto t_, bf16x8(&in)[16], bf16x8(&out)[16]) {
    constexpr int TT = decltype(t_)::value;
    constexpr int l = bwd_dense(TT);  // dense layer whose transpose is applied
    chain_layer<bwd_cons_base(TT), bwd_nk(TT), bwd_no(TT)>(
        ring, [&](auto) { return zero_acc(); },
        [&](auto k_) -> bf16x8 { return in[decltype(k_)::value]; },
        [&](auto o_, const f32x16& acc) {
          constexpr int o = decltype(o_)::value;
          const uint4 mk = relu_mask[l - 1];
          const unsigned mb = (o >> 1) == 0 ? mk.x : ((o >> 1) == 1 ? mk.y : ((o >> 1) == 2 ? mk.z : mk.w));
          out[2 * o] = masked_frag<0>(acc, mb, 16 * (o & 1));
          out[2 * o + 1] = masked_frag<1>(acc, mb, 16 * (o & 1));
          gd.store(grad_dy_slot(l - 1) + 2 * o, frag_to_bits(out[2 * o]));
          gd.store(grad_dy_slot(l - 1) + 2 * o + 1, frag_to_bits(out[2 * o + 1]));
        });
  };
  back(std::integral_constant<int, 2>{}, a1, a0);  // Dense_8^T: dy8 -> dy7
  back(std::integral_constant<int, 3>{}, a0, a1);  // dy7 -> dy6
  back(std::integral_constant<int, 4>{}, a1, a0);  // dy6 -> dy5
  back(std::integral_constant<int, 5>{}, a0, a1);  // Dense_5^T (h rows): dy5 -> dy4
  back(std::integral_constant<int, 6>{}, a1, a0);  // dy4 -> dy3
  back(std::integral_constant<int, 7>{}, a0, a1);  // dy3 -> dy2
  back(std::integral_constant<int, 8>{}, a1, a0);  // dy2 -> dy1
  back(std::integral_constant<int, 9>{}, a0, a1);  // Dense_1^T: dy1 -> dy0
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
