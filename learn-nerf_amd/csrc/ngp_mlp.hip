// ngp_mlp.hip — fused InstantNGPModel MLP (learn_nerf/instant_ngp.py:38-54) on the bf16 MFMA of gfx950.
//
//   enc (L*F hash-grid features) -> Dense_0 64 relu -> Dense_1 16 (density = exp(out[0]))
//   [d_emb(24), out(16)] -> Dense_2 64 relu -> Dense_3 64 relu -> Dense_4 3 tanh
//
// Same construction as nerf_mlp.hip: one wave owns 32 evaluations, the f32 accumulator tile of a layer is
// converted in place into the B operand of the next one, the packed A-fragment stream (26 + 20 fragments)
// goes through the shared LDS ring.  The network is so small that the backward kernel recomputes the
// forward (26 MFMAs) instead of reading saved activations, then runs the transposed chain, writes
// d loss / d enc feature-major for the hash-grid scatter, and forms the weight gradients in the same
// launch.  All index arithmetic lives in ngp_layout.h.
// Precision: bf16 operands, fp32 accumulate, fp32 bias / activations / directional encoding.

#include "fused_chain.h"
#include "ngp_layout.h"

namespace lnrf {

constexpr int kNgpLds = kRingBytes + 1024;
template <int N>
using Int = std::integral_constant<int, N>;
template <int L>
using NgpDense = Int<ngp_wgrad_problem(L)>;  // Dense_L's row of the weight-gradient table

// forward layer L / backward step T of the chain, shaped by the tables of ngp_layout.h
template <int NE, int L, class RING, class GetB, class Epi>
__device__ __forceinline__ void ngp_fwd_layer(RING& ring, int h, GetB getb, Epi epi) {
  chain_layer<ngp_fwd_base(L, NE), ngp_fwd_nk(L, NE), ngp_fwd_no(L)>(
      ring, [&](auto o_) { return bias_acc(ngp_bias_base(L) + 32 * decltype(o_)::value, h); }, getb, epi);
}
template <int NE, int T, class RING, class GetB, class Epi>
__device__ __forceinline__ void ngp_bwd_layer(RING& ring, GetB getb, Epi epi) {
  chain_layer<ngp_bwd_base(T, NE), ngp_bwd_nk(T), ngp_bwd_no(T)>(ring, [&](auto) { return zero_acc(); }, getb, epi);
}

// out tile O of a 64-wide relu layer -> k-steps 2 O, 2 O + 1 of the next layer's B operand
template <int O>
__device__ __forceinline__ void relu_frags(const f32x16& acc, bf16x8 (&dst)[4]) {
  dst[2 * O] = acc_to_frag<0, true>(acc);
  dst[2 * O + 1] = acc_to_frag<1, true>(acc);
}
template <int O>
__device__ __forceinline__ void relu_frags_split(const f32x16& acc, bf16x8 (&hi)[4], bf16x8 (&lo)[4]) {
  acc_to_frag_split<0, true>(acc, hi[2 * O], lo[2 * O]);
  acc_to_frag_split<1, true>(acc, hi[2 * O + 1], lo[2 * O + 1]);
}

// dh * relu'(h): keep accumulator registers 8S..8S+7 where the bf16 activation fragment is non-zero
template <int S>
__device__ __forceinline__ bf16x8 masked_by(const f32x16& acc, const bf16x8& ref) {
  const uint4 rb = frag_to_bits(ref);
  const unsigned w[4] = {rb.x, rb.y, rb.z, rb.w};
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned e = (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xFFFFu);
    f[j] = (__bf16)(e != 0u ? acc[8 * S + j] : 0.0f);
  }
  return f;
}
template <int O>
__device__ __forceinline__ void masked_frags(const f32x16& acc, const bf16x8 (&ref)[4], bf16x8 (&dst)[4]) {
  dst[2 * O] = masked_by<0>(acc, ref[2 * O]);
  dst[2 * O + 1] = masked_by<1>(acc, ref[2 * O + 1]);
}

// Backward: the weight gradients are formed inside the kernel.  The model has 10 K parameters, so a
// workgroup can keep its share of dW in registers for the whole launch: the workgroups are persistent (one per CU,
// groups of 8 tiles taken round-robin), and after every backward step the 8 waves put the layer's X and dy fragments
// into an LDS staging area (the layout the split-K body of fused_chain.h reads: one 32-evaluation step per wave),
// then every wave accumulates ONE 32x32 tile of that layer's dW over its share of the 8 steps (transposed
// ds_read_b64_tr_b16 reads) and the tiles leave once, at the end of the launch (plain stores).  This removes the
// 34 KiB per tile of X / dy dumps (written and read back: 2.3 GB per step at 4096 rays) and a second launch.
// Which waves accumulate which layer in which slot is kNgpWgrad (ngp_layout.h).

// grads[dense_off + p] += sum over workgroups and the layer's k-parts of wparts[(wg, part)][p].  One workgroup folds 32
// neighbouring parameters: thread (slice s, parameter) sums the rows of slice s of the workgroups in order, the eight
// slice sums meet in LDS and are added in order by slice 0, which owns the parameter (plain read-modify-write).  Every
// addition has a fixed place, so the Dense gradients of the fused backward are bit-reproducible.
constexpr int kNgpReduceSlices = 8;
__global__ __launch_bounds__(256) void ngp_wparts_reduce_kernel(const float* __restrict__ wparts, int n_wg, int pstride,
                                                                int n_params, NgpPartsPlan plan,
                                                                float* __restrict__ grads_dense) {
  __shared__ float part[kNgpReduceSlices][32];
  const int pl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int p = blockIdx.x * 32 + pl;
  int parts = 0;
  if (p < n_params) {
#pragma unroll
    for (int l = 0; l < kNgpLayers; ++l)
      if (p >= plan.lo[l] && p < plan.hi[l]) parts = plan.parts[l];
  }
  const int w0 = (int)((int64_t)n_wg * sl / kNgpReduceSlices), w1 = (int)((int64_t)n_wg * (sl + 1) / kNgpReduceSlices);
  float acc = 0.0f;
  for (int w = w0; w < w1; ++w)
    for (int q = 0; q < parts; ++q) acc += wparts[((int64_t)w * kNgpMaxParts + q) * pstride + p];
  part[sl][pl] = acc;
  __syncthreads();
  if (sl == 0 && parts > 0) {
    float tot = part[0][pl];
#pragma unroll
    for (int q = 1; q < kNgpReduceSlices; ++q) tot += part[q][pl];
    grads_dense[p] += tot;
  }
}

constexpr int kNgpStageStep = 8 * kFragBytes;                 // backward: staging bytes per wave (<= 8 fragments per layer)
constexpr int kNgpGmaxOff = kNgpLds + kWaves * kNgpStageStep;    // backward: 8 running maxima per lane (32 B)
constexpr int kNgpFusedLds = kNgpGmaxOff + kThreads * 32;        // 129 KiB: one persistent workgroup per CU

#ifdef LNRF_TIMELINE
__device__ unsigned long long* g_ngp_timeline_buf = nullptr;  // 8 waves x 1024 stamps (debug build only)
#endif

template <int NE, bool BWD>
__global__ __launch_bounds__(kThreads) void ngp_mlp_kernel(
    const char* __restrict__ packed, const float* __restrict__ enc_t, const float* __restrict__ d_g, int lf,
    int64_t M, int64_t n_tiles, float* __restrict__ density, float* __restrict__ rgb,
    const float* __restrict__ g_density, const float* __restrict__ g_rgb, float* __restrict__ g_enc_t,
    float* __restrict__ lmax_parts = nullptr, NgpWgradArgs wargs = NgpWgradArgs{}, float* __restrict__ wparts = nullptr,
    int pstride = 0, int64_t dense_off = 0) {
  // backward: running max |d loss / d enc| of the rows this lane writes, 8 slots (rows 4h + 8j + {0,1} / + {2,3} are
  // the two features of levels 2h + 4j / 2h + 4j + 1): the fixed-point scale of the scatter pass.  The persistent
  // kernel keeps the slots in LDS (32 bytes per lane, its registers are full), reduces them once at the end
  // and stores one row of 16 per workgroup — plain stores; ngp_level_max_kernel folds the rows.  (Same-address
  // global atomics retire at ~10 ns each: 256 workgroups x 16 of them at the end of the launch measured +30 us,
  // a wave reduction per group +35 us.)
  __shared__ unsigned s_lmax[16];
  if constexpr (BWD) {
    float4* gm = reinterpret_cast<float4*>(smem + kNgpGmaxOff + threadIdx.x * 32);
    gm[0] = gm[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  stage_bias<kThreads>(packed + kNgpPackBiasOff, kNgpBiasFloats);
  if (tid < 16) s_lmax[tid] = 0u;
  // persistent accumulators of the backward: kNgpWgrad says which half of the workgroup and which slot a layer gets
  f32x16 wacc[BWD ? kNgpWSlots : 1];
  float wbias[BWD ? kNgpWSlots : 1];
  if constexpr (BWD) {
#pragma unroll
    for (int i = 0; i < kNgpWSlots; ++i) {
      wacc[i] = zero_acc();
      wbias[i] = 0.0f;
    }
  }
  const int64_t n_groups = n_tiles / kWaves;
  for (int64_t group = blockIdx.x; group < n_groups; group += BWD ? (int64_t)gridDim.x : n_groups) {
  const int64_t tile = group * kWaves + wave;
  const int64_t m = tile * kTileCols + c;
  const bool valid = m < M;
  using Seq = LinSeq<BWD ? ngp_total_count(NE) : ngp_fwd_count(NE)>;
  Ring<(Seq::count + kStageFrags - 1) / kStageFrags, Seq> ring;
#ifdef LNRF_TIMELINE
  ring.tl.buf = g_ngp_timeline_buf;
  ring.tl.n = 0;
  ring.tl.on = BWD && NE == 2 && g_ngp_timeline_buf != nullptr && blockIdx.x == gridDim.x / 2 &&
               group == (int64_t)blockIdx.x + 2 * (int64_t)gridDim.x;
#endif
  LNRF_TL_STAMP(ring);  // 0: group start
  if constexpr (BWD) __syncthreads();  // previous group's LDS reads (ring, staging) are finished
  LNRF_TL_STAMP(ring);  // 1: after the top barrier

  // encoding fragments: k slot (ks, h, j) <-> feature hidden_feat(ks, h, j) (row of enc_t; spelled out).
  // All loads are issued before the first use: clamped addresses instead of branches, and the row stride re-read
  // through an opaque copy so that the 16 row addresses are computed here instead of being hoisted out of the group
  // loop and spilled (that version waited for 32 scratch / global round trips in a row: 12 us of a 32 us group).
  int64_t Ms = M;
  if constexpr (BWD) asm volatile("" : "+s"(Ms));
  const int64_t mm = valid ? m : M - 1;
  float ev[NE][8];
  static_for<NE>([&](auto ks_) {
    constexpr int ks = decltype(ks_)::value;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int feat = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
      ev[ks][j] = enc_t[(int64_t)(feat < lf ? feat : lf - 1) * Ms + mm];
    }
  });
  bf16x8 ef[NE];
  static_for<NE>([&](auto ks_) {
    constexpr int ks = decltype(ks_)::value;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int feat = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
      ef[ks][j] = (__bf16)((valid && feat < lf) ? ev[ks][j] : 0.0f);
    }
  });
  LNRF_TL_STAMP(ring);  // 2: encoding loaded and converted
  float pd[3] = {0, 0, 0};
  float gy4[3] = {0, 0, 0}, g_dens = 0.0f;
  if (valid) {
#pragma unroll
    for (int a = 0; a < 3; ++a) pd[a] = d_g[m * 3 + a];
    if (BWD && h == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) gy4[k] = g_rgb[m * 3 + k];
      g_dens = g_density[m];
    }
  }
  LNRF_TL_STAMP(ring);  // 3: direction / output gradients requested
  __syncthreads();
  LNRF_TL_STAMP(ring);  // 4: after the barrier

  const char* wstream = packed;
  if constexpr (BWD) asm volatile("" : "+s"(wstream));  // keep the stage addresses out of the group loop's preheader
  ring.stream = wstream;
  ring.wave = wave;
  ring.lane = lane;
  ring.prologue();
  LNRF_TL_STAMP(ring);  // 5: ring prologue done

  // sinusoidal direction embedding (model.py:65-77): feature e = 8 coord + 4 is_cos + freq, slot order = e
  bf16x8 de[2];
  static_for<2>([&](auto ks_) {
    constexpr int ks = decltype(ks_)::value;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
      float v = 0.0f;
      if (e < kNgpDembDim) {
        const int cd = e >> 3, fr = e & 3;
        const float x = cd == 0 ? pd[0] : (cd == 1 ? pd[1] : pd[2]);
        float s, co;
        sincos_pe(x * (float)(1 << fr), &s, &co);
        v = (e & 4) ? co : s;
      }
      de[ks][j] = (__bf16)v;
    }
  });

  // backward: stage fragment f (X fragments first, then dy) of this wave's tile; weight-gradient step of layer P
  char* stage = smem + kNgpLds + wave * kNgpStageStep;
  auto stage_frag = [&](int f, const bf16x8& v) {
    *reinterpret_cast<uint4*>(stage + f * kFragBytes + dump_lane_off(f, c, h)) = frag_to_bits(v);
  };
  auto wgrad_layer = [&](auto p_) {
    constexpr int P = decltype(p_)::value, SLOT = kNgpWgrad[P].slot, HALF = kNgpWgrad[P].half, NXF = kNgpWgrad[P].nxf;
    constexpr int STEPS = 2 * ngp_wgrad_tiles(P);  // 4 waves = NT tiles x (4 / NT) k-parts of 8 / (4 / NT) steps
    LNRF_TL_STAMP(ring);                                     // staged, arrive
    __syncthreads();                                         // all 8 tiles staged
    LNRF_TL_STAMP(ring);                                     // released
    if ((wave >> 2) == HALF) {
      constexpr int NO = kNgpWgrad[P].nyf / 2, NT = ngp_wgrad_tiles(P);
      const int w4 = wave & 3;
      const int tile_id = w4 % NT, part = w4 / NT;
      const int it = tile_id / NO, ot = tile_id % NO;
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        const char* buf = smem + kNgpLds + (part * STEPS + st) * kNgpStageStep;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const bf16x8 bfv = tr_frag(buf + (NXF + 2 * ot) * kFragBytes, lane, 0, q);
          if (it == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) wbias[SLOT] += (float)bfv[j];
          }
          const bf16x8 afv = tr_frag(buf + 2 * it * kFragBytes, lane, 0, q);
          wacc[SLOT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afv, bfv, wacc[SLOT], 0, 0, 0);
        }
      }
    }
    LNRF_TL_STAMP(ring);  // weight-gradient MFMAs issued
    __syncthreads();  // staging area free for the next layer
    LNRF_TL_STAMP(ring);  // released
  };

  bf16x8 h0[4], o16, c1[4], c2[4];
  float logit = 0.0f;
  // Dense_0 + relu
  ngp_fwd_layer<NE, 0>(ring, h, [&](auto k_) -> bf16x8 { return ef[decltype(k_)::value]; },
                       [&](auto o_, const f32x16& acc) { relu_frags<decltype(o_)::value>(acc, h0); });
  // Dense_1 (linear): 16 features = rows 0..15 of the tile; density logit = feature 0
  ngp_fwd_layer<NE, 1>(ring, h, [&](auto k_) -> bf16x8 { return h0[decltype(k_)::value]; },
                       [&](auto, const f32x16& acc) {
                         o16 = acc_to_frag<0, false>(acc);
                         logit = acc[0];
                       });
  const float dens = __expf(logit);  // instant_ngp.py:49, valid on lanes h == 0
  // Dense_2 + relu on [d_emb, out]
  ngp_fwd_layer<NE, 2>(
      ring, h,
      [&](auto k_) -> bf16x8 {
        constexpr int ks = decltype(k_)::value;
        if constexpr (ks < 2) return de[ks];
        else return o16;
      },
      [&](auto o_, const f32x16& acc) { relu_frags<decltype(o_)::value>(acc, c1); });
  // Dense_3 + relu
  ngp_fwd_layer<NE, 3>(ring, h, [&](auto k_) -> bf16x8 { return c1[decltype(k_)::value]; },
                       [&](auto o_, const f32x16& acc) { relu_frags<decltype(o_)::value>(acc, c2); });
  // Dense_4 + tanh
  float y[3] = {0, 0, 0};
  ngp_fwd_layer<NE, 4>(ring, h, [&](auto k_) -> bf16x8 { return c2[decltype(k_)::value]; },
                       [&](auto, const f32x16& acc) {
                         y[0] = tanhf(acc[0]);
                         y[1] = tanhf(acc[1]);
                         y[2] = tanhf(acc[2]);
                       });
  if constexpr (!BWD) {
    if (h == 0 && valid) {
      density[m] = dens;
      rgb[m * 3 + 0] = y[0];
      rgb[m * 3 + 1] = y[1];
      rgb[m * 3 + 2] = y[2];
    }
    return;
  } else {
    // ---- backward
    // head gradients in fp32: tanh' and exp'
    bf16x8 dy4 = zero_frag();
    dy4[0] = (__bf16)(gy4[0] * (1.0f - y[0] * y[0]));
    dy4[1] = (__bf16)(gy4[1] * (1.0f - y[1] * y[1]));
    dy4[2] = (__bf16)(gy4[2] * (1.0f - y[2] * y[2]));
    if (h != 0) dy4 = zero_frag();
    const float g_logit = h == 0 ? g_dens * dens : 0.0f;
    {  // Dense_4: X = c2, dy = dy4
      static_for<4>([&](auto i_) { stage_frag(decltype(i_)::value, c2[decltype(i_)::value]); });
      stage_frag(4, dy4);
      stage_frag(5, zero_frag());
      wgrad_layer(NgpDense<4>{});
    }

    bf16x8 dy3[4], dy2[4], dy1, dy0[4];
    // T0: Dense_4^T -> dc2, relu mask of c2
    ngp_bwd_layer<NE, 0>(ring, [&](auto) -> bf16x8 { return dy4; },
                         [&](auto o_, const f32x16& acc) { masked_frags<decltype(o_)::value>(acc, c2, dy3); });
    {  // Dense_3: X = c1, dy = dy3
      static_for<4>([&](auto i_) {
        stage_frag(decltype(i_)::value, c1[decltype(i_)::value]);
        stage_frag(4 + decltype(i_)::value, dy3[decltype(i_)::value]);
      });
      wgrad_layer(NgpDense<3>{});
    }
    // T1: Dense_3^T -> dc1, relu mask of c1
    ngp_bwd_layer<NE, 1>(ring, [&](auto k_) -> bf16x8 { return dy3[decltype(k_)::value]; },
                         [&](auto o_, const f32x16& acc) { masked_frags<decltype(o_)::value>(acc, c1, dy2); });
    {  // Dense_2: X = [d_emb, out] (24 + 16 features in 4 fragments), dy = dy2
      stage_frag(0, de[0]);
      stage_frag(1, de[1]);
      stage_frag(2, o16);
      stage_frag(3, zero_frag());
      static_for<4>([&](auto i_) { stage_frag(4 + decltype(i_)::value, dy2[decltype(i_)::value]); });
      wgrad_layer(NgpDense<2>{});
    }
    // T2: Dense_2^T restricted to the rows of `out` (d_emb has no parameters upstream); the density
    // head adds d exp(out_0) to feature 0 (lane h == 0, register 0)
    ngp_bwd_layer<NE, 2>(ring, [&](auto k_) -> bf16x8 { return dy2[decltype(k_)::value]; },
                         [&](auto, const f32x16& acc) {
                           f32x16 t = acc;
                           t[0] += g_logit;
                           dy1 = acc_to_frag<0, false>(t);
                         });
    {  // Dense_1: X = h0, dy = dy1
      static_for<4>([&](auto i_) { stage_frag(decltype(i_)::value, h0[decltype(i_)::value]); });
      stage_frag(4, dy1);
      stage_frag(5, zero_frag());
      wgrad_layer(NgpDense<1>{});
    }
    // T3: Dense_1^T -> dh0, relu mask of h0
    ngp_bwd_layer<NE, 3>(ring, [&](auto) -> bf16x8 { return dy1; },
                         [&](auto o_, const f32x16& acc) { masked_frags<decltype(o_)::value>(acc, h0, dy0); });
    {  // Dense_0: X = hash-grid encoding, dy = dy0
      stage_frag(0, ef[0]);
      if constexpr (NE > 1) stage_frag(1, ef[1]);
      else stage_frag(1, zero_frag());
      static_for<4>([&](auto i_) { stage_frag(2 + decltype(i_)::value, dy0[decltype(i_)::value]); });
      wgrad_layer(NgpDense<0>{});
    }
    // T4: Dense_0^T -> d loss / d enc, feature-major fp32 for the hash-grid scatter
    ngp_bwd_layer<NE, 4>(
        ring, [&](auto k_) -> bf16x8 { return dy0[decltype(k_)::value]; }, [&](auto, const f32x16& acc) {
          float tmax[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) tmax[i] = 0.0f;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
            if (valid && row < lf) {
              g_enc_t[(int64_t)row * Ms + m] = acc[q];  // Ms: addresses formed here, not hoisted and spilled
              tmax[q >> 1] = fmaxf(tmax[q >> 1], fabsf(acc[q]));
            }
          }
          float4* gm = reinterpret_cast<float4*>(smem + kNgpGmaxOff + tid * 32);
          const float4 a = gm[0], b = gm[1];
          gm[0] = make_float4(fmaxf(a.x, tmax[0]), fmaxf(a.y, tmax[1]), fmaxf(a.z, tmax[2]), fmaxf(a.w, tmax[3]));
          gm[1] = make_float4(fmaxf(b.x, tmax[4]), fmaxf(b.y, tmax[5]), fmaxf(b.z, tmax[6]), fmaxf(b.w, tmax[7]));
        });
  LNRF_TL_STAMP(ring);  // group end
  }
  }  // group loop
  if constexpr (BWD) {
    if (lmax_parts) {  // kernel argument: uniform
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float v = reinterpret_cast<const float*>(smem + kNgpGmaxOff + tid * 32)[i];
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        // non-negative floats order like their bit patterns
        if (c == 0 && v > 0.0f) atomicMax(&s_lmax[4 * (i >> 1) + 2 * h + (i & 1)], __float_as_uint(v));
      }
      __syncthreads();
      if (tid < 16) lmax_parts[(int64_t)blockIdx.x * 16 + tid] = __uint_as_float(s_lmax[tid]);
    }
    // The launch's share of dW: every wave stores its tile (and bias sums) ONCE, with plain stores, into the row of its
    // (workgroup, k-part) in `wparts`; ngp_wparts_reduce_kernel folds the rows into the gradient vector.  (fp32
    // atomics straight into the gradient — 256 workgroups hitting the same 10 K addresses — cost 76 us per launch,
    // half of the coarse model's backward: same-line memory atomics retire one after the other.)
    // KEEP IN STEP with ngp_count_owners (layout_host.cpp), the copy of this arithmetic that the CPU test walks.
    const int colr = lane & 31, hh = lane >> 5;
    auto flush = [&](auto p_) {
      constexpr int P = decltype(p_)::value, SLOT = kNgpWgrad[P].slot, HALF = kNgpWgrad[P].half;
      constexpr int NO = kNgpWgrad[P].nyf / 2, NT = ngp_wgrad_tiles(P);
      if ((wave >> 2) != HALF) return;
      const NgpWgradProblem& pb = wargs.p[P];
      const int tile_id = (wave & 3) % NT, part = (wave & 3) / NT;
      const int it = tile_id / NO, ot = tile_id % NO;
      int out_idx = -1, out_dim = 1;
      int64_t w_off = 0, b_off = 0;
      NgpWgradEpi::cols(pb, ot, colr, out_idx, out_dim, w_off, b_off);
      float* __restrict__ row = wparts + ((int64_t)blockIdx.x * kNgpMaxParts + part) * pstride;
      w_off -= dense_off;  // rows hold the Dense parameters only
      b_off -= dense_off;
      if (it == 0) {
        float sacc = wbias[SLOT];
        sacc += __shfl_xor(sacc, 32, 64);
        if (hh == 0 && out_idx >= 0) row[b_off + out_idx] = sacc;
      }
      static_for<16>([&](auto q_) {
        constexpr int qq = decltype(q_)::value;
        const int r = ngp_acc_row(qq, hh);
        const int f = 2 * it + (r >> 4);
        const int in_idx = NgpWgradEpi::row(pb, f, r & 15);
        if (out_idx >= 0 && in_idx >= 0) row[w_off + (int64_t)in_idx * out_dim + out_idx] = wacc[SLOT][qq];
      });
    };
    flush(NgpDense<3>{}), flush(NgpDense<4>{}), flush(NgpDense<0>{});  // waves 0-3
    flush(NgpDense<2>{}), flush(NgpDense<1>{});                        // waves 4-7
  }
}

// level_absmax[l] = max(level_absmax[l], max over the workgroup rows parts[n_parts][16]); one workgroup of 256 threads
__global__ __launch_bounds__(256) void ngp_level_max_kernel(const float* __restrict__ parts, int n_parts, int n_levels,
                                                            unsigned* __restrict__ level_absmax) {
  __shared__ unsigned s_max[16];
  if (threadIdx.x < 16) s_max[threadIdx.x] = 0u;
  __syncthreads();
  const int l = threadIdx.x & 15;
  float v = 0.0f;
  for (int p = threadIdx.x >> 4; p < n_parts; p += 16) v = fmaxf(v, parts[(int64_t)p * 16 + l]);
  if (v > 0.0f) atomicMax(&s_max[l], __float_as_uint(v));
  __syncthreads();
  if ((int)threadIdx.x < n_levels && threadIdx.x < 16 && s_max[threadIdx.x] != 0u)
    atomicMax(&level_absmax[threadIdx.x], s_max[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// Split-precision forward ("bf16x3", the render / evaluation path; instant_ngp.py:38-54 is fp32 in the reference): every
// fp32 operand — weight, hash-grid feature, direction embedding, activation — is a bf16 pair (hi, lo) with hi + lo equal
// to the value to 16 significant bits and every product is lo*hi + hi*lo + hi*hi on the bf16 MFMA with fp32 accumulation,
// as nerf_fwd_split_kernel does for NeRFModel.  The whole stream ([hi, lo] per forward fragment: at most 52 KiB) is
// staged in LDS once per persistent workgroup.
// ---------------------------------------------------------------------------------------------
template <int NE>
__global__ __launch_bounds__(kThreads) void ngp_mlp_fwd_split_kernel(
    const char* __restrict__ packed3, const float* __restrict__ enc_t, const float* __restrict__ d_g, int lf, int64_t M,
    int64_t n_tiles, float* __restrict__ density, float* __restrict__ rgb) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;
  for (int i = tid; i < kNgpSplitBytes / 16; i += kThreads)
    reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(packed3)[i];
  __syncthreads();
  const float* bias_l = reinterpret_cast<const float*>(smem + kNgpSplitBiasOff);
  // the per-lane LDS offset is made opaque once per group: the stream does not change, so the compiler would otherwise
  // hoist all 52 fragment reads (208 registers) out of the group loop and spill them
  int lds_lane = lane * 16;
  auto afrag = [&](int g, int part) -> bf16x8 {
    return bits_to_frag(*reinterpret_cast<const uint4*>(smem + (2 * g + part) * kFragBytes + lds_lane));
  };
  auto bias_tile = [&](int row0) -> f32x16 {  // accumulator rows (q & 3) + 8 (q >> 2) + 4 h of the 32-row tile at row0
    f32x16 acc;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const float4 v = *reinterpret_cast<const float4*>(bias_l + row0 + 4 * h + 8 * gq);
      acc[4 * gq + 0] = v.x; acc[4 * gq + 1] = v.y; acc[4 * gq + 2] = v.z; acc[4 * gq + 3] = v.w;
    }
    return acc;
  };
  // one layer: out tiles x k-steps, three MFMAs per product (small terms first)
  auto layer = [&](auto l_, auto&& bhi, auto&& blo, auto&& epi) {
    constexpr int L = decltype(l_)::value, bias0 = ngp_bias_base(L);
    constexpr int G0 = ngp_fwd_base(L, NE), NK = ngp_fwd_nk(L, NE), NO = ngp_fwd_no(L);
    static_for<NO>([&](auto o_) {
      constexpr int o = decltype(o_)::value;
      f32x16 acc = bias_tile(bias0 + 32 * o);
      static_for<NK>([&](auto k_) {
        constexpr int ks = decltype(k_)::value;
        const bf16x8 ahi = afrag(G0 + o * NK + ks, 0), alo = afrag(G0 + o * NK + ks, 1);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi(k_), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo(k_), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi(k_), acc, 0, 0, 0);
      });
      epi(o_, acc);
    });
  };
  const int64_t n_groups = n_tiles / kWaves;
  for (int64_t group = blockIdx.x; group < n_groups; group += gridDim.x) {
    asm volatile("" : "+v"(lds_lane));
    const int64_t tile = group * kWaves + wave;
    const int64_t m = tile * kTileCols + c;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    bf16x8 ef_hi[NE], ef_lo[NE];
    static_for<NE>([&](auto ks_) {
      constexpr int ks = decltype(ks_)::value;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int feat = hidden_feat(ks, h, j);
        const float v = (valid && feat < lf) ? enc_t[(int64_t)(feat < lf ? feat : lf - 1) * M + mm] : 0.0f;
        split_store(v, ef_hi[ks], ef_lo[ks], j);
      }
    });
    float pd[3] = {0, 0, 0};
    if (valid) {
#pragma unroll
      for (int a = 0; a < 3; ++a) pd[a] = d_g[m * 3 + a];
    }
    bf16x8 de_hi[2], de_lo[2];  // sinusoidal direction embedding (model.py:65-77): feature e = 8 coord + 4 is_cos + freq
    static_for<2>([&](auto ks_) {
      constexpr int ks = decltype(ks_)::value;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = hidden_feat(ks, h, j);
        float v = 0.0f;
        if (e < kNgpDembDim) {
          const int cd = e >> 3, fr = e & 3;
          const float x = cd == 0 ? pd[0] : (cd == 1 ? pd[1] : pd[2]);
          float sn, co;
          sincos_pe(x * (float)(1 << fr), &sn, &co);
          v = (e & 4) ? co : sn;
        }
        split_store(v, de_hi[ks], de_lo[ks], j);
      }
    });
    bf16x8 h0h[4], h0l[4], o16h, o16l, c1h[4], c1l[4], c2h[4], c2l[4];
    float logit = 0.0f, y[3] = {0, 0, 0};
    layer(Int<0>{}, [&](auto k_) -> bf16x8 { return ef_hi[decltype(k_)::value]; },
          [&](auto k_) -> bf16x8 { return ef_lo[decltype(k_)::value]; },
          [&](auto o_, const f32x16& acc) { relu_frags_split<decltype(o_)::value>(acc, h0h, h0l); });
    layer(Int<1>{}, [&](auto k_) -> bf16x8 { return h0h[decltype(k_)::value]; },
          [&](auto k_) -> bf16x8 { return h0l[decltype(k_)::value]; },
          [&](auto, const f32x16& acc) {
            acc_to_frag_split<0, false>(acc, o16h, o16l);
            logit = acc[0];
          });
    layer(Int<2>{},
          [&](auto k_) -> bf16x8 {
            constexpr int ks = decltype(k_)::value;
            if constexpr (ks < 2) return de_hi[ks];
            else return o16h;
          },
          [&](auto k_) -> bf16x8 {
            constexpr int ks = decltype(k_)::value;
            if constexpr (ks < 2) return de_lo[ks];
            else return o16l;
          },
          [&](auto o_, const f32x16& acc) { relu_frags_split<decltype(o_)::value>(acc, c1h, c1l); });
    layer(Int<3>{}, [&](auto k_) -> bf16x8 { return c1h[decltype(k_)::value]; },
          [&](auto k_) -> bf16x8 { return c1l[decltype(k_)::value]; },
          [&](auto o_, const f32x16& acc) { relu_frags_split<decltype(o_)::value>(acc, c2h, c2l); });
    layer(Int<4>{}, [&](auto k_) -> bf16x8 { return c2h[decltype(k_)::value]; },
          [&](auto k_) -> bf16x8 { return c2l[decltype(k_)::value]; },
          [&](auto, const f32x16& acc) {
            y[0] = tanhf(acc[0]);
            y[1] = tanhf(acc[1]);
            y[2] = tanhf(acc[2]);
          });
    if (h == 0 && valid) {
      density[m] = expf(logit);  // instant_ngp.py:49
      rgb[m * 3 + 0] = y[0];
      rgb[m * 3 + 1] = y[1];
      rgb[m * 3 + 2] = y[2];
    }
  }
}

// SPLIT: [hi, lo] pairs of the forward fragments (the render blob), else the 48-fragment stream; then the fp32 biases
template <bool SPLIT>
__global__ void ngp_pack_kernel(const float* __restrict__ params, NgpOffsets off, int lf, int ne,
                                char* __restrict__ packed) {
  constexpr int total_w = (SPLIT ? kNgpSplitMaxFrags : kNgpStreamFrags) * 512;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total_w + kNgpBiasFloats; e += gridDim.x * blockDim.x) {
    if (e < total_w) {
      const int g = SPLIT ? e >> 10 : e >> 9, lane = (e >> 3) & 63, j = e & 7;
      const int64_t idx = SPLIT || g < ngp_fwd_count(ne) ? ngp_fwd_stream_index(g, lane, j, off, lf, ne)
                                                         : ngp_bwd_stream_index(g, lane, j, off, lf, ne);
      const float w = param_or_zero(params, idx);
      reinterpret_cast<__bf16*>(packed)[e] = SPLIT ? split_half(w, (e >> 9) & 1) : (__bf16)w;
    } else {
      float* bias = reinterpret_cast<float*>(packed + (SPLIT ? kNgpSplitBiasOff : kNgpPackBiasOff));
      bias[e - total_w] = param_or_zero(params, ngp_bias_index(e - total_w, off));
    }
  }
}

}  // namespace lnrf

using namespace lnrf;

static bool ngp_supported(const lnrf_ngp_mlp_desc* d) {
  return d && d->hidden_dim == kNgpHidden && d->density_dim == kNgpDensityDim && d->density_layers == 1 &&
         d->color_layers == 2 && d->d_freqs == 4 && d->enc_dim >= 1 && d->enc_dim <= 32;
}
static NgpOffsets ngp_offsets(const lnrf_ngp_mlp_desc* d) { return ngp_offsets((int)d->enc_dim, d->dense_offset); }
// The kernels exist for NE = 1 and 2 k-steps of encoding (L*F <= 16 / <= 32): launch(integral_constant<int, NE>) -> rc
template <class F>
static int ngp_with_ne(const lnrf_ngp_mlp_desc* d, F&& launch) {
  return ngp_ne((int)d->enc_dim) == 1 ? launch(Int<1>{}) : launch(Int<2>{});
}
#define NGP_REQUIRE_SUPPORTED(fn)                                                                          \
  if (!ngp_supported(desc)) {                                                                              \
    set_error(fn ": only InstantNGPModel{hidden 64, density_dim 16, 1 density layer, 2 color layers, "    \
                 "d_freqs 4, L*F <= 32} is fused");                                                        \
    return LNRF_ERR_UNSUPPORTED;                                                                           \
  }

extern "C" int64_t lnrf_ngp_mlp_packed_bytes(const lnrf_ngp_mlp_desc* desc) {
  return ngp_supported(desc) ? kNgpPackBytes : -1;
}
static int64_t ngp_lmax_bytes(int64_t n_tiles) { return (n_tiles + kWaves - 1) / kWaves * 16 * (int64_t)sizeof(float); }

// scratch = [partial dW rows of the persistent backward] then one row of 16 per-level maxima per workgroup.  At most
// kNgpMaxPersistent workgroups form partial rows.
constexpr int kNgpMaxPersistent = 512;
static int ngp_pstride(const lnrf_ngp_mlp_desc* d) { return (ngp_dense_params((int)d->enc_dim) + 63) / 64 * 64; }
static int64_t ngp_lmax_off(const lnrf_ngp_mlp_desc* d, int64_t n_tiles) {
  int64_t rows = n_tiles / kWaves;
  if (rows > kNgpMaxPersistent) rows = kNgpMaxPersistent;
  const int64_t bytes = rows * kNgpMaxParts * ngp_pstride(d) * (int64_t)sizeof(float);
  return (bytes + 255) / 256 * 256;
}

extern "C" int64_t lnrf_ngp_mlp_scratch_bytes(const lnrf_ngp_mlp_desc* desc, int64_t m) {
  return ngp_supported(desc) ? ngp_lmax_off(desc, padded_tiles(m)) + ngp_lmax_bytes(padded_tiles(m)) : -1;
}

extern "C" int lnrf_ngp_mlp_pack(const lnrf_ngp_mlp_desc* desc, const float* params, void* packed,
                                 lnrf_stream_t stream) {
  NGP_REQUIRE_SUPPORTED("lnrf_ngp_mlp_pack");
  LNRF_CHECK_ARG(params && packed, "null pointer");
  LNRF_CHECK_ARG(desc->dense_offset >= 0, "bad dense_offset");
  hipLaunchKernelGGL(ngp_pack_kernel<false>, dim3(64), dim3(256), 0, as_stream(stream), params, ngp_offsets(desc),
                     (int)desc->enc_dim, ngp_ne((int)desc->enc_dim), (char*)packed);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int64_t lnrf_ngp_mlp_packed_split_bytes(const lnrf_ngp_mlp_desc* desc) {
  return ngp_supported(desc) ? kNgpSplitBytes : -1;
}

extern "C" int lnrf_ngp_mlp_pack_split(const lnrf_ngp_mlp_desc* desc, const float* params, void* packed_split,
                                       lnrf_stream_t stream) {
  NGP_REQUIRE_SUPPORTED("lnrf_ngp_mlp_pack_split");
  LNRF_CHECK_ARG(params && packed_split, "null pointer");
  LNRF_CHECK_ARG(desc->dense_offset >= 0, "bad dense_offset");
  hipLaunchKernelGGL(ngp_pack_kernel<true>, dim3(64), dim3(256), 0, as_stream(stream), params, ngp_offsets(desc),
                     (int)desc->enc_dim, ngp_ne((int)desc->enc_dim), (char*)packed_split);
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_ngp_mlp_fwd_split(const lnrf_ngp_mlp_desc* desc, const void* packed_split, const float* enc_t,
                                      const float* d, int64_t m, float* density, float* rgb, lnrf_stream_t stream) {
  NGP_REQUIRE_SUPPORTED("lnrf_ngp_mlp_fwd_split");
  LNRF_CHECK_ARG(m >= 0, "bad m");
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(packed_split && enc_t && d && density && rgb, "null pointer");
  const int64_t n_tiles = padded_tiles(m);
  int cus = 0;
  if (int rc = cu_count(&cus)) return rc;
  int64_t nb = n_tiles / kWaves;
  if (nb > 2 * (int64_t)cus) nb = 2 * (int64_t)cus;  // persistent: the stream is staged in LDS once per workgroup
  hipStream_t st = as_stream(stream);
  const int rc = ngp_with_ne(desc, [&](auto ne_) {
    constexpr int NE = decltype(ne_)::value;
    if (int rc = set_max_dynamic_lds(ngp_mlp_fwd_split_kernel<NE>, kNgpSplitBytes)) return rc;
    hipLaunchKernelGGL((ngp_mlp_fwd_split_kernel<NE>), dim3((unsigned)nb), dim3(kThreads), kNgpSplitBytes, st,
                       (const char*)packed_split, enc_t, d, (int)desc->enc_dim, m, n_tiles, density, rgb);
    return (int)LNRF_OK;
  });
  if (rc) return rc;
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_ngp_mlp_fwd(const lnrf_ngp_mlp_desc* desc, const void* packed, const float* enc_t,
                                const float* d, int64_t m, float* density, float* rgb, lnrf_stream_t stream) {
  NGP_REQUIRE_SUPPORTED("lnrf_ngp_mlp_fwd");
  LNRF_CHECK_ARG(m >= 0, "bad m");
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(packed && enc_t && d && density && rgb, "null pointer");
  const int64_t n_tiles = padded_tiles(m);
  const dim3 grid((unsigned)((n_tiles + kWaves - 1) / kWaves)), block(kThreads);
  hipStream_t st = as_stream(stream);
  const int rc = ngp_with_ne(desc, [&](auto ne_) {
    constexpr int NE = decltype(ne_)::value;
    if (int rc = set_max_dynamic_lds(ngp_mlp_kernel<NE, false>, kNgpLds)) return rc;
    hipLaunchKernelGGL((ngp_mlp_kernel<NE, false>), grid, block, kNgpLds, st, (const char*)packed, enc_t, d,
                       (int)desc->enc_dim, m, n_tiles, density, rgb, nullptr, nullptr, nullptr);
    return (int)LNRF_OK;
  });
  if (rc) return rc;
  LNRF_LAUNCH_CHECK();
  return LNRF_OK;
}

extern "C" int lnrf_ngp_mlp_bwd(const lnrf_ngp_mlp_desc* desc, const void* packed, const float* enc_t,
                                const float* d, const float* g_density, const float* g_rgb, int64_t m,
                                void* scratch, float* g_enc_t, float* level_absmax, float* grads,
                                lnrf_stream_t stream) {
  NGP_REQUIRE_SUPPORTED("lnrf_ngp_mlp_bwd");
  LNRF_CHECK_ARG(m >= 0, "bad m");
  if (m == 0) return LNRF_OK;
  LNRF_CHECK_ARG(packed && enc_t && d && g_density && g_rgb && scratch && g_enc_t && grads, "null pointer");
  const int64_t n_tiles = padded_tiles(m);
  hipStream_t st = as_stream(stream);
  // per-workgroup rows of level maxima live behind the partial dW rows in the scratch buffer
  float* lmax_parts = level_absmax ? reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) +
                                                              ngp_lmax_off(desc, n_tiles))
                                   : nullptr;
  const int n_levels = desc->enc_dim / 2;
  // weight-gradient problems (five Dense layers): where each kernel's rows and columns sit in the gradient vector
  const NgpOffsets off = ngp_offsets(desc);
  const NgpWgradArgs a = ngp_wgrad_args(off, desc->enc_dim);
  // one persistent workgroup per CU forms the weight gradients itself (no dumps, no second launch)
  int cus = 0;
  if (int rc = cu_count(&cus)) return rc;
  int64_t nb = n_tiles / kWaves;
  if (nb > cus) nb = cus;
  if (nb > kNgpMaxPersistent) nb = kNgpMaxPersistent;
  const dim3 pgrid((unsigned)nb), block(kThreads);
  // partial dW rows (workgroup, k-part) at the front of the scratch buffer
  const NgpPartsPlan plan = ngp_parts_plan(off, desc->dense_offset);
  const int n_params = ngp_dense_params((int)desc->enc_dim);
  const int pstride = ngp_pstride(desc);
  float* wparts = reinterpret_cast<float*>(scratch);
  const int rc = ngp_with_ne(desc, [&](auto ne_) {
    constexpr int NE = decltype(ne_)::value;
    if (int rc = set_max_dynamic_lds(ngp_mlp_kernel<NE, true>, kNgpFusedLds)) return rc;
    hipLaunchKernelGGL((ngp_mlp_kernel<NE, true>), pgrid, block, kNgpFusedLds, st, (const char*)packed, enc_t, d,
                       (int)desc->enc_dim, m, n_tiles, nullptr, nullptr, g_density, g_rgb, g_enc_t,
                       lmax_parts, a, wparts, pstride, (int64_t)desc->dense_offset);
    return (int)LNRF_OK;
  });
  if (rc) return rc;
  LNRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(ngp_wparts_reduce_kernel, dim3((unsigned)((n_params + 31) / 32)), dim3(256), 0, st, wparts,
                     (int)nb, pstride, n_params, plan, grads + desc->dense_offset);
  LNRF_LAUNCH_CHECK();
  if (lmax_parts) {
    hipLaunchKernelGGL(ngp_level_max_kernel, dim3(1), dim3(256), 0, st, lmax_parts, (int)nb, n_levels,
                       reinterpret_cast<unsigned*>(level_absmax));
    LNRF_LAUNCH_CHECK();
  }
  return LNRF_OK;
}

#ifdef LNRF_TIMELINE
// debug library only (tools/build_timeline.sh): where the stamped workgroup of the fused backward writes its stamps
extern "C" int lnrf_debug_set_ngp_timeline(void* buf) {
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(lnrf::g_ngp_timeline_buf), &buf, sizeof(buf));
  return e == hipSuccess ? LNRF_OK : lnrf::hip_fail(e, "hipMemcpyToSymbol(g_ngp_timeline_buf)");
}
#endif
