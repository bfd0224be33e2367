/*
 * lnrf.h — C ABI of the MI355X-native NeRF volume-rendering hot path (liblnrf.so).
 *
 * The reference (unixpickle/learn-nerf) has no FFI: its hot path is Python on JAX
 * (SURVEY.md §8b).  This header is the boundary a maintainer binds instead of
 * jax.jit: every entry point names the reference function (file:line under
 * /root/reference/learn_nerf) whose arithmetic it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP types in signatures
 *     (lnrf_stream_t is a hipStream_t passed as void*; NULL = default stream).
 *   - every pointer is DEVICE memory unless marked (host); the caller owns every
 *     buffer, the library allocates nothing persistent.
 *   - all work is enqueued asynchronously on the given stream; no hidden sync.
 *   - return 0 = ok, <0 = lnrf argument/shape error, >0 = hipError_t passthrough;
 *     message via lnrf_last_error() (thread-local).  Never throws or aborts.
 *   - arrays are row-major contiguous fp32 unless noted; rays are
 *     (origin[3], direction[3]) with `ray_stride` floats between consecutive rays
 *     (6 for [N,2,3] batches, 9 for [N,3,3] training batches with colours).
 *   - sampling noise: `u` (explicit uniforms in [0,1)) or, when u == NULL, the
 *     Philox4x32-10 stream (seed, stream_id, element (ray_offset+n)*count+i)
 *     documented in oracle/philox.py.
 */
#ifndef LNRF_H
#define LNRF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lnrf_stream_t;

#define LNRF_VERSION 200 /* 0.2.0 */

#define LNRF_OK 0
#define LNRF_ERR_ARG (-1)
#define LNRF_ERR_SHAPE (-2)
#define LNRF_ERR_UNSUPPORTED (-3)

/* activation codes for the dense kernels */
#define LNRF_ACT_NONE 0
#define LNRF_ACT_RELU 1
#define LNRF_ACT_SOFTPLUS 2
#define LNRF_ACT_TANH 3
#define LNRF_ACT_EXP 4
#define LNRF_ACT_SIGMOID 5

int lnrf_version(void);
const char* lnrf_last_error(void);

/* ------------------------------------------------------------------ rays ---- */

/* ray_t_range (render.py:346-389) + NeRFRenderer.t_range (render.py:93-111) fused with
 * RaySamples.stratified_sampling (render.py:121-143).  bbox_min/max: (host) 3 floats.
 * count may be 0 (then ts/u are ignored).  mask: 1 byte per ray (0/1). */
int lnrf_ray_aabb_stratified(const float* rays, int64_t ray_stride, int64_t n_rays,
                             const float* bbox_min, const float* bbox_max, float min_t_range,
                             float epsilon, int32_t count, const float* u, uint64_t seed,
                             uint32_t stream_id, int64_t ray_offset, float* t_min, float* t_max,
                             uint8_t* mask, float* ts, lnrf_stream_t stream);

/* CameraView.bare_rays (dataset.py:52-78): all rays of a pinhole view in raster order, rays[H*W, 2, 3]
 * (device).  origin / axes: (host) 3 floats each; fields of view in radians. */
int lnrf_camera_rays(const float* origin, const float* x_axis, const float* y_axis, const float* z_axis,
                     float x_fov, float y_fov, int32_t width, int32_t height, float* rays,
                     lnrf_stream_t stream);

/* The shuffled batch iterator's row movement (ShuffledDataset.iterate_batches, dataset.py:222-240: the reference
 * permutes a shard and concatenates it to the pending rows on the host for every batch): with the shards resident in
 * HBM, out[i, :] = src[idx[i], :] for i < n, rows of row_floats fp32 (9 = origin, direction, colour).  idx: int32
 * row numbers in [0, n_src); a row number outside that range writes zeros (never reads out of bounds). */
int lnrf_gather_rows(const float* src, int64_t n_src, int32_t row_floats, const int32_t* idx, int64_t n,
                     float* out, lnrf_stream_t stream);

/* RaySamples.stratified_sampling (render.py:121-143) from given t_min/t_max. */
int lnrf_stratified(const float* t_min, const float* t_max, int64_t n_rays, int32_t count,
                    const float* u, uint64_t seed, uint32_t stream_id, int64_t ray_offset,
                    float* ts, lnrf_stream_t stream);

/* RaySamples.points (render.py:145-153) + direction tile (render.py:319):
 * x[n,t,:] = o + d*ts[n,t];  dirs[n,t,:] = d.  Either output may be NULL. */
int lnrf_ray_points(const float* rays, int64_t ray_stride, const float* ts, int64_t n_rays,
                    int32_t t, float* points, float* dirs, lnrf_stream_t stream);

/* RaySamples.fine_sampling (render.py:211-257): termination probs of the coarse pass ->
 * inverse-CDF (jnp.interp) at stratified u' -> optional sort with the coarse ts.
 * ts_out is [N, tc+tf] when combine != 0 else [N, tf]. */
int lnrf_fine_sample(const float* ts_c, const float* t_min, const float* t_max,
                     const float* density_c, int64_t n_rays, int32_t tc, int32_t tf, float eps,
                     int32_t combine, const float* u, uint64_t seed, uint32_t stream_id,
                     int64_t ray_offset, float* ts_out, lnrf_stream_t stream);

/* RaySamples.starts / ends (render.py:259-265): bin edges [N,T] each (either may be NULL). */
int lnrf_bin_edges(const float* ts, const float* t_min, const float* t_max, int64_t n_rays,
                   int32_t t, float* starts, float* ends, lnrf_stream_t stream);

/* RaySamples.termination_probs (render.py:270-287): probs [N, T+1]. */
int lnrf_termination_probs(const float* ts, const float* t_min, const float* t_max,
                           const float* density, int64_t n_rays, int32_t t, float* probs,
                           lnrf_stream_t stream);

/* RaySamples.render_rays / render_alpha / average_aux_losses and the free render_rays
 * (render.py:155-209, 293-343) in one pass per ray:
 *   outputs[N,3] = mask ? sum_t probs*rgb + probs_T*background : background
 *   alphas[N]    = mask ? 1 - probs_T : 0
 *   coords[N,3]  = mask ? sum_t probs*(o + d*ts) : 0
 *   aux_sum[N,n_aux] = mask ? sum_t probs*aux : 0           (aux [N,T,n_aux], may be NULL)
 * If targets != NULL (stride target_stride floats per ray), sum over rays/channels of
 * (outputs-targets)^2 is atomically added to *sq_err (train.py:141-142 numerator).
 * Any output pointer may be NULL. */
int lnrf_composite_fwd(const float* rays, int64_t ray_stride, const float* ts, const float* t_min,
                       const float* t_max, const uint8_t* mask, const float* density,
                       const float* rgb, const float* aux, int32_t n_aux, const float* background,
                       int64_t n_rays, int32_t t, float* outputs, float* alphas, float* coords,
                       float* aux_sum, const float* targets, int64_t target_stride, float* sq_err,
                       lnrf_stream_t stream);

/* Backward of the compositing integral for the loss of TrainLoop.losses (train.py:140-151).
 * Upstream gradient per ray: g_out[N,3] if non-NULL, else out_scale*(outputs - targets)
 * (i.e. d/d outputs of mean squared error when out_scale = 2/(3*N_global)).
 * g_aux_w: (host) n_aux weights = d total / d aux_sum[n,k] (same for every ray).
 * Writes g_density[N,T], g_rgb[N,T,3], g_aux[N,T,n_aux]; accumulates g_background[3] (may be NULL) in a fixed
 * order: per-workgroup partial sums in `scratch` (lnrf_composite_bwd_scratch_bytes(n_rays) bytes, 16-byte aligned),
 * folded by a second launch — bit-reproducible.  No gradient flows to ts (fine sampling uses stop_gradient,
 * render.py:76; stratified ts do not depend on parameters). */
int64_t lnrf_composite_bwd_scratch_bytes(int64_t n_rays);
int lnrf_composite_bwd_det(const float* ts, const float* t_min, const float* t_max, const uint8_t* mask,
                           const float* density, const float* rgb, const float* aux, int32_t n_aux,
                           const float* background, int64_t n_rays, int32_t t, const float* g_out, const float* outputs,
                           const float* targets, int64_t target_stride, float out_scale, const float* g_aux_w,
                           float* g_density, float* g_rgb, float* g_aux, float* g_background, void* scratch,
                           int64_t scratch_bytes, lnrf_stream_t stream);

/* Distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15) on the compositing weights of each ray, and its
 * gradient to the densities.  With the bins, a_i and A_i of lnrf_termination_probs, w_i = probs[n, i] for i < T (the
 * background's share takes no part), r = t_max - t_min, m_i = ((start_i + end_i) / 2 - t_min) / r, d_i = delta_i / r:
 *   L_n = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
 * loss[N] = L_n is written (may be NULL); g_density[N,T] += grad_scale * dL_n/dsigma (may be NULL; not both).
 * A ray with mask == 0, r <= 0 or a non-finite r has loss 0 and its g_density row is left untouched.  No gradient
 * flows to ts, t_min or t_max.  One launch, no scratch; each ray's result depends on that ray alone (bit-reproducible). */
int lnrf_distortion(const float* ts, const float* t_min, const float* t_max, const uint8_t* mask,
                    const float* density, int64_t n_rays, int32_t t, float grad_scale, float* loss,
                    float* g_density, lnrf_stream_t stream);

/* ----------------------------------------------------------- generic dense ---- */

/* sinusoidal_emb (model.py:65-77): out[m, col_off + c*2F + {f | F+f}] = sin|cos(2^f x[m,c]).
 * x has `dims` columns (row stride ldx), out row stride ldo. */
int lnrf_sinusoidal_emb(const float* x, int64_t ldx, int64_t m, int32_t dims, int32_t freqs,
                        float* out, int64_t ldo, int64_t col_off, lnrf_stream_t stream);

/* Operand precision of the generic dense path (lnrf_dense_fwd / _bwd_input / _bwd_weight / lnrf_gemm_f32), a
 * thread-local mode like a rounding mode.  LNRF_DENSE_FP32 (default): exact fp32 products on the f32 MFMA, the
 * arithmetic of the reference's jnp.float32 Dense layers.  LNRF_DENSE_BF16: both operands of every product are
 * rounded to bf16 (round-to-nearest-even) when staged, fp32 accumulate / bias / activation — the arithmetic of the
 * fused kernels, for the models that have no fused kernel (RefNERFModel, InstantNGPRefNERFModel, non-default
 * shapes). */
#define LNRF_DENSE_FP32 0
#define LNRF_DENSE_BF16 1
int lnrf_set_dense_precision(int32_t precision);
int32_t lnrf_get_dense_precision(void);

/* flax.linen.Dense + activation (model.py:51-60): y = act(x[M,K] @ w[K,N] + b[N]).
 * fp32 in / fp32 accumulate on the f32 MFMA.  ldx/ldy row strides (concat without copies).
 * b may be NULL. */
int lnrf_dense_fwd(const float* x, int64_t ldx, const float* w, const float* b, int32_t act,
                   float* y, int64_t ldy, int64_t m, int32_t k, int32_t n, lnrf_stream_t stream);

/* g_pre = g_y * act'(y) elementwise in place on g (y = saved activation output). */
int lnrf_act_bwd(float* g, int64_t ldg, const float* y, int64_t ldy, int32_t act, int64_t m,
                 int32_t n, lnrf_stream_t stream);

/* g_x[M,K] (+)= g_y[M,N] @ w[K,N]^T. accumulate != 0 adds into g_x. */
int lnrf_dense_bwd_input(const float* gy, int64_t ldgy, const float* w, float* gx, int64_t ldgx,
                         int32_t accumulate, int64_t m, int32_t k, int32_t n, lnrf_stream_t stream);

/* lnrf_dense_bwd_input fused with the activation backward of the layer below:
 * gx[i][c] (+)= (sum_r gy[i][r] w[c][r]) * act'(y_below[i][c]) for c < n_gated (act' expressed through the activation's
 * OUTPUT, as lnrf_act_bwd), plain input gradient for the other columns (e.g. the x_emb part of a concatenated input).
 * Saves one read-modify-write pass over gx per layer. */
int lnrf_dense_bwd_input_gated(const float* gy, int64_t ldgy, const float* w, const float* y_below, int64_t ldy,
                               int32_t act_below, int32_t n_gated, float* gx, int64_t ldgx, int32_t accumulate,
                               int64_t m, int32_t k, int32_t n, lnrf_stream_t stream);
/* lnrf_dense_fwd whose result is multiplied by act_gate'(y_gate[i][j]): the masked forward product of the
 * second-order (normal) chain of ref_nerf.py:38-43, tbar_l = relu'(h_l) * (tbar_{l-1} W_l). */
int lnrf_dense_fwd_gated(const float* x, int64_t ldx, const float* w, const float* b, int32_t act,
                         const float* y_gate, int64_t ldg, int32_t act_gate, float* y, int64_t ldy, int64_t m,
                         int32_t k, int32_t n, lnrf_stream_t stream);

/* g_w[K,N] += x[M,K]^T @ g_y[M,N];  g_b[N] += sum_m g_y (g_b may be NULL).
 * x == NULL and gw == NULL: bias gradient only.
 * FIXED summation order (bit-reproducible): the splits of the reduction over m leave their partial sums in `scratch`
 * (lnrf_dense_bwd_weight_scratch_bytes(m, k, n) bytes; k = 0 when x / gw are null) and a second launch adds them in
 * order.  What the package's exact-fp32 path uses (reference: jax.grad through nn.Dense, model.py:51-60, is
 * deterministic on one device). */
int64_t lnrf_dense_bwd_weight_scratch_bytes(int64_t m, int32_t k, int32_t n);
int lnrf_dense_bwd_weight_det(const float* x, int64_t ldx, const float* gy, int64_t ldgy, float* gw, float* gb,
                              int64_t m, int32_t k, int32_t n, void* scratch, int64_t scratch_bytes,
                              lnrf_stream_t stream);

/* General strided fp32 GEMM on the f32 MFMA behind the dense entry points above:
 *   C[i*ldc + j] (op)= sum_r A[i*sa_i + r*sa_r] * B[r*sb_r + j*sb_j],  i < I, j < J, r < R
 * mode 0: C = act(sum + bias[j]);  1: C += sum;  2: atomic C += sum with the reduction split over
 * `splits` workgroups (0 = choose).  Lets a layer consume a transposed operand (e.g. the feature-major
 * hash-grid encoding) without a copy.
 * Any strides and any 4-byte-aligned pointers are accepted: strides and alignment only select the kernel
 * (csrc/dense_plan.h), and every kernel gives the same result to within the rounding of an fp32 sum,
 *   |C - C_exact| <= (R + splits + 2) 2^-23 (|A| |B|)_ij + 2^-23 |C_exact|
 * (C_exact: the product of the operands as multiplied, i.e. rounded to bf16 under LNRF_DENSE_BF16).  Nothing outside
 * the I x J elements of C is written, and nothing outside the I x R elements of A and the R x J elements of B (rows
 * and columns beyond the extents, the padding between rows, elements skipped by a stride) influences the result.
 * tests/test_gpu_gemm_paths.py pins this for every kernel the plan can select. */
int lnrf_gemm_f32(const float* a, int64_t sa_i, int64_t sa_r, const float* b, int64_t sb_r, int64_t sb_j,
                  float* c, int64_t ldc, const float* bias, int32_t act, int32_t mode, int64_t i_rows,
                  int32_t j_cols, int64_t r_depth, int32_t splits, lnrf_stream_t stream);

/* lnrf_gemm_f32 mode 2 (C += A B, reduction split over workgroups) with a FIXED summation order: C has contiguous
 * rows (ldc == J); the splits leave their partial tiles in `scratch` (lnrf_gemm_f32_det_scratch_bytes bytes) and a
 * second launch adds them in order — bit-reproducible, unlike the atomic form. */
int64_t lnrf_gemm_f32_det_scratch_bytes(int64_t i_rows, int32_t j_cols, int64_t r_depth);
int lnrf_gemm_f32_det(const float* a, int64_t sa_i, int64_t sa_r, const float* b, int64_t sb_r, int64_t sb_j, float* c,
                      int64_t i_rows, int32_t j_cols, int64_t r_depth, void* scratch, int64_t scratch_bytes,
                      lnrf_stream_t stream);

/* --------------------------------------------------- hash-grid encoding ---- */

/* MultiresHashTableEncoding / HashTableEncoding (instant_ngp.py:92-208). Tables of all levels live in one
 * flat fp32 buffer; level l is [table_size[l], feature_dim] row-major at table_offset[l] (floats). */
typedef struct {
  int32_t n_levels, feature_dim, smooth, pad_;
  float bbox_min[3], bbox_max[3];
  int32_t grid_size[32];
  int32_t table_size[32];
  int64_t table_offset[32];
  int32_t hashed[32]; /* 1 when grid_size^3 > requested table size (instant_ngp.py:178) */
} lnrf_hashgrid_desc;

/* enc_t[(level*F + f) * m_total + m] = sum over the 8 cell corners of weight * table[index][f]
 * (feature-major output, [L*F][M]). x: [M,3] points. */
int lnrf_hashgrid_fwd(const lnrf_hashgrid_desc* desc, const float* tables, const float* x, int64_t m,
                      float* enc_t, lnrf_stream_t stream);

/* g_tables += scatter of g_enc_t (same layout as enc_t) through the same indices/weights, with caller-provided
 * scratch (lnrf_hashgrid_bwd_scratch_bytes): every level of at most 256 4096-entry table slices, hashed or dense, is
 * reduced without global float atomics (bin by 4096-entry slice, then one workgroup per bucket, several for a large
 * one, accumulates in LDS).  u == NULL: value weights (first-order gradient); u [M,3]: derivative weights (see bwd_dir).
 * level_absmax (optional, u == NULL only): n_levels floats, level_absmax[l] >= max |g_enc_t rows 2l, 2l+1|;
 * lnrf_ngp_mlp_bwd produces it while writing g_enc_t.  WITH it the contributions are binned as 26-bit fixed point of
 * that bound (8-byte tuples: resolution 2^-25 of the level's bound per contribution — a QUANTISED scatter, the fused
 * bf16 path's; values beyond a too-small bound saturate).  NULL: 12-byte fp32 tuples, the level maximum is found while
 * binning and the reduce pass sums in 64-bit fixed point at 2^-46 of it per contribution — the exact-fp32 path's
 * scatter (instant_ngp.py:211-224 under jax.grad).  Either way NaN / Inf contributions reach the table through float
 * atomics, as a floating-point scatter-add would propagate them.
 * scratch == NULL, and a larger table, fall back to float atomics (pre-reduced in LDS for tables of up to 64 8192-entry
 * slices, except a hashed table of one). */
int64_t lnrf_hashgrid_bwd_scratch_bytes(const lnrf_hashgrid_desc* desc, int64_t m);
int lnrf_hashgrid_bwd_bucketed(const lnrf_hashgrid_desc* desc, const float* x, const float* u, int64_t m,
                               const float* g_enc_t, const float* level_absmax, float* g_tables, void* scratch,
                               int64_t scratch_bytes, lnrf_stream_t stream);

/* Input-derivative maps of the encoding, needed when a Ref-NeRF head sits on the hash grid
 * (InstantNGPRefNERFModel, instant_ngp.py:57-89: normals = -d out[:,0]/dx, ref_nerf.py:38-43):
 *   jvp:        enc_t-shaped (d enc / d x) u,            u [M,3]
 *   input_grad: g_x[M,3] = (d enc / d x)^T g_enc
 *   bwd_dir:    g_tables += d/d tables of < (d enc / d x) u , g_enc >   (second-order term)
 * Boundary convention of all three: the derivative along an axis is zero when the point lies on or outside the
 * bounding box on that axis (x <= bbox_min or x >= bbox_max: the clip of instant_ngp.py:138-140 has zero slope
 * there; exactly 0.0 in input_grad, and in jvp for a u along that axis).  With smooth == 0 the encoding is only
 * piecewise differentiable: the maps return the one-sided derivative of the cell that contains the point (the cell
 * the forward pass interpolates in); with smooth == 1 the derivative is continuous across cell faces.
 * table_size[l] need not be a power of two, in any of the hash-grid entry points: hashed levels then index with
 * hash % table_size (a mask for powers of two), and the scatters handle a ragged last table slice. */
int lnrf_hashgrid_jvp(const lnrf_hashgrid_desc* desc, const float* tables, const float* x, const float* u,
                      int64_t m, float* enc_t, lnrf_stream_t stream);
int lnrf_hashgrid_input_grad(const lnrf_hashgrid_desc* desc, const float* tables, const float* x, int64_t m,
                             const float* g_enc_t, float* g_x, lnrf_stream_t stream);
int lnrf_hashgrid_bwd_dir(const lnrf_hashgrid_desc* desc, const float* x, const float* u, int64_t m,
                          const float* g_enc_t, float* g_tables, lnrf_stream_t stream);

/* ------------------------------------------------------------- Ref-NeRF ---- */

/* Transpose / tangent of d sinusoidal_emb / d x (model.py:65-77), needed by the analytic normals
 * -d out[:,0]/dx of RefNERFBase (ref_nerf.py:38-43) and by their second-order term:
 *   bwd: g_x[m,c]   = sum_f 2^f (cos(2^f x) g_emb[sin f] - sin(2^f x) g_emb[cos f])
 *   jvp: v_emb[...] = (d emb / d x) u,  u [M,dims]. */
int lnrf_sinusoidal_emb_bwd(const float* x, int64_t ldx, int64_t m, int32_t dims, int32_t freqs,
                            const float* g_emb, int64_t ldg, int64_t col_off, float* g_x,
                            lnrf_stream_t stream);
int lnrf_sinusoidal_emb_jvp(const float* x, int64_t ldx, int64_t m, int32_t dims, int32_t freqs,
                            const float* u, float* v_emb, int64_t ldv, int64_t col_off,
                            lnrf_stream_t stream);

/* integrated_directional_encoding (ref_nerf.py:121-143) on spherical_harmonic (:146-311):
 * out[M, sh_degree^2]; roughness [M] or NULL (plain spherical harmonics). */
int lnrf_integrated_directional_encoding(int32_t sh_degree, const float* coords, const float* roughness,
                                         int64_t m, float* out, lnrf_stream_t stream);

/* RefNERFBase.__call__ between spatial_block and directional_block (ref_nerf.py:41-63, 72-75).
 * spatial: [M, >=9] (row stride lds): density logit, diffuse(3), spectral, roughness, normal(3).
 * nraw [M,3] = -d sum(out[:,0]) / dx (unnormalised analytic normal), d [M,3] view directions.
 * Writes density[M], diffuse[M,3], spectral[M], tail[m, 0..sh^2] = IDE of the reflection direction,
 * tail[m, sh^2] = -d.n  (the columns appended to spatial_out for the directional block), and
 * aux[M,2] = (normal_mse, neg_normal) per sample. */
int lnrf_refnerf_head_fwd(const float* spatial, int64_t lds, const float* nraw, const float* d, int64_t m,
                          int32_t sh_degree, float* density, float* diffuse, float* spectral, float* tail,
                          int64_t ld_tail, float* aux, lnrf_stream_t stream);
/* VJP of the above: g_spatial[m, 0..8] += ..., g_nraw[M,3] = ... */
int lnrf_refnerf_head_bwd(const float* spatial, int64_t lds, const float* nraw, const float* d, int64_t m,
                          int32_t sh_degree, const float* g_density, const float* g_diffuse,
                          const float* g_spectral, const float* g_tail, int64_t ld_tail, const float* g_aux,
                          float* g_spatial, int64_t ldgs, float* g_nraw, lnrf_stream_t stream);

/* full_color = linear_rgb_to_srgb(_leaky_clip(sigmoid(dir_out) * spectral + diffuse)) * 2 - 1
 * (ref_nerf.py:64-71, 110-118, 320-326) and its VJP. */
int lnrf_refnerf_color_fwd(const float* dir_out, const float* spectral, const float* diffuse, int64_t m,
                           float* rgb, lnrf_stream_t stream);
int lnrf_refnerf_color_bwd(const float* dir_out, const float* spectral, const float* diffuse, int64_t m,
                           const float* g_rgb, float* g_dir_out, float* g_spectral, float* g_diffuse,
                           lnrf_stream_t stream);

/* ------------------------------------------------ fused NeRF MLP (bf16 MFMA) ---- */

/* NeRFModel hyper-parameters (model.py:35-40). The fused kernels support the reference
 * default {5,4,256,128,10,4}; anything else returns LNRF_ERR_UNSUPPORTED (use the dense path). */
typedef struct {
  int32_t input_layers, mid_layers, hidden_dim, color_layer_dim, x_freqs, d_freqs;
} lnrf_nerf_shape;

/* number of fp32 parameters in Flax creation order (Dense_i.kernel[in,out], Dense_i.bias). */
int64_t lnrf_nerf_param_count(const lnrf_nerf_shape* shape);
/* bytes of the opaque MFMA-fragment-ordered bf16 copy produced by lnrf_nerf_pack_weights. */
int64_t lnrf_nerf_packed_bytes(const lnrf_nerf_shape* shape);
/* bytes of the saved-activation buffer for m evaluations (forward -> backward). */
int64_t lnrf_nerf_save_bytes(const lnrf_nerf_shape* shape, int64_t m);
/* bytes of backward scratch for m evaluations: the pre-activation gradients in fragment order (written by
 * lnrf_nerf_mlp_bwd_chain, read by lnrf_nerf_mlp_bwd_weights) followed by the partial-sum slabs that
 * lnrf_nerf_mlp_bwd_weights writes and folds (deterministic reduction instead of fp32 atomics). */
int64_t lnrf_nerf_bwd_scratch_bytes(const lnrf_nerf_shape* shape, int64_t m);

/* Repack fp32 Flax-layout parameters into the bf16 fragment streams (forward + transposed). */
int lnrf_nerf_pack_weights(const lnrf_nerf_shape* shape, const float* params, void* packed,
                           lnrf_stream_t stream);

/* NeRFModel.__call__ (model.py:43-62) for M evaluations, positional encoding included.
 * Points come either from explicit x[M,3], d[M,3] (rays == NULL) or, without materialising
 * them (render.py:318-319), from rays + ts: evaluation m = n*t + i is x = o_n + d_n*ts[n,i].
 * density[M] >= 0, rgb[M,3] in (-1,1).  save (nullable): activations for the backward. */
int lnrf_nerf_mlp_fwd(const lnrf_nerf_shape* shape, const void* packed, const float* x,
                      const float* d, const float* rays, int64_t ray_stride, const float* ts,
                      int32_t t, int64_t m, float* density, float* rgb, void* save,
                      lnrf_stream_t stream);

/* The same forward for a backward by lnrf_nerf_mlp_bwd_ls / _ls2 (save must not be NULL): that backward takes the ReLU
 * masks of Dense_0..7 from the saved activations, so their mask slots in `save` are left unwritten (8 KiB per 32
 * evaluations less to store, ~1/4 fewer epilogue instructions).  A save written by this entry must NOT be handed to
 * lnrf_nerf_mlp_bwd_chain. */
int lnrf_nerf_mlp_fwd_ls(const lnrf_nerf_shape* shape, const void* packed, const float* x,
                         const float* d, const float* rays, int64_t ray_stride, const float* ts,
                         int32_t t, int64_t m, float* density, float* rgb, void* save,
                         lnrf_stream_t stream);

/* Split-precision ("bf16x3") evaluation of NeRFModel.__call__ (model.py:43-62), the render / evaluation path:
 * the reference computes this in fp32 (model.py:72, render.py:140); here every fp32 operand is carried as
 * a bf16 pair hi + lo and every product is hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation
 * (16 significant bits per operand; rendered RGB within 1e-3 of the fp32 reference, tests/test_gpu_nerf_mlp.py).
 * lnrf_nerf_packed_split_bytes: size of the opaque [hi,lo] fragment stream made by lnrf_nerf_pack_weights_split.
 * lnrf_nerf_mlp_fwd_split: same arguments as lnrf_nerf_mlp_fwd without the save buffer (inference only). */
int64_t lnrf_nerf_packed_split_bytes(const lnrf_nerf_shape* shape);
int lnrf_nerf_pack_weights_split(const lnrf_nerf_shape* shape, const float* params, void* packed_split,
                                 lnrf_stream_t stream);
int lnrf_nerf_mlp_fwd_split(const lnrf_nerf_shape* shape, const void* packed_split, const float* x,
                            const float* d, const float* rays, int64_t ray_stride, const float* ts,
                            int32_t t, int64_t m, float* density, float* rgb, lnrf_stream_t stream);

/* Backward of the above wrt the parameters, grads[param_count] += d L / d params given g_density[M], g_rgb[M,3]
 * (= d L / d outputs), the forward outputs and the save buffer, in two launches.
 * Part 1: input-gradient chain (what jax.grad does through model.py:49-60 back to front);
 * writes the pre-activation gradients of every Dense layer into scratch (fragment order). */
int lnrf_nerf_mlp_bwd_chain(const lnrf_nerf_shape* shape, const void* packed, const void* save,
                            const float* density, const float* rgb, const float* g_density,
                            const float* g_rgb, int64_t m, void* scratch, lnrf_stream_t stream);

/* Part 2: grads += X_l^T dy_l for every Dense kernel and sum_m dy_l for every bias.  Reads the gradient dump at
 * the start of scratch and uses the slab region behind it (lnrf_nerf_bwd_scratch_bytes covers both). */
int lnrf_nerf_mlp_bwd_weights(const lnrf_nerf_shape* shape, const void* save, void* scratch,
                              int64_t m, float* grads, lnrf_stream_t stream);

/* The same backward (jax.grad through model.py:43-62, as lnrf_nerf_mlp_bwd_chain + _bwd_weights) as a LAYER-STATIONARY pipeline
 * (csrc/nerf_bwd_ls.hip): a head launch (Dense_11, Dense_10, Dense_9 -> dz), then ONE persistent launch in which every
 * CU owns one of Dense_8 ... Dense_1 — W_l^T and the dW_l accumulators stay in its registers for the whole launch — and
 * the 32-evaluation tiles pass from CU to CU (dy handed over through write-through stores and flag words), then the
 * five small weight-gradient problems and a fixed-order fold of the per-pipeline partial sums (bit-reproducible).
 * grads += d L / d params.  scratch: lnrf_nerf_bwd_ls_scratch_bytes(shape, m) bytes; the 32-bit word at byte offset
 * lnrf_nerf_bwd_ls_status_offset(shape, m) is non-zero after the launch if a bounded hand-off wait gave up (gradients of
 * that call are then invalid).  lnrf_nerf_mlp_bwd_ls2 runs two models (train.py:141-142: coarse and fine) in the same
 * persistent launch, pipelines shared in proportion to their evaluations.
 * phases: 7 = the whole backward; a caller that wants to time the parts passes 1 (head launches), then 2 (the persistent
 * pipeline launch), then 4 (small weight-gradient problems + folds) with the same arguments, in that order. */
int64_t lnrf_nerf_bwd_ls_scratch_bytes(const lnrf_nerf_shape* shape, int64_t m);
int64_t lnrf_nerf_bwd_ls_status_offset(const lnrf_nerf_shape* shape, int64_t m);
int lnrf_nerf_mlp_bwd_ls(const lnrf_nerf_shape* shape, const void* packed, const void* save,
                         const float* density, const float* rgb, const float* g_density,
                         const float* g_rgb, int64_t m, void* scratch, float* grads, int32_t phases,
                         lnrf_stream_t stream);
int lnrf_nerf_mlp_bwd_ls2(const lnrf_nerf_shape* shape, const void* packed_a, const void* save_a,
                          const float* density_a, const float* rgb_a, const float* g_density_a,
                          const float* g_rgb_a, int64_t m_a, void* scratch_a, float* grads_a,
                          const void* packed_b, const void* save_b, const float* density_b,
                          const float* rgb_b, const float* g_density_b, const float* g_rgb_b, int64_t m_b,
                          void* scratch_b, float* grads_b, int32_t phases, lnrf_stream_t stream);

/* ---- fused spatial block of RefNERFModel (reference learn_nerf/ref_nerf.py:80-107; csrc/refnerf_fused.hip) ----
 * The spatial block of RefNERFModel is the NeRFModel trunk (Dense_0..8: 60 -> 256 x5, 316 -> 256, 256 x3, default
 * widths and x_freqs = 10 only; parameters in Flax creation order, so Dense_0..8 sit where they sit in NeRFModel's
 * vector).  These entries run it — and everything that differentiates through it — on the fused bf16-MFMA chain:
 *   lnrf_refnerf_trunk_pack     fp32 parameters -> opaque fragment streams (lnrf_refnerf_trunk_packed_bytes bytes)
 *   lnrf_refnerf_trunk_fwd      spatial_out[m, 0:256] (fp32, `ld` floats per row, rows 16-byte aligned) =
 *                               spatial_block(x) (ref_nerf.py:37); `save` (lnrf_nerf_save_bytes of the default
 *                               lnrf_nerf_shape) receives the bf16 activations and ReLU masks of the pass
 *   lnrf_refnerf_normal_pass    n_raw[m, 3] = -d spatial_out[:, 0] / dx (ref_nerf.py:38-43: the jax.grad inside
 *                               RefNERFBase.__call__); cdump (lnrf_nerf_bwd_scratch_bytes) keeps the chain states
 *                               (zero for the pad evaluations m .. of the last tiles, like every gradient dump)
 *   lnrf_refnerf_trunk_bwd      grads += d L / d Dense_0..8 given g_spatial = d L / d spatial_out [m, ld]
 *                               (first-order path, on the layer-stationary pipeline of lnrf_nerf_mlp_bwd_ls;
 *                               scratch: lnrf_refnerf_trunk_bwd_scratch_bytes(m))
 *   lnrf_refnerf_normal_bwd     grads += the second-order term: d L / d Dense_0..8 through n_raw, given
 *                               u = d L / d n_raw [m, 3] (jax.grad of a function that calls jax.grad, train.py:89-90
 *                               over ref_nerf.py:42; scratch: lnrf_nerf_save_bytes; the slab region behind the chain
 *                               states in cdump is used as workspace for the fixed-order weight-gradient fold)
 * Head and integrated directional encoding: lnrf_refnerf_head_*, lnrf_refnerf_color_*.  The 273 -> 128 -> 3 directional
 * block is fused as well: lnrf_refnerf_dir_* below (its streams are part of the same packed blob). */
int64_t lnrf_refnerf_trunk_packed_bytes(void);
int lnrf_refnerf_trunk_pack(const float* params, void* packed, lnrf_stream_t stream);
int lnrf_refnerf_trunk_fwd(const void* packed, const float* x, int64_t m, void* save, float* spatial_out,
                           int64_t ld, lnrf_stream_t stream);
int lnrf_refnerf_normal_pass(const void* packed, const void* save, const float* x, int64_t m, void* cdump,
                             float* nraw, lnrf_stream_t stream);
int64_t lnrf_refnerf_trunk_bwd_scratch_bytes(int64_t m);
int lnrf_refnerf_trunk_bwd(const void* packed, const void* save, const float* g_spatial, int64_t ld, int64_t m,
                           void* scratch, float* grads, lnrf_stream_t stream);
int lnrf_refnerf_normal_bwd(const void* packed, const void* save, const void* cdump, const float* x,
                            const float* u, int64_t m, void* scratch, float* grads, lnrf_stream_t stream);
/* Directional block of RefNERFModel (ref_nerf.py:100-107: Dense_9 273 -> 128 relu, Dense_10 128 -> 3; sh_degree 4,
 * color_layer_dim 128), fused like the trunk (the same `packed` blob carries its streams).
 *   lnrf_refnerf_dir_fwd   dir_out[m, 3] (pre-sigmoid) from dir_in[m, 0:273] = [spatial_out, IDE, -d.n] (fp32, `ld` >=
 *                          276 floats per row, rows 16-byte aligned); dsave: lnrf_refnerf_dir_save_bytes(m)
 *   lnrf_refnerf_dir_bwd   g_dir_in[m, 0:273] = d L / d dir_in (overwritten) and grads += d L / d Dense_9, Dense_10 given
 *                          g_dir_out[m, 3]; scratch: lnrf_refnerf_dir_scratch_bytes(m).  g_dir_in has `ld` floats per row
 *                          (>= 276, a multiple of 4, rows 16-byte aligned); of each of the m rows, columns
 *                          273 .. min(ld, 288) - 1 receive 0, nothing at or beyond column 288 is touched.
 * Neither call reads columns 273 .. ld - 1 of dir_in. */
int64_t lnrf_refnerf_dir_save_bytes(int64_t m);
int64_t lnrf_refnerf_dir_scratch_bytes(int64_t m);
int lnrf_refnerf_dir_fwd(const void* packed, const float* dir_in, int64_t ld, int64_t m, void* dsave,
                         float* dir_out, lnrf_stream_t stream);
int lnrf_refnerf_dir_bwd(const void* packed, const void* dsave, const float* g_dir_out, int64_t m, void* scratch,
                         float* g_dir_in, int64_t ld, float* grads, lnrf_stream_t stream);

/* Split-precision render path of RefNERFModel ("bf16x3": every forward WITHOUT a backward — rendering, evaluation,
 * model.apply).  The reference evaluates ref_nerf.py:35-77 in fp32; here every fp32 operand of the trunk forward, the
 * normal pass and the directional block is a bf16 pair hi + lo and every product is lo*hi + hi*lo + hi*hi on the bf16 MFMA
 * with fp32 accumulation (~1e-5 of fp32), so that rendered RGB meets the 1e-3 gate on the fused path.
 *   lnrf_refnerf_render_pack         fp32 parameters -> the split streams (lnrf_refnerf_render_packed_bytes bytes)
 *   lnrf_refnerf_trunk_normal_split  spatial_out[m, 0:256] (fp32, `ld` floats per row) and n_raw[m, 3] = -d spatial_out[:, 0]
 *                                    / dx in one launch; scratch: lnrf_refnerf_trunk_normal_split_scratch_bytes(m)
 *   lnrf_refnerf_dir_fwd_split       dir_out[m, 3] from dir_in[m, 0:273] as lnrf_refnerf_dir_fwd, nothing saved */
int64_t lnrf_refnerf_render_packed_bytes(void);
int lnrf_refnerf_render_pack(const float* params, void* packed_split, lnrf_stream_t stream);
int64_t lnrf_refnerf_trunk_normal_split_scratch_bytes(int64_t m);
int lnrf_refnerf_trunk_normal_split(const void* packed_split, const float* x, int64_t m, float* spatial_out, int64_t ld,
                                    float* n_raw, void* scratch, lnrf_stream_t stream);
int lnrf_refnerf_dir_fwd_split(const void* packed_split, const float* dir_in, int64_t ld, int64_t m, float* dir_out,
                               lnrf_stream_t stream);

/* ------------------------------------------------------- data-parallel exchange ---- */

/* One process per GPU; rays shard across ranks and the ONLY exchange of a training step is one all-reduce (sum) of
 * the flat fp32 gradient over RCCL/xGMI, between the backward pass and Adam — the data-parallel form of
 * TrainLoop.step_fn (train.py:85-106; the reference itself is single-device).  The mean over ranks is
 * lnrf_adam_step's grad_scale = 1/world.  The communicator is an opaque handle (the only persistent object the
 * library creates).  Bootstrap: rank 0 calls lnrf_comm_get_unique_id and hands the LNRF_COMM_UNIQUE_ID_BYTES bytes to
 * the other ranks by any channel (file, TCP store); then EVERY rank calls lnrf_comm_init (collective; binds to the
 * calling thread's current HIP device).  Errors of RCCL are returned as positive ncclResult_t values. */
#define LNRF_COMM_UNIQUE_ID_BYTES 128
typedef struct lnrf_comm* lnrf_comm_t;
int lnrf_comm_get_unique_id(void* unique_id /* (host) LNRF_COMM_UNIQUE_ID_BYTES bytes out */);
int lnrf_comm_init(const void* unique_id /* (host) */, int32_t rank, int32_t world, lnrf_comm_t* comm_out);
/* in-place sum over all ranks of buf[n] (device), enqueued on `stream` */
int lnrf_comm_allreduce(lnrf_comm_t comm, float* buf, int64_t n, lnrf_stream_t stream);
int lnrf_comm_info(lnrf_comm_t comm, int32_t* rank, int32_t* world);
int lnrf_comm_destroy(lnrf_comm_t comm);

/* ------------------------------------------------------------- optimiser ---- */

/* ---- fused InstantNGPModel MLP (reference learn_nerf/instant_ngp.py:38-54: the Dense stack after the
 * MultiresHashTableEncoding: Dense(hidden) relu x density_layers, Dense(density_dim), density = exp(out[:, :1]),
 * concat [sinusoidal_emb(d), out], Dense(hidden) relu x color_layers, tanh(Dense(3))).  bf16 MFMA operands,
 * fp32 accumulate.  Fused configuration: hidden_dim 64, density_dim 16, density_layers 1, color_layers 2,
 * d_freqs 4 (the reference defaults) and enc_dim = L*F <= 32; anything else returns LNRF_ERR_UNSUPPORTED and the
 * caller uses lnrf_dense_* / lnrf_gemm_f32.  dense_offset = float offset of Dense_0/kernel in the flat parameter
 * vector (parameters are laid out Dense_i kernel [fan_in][fan_out] then bias, i = 0..4). */
typedef struct lnrf_ngp_mlp_desc {
  int32_t enc_dim;        /* L * table_feature_dim */
  int32_t hidden_dim;
  int32_t density_dim;
  int32_t density_layers;
  int32_t color_layers;
  int32_t d_freqs;
  int64_t dense_offset;
} lnrf_ngp_mlp_desc;

int64_t lnrf_ngp_mlp_packed_bytes(const lnrf_ngp_mlp_desc* desc);
int64_t lnrf_ngp_mlp_scratch_bytes(const lnrf_ngp_mlp_desc* desc, int64_t m);
/* params: the flat fp32 parameter vector (tables included); packed: lnrf_ngp_mlp_packed_bytes bytes. */
int lnrf_ngp_mlp_pack(const lnrf_ngp_mlp_desc* desc, const float* params, void* packed, lnrf_stream_t stream);
/* enc_t: [enc_dim][m] feature-major output of lnrf_hashgrid_fwd; d: [m][3]; density [m], rgb [m][3]. */
int lnrf_ngp_mlp_fwd(const lnrf_ngp_mlp_desc* desc, const void* packed, const float* enc_t, const float* d,
                     int64_t m, float* density, float* rgb, lnrf_stream_t stream);
/* The same forward in split precision ("bf16x3", the render / evaluation path): every fp32 operand is carried as a
 * bf16 pair hi + lo and every product is lo*hi + hi*lo + hi*hi on the bf16 MFMA with fp32 accumulation, which
 * reproduces the reference's fp32 arithmetic (instant_ngp.py:38-54) to ~1e-5, so that rendered RGB meets the 1e-3
 * gate.  packed_split: lnrf_ngp_mlp_packed_split_bytes bytes, written by lnrf_ngp_mlp_pack_split. */
int64_t lnrf_ngp_mlp_packed_split_bytes(const lnrf_ngp_mlp_desc* desc);
int lnrf_ngp_mlp_pack_split(const lnrf_ngp_mlp_desc* desc, const float* params, void* packed_split,
                            lnrf_stream_t stream);
int lnrf_ngp_mlp_fwd_split(const lnrf_ngp_mlp_desc* desc, const void* packed_split, const float* enc_t,
                           const float* d, int64_t m, float* density, float* rgb, lnrf_stream_t stream);
/* VJP of lnrf_ngp_mlp_fwd (recomputes the forward): g_enc_t [enc_dim][m] = d loss / d enc (written),
 * grads (the flat gradient vector, same layout as params) += Dense kernel / bias gradients.
 * level_absmax (optional): enc_dim / 2 floats ZEROED by the caller; on return level_absmax[l] = max |g_enc_t| over
 * the two feature rows of level l (max-combined with what was there), for lnrf_hashgrid_bwd_bucketed.
 * scratch: lnrf_ngp_mlp_scratch_bytes(desc, m) bytes. */
int lnrf_ngp_mlp_bwd(const lnrf_ngp_mlp_desc* desc, const void* packed, const float* enc_t, const float* d,
                     const float* g_density, const float* g_rgb, int64_t m, void* scratch, float* g_enc_t,
                     float* level_absmax, float* grads, lnrf_stream_t stream);

/* optax.adam (train.py:59), fused over a flat buffer:
 *   g' = g*grad_scale; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 *   p -= lr * (m/(1-b1^step)) / (sqrt(v/(1-b2^step)) + eps).   step counts from 1. */
int lnrf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                   float b2, float eps, int32_t step, float grad_scale, lnrf_stream_t stream);

/* lnrf_adam_step that also accumulates the two tree_norm numerators of the step's log (train.py:92-104) while it
 * streams the buffers: sq_norms[0] += sum g^2 (g as passed in, i.e. the all-reduced SUM; multiply the root by
 * grad_scale), sq_norms[1] += sum p^2 of the parameters BEFORE the update.  sq_norms: 2 floats, zeroed by the caller. */
int lnrf_adam_step_norms(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                         float b2, float eps, int32_t step, float grad_scale, float* sq_norms,
                         lnrf_stream_t stream);

/* The scalar log of one step (train.py:141-144: mean squared errors; train.py:99-104: norms) from its accumulators:
 * sums = [sum sq err coarse, sum sq err fine, sum g^2, sum p^2] -> out = [sums[0] * inv_count, sums[1] * inv_count,
 * sqrt(sums[2]) * grad_scale, sqrt(sums[3])]; clear != 0 zeroes sums afterwards (ready for the next step). */
int lnrf_step_log(float* sums, float inv_count, float grad_scale, int32_t clear, float* out,
                  lnrf_stream_t stream);

/* *out += sum x^2 (tree_norm numerator, train.py:92-97). out must be zeroed by the caller. */
int lnrf_sq_norm(const float* x, int64_t n, float* out, lnrf_stream_t stream);

/* ------------------------------------------------------------------ mesh ---- */

/* Marching cubes over a volume (scripts/marching_cubes.py:62-66: skimage.measure.marching_cubes of the padded occupancy
 * grid at the threshold), in two passes with one read-back of the two counts between them.  vol: fp32 [nx, ny, nz]
 * in C order, every dimension >= 2; a point is inside when v > level (NaN is outside).  Vertex, face and edge
 * conventions: the header comment of csrc/mesh.hip.  Output order is deterministic (no atomics).
 * scratch: lnrf_mc_scratch_bytes bytes, 16-byte aligned (-1 for a dimension < 2). */
int64_t lnrf_mc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz);
/* pass 1: per-point codes and per-tile counts, scanned; counts (device int64 [2]): [0] = vertices V, [1] = faces F. */
int lnrf_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, void* scratch, int64_t* counts,
                  lnrf_stream_t stream);
/* pass 2, from the scratch of an lnrf_mc_count of the same volume and level and its counts n_verts = V, n_faces = F
 * (host values): verts [V, 3] (fp32, index space) and faces [F, 3] (int32, outward); nothing is written at or beyond
 * V or F.  LNRF_ERR_SHAPE when V or F does not fit in int32.  verts / faces may be NULL when V / F is 0. */
int lnrf_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, const void* scratch,
                 int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, lnrf_stream_t stream);
/* (host) the compile-time case table: out[256 * 16] int8, triangles as triples of edge numbers, -1 terminated. */
int lnrf_mc_case_table(int8_t* out);

/* ----------------------------------------------------------- point cloud ---- */

/* Exact neighbour search over a point cloud (the KD-tree queries of point_cloud/main.go:111-125, 177-187) on a uniform
 * grid of cubic cells: origin lo, edge h > 0, dims [gx, gy, gz] each in [1, 4096] and at most 2^24 cells in all
 * (LNRF_ERR_SHAPE beyond).  Results do not depend on h.  Cell, order, distance and tie conventions: the header comment
 * of csrc/pointcloud.hip.  Point and query counts above INT32_MAX give LNRF_ERR_SHAPE.  No entry point allocates,
 * copies, synchronises or uses atomics. */
typedef struct lnrf_pc_grid {
  float lo[3];
  float h;
  int32_t dims[3];
  int32_t pad_;
} lnrf_pc_grid;

/* ids [n] (device int32): linear cell id (cx*gy + cy)*gz + cz of each point of pts [n, 3], clamped into the grid (a
 * point on the upper face belongs to the last cell).  The caller sorts by it (stable) and builds cell_start. */
int lnrf_pc_cell_ids(const lnrf_pc_grid* grid, const float* pts, int64_t n, int32_t* ids, lnrf_stream_t stream);
/* out_d2 [m]: squared distance from each query to its k-th nearest point, 1 <= k <= 32 (LNRF_ERR_UNSUPPORTED above); a
 * query that is one of the points counts itself; +inf when n < k.  sorted_pts [n, 3]: the points in cell order,
 * cell_start [cells + 1] int32.  Queries should come in cell order (speed only). */
int lnrf_pc_knn_dist2(const lnrf_pc_grid* grid, const float* sorted_pts, const int32_t* cell_start, int64_t n,
                      const float* queries, int64_t m, int32_t k, float* out_d2, lnrf_stream_t stream);
/* out_d2 / out_idx [m]: squared distance to the nearest point with d2 <= max_radius^2 (max_radius >= 0, may be +inf)
 * and its original index order[j], the lowest index among equal distances; +inf and -1 without one.  Queries may lie
 * anywhere in space. */
int lnrf_pc_nearest(const lnrf_pc_grid* grid, const float* sorted_pts, const int32_t* order,
                    const int32_t* cell_start, int64_t n, const float* queries, int64_t m, float max_radius,
                    float* out_d2, int32_t* out_idx, lnrf_stream_t stream);

/* -------------------------------------------------------------- ray casting ---- */

/* Ray casting against a triangle mesh (the collider and RayCaster queries of simple_dataset/main.go:96-100, 132-136): an
 * implicit binary tree over Morton-sorted leaves of leaf_size triangles.  The pinned fp32 ray-triangle test, the tie
 * rule, the node layout, the per-ray margin of the box test and the domain on which it is conservative: the header
 * comment of csrc/raycast.hip.  Results do not depend on leaf_size.  center / half: centre and half extents of the
 * mesh's box, radius >= half[0] + half[1] + half[2], > 0; 1 <= n_tris <= 2^28, 1 <= leaf_size <= 64 (LNRF_ERR_SHAPE
 * beyond).  No entry point allocates, copies, synchronises or uses atomics. */
typedef struct lnrf_rt_bvh {
  float center[3];
  float radius;
  float half[3];
  int32_t n_tris;
  int32_t leaf_size;
  int32_t pad_;
} lnrf_rt_bvh;

/* (host) rows of the nodes array [rows, 8] fp32 for n_tris triangles: twice the power of two >= ceil(n_tris /
 * leaf_size); -1 outside the limits above. */
int64_t lnrf_rt_node_count(int64_t n_tris, int32_t leaf_size);
/* codes [n_tris] (device int32): 30-bit Morton code of each centroid of tris [n_tris, 3, 3] in the box, 2^30 for a
 * sliver (always-tested set).  The caller sorts by it (stable) and gathers the triangles. */
int lnrf_rt_morton(const lnrf_rt_bvh* bvh, const float* tris, int32_t* codes, lnrf_stream_t stream);
/* nodes [lnrf_rt_node_count, 8] (16-byte aligned): the bounds of every node over sorted_tris, leaves first, then level
 * by level. */
int lnrf_rt_fit(const lnrf_rt_bvh* bvh, const float* sorted_tris, float* nodes, lnrf_stream_t stream);
/* out_t / out_id [m]: parameter and original index order[j] of the nearest accepted triangle of each ray of rays
 * [m, 2, 3] (origin, direction), the lowest index among equal t; +inf and -1 without one.  window [m, 2] = (t_min,
 * t_max) per ray, or NULL for (0, +inf). */
int lnrf_rt_closest(const lnrf_rt_bvh* bvh, const float* sorted_tris, const int32_t* order, const float* nodes,
                    const float* rays, const float* window, int64_t m, float* out_t, int32_t* out_id,
                    lnrf_stream_t stream);
/* out [m] (uint8): 1 iff any triangle is accepted within the ray's window, else 0. */
int lnrf_rt_occluded(const lnrf_rt_bvh* bvh, const float* sorted_tris, const float* nodes, const float* rays,
                     const float* window, int64_t m, uint8_t* out, lnrf_stream_t stream);

/* ---------------------------------------------------------- mesh comparison ---- */

/* Point-to-mesh queries and surface sampling behind learn_nerf/mesh_metrics.py and scripts/eval_mesh.py, over the tree
 * above (bvh, sorted_tris, order, nodes exactly as lnrf_rt_morton / lnrf_rt_fit leave them).  The pinned fp32
 * point-triangle distance, the tie rule, the margin of the box test with its derivation and the domain: the header
 * comment of csrc/raycast.hip, section "Nearest triangle"; areas, sampling and the statistics: csrc/mesh_metrics.hip.
 * No entry point allocates, copies, synchronises or uses atomics; every output element is written. */

/* out_d2 / out_id [m]: the pinned squared distance from each point of pts [m, 3] to the nearest triangle and that
 * triangle's original index order[j], the lowest index among equal d2.  out_point (nullable) [m, 3]: the closest point
 * of that triangle.  Results do not depend on leaf_size. */
int lnrf_mesh_nearest(const lnrf_rt_bvh* bvh, const float* sorted_tris, const int32_t* order, const float* nodes,
                      const float* pts, int64_t m, float* out_d2, int32_t* out_id, float* out_point,
                      lnrf_stream_t stream);
/* areas [n] fp32 of tris [n, 3, 3]: 0.5 * sqrt(|e1 x e2|^2), every operation rounded once, sqrt correctly rounded. */
int lnrf_mesh_tri_areas(const float* tris, int64_t n, float* areas, lnrf_stream_t stream);
/* m stratified samples in proportion to area.  cdf [n] (device float64): non-decreasing running sum of the areas of
 * tris [n, 3, 3] in their order, the total last (> 0, finite; the caller checks).  Sample i draws u0, u1, u2 = elements
 * 3i, 3i + 1, 3i + 2 of Philox stream stream_id under seed (csrc/philox.h); x = ((i + u0) / m) * total in fp64; its
 * triangle is the first j with cdf[j] > x, or, when there is none, the first j with cdf[j] >= total (the last triangle
 * of positive area), so a zero-area triangle is never chosen; (u1, u2) is folded to (1 - u1, 1 - u2) if u1 + u2 > 1 and
 * the point is (v0 + u1 * e1) + u2 * e2 in fp32, one rounding per operation.  pts [m, 3]; ids [m]: order[j], or j when
 * order is NULL.  1 <= n <= 2^28, 0 <= m < 2^40. */
int lnrf_mesh_sample_surface(const float* tris, const int32_t* order, const double* cdf, int64_t n, int64_t m,
                             uint64_t seed, uint32_t stream_id, float* pts, int32_t* ids, lnrf_stream_t stream);
/* Statistics of m squared distances d2 [m] fp32 (finite, >= 0) in fp64 and in the fixed order of the dataset
 * diagnostics below (min(ceil(m / 256), 1024) workgroups of 256 leave their partials in `scratch`, 8-byte aligned, and
 * a second launch of one workgroup folds them; every partial that is read is written first).  acc: device double
 * [4 + n_thresholds]: acc[0] += sum sqrt(double(d2)), acc[1] += sum double(d2), acc[2] += sum |double(cosine)| (cosine
 * [m] fp32, nullable: acc[2] is then left alone), acc[3] = max(acc[3], max d2), acc[4 + k] += the number of elements
 * with sqrt(double(d2)) <= thresholds[k] (as a double: exact below 2^53).  thresholds: (host) n_thresholds <= 8
 * doubles.  Successive calls on one stream may share acc.  m == 0 returns LNRF_OK and touches nothing.
 * scratch: lnrf_dist_stats_scratch_bytes(m) bytes (-1 for m < 0). */
int64_t lnrf_dist_stats_scratch_bytes(int64_t m);
int lnrf_dist_stats_f64(const float* d2, const float* cosine, int64_t m, const double* thresholds,
                        int32_t n_thresholds, double* acc, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);

/* ------------------------------------------------------ dataset diagnostics ---- */

/* Whole-view reductions behind scripts/cv_nerf.py and scripts/check_bbox.py (csrc/view_stats.hip), with a FIXED order
 * of combination: workgroups of 256 whose count min(ceil(n / 256), 1024) depends on the problem size only leave one
 * partial each in `scratch` (8-byte aligned; every partial that is read is written first), and a second launch of one
 * workgroup folds the partials into the caller's accumulator — bit-reproducible on any device.  No entry point
 * allocates, copies, synchronises or uses atomics. */

/* *acc += S, S = sum_n sum_c (double(outputs[n, c]) - double(targets[n * target_stride + c]))^2 with every operation in
 * fp64: the numerator of the mean squared error of TrainLoop.losses (train.py:141-142), the deterministic counterpart
 * of the sq_err atomic of lnrf_composite_fwd.  outputs [n, 3] fp32; targets: rows of target_stride >= 3 floats (9 for
 * the colour column of an [n, 3, 3] batch); ray_err (nullable) [n] fp32 receives float(sum_c ...) per ray; acc: one
 * device double, which successive calls on one stream may share.  NaN / Inf propagate.  n == 0 returns LNRF_OK and
 * touches nothing.  scratch: lnrf_sq_err_scratch_bytes(n) bytes (-1 for n < 0). */
int64_t lnrf_sq_err_scratch_bytes(int64_t n);
int lnrf_sq_err_f64(const float* outputs, const float* targets, int64_t target_stride, int64_t n, float* ray_err,
                    double* acc, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);

/* The pixels of a view whose ray misses the scene box (scripts/check_bbox.py:31-46): for every pixel in raster order
 * the ray of CameraView.bare_rays (dataset.py:52-78, the arithmetic of lnrf_camera_rays) is tested with ray_t_range
 * (render.py:346-389, the arithmetic of lnrf_ray_aabb_stratified), and the pixels whose mask is false are combined
 * into stats (device int64 [10]): [0] += count, [1..3] += sums of the uint8 channel values, [4..6] = min(., channel
 * minima), [7..9] = max(., channel maxima) — the caller initialises [4..6] to 255 and [7..9] to 0, and may run several
 * views into one stats.  Integer arithmetic: exact.  image: uint8 [height, width, 3]; miss (nullable): uint8
 * [height * width], 1 for a ray that misses, 0 for one that hits.  origin / axes / bbox_min / bbox_max: (host) 3 floats
 * each; fields of view in radians.  width, height >= 1 and width * height <= INT32_MAX, else LNRF_ERR_SHAPE (scratch
 * bytes: -1); a width or height of 1 uses the -1 end of the linspace, like lnrf_camera_rays.
 * scratch: lnrf_view_miss_scratch_bytes(width, height) bytes. */
int64_t lnrf_view_miss_scratch_bytes(int32_t width, int32_t height);
int lnrf_view_miss_stats(const float* origin, const float* x_axis, const float* y_axis, const float* z_axis,
                         float x_fov, float y_fov, int32_t width, int32_t height, const uint8_t* image,
                         const float* bbox_min, const float* bbox_max, float min_t_range, float epsilon, uint8_t* miss,
                         int64_t* stats, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);

/* --------------------------------------------------------- image metrics ---- */

/* SSIM of two images (csrc/image_metrics.hip; learn_nerf/metrics.py, scripts/eval_nerf.py), Wang et al. 2004 as
 * skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1,
 * channel_axis=-1) computes it: a, b fp32 [height, width, 3] in [0, 1], each channel on its own; 11 x 11 Gaussian
 * window g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1 and applied separably; VALID region only, no padding;
 * population moments s_xx = filt(x x) - mu_x^2 (likewise s_yy, s_xy), not clamped; C1 = 0.01^2, C2 = 0.03^2;
 * ssim = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)).  Taps, moments, ratio and sum
 * are fp64.  ssim_map (nullable): double [height - 10, width - 10, 3]; *acc (one device double, which successive calls
 * on one stream may share) += the sum of the map's entries — the view's SSIM is that sum / (3 (height - 10)(width - 10)).
 * The order of summation is fixed, by the scheme of the dataset diagnostics above: min(tiles, 1024) workgroups of 256,
 * tiles = 3 * ceil((height - 10) / 16) * ceil((width - 10) / 32), leave one partial each in `scratch` (8-byte aligned;
 * every partial that is read is written first) and a second launch of one workgroup folds them into *acc.  No atomics,
 * allocation, copy or synchronisation.  NaN / Inf propagate.  width, height >= 11 and width * height <= INT32_MAX, else
 * LNRF_ERR_SHAPE (scratch bytes: -1).  scratch: lnrf_ssim_scratch_bytes(width, height) bytes. */
int64_t lnrf_ssim_scratch_bytes(int32_t width, int32_t height);
int lnrf_ssim_f64(const float* a, const float* b, int32_t width, int32_t height, double* ssim_map, double* acc,
                  void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);

/* ------------------------------------------------------------- occupancy ---- */

/* Occupancy grid for the inference renderer (additive: the reference samples every ray over its whole box range).
 * Conventions, passes and the walk's pad: the header comments of csrc/occupancy.hip and csrc/occ_geom.h.
 * lnrf_occ_build: sigma fp32 [(R+1)^3], densities at the cell-corner lattice in C order, R = resolution in [1, 512]
 * (else LNRF_ERR_SHAPE; scratch bytes -1).  Cell (i, j, k) is raw-occupied iff some corner has NOT (sigma < sigma_thr)
 * (NaN and +inf occupy), occupied iff a raw-occupied cell lies within Chebyshev distance dilate >= 0.  bits: uint32
 * [ceil(R^3 / 32)], cell (i*R + j)*R + k = bit idx & 31 of word idx >> 5, unused bits of the last word zero; count: one
 * device int64, the occupied cells (integer sums in a fixed order, no atomics).
 * scratch: lnrf_occ_scratch_bytes(R) bytes, 16-byte aligned. */
int64_t lnrf_occ_scratch_bytes(int32_t resolution);
int lnrf_occ_build(const float* sigma, int32_t resolution, float sigma_thr, int32_t dilate, uint32_t* bits,
                   int64_t* count, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);

/* Clips the (t_min, t_max, mask) of lnrf_ray_aabb_stratified (same rays, ray_stride, box, min_t_range and epsilon) to
 * the occupied cells each ray crosses, one ray per lane: t_min' = max(t_min, t_first - pad), t_max' = min(t_max,
 * max(t_last + pad, t_min' + min_t_range)), mask' = mask & (an occupied cell was crossed), the null range
 * (0, min_t_range) where mask' is 0.  A full grid returns its inputs bit for bit.  The outputs may be the inputs. */
int lnrf_occ_clip_rays(const float* rays, int64_t ray_stride, int64_t n_rays, const float* bbox_min,
                       const float* bbox_max, const uint32_t* bits, int32_t resolution, float min_t_range,
                       float epsilon, const float* t_min, const float* t_max, const uint8_t* mask, float* t_min_out,
                       float* t_max_out, uint8_t* mask_out, lnrf_stream_t stream);

/* idx[0..count) = the indices of the non-zero bytes of mask [n] in ascending order (idx holds n int32), count: one
 * device int64 that the host reads back.  Deterministic: a scan, no atomics.  n <= INT32_MAX, else LNRF_ERR_SHAPE. */
int lnrf_compact_mask(const uint8_t* mask, int64_t n, int32_t* idx, int64_t* count, lnrf_stream_t stream);

/* The inverse of lnrf_gather_rows: out[idx[i], :] = src[i, :] for i < n, rows of row_floats fp32, out of n_out rows.
 * Rows that idx does not name are left as they are; an index outside [0, n_out) is skipped; idx must not repeat. */
int lnrf_scatter_rows(const float* src, int32_t row_floats, const int32_t* idx, int64_t n, float* out, int64_t n_out,
                      lnrf_stream_t stream);

/* ---------------------------------------------------- connected components ---- */

/* Connected components of a 3-D mask (additive; csrc/components.hip, whose header comment fixes the conventions and
 * names the passes; learn_nerf/components.py runs the rounds).  mask: uint8 [nx, ny, nz], non-zero = foreground, linear
 * index (i*ny + j)*nz + k, every dimension >= 1 (LNRF_ERR_ARG) and N = nx*ny*nz <= INT32_MAX (LNRF_ERR_UNSUPPORTED,
 * scratch bytes -1; checked before any pointer is looked at).  connectivity: 6 or 26 (LNRF_ERR_ARG otherwise).
 * labels: int32 [N], the smallest linear index of the cell's component, -1 for background.
 * scratch: lnrf_cc_scratch_bytes(nx, ny, nz) bytes, 4-byte aligned, the same block for lnrf_cc_local and every
 * lnrf_cc_merge_round of one labelling; every byte that is read is written first. */
#define LNRF_CC_MAX_ROUNDS 64
int32_t lnrf_cc_max_rounds(void); /* (host) LNRF_CC_MAX_ROUNDS */
int64_t lnrf_cc_scratch_bytes(int64_t nx, int64_t ny, int64_t nz);
/* init + per-tile pass: labels = the smallest index of the cell's component WITHIN its 8^3 tile. */
int lnrf_cc_local(const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int32_t* labels,
                  void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);
/* One merge round (merge across all neighbours + flatten) on the labels and scratch of lnrf_cc_local.  changed: one
 * device int32, cleared first and set to 1 when the round lowered a parent or a bounded walk gave up; the host reads it
 * back, and the labels are final after the first round that leaves 0 — not before.  round: 0, 1, ... as counted by the
 * caller; round >= LNRF_CC_MAX_ROUNDS launches nothing and returns LNRF_ERR_UNSUPPORTED ("no fixed point"). */
int lnrf_cc_merge_round(int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int32_t round, int32_t* labels,
                        int32_t* changed, void* scratch, int64_t scratch_bytes, lnrf_stream_t stream);
/* sizes int32 [n]: the number of cells labelled r at index r, 0 elsewhere (integer atomics: exact).  Labels outside
 * [0, n) count nowhere.  1 <= n <= INT32_MAX. */
int lnrf_cc_sizes(const int32_t* labels, int64_t n, int32_t* sizes, lnrf_stream_t stream);
/* keep uint8 [n]: 1 iff labels[c] >= 0, s = sizes[labels[c]] >= min_cells (>= 1) and (s > cut_size or (s == cut_size
 * and labels[c] <= cut_label)): (cut_size, cut_label) is the last component kept in the order (size descending, label
 * ascending), which the host finds from sizes; cut_size = 0 keeps every component of min_cells or more. */
int lnrf_cc_keep(const int32_t* labels, const int32_t* sizes, int64_t n, int32_t min_cells, int32_t cut_size,
                 int32_t cut_label, uint8_t* keep, lnrf_stream_t stream);

/* ------------------------------------------------------------- TSDF fusion ---- */

/* Truncated-signed-distance fusion of RGB-D views into a grid of nx x ny x nz points (additive; csrc/tsdf.hip, and
 * csrc/tsdf_geom.h for the arithmetic, operation by operation; learn_nerf/tsdf.py drives it).  Grid point (i, j, k) is
 * at (xs[i], ys[j], zs[k]) (device arrays) and has linear index (i*ny + j)*nz + k.  Every dimension >= 1 and
 * (nx+2)(ny+2)(nz+2) <= INT32_MAX, else LNRF_ERR_SHAPE (checked before any pointer is looked at).  No entry point
 * allocates, copies or synchronises.
 * State, caller-owned and zeroed before the first view: sum_t f32 [N], n_obs i32 [N], behind u8 [N], rgb_sum i32 [N, 3],
 * n_col i32 [N]. */
typedef struct lnrf_tsdf_view {
  float origin[3];
  float inv[9];    /* rows of M^-1, M = [tan(x_fov/2) x_axis | tan(y_fov/2) y_axis | camera_direction] (columns) */
  float zaxis[3];  /* camera_direction */
  int32_t width, height; /* each >= 2 */
  int32_t pad_;
  int64_t depth_offset; /* element offset of this view's uint16 [height, width] z-depth in `depth` */
  int64_t color_offset; /* element offset of this view's uint8 [height, width, 3] RGB image in `color` */
} lnrf_tsdf_view;

/* Adds views[0 .. n_views) (a device array), in order, to the state.  depth / color: the packed device buffers that
 * the descriptors' offsets index; a view's images must lie inside them (not checked: the descriptors are on the
 * device).  z-depth = (float)d16 / 65535 * max_depth, 0xFFFF = nothing hit; with carve != 0 such a pixel counts as
 * free space (sum_t += 1).  trunc, max_depth > 0 and finite (LNRF_ERR_ARG).  One lane owns a voxel: no atomics, and
 * the same bits however the views are split over calls.  n_views = 0 launches nothing. */
int lnrf_tsdf_integrate(const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                        const lnrf_tsdf_view* views, int64_t n_views, const uint16_t* depth, const uint8_t* color,
                        float trunc, float max_depth, int32_t carve, float* sum_t, int32_t* n_obs, uint8_t* behind,
                        int32_t* rgb_sum, int32_t* n_col, lnrf_stream_t stream);
/* out fp32 [nx+2, ny+2, nz+2], ready for lnrf_mc_* at level 0 (inside = out > 0): -1 on the padding layer and -F at
 * the grid points, F = sum_t / (float)n_obs where n_obs > 0, else -1 when behind and unseen_inside != 0, else +1. */
int lnrf_tsdf_volume(const float* sum_t, const int32_t* n_obs, const uint8_t* behind, int64_t nx, int64_t ny,
                     int64_t nz, int32_t unseen_inside, float* out, lnrf_stream_t stream);
/* rgb_out fp32 [n, 3] in [0, 1] for the vertices verts [n, 3] of lnrf_mc_emit on that volume (padded index space):
 * the mean colours rgb_sum / n_col / 255 of the two grid points of the vertex's edge, interpolated as the vertex is;
 * the one that has a colour when the other has none; 0.5 grey when neither has.  n_missing: one device int32, cleared
 * first, = the number of grey vertices (integer atomics: exact).  0 <= n <= INT32_MAX, else LNRF_ERR_SHAPE. */
int lnrf_tsdf_vertex_colors(const float* verts, int64_t n, int64_t nx, int64_t ny, int64_t nz, const int32_t* rgb_sum,
                            const int32_t* n_col, float* rgb_out, int32_t* n_missing, lnrf_stream_t stream);

/* ----------------------------------------------------- mesh simplification ---- */

/* Vertex clustering with quadric error metrics (Lindstrom 2000) on a grid of cubic cells (additive; csrc/simplify.hip,
 * whose header comment fixes the conventions and the order of the fold, and csrc/simplify_geom.h for the arithmetic,
 * operation by operation; learn_nerf/simplify.py drives the passes).  Everything is defined on triangle corners:
 * entry e = 3t + k is corner k of triangle t of tris [n_tris, 3, 3] fp32, n_tris <= INT32_MAX / 3 (LNRF_ERR_SHAPE
 * beyond).  Grid: origin lo (at or below every corner), inv_h = the fp32 rounding of 1 / h, dims each >= 1 with fewer
 * than 2^31 cells in all (LNRF_ERR_SHAPE; checked before any pointer is looked at).  No entry point allocates, copies
 * or synchronises; the only atomics are integer adds. */
typedef struct lnrf_simp_grid {
  float lo[3];
  float inv_h;
  int32_t dims[3];
  int32_t pad_;
} lnrf_simp_grid;

#define LNRF_SIMP_MEAN 0
#define LNRF_SIMP_QUADRIC 1

/* keys [n] (device int32): (cx*ny + cy)*nz + cz of each point of pts [n, 3], c_a = min(n_a - 1,
 * (int)floorf((p_a - lo_a) * inv_h)), every fp32 operation rounded once. */
int lnrf_simp_cell_keys(const lnrf_simp_grid* grid, const float* pts, int64_t n, int32_t* keys, lnrf_stream_t stream);
/* *count (one device int64, which the caller clears) += the triangles whose three corners have three distinct keys. */
int lnrf_simp_count_faces(const lnrf_simp_grid* grid, const float* tris, int64_t n_tris, int64_t* count,
                          lnrf_stream_t stream);
/* (host) the segment length above which shape 0 of lnrf_simp_accumulate gives a segment to a wave. */
int32_t lnrf_simp_long_segment(void);
/* The per-cell sums.  keys [3 n_tris]: lnrf_simp_cell_keys of the corners; order [3 n_tris] int32: the entries stably
 * sorted by key; seg_start [n_cells + 1] int32: the first sorted entry of each occupied cell, [n_cells] = 3 n_tris.
 * colors (nullable, with col_sums): uint8 [3 n_tris, 3], one RGB per corner.  Per cell: counts int32 = its corners,
 * sums double [13] = the corner position sum and the 10 coefficients (A upper triangle, b, c) of the area-weighted plane
 * quadrics of its triangles, each triangle once, folded in fp64 in the fixed order of csrc/simplify.hip; col_sums int64
 * [3].  shape: 0 = a 16-lane group per short segment and a wave per long one, 1 = groups only, 2 = waves only; the
 * results do not depend on it.  Entries outside [0, 3 n_tris) and segment bounds outside the array are skipped. */
int lnrf_simp_accumulate(const float* tris, int64_t n_tris, const int32_t* keys, const int32_t* order,
                         const int32_t* seg_start, int64_t n_cells, const uint8_t* colors, int32_t shape,
                         int32_t* counts, double* sums, int64_t* col_sums, lnrf_stream_t stream);
/* verts fp32 [n_cells, 3]: the vertex of each occupied cell (cell_keys [n_cells] int32) from its counts and sums:
 * LNRF_SIMP_MEAN = the corner mean x0, LNRF_SIMP_QUADRIC = x0 + A^+ (b - A x0) by a cyclic Jacobi eigen-decomposition
 * in fp64 with eigenvalues at or below 1e-3 of the largest dropped; fell_back uint8 [n_cells] = 1 where the result was
 * not finite or further than h from the cell centre in the max norm and x0 was returned instead.  h: the cell edge in
 * fp64.  colors (nullable, with col_sums) uint8 [n_cells, 3] = floor(sum / count + 0.5). */
int lnrf_simp_place(const lnrf_simp_grid* grid, double h, const int32_t* cell_keys, const int32_t* counts,
                    const double* sums, const int64_t* col_sums, int64_t n_cells, int32_t placement, float* verts,
                    uint8_t* colors, uint8_t* fell_back, lnrf_stream_t stream);
/* *count (one device int64, which the caller clears) += the faces [n_faces, 3] (int32 into verts [n_verts, 3]) whose
 * fp64 normal has a negative dot product with that of their input triangle tris[face_src[f]].  Faces that name a
 * triangle or a vertex out of range are skipped. */
int lnrf_simp_flipped(const float* tris, int64_t n_tris, const int32_t* face_src, const int32_t* faces,
                      int64_t n_faces, const float* verts, int64_t n_verts, int64_t* count, lnrf_stream_t stream);

/* ---------------------------------------------------------- texture baking ---- */

/* A texture atlas with one right-angled patch per triangle and the bake of dataset views into it (additive;
 * csrc/texture.hip, the bake kernel in csrc/raycast.hip, and csrc/tex_geom.h for the layout, the no-bleed argument and
 * the arithmetic, operation by operation; learn_nerf/texture.py drives the passes).  The texture is size x size texels,
 * texel (x, y) has linear index y * size + x; faces go two to a cell of cell x cell texels, cells_per_row =
 * ceil(sqrt(ceil(faces / 2))), size = cells_per_row * cell, 6 <= cell <= 256, size <= 2^15, faces >= 1: anything else
 * is LNRF_ERR_SHAPE (checked before any pointer is looked at).  tris [faces, 3, 3] fp32 in the caller's face order.
 * No entry point allocates, copies or synchronises; the only atomic is the integer add of lnrf_tex_fill. */
typedef struct lnrf_tex_atlas {
  int32_t faces, cells_per_row, cell, size;
} lnrf_tex_atlas;

typedef struct lnrf_tex_view {
  float origin[3];
  float inv[9]; /* rows of M^-1, M = [tan(x_fov/2) x_axis | tan(y_fov/2) y_axis | camera_direction] (columns) */
  int32_t width, height; /* each >= 2 */
  int64_t pixel_offset;  /* this view's first pixel in `rgba` (uint8 [.., 4]), in pixels */
} lnrf_tex_view;

/* Per texel: face int32 [size^2] (-1: none), position fp32 [size^2, 3] (the clamped surface point), normal fp32
 * [size^2, 3] (unit, geometric; (0, 0, 0) marks a zero-area face), bary fp32 [size^2, 3] in the face's vertex order.
 * Texels without a face get zeros.  Any output but face may be NULL. */
int lnrf_tex_texels(const lnrf_tex_atlas* atlas, const float* tris, int32_t* face, float* position, float* normal,
                    float* bary, lnrf_stream_t stream);
/* uv fp32 [m, 2] (texels; OBJ coordinates are u / size, 1 - v / size) of the surface points points [m, 3] of the faces
 * ids [m]: projected onto the face's plane, the barycentrics clamped into the triangle.  An id outside [0, faces)
 * gives NaN. */
int lnrf_tex_uv(const lnrf_tex_atlas* atlas, const float* tris, const float* points, const int32_t* ids, int64_t m,
                float* uv, lnrf_stream_t stream);
/* out fp32 [m, 3]: the bilinear sample at uv [m, 2] (texels) of texture [height, width, 3], uint8 (is_float = 0) or
 * fp32; nested lerps a + t * (b - a), indices clamped at the border, a texel of weight 0 is not read.  height and
 * width in [1, 2^15] (LNRF_ERR_SHAPE). */
int lnrf_tex_sample(const void* texture, int32_t is_float, int64_t height, int64_t width, const float* uv, int64_t m,
                    float* out, lnrf_stream_t stream);
/* Adds views[0 .. n_views) (a device array), in order, to state fp32 [size^2, 4] = (sum w r, sum w g, sum w b, sum w),
 * caller-owned and zeroed before the first view; r, g, b in 0 .. 255.  A view contributes to a texel of a face with a
 * normal when the cosine between the normal and the direction to the camera exceeds cos_max, the bilinear footprint of
 * the projection lies inside the image, its pixels all have alpha >= 128, and the ray from the point (moved by offset
 * along the normal) to the camera hits no triangle of the tree (bvh, sorted_tris, nodes: lnrf_rt_fit of the same
 * triangles); weight = cosine^power.  rgba: the packed uint8 [.., 4] images that the descriptors index (not checked:
 * the descriptors are on the device).  0 <= power <= 64, offset >= 0 and finite, cos_max finite (LNRF_ERR_ARG).  One
 * lane owns a texel: no atomics, and the same bits however the views are split over calls.  n_views = 0 launches
 * nothing. */
int lnrf_tex_bake_views(const lnrf_rt_bvh* bvh, const float* sorted_tris, const float* nodes,
                        const lnrf_tex_atlas* atlas, const float* tris, const lnrf_tex_view* views, int64_t n_views,
                        const uint8_t* rgba, float cos_max, int32_t power, float offset, float* state,
                        lnrf_stream_t stream);
/* rgb uint8 [size^2, 3] and seen uint8 [size^2] from the state: seen = sum w > 0, byte = floor(255 * clamp((sum w c /
 * sum w) / 255, 0, 1) + 0.5); an unseen texel gets (unseen_r, unseen_g, unseen_b), each in [0, 255]. */
int lnrf_tex_resolve(const lnrf_tex_atlas* atlas, const float* state, int32_t unseen_r, int32_t unseen_g,
                     int32_t unseen_b, uint8_t* rgb, uint8_t* seen, lnrf_stream_t stream);
/* One Jacobi pass from (rgb_in, seen_in) to (rgb_out, seen_out), distinct buffers: a texel with seen == 0 and a face
 * takes the mean (integers, round half up; order left, right, up, down) of its 4-neighbours that have seen != 0 and the
 * same face, and seen = 2; every other texel is copied.  *filled (one device int32, which the caller clears) += the
 * texels filled. */
int lnrf_tex_fill(const lnrf_tex_atlas* atlas, const uint8_t* rgb_in, const uint8_t* seen_in, uint8_t* rgb_out,
                  uint8_t* seen_out, int32_t* filled, lnrf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LNRF_H */
