// common.h — shared host/device helpers for liblnrf (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include "../../include/lnrf.h"
#include "nerf_layout.h"

namespace lnrf {

void set_error(const char* fmt, ...);

inline int hip_fail(hipError_t e, const char* what) {
  set_error("%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

#define LNRF_CHECK_ARG(cond, msg)                 \
  do {                                            \
    if (!(cond)) {                                \
      lnrf::set_error("%s: %s", __func__, msg);   \
      return LNRF_ERR_ARG;                        \
    }                                             \
  } while (0)

#define LNRF_LAUNCH_CHECK()                                    \
  do {                                                         \
    hipError_t e_ = hipGetLastError();                         \
    if (e_ != hipSuccess) return lnrf::hip_fail(e_, __func__); \
  } while (0)

// the fused NeRF kernels exist for one model shape only
#define LNRF_REQUIRE_NERF_SHAPE(shape)                                                                    \
  do {                                                                                                    \
    if (!lnrf::nerf_shape_fused(shape)) {                                                                 \
      lnrf::set_error("%s: only the default NeRFModel shape {5,4,256,128,10,4} is fused", __func__);      \
      return LNRF_ERR_UNSUPPORTED;                                                                        \
    }                                                                                                     \
  } while (0)

static inline hipStream_t as_stream(lnrf_stream_t s) { return (hipStream_t)s; }

static inline bool nerf_shape_fused(const lnrf_nerf_shape* s) {
  return s && s->input_layers == 5 && s->mid_layers == 4 && s->hidden_dim == 256 && s->color_layer_dim == 128 &&
         s->x_freqs == 10 && s->d_freqs == 4;
}

// Evaluations -> 32-evaluation tiles, padded to whole workgroups (8 waves): every wave then owns a dump slot, so the dump
// stores need no branch — a conditional store makes hipcc lose count of the outstanding VMEM operations and wait vmcnt(0)
// (= drain all dump stores) before every ring write.  Padding tiles hold finite activations and zero gradients.
static inline int64_t padded_tiles(int64_t m) {
  return ((m + nl::kTileCols - 1) / nl::kTileCols + nl::kWaves - 1) / nl::kWaves * nl::kWaves;
}

template <class K>
static int set_max_dynamic_lds(K kernel, int bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e == hipSuccess ? LNRF_OK : hip_fail(e, "hipFuncSetAttribute(max dynamic LDS)");
}

// compute units of the current device: the size of a persistent launch
static inline int cu_count(int* cus) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
  return e == hipSuccess ? LNRF_OK : hip_fail(e, "hipDeviceGetAttribute(multiprocessor count)");
}

constexpr int kWave = 64;

// ---- wave64 helpers -------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// inclusive prefix sum across the 64 lanes of a wave
__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    float t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

}  // namespace lnrf
