// Shared helpers for the gfx950 kernels behind include/hscn.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/hscn.h"

#define HSCN_WAVE 64

#define HSCN_RETURN_IF_LAUNCH_FAILED()                 \
  do {                                                 \
    hipError_t e__ = hipGetLastError();                \
    if (e__ != hipSuccess) return (int)e__;            \
  } while (0)

static inline hipStream_t hscn_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline unsigned hscn_blocks(int64_t work, int per_block) {
  int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b);
}

// what the float4 paths ask of a pointer
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// LDS of a gfx950 CU, the most one workgroup can be given; and the LDS (static + dynamic) a kernel gets without asking
constexpr size_t LDS_CU_BYTES = 160 * 1024;
constexpr size_t LDS_NO_OPT_IN_BYTES = 64 * 1024;

// One launch with `lds` bytes of dynamic LDS, for every kernel that can need more than a launch gets unasked: the
// opt-in, the launch, the error check.  STATIC_LDS is what the kernel declares as __shared__ arrays of its own; it
// counts towards the line but not into the request.  The attribute is requested on EVERY call that needs it: it belongs
// to the current device's copy of the kernel, so nothing here remembers an earlier request.  A refused request is
// answered here (HSCN_E_UNSUPPORTED, nothing launched), not by the launch that would follow; callers keep `lds` +
// STATIC_LDS within LDS_CU_BYTES, which gfx950 grants.
template <size_t STATIC_LDS = 0, typename... KA, typename... A>
static int launch_with_lds(void (*kernel)(KA...), unsigned grid, int threads, size_t lds, hipStream_t st,
                           const A&... args) {
  if (lds + STATIC_LDS > LDS_NO_OPT_IN_BYTES &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return HSCN_E_UNSUPPORTED;
  }
  kernel<<<grid, threads, lds, st>>>(args...);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

// Separately rounded multiply / add: the CPU reference accumulates messages as
// round(w*x) followed by round(acc + .) (torch index_add_), never a fused fma.
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

// VEC = 4 or 1 feature columns a lane: float4 where width and pointers allow, float otherwise (the row-walk kernels of
// gine.hip, gatedgcn.hip and edge_attention.hip)
template <int VEC>
struct GV;
template <>
struct GV<4> {
  using T = float4;
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ void store(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ float get(const T& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
  static __device__ __forceinline__ T make(const float* a) { return make_float4(a[0], a[1], a[2], a[3]); }
};
template <>
struct GV<1> {
  using T = float;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ float get(const T& v, int) { return v; }
  static __device__ __forceinline__ T make(const float* a) { return a[0]; }
};

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case HSCN_ACT_RELU: return v > 0.f ? v : 0.f;
    case HSCN_ACT_ELU: return v > 0.f ? v : expm1f(v);
    case HSCN_ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// derivative expressed through the forward OUTPUT y
__device__ __forceinline__ float act_grad_from_output(float y, int act) {
  switch (act) {
    case HSCN_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case HSCN_ACT_ELU: return y > 0.f ? 1.f : y + 1.f;
    case HSCN_ACT_TANH: return 1.f - y * y;
    default: return 1.f;
  }
}

// One element of the loss tail (reference graph_hscn/loss.py:6-19): kind 0 = BCE with logits
// max(x,0) - x*y + log1p(exp(-|x|)), kind 1 = L1; l = loss term, sg = sigmoid(x) (the score of both
// branches), g = d(mean loss)/dx with inv = 1/count.  Shared by k_criterion and the graph-resident
// backward, which must agree bit for bit.
__device__ __forceinline__ void criterion_elem(int kind, float x, float y, float inv, float& l, float& sg, float& g) {
  sg = 1.0f / (1.0f + expf(-x));
  if (kind == 0) {
    l = fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    g = (sg - y) * inv;
  } else {
    const float d = x - y;
    l = fabsf(d);
    g = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * inv;
  }
}

// Philox-4x32-10: the four 32-bit draws of block `ctr` under key `seed` (hscn_dropout's generator)
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  c[0] = hi1 ^ c[1] ^ k0;
  c[1] = lo1;
  c[2] = hi0 ^ c[3] ^ k1;
  c[3] = lo0;
}

__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t ctr, uint32_t (&c)[4]) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  c[0] = (uint32_t)ctr;
  c[1] = (uint32_t)(ctr >> 32);
  c[2] = 0u;
  c[3] = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// hscn_dropout's keep rule for a drop probability p in [0, 1): keep iff the draw is >= threshold = p 2^32 (computed
// in integers), kept values times scale = 1 / (1 - p)
static inline void dropout_keep_rule(float p, uint32_t& threshold, float& scale) {
  const double t = (double)p * 4294967296.0;
  threshold = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  scale = 1.0f / (1.0f - p);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// the same over aligned groups of `width` lanes (a power of two <= 64): every lane of a group receives its group's value
__device__ __forceinline__ float group_sum(float v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
