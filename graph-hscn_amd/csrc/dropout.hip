// Inverted dropout of the MPNN baseline (reference model/mpnn.py:58, F.dropout(x, p, training)):
// y = x * keep / (1 - p).  The keep decision of element i is a pure function of (seed, i) -- a
// Philox-4x32-10 block per four consecutive elements -- so the backward regenerates the mask from
// the same (seed, count) instead of storing it: one read + one write per element either way.
#include "hscn_common.h"

namespace {

__global__ void __launch_bounds__(256)
k_dropout(const float* __restrict__ x, float* __restrict__ y, int64_t n, uint32_t threshold, float scale,
          uint64_t seed) {
  const int64_t quads = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    uint32_t c[4];
    philox4x32_10(seed, (uint64_t)q, c);
    const int64_t i = q << 2;
    if (i + 3 < n && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
      float4 v = *reinterpret_cast<const float4*>(x + i);
      v.x = c[0] >= threshold ? v.x * scale : 0.f;
      v.y = c[1] >= threshold ? v.y * scale : 0.f;
      v.z = c[2] >= threshold ? v.z * scale : 0.f;
      v.w = c[3] >= threshold ? v.w * scale : 0.f;
      *reinterpret_cast<float4*>(y + i) = v;
    } else {
      for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = c[k] >= threshold ? x[i + k] * scale : 0.f;
    }
  }
}

}  // namespace

extern "C" int hscn_dropout(const float* x, float* y, int64_t count, float p, uint64_t seed, void* stream_) {
  if (count < 0 || !(p >= 0.f && p < 1.f) || (count > 0 && (!x || !y))) return HSCN_E_BADARG;
  if (count == 0) return 0;
  uint32_t threshold;
  float scale;
  dropout_keep_rule(p, threshold, scale);
  unsigned nb = hscn_blocks((count + 3) / 4, 256);
  if (nb > 4096) nb = 4096;
  k_dropout<<<nb, 256, 0, hscn_stream(stream_)>>>(x, y, count, threshold, scale, seed);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
