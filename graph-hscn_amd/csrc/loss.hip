// Loss tail of the training step (reference graph_hscn/loss.py:6-19 called at
// train/train.py:82): binary-cross-entropy-with-logits / L1, mean reduction, and the
// sigmoid score, on the [B, C] prediction.  One launch produces the loss, the score and
// dL/dpred (so the backward is a single scale), replacing ~8 elementwise/reduce launches
// of a few microseconds each on a 1 280-element tensor.  Ordered block reduction: reproducible.
//
// The multiclass branch (loss.py:11-14: nll_loss(log_softmax(pred, -1), true) on class-index targets) is
// k_softmax_nll: a row lives in an aligned group of W lanes, W the power of two that covers C (up to the wave), a
// lane holds K columns W apart (K = 1 for C <= 64, 4 up to 256, 16 up to SNL_MAX_C), so a row is read once and its
// maximum and its sum are lane-group shuffles.  A workgroup owns a slab of SNL_SLAB rows; R <= SNL_SLAB is ONE launch
// (the [128, 10] prediction of a training step), beyond that every workgroup leaves its partial sum in the workspace
// and a one-workgroup launch adds them in index order.  No float atomics: the same input gives the same bits.
//
// Class weights and ignore_index (F.cross_entropy(pred, true, weight=w, ignore_index=i)) are two calls.
// hscn_class_weights counts the targets (a per-workgroup LDS histogram, integer adds into the global one: any order
// gives the same counts), then ONE thread derives the weights and the denominator sum_c n_c w_c in double, in class
// order, and leaves it on the device.  hscn_softmax_nll_fwd_ex is k_softmax_nll's row machinery (snl_row: group
// width W, K columns per lane) with the row's term and gradient times w[target] and the division by that
// denominator; with no weights and nothing ignored the denominator is R and every operation is the unweighted
// kernel's, bit for bit.  A zero denominator (every row ignored, or weights that are zero on every class present)
// is torch's own 0 / 0: the loss is NaN, a counted row's gradient 0 * inf = NaN, an ignored row's gradient 0.
#include "hscn_common.h"

namespace {

// One workgroup of 16 waves; a thread requests its (up to four) elements of a 4096-element slab
// before it computes any: a [128, 10] prediction is one memory round trip, not five.
__global__ void __launch_bounds__(1024) k_criterion(const float* __restrict__ pred, const float* __restrict__ target,
                                                    int64_t count, int kind, float* __restrict__ loss,
                                                    float* __restrict__ score, float* __restrict__ grad) {
  __shared__ float red[16];
  const float inv = 1.0f / (float)count;
  float s = 0.f;
  for (int64_t base = 0; base < count; base += 4096) {
    float xs[4], ys[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + u * 1024 + threadIdx.x;
      xs[u] = pred[i < count ? i : 0];
      ys[u] = target[i < count ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + u * 1024 + threadIdx.x;
      if (i >= count) continue;
      float l, sg, g;
      criterion_elem(kind, xs[u], ys[u], inv, l, sg, g);
      s += l;
      if (score) score[i] = sg;
      grad[i] = g;
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    loss[0] = t * inv;
  }
}

__global__ void k_scale(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const float s = g[0];
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) y[i] = s * x[i];
}

constexpr int SNL_THREADS = 1024;   // 16 waves, as k_criterion
constexpr int SNL_SLAB = 256;       // rows of a workgroup
constexpr int SNL_MAX_C = 1024;     // 16 columns per lane of a 64-lane group
constexpr int SNL_RANGE = 1, SNL_NAN = 2;   // bits of `flags` (include/hscn.h)

int snl_group_width(int C) {
  int w = 1;
  while (w < C && w < 64) w <<= 1;
  return w;
}

// sum of v over the workgroup in a fixed order (lanes: xor tree; waves: in index order), valid in thread 0
__device__ __forceinline__ float snl_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < SNL_THREADS / 64; ++w) t += red[w];
  }
  return t;
}

// One row in its lane group: the lane's K columns x (padding: -inf), e = exp(x - m) and the group's maximum m and
// exponential sum s; ORs SNL_NAN into f for a NaN of a live row.  Every lane of the wave calls it (shuffles).
template <int K>
__device__ __forceinline__ void snl_row(const float* __restrict__ x_row, int C, int W, int j, bool live, int& f,
                                        float (&x)[K], float (&e)[K], float& m, float& s) {
  m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = j + k * W;
    x[k] = c < C ? x_row[c] : -INFINITY;
    if (x[k] != x[k]) f |= live ? SNL_NAN : 0;
    m = fmaxf(m, x[k]);
  }
  m = group_max(m, W);
  s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] = expf(x[k] - m);                              // (a padding column: exp(-inf) = 0)
    s += e[k];
  }
  s = group_sum(s, W);
}

// out = gridDim.x == 1 ? loss : the workspace's partial sums
template <int K>
__global__ void __launch_bounds__(SNL_THREADS) k_softmax_nll(const float* __restrict__ pred,
                                                             const int64_t* __restrict__ target, int64_t R, int C,
                                                             int W, float* __restrict__ out, float* __restrict__ logp,
                                                             float* __restrict__ grad, int32_t* __restrict__ flags) {
  __shared__ float red[SNL_THREADS / 64];
  const int groups = SNL_THREADS / W;                   // rows in flight
  const int g = threadIdx.x / W, j = threadIdx.x & (W - 1);
  const int64_t row0 = (int64_t)blockIdx.x * SNL_SLAB;
  const int64_t rows = R - row0 < SNL_SLAB ? R - row0 : SNL_SLAB;
  const float inv = 1.0f / (float)R;
  float acc = 0.f;
  int f = 0;
  // (every thread takes every pass: the shuffles below run with all lanes on; a row past the slab is masked)
  for (int base = 0; base < rows; base += groups) {
    const bool live = base + g < rows;
    const int64_t r = row0 + (live ? base + g : 0);
    float x[K], e[K], m, s;
    snl_row<K>(pred + r * C, C, W, j, live, f, x, e, m, s);
    const float ls = logf(s), rs = 1.0f / s;
    const int64_t t = target[r];
    const bool in_range = t >= 0 && t < C;
    if (live && !in_range) f |= SNL_RANGE;
    if (!live) continue;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = j + k * W;
      if (c >= C) continue;
      const float lp = (x[k] - m) - ls;
      const bool hit = in_range && c == (int)t;
      if (logp) logp[r * C + c] = lp;
      // a row whose target is out of range takes no part in the loss: no term, no gradient
      grad[r * C + c] = in_range ? (e[k] * rs - (hit ? 1.f : 0.f)) * inv : 0.f;
      if (hit) acc -= lp;
    }
  }
  if (f) atomicOr(flags, f);
  const float total = snl_block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = gridDim.x == 1 ? total * inv : total;
}

// loss = (sum of the workgroups' partial sums, in index order) / R
__global__ void __launch_bounds__(SNL_THREADS) k_softmax_nll_fold(const float* __restrict__ partials, int64_t n,
                                                                  int64_t R, float* __restrict__ loss) {
  __shared__ float red[SNL_THREADS / 64];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += SNL_THREADS) s += partials[i];
  const float total = snl_block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = total * (1.0f / (float)R);
}

// ---- class weights and ignore_index ----
constexpr int CW_THREADS = 256;
constexpr int CW_MAX_BLOCKS = 256;

__global__ void __launch_bounds__(CW_THREADS) k_cw_zero(int32_t* __restrict__ counts, int C) {
  for (int c = blockIdx.x * CW_THREADS + threadIdx.x; c < C; c += gridDim.x * CW_THREADS) counts[c] = 0;
}

__global__ void __launch_bounds__(CW_THREADS) k_cw_count(const int64_t* __restrict__ target, int64_t R, int C,
                                                         int64_t ignore_index, int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ flags) {
  __shared__ int32_t hist[SNL_MAX_C];
  for (int c = threadIdx.x; c < C; c += CW_THREADS) hist[c] = 0;
  __syncthreads();
  int f = 0;
  for (int64_t r = (int64_t)blockIdx.x * CW_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * CW_THREADS) {
    const int64_t t = target[r];
    if (t == ignore_index) continue;
    if (t < 0 || t >= C) { f |= SNL_RANGE; continue; }
    atomicAdd(&hist[(int)t], 1);
  }
  if (f) atomicOr(flags, f);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += CW_THREADS) {
    const int v = hist[c];
    if (v) atomicAdd(&counts[c], v);
  }
}

// mode 0: ones; 1: the caller's weights; 2: (V - n_c) / V on the classes present, 0 elsewhere (V = counted rows).
// The denominator is added by one thread in class order: C <= 1024 double adds.
__global__ void __launch_bounds__(CW_THREADS) k_cw_finish(const int32_t* __restrict__ counts, int C, int mode,
                                                          const float* __restrict__ weight_in,
                                                          float* __restrict__ weight, double* __restrict__ denom) {
  __shared__ int64_t s_v;
  if (threadIdx.x == 0) {
    int64_t v = 0;
    for (int c = 0; c < C; ++c) v += counts[c];
    s_v = v;
  }
  __syncthreads();
  const int64_t V = s_v;
  for (int c = threadIdx.x; c < C; c += CW_THREADS) {
    const int n = counts[c];
    float w = 1.0f;
    if (mode == 1) w = weight_in[c];
    if (mode == 2) w = n > 0 ? __fdiv_rn((float)(V - n), (float)V) : 0.0f;
    weight[c] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0;
    for (int c = 0; c < C; ++c) d += (double)counts[c] * (double)weight[c];
    denom[0] = d;
  }
}

// k_softmax_nll with the row's weight, the ignored rows and the device denominator
template <int K>
__global__ void __launch_bounds__(SNL_THREADS) k_softmax_nll_ex(const float* __restrict__ pred,
                                                                const int64_t* __restrict__ target, int64_t R, int C,
                                                                int W, const float* __restrict__ weight,
                                                                int64_t ignore_index, const double* __restrict__ denom,
                                                                float* __restrict__ out, float* __restrict__ logp,
                                                                float* __restrict__ grad, int32_t* __restrict__ flags) {
  __shared__ float red[SNL_THREADS / 64];
  const int groups = SNL_THREADS / W;
  const int g = threadIdx.x / W, j = threadIdx.x & (W - 1);
  const int64_t row0 = (int64_t)blockIdx.x * SNL_SLAB;
  const int64_t rows = R - row0 < SNL_SLAB ? R - row0 : SNL_SLAB;
  const float inv = 1.0f / (float)denom[0];
  float acc = 0.f;
  int f = 0;
  for (int base = 0; base < rows; base += groups) {
    const bool live = base + g < rows;
    const int64_t r = row0 + (live ? base + g : 0);
    float x[K], e[K], m, s;
    snl_row<K>(pred + r * C, C, W, j, live, f, x, e, m, s);
    const float ls = logf(s), rs = 1.0f / s;
    const int64_t t = target[r];
    const bool ignored = t == ignore_index;
    const bool in_range = !ignored && t >= 0 && t < C;
    if (live && !ignored && !in_range) f |= SNL_RANGE;
    if (!live) continue;
    const float wt = (in_range && weight) ? weight[t] : 1.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = j + k * W;
      if (c >= C) continue;
      const float lp = (x[k] - m) - ls;
      const bool hit = in_range && c == (int)t;
      if (logp) logp[r * C + c] = lp;
      // an ignored row and a row whose target is out of range take no part in the loss: no term, no gradient
      const float d = (e[k] * rs - (hit ? 1.f : 0.f)) * inv;
      grad[r * C + c] = in_range ? (weight ? wt * d : d) : 0.f;
      if (hit) acc -= weight ? wt * lp : lp;
    }
  }
  if (f) atomicOr(flags, f);
  const float total = snl_block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = gridDim.x == 1 ? total * inv : total;
}

__global__ void __launch_bounds__(SNL_THREADS) k_softmax_nll_fold_ex(const float* __restrict__ partials, int64_t n,
                                                                     const double* __restrict__ denom,
                                                                     float* __restrict__ loss) {
  __shared__ float red[SNL_THREADS / 64];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += SNL_THREADS) s += partials[i];
  const float total = snl_block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = total * (1.0f / (float)denom[0]);
}

}  // namespace

extern "C" {

int hscn_criterion_fwd(const float* pred, const float* target, int64_t count, int kind, float* loss, float* score,
                       float* grad, void* stream_) {
  if (count < 1 || !pred || !target || !loss || !grad || (kind != 0 && kind != 1)) return HSCN_E_BADARG;
  k_criterion<<<1, 1024, 0, hscn_stream(stream_)>>>(pred, target, count, kind, loss, score, grad);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_scale(const float* g, const float* x, float* y, int64_t count, void* stream_) {
  if (count < 0 || (count > 0 && (!g || !x || !y))) return HSCN_E_BADARG;
  if (count == 0) return 0;
  unsigned nb = hscn_blocks(count, 256);
  if (nb > 1024) nb = 1024;
  k_scale<<<nb, 256, 0, hscn_stream(stream_)>>>(g, x, y, count);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

size_t hscn_softmax_nll_workspace_bytes(int64_t R, int C) {
  if (R < 1 || C < 1 || C > SNL_MAX_C || R > ((int64_t)1 << 40)) return 0;
  const int64_t nb = (R + SNL_SLAB - 1) / SNL_SLAB;
  return nb > 1 ? (size_t)nb * sizeof(float) : 0;
}

int hscn_softmax_nll_fwd(const float* pred, const int64_t* target, int64_t R, int C, float* loss, float* logp,
                         float* grad, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream_) {
  if (R < 1 || C < 1 || C > SNL_MAX_C || R > ((int64_t)1 << 40) || !pred || !target || !loss || !grad || !flags)
    return HSCN_E_BADARG;
  const size_t need = hscn_softmax_nll_workspace_bytes(R, C);
  if (need && !workspace) return HSCN_E_BADARG;
  if (workspace_bytes < need) return HSCN_E_WORKSPACE;
  const int64_t nb = (R + SNL_SLAB - 1) / SNL_SLAB;
  if (nb > 0x7fffffff) return HSCN_E_BADARG;
  const int W = snl_group_width(C);
  float* out = nb == 1 ? loss : static_cast<float*>(workspace);
  hipStream_t st = hscn_stream(stream_);
  if (C <= 64)
    k_softmax_nll<1><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, out, logp, grad, flags);
  else if (C <= 256)
    k_softmax_nll<4><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, out, logp, grad, flags);
  else
    k_softmax_nll<16><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, out, logp, grad, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  if (nb > 1) {
    k_softmax_nll_fold<<<1, SNL_THREADS, 0, st>>>(out, nb, R, loss);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

int hscn_class_weights(const int64_t* target, int64_t R, int C, int64_t ignore_index, int mode,
                       const float* weight_in, int32_t* counts, float* weight, double* denom, int32_t* flags,
                       void* stream_) {
  if (R < 1 || R > 0x7fffffff || C < 1 || C > SNL_MAX_C || mode < 0 || mode > 2 || !target || !counts || !weight ||
      !denom || !flags || (mode == 1 && !weight_in))
    return HSCN_E_BADARG;
  hipStream_t st = hscn_stream(stream_);
  k_cw_zero<<<hscn_blocks(C, CW_THREADS), CW_THREADS, 0, st>>>(counts, C);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  unsigned nb = hscn_blocks(R, CW_THREADS);
  if (nb > CW_MAX_BLOCKS) nb = CW_MAX_BLOCKS;
  k_cw_count<<<nb, CW_THREADS, 0, st>>>(target, R, C, ignore_index, counts, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  k_cw_finish<<<1, CW_THREADS, 0, st>>>(counts, C, mode, weight_in, weight, denom);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_softmax_nll_fwd_ex(const float* pred, const int64_t* target, int64_t R, int C, const float* weight,
                            int64_t ignore_index, const double* denom, float* loss, float* logp, float* grad,
                            int32_t* flags, void* workspace, size_t workspace_bytes, void* stream_) {
  if (R < 1 || C < 1 || C > SNL_MAX_C || R > ((int64_t)1 << 40) || !pred || !target || !denom || !loss || !grad ||
      !flags)
    return HSCN_E_BADARG;
  const size_t need = hscn_softmax_nll_workspace_bytes(R, C);
  if (need && !workspace) return HSCN_E_BADARG;
  if (workspace_bytes < need) return HSCN_E_WORKSPACE;
  const int64_t nb = (R + SNL_SLAB - 1) / SNL_SLAB;
  if (nb > 0x7fffffff) return HSCN_E_BADARG;
  const int W = snl_group_width(C);
  float* out = nb == 1 ? loss : static_cast<float*>(workspace);
  hipStream_t st = hscn_stream(stream_);
  if (C <= 64)
    k_softmax_nll_ex<1><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, weight, ignore_index, denom, out,
                                                              logp, grad, flags);
  else if (C <= 256)
    k_softmax_nll_ex<4><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, weight, ignore_index, denom, out,
                                                              logp, grad, flags);
  else
    k_softmax_nll_ex<16><<<(unsigned)nb, SNL_THREADS, 0, st>>>(pred, target, R, C, W, weight, ignore_index, denom,
                                                               out, logp, grad, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  if (nb > 1) {
    k_softmax_nll_fold_ex<<<1, SNL_THREADS, 0, st>>>(out, nb, denom, loss);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

}  // extern "C"
