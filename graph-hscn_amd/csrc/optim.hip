// The optimizer step behind a resident training step (reference: torch.optim.Adam / AdamW built by
// train/train.py:82 and train/train_clustering.py:30-33 from config.py's OPTIM_DICT) as ONE launch.
//
// The resident steps leave every parameter gradient in one flat buffer (graph_hscn/step.py); the parameters
// themselves stay the module's own tensors.  torch's capturable fused Adam is two launches (step counter, update):
// 8.6 us of kernel time behind a 21 us stage-A step.  This kernel walks the flat buffer once, finds each element's
// parameter tensor through a small offset table and applies torch's single-tensor update, operation for operation
// (torch/optim/adam.py::_single_tensor_adam, adamw.py):
//   [Adam, weight_decay]   g   = g + wd * p
//   [AdamW]                p   = p * (1 - lr * wd)
//   m   = m + (1 - beta1) * (g - m)                      (Tensor.lerp_)
//   v   = v * beta2;  v = v + ((1 - beta2) * g) * g       (mul_, addcmul_)
//   p   = p + (-(lr / (1 - beta1^t))) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))     (addcdiv_)
// with the step-dependent scalars formed in double as Python does and rounded to float once.  The model family has
// a few thousand parameters: one workgroup, so the step counter needs no second launch.
//
// hscn_adam_step_ex adds, in the same launch, torch.nn.utils.clip_grad_norm_(params, max_norm) in front of the update
// (train/train.py:91-92) and optimizer.zero_grad() behind it (the accumulation loop's zeroing, train.py:94), and
// hscn_clip_grad_norm_flat is the clip alone (for optimizers that are not this one).  The norm is the sum of g^2 in
// double in a FIXED order -- per-thread partials, a butterfly over the wave, the 16 wave sums folded in wave order --
// so it is bitwise the same from run to run; from there on torch's formulas (clip_grad.py::_clip_grads_with_norm_):
//   norm = (float)sqrt(sum);  coef = min(reciprocal(norm + 1e-6f) * max_norm, 1);  g = g * coef
// (`max_norm / t` on a tensor is t.reciprocal() * max_norm; the multiply happens at coef == 1 too, as in torch, and is
// bitwise neutral there; a NaN / inf norm propagates as it does in torch).
//
// hscn_adam_step_sched is hscn_adam_step_ex with a learning-rate schedule (include/hscn.h: hscn_lr_schedule) evaluated
// in the launch: the rate is a function of the step counter the kernel reads anyway, so a warm-up / cosine / linear /
// step-decay schedule costs no launch and no host decision between two replays of a captured iteration.  The factor is
// formed in double as Python would (torch.optim.lr_scheduler.LambdaLR: lr = base_lr * f(s)); thread 0 leaves the rate
// it used in the device lr word.  hscn_adagrad_step is torch.optim.Adagrad on the same flat layout -- the same walk
// with one state vector in place of two (torch/optim/adagrad.py::_single_tensor_adagrad):
//   [weight_decay]  g = g + wd * p
//   clr = lr / (1 + (t - 1) * lr_decay)                     (double, rounded to float once)
//   sum = sum + g * g;  std = sqrt(sum) + eps;  p = p + (-clr) * (g / std)       (addcmul_, sqrt().add_, addcdiv_)
#include <stddef.h>

#include "hscn_common.h"

namespace {

constexpr int ADAM_MAXSEG = 64;   // the tables travel in the kernel arguments: no dependent load in front of the update

struct AdamArgs {
  float* params[ADAM_MAXSEG];   // the parameter tensors, in the order of the flat buffers
  int32_t off[ADAM_MAXSEG + 1]; // element offsets of the segments in the flat buffers
  const float* grads;     // [P]
  float *m, *v;           // [P] exp_avg, exp_avg_sq
  float* step;            // [1] float step counter (torch keeps a float tensor), incremented here
  double* pows;           // [2] beta1^t, beta2^t of the LAST step (1, 1 before the first): running products -- a
                          // double pow per step costs more than the whole update
  const double* lr;       // [1] learning rate on the device (a scheduler may rewrite it between launches)
  double beta1, beta2, eps, wd;   // (doubles: Python forms the step's scalars from them in double)
  int nseg, P, decoupled;
};

// hscn_adam_step_ex: the plain step's arguments FIRST (the kernel reads its tables at the start of its argument block)
struct AdamExArgs {
  AdamArgs a;
  float* grads;           // = a.grads, written: the clipped gradient, or 0 with `zero`
  float* norm_out;        // [1] or NULL: the pre-clip norm (clip_grad_norm_'s return value)
  float max_norm;
  int clip, zero;
};

// what every flat-buffer kernel has at the START of its argument block (AdamArgs spells the two members out)
struct FlatTables {
  float* params[ADAM_MAXSEG];
  int32_t off[ADAM_MAXSEG + 1];
};
static_assert(offsetof(AdamArgs, params) == offsetof(FlatTables, params) &&
              offsetof(AdamArgs, off) == offsetof(FlatTables, off), "the tables lead the argument block");

struct SchedArgs {
  hscn_lr_schedule r;
  double* lr_out;         // [1] the device lr word: receives the rate this step used
  double* gpow;           // [1] gamma^floor(s / period) (HSCN_LR_STEP): a running product, like AdamArgs::pows
};

struct AdagradArgs {
  FlatTables t;
  float* grads;           // [P]; written: the clipped gradient, or 0 with `zero`
  float* sum;             // [P] state_sum
  float* step;            // [1] float step counter, incremented here
  const double* lr;       // [1] (read without a schedule)
  double lr_decay, eps, wd;
  float* norm_out;        // [1] or NULL
  float max_norm;
  int nseg, P, clip, zero;
};

constexpr int FLAT_THREADS = 1024, FLAT_WAVES = FLAT_THREADS / HSCN_WAVE;

// The segment tables go from the kernel arguments to LDS through ONE vector load per table entry (lane k reads
// entry k of the argument block as plain memory), requested together with the thread's gradients and moments; a
// thread then finds its element's tensor by a 5-step binary search in LDS (seg_addr, behind a barrier).  (A select
// chain over the arguments costs ~150 VALU operations per element -- 4 us on one CU; a scalar loop over them one
// dependent load per entry.)  soff: ADAM_MAXSEG + 1 ints, sp: ADAM_MAXSEG pointers of LDS.
__device__ __forceinline__ void stage_tables(int nseg, int* soff, float** sp) {
  const FlatTables* kp = reinterpret_cast<const FlatTables*>(
      (const char*)__builtin_amdgcn_kernarg_segment_ptr());   // (generic pointer: a vector load, per-lane index)
  if (threadIdx.x <= ADAM_MAXSEG) soff[threadIdx.x] = (int)threadIdx.x <= nseg ? kp->off[threadIdx.x] : 0x7fffffff;
  if (threadIdx.x < ADAM_MAXSEG) sp[threadIdx.x] = (int)threadIdx.x < nseg ? kp->params[threadIdx.x] : nullptr;
}

__device__ __forceinline__ float* seg_addr(const int* soff, float* const* sp, int nseg, int i) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (soff[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return sp[lo] + (i - soff[lo]);
}

// lr(s) = base_lr * f(s) of the step about to be taken (`step`: the counter BEFORE its increment), in double with
// Python's operation order (include/hscn.h spells the formulas out); every thread forms the same value.
__device__ __forceinline__ double sched_lr(const SchedArgs& S, float step) {
  const hscn_lr_schedule& r = S.r;
  const int64_t s = (int64_t)step, w = r.warmup_steps, T = r.total_steps;
  double f;
  if (r.kind == HSCN_LR_STEP) {
    f = S.gpow[0];
  } else if (s < w) {
    f = (double)s / (double)(w > 1 ? w : 1);
    f = f > 1e-6 ? f : 1e-6;
  } else {
    const int64_t sc = s < T ? s : T;
    const double span = (double)(T - w > 1 ? T - w : 1);
    if (r.kind == HSCN_LR_WARMUP_COSINE) f = 0.5 * (1.0 + cos(3.141592653589793 * (double)(sc - w) / span));
    else f = (double)(T - sc) / span;
    f = f > r.min_factor ? f : r.min_factor;
  }
  return r.base_lr * f;
}

// thread 0, behind the closing barrier: the rate this step used, and the running product when s + 1 ends a period
__device__ __forceinline__ void sched_advance(const SchedArgs& S, float step, double lr) {
  S.lr_out[0] = lr;
  if (S.r.kind == HSCN_LR_STEP && ((int64_t)step + 1) % S.r.period == 0) S.gpow[0] = S.gpow[0] * S.r.gamma;
}

// sum of g^2 over the flat buffer: `part` is this thread's partial (elements threadIdx.x + k * 1024); every thread
// returns the same total, formed in the same order on every run.  `red`: FLAT_WAVES doubles of LDS.
__device__ __forceinline__ double flat_sumsq(double part, double* red) {
#pragma unroll
  for (int o = HSCN_WAVE / 2; o > 0; o >>= 1) part += __shfl_xor(part, o);   // (a + b == b + a: all lanes agree)
  if ((threadIdx.x & (HSCN_WAVE - 1)) == 0) red[threadIdx.x / HSCN_WAVE] = part;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < FLAT_WAVES; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ float clip_coef(double sumsq, float max_norm, float* norm_out) {
  const float norm = (float)sqrt(sumsq);
  if (norm_out && threadIdx.x == 0) norm_out[0] = norm;
  const float c = (1.0f / (norm + 1e-6f)) * max_norm;
  return c > 1.0f ? 1.0f : c;       // (torch.clamp(max=1): NaN stays NaN)
}

template <bool EX, bool SCHED = false>
__device__ __forceinline__ void adam_flat(const AdamArgs& A, const AdamExArgs& X, const SchedArgs& S = SchedArgs{}) {
  __shared__ int soff[ADAM_MAXSEG + 1];
  __shared__ float* sp[ADAM_MAXSEG];
  stage_tables(A.nseg, soff, sp);
  constexpr int EPT = 4;   // (a model of this family is a few thousand parameters: one batch of requests)
  float g0[EPT], m0[EPT], v0[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    const bool has = i < A.P;
    g0[u] = A.grads[has ? i : 0]; m0[u] = A.m[has ? i : 0]; v0[u] = A.v[has ? i : 0];
  }
  float coef = 1.0f;
  if (EX && X.clip) {   // the norm first: every gradient is in registers (P <= 4096), the rest is read twice
    __shared__ double red[FLAT_WAVES];
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < EPT; ++u)
      if (threadIdx.x + u * 1024 < A.P) s += (double)g0[u] * (double)g0[u];
    for (int i = threadIdx.x + EPT * 1024; i < A.P; i += 1024) {
      const double g = A.grads[i];
      s += g * g;
    }
    coef = clip_coef(flat_sumsq(s, red), X.max_norm, X.norm_out);   // (its barrier also publishes the tables)
#pragma unroll
    for (int u = 0; u < EPT; ++u) g0[u] = g0[u] * coef;
  }
  __syncthreads();
  auto addr = [&](int i) -> float* { return seg_addr(soff, sp, A.nseg, i); };
  float* pp0[EPT];
  float p0[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    pp0[u] = addr(i < A.P ? i : 0);
    p0[u] = *pp0[u];
  }
  const float t = A.step[0] + 1.0f;
  const double lr = SCHED ? sched_lr(S, A.step[0]) : A.lr[0];
  const double b1t = A.pows[0] * A.beta1, b2t = A.pows[1] * A.beta2;
  const double bc1 = 1.0 - b1t, bc2 = 1.0 - b2t;
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float w1 = (float)(1.0 - A.beta1), w2 = (float)(1.0 - A.beta2), b2f = (float)A.beta2;
  const float decay = (float)(1.0 - lr * A.wd), wdf = (float)A.wd, epsf = (float)A.eps;
  auto update = [&](float* pp, int i, float p, float g, float m, float v) {
    if (EX) {
      if (X.clip && i >= EPT * 1024) g = g * coef;
      if (X.zero) X.grads[i] = 0.0f;
      else if (X.clip) X.grads[i] = g;
    }
    if (A.wd != 0.0) {
      if (A.decoupled) p = p * decay;
      else g = g + wdf * p;
    }
    m = m + w1 * (g - m);
    v = v * b2f;
    v = v + (w2 * g) * g;
    const float denom = sqrtf(v) / bc2_sqrt + epsf;
    p = p + (-step_size) * (m / denom);
    *pp = p;
    A.m[i] = m;
    A.v[i] = v;
  };
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    if (i < A.P) update(pp0[u], i, p0[u], g0[u], m0[u], v0[u]);
  }
  for (int i = threadIdx.x + EPT * 1024; i < A.P; i += 1024) {
    float* pp = addr(i);
    update(pp, i, *pp, A.grads[i], A.m[i], A.v[i]);
  }
  __syncthreads();   // every thread has read the old counter
  if (threadIdx.x == 0) {
    if (SCHED) sched_advance(S, A.step[0], lr);
    A.step[0] = t; A.pows[0] = b1t; A.pows[1] = b2t;
  }
}

__global__ void __launch_bounds__(1024) k_adam_flat(const AdamArgs A) { adam_flat<false>(A, AdamExArgs{}); }

__global__ void __launch_bounds__(1024) k_adam_flat_ex(const AdamExArgs X) { adam_flat<true>(X.a, X); }

__global__ void __launch_bounds__(1024) k_adam_flat_sched(const AdamExArgs X, const SchedArgs S) {
  adam_flat<true, true>(X.a, X, S);
}

// Adagrad: adam_flat's walk with one state vector (the first 4096 elements in registers, the rest in a tail loop)
template <bool SCHED>
__global__ void __launch_bounds__(1024) k_adagrad_flat(const AdagradArgs A, const SchedArgs S) {
  __shared__ int soff[ADAM_MAXSEG + 1];
  __shared__ float* sp[ADAM_MAXSEG];
  stage_tables(A.nseg, soff, sp);
  constexpr int EPT = 4;
  float g0[EPT], s0[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    const bool has = i < A.P;
    g0[u] = A.grads[has ? i : 0]; s0[u] = A.sum[has ? i : 0];
  }
  float coef = 1.0f;
  if (A.clip) {
    __shared__ double red[FLAT_WAVES];
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < EPT; ++u)
      if (threadIdx.x + u * 1024 < A.P) s += (double)g0[u] * (double)g0[u];
    for (int i = threadIdx.x + EPT * 1024; i < A.P; i += 1024) {
      const double g = A.grads[i];
      s += g * g;
    }
    coef = clip_coef(flat_sumsq(s, red), A.max_norm, A.norm_out);
#pragma unroll
    for (int u = 0; u < EPT; ++u) g0[u] = g0[u] * coef;
  }
  __syncthreads();   // the tables are in LDS
  float* pp0[EPT];
  float p0[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    pp0[u] = seg_addr(soff, sp, A.nseg, i < A.P ? i : 0);
    p0[u] = *pp0[u];
  }
  const float step0 = A.step[0], t = step0 + 1.0f;
  const double lr = SCHED ? sched_lr(S, step0) : A.lr[0];
  const float clr = (float)(lr / (1.0 + ((double)t - 1.0) * A.lr_decay));
  const float wdf = (float)A.wd, epsf = (float)A.eps;
  auto update = [&](float* pp, int i, float p, float g, float sum) {
    if (A.clip && i >= EPT * 1024) g = g * coef;
    if (A.zero) A.grads[i] = 0.0f;
    else if (A.clip) A.grads[i] = g;
    if (A.wd != 0.0) g = g + wdf * p;
    sum = sum + g * g;
    const float std = sqrtf(sum) + epsf;
    p = p + (-clr) * (g / std);
    *pp = p;
    A.sum[i] = sum;
  };
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    if (i < A.P) update(pp0[u], i, p0[u], g0[u], s0[u]);
  }
  for (int i = threadIdx.x + EPT * 1024; i < A.P; i += 1024) {
    float* pp = seg_addr(soff, sp, A.nseg, i);
    update(pp, i, *pp, A.grads[i], A.sum[i]);
  }
  __syncthreads();   // every thread has read the old counter (and the running product)
  if (threadIdx.x == 0) {
    if (SCHED) sched_advance(S, step0, lr);
    A.step[0] = t;
  }
}

// the clip alone, in place: one workgroup (the buffer is the same few thousand floats)
__global__ void __launch_bounds__(1024) k_clip_grad_norm_flat(float* __restrict__ g, int P, float max_norm,
                                                              float* norm_out) {
  __shared__ double red[FLAT_WAVES];
  constexpr int EPT = 4;
  float g0[EPT];
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    g0[u] = g[i < P ? i : 0];
    if (i < P) s += (double)g0[u] * (double)g0[u];
  }
  for (int i = threadIdx.x + EPT * 1024; i < P; i += 1024) {
    const double v = g[i];
    s += v * v;
  }
  const float coef = clip_coef(flat_sumsq(s, red), max_norm, norm_out);
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int i = threadIdx.x + u * 1024;
    if (i < P) g[i] = g0[u] * coef;
  }
  for (int i = threadIdx.x + EPT * 1024; i < P; i += 1024) g[i] = g[i] * coef;
}

// the segment tables into an argument block (P > 0, 1 <= nseg <= ADAM_MAXSEG): HSCN_E_BADARG unless they tile [0, P)
static int fill_tables(float** params, int32_t* off, float* const* params_host, const int32_t* seg_off_host, int nseg,
                       int64_t P) {
  for (int k = 0; k < ADAM_MAXSEG; ++k) { params[k] = k < nseg ? params_host[k] : nullptr; off[k] = k <= nseg ? seg_off_host[k] : 0; }
  off[ADAM_MAXSEG] = nseg == ADAM_MAXSEG ? seg_off_host[nseg] : 0;
  for (int k = 0; k < nseg; ++k)
    if (!params_host[k] || seg_off_host[k + 1] < seg_off_host[k]) return HSCN_E_BADARG;
  if (seg_off_host[0] != 0 || seg_off_host[nseg] != P) return HSCN_E_BADARG;
  return 0;
}

// a schedule record that is one (not NULL, not HSCN_LR_CONSTANT) into the kernel's argument
static int fill_sched_args(SchedArgs& S, const hscn_lr_schedule* sched, double* lr_dev, double* sched_state_dev) {
  const hscn_lr_schedule& r = *sched;
  if (r.kind != HSCN_LR_WARMUP_COSINE && r.kind != HSCN_LR_WARMUP_LINEAR && r.kind != HSCN_LR_STEP) return HSCN_E_BADARG;
  if (!(r.base_lr >= 0.0) || r.warmup_steps < 0 || r.total_steps < r.warmup_steps || r.period < 1) return HSCN_E_BADARG;
  if (!(r.gamma > 0.0 && r.gamma <= 1.0) || !(r.min_factor >= 0.0)) return HSCN_E_BADARG;
  if (!lr_dev || !sched_state_dev) return HSCN_E_BADARG;
  S.r = r; S.lr_out = lr_dev; S.gpow = sched_state_dev;
  return 0;
}

static bool scheduled(const hscn_lr_schedule* sched) { return sched && sched->kind != HSCN_LR_CONSTANT; }

static int fill_adam_args(AdamArgs& A, float* const* params_host, const int32_t* seg_off_host, int nseg,
                          const float* grads, float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev,
                          double* beta_pows_dev, const double* lr_dev, double beta1, double beta2, double eps,
                          double weight_decay, int decoupled) {
  if (nseg < 1 || nseg > ADAM_MAXSEG || P < 0 || P > (1 << 24)) return HSCN_E_UNSUPPORTED;
  if (!params_host || !seg_off_host || !grads || !exp_avg || !exp_avg_sq || !step_dev || !beta_pows_dev || !lr_dev)
    return HSCN_E_BADARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
    return HSCN_E_BADARG;
  if (P == 0) return 0;   // (nothing to launch: the callers return before they do)
  if (int rc = fill_tables(A.params, A.off, params_host, seg_off_host, nseg, P)) return rc;
  A.grads = grads; A.m = exp_avg; A.v = exp_avg_sq; A.step = step_dev; A.pows = beta_pows_dev;
  A.lr = lr_dev; A.beta1 = beta1; A.beta2 = beta2; A.eps = eps; A.wd = weight_decay; A.nseg = nseg; A.P = (int)P;
  A.decoupled = decoupled;
  return 0;
}

}  // namespace

extern "C" int hscn_adam_step(float* const* params_host, const int32_t* seg_off_host, int nseg, const float* grads,
                              float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev, double* beta_pows_dev,
                              const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                              void* stream) {
  AdamArgs A;
  if (int rc = fill_adam_args(A, params_host, seg_off_host, nseg, grads, exp_avg, exp_avg_sq, P, step_dev, beta_pows_dev,
                              lr_dev, beta1, beta2, eps, weight_decay, decoupled))
    return rc;
  if (P == 0) return 0;
  k_adam_flat<<<1, 1024, 0, hscn_stream(stream)>>>(A);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int hscn_adam_step_ex(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                                 float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev, double* beta_pows_dev,
                                 const double* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                                 int decoupled, float max_norm, float* norm_out, int zero_grads, void* stream) {
  AdamExArgs X;
  if (int rc = fill_adam_args(X.a, params_host, seg_off_host, nseg, grads, exp_avg, exp_avg_sq, P, step_dev,
                              beta_pows_dev, lr_dev, beta1, beta2, eps, weight_decay, decoupled))
    return rc;
  if (!(max_norm > 0.0f) && max_norm != 0.0f) return HSCN_E_BADARG;   // (NaN / negative)
  if (P == 0) return 0;
  X.grads = grads; X.norm_out = norm_out; X.max_norm = max_norm; X.clip = max_norm > 0.0f; X.zero = zero_grads != 0;
  k_adam_flat_ex<<<1, 1024, 0, hscn_stream(stream)>>>(X);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int hscn_adam_step_sched(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                                    float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev,
                                    double* beta_pows_dev, double* lr_dev, double beta1, double beta2, double eps,
                                    double weight_decay, int decoupled, float max_norm, float* norm_out,
                                    int zero_grads, const hscn_lr_schedule* sched, double* sched_state_dev,
                                    void* stream) {
  if (!scheduled(sched))
    return hscn_adam_step_ex(params_host, seg_off_host, nseg, grads, exp_avg, exp_avg_sq, P, step_dev, beta_pows_dev,
                             lr_dev, beta1, beta2, eps, weight_decay, decoupled, max_norm, norm_out, zero_grads, stream);
  AdamExArgs X;
  SchedArgs S;
  if (int rc = fill_adam_args(X.a, params_host, seg_off_host, nseg, grads, exp_avg, exp_avg_sq, P, step_dev,
                              beta_pows_dev, lr_dev, beta1, beta2, eps, weight_decay, decoupled))
    return rc;
  if (!(max_norm > 0.0f) && max_norm != 0.0f) return HSCN_E_BADARG;   // (NaN / negative)
  if (int rc = fill_sched_args(S, sched, lr_dev, sched_state_dev)) return rc;
  if (P == 0) return 0;
  X.grads = grads; X.norm_out = norm_out; X.max_norm = max_norm; X.clip = max_norm > 0.0f; X.zero = zero_grads != 0;
  k_adam_flat_sched<<<1, 1024, 0, hscn_stream(stream)>>>(X, S);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int hscn_adagrad_step(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                                 float* state_sum, int64_t P, float* step_dev, double* lr_dev, double lr_decay,
                                 double eps, double weight_decay, float max_norm, float* norm_out, int zero_grads,
                                 const hscn_lr_schedule* sched, double* sched_state_dev, void* stream) {
  if (nseg < 1 || nseg > ADAM_MAXSEG || P < 0 || P > (1 << 24)) return HSCN_E_UNSUPPORTED;
  if (!params_host || !seg_off_host || !grads || !state_sum || !step_dev || !lr_dev) return HSCN_E_BADARG;
  if (!(lr_decay >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return HSCN_E_BADARG;
  if (!(max_norm > 0.0f) && max_norm != 0.0f) return HSCN_E_BADARG;   // (NaN / negative)
  AdagradArgs A;
  SchedArgs S{};
  if (scheduled(sched))
    if (int rc = fill_sched_args(S, sched, lr_dev, sched_state_dev)) return rc;
  if (P == 0) return 0;
  if (int rc = fill_tables(A.t.params, A.t.off, params_host, seg_off_host, nseg, P)) return rc;
  A.grads = grads; A.sum = state_sum; A.step = step_dev; A.lr = lr_dev; A.lr_decay = lr_decay; A.eps = eps;
  A.wd = weight_decay; A.norm_out = norm_out; A.max_norm = max_norm; A.nseg = nseg; A.P = (int)P;
  A.clip = max_norm > 0.0f; A.zero = zero_grads != 0;
  if (scheduled(sched)) k_adagrad_flat<true><<<1, 1024, 0, hscn_stream(stream)>>>(A, S);
  else k_adagrad_flat<false><<<1, 1024, 0, hscn_stream(stream)>>>(A, S);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int hscn_clip_grad_norm_flat(float* grads, int64_t P, float max_norm, float* norm_out, void* stream) {
  if (P < 0 || P > (1 << 24)) return HSCN_E_UNSUPPORTED;
  if (!(max_norm > 0.0f) || (P > 0 && !grads)) return HSCN_E_BADARG;
  if (P == 0) return 0;
  k_clip_grad_norm_flat<<<1, 1024, 0, hscn_stream(stream)>>>(grads, (int)P, max_norm, norm_out);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
