// Epoch metrics (reference graph_hscn/metrics.py:6-36): average precision per class and mean absolute error over the
// epoch's [G, C] labels and scores, on the device.  The torch restatement (graph_hscn/metrics.py: eval_ap) loops over
// the classes on the host, three read-backs and a float64 sort + cumsum dispatch per class; here one workgroup per
// class sorts 64-bit keys and scans the label bits, and a one-wave launch folds the classes.
//
// Key of a labelled row: (~image(score)) << 1 | (label == 1), where image() is the order-preserving unsigned image
// of the float with -0.0 canonicalised to +0.0 -- ascending keys are descending scores, equal scores are equal in
// key >> 1 (one threshold run), and inside a run the label order does not matter (tp is taken at the run's last
// row).  Rows with a NaN label, and the padding up to the power of two, carry the all-ones key and sort behind
// every labelled row.
//
// Layout.  n2 = G rounded up to a power of two keys of 8 B: in LDS for n2 <= 16384 (128 KB of the CU's 160 KB, plus
// 16 KB of scan / reduction scratch), in the caller's workspace beyond (the same code over a global pointer; the
// workgroup's own writes are visible to it behind __syncthreads).  After the bitonic sort thread t owns the
// contiguous chunk [t * chunk, (t + 1) * chunk) of the n labelled rows, chunk odd (lanes 8 B * odd apart: no LDS
// bank is hit twice by a lane group): pass 1 counts the chunk's positives and those up to its last run end, two
// block scans give every chunk the tp before it and the tp at the last run end before it (a max-scan: tp at run ends
// never decreases), pass 2 adds the chunk's terms in row order, and a fixed tree adds the 1024 chunk sums.  No atomics.
//
// Class-index targets (accuracy, macro-F1): the [C, C] confusion matrix.  A thread takes a row, finds the first
// maximal column and adds one to confusion[target][column] in the workgroup's LDS copy; the copies are added to the
// global matrix entry by entry.  Integer adds only: any order gives the same matrix.  A one-workgroup launch then
// reads the diagonal, the row sums and the column sums and writes accuracy and macro-F1 in float64, class by class.
#include "hscn_common.h"

namespace {

constexpr int MT = 1024;                       // threads of a class workgroup
constexpr int64_t AP_LDS_ROWS = 16384;         // keys that stay in LDS
constexpr size_t AP_STATIC_LDS = 2 * MT * sizeof(int) + MT * sizeof(double);   // k_ap_class's ibuf and dbuf: 16 KB
constexpr size_t AP_WS_HEAD = 256;             // workspace: per-class NaN-score words in front of the keys
constexpr uint64_t KEY_NONE = ~0ull;

__device__ __forceinline__ uint64_t ap_key(float s, bool positive) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;                                      // -0.0 ties +0.0
  const uint32_t img = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending with the float
  return ((uint64_t)(~img) << 1) | (positive ? 1ull : 0ull);
}

// sum of v over the workgroup, returned to every thread (fixed order; red: MT / 64 words)
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                                   // (red may still be read from the last call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < MT / 64; ++w) t += red[w];
  return t;
}

// exclusive scan over the workgroup's threads in `buf` [2 * MT]: OP = 0 sum, 1 max (identity 0: values are >= 0)
template <int OP>
__device__ __forceinline__ int block_exclusive_scan(int v, int* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  int* a = buf;
  int* b = buf + MT;
  a[t] = v;
  __syncthreads();
  for (int o = 1; o < MT; o <<= 1) {
    int x = a[t];
    if (t >= o) x = OP == 0 ? x + a[t - o] : max(x, a[t - o]);
    b[t] = x;
    __syncthreads();
    int* s = a; a = b; b = s;
  }
  return t == 0 ? 0 : a[t - 1];
}

template <typename KeyPtr>
__device__ __forceinline__ void bitonic_sort(KeyPtr keys, int64_t n2) {
  const int64_t half = n2 >> 1;
  for (int64_t k = 2; k <= n2; k <<= 1) {
    for (int64_t j = k >> 1; j > 0; j >>= 1) {
      for (int64_t idx = threadIdx.x; idx < half; idx += MT) {
        const int64_t lo = idx & (j - 1);
        const int64_t i = ((idx - lo) << 1) | lo;                     // bit j of i is 0
        const int64_t l = i | j;
        const uint64_t a = keys[i], b = keys[l];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { keys[i] = b; keys[l] = a; }
      }
      __syncthreads();
    }
  }
}

template <typename KeyPtr>
__device__ __forceinline__ void ap_class(KeyPtr keys, int64_t n2, const float* __restrict__ y_true,
                                         const float* __restrict__ y_score, int64_t G, int C, int c,
                                         double* __restrict__ ap, int32_t* __restrict__ valid,
                                         int32_t* __restrict__ nan_score, int* ibuf, double* dbuf) {
  const int t = threadIdx.x;
  int n_lab = 0, n_pos = 0, n_neg = 0, n_nan = 0;
  for (int64_t i = t; i < n2; i += MT) {
    uint64_t key = KEY_NONE;
    if (i < G) {
      const float y = y_true[i * C + c];
      const float s = y_score[i * C + c];
      if (y == y) {
        ++n_lab;
        n_pos += y == 1.0f;
        n_neg += y == 0.0f;
        n_nan += s != s;
        key = ap_key(s, y == 1.0f);
      }
    }
    keys[i] = key;
  }
  const int n = block_sum_int(n_lab, ibuf);
  const int P = block_sum_int(n_pos, ibuf);
  const int Z = block_sum_int(n_neg, ibuf);
  const int nans = block_sum_int(n_nan, ibuf);
  const bool ok = P > 0 && Z > 0;                                     // uniform over the workgroup
  if (!ok) {
    if (t == 0) { ap[c] = 0.0; valid[c] = 0; nan_score[c] = 0; }
    return;
  }
  __syncthreads();
  bitonic_sort(keys, n2);

  const int chunk = ((n + MT - 1) / MT) | 1;
  const int64_t first = (int64_t)t * chunk;
  const int64_t last = first + chunk < n ? first + chunk : n;         // (first >= n: an empty chunk)
  // pass 1: positives of the chunk, and positives up to its last run end (-1: no run ends here)
  int ones = 0, ones_at_end = -1;
  for (int64_t i = first; i < last; ++i) {
    const uint64_t k = keys[i];
    ones += (int)(k & 1ull);
    if (i + 1 == n || (keys[i + 1] >> 1) != (k >> 1)) ones_at_end = ones;
  }
  const int before = block_exclusive_scan<0>(ones, ibuf);
  const int tp_end = ones_at_end < 0 ? 0 : before + ones_at_end;
  const int tp_prev0 = block_exclusive_scan<1>(tp_end, ibuf);
  // pass 2: the chunk's terms (recall_run - recall_prev) * precision_run, in row order
  const double dP = (double)P;
  double r_prev = (double)tp_prev0 / dP, sum = 0.0;
  int tp = before;
  for (int64_t i = first; i < last; ++i) {
    const uint64_t k = keys[i];
    tp += (int)(k & 1ull);
    if (i + 1 == n || (keys[i + 1] >> 1) != (k >> 1)) {
      const double r = (double)tp / dP;
      sum += (r - r_prev) * ((double)tp / (double)(i + 1));
      r_prev = r;
    }
  }
  __syncthreads();
  dbuf[t] = sum;
  __syncthreads();
  for (int o = MT / 2; o > 0; o >>= 1) {
    if (t < o) dbuf[t] += dbuf[t + o];
    __syncthreads();
  }
  if (t == 0) { ap[c] = dbuf[0]; valid[c] = 1; nan_score[c] = nans > 0; }
}

template <bool IN_LDS>
__global__ void __launch_bounds__(MT) k_ap_class(const float* __restrict__ y_true, const float* __restrict__ y_score,
                                                 int64_t G, int C, int64_t n2, double* __restrict__ ap,
                                                 int32_t* __restrict__ valid, int32_t* __restrict__ nan_score,
                                                 uint64_t* __restrict__ ws_keys) {
  extern __shared__ uint64_t lds_keys[];
  __shared__ int ibuf[2 * MT];
  __shared__ double dbuf[MT];
  const int c = blockIdx.x;
  if (IN_LDS)
    ap_class(lds_keys, n2, y_true, y_score, G, C, c, ap, valid, nan_score, ibuf, dbuf);
  else
    ap_class(ws_keys + (int64_t)c * n2, n2, y_true, y_score, G, C, c, ap, valid, nan_score, ibuf, dbuf);
}

// the mean over the valid classes, in class order (one wave; lane 0 adds)
__global__ void __launch_bounds__(64) k_ap_finish(const double* __restrict__ ap, const int32_t* __restrict__ valid,
                                                  const int32_t* __restrict__ nan_score, int C,
                                                  double* __restrict__ result, int32_t* __restrict__ flags) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  int nv = 0, f = 0;
  for (int c = 0; c < C; ++c)
    if (valid[c]) {
      s += ap[c];
      ++nv;
      if (nan_score[c]) f |= 2;
    }
  if (nv == 0) f |= 1;
  result[0] = nv ? s / (double)nv : 0.0;
  result[1] = (double)nv;
  flags[0] = f;
}

__global__ void __launch_bounds__(MT) k_mae(const float* __restrict__ y_true, const float* __restrict__ y_pred,
                                            int64_t count, double* __restrict__ result, int32_t* __restrict__ flags) {
  __shared__ double dbuf[MT];
  __shared__ int ibuf[MT / 64];
  const int t = threadIdx.x;
  double s = 0.0;
  int nans = 0;
  for (int64_t i = t; i < count; i += MT) {
    const float p = y_pred[i];
    nans += p != p;
    s += fabs((double)y_true[i] - (double)p);
  }
  const int n_nan = block_sum_int(nans, ibuf);
  dbuf[t] = s;
  __syncthreads();
  for (int o = MT / 2; o > 0; o >>= 1) {
    if (t < o) dbuf[t] += dbuf[t + o];
    __syncthreads();
  }
  if (t == 0) {
    result[0] = dbuf[0] / (double)count;
    result[1] = (double)count;
    flags[0] = n_nan > 0 ? 2 : 0;
  }
}

constexpr int MC_THREADS = 256;
constexpr int MC_MAX_C = 128;                  // the confusion matrix fits 64 KB of LDS
constexpr int MC_MAX_BLOCKS = 256;
constexpr int MC_NAN = 2, MC_RANGE = 4;        // bits of `flags` (include/hscn.h)

__global__ void __launch_bounds__(MC_THREADS) k_mc_zero(int32_t* __restrict__ confusion, int n,
                                                        int32_t* __restrict__ flags) {
  for (int i = blockIdx.x * MC_THREADS + threadIdx.x; i < n; i += gridDim.x * MC_THREADS) confusion[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[0] = 0;
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_confusion(const int64_t* __restrict__ target,
                                                             const float* __restrict__ score, int64_t G, int C,
                                                             int32_t* __restrict__ confusion,
                                                             int32_t* __restrict__ flags) {
  extern __shared__ int32_t lds_conf[];
  const int n = C * C;
  for (int i = threadIdx.x; i < n; i += MC_THREADS) lds_conf[i] = 0;
  __syncthreads();
  int f = 0;
  for (int64_t r = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; r < G; r += (int64_t)gridDim.x * MC_THREADS) {
    const float* __restrict__ row = score + r * C;
    float best = row[0];
    int arg = 0;
    if (best != best) f |= MC_NAN;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v != v) f |= MC_NAN;
      if (v > best) { best = v; arg = c; }                 // strict: the first maximal column stays
    }
    const int64_t t = target[r];
    if (t < 0 || t >= C) { f |= MC_RANGE; continue; }
    atomicAdd(&lds_conf[(int)t * C + arg], 1);
  }
  if (f) atomicOr(flags, f);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += MC_THREADS) {
    const int v = lds_conf[i];
    if (v) atomicAdd(&confusion[i], v);
  }
}

// accuracy = trace / G; F1 of class c = 2 tp / (true_c + predicted_c), 0 where tp is 0; macro-F1 = the mean over the
// classes with true_c + predicted_c > 0 (sklearn's labels = unique(y_true U y_pred)), added in class order
__global__ void __launch_bounds__(MC_THREADS) k_mc_finish(const int32_t* __restrict__ confusion, int64_t G, int C,
                                                          double* __restrict__ result,
                                                          double* __restrict__ per_class) {
  __shared__ int s_tp[MC_MAX_C], s_present[MC_MAX_C];
  __shared__ double s_f1[MC_MAX_C];
  for (int c = threadIdx.x; c < C; c += MC_THREADS) {
    int64_t n_true = 0, n_pred = 0;
    for (int k = 0; k < C; ++k) {
      n_true += confusion[c * C + k];
      n_pred += confusion[k * C + c];
    }
    const int tp = confusion[c * C + c];
    const double f1 = tp > 0 ? 2.0 * (double)tp / (double)(n_true + n_pred) : 0.0;
    s_tp[c] = tp;
    s_present[c] = n_true + n_pred > 0;
    s_f1[c] = f1;
    per_class[c] = f1;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int64_t trace = 0;
  int labels = 0;
  double sum = 0.0;
  for (int c = 0; c < C; ++c) {
    trace += s_tp[c];
    if (s_present[c]) { sum += s_f1[c]; ++labels; }
  }
  result[0] = (double)trace / (double)G;
  result[1] = labels ? sum / (double)labels : 0.0;
}

int64_t ap_pow2(int64_t G) {
  int64_t n2 = 2;
  while (n2 < G) n2 <<= 1;
  return n2;
}

}  // namespace

extern "C" {

size_t hscn_average_precision_workspace_bytes(int64_t G, int C) {
  if (G < 1 || C < 1 || G > ((int64_t)1 << 30)) return 0;
  const int64_t n2 = ap_pow2(G);
  return AP_WS_HEAD * (((size_t)C * 4 + AP_WS_HEAD - 1) / AP_WS_HEAD) +
         (n2 > AP_LDS_ROWS ? (size_t)C * (size_t)n2 * 8 : 0);
}

int hscn_average_precision(const float* y_true, const float* y_score, int64_t G, int C, double* ap, int32_t* valid,
                           double* result, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream_) {
  if (G < 1 || C < 1 || G > ((int64_t)1 << 30) || !y_true || !y_score || !ap || !valid || !result || !flags ||
      !workspace)
    return HSCN_E_BADARG;
  if (workspace_bytes < hscn_average_precision_workspace_bytes(G, C)) return HSCN_E_WORKSPACE;
  const int64_t n2 = ap_pow2(G);
  const size_t head = AP_WS_HEAD * (((size_t)C * 4 + AP_WS_HEAD - 1) / AP_WS_HEAD);
  int32_t* nan_score = static_cast<int32_t*>(workspace);
  uint64_t* ws_keys = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + head);
  hipStream_t st = hscn_stream(stream_);
  if (n2 <= AP_LDS_ROWS) {   // the keys (a power of two of them, 128 KB at the most) beside the kernel's static scratch
    if (int rc = launch_with_lds<AP_STATIC_LDS>(k_ap_class<true>, (unsigned)C, MT, (size_t)n2 * 8, st, y_true, y_score,
                                                G, C, n2, ap, valid, nan_score, nullptr))
      return rc;
  } else {
    k_ap_class<false><<<(unsigned)C, MT, 0, st>>>(y_true, y_score, G, C, n2, ap, valid, nan_score, ws_keys);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  k_ap_finish<<<1, 64, 0, st>>>(ap, valid, nan_score, C, result, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_mean_absolute_error(const float* y_true, const float* y_pred, int64_t G, int C, double* result,
                             int32_t* flags, void* stream_) {
  if (G < 1 || C < 1 || G > ((int64_t)1 << 30) || !y_true || !y_pred || !result || !flags) return HSCN_E_BADARG;
  k_mae<<<1, MT, 0, hscn_stream(stream_)>>>(y_true, y_pred, G * (int64_t)C, result, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_multiclass_metrics(const int64_t* target, const float* score, int64_t G, int C, int32_t* confusion,
                            double* result, double* per_class, int32_t* flags, void* stream_) {
  if (G < 1 || C < 1 || C > MC_MAX_C || G > ((int64_t)1 << 30) || !target || !score || !confusion || !result ||
      !per_class || !flags)
    return HSCN_E_BADARG;
  hipStream_t st = hscn_stream(stream_);
  const int n = C * C;
  k_mc_zero<<<hscn_blocks(n, MC_THREADS), MC_THREADS, 0, st>>>(confusion, n, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  unsigned nb = hscn_blocks(G, MC_THREADS);
  if (nb > MC_MAX_BLOCKS) nb = MC_MAX_BLOCKS;
  k_mc_confusion<<<nb, MC_THREADS, (size_t)n * sizeof(int32_t), st>>>(target, score, G, C, confusion, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  k_mc_finish<<<1, MC_THREADS, 0, st>>>(confusion, G, C, result, per_class);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
