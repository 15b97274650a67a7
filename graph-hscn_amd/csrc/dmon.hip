// DMoN modularity pooling (Tsitsulin et al., "Graph Clustering with Graph Neural Networks"; PyG dense_dmon_pool) on
// the edge-list route, the sibling of mincut.hip.  A is never densified:
//   tr(S^T A S)   = sum_i S_i . (A S)_i,   (A S)_i = sum_{p in row i} S[col[p]]
//   d^T S, c      = sum_i d_i S_i, sum_i S_i,   d_i = |row i|,  2m = sum_i d_i
//   spectral      = -(tr(S^T A S) - |d^T S|^2 / 2m) / 2m         (0 for a graph without edges)
//   ortho         = | S^T S / |S^T S|_F - I / sqrt(K) |_F        (MinCUT's term)
//   cluster       = |c| sqrt(K) / n - 1
// One workgroup per graph: node tiles of S / (A S) / X are staged in LDS and every K x K, K x Fx and K-vector
// accumulator is an LDS cell owned by one thread, so all sums run in node order and are reproducible.  The row softmax
// stays a launch of its own, as in mincut.hip: (A S)_i gathers the S rows of whatever nodes the edge list names, so S
// has to be complete before the first tile, and one thread per row spreads the expf over all CUs instead of over G
// workgroups.
#include "hscn_common.h"

namespace {

constexpr int DM_THREADS = 256;
constexpr int DM_T = 16;      // nodes per LDS tile
constexpr int DM_STATS = 8;   // floats per graph in `stats` (include/hscn.h)

// One thread per row.  The K exponentials are summed and divided in double: the gradient of a small graph is
// ill-conditioned in S (a 2-node graph at K = 64: 3 ulp on S, what a float sum of 64 terms leaves, became 6e-8 on a
// gradient of 0.12), and a row is all the work there is here.
__global__ void k_dmon_softmax_rows(const float* __restrict__ logits, float* __restrict__ S, int64_t n, int K) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = logits + i * K;
  float m = r[0];
  for (int k = 1; k < K; ++k) m = fmaxf(m, r[k]);
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += (double)expf(r[k] - m);
  for (int k = 0; k < K; ++k) S[i * K + k] = (float)((double)expf(r[k] - m) / sum);
}

// wave-0 ordered reduction of f(idx) over idx in [0,n)
template <typename F>
__device__ __forceinline__ float wave0_reduce(int n, F f) {
  float v = 0.f;
  for (int idx = threadIdx.x; idx < n; idx += 64) v += f(idx);
  return wave_sum(v);
}

__device__ __forceinline__ float selu(float v) {
  const float alpha = 1.6732632423543772f, scale = 1.0507009873554805f;
  return scale * (v > 0.f ? v : alpha * expm1f(v));
}

// LDS floats: forward 2 K^2 + K Fx + 2 T K + T Fx + T + 3 K + 4, backward K^2 + 2 T K + 2 K + T + 4  (T = 16)
static size_t dmon_fwd_lds(int K, int Fx) {
  return (size_t)(2 * K * K + K * Fx + 2 * DM_T * K + DM_T * Fx + DM_T + 3 * K + 4) * 4;
}
static size_t dmon_bwd_lds(int K) { return (size_t)(K * K + 2 * DM_T * K + 2 * K + DM_T + 4) * 4; }
static_assert(DM_THREADS == 16 * DM_T, "k_dmon_bwd gives every row of a tile 16 lanes for its <dS, S>");

__global__ void __launch_bounds__(DM_THREADS)
k_dmon_stats(const float* __restrict__ S, const float* __restrict__ x, const int32_t* __restrict__ rowptr,
             const int32_t* __restrict__ col, const int32_t* __restrict__ node_ptr, float* __restrict__ stats,
             float* __restrict__ ss_out, float* __restrict__ vec_out, float* __restrict__ pooled_x,
             float* __restrict__ pooled_adj, int K, int Fx) {
  extern __shared__ __align__(16) float lds[];
  const int KK = K * K;
  float* acc_ss = lds;                 // [K][K]  S^T S
  float* acc_oa = acc_ss + KK;         // [K][K]  S^T A S
  float* acc_px = acc_oa + KK;         // [K][Fx] S^T X
  float* S_t = acc_px + K * Fx;        // [T][K]
  float* AS_t = S_t + DM_T * K;        // [T][K]
  float* x_t = AS_t + DM_T * K;        // [T][Fx]
  float* d_t = x_t + DM_T * Fx;        // [T]
  float* ds_a = d_t + DM_T;            // [K]  d^T S
  float* c_a = ds_a + K;               // [K]  sum_i S_i
  float* dn = c_a + K;                 // [K]

  const int g = blockIdx.x;
  const int n0 = node_ptr[g], n1 = node_ptr[g + 1];
  for (int idx = threadIdx.x; idx < 2 * KK + K * Fx; idx += DM_THREADS) lds[idx] = 0.f;
  for (int idx = threadIdx.x; idx < 2 * K; idx += DM_THREADS) ds_a[idx] = 0.f;   // (ds_a and c_a are adjacent)

  for (int base = n0; base < n1; base += DM_T) {
    const int nt = (n1 - base) < DM_T ? (n1 - base) : DM_T;
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * K; idx += DM_THREADS) {
      const int t = idx / K, k = idx - t * K;
      const int i = base + t;
      S_t[idx] = S[(size_t)i * K + k];
      float a = 0.f;
      for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) a += S[(size_t)col[p] * K + k];
      AS_t[idx] = a;
    }
    if (x)
      for (int idx = threadIdx.x; idx < nt * Fx; idx += DM_THREADS) x_t[idx] = x[(size_t)base * Fx + idx];
    for (int t = threadIdx.x; t < nt; t += DM_THREADS)
      d_t[t] = (float)(rowptr[base + t + 1] - rowptr[base + t]);
    __syncthreads();
    for (int idx = threadIdx.x; idx < KK; idx += DM_THREADS) {
      const int a = idx / K, b = idx - a * K;
      float s1 = acc_ss[idx], s2 = acc_oa[idx];
      for (int t = 0; t < nt; ++t) {
        const float sa = S_t[t * K + a];
        s1 = fmaf(sa, S_t[t * K + b], s1);
        s2 = fmaf(sa, AS_t[t * K + b], s2);
      }
      acc_ss[idx] = s1;
      acc_oa[idx] = s2;
    }
    if (x)
      for (int idx = threadIdx.x; idx < K * Fx; idx += DM_THREADS) {
        const int a = idx / Fx, f = idx - a * Fx;
        float s = acc_px[idx];
        for (int t = 0; t < nt; ++t) s = fmaf(S_t[t * K + a], x_t[t * Fx + f], s);
        acc_px[idx] = s;
      }
    for (int a = threadIdx.x; a < K; a += DM_THREADS) {
      float sd = ds_a[a], sc = c_a[a];
      for (int t = 0; t < nt; ++t) {
        const float sa = S_t[t * K + a];
        sd = fmaf(d_t[t], sa, sd);
        sc += sa;
      }
      ds_a[a] = sd;
      c_a[a] = sc;
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    // 2m = sum_i d_i = the graph's edge count, exact in integers
    const float two_m = (float)(rowptr[n1] - rowptr[n0]);
    const float trace = wave0_reduce(K, [&](int a) { return acc_oa[a * K + a]; });
    const float ds2 = wave0_reduce(K, [&](int a) { return ds_a[a] * ds_a[a]; });
    const float c2 = wave0_reduce(K, [&](int a) { return c_a[a] * c_a[a]; });
    const float nrm2 = wave0_reduce(KK, [&](int i) { return acc_ss[i] * acc_ss[i]; });
    const float nrm = sqrtf(nrm2);
    const float isk = 1.0f / sqrtf((float)K);
    const float o2 = wave0_reduce(KK, [&](int i) {
      const int a = i / K, b = i - a * K;
      const float q = acc_ss[i] / nrm - (a == b ? isk : 0.f);
      return q * q;
    });
    if (threadIdx.x == 0) {
      const float null_term = two_m > 0.f ? ds2 / two_m : 0.f;
      const float cnorm = sqrtf(c2);
      float* st = stats + (size_t)g * DM_STATS;
      st[0] = trace;
      st[1] = two_m;
      st[2] = null_term;
      st[3] = nrm;
      st[4] = sqrtf(o2);
      st[5] = cnorm;
      st[6] = two_m > 0.f ? -((trace - null_term) / two_m) : 0.f;
      st[7] = cnorm * sqrtf((float)K) / (float)(n1 - n0) - 1.0f;
    }
  }
  for (int idx = threadIdx.x; idx < KK; idx += DM_THREADS) ss_out[(size_t)g * KK + idx] = acc_ss[idx];
  for (int idx = threadIdx.x; idx < 2 * K; idx += DM_THREADS) vec_out[(size_t)g * 2 * K + idx] = ds_a[idx];
  if (pooled_x && x)
    for (int idx = threadIdx.x; idx < K * Fx; idx += DM_THREADS)
      pooled_x[(size_t)g * K * Fx + idx] = selu(acc_px[idx]);
  if (pooled_adj) {
    for (int a = threadIdx.x; a < K; a += DM_THREADS) {
      float s = 0.f;
      for (int b = 0; b < K; ++b) s += (a == b) ? 0.f : acc_oa[a * K + b];
      dn[a] = sqrtf(s) + 1e-15f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < KK; idx += DM_THREADS) {
      const int a = idx / K, b = idx - a * K;
      pooled_adj[(size_t)g * KK + idx] = (a == b) ? 0.f : (acc_oa[idx] / dn[b]) / dn[a];
    }
  }
}

__global__ void k_dmon_losses(const float* __restrict__ stats, float* __restrict__ losses, int G) {
  // single wave, ordered
  float sp = 0.f, o = 0.f, cl = 0.f;
  for (int g = threadIdx.x; g < G; g += 64) {
    sp += stats[(size_t)g * DM_STATS + 6];
    o += stats[(size_t)g * DM_STATS + 4];
    cl += stats[(size_t)g * DM_STATS + 7];
  }
  sp = wave_sum(sp);
  o = wave_sum(o);
  cl = wave_sum(cl);
  if (threadIdx.x == 0) {
    losses[0] = sp / (float)G;
    losses[1] = o / (float)G;
    losses[2] = cl / (float)G;
  }
}

__global__ void __launch_bounds__(DM_THREADS)
k_dmon_bwd(const float* __restrict__ S, const float* __restrict__ stats, const float* __restrict__ ss,
           const float* __restrict__ vec, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
           const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
           const int32_t* __restrict__ node_ptr, const float* __restrict__ g_losses, float* __restrict__ g_logits,
           int K, int G) {
  extern __shared__ __align__(16) float lds[];
  const int KK = K * K;
  float* Gss = lds;               // [K][K]  d ortho / d (S^T S)
  float* S_t = Gss + KK;          // [T][K]
  float* dS_t = S_t + DM_T * K;   // [T][K]
  float* dsv = dS_t + DM_T * K;   // [K]  d^T S
  float* cv = dsv + K;            // [K]  c
  float* dot_t = cv + K;          // [T]  <dS_i, S_i>
  float* red = dot_t + DM_T;      // [4]
  const int g = blockIdx.x;
  const int n0 = node_ptr[g], n1 = node_ptr[g + 1];
  const float* st = stats + (size_t)g * DM_STATS;
  const float two_m = st[1], nrm = st[3], o = st[4], cnorm = st[5];
  const float gsp = g_losses[0] / (float)G, go = g_losses[1] / (float)G, gcl = g_losses[2] / (float)G;
  const float isk = 1.0f / sqrtf((float)K);
  const float* ssg = ss + (size_t)g * KK;
  // inner = <Gq, ss>,  Gq = (ss/nrm - I/sqrt(K)) / o
  if (threadIdx.x < 64) {
    float v = 0.f;
    if (o > 0.f)
      for (int i = threadIdx.x; i < KK; i += 64) {
        const int a = i / K, b = i - a * K;
        v += ((ssg[i] / nrm - (a == b ? isk : 0.f)) / o) * ssg[i];
      }
    v = wave_sum(v);
    if (threadIdx.x == 0) red[0] = v;
  }
  for (int idx = threadIdx.x; idx < 2 * K; idx += DM_THREADS) dsv[idx] = vec[(size_t)g * 2 * K + idx];
  __syncthreads();
  const float inner = red[0];
  for (int i = threadIdx.x; i < KK; i += DM_THREADS) {
    const int a = i / K, b = i - a * K;
    const float gq = o > 0.f ? (ssg[i] / nrm - (a == b ? isk : 0.f)) / o : 0.f;
    Gss[i] = (gq - inner / (nrm * nrm) * ssg[i]) / nrm;
  }
  // d spectral / dS_ik = -(1/2m) [ (A S + A^T S)_ik - 2 d_i (d^T S)_k / 2m ]: nothing for a graph without edges
  const float c_sp = two_m > 0.f ? -gsp / two_m : 0.f;
  const float c_null = two_m > 0.f ? 2.f / two_m : 0.f;
  // d cluster / dS_ik = (sqrt(K) / n) c_k / |c|
  const float c_cl = cnorm > 0.f ? gcl * sqrtf((float)K) / (float)(n1 - n0) / cnorm : 0.f;
  for (int base = n0; base < n1; base += DM_T) {
    const int nt = (n1 - base) < DM_T ? (n1 - base) : DM_T;
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * K; idx += DM_THREADS) S_t[idx] = S[(size_t)base * K + idx];
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * K; idx += DM_THREADS) {
      const int t = idx / K, k = idx - t * K;
      const int i = base + t;
      float as = 0.f;
      for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) as += S[(size_t)col[p] * K + k];
      for (int q = rowptr_t[i]; q < rowptr_t[i + 1]; ++q) as += S[(size_t)col_t[q] * K + k];
      const float d_i = (float)(rowptr[i + 1] - rowptr[i]);
      // four interleaved partial sums, joined pairwise: a fixed order, a quarter of one chain's rounding growth
      float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
      int a = 0;
      for (; a + 3 < K; a += 4) {
        o0 = fmaf(S_t[t * K + a], Gss[a * K + k], o0);
        o1 = fmaf(S_t[t * K + a + 1], Gss[(a + 1) * K + k], o1);
        o2 = fmaf(S_t[t * K + a + 2], Gss[(a + 2) * K + k], o2);
        o3 = fmaf(S_t[t * K + a + 3], Gss[(a + 3) * K + k], o3);
      }
      for (; a < K; ++a) o0 = fmaf(S_t[t * K + a], Gss[a * K + k], o0);
      const float orth = (o0 + o1) + (o2 + o3);
      // Gss is symmetric: d o / dS = S (Gss + Gss^T) = 2 S Gss
      dS_t[idx] = c_sp * (as - c_null * d_i * dsv[k]) + go * 2.f * orth + c_cl * cv[k];
    }
    __syncthreads();
    {
      // <dS_i, S_i> once per row: 16 lanes take every 16th cluster, then the butterfly over those 16 lanes (every lane
      // of the wave takes part in the shuffles; a row beyond the tile carries zeros)
      const int t = threadIdx.x >> 4, j = threadIdx.x & 15;
      float v = 0.f;
      if (t < nt)
        for (int a = j; a < K; a += 16) v = fmaf(dS_t[t * K + a], S_t[t * K + a], v);
      v = group_sum(v, 16);
      if (j == 0 && t < nt) dot_t[t] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * K; idx += DM_THREADS)
      g_logits[(size_t)base * K + idx] = S_t[idx] * (dS_t[idx] - dot_t[idx / K]);
  }
}

}  // namespace

extern "C" {

int hscn_dmon_sparse_fwd(const float* logits, const float* x, const int32_t* rowptr, const int32_t* col,
                         const int32_t* node_ptr, float* S, float* stats, float* ss, float* vec, float* pooled_x,
                         float* pooled_adj, float* losses, int64_t num_nodes, int64_t num_graphs, int K, int Fx,
                         void* stream_) {
  if (num_nodes < 0 || num_graphs < 1 || K < 1 || K > 256 || Fx < 0) return HSCN_E_BADARG;
  if (!logits || !rowptr || !col || !node_ptr || !S || !stats || !ss || !vec || !losses) return HSCN_E_BADARG;
  if (!x) Fx = 0;
  const size_t lds = dmon_fwd_lds(K, Fx);
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  hipStream_t st = hscn_stream(stream_);
  if (num_nodes > 0) {
    k_dmon_softmax_rows<<<hscn_blocks(num_nodes, 256), 256, 0, st>>>(logits, S, num_nodes, K);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  if (int rc = launch_with_lds(k_dmon_stats, (unsigned)num_graphs, DM_THREADS, lds, st, S, x, rowptr, col, node_ptr,
                               stats, ss, vec, pooled_x, pooled_adj, K, Fx))
    return rc;
  k_dmon_losses<<<1, 64, 0, st>>>(stats, losses, (int)num_graphs);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_dmon_sparse_bwd(const float* S, const float* stats, const float* ss, const float* vec,
                         const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t,
                         const int32_t* node_ptr, const float* g_losses, float* g_logits, int64_t num_nodes,
                         int64_t num_graphs, int K, void* stream_) {
  if (num_nodes < 0 || num_graphs < 1 || K < 1 || K > 256) return HSCN_E_BADARG;
  if (!S || !stats || !ss || !vec || !rowptr || !col || !rowptr_t || !col_t || !node_ptr || !g_losses || !g_logits)
    return HSCN_E_BADARG;
  const size_t lds = dmon_bwd_lds(K);
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  return launch_with_lds(k_dmon_bwd, (unsigned)num_graphs, DM_THREADS, lds, hscn_stream(stream_), S, stats, ss, vec,
                         rowptr, col, rowptr_t, col_t, node_ptr, g_losses, g_logits, K, (int)num_graphs);
}

}  // extern "C"
