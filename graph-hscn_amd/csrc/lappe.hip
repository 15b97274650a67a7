// LapPE node encoder, DeepSet model (GraphGPS's LapPENodeEncoder): per node i and frequency k the pair
// u_ik = (s_k vec[i,k], val[i,k]) goes through `layers` Linear + ReLU (widths 2 -> 2 dim_pe -> ... -> dim_pe) and the
// results of the frequencies that are not NaN padding are summed: pe_sum [N, dim_pe].  s_k = -1 iff `flip` and word 0 of
// philox4x32_10(seed, k) >= 2^31: one sign per frequency column, never stored.
//
// Forward: ONE launch.  A workgroup is four waves over the same 64 nodes, one node per lane; wave q takes the frequencies
// k = q, q + 4, ...  The parameters sit transposed in LDS and are read as broadcasts (every lane of a wave reads the
// same address), the chain lives in registers with the widths as template parameters, and the [N, K, H] activations
// never reach HBM.  A lane adds its frequencies in ascending order, waves 1..3 hand their sums over through LDS and
// wave 0 adds them in wave order: a node's row is a fixed sequence of operations on its own statistics and the
// parameters, whatever N, its place in the batch or the grid.
//
// Backward (parameters only): a workgroup walks a contiguous range of the N K (node, frequency) samples S at a time
// (S = 256, 128, 64 or 32, the largest whose rows fit 64 KB of LDS beside the parameters and their gradient).  Per pass
// it recomputes the chain with the forward's own fmaf order (so every ReLU gate is the forward's), keeps the
// activations of the pass in LDS, walks the layers down -- delta^l, then delta^l (x) [a^{l-1} | 1] summed over the
// samples of the pass in sample order into the workgroup's accumulators (LDS, one owner thread per parameter) -- and
// stores its partial gradient to the workspace; a second launch folds the partials in workgroup order (the fixed tree
// of csrc/linear.hip).  No float atomics: two runs give the same bits.
#include "hscn_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_FWD_NODES = 64;      // forward: nodes per workgroup (hscn_lappe_tile), one per lane of a wave
constexpr int LP_FWD_SPLIT = LP_THREADS / LP_FWD_NODES;   // waves of a workgroup: wave q takes the frequencies k = q mod 4
constexpr int LP_MAX_LAYERS = 4;
constexpr int LP_MAX_FREQS = 64;      // hscn_lap_eig_stats' cap
constexpr int LP_MAX_DIM = 32;
constexpr int LP_BWD_MAX_SAMPLES = 256;   // backward: samples per pass, a power of two in [32, 256]: the largest whose
constexpr size_t LP_BWD_LDS_BYTES = 64 * 1024;    // rows, beside the parameters and their gradient, fit this much LDS
constexpr int LP_BWD_MAX_CHUNKS = 512;

struct LappeParams {
  const float* W[LP_MAX_LAYERS];
  const float* b[LP_MAX_LAYERS];
};

__host__ __device__ inline int lp_in(int l, int dp) { return l == 0 ? 2 : 2 * dp; }
__host__ __device__ inline int lp_out(int l, int L, int dp) { return l == L - 1 ? dp : 2 * dp; }
__host__ __device__ inline int lp_param_count(int L, int dp) {
  int p = 0;
  for (int l = 0; l < L; ++l) p += (lp_in(l, dp) + 1) * lp_out(l, L, dp);
  return p;
}

inline bool lp_supported(int K, int dp, int L) {
  return K >= 1 && K <= LP_MAX_FREQS && dp >= 4 && dp <= LP_MAX_DIM && dp % 4 == 0 && L >= 1 && L <= LP_MAX_LAYERS;
}

// (a kernel argument indexed by a runtime layer would be copied to scratch)
__device__ __forceinline__ const float* lp_pick(const float* p0, const float* p1, const float* p2, const float* p3, int l) {
  return l == 0 ? p0 : (l == 1 ? p1 : (l == 2 ? p2 : p3));
}
__device__ __forceinline__ const float* lp_W(const LappeParams& P, int l) { return lp_pick(P.W[0], P.W[1], P.W[2], P.W[3], l); }
__device__ __forceinline__ const float* lp_b(const LappeParams& P, int l) { return lp_pick(P.b[0], P.b[1], P.b[2], P.b[3], l); }

__device__ __forceinline__ float lp_sign(int flip, uint64_t seed, int k) {
  if (!flip) return 1.f;
  uint32_t c[4];
  philox4x32_10(seed, (uint64_t)k, c);
  return c[0] >= 0x80000000u ? -1.f : 1.f;
}

// y = relu(b + W a), Wt = W transposed [I][O] in LDS: y[o] starts at b[o] and takes fmaf(a[i], W[o][i], .) for i ascending
template <int I, int O>
__device__ __forceinline__ void lp_dense_relu(const float* __restrict__ Wt, const float* __restrict__ b,
                                              const float (&a)[I], float (&y)[O]) {
#pragma unroll
  for (int o = 0; o < O; ++o) y[o] = b[o];
#pragma unroll
  for (int i = 0; i < I; ++i) {
#pragma unroll
    for (int o = 0; o < O; ++o) y[o] = fmaf(a[i], Wt[i * O + o], y[o]);
  }
#pragma unroll
  for (int o = 0; o < O; ++o) y[o] = y[o] > 0.f ? y[o] : 0.f;
}

template <int DP>
__global__ void __launch_bounds__(LP_THREADS)
k_lappe_fwd(const float* __restrict__ vec, const float* __restrict__ val, LappeParams P, float* __restrict__ out,
            int64_t N, int K, int L, int flip, uint64_t seed) {
  constexpr int HID = 2 * DP;
  extern __shared__ __align__(16) float lds[];
  {
    int off = 0;
#pragma unroll
    for (int l = 0; l < LP_MAX_LAYERS; ++l) {
      if (l < L) {
        const int I = lp_in(l, DP), O = lp_out(l, L, DP);
        const float* W = P.W[l];
        const float* b = P.b[l];
        for (int idx = threadIdx.x; idx < I * O; idx += LP_THREADS) {
          const int i = idx / O, o = idx - i * O;
          lds[off + idx] = W[o * I + i];
        }
        for (int idx = threadIdx.x; idx < O; idx += LP_THREADS) lds[off + I * O + idx] = b[idx];
        off += (I + 1) * O;
      }
    }
  }
  __syncthreads();
  float* part = lds + lp_param_count(L, DP);       // [LP_FWD_SPLIT - 1][DP][LP_FWD_NODES]: waves 1.. hand their sums over
  const int t = threadIdx.x & (LP_FWD_NODES - 1), q = threadIdx.x / LP_FWD_NODES;
  const int64_t node = (int64_t)blockIdx.x * LP_FWD_NODES + t;
  const bool live = node < N;
  float acc[DP];
#pragma unroll
  for (int o = 0; o < DP; ++o) acc[o] = 0.f;
  for (int k = q; live && k < K; k += LP_FWD_SPLIT) {
    const float v = vec[node * K + k], lam = val[node * K + k];
    const bool valid = v == v;                     // NaN marks padding
    float u[2];
    u[0] = valid ? lp_sign(flip, seed, k) * v : 0.f;
    u[1] = lam == lam ? lam : 0.f;
    if (L == 1) {
      float y[DP];
      lp_dense_relu<2, DP>(lds, lds + 2 * DP, u, y);
#pragma unroll
      for (int o = 0; o < DP; ++o) acc[o] += valid ? y[o] : 0.f;
    } else {
      float a[HID];
      lp_dense_relu<2, HID>(lds, lds + 2 * HID, u, a);
      int off = 3 * HID;
      for (int l = 1; l < L - 1; ++l) {
        float y[HID];
        lp_dense_relu<HID, HID>(lds + off, lds + off + HID * HID, a, y);
#pragma unroll
        for (int o = 0; o < HID; ++o) a[o] = y[o];
        off += (HID + 1) * HID;
      }
      float z[DP];
      lp_dense_relu<HID, DP>(lds + off, lds + off + HID * DP, a, z);
#pragma unroll
      for (int o = 0; o < DP; ++o) acc[o] += valid ? z[o] : 0.f;
    }
  }
  if (q > 0) {
#pragma unroll
    for (int o = 0; o < DP; ++o) part[((q - 1) * DP + o) * LP_FWD_NODES + t] = acc[o];
  }
  __syncthreads();
  if (q > 0 || !live) return;
#pragma unroll
  for (int w = 0; w < LP_FWD_SPLIT - 1; ++w) {     // the waves' sums in wave order
#pragma unroll
    for (int o = 0; o < DP; ++o) acc[o] += part[(w * DP + o) * LP_FWD_NODES + t];
  }
  float4* dst = reinterpret_cast<float4*>(out + node * DP);
#pragma unroll
  for (int o = 0; o < DP; o += 4) dst[o >> 2] = make_float4(acc[o], acc[o + 1], acc[o + 2], acc[o + 3]);
}

// rows of the pass in LDS: [S][R], R odd; columns [0, 2) u, then a^0 .. a^{L-2} (2 dp each), then the two
// delta buffers (2 dp each), layer l's delta in buffer (L - 1 - l) & 1
__host__ __device__ inline int lp_row_stride(int L, int dp) { return (2 + (L + 1) * 2 * dp) | 1; }

__global__ void __launch_bounds__(LP_THREADS)
k_lappe_bwd_partial(const float* __restrict__ vec, const float* __restrict__ val, const float* __restrict__ g,
                    LappeParams P, float* __restrict__ partial, int K, int L, int dp, int flip, uint64_t seed,
                    int64_t M, int64_t per_chunk, int S) {
  extern __shared__ __align__(16) float lds[];
  const int HID = 2 * dp, R = lp_row_stride(L, dp), PT = lp_param_count(L, dp);
  float* Wl = lds;                                 // the parameters, flat as the tensors are: W_l [O][I], b_l [O], ...
  float* accL = lds + PT;                          // the workgroup's gradient, same layout
  float* rows = lds + 2 * PT;
  const int t = threadIdx.x & (S - 1), q = threadIdx.x / S;     // S a power of two: S samples x Q threads each
  const int Q = LP_THREADS / S;
  const int colD = 2 + (L - 1) * HID;
  {
    int off = 0;
    for (int l = 0; l < L; ++l) {
      const int I = lp_in(l, dp), O = lp_out(l, L, dp);
      const float* __restrict__ W = lp_W(P, l);
      const float* __restrict__ b = lp_b(P, l);
      for (int idx = threadIdx.x; idx < I * O; idx += LP_THREADS) Wl[off + idx] = W[idx];
      for (int idx = threadIdx.x; idx < O; idx += LP_THREADS) Wl[off + I * O + idx] = b[idx];
      off += (I + 1) * O;
    }
  }
  for (int p = threadIdx.x; p < PT; p += LP_THREADS) accL[p] = 0.f;
  const int64_t s_begin = (int64_t)blockIdx.x * per_chunk;
  int64_t s_end = s_begin + per_chunk;
  if (s_end > M) s_end = M;
  float* row = rows + t * R;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += S) {
    const int64_t s = s0 + t;
    const bool in = s < s_end;
    const int64_t node = in ? s / K : 0;
    const int k = in ? (int)(s - node * K) : 0;
    float v = 0.f, lam = 0.f;
    if (in) { v = vec[s]; lam = val[s]; }
    const bool valid = in && v == v;
    __syncthreads();                               // the parameters are staged / the last pass's readers are done
    if (q == 0) {
      row[0] = valid ? lp_sign(flip, seed, k) * v : 0.f;
      row[1] = lam == lam ? lam : 0.f;
    }
    __syncthreads();
    // the chain, in the forward's fmaf order, four outputs a turn (every width is a multiple of 4); the last layer
    // leaves delta^{L-1} = gate * g
    int woff = 0;
    for (int l = 0; l < L; ++l) {
      const int I = lp_in(l, dp), O = lp_out(l, L, dp);
      const float* W = Wl + woff;
      const float* b = W + I * O;
      const float* src = row + (l == 0 ? 0 : 2 + (l - 1) * HID);
      for (int o = 4 * q; o < O; o += 4 * Q) {
        float y0 = b[o], y1 = b[o + 1], y2 = b[o + 2], y3 = b[o + 3];
        const float* w0 = W + o * I;
        for (int i = 0; i < I; ++i) {
          const float a = src[i];
          y0 = fmaf(a, w0[i], y0);
          y1 = fmaf(a, w0[I + i], y1);
          y2 = fmaf(a, w0[2 * I + i], y2);
          y3 = fmaf(a, w0[3 * I + i], y3);
        }
        const float y[4] = {y0, y1, y2, y3};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (l < L - 1) row[2 + l * HID + o + j] = y[j] > 0.f ? y[j] : 0.f;
          else row[colD + o + j] = (valid && y[j] > 0.f) ? g[node * dp + o + j] : 0.f;
        }
      }
      woff += (I + 1) * O;
      __syncthreads();
    }
    int poff = PT;
    for (int l = L - 1; l >= 0; --l) {
      const int I = lp_in(l, dp), O = lp_out(l, L, dp);
      poff -= (I + 1) * O;
      const int cur = colD + (((L - 1 - l) & 1) ? HID : 0), nxt = colD + (((L - 1 - l) & 1) ? 0 : HID);
      const int colA = l == 0 ? 0 : 2 + (l - 1) * HID;
      // this pass's share of [gW_l | gb_l]: the samples of the pass in sample order
      for (int r = threadIdx.x; r < (I + 1) * O; r += LP_THREADS) {
        float sum = 0.f;
        if (r < I * O) {
          const int o = r / I, i = r - o * I;
          const float* d = rows + cur + o;
          const float* a = rows + colA + i;
#pragma unroll 8
          for (int tt = 0; tt < S; ++tt) sum = fmaf(d[tt * R], a[tt * R], sum);
        } else {
          const float* d = rows + cur + (r - I * O);
#pragma unroll 8
          for (int tt = 0; tt < S; ++tt) sum += d[tt * R];
        }
        accL[poff + r] += sum;
      }
      if (l > 0) {                                 // delta^{l-1} = gate(a^{l-1}) * W_l^T delta^l, four inputs a turn
        const float* W = Wl + poff;
        for (int i = 4 * q; i < I; i += 4 * Q) {
          float s0_ = 0.f, s1_ = 0.f, s2_ = 0.f, s3_ = 0.f;
          for (int o = 0; o < O; ++o) {
            const float d = row[cur + o];
            const float* w = W + o * I + i;
            s0_ = fmaf(d, w[0], s0_);
            s1_ = fmaf(d, w[1], s1_);
            s2_ = fmaf(d, w[2], s2_);
            s3_ = fmaf(d, w[3], s3_);
          }
          const float sv[4] = {s0_, s1_, s2_, s3_};
#pragma unroll
          for (int j = 0; j < 4; ++j) row[nxt + i + j] = row[colA + i + j] > 0.f ? sv[j] : 0.f;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < PT; p += LP_THREADS) partial[(size_t)blockIdx.x * PT + p] = accL[p];
}

// gflat[p] = sum over the G workgroups of partial[g][p] in a FIXED tree (csrc/linear.hip k_linear_bwd_w_reduce's): a
// block owns 32 parameters x 8 contiguous slices of workgroups, a slice is summed in workgroup order, the slices are
// folded in slice order
__global__ void __launch_bounds__(256)
k_lappe_bwd_fold(const float* __restrict__ partial, float* __restrict__ gflat, int G, int PT) {
  __shared__ float red[8][32];
  const int pl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int p = blockIdx.x * 32 + pl;
  const int per = (G + 7) / 8;
  const int g0 = sl * per, g1 = (g0 + per) < G ? (g0 + per) : G;
  float s = 0.f;
  if (p < PT) {
    int gi = g0;
    for (; gi + 16 <= g1; gi += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(gi + u) * PT + p];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; gi < g1; ++gi) s += partial[(size_t)gi * PT + p];
  }
  red[sl][pl] = s;
  __syncthreads();
  if (sl != 0 || p >= PT) return;
  s = 0.f;
#pragma unroll
  for (int qd = 0; qd < 8; ++qd) s += red[qd][pl];
  gflat[p] = s;
}

inline int lp_bwd_samples(int L, int dp) {
  int S = LP_BWD_MAX_SAMPLES;                      // (32 samples always fit the CU's 160 KB: 126 KB at the widest)
  while (S > 32 && ((size_t)S * lp_row_stride(L, dp) + 2 * lp_param_count(L, dp)) * 4 > LP_BWD_LDS_BYTES) S >>= 1;
  return S;
}

// workgroups of the backward: one per 256 samples (whatever a pass holds), at most LP_BWD_MAX_CHUNKS
inline int lp_chunks(int64_t M) {
  int64_t passes = (M + LP_BWD_MAX_SAMPLES - 1) / LP_BWD_MAX_SAMPLES;
  if (passes < 1) passes = 1;
  return (int)(passes > LP_BWD_MAX_CHUNKS ? LP_BWD_MAX_CHUNKS : passes);
}

inline int lp_load_params(const void* const* params_host, int L, LappeParams& P) {
  for (int l = 0; l < LP_MAX_LAYERS; ++l) {
    P.W[l] = l < L ? (const float*)params_host[2 * l] : nullptr;
    P.b[l] = l < L ? (const float*)params_host[2 * l + 1] : nullptr;
    if (l < L && (!P.W[l] || !P.b[l])) return HSCN_E_BADARG;
  }
  return 0;
}

}  // namespace

extern "C" {

int hscn_lappe_supported(int max_freqs, int dim_pe, int layers) { return lp_supported(max_freqs, dim_pe, layers) ? 1 : 0; }

int hscn_lappe_tile(void) { return LP_FWD_NODES; }

int64_t hscn_lappe_workspace_floats(int64_t N, int max_freqs, int dim_pe, int layers) {
  if (N < 0 || !lp_supported(max_freqs, dim_pe, layers)) return 0;
  return (int64_t)lp_chunks(N * max_freqs) * lp_param_count(layers, dim_pe);
}

int hscn_lappe_fwd(const float* vec, const float* val, const void* const* params_host, int64_t N, int max_freqs,
                   int dim_pe, int layers, int flip, uint64_t seed, float* out, void* stream_) {
  if (N < 0 || !params_host || (N > 0 && (!vec || !val || !out))) return HSCN_E_BADARG;
  if (!lp_supported(max_freqs, dim_pe, layers)) return HSCN_E_UNSUPPORTED;
  LappeParams P;
  if (int rc = lp_load_params(params_host, layers, P)) return rc;
  if (N == 0) return 0;
  if (!aligned16(out)) return HSCN_E_BADARG;
  hipStream_t st = hscn_stream(stream_);
  const size_t lds = ((size_t)lp_param_count(layers, dim_pe) + (LP_FWD_SPLIT - 1) * dim_pe * LP_FWD_NODES) * 4;
  const unsigned grid = hscn_blocks(N, LP_FWD_NODES);
#define HSCN_LP_FWD(DP_) \
  case DP_: return launch_with_lds(k_lappe_fwd<DP_>, grid, LP_THREADS, lds, st, vec, val, P, out, N, max_freqs, layers, \
                                   flip ? 1 : 0, seed);
  switch (dim_pe) {
    HSCN_LP_FWD(4) HSCN_LP_FWD(8) HSCN_LP_FWD(12) HSCN_LP_FWD(16)
    HSCN_LP_FWD(20) HSCN_LP_FWD(24) HSCN_LP_FWD(28) HSCN_LP_FWD(32)
  }
#undef HSCN_LP_FWD
  return HSCN_E_UNSUPPORTED;
}

int hscn_lappe_bwd(const float* vec, const float* val, const float* g_out, const void* const* params_host, int64_t N,
                   int max_freqs, int dim_pe, int layers, int flip, uint64_t seed, float* g_params, float* workspace,
                   int64_t workspace_floats, void* stream_) {
  if (N < 0 || !params_host || !g_params || (N > 0 && (!vec || !val || !g_out || !workspace))) return HSCN_E_BADARG;
  if (!lp_supported(max_freqs, dim_pe, layers)) return HSCN_E_UNSUPPORTED;
  LappeParams P;
  if (int rc = lp_load_params(params_host, layers, P)) return rc;
  if (N == 0) return 0;
  if (workspace_floats < hscn_lappe_workspace_floats(N, max_freqs, dim_pe, layers)) return HSCN_E_WORKSPACE;
  hipStream_t st = hscn_stream(stream_);
  const int64_t M = N * max_freqs;
  const int G = lp_chunks(M), PT = lp_param_count(layers, dim_pe);
  const int S = lp_bwd_samples(layers, dim_pe);
  const int64_t passes = (M + LP_BWD_MAX_SAMPLES - 1) / LP_BWD_MAX_SAMPLES;
  const int64_t per_chunk = (passes + G - 1) / G * LP_BWD_MAX_SAMPLES;
  const size_t lds = ((size_t)S * lp_row_stride(layers, dim_pe) + 2 * PT) * 4;
  if (int rc = launch_with_lds(k_lappe_bwd_partial, (unsigned)G, LP_THREADS, lds, st, vec, val, g_out, P, workspace,
                               max_freqs, layers, dim_pe, flip ? 1 : 0, seed, M, per_chunk, S))
    return rc;
  k_lappe_bwd_fold<<<hscn_blocks(PT, 32), 256, 0, st>>>(workspace, g_params, G, PT);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
