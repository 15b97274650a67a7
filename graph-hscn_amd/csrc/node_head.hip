// The per-node head of a node-level model: pred = lin_2(act(lin_1(x))) on every row of x [N, H] (the head of
// model/hscn.py:112-113 applied to the local nodes instead of the pooled graphs).  With the layered operators the head
// and its backward are nine launches over [N, H] rows whose hidden activation makes two round trips through HBM; here
// the forward is one launch and the backward one launch plus one ordered fold, and the hidden row never leaves
// registers.
//
// Mapping.  A lane owns a row: it holds x[H] and h[H] in registers (H is a template parameter, the loops unroll), and
// reads W1 [H, H], b1, W2 [C, H], b2 from LDS, every lane of a wave at the same address (a broadcast: no bank
// conflicts).  A workgroup is 256 lanes = NH_ROWS rows per tile.  H <= 64 and C <= 64: the weights are at most 33 KB.
//
// Backward.  The lane recomputes h from x, forms g_h = sum_c g_pred[c] W2[c, :] (g_pred times the optional device
// scalar), g_pre = g_h act'(h) and g_x = g_pre W1, and writes g_x.  The parameter gradients are sums over ROWS, that
// is over lanes: the tile's four waves take turns to lay their 64 rows {g_pre | g_pred | x | h} into one LDS sub-tile
// (row stride odd: lanes 4 B * odd apart), and all 256 threads then walk it, thread t owning the pairs p = t, t +
// 256, ... of gW1|gb1 [H, H + 1] followed by gW2|gb2 [C, H + 1] (the bias is the column whose input is 1), one fmaf
// per row in row order.  A workgroup strides over the tiles (at most NH_MAX_WG workgroups), keeps its pair sums in
// registers across them and writes them to its row of the workspace; a one-workgroup launch adds the rows in workgroup
// order and stores -- or, with `accumulate`, adds last into -- the four gradients.  No float atomics: the same input
// gives the same bits.
#include "hscn_common.h"

namespace {

constexpr int NH_THREADS = 256;
constexpr int NH_ROWS = 256;        // rows of a tile: one per lane
constexpr int NH_MAX_WG = 256;      // workgroups of the backward (rows of the workspace)
constexpr int NH_MAX_C = 64;
constexpr int NH_FOLD_THREADS = 1024;

inline bool nh_supported(int H, int C) { return (H == 16 || H == 32 || H == 64) && C >= 1 && C <= NH_MAX_C; }
inline int nh_pairs(int H, int C) { return (H + C) * (H + 1); }
inline int64_t nh_tiles(int64_t N) { return (N + NH_ROWS - 1) / NH_ROWS; }
inline int nh_bwd_wgs(int64_t N) {
  const int64_t t = nh_tiles(N);
  return (int)(t < 1 ? 1 : (t > NH_MAX_WG ? NH_MAX_WG : t));
}

// W1 [H, H], b1 [H], W2 [C, H], b2 [C] into LDS, in that order
template <int H>
__device__ __forceinline__ void nh_load_weights(float* lds, const float* __restrict__ W1, const float* __restrict__ b1,
                                                const float* __restrict__ W2, const float* __restrict__ b2, int C) {
  float* W1s = lds;
  float* b1s = W1s + H * H;
  float* W2s = b1s + H;
  float* b2s = W2s + C * H;
  for (int i = threadIdx.x; i < H * H; i += NH_THREADS) W1s[i] = W1[i];
  for (int i = threadIdx.x; i < H; i += NH_THREADS) b1s[i] = b1[i];
  for (int i = threadIdx.x; i < C * H; i += NH_THREADS) W2s[i] = W2[i];
  for (int i = threadIdx.x; i < C; i += NH_THREADS) b2s[i] = b2[i];
}

template <int H>
__device__ __forceinline__ void nh_load_row(const float* __restrict__ x, int64_t r, float (&xr)[H]) {
  const float4* p = reinterpret_cast<const float4*>(x + r * H);     // (H * 4 B rows: 16 B aligned)
#pragma unroll
  for (int q = 0; q < H / 4; ++q) {
    const float4 t = p[q];
    xr[4 * q] = t.x; xr[4 * q + 1] = t.y; xr[4 * q + 2] = t.z; xr[4 * q + 3] = t.w;
  }
}

// h = act(b1 + W1 x): one fmaf chain per hidden unit, inputs in index order
template <int H>
__device__ __forceinline__ void nh_hidden(const float (&xr)[H], const float* W1s, const float* b1s, int act,
                                          float (&h)[H]) {
#pragma unroll
  for (int k = 0; k < H; ++k) {
    float a = b1s[k];
#pragma unroll
    for (int i = 0; i < H; ++i) a = fmaf(xr[i], W1s[k * H + i], a);
    h[k] = apply_act(a, act);
  }
}

template <int H>
__global__ void __launch_bounds__(NH_THREADS) k_node_head_fwd(const float* __restrict__ x, const float* __restrict__ W1,
                                                              const float* __restrict__ b1,
                                                              const float* __restrict__ W2,
                                                              const float* __restrict__ b2, int64_t N, int C, int act,
                                                              float* __restrict__ pred) {
  extern __shared__ __align__(16) float lds[];
  nh_load_weights<H>(lds, W1, b1, W2, b2, C);
  __syncthreads();
  const float* W1s = lds;
  const float* b1s = W1s + H * H;
  const float* W2s = b1s + H;
  const float* b2s = W2s + C * H;
  const int64_t r = (int64_t)blockIdx.x * NH_ROWS + threadIdx.x;
  if (r >= N) return;
  float xr[H], h[H];
  nh_load_row<H>(x, r, xr);
  nh_hidden<H>(xr, W1s, b1s, act, h);
  float* __restrict__ out = pred + r * C;
  for (int c = 0; c < C; ++c) {
    float a = b2s[c];
#pragma unroll
    for (int k = 0; k < H; ++k) a = fmaf(h[k], W2s[c * H + k], a);
    out[c] = a;
  }
}

template <int H>
__global__ void __launch_bounds__(NH_THREADS) k_node_head_bwd(const float* __restrict__ x, const float* __restrict__ W1,
                                                              const float* __restrict__ b1,
                                                              const float* __restrict__ W2,
                                                              const float* __restrict__ b2,
                                                              const float* __restrict__ g_pred,
                                                              const float* __restrict__ scale, int64_t N, int C,
                                                              int act, float* __restrict__ g_x,
                                                              float* __restrict__ partial) {
  extern __shared__ __align__(16) float lds[];
  constexpr int I1 = H + 1;
  constexpr int PPT = ((H + NH_MAX_C) * I1 + NH_THREADS - 1) / NH_THREADS;   // pairs per thread at C = 64
  const int RW = (3 * H + C) | 1;                 // sub-tile row: g_pre [H] | g_pred [C] | x [H] | h [H]; odd stride
  nh_load_weights<H>(lds, W1, b1, W2, b2, C);
  const float* W1s = lds;
  const float* b1s = W1s + H * H;
  const float* W2s = b1s + H;
  float* sub = lds + H * H + H + C * H + C;       // [64][RW]
  const int P1 = H * I1, P = (H + C) * I1;
  float acc[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) acc[k] = 0.f;
  const float sc = scale ? scale[0] : 1.0f;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tiles = (N + NH_ROWS - 1) / NH_ROWS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r = tile * NH_ROWS + threadIdx.x;
    const bool live = r < N;
    float xr[H], h[H], gpre[H];
    __syncthreads();                              // the weights are loaded / the last sub-tile has been read
    if (live) {
      nh_load_row<H>(x, r, xr);
      nh_hidden<H>(xr, W1s, b1s, act, h);
#pragma unroll
      for (int k = 0; k < H; ++k) gpre[k] = 0.f;
      const float* __restrict__ gp_row = g_pred + r * C;
      for (int c = 0; c < C; ++c) {
        const float gp = scale ? sc * gp_row[c] : gp_row[c];
#pragma unroll
        for (int k = 0; k < H; ++k) gpre[k] = fmaf(gp, W2s[c * H + k], gpre[k]);
      }
#pragma unroll
      for (int k = 0; k < H; ++k) gpre[k] *= act_grad_from_output(h[k], act);
      if (g_x) {
        float4* out = reinterpret_cast<float4*>(g_x + r * H);
#pragma unroll
        for (int q = 0; q < H / 4; ++q) {
          float gx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < H; ++k)
#pragma unroll
            for (int u = 0; u < 4; ++u) gx[u] = fmaf(gpre[k], W1s[k * H + 4 * q + u], gx[u]);
          out[q] = make_float4(gx[0], gx[1], gx[2], gx[3]);
        }
      }
    }
    for (int s = 0; s < 4; ++s) {
      if (s) __syncthreads();                     // the previous sub-tile has been read
      if (wave == s && live) {                    // this wave's rows into the sub-tile
        float* rec = sub + lane * RW;
        const float* __restrict__ gp_row = g_pred + r * C;
        for (int c = 0; c < C; ++c) rec[H + c] = scale ? sc * gp_row[c] : gp_row[c];
#pragma unroll
        for (int k = 0; k < H; ++k) {
          rec[k] = gpre[k];
          rec[H + C + k] = xr[k];
          rec[2 * H + C + k] = h[k];
        }
      }
      __syncthreads();
      const int64_t left = N - (tile * NH_ROWS + s * 64);
      const int nt = left < 0 ? 0 : (left < 64 ? (int)left : 64);      // rows of this sub-tile
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int p = k * NH_THREADS + threadIdx.x;
        if (p >= P) continue;
        // the pair's two factors in a sub-tile row: gW1|gb1 = g_pre x [x | 1], gW2|gb2 = g_pred x [h | 1]
        const bool first = p < P1;
        const int q = first ? p : p - P1;
        const int o = q / I1, i = q - o * I1;
        const int fa = first ? o : H + o;
        const int fb = (first ? H + C : 2 * H + C) + i;
        float a = acc[k];
        if (i == H) {
          for (int t = 0; t < nt; ++t) a += sub[t * RW + fa];
        } else {
          for (int t = 0; t < nt; ++t) a = fmaf(sub[t * RW + fa], sub[t * RW + fb], a);
        }
        acc[k] = a;
      }
    }
  }
  float* out = partial + (size_t)blockIdx.x * P;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = k * NH_THREADS + threadIdx.x;
    if (p < P) out[p] = acc[k];
  }
}

// gradient [p] = sum over the G workgroups of partial[g][p], in workgroup order
__global__ void __launch_bounds__(NH_FOLD_THREADS) k_node_head_fold(const float* __restrict__ partial, int G, int H,
                                                                    int C, float* __restrict__ gW1,
                                                                    float* __restrict__ gb1, float* __restrict__ gW2,
                                                                    float* __restrict__ gb2, int accumulate) {
  const int I1 = H + 1, P1 = H * I1, P = (H + C) * I1;
  for (int p = threadIdx.x; p < P; p += NH_FOLD_THREADS) {
    float s = 0.f;
    int g = 0;
    for (; g + 32 <= G; g += 32) {               // 32 loads in flight, added in workgroup order
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = partial[(size_t)(g + u) * P + p];
#pragma unroll
      for (int u = 0; u < 32; ++u) s += v[u];
    }
    for (; g < G; ++g) s += partial[(size_t)g * P + p];
    const bool first = p < P1;
    const int q = first ? p : p - P1;
    const int o = q / I1, i = q - o * I1;
    float* dst = i < H ? (first ? gW1 : gW2) + (size_t)o * H + i : (first ? gb1 : gb2) + o;
    dst[0] = accumulate ? dst[0] + s : s;
  }
}

// rows are read and written as float4
inline bool nh_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline size_t nh_fwd_lds(int H, int C) { return (size_t)(H * H + H + C * H + C) * sizeof(float); }
inline size_t nh_bwd_lds(int H, int C) { return nh_fwd_lds(H, C) + (size_t)64 * ((3 * H + C) | 1) * sizeof(float); }

}  // namespace

extern "C" {

int hscn_node_head_supported(int H, int C) { return nh_supported(H, C) ? 1 : 0; }

int hscn_node_head_rows_per_workgroup(void) { return NH_ROWS; }

size_t hscn_node_head_workspace_bytes(int64_t N, int H, int C) {
  if (N < 1 || N > ((int64_t)1 << 31) || !nh_supported(H, C)) return 0;
  return (size_t)nh_bwd_wgs(N) * (size_t)nh_pairs(H, C) * sizeof(float);
}

int hscn_node_head_fwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int64_t N,
                       int H, int C, int act, float* pred, void* stream_) {
  if (N < 0 || N > ((int64_t)1 << 31) || !W1 || !b1 || !W2 || !b2 || act < HSCN_ACT_IDENTITY || act > HSCN_ACT_TANH ||
      (N > 0 && (!x || !pred)) || !nh_aligned(x))
    return HSCN_E_BADARG;
  if (!nh_supported(H, C)) return HSCN_E_UNSUPPORTED;
  if (N == 0) return 0;
  hipStream_t st = hscn_stream(stream_);
  const unsigned nb = (unsigned)nh_tiles(N);
  const size_t lds = nh_fwd_lds(H, C);
  if (H == 16)
    k_node_head_fwd<16><<<nb, NH_THREADS, lds, st>>>(x, W1, b1, W2, b2, N, C, act, pred);
  else if (H == 32)
    k_node_head_fwd<32><<<nb, NH_THREADS, lds, st>>>(x, W1, b1, W2, b2, N, C, act, pred);
  else
    k_node_head_fwd<64><<<nb, NH_THREADS, lds, st>>>(x, W1, b1, W2, b2, N, C, act, pred);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_node_head_bwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* g_pred, const float* scale, int64_t N, int H, int C, int act, float* g_x,
                       float* gW1, float* gb1, float* gW2, float* gb2, int accumulate, void* workspace,
                       size_t workspace_bytes, void* stream_) {
  if (N < 1 || N > ((int64_t)1 << 31) || !x || !W1 || !b1 || !W2 || !b2 || !g_pred || !gW1 || !gb1 || !gW2 || !gb2 ||
      !workspace || act < HSCN_ACT_IDENTITY || act > HSCN_ACT_TANH || (accumulate != 0 && accumulate != 1) ||
      !nh_aligned(x) || !nh_aligned(g_x))
    return HSCN_E_BADARG;
  if (!nh_supported(H, C)) return HSCN_E_UNSUPPORTED;
  if (workspace_bytes < hscn_node_head_workspace_bytes(N, H, C)) return HSCN_E_WORKSPACE;
  hipStream_t st = hscn_stream(stream_);
  const int G = nh_bwd_wgs(N);
  const size_t lds = nh_bwd_lds(H, C);            // at most 33 KB + 64 KB
  float* partial = static_cast<float*>(workspace);
  auto k = k_node_head_bwd<16>;
  if (H == 32) k = k_node_head_bwd<32>;
  else if (H == 64) k = k_node_head_bwd<64>;
  if (int rc = launch_with_lds(k, (unsigned)G, NH_THREADS, lds, st, x, W1, b1, W2, b2, g_pred, scale, N, C, act, g_x,
                               partial))
    return rc;
  k_node_head_fold<<<1, NH_FOLD_THREADS, 0, st>>>(partial, G, H, C, gW1, gb1, gW2, gb2, accumulate);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
