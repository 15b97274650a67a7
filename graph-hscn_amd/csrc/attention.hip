// Block-diagonal multi-head self-attention over a collated batch (the global half of a GPS layer), pad-free, plain or
// with a learned bias per (shortest-path bucket, head): Graphormer's spatial encoding.  One kernel family, templated on
// the argument struct: AttnArgs (plain) or BiasArgs (biased); everything the bias adds sits under `if constexpr (bias)`.
//
//   qkv [N, 3D] f32, the packed input projection: Q = columns [0, D), K = [D, 2D), V = [2D, 3D); head h owns columns
//   [h dh, (h + 1) dh) of each third (torch.nn.MultiheadAttention's layout), D = heads * dh, scale = dh^-1/2.
//   Node i of graph g attends to the nodes [ptr[g], ptr[g + 1]) of its own graph, itself included:
//     s_ij = scale <q_i, k_j>     p_ij = exp(s_ij - lse_i)     out_i = sum_j p_ij v_j     lse_i = log sum_j exp(s_ij)
//
// Work split: one workgroup of ONE wave takes AT_TILE = 64 consecutive rows of one (graph, head), one row per lane; the
// row's q (or k, v) and its accumulators live in registers (dh is a template parameter).  The other side of the product
// is streamed through LDS in chunks of AT_CHUNK = 32 rows, starting at the graph's first node.  Every lane reads the
// SAME LDS address at a time (row j, columns d .. d + 3 of the chunk): a broadcast, free of bank conflicts at any
// pitch, so the chunk is stored densely at pitch dh and filled with consecutive 16-byte writes.  A lane's scores of
// one chunk go through Ss[j][lane] (consecutive lanes, consecutive banks).  LDS: 2 * 32 * 64 * 4 + 32 * 64 * 4 = 24 KB
// at dh = 64.  No [B, n_max, n_max] or [B, n_max, D] tensor exists anywhere: memory is O(N D).
//
// Online softmax per chunk: the chunk's scores and their maximum first, ONE rescale of (l, acc) by exp(m - m_new), then
// the chunk's exp / accumulate.  The running maximum is the first chunk's maximum (no rescale, no -inf arithmetic).
//
// Determinism: a row is computed by one lane from its own graph's rows only, in key order and chunk order from the
// graph's first node; the grid, the graph's position in the batch and its neighbours do not enter.  No float atomics.
//
// Backward, two owner-computes passes that both recompute p_ij from lse (GINE's two CSR directions, dense):
//   k_attn_bwd_q  (one query per lane):  delta_i = sum_d g_out_id out_id  (also written to delta [N, heads]),
//                                        gQ_i = scale sum_j p_ij (<g_out_i, v_j> - delta_i) k_j
//   k_attn_bwd_kv (one key per lane):    gV_j = sum_i p_ij g_out_i,
//                                        gK_j = scale sum_i p_ij (<g_out_i, v_j> - delta_i) q_i      (i in row order)
// g_qkv [N, 3D] is written once with plain stores: the Q third by the first pass, the K and V thirds by the second.
//
// A graph with more than max_nodes nodes (the grid has ceil(max_nodes / AT_TILE) tiles per graph) raises flag bit 2
// and gets NaN in all its rows of every output; graph ranges are clamped to [0, N].
//
// What the bias adds:   s_ij = scale <q_i, k_j> + T[bucket_ij, h]
//   T [nb, heads] f32, nb <= 64.  bucket: uint8, graph g's [n_g, n_g] matrix row-major (row = query, column = key) at
//   bucket + spd_ptr[g] (csrc/spd.hip).  The logit is the plain one with the bias added to it, in the same kernel body,
//   so an all-zero T gives the bits of the unbiased operator (out, lse, g_qkv).
//
// The bucket bytes of a tile x chunk are staged into LDS by the whole wave:
//   query-owner kernels (forward, bwd_q): 64 rows x 32 keys; lanes 0..31 copy the 32 consecutive bytes of one row, lanes
//     32..63 those of the next (never one lane walking a column at stride n_g).  A row is stored at a pitch of 36 bytes
//     = 9 dwords and read back a dword (four keys) at a time: lane l's dword k sits in bank (9 l + k) % 32.
//   key-owner kernel (bwd_kv): for each of the chunk's 32 queries the 64 bytes of the tile's keys, consecutive across
//     lanes in memory and in LDS.
// Head h's column of T sits in LDS (64 floats).  LDS at dh = 64: forward 16 + 8 + 2.3 + 0.25 KB, bwd_q 16 + 2.3 +
// 0.25 KB and the bins (nb * 256 bytes of dynamic LDS, 16 KB at nb = 64, none where no table gradient is wanted),
// bwd_kv 16 + 0.25 + 2 + 0.25 KB: below the 64 KB a launch gets unasked.  The plain instantiations do not touch these
// arrays and carry none of them.
//
// The table's gradient   gT[b, h] = sum over pairs with bucket_ij = b of p_ij (<g_out_i, v_j> - delta_i)
// comes without float atomics from the query-owner pass: lane i adds its ds_ij into ITS column of bins [nb][64] in LDS,
// in key order; thread b of the tile then adds bins[b][0 .. 63] in lane order and writes one partial [tile, head, b];
// tiles without rows write zeros.  k_bias_fold adds the partials of all tiles in tile order.  Every sum has a fixed
// order: two runs give the same bits.
//
// Flag word (one for both variants): bit 2 as above, bit 3 = a graph whose bucket range [spd_ptr[g], spd_ptr[g] + n^2)
// leaves the bucket tensor; such a graph gets NaN in all its rows of every output and a NaN partial.  A bucket value
// >= nb is read as nb - 1.
#include "hscn_common.h"
#include <math.h>

namespace {

constexpr int AT_TILE = 64;      // rows per workgroup, one per lane (hscn_attention_tile)
constexpr int AT_CHUNK = 32;     // streamed rows per LDS chunk (hscn_attention_chunk)
constexpr int AT_THREADS = 64;
constexpr int AT_MIN_DH = 4, AT_MAX_DH = 64, AT_MAX_D = 512;
constexpr int AT_FLAG_OVERFLOW = 4;   // bit 2
constexpr int AB_FLAG_RANGE = 8;      // bit 3
constexpr int AB_MAX_BUCKETS = 64;
constexpr int AB_PITCH32 = 9;         // dwords per staged bucket row: 32 bytes + one dword of padding
constexpr int AB_FOLD_THREADS = 64;
constexpr int AB_FOLD_AHEAD = 32;     // partials a fold thread loads before it adds them (one dependent chain of adds)

struct AttnArgs {
  static constexpr bool bias = false;
  const float* qkv;      // [N, 3D]
  const int32_t* ptr;    // [B + 1]
  const float* out;      // bwd_q: [N, D]
  const float* lse_in;   // bwd: [N, heads]
  const float* delta_in; // bwd_kv: [N, heads]
  const float* g_out;    // bwd: [N, D]
  float* o;              // fwd: out [N, D];  bwd: g_qkv [N, 3D]
  float* o2;             // fwd: lse [N, heads];  bwd_q: delta [N, heads]
  int64_t N;
  int tiles, max_nodes, heads;
  float scale;
  int32_t* flag;
};

struct BiasArgs {
  static constexpr bool bias = true;
  const float* qkv;      // as in AttnArgs, down to o2
  const int32_t* ptr;
  const float* out;
  const float* lse_in;
  const float* delta_in;
  const float* g_out;
  float* o;              // (bwd_q: may be NULL)
  float* o2;
  const float* table;    // [nb, heads]
  const uint8_t* bucket; // [total]
  const int64_t* sptr;   // [B + 1]
  float* gt_part;        // bwd_q: [B * tiles, heads, nb] or NULL
  int64_t N, total;
  int tiles, max_nodes, heads, nb;
  float scale;
  int32_t* flag;
};

// this workgroup's graph g, its range [s, s + n) clamped to [0, N], and the first row of its tile relative to s
template <class Args>
__device__ __forceinline__ void graph_range(const Args& A, int& g, int& s, int& n, int& row0) {
  g = blockIdx.x / A.tiles;
  const int t = blockIdx.x - g * A.tiles;
  int64_t a = A.ptr[g], b = A.ptr[g + 1];
  a = a < 0 ? 0 : (a > A.N ? A.N : a);
  b = b < a ? a : (b > A.N ? A.N : b);
  s = (int)a;
  n = (int)(b - a);
  row0 = t * AT_TILE;
}

// 0, or the flag bit that refuses graph g: more nodes than max_nodes, or (biased) a bucket range outside the bucket
// tensor; bk := the graph's bucket matrix
template <class Args>
__device__ __forceinline__ int refusal(const Args& A, int g, int n, const uint8_t*& bk) {
  if (n > A.max_nodes) return AT_FLAG_OVERFLOW;
  if constexpr (Args::bias) {
    const int64_t base = A.sptr[g], nn = (int64_t)n * n;
    if (base < 0 || nn > A.total || base > A.total - nn) return AB_FLAG_RANGE;
    bk = A.bucket + base;
  }
  return 0;
}

// rows [s, s + n), columns [c0, c0 + cols) of a [*, ld] matrix := NaN (the whole wave strides over the rows)
__device__ __forceinline__ void fill_nan(float* base, int ld, int c0, int cols, int s, int n) {
  const float nan = __int_as_float(0x7fc00000);
  for (int r = threadIdx.x; r < n; r += AT_THREADS)
    for (int c = 0; c < cols; ++c) base[(size_t)(s + r) * ld + c0 + c] = nan;
}

// `cnt` rows of DH columns starting at row `r0`, column `c0` of the [*, ld] matrix -> dst [cnt][DH], 16 bytes a lane
template <int DH>
__device__ __forceinline__ void load_chunk(float* dst, const float* __restrict__ src, int ld, int r0, int c0, int cnt) {
  constexpr int Q4 = DH / 4;
  for (int idx = threadIdx.x; idx < cnt * Q4; idx += AT_THREADS) {
    const int r = idx / Q4, c = idx - r * Q4;
    *reinterpret_cast<float4*>(dst + (size_t)idx * 4) =
        *reinterpret_cast<const float4*>(src + (size_t)(r0 + r) * ld + c0 + c * 4);
  }
}

template <int DH>
__device__ __forceinline__ void load_row(float (&v)[DH], const float* __restrict__ p) {
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + d);
    v[d] = t.x; v[d + 1] = t.y; v[d + 2] = t.z; v[d + 3] = t.w;
  }
}

template <int DH>
__device__ __forceinline__ void store_row(float* p, const float (&v)[DH], float mul) {
#pragma unroll
  for (int d = 0; d < DH; d += 4)
    *reinterpret_cast<float4*>(p + d) = make_float4(v[d] * mul, v[d + 1] * mul, v[d + 2] * mul, v[d + 3] * mul);
}

// <a, row> with the row in LDS (a broadcast read), d ascending, fused
template <int DH>
__device__ __forceinline__ float dot_lds(const float (&a)[DH], const float* row) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + d);
    s = fmaf(a[d], t.x, s);
    s = fmaf(a[d + 1], t.y, s);
    s = fmaf(a[d + 2], t.z, s);
    s = fmaf(a[d + 3], t.w, s);
  }
  return s;
}

// acc += w * row
template <int DH>
__device__ __forceinline__ void axpy_lds(float (&acc)[DH], float w, const float* row) {
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + d);
    acc[d] = fmaf(w, t.x, acc[d]);
    acc[d + 1] = fmaf(w, t.y, acc[d + 1]);
    acc[d + 2] = fmaf(w, t.z, acc[d + 2]);
    acc[d + 3] = fmaf(w, t.w, acc[d + 3]);
  }
}

// head h's column of the table -> Ts [nb]
__device__ __forceinline__ void load_table(float* Ts, const BiasArgs& A, int h) {
  if ((int)threadIdx.x < A.nb) Ts[threadIdx.x] = A.table[(size_t)threadIdx.x * A.heads + h];
}

// query-owner staging: Bs[r][jj] := bucket(row0 + r, c0 + jj) for the tile's rows below n and jj < cnt
__device__ __forceinline__ void stage_rows(uint32_t* Bs32, const uint8_t* __restrict__ bk, int n, int row0, int c0,
                                           int cnt) {
  uint8_t* Bs = reinterpret_cast<uint8_t*>(Bs32);
  const int jj = threadIdx.x & (AT_CHUNK - 1), half = threadIdx.x >> 5;
  if (jj < cnt) {
#pragma unroll 8
    for (int r = half; r < AT_TILE; r += 2) {
      const int i = row0 + r;
      if (i < n) Bs[r * (AB_PITCH32 * 4) + jj] = bk[(size_t)i * n + c0 + jj];
    }
  }
}

// this lane's bucket of the chunk's key j, below nb
__device__ __forceinline__ int staged_bucket(const uint32_t* Bs32, int j, int nb) {
  const uint32_t w = Bs32[threadIdx.x * AB_PITCH32 + (j >> 2)];
  const int b = (int)((w >> ((j & 3) * 8)) & 255u);
  return b < nb ? b : nb - 1;
}

// this tile's partial of the table gradient := v (a tile without rows: 0; a refused graph's first tile: NaN)
__device__ __forceinline__ void write_partial(const BiasArgs& A, int h, float v) {
  if (A.gt_part && (int)threadIdx.x < A.nb)
    A.gt_part[((size_t)blockIdx.x * A.heads + h) * A.nb + threadIdx.x] = v;
}

template <int DH, class Args>
__global__ void __launch_bounds__(AT_THREADS) k_attn_fwd(const Args A) {
  constexpr bool bias = Args::bias;
  __shared__ __attribute__((aligned(16))) float Ks[AT_CHUNK * DH];
  __shared__ __attribute__((aligned(16))) float Vs[AT_CHUNK * DH];
  __shared__ float Ss[AT_CHUNK * AT_THREADS];
  __shared__ uint32_t Bs[AT_TILE * AB_PITCH32];            // (the bias's; the plain kernel carries neither)
  __shared__ float Ts[AB_MAX_BUCKETS];
  const int h = blockIdx.y, D = A.heads * DH, ld = 3 * D;
  int g, s, n, row0;
  graph_range(A, g, s, n, row0);
  const uint8_t* bk = nullptr;
  if (const int why = refusal(A, g, n, bk)) {              // workgroup-uniform
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, why);
      fill_nan(A.o, D, h * DH, DH, s, n);
      fill_nan(A.o2, A.heads, h, 1, s, n);
    }
    return;
  }
  if (row0 >= n) return;
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  float q[DH], acc[DH];
  float m = 0.f, l = 0.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) { q[d] = 0.f; acc[d] = 0.f; }
  if (live) load_row<DH>(q, A.qkv + (size_t)(s + i) * ld + h * DH);
  if constexpr (bias) load_table(Ts, A, h);
  for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
    const int cnt = n - c0 < AT_CHUNK ? n - c0 : AT_CHUNK;
    __syncthreads();                                       // the previous chunk has been read
    load_chunk<DH>(Ks, A.qkv, ld, s + c0, D + h * DH, cnt);
    load_chunk<DH>(Vs, A.qkv, ld, s + c0, 2 * D + h * DH, cnt);
    if constexpr (bias) stage_rows(Bs, bk, n, row0, c0, cnt);
    __syncthreads();
    if (live) {
      float cmax = 0.f;
      for (int j = 0; j < cnt; ++j) {
        float sc;
        if constexpr (bias) sc = A.scale * dot_lds<DH>(q, Ks + j * DH) + Ts[staged_bucket(Bs, j, A.nb)];
        else sc = A.scale * dot_lds<DH>(q, Ks + j * DH);
        Ss[j * AT_THREADS + threadIdx.x] = sc;
        cmax = j == 0 ? sc : fmaxf(cmax, sc);
      }
      if (c0 == 0) {
        m = cmax;                                          // the first chunk sets the maximum: nothing to rescale
      } else if (cmax > m) {
        const float alpha = expf(m - cmax);
        l *= alpha;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] *= alpha;
        m = cmax;
      }
      for (int j = 0; j < cnt; ++j) {
        const float p = expf(Ss[j * AT_THREADS + threadIdx.x] - m);
        l += p;
        axpy_lds<DH>(acc, p, Vs + j * DH);
      }
    }
  }
  if (live) {
    store_row<DH>(A.o + (size_t)(s + i) * D + h * DH, acc, 1.0f / l);
    A.o2[(size_t)(s + i) * A.heads + h] = m + logf(l);
  }
}

// bwd_q writes the Q third of g_qkv; the biased pass may be asked for the table's gradient alone (no g_qkv)
template <class Args>
__device__ __forceinline__ bool wants_q(const Args& A) {
  if constexpr (Args::bias) return A.o != nullptr;
  else return true;
}

template <int DH, class Args>
__global__ void __launch_bounds__(AT_THREADS) k_attn_bwd_q(const Args A) {
  constexpr bool bias = Args::bias;
  __shared__ __attribute__((aligned(16))) float Ks[AT_CHUNK * DH];
  __shared__ __attribute__((aligned(16))) float Vs[AT_CHUNK * DH];
  __shared__ uint32_t Bs[AT_TILE * AB_PITCH32];
  __shared__ float Ts[AB_MAX_BUCKETS];
  extern __shared__ __attribute__((aligned(16))) float bins[];     // [nb][lane], where the table's gradient is wanted
  const int h = blockIdx.y, D = A.heads * DH, ld = 3 * D;
  int g, s, n, row0;
  graph_range(A, g, s, n, row0);
  const uint8_t* bk = nullptr;
  if (const int why = refusal(A, g, n, bk)) {
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, why);
      if (wants_q(A)) fill_nan(A.o, ld, h * DH, DH, s, n);
      fill_nan(A.o2, A.heads, h, 1, s, n);
    }
    if constexpr (bias) write_partial(A, h, row0 == 0 ? __int_as_float(0x7fc00000) : 0.f);
    return;
  }
  if (row0 >= n) {
    if constexpr (bias) write_partial(A, h, 0.f);
    return;
  }
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  bool want_t = false;                                     // workgroup-uniform
  if constexpr (bias) want_t = A.gt_part != nullptr;
  float q[DH], go[DH], gq[DH];
  float lse = 0.f, delta = 0.f;
#pragma unroll
  for (int d = 0; d < DH; ++d) { q[d] = 0.f; go[d] = 0.f; gq[d] = 0.f; }
  if (live) {
    load_row<DH>(q, A.qkv + (size_t)(s + i) * ld + h * DH);
    load_row<DH>(go, A.g_out + (size_t)(s + i) * D + h * DH);
    const float* o = A.out + (size_t)(s + i) * D + h * DH;
#pragma unroll
    for (int d = 0; d < DH; ++d) delta = fmaf(go[d], o[d], delta);
    lse = A.lse_in[(size_t)(s + i) * A.heads + h];
    A.o2[(size_t)(s + i) * A.heads + h] = delta;
  }
  if constexpr (bias) {
    load_table(Ts, A, h);
    if (want_t)
      for (int b = 0; b < A.nb; ++b) bins[b * AT_THREADS + threadIdx.x] = 0.f;   // a lane's own column
  }
  for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
    const int cnt = n - c0 < AT_CHUNK ? n - c0 : AT_CHUNK;
    __syncthreads();
    load_chunk<DH>(Ks, A.qkv, ld, s + c0, D + h * DH, cnt);
    load_chunk<DH>(Vs, A.qkv, ld, s + c0, 2 * D + h * DH, cnt);
    if constexpr (bias) stage_rows(Bs, bk, n, row0, c0, cnt);
    __syncthreads();
    if (live) {
      for (int j = 0; j < cnt; ++j) {
        int b = 0;
        float p;
        if constexpr (bias) {
          b = staged_bucket(Bs, j, A.nb);
          p = expf(A.scale * dot_lds<DH>(q, Ks + j * DH) + Ts[b] - lse);
        } else {
          p = expf(A.scale * dot_lds<DH>(q, Ks + j * DH) - lse);
        }
        const float ds = p * (dot_lds<DH>(go, Vs + j * DH) - delta);
        axpy_lds<DH>(gq, ds, Ks + j * DH);
        if (want_t) bins[b * AT_THREADS + threadIdx.x] += ds;
      }
    }
  }
  if (live && wants_q(A)) store_row<DH>(A.o + (size_t)(s + i) * ld + h * DH, gq, A.scale);
  if constexpr (bias) {
    if (want_t) {
      __syncthreads();                                     // every lane's column is complete
      if ((int)threadIdx.x < A.nb) {
        float t = 0.f;
        for (int lane = 0; lane < AT_THREADS; ++lane) t += bins[threadIdx.x * AT_THREADS + lane];
        A.gt_part[((size_t)blockIdx.x * A.heads + h) * A.nb + threadIdx.x] = t;
      }
    }
  }
}

template <int DH, class Args>
__global__ void __launch_bounds__(AT_THREADS) k_attn_bwd_kv(const Args A) {
  constexpr bool bias = Args::bias;
  __shared__ __attribute__((aligned(16))) float Qs[AT_CHUNK * DH];
  __shared__ __attribute__((aligned(16))) float Gs[AT_CHUNK * DH];
  __shared__ float Ls[AT_CHUNK], Ds[AT_CHUNK];
  __shared__ uint8_t Bt[AT_CHUNK * AT_THREADS];            // [query of the chunk][lane]
  __shared__ float Ts[AB_MAX_BUCKETS];
  const int h = blockIdx.y, D = A.heads * DH, ld = 3 * D;
  int g, s, n, row0;
  graph_range(A, g, s, n, row0);
  const uint8_t* bk = nullptr;
  if (const int why = refusal(A, g, n, bk)) {
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, why);
      fill_nan(A.o, ld, D + h * DH, DH, s, n);
      fill_nan(A.o, ld, 2 * D + h * DH, DH, s, n);
    }
    return;
  }
  if (row0 >= n) return;
  const int j = row0 + threadIdx.x;
  const bool live = j < n;
  float k[DH], v[DH], gk[DH], gv[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) { k[d] = 0.f; v[d] = 0.f; gk[d] = 0.f; gv[d] = 0.f; }
  if (live) {
    load_row<DH>(k, A.qkv + (size_t)(s + j) * ld + D + h * DH);
    load_row<DH>(v, A.qkv + (size_t)(s + j) * ld + 2 * D + h * DH);
  }
  if constexpr (bias) load_table(Ts, A, h);
  for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
    const int cnt = n - c0 < AT_CHUNK ? n - c0 : AT_CHUNK;
    __syncthreads();
    load_chunk<DH>(Qs, A.qkv, ld, s + c0, h * DH, cnt);
    load_chunk<DH>(Gs, A.g_out, D, s + c0, h * DH, cnt);
    if ((int)threadIdx.x < cnt) {
      Ls[threadIdx.x] = A.lse_in[(size_t)(s + c0 + threadIdx.x) * A.heads + h];
      Ds[threadIdx.x] = A.delta_in[(size_t)(s + c0 + threadIdx.x) * A.heads + h];
    }
    if constexpr (bias) {
      if (live) {                                          // row c0 + i of the matrix, columns of this tile: consecutive lanes
#pragma unroll 8
        for (int i = 0; i < cnt; ++i) Bt[i * AT_THREADS + threadIdx.x] = bk[(size_t)(c0 + i) * n + j];
      }
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < cnt; ++i) {
        float p;
        if constexpr (bias) {
          int b = Bt[i * AT_THREADS + threadIdx.x];
          b = b < A.nb ? b : A.nb - 1;
          p = expf(A.scale * dot_lds<DH>(k, Qs + i * DH) + Ts[b] - Ls[i]);
        } else {
          p = expf(A.scale * dot_lds<DH>(k, Qs + i * DH) - Ls[i]);
        }
        axpy_lds<DH>(gv, p, Gs + i * DH);
        const float ds = p * (dot_lds<DH>(v, Gs + i * DH) - Ds[i]);
        axpy_lds<DH>(gk, ds, Qs + i * DH);
      }
    }
  }
  if (live) {
    store_row<DH>(A.o + (size_t)(s + j) * ld + D + h * DH, gk, A.scale);
    store_row<DH>(A.o + (size_t)(s + j) * ld + 2 * D + h * DH, gv, 1.0f);
  }
}

// g_table[b, h] := sum over tiles t, in tile order, of part[t, h, b]
__global__ void __launch_bounds__(AB_FOLD_THREADS) k_bias_fold(const float* __restrict__ part, float* g_table,
                                                               int64_t tiles, int heads, int nb) {
  const int idx = blockIdx.x * AB_FOLD_THREADS + threadIdx.x, hb = heads * nb;
  if (idx >= hb) return;
  float t = 0.f;
  int64_t k = 0;
  for (; k + AB_FOLD_AHEAD <= tiles; k += AB_FOLD_AHEAD) {     // the loads of a block in flight together, the adds in order
    float v[AB_FOLD_AHEAD];
#pragma unroll
    for (int u = 0; u < AB_FOLD_AHEAD; ++u) v[u] = part[(size_t)(k + u) * hb + idx];
#pragma unroll
    for (int u = 0; u < AB_FOLD_AHEAD; ++u) t += v[u];
  }
  for (; k < tiles; ++k) t += part[(size_t)k * hb + idx];
  const int h = idx / nb, b = idx - h * nb;
  g_table[(size_t)b * heads + h] = t;
}

bool attn_supported(int heads, int dh) {
  return heads >= 1 && dh >= AT_MIN_DH && dh <= AT_MAX_DH && dh % 4 == 0 && (int64_t)heads * dh <= AT_MAX_D;
}

bool bias_supported(int heads, int dh, int nb) { return attn_supported(heads, dh) && nb >= 1 && nb <= AB_MAX_BUCKETS; }

int tiles_of(int max_nodes) {
  const int t = (max_nodes + AT_TILE - 1) / AT_TILE;
  return t < 1 ? 1 : t;
}

// sizes and envelope: everything that answers without looking at a pointer
int check_common(int64_t N, int64_t B, int max_nodes, int heads, int dh) {
  if (N < 0 || B < 0 || max_nodes < 0) return HSCN_E_BADARG;
  if (N > INT32_MAX || B >= INT32_MAX) return HSCN_E_BADARG;     // ptr32 is int32
  if (!attn_supported(heads, dh)) return HSCN_E_UNSUPPORTED;
  return 0;
}

// the same for the biased entry points, which also answer for the grid here (the plain ones do in launch)
int check_common(int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh, int nb) {
  if (N < 0 || B < 0 || total < 0 || max_nodes < 0) return HSCN_E_BADARG;
  if (N > INT32_MAX || B >= INT32_MAX) return HSCN_E_BADARG;
  if (!bias_supported(heads, dh, nb)) return HSCN_E_UNSUPPORTED;
  if (B * tiles_of(max_nodes) > INT32_MAX) return HSCN_E_BADARG;
  return 0;
}

enum { AT_FWD, AT_BWD_Q, AT_BWD_KV };

template <int DH, class Args>
void launch_one(int which, dim3 grid, hipStream_t st, const Args& A) {
  size_t bins = 0;                  // bwd_q's: nb * 64 floats of dynamic LDS (16 KB at most), none without a g_table
  if constexpr (Args::bias) bins = A.gt_part ? (size_t)A.nb * AT_THREADS * sizeof(float) : 0;
  if (which == AT_FWD) k_attn_fwd<DH, Args><<<grid, AT_THREADS, 0, st>>>(A);
  else if (which == AT_BWD_Q) k_attn_bwd_q<DH, Args><<<grid, AT_THREADS, bins, st>>>(A);
  else k_attn_bwd_kv<DH, Args><<<grid, AT_THREADS, 0, st>>>(A);
}

template <class Args>
int launch(int which, Args A, int64_t B, int dh, hipStream_t st) {
  A.tiles = tiles_of(A.max_nodes);
  A.scale = 1.0f / sqrtf((float)dh);
  if (B * A.tiles > INT32_MAX) return HSCN_E_BADARG;
  const dim3 grid((unsigned)(B * A.tiles), (unsigned)A.heads);
  switch (dh) {
#define HSCN_ATTN_CASE(D_) case D_: launch_one<D_>(which, grid, st, A); break;
    HSCN_ATTN_CASE(4) HSCN_ATTN_CASE(8) HSCN_ATTN_CASE(12) HSCN_ATTN_CASE(16)
    HSCN_ATTN_CASE(20) HSCN_ATTN_CASE(24) HSCN_ATTN_CASE(28) HSCN_ATTN_CASE(32)
    HSCN_ATTN_CASE(36) HSCN_ATTN_CASE(40) HSCN_ATTN_CASE(44) HSCN_ATTN_CASE(48)
    HSCN_ATTN_CASE(52) HSCN_ATTN_CASE(56) HSCN_ATTN_CASE(60) HSCN_ATTN_CASE(64)
#undef HSCN_ATTN_CASE
    default: return HSCN_E_UNSUPPORTED;
  }
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // namespace

extern "C" {

int hscn_attention_supported(int heads, int dh) { return attn_supported(heads, dh) ? 1 : 0; }
int hscn_attention_tile(void) { return AT_TILE; }
int hscn_attention_chunk(void) { return AT_CHUNK; }

int hscn_attention_fwd(const float* qkv, const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh,
                       float* out, float* lse, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, max_nodes, heads, dh)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!qkv || !ptr32 || !out || !lse || !flag) return HSCN_E_BADARG;
  if (!aligned16(qkv) || !aligned16(out)) return HSCN_E_BADARG;
  AttnArgs A{qkv, ptr32, nullptr, nullptr, nullptr, nullptr, out, lse, N, 0, max_nodes, heads, 0.f, flag};
  return launch(AT_FWD, A, B, dh, hscn_stream(stream_));
}

int hscn_attention_bwd_q(const float* qkv, const float* out, const float* lse, const float* g_out,
                         const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh, float* g_qkv,
                         float* delta, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, max_nodes, heads, dh)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!qkv || !out || !lse || !g_out || !ptr32 || !g_qkv || !delta || !flag) return HSCN_E_BADARG;
  if (!aligned16(qkv) || !aligned16(g_out) || !aligned16(g_qkv)) return HSCN_E_BADARG;
  AttnArgs A{qkv, ptr32, out, lse, nullptr, g_out, g_qkv, delta, N, 0, max_nodes, heads, 0.f, flag};
  return launch(AT_BWD_Q, A, B, dh, hscn_stream(stream_));
}

int hscn_attention_bwd_kv(const float* qkv, const float* lse, const float* delta, const float* g_out,
                          const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh, float* g_qkv,
                          int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, max_nodes, heads, dh)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!qkv || !lse || !delta || !g_out || !ptr32 || !g_qkv || !flag) return HSCN_E_BADARG;
  if (!aligned16(qkv) || !aligned16(g_out) || !aligned16(g_qkv)) return HSCN_E_BADARG;
  AttnArgs A{qkv, ptr32, nullptr, lse, delta, g_out, g_qkv, nullptr, N, 0, max_nodes, heads, 0.f, flag};
  return launch(AT_BWD_KV, A, B, dh, hscn_stream(stream_));
}

int hscn_attention_bias_supported(int heads, int dh, int num_buckets) {
  return bias_supported(heads, dh, num_buckets) ? 1 : 0;
}

int hscn_attention_bias_fwd(const float* qkv, const float* table, const uint8_t* bucket, const int64_t* spd_ptr,
                            const int32_t* ptr32, int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh,
                            int num_buckets, float* out, float* lse, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, total, max_nodes, heads, dh, num_buckets)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!qkv || !table || !bucket || !spd_ptr || !ptr32 || !out || !lse || !flag) return HSCN_E_BADARG;
  if (!aligned16(qkv) || !aligned16(out)) return HSCN_E_BADARG;
  BiasArgs A{qkv, ptr32, nullptr, nullptr, nullptr, nullptr, out, lse, table, bucket, spd_ptr, nullptr,
             N, total, 0, max_nodes, heads, num_buckets, 0.f, flag};
  return launch(AT_FWD, A, B, dh, hscn_stream(stream_));
}

int hscn_attention_bias_bwd_q(const float* qkv, const float* out, const float* lse, const float* g_out,
                              const float* table, const uint8_t* bucket, const int64_t* spd_ptr, const int32_t* ptr32,
                              int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh, int num_buckets,
                              float* g_qkv, float* delta, float* g_table, float* workspace, int64_t workspace_floats,
                              int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, total, max_nodes, heads, dh, num_buckets)) return rc;
  if (!g_qkv && !g_table) return HSCN_E_BADARG;                  // nothing asked for
  const int64_t tiles = B * tiles_of(max_nodes);
  if (g_table) {
    if (!workspace) return HSCN_E_BADARG;
    if (workspace_floats < tiles * heads * num_buckets) return HSCN_E_WORKSPACE;
  }
  hipStream_t st = hscn_stream(stream_);
  if (N > 0 && B > 0) {
    if (!qkv || !out || !lse || !g_out || !table || !bucket || !spd_ptr || !ptr32 || !delta || !flag)
      return HSCN_E_BADARG;
    if (!aligned16(qkv) || !aligned16(g_out) || (g_qkv && !aligned16(g_qkv))) return HSCN_E_BADARG;
    BiasArgs A{qkv, ptr32, out, lse, nullptr, g_out, g_qkv, delta, table, bucket, spd_ptr,
               g_table ? workspace : nullptr, N, total, 0, max_nodes, heads, num_buckets, 0.f, flag};
    if (int rc = launch(AT_BWD_Q, A, B, dh, st)) return rc;
  }
  if (g_table) {                                                 // (no rows: no tiles ran, the fold writes zeros)
    const int hb = heads * num_buckets;
    k_bias_fold<<<hscn_blocks(hb, AB_FOLD_THREADS), AB_FOLD_THREADS, 0, st>>>(
        workspace, g_table, (N > 0 && B > 0) ? tiles : 0, heads, num_buckets);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

int hscn_attention_bias_bwd_kv(const float* qkv, const float* lse, const float* delta, const float* g_out,
                               const float* table, const uint8_t* bucket, const int64_t* spd_ptr, const int32_t* ptr32,
                               int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh, int num_buckets,
                               float* g_qkv, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, B, total, max_nodes, heads, dh, num_buckets)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!qkv || !lse || !delta || !g_out || !table || !bucket || !spd_ptr || !ptr32 || !g_qkv || !flag)
    return HSCN_E_BADARG;
  if (!aligned16(qkv) || !aligned16(g_out) || !aligned16(g_qkv)) return HSCN_E_BADARG;
  BiasArgs A{qkv, ptr32, nullptr, lse, delta, g_out, g_qkv, nullptr, table, bucket, spd_ptr, nullptr,
             N, total, 0, max_nodes, heads, num_buckets, 0.f, flag};
  return launch(AT_BWD_KV, A, B, dh, hscn_stream(stream_));
}

}  // extern "C"
