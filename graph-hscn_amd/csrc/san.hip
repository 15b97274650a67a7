// SAN's attention (Kreuzer et al., "Rethinking Graph Transformers with Spectral Attention", 2021, as GraphGPS's
// SANLayer spells it): every node attends to its in-neighbours through one set of projections and the edge's features
// ("real" pairs) and to every other node of its graph through a second set and one learned row ("fake" pairs), the two
// kinds mixed by gamma under ONE denominator.  Per head h of width C, target i of graph g, scale = 1 / sqrt(C):
//
//   real   every edge x = (j -> i) with both ends in g, each listed edge once, in CSR order:
//            s_x   = scale sum_c q[i,c] (k[j,c] e[x,c])          w_x   = a exp(clamp(s_x, -5, 5))
//   fake   every node j of g (j = i included) for which no edge j -> i is listed, in key order:
//            s2_ij = scale sum_c q2[i,c] k2e[j,c]                w2_ij = b exp(clamp(s2_ij, -5, 5))
//   a = 1 / (1 + gamma), b = gamma / (1 + gamma)
//   Z_i = sum w_x + sum w2_ij        out_i = (sum w_x v_j + sum w2_ij v_j) / (Z_i + 1e-6)
//   full = 0: the real term alone with a = 1; a node without in-edges gets zeros.
//
// q, k, v, q2, k2e are [N, heads * C], e is [E, heads * C] in the order of the edge list.  The relation is directed:
// j -> i makes (j, i) real and leaves (i, j) fake unless that edge is listed too.
//
// Work split, the dense half as in attention.hip: one workgroup of ONE wave takes SN_TILE = 64 consecutive rows of one
// (graph, head), one row per lane, the row's operands and accumulators in registers (C is a template parameter).
//   * The tile's adjacency is a bitset in LDS, [64 rows][pitch words], pitch = ceil(max_nodes / 32) | 1: lane l walks
//     ITS CSR row and sets bits in ITS bitset row (words l * pitch + w: an odd pitch keeps the 64 lanes' reads of "their
//     word of chunk c" on distinct banks).  Bit j - s of row i = an edge j -> i is listed.
//   * The real term is the same walk: the lane gathers k[j], v[j], e[x] of each of its slots from memory.
//   * The fake term streams k2e and v through LDS in chunks of SN_CHUNK = 32 rows from the graph's first node; every
//     lane reads the SAME LDS address at a time (a broadcast).  A chunk is exactly one word of the lane's bitset row.
//   Scores are clamped to +-5 and w <= e^5, so there is no running maximum and no rescale; kept for the backward are the
//   inputs, out and ONE float per (row, head), Z.  No weight, no [n, n] and no [E, heads] tensor exists anywhere.
//   LDS at C = 64: 2 * 32 * 64 * 4 = 16 KB of chunks (+ 256 B in the key-keyed pass) and 256 * pitch bytes of bitset,
//   3.8 KB at max_nodes = 480, 16.3 KB at 2048, 32.3 KB at SN_MAX_NODES = 4096: below the 64 KB a launch gets unasked.
//
// Backward, two owner-computes passes that recompute the weights from Z with the forward's arithmetic:
//   k_san_bwd_dst (one query per lane, target-keyed CSR): delta_i = sum_c g_out[i,c] out[i,c] (stored),
//       r_i = 1 / (Z_i + 1e-6),  ds = w r_i (<g_out_i, v_j> - delta_i) [-5 < s < 5] scale,
//       dq_i = sum ds_x (k_j e_x),  de_x = ds_x (q_i k_j) (every edge has one target row: one writer),
//       dq2_i = sum ds_ij k2e_j
//   k_san_bwd_src (one key per lane, source-keyed CSR; the bitset holds the key's OUT-edges, the dense walk is over
//       chunks of queries carrying q2, g_out, Z, delta):
//       dk_j = sum ds_x (q_i e_x),  dk2e_j = sum ds_ij q2_i,  dv_j = sum w r_i g_out_i over both kinds
// Plain stores, each element written once, no float atomics: two runs give the same bits, and a row depends on the rows
// and edges of its own graph alone (not on the graph's place in the batch or on the grid).
//
// Guards.  A slot whose other end lies outside the row's graph range (ranges are clamped to [0, N]) or whose edge id
// lies outside [0, E) is left out of the real walk AND of the bitset in both directions, and raises flag bit 0; its
// row of de is not written (the caller hands in zeros).  The bitset word is range-checked before the write.  A graph
// with more than max_nodes nodes (or more than SN_MAX_NODES) raises bit 1 and gets NaN in all its rows of every
// output of the launch but de; it touches no LDS.
#include "hscn_common.h"
#include <math.h>
#include <initializer_list>

namespace {

constexpr int SN_TILE = 64;      // rows per workgroup, one per lane
constexpr int SN_CHUNK = 32;      // streamed rows per LDS chunk = bits of one bitset word
constexpr int SN_THREADS = 64;
constexpr int SN_MIN_C = 4, SN_MAX_C = 64, SN_MAX_HC = 512;
constexpr int SN_MAX_NODES = 4096;
constexpr int SN_FLAG_EDGE = 1;       // bit 0
constexpr int SN_FLAG_OVERFLOW = 2;   // bit 1
constexpr float SN_CLAMP = 5.0f;
constexpr float SN_EPS = 1e-6f;
static_assert(SN_CHUNK == 32, "a chunk is one word of a bitset row");

struct SanArgs {
  const int32_t* rowptr;   // the walked CSR: keyed by target (fwd, bwd_dst) or by source (bwd_src)
  const int32_t* col;
  const int32_t* eid;
  const int32_t* ptr;      // [B + 1]
  const float* q;          // [N, HC]
  const float* k;
  const float* v;
  const float* e;          // [E, HC]
  const float* q2;         // [N, HC], full only
  const float* k2e;
  const float* out;        // bwd_dst: [N, HC]
  const float* z_in;       // bwd: [N, heads]
  const float* delta_in;   // bwd_src: [N, heads]
  const float* go;         // bwd: [N, HC]
  float* o;                // fwd: out
  float* o2;               // fwd: z;  bwd_dst: delta
  float* g0;               // bwd_dst: dq or NULL;   bwd_src: dk or NULL
  float* g1;               // bwd_dst: de or NULL;   bwd_src: dv or NULL
  float* g2;               // bwd_dst: dq2 or NULL;  bwd_src: dk2e or NULL
  int64_t N, E;
  int tiles, max_nodes, heads, pitch, full;
  float scale, a, b;
  int32_t* flag;
};

// this workgroup's graph range [s, s + n) clamped to [0, N], and the first row of its tile relative to s
__device__ __forceinline__ void graph_range(const SanArgs& A, int& s, int& n, int& row0) {
  const int g = blockIdx.x / A.tiles;
  const int t = blockIdx.x - g * A.tiles;
  int64_t a = A.ptr[g], b = A.ptr[g + 1];
  a = a < 0 ? 0 : (a > A.N ? A.N : a);
  b = b < a ? a : (b > A.N ? A.N : b);
  s = (int)a;
  n = (int)(b - a);
  row0 = t * SN_TILE;
}

__device__ __forceinline__ bool refused(const SanArgs& A, int n) { return n > A.max_nodes || n > SN_MAX_NODES; }

// the slots [lo, hi) of row r of the walked CSR, inside [0, E]
__device__ __forceinline__ void row_slots(const SanArgs& A, int r, int& lo, int& hi) {
  const int64_t a = A.rowptr[r], b = A.rowptr[r + 1];
  lo = (int)(a < 0 ? 0 : (a > A.E ? A.E : a));
  hi = (int)(b < lo ? lo : (b > A.E ? A.E : b));
}

// slot p names node j of the row's own graph [s, s + n) and an edge of the list
__device__ __forceinline__ bool slot_ok(const SanArgs& A, int s, int n, int j, int x) {
  return j >= s && j < s + n && x >= 0 && x < A.E;
}

// rows [s, s + n), columns [c0, c0 + cols) of a [*, ld] matrix := NaN (the whole wave strides over the rows)
__device__ __forceinline__ void fill_nan(float* base, int ld, int c0, int cols, int s, int n) {
  if (!base) return;
  const float nan = __int_as_float(0x7fc00000);
  for (int r = threadIdx.x; r < n; r += SN_THREADS)
    for (int c = 0; c < cols; ++c) base[(size_t)(s + r) * ld + c0 + c] = nan;
}

// `cnt` rows of C columns starting at row `r0`, column `c0` of the [*, ld] matrix -> dst [cnt][C], 16 bytes a lane
template <int C>
__device__ __forceinline__ void load_chunk(float* dst, const float* __restrict__ src, int ld, int r0, int c0, int cnt) {
  constexpr int Q4 = C / 4;
  for (int idx = threadIdx.x; idx < cnt * Q4; idx += SN_THREADS) {
    const int r = idx / Q4, c = idx - r * Q4;
    *reinterpret_cast<float4*>(dst + (size_t)idx * 4) =
        *reinterpret_cast<const float4*>(src + (size_t)(r0 + r) * ld + c0 + c * 4);
  }
}

template <int C>
__device__ __forceinline__ void load_row(float (&v)[C], const float* __restrict__ p) {
#pragma unroll
  for (int d = 0; d < C; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + d);
    v[d] = t.x; v[d + 1] = t.y; v[d + 2] = t.z; v[d + 3] = t.w;
  }
}

template <int C>
__device__ __forceinline__ void store_row(float* p, const float (&v)[C], float mul) {
#pragma unroll
  for (int d = 0; d < C; d += 4)
    *reinterpret_cast<float4*>(p + d) = make_float4(v[d] * mul, v[d + 1] * mul, v[d + 2] * mul, v[d + 3] * mul);
}

// <a, row>, d ascending, fused; `row` in LDS (a broadcast read) or in memory (a lane's own gather)
template <int C>
__device__ __forceinline__ float dot_row(const float (&a)[C], const float* row) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < C; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + d);
    s = fmaf(a[d], t.x, s);
    s = fmaf(a[d + 1], t.y, s);
    s = fmaf(a[d + 2], t.z, s);
    s = fmaf(a[d + 3], t.w, s);
  }
  return s;
}

// acc += w * row
template <int C>
__device__ __forceinline__ void axpy_row(float (&acc)[C], float w, const float* row) {
#pragma unroll
  for (int d = 0; d < C; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + d);
    acc[d] = fmaf(w, t.x, acc[d]);
    acc[d + 1] = fmaf(w, t.y, acc[d + 1]);
    acc[d + 2] = fmaf(w, t.z, acc[d + 2]);
    acc[d + 3] = fmaf(w, t.w, acc[d + 3]);
  }
}

// The real logit sum_c q_c (k_c e_c), the product k e rounded first, c ascending.  One operand is the lane's own
// register row, the other two are gathered: the forward and bwd_dst hold q, bwd_src holds k -- the same products in the
// same order, so every pass sees the same bits.
template <int C>
__device__ __forceinline__ float real_dot_q(const float (&q)[C], const float* kp, const float* ep) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < C; d += 4) {
    const float4 kk = *reinterpret_cast<const float4*>(kp + d);
    const float4 ee = *reinterpret_cast<const float4*>(ep + d);
    s = fmaf(q[d], kk.x * ee.x, s);
    s = fmaf(q[d + 1], kk.y * ee.y, s);
    s = fmaf(q[d + 2], kk.z * ee.z, s);
    s = fmaf(q[d + 3], kk.w * ee.w, s);
  }
  return s;
}

template <int C>
__device__ __forceinline__ float real_dot_k(const float (&k)[C], const float* qp, const float* ep) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < C; d += 4) {
    const float4 qq = *reinterpret_cast<const float4*>(qp + d);
    const float4 ee = *reinterpret_cast<const float4*>(ep + d);
    s = fmaf(qq.x, k[d] * ee.x, s);
    s = fmaf(qq.y, k[d + 1] * ee.y, s);
    s = fmaf(qq.z, k[d + 2] * ee.z, s);
    s = fmaf(qq.w, k[d + 3] * ee.w, s);
  }
  return s;
}

__device__ __forceinline__ float weight_of(float s) { return expf(fminf(fmaxf(s, -SN_CLAMP), SN_CLAMP)); }
__device__ __forceinline__ float gate_of(float s) { return (s > -SN_CLAMP && s < SN_CLAMP) ? 1.f : 0.f; }

// bit (j - s) of this lane's bitset row, the word range-checked: nothing is written outside the row
__device__ __forceinline__ void set_bit(uint32_t* mine, int pitch, int jl) {
  const int w = jl >> 5;
  if (jl >= 0 && w < pitch) mine[w] |= 1u << (jl & 31);
}

template <int C>
__global__ void __launch_bounds__(SN_THREADS) k_san_fwd(const SanArgs A) {
  __shared__ __attribute__((aligned(16))) float Ks[SN_CHUNK * C];
  __shared__ __attribute__((aligned(16))) float Vs[SN_CHUNK * C];
  extern __shared__ uint32_t bits[];                       // [SN_TILE][pitch], full only
  const int h = blockIdx.y, HC = A.heads * C;
  int s, n, row0;
  graph_range(A, s, n, row0);
  if (refused(A, n)) {                                     // workgroup-uniform, before any LDS write
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, SN_FLAG_OVERFLOW);
      fill_nan(A.o, HC, h * C, C, s, n);
      fill_nan(A.o2, A.heads, h, 1, s, n);
    }
    return;
  }
  if (row0 >= n) return;
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  uint32_t* mine = bits + (size_t)threadIdx.x * A.pitch;
  if (A.full)
    for (int w = 0; w < A.pitch; ++w) mine[w] = 0u;
  float acc[C];
  float Z = 0.f;
  bool bad = false;
#pragma unroll
  for (int d = 0; d < C; ++d) acc[d] = 0.f;
  if (live) {                                              // the real pairs, in CSR order
    float q[C];
    load_row<C>(q, A.q + (size_t)(s + i) * HC + h * C);
    int lo, hi;
    row_slots(A, s + i, lo, hi);
    for (int p = lo; p < hi; ++p) {
      const int j = A.col[p], x = A.eid[p];
      if (!slot_ok(A, s, n, j, x)) { bad = true; continue; }
      if (A.full) set_bit(mine, A.pitch, j - s);
      const float sc = real_dot_q<C>(q, A.k + (size_t)j * HC + h * C, A.e + (size_t)x * HC + h * C) * A.scale;
      const float w = A.a * weight_of(sc);
      Z += w;
      axpy_row<C>(acc, w, A.v + (size_t)j * HC + h * C);
    }
  }
  if (A.full) {                                            // the fake pairs, in key order
    float q2[C];
#pragma unroll
    for (int d = 0; d < C; ++d) q2[d] = 0.f;
    if (live) load_row<C>(q2, A.q2 + (size_t)(s + i) * HC + h * C);
    for (int c0 = 0; c0 < n; c0 += SN_CHUNK) {
      const int cnt = n - c0 < SN_CHUNK ? n - c0 : SN_CHUNK;
      __syncthreads();                                     // the previous chunk has been read
      load_chunk<C>(Ks, A.k2e, HC, s + c0, h * C, cnt);
      load_chunk<C>(Vs, A.v, HC, s + c0, h * C, cnt);
      __syncthreads();
      if (live) {
        const uint32_t real = mine[c0 >> 5];
        for (int j = 0; j < cnt; ++j) {
          if ((real >> j) & 1u) continue;
          const float sc = dot_row<C>(q2, Ks + j * C) * A.scale;
          const float w = A.b * weight_of(sc);
          Z += w;
          axpy_row<C>(acc, w, Vs + j * C);
        }
      }
    }
  }
  if (bad) atomicOr(A.flag, SN_FLAG_EDGE);
  if (live) {
    store_row<C>(A.o + (size_t)(s + i) * HC + h * C, acc, 1.0f / (Z + SN_EPS));
    A.o2[(size_t)(s + i) * A.heads + h] = Z;
  }
}

template <int C>
__global__ void __launch_bounds__(SN_THREADS) k_san_bwd_dst(const SanArgs A) {
  __shared__ __attribute__((aligned(16))) float Ks[SN_CHUNK * C];
  __shared__ __attribute__((aligned(16))) float Vs[SN_CHUNK * C];
  extern __shared__ uint32_t bits[];
  const int h = blockIdx.y, HC = A.heads * C;
  int s, n, row0;
  graph_range(A, s, n, row0);
  if (refused(A, n)) {
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, SN_FLAG_OVERFLOW);
      fill_nan(A.o2, A.heads, h, 1, s, n);
      fill_nan(A.g0, HC, h * C, C, s, n);
      fill_nan(A.g2, HC, h * C, C, s, n);
    }
    return;
  }
  if (row0 >= n) return;
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  const bool want_real = A.g0 || A.g1, want_fake = A.full && A.g2;   // workgroup-uniform
  uint32_t* mine = bits + (size_t)threadIdx.x * A.pitch;
  if (want_fake)
    for (int w = 0; w < A.pitch; ++w) mine[w] = 0u;
  float go[C];
  float delta = 0.f, r = 0.f;
  bool bad = false;
#pragma unroll
  for (int d = 0; d < C; ++d) go[d] = 0.f;
  if (live) {
    load_row<C>(go, A.go + (size_t)(s + i) * HC + h * C);
    delta = dot_row<C>(go, A.out + (size_t)(s + i) * HC + h * C);
    r = 1.0f / (A.z_in[(size_t)(s + i) * A.heads + h] + SN_EPS);
    A.o2[(size_t)(s + i) * A.heads + h] = delta;
  }
  if (live && (want_real || want_fake)) {
    float q[C], gq[C];
#pragma unroll
    for (int d = 0; d < C; ++d) gq[d] = 0.f;
    load_row<C>(q, A.q + (size_t)(s + i) * HC + h * C);
    int lo, hi;
    row_slots(A, s + i, lo, hi);
    for (int p = lo; p < hi; ++p) {
      const int j = A.col[p], x = A.eid[p];
      if (!slot_ok(A, s, n, j, x)) { bad = true; continue; }
      if (want_fake) set_bit(mine, A.pitch, j - s);
      if (!want_real) continue;
      const float* kp = A.k + (size_t)j * HC + h * C;
      const float* ep = A.e + (size_t)x * HC + h * C;
      const float sc = real_dot_q<C>(q, kp, ep) * A.scale;
      const float w = A.a * weight_of(sc);
      const float ds = w * r * (dot_row<C>(go, A.v + (size_t)j * HC + h * C) - delta) * gate_of(sc) * A.scale;
      float* dep = A.g1 ? A.g1 + (size_t)x * HC + h * C : nullptr;
#pragma unroll
      for (int d = 0; d < C; d += 4) {
        const float4 kk = *reinterpret_cast<const float4*>(kp + d);
        const float4 ee = *reinterpret_cast<const float4*>(ep + d);
        gq[d] = fmaf(ds, kk.x * ee.x, gq[d]);
        gq[d + 1] = fmaf(ds, kk.y * ee.y, gq[d + 1]);
        gq[d + 2] = fmaf(ds, kk.z * ee.z, gq[d + 2]);
        gq[d + 3] = fmaf(ds, kk.w * ee.w, gq[d + 3]);
        if (dep)                                           // this slot is the edge's one writer
          *reinterpret_cast<float4*>(dep + d) = make_float4(ds * (q[d] * kk.x), ds * (q[d + 1] * kk.y),
                                                            ds * (q[d + 2] * kk.z), ds * (q[d + 3] * kk.w));
      }
    }
    if (A.g0) store_row<C>(A.g0 + (size_t)(s + i) * HC + h * C, gq, 1.0f);
  }
  if (want_fake) {
    float q2[C], gq2[C];
#pragma unroll
    for (int d = 0; d < C; ++d) { q2[d] = 0.f; gq2[d] = 0.f; }
    if (live) load_row<C>(q2, A.q2 + (size_t)(s + i) * HC + h * C);
    for (int c0 = 0; c0 < n; c0 += SN_CHUNK) {
      const int cnt = n - c0 < SN_CHUNK ? n - c0 : SN_CHUNK;
      __syncthreads();
      load_chunk<C>(Ks, A.k2e, HC, s + c0, h * C, cnt);
      load_chunk<C>(Vs, A.v, HC, s + c0, h * C, cnt);
      __syncthreads();
      if (live) {
        const uint32_t real = mine[c0 >> 5];
        for (int j = 0; j < cnt; ++j) {
          if ((real >> j) & 1u) continue;
          const float sc = dot_row<C>(q2, Ks + j * C) * A.scale;
          const float w = A.b * weight_of(sc);
          const float ds = w * r * (dot_row<C>(go, Vs + j * C) - delta) * gate_of(sc) * A.scale;
          axpy_row<C>(gq2, ds, Ks + j * C);
        }
      }
    }
    if (live) store_row<C>(A.g2 + (size_t)(s + i) * HC + h * C, gq2, 1.0f);
  }
  if (bad) atomicOr(A.flag, SN_FLAG_EDGE);
}

template <int C>
__global__ void __launch_bounds__(SN_THREADS) k_san_bwd_src(const SanArgs A) {
  __shared__ __attribute__((aligned(16))) float Qs[SN_CHUNK * C];
  __shared__ __attribute__((aligned(16))) float Gs[SN_CHUNK * C];
  __shared__ float Rs[SN_CHUNK], Ds[SN_CHUNK];
  extern __shared__ uint32_t bits[];
  const int h = blockIdx.y, HC = A.heads * C;
  int s, n, row0;
  graph_range(A, s, n, row0);
  if (refused(A, n)) {
    if (row0 == 0) {
      if (threadIdx.x == 0) atomicOr(A.flag, SN_FLAG_OVERFLOW);
      fill_nan(A.g0, HC, h * C, C, s, n);
      fill_nan(A.g1, HC, h * C, C, s, n);
      fill_nan(A.g2, HC, h * C, C, s, n);
    }
    return;
  }
  if (row0 >= n) return;
  const int j = row0 + threadIdx.x;
  const bool live = j < n;
  const bool want_real = A.g0 || A.g1, want_fake = A.full && (A.g1 || A.g2);   // workgroup-uniform
  uint32_t* mine = bits + (size_t)threadIdx.x * A.pitch;
  if (want_fake)
    for (int w = 0; w < A.pitch; ++w) mine[w] = 0u;
  float v[C], gv[C];
  bool bad = false;
#pragma unroll
  for (int d = 0; d < C; ++d) { v[d] = 0.f; gv[d] = 0.f; }
  if (live) load_row<C>(v, A.v + (size_t)(s + j) * HC + h * C);
  if (live && (want_real || want_fake)) {                  // the key's out-edges, in the source-keyed CSR's order
    float k[C], gk[C];
#pragma unroll
    for (int d = 0; d < C; ++d) gk[d] = 0.f;
    load_row<C>(k, A.k + (size_t)(s + j) * HC + h * C);
    int lo, hi;
    row_slots(A, s + j, lo, hi);
    for (int p = lo; p < hi; ++p) {
      const int i = A.col[p], x = A.eid[p];
      if (!slot_ok(A, s, n, i, x)) { bad = true; continue; }
      if (want_fake) set_bit(mine, A.pitch, i - s);
      if (!want_real) continue;
      const float* qp = A.q + (size_t)i * HC + h * C;
      const float* ep = A.e + (size_t)x * HC + h * C;
      const float* gp = A.go + (size_t)i * HC + h * C;
      const float sc = real_dot_k<C>(k, qp, ep) * A.scale;
      const float wr = A.a * weight_of(sc) * (1.0f / (A.z_in[(size_t)i * A.heads + h] + SN_EPS));
      const float ds = wr * (dot_row<C>(v, gp) - A.delta_in[(size_t)i * A.heads + h]) * gate_of(sc) * A.scale;
#pragma unroll
      for (int d = 0; d < C; d += 4) {
        const float4 qq = *reinterpret_cast<const float4*>(qp + d);
        const float4 ee = *reinterpret_cast<const float4*>(ep + d);
        const float4 gg = *reinterpret_cast<const float4*>(gp + d);
        gk[d] = fmaf(ds, qq.x * ee.x, gk[d]);
        gk[d + 1] = fmaf(ds, qq.y * ee.y, gk[d + 1]);
        gk[d + 2] = fmaf(ds, qq.z * ee.z, gk[d + 2]);
        gk[d + 3] = fmaf(ds, qq.w * ee.w, gk[d + 3]);
        gv[d] = fmaf(wr, gg.x, gv[d]);
        gv[d + 1] = fmaf(wr, gg.y, gv[d + 1]);
        gv[d + 2] = fmaf(wr, gg.z, gv[d + 2]);
        gv[d + 3] = fmaf(wr, gg.w, gv[d + 3]);
      }
    }
    if (A.g0) store_row<C>(A.g0 + (size_t)(s + j) * HC + h * C, gk, 1.0f);
  }
  if (want_fake) {                                         // the queries the key has no edge to, in row order
    float k2[C], gk2[C];
#pragma unroll
    for (int d = 0; d < C; ++d) { k2[d] = 0.f; gk2[d] = 0.f; }
    if (live) load_row<C>(k2, A.k2e + (size_t)(s + j) * HC + h * C);
    for (int c0 = 0; c0 < n; c0 += SN_CHUNK) {
      const int cnt = n - c0 < SN_CHUNK ? n - c0 : SN_CHUNK;
      __syncthreads();
      load_chunk<C>(Qs, A.q2, HC, s + c0, h * C, cnt);
      load_chunk<C>(Gs, A.go, HC, s + c0, h * C, cnt);
      if ((int)threadIdx.x < cnt) {
        Rs[threadIdx.x] = 1.0f / (A.z_in[(size_t)(s + c0 + threadIdx.x) * A.heads + h] + SN_EPS);
        Ds[threadIdx.x] = A.delta_in[(size_t)(s + c0 + threadIdx.x) * A.heads + h];
      }
      __syncthreads();
      if (live) {
        const uint32_t real = mine[c0 >> 5];
        for (int i = 0; i < cnt; ++i) {
          if ((real >> i) & 1u) continue;
          const float sc = dot_row<C>(k2, Qs + i * C) * A.scale;
          const float wr = A.b * weight_of(sc) * Rs[i];
          const float ds = wr * (dot_row<C>(v, Gs + i * C) - Ds[i]) * gate_of(sc) * A.scale;
          axpy_row<C>(gv, wr, Gs + i * C);
          axpy_row<C>(gk2, ds, Qs + i * C);
        }
      }
    }
    if (live && A.g2) store_row<C>(A.g2 + (size_t)(s + j) * HC + h * C, gk2, 1.0f);
  }
  if (bad) atomicOr(A.flag, SN_FLAG_EDGE);
  if (live && A.g1) store_row<C>(A.g1 + (size_t)(s + j) * HC + h * C, gv, 1.0f);
}

bool san_supported(int heads, int C, int max_nodes) {
  return heads >= 1 && C >= SN_MIN_C && C <= SN_MAX_C && C % 4 == 0 && (int64_t)heads * C <= SN_MAX_HC &&
         max_nodes >= 0 && max_nodes <= SN_MAX_NODES;
}

int tiles_of(int max_nodes) {
  const int t = (max_nodes + SN_TILE - 1) / SN_TILE;
  return t < 1 ? 1 : t;
}

int pitch_of(int max_nodes) { return ((max_nodes + 31) / 32) | 1; }     // odd: lane l's word c sits in bank (l pitch + c) % 64

// sizes and envelope: everything that answers without looking at a pointer
int check_common(int64_t N, int64_t E, int64_t B, int max_nodes, int heads, int C, double gamma, int full) {
  if (N < 0 || E < 0 || B < 0 || max_nodes < 0) return HSCN_E_BADARG;
  if (N > INT32_MAX || E > INT32_MAX || B >= INT32_MAX) return HSCN_E_BADARG;
  if (full && !(gamma >= 0.0 && gamma <= 3.0e38)) return HSCN_E_BADARG;      // negative, NaN or infinite
  if (!san_supported(heads, C, max_nodes)) return HSCN_E_UNSUPPORTED;
  if (B * tiles_of(max_nodes) > INT32_MAX) return HSCN_E_BADARG;
  return 0;
}

void set_shape(SanArgs& A, int64_t N, int64_t E, int max_nodes, int heads, int C, double gamma, int full) {
  A.N = N, A.E = E;
  A.tiles = tiles_of(max_nodes), A.max_nodes = max_nodes, A.heads = heads, A.pitch = pitch_of(max_nodes);
  A.full = full ? 1 : 0;
  A.scale = 1.0f / sqrtf((float)C);
  A.a = full ? (float)(1.0 / (1.0 + gamma)) : 1.0f;
  A.b = full ? (float)(gamma / (1.0 + gamma)) : 0.0f;
}

enum { SN_FWD, SN_BWD_DST, SN_BWD_SRC };

template <int C>
void launch_one(int which, dim3 grid, size_t lds, hipStream_t st, const SanArgs& A) {
  if (which == SN_FWD) k_san_fwd<C><<<grid, SN_THREADS, lds, st>>>(A);
  else if (which == SN_BWD_DST) k_san_bwd_dst<C><<<grid, SN_THREADS, lds, st>>>(A);
  else k_san_bwd_src<C><<<grid, SN_THREADS, lds, st>>>(A);
}

int launch(int which, const SanArgs& A, int64_t B, int C, hipStream_t st) {
  const dim3 grid((unsigned)(B * A.tiles), (unsigned)A.heads);
  // 256 * pitch bytes, 32.3 KB at SN_MAX_NODES, beside at most 16.25 KB of static chunks: no opt-in
  const size_t lds = A.full ? (size_t)SN_TILE * A.pitch * sizeof(uint32_t) : 0;
  switch (C) {
#define HSCN_SAN_CASE(C_) case C_: launch_one<C_>(which, grid, lds, st, A); break;
    HSCN_SAN_CASE(4) HSCN_SAN_CASE(8) HSCN_SAN_CASE(12) HSCN_SAN_CASE(16)
    HSCN_SAN_CASE(20) HSCN_SAN_CASE(24) HSCN_SAN_CASE(28) HSCN_SAN_CASE(32)
    HSCN_SAN_CASE(36) HSCN_SAN_CASE(40) HSCN_SAN_CASE(44) HSCN_SAN_CASE(48)
    HSCN_SAN_CASE(52) HSCN_SAN_CASE(56) HSCN_SAN_CASE(60) HSCN_SAN_CASE(64)
#undef HSCN_SAN_CASE
    default: return HSCN_E_UNSUPPORTED;
  }
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

bool all_aligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (p && !aligned16(p)) return false;
  return true;
}

}  // namespace

extern "C" {

int hscn_san_attn_supported(int heads, int head_dim, int max_nodes) {
  return san_supported(heads, head_dim, max_nodes) ? 1 : 0;
}

int hscn_san_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* ptr32,
                      const float* q, const float* k, const float* v, const float* e, const float* q2,
                      const float* k2e, float* out, float* z, int64_t N, int64_t E, int64_t B, int max_nodes,
                      int heads, int head_dim, double gamma, int full_graph, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, B, max_nodes, heads, head_dim, gamma, full_graph)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!rowptr || !ptr32 || !q || !k || !v || !out || !z || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !e)) return HSCN_E_BADARG;
  if (full_graph && (!q2 || !k2e)) return HSCN_E_BADARG;
  if (!all_aligned({q, k, v, e, q2, k2e, out})) return HSCN_E_BADARG;
  SanArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.ptr = ptr32;
  A.q = q, A.k = k, A.v = v, A.e = e, A.q2 = q2, A.k2e = k2e;
  A.o = out, A.o2 = z, A.flag = flag;
  set_shape(A, N, E, max_nodes, heads, head_dim, gamma, full_graph);
  return launch(SN_FWD, A, B, head_dim, hscn_stream(stream_));
}

int hscn_san_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* ptr32,
                          const float* q, const float* k, const float* v, const float* e, const float* q2,
                          const float* k2e, const float* out, const float* z, const float* g_out, float* delta,
                          float* dq, float* de, float* dq2, int64_t N, int64_t E, int64_t B, int max_nodes, int heads,
                          int head_dim, double gamma, int full_graph, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, B, max_nodes, heads, head_dim, gamma, full_graph)) return rc;
  if (N == 0 || B == 0) return 0;
  if (!rowptr || !ptr32 || !q || !k || !v || !out || !z || !g_out || !delta || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !e)) return HSCN_E_BADARG;
  if (full_graph && (!q2 || !k2e)) return HSCN_E_BADARG;
  if (!full_graph && dq2) return HSCN_E_BADARG;
  if (!all_aligned({q, k, v, e, q2, k2e, out, g_out, dq, de, dq2})) return HSCN_E_BADARG;
  SanArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.ptr = ptr32;
  A.q = q, A.k = k, A.v = v, A.e = e, A.q2 = q2, A.k2e = k2e;
  A.out = out, A.z_in = z, A.go = g_out;
  A.o2 = delta, A.g0 = dq, A.g1 = E > 0 ? de : nullptr, A.g2 = dq2, A.flag = flag;
  set_shape(A, N, E, max_nodes, heads, head_dim, gamma, full_graph);
  return launch(SN_BWD_DST, A, B, head_dim, hscn_stream(stream_));
}

int hscn_san_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const int32_t* ptr32,
                          const float* q, const float* k, const float* v, const float* e, const float* q2,
                          const float* k2e, const float* z, const float* delta, const float* g_out, float* dk,
                          float* dv, float* dk2e, int64_t N, int64_t E, int64_t B, int max_nodes, int heads,
                          int head_dim, double gamma, int full_graph, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, B, max_nodes, heads, head_dim, gamma, full_graph)) return rc;
  if (N == 0 || B == 0 || (!dk && !dv && !dk2e)) return 0;
  if (!rowptr_t || !ptr32 || !q || !k || !v || !z || !delta || !g_out || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t || !e)) return HSCN_E_BADARG;
  if (full_graph && (!q2 || !k2e)) return HSCN_E_BADARG;
  if (!full_graph && dk2e) return HSCN_E_BADARG;
  if (!all_aligned({q, k, v, e, q2, k2e, g_out, dk, dv, dk2e})) return HSCN_E_BADARG;
  SanArgs A{};
  A.rowptr = rowptr_t, A.col = col_t, A.eid = eid_t, A.ptr = ptr32;
  A.q = q, A.k = k, A.v = v, A.e = e, A.q2 = q2, A.k2e = k2e;
  A.z_in = z, A.delta_in = delta, A.go = g_out;
  A.g0 = dk, A.g1 = dv, A.g2 = dk2e, A.flag = flag;
  set_shape(A, N, E, max_nodes, heads, head_dim, gamma, full_graph);
  return launch(SN_BWD_SRC, A, B, head_dim, hscn_stream(stream_));
}

}  // extern "C"
