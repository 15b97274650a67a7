// Random-walk structural encoding of a collated batch as ONE launch (the host restatement is
// graph_hscn/transform/rwse.py): rw[i, k-1] = (P^k)[i, i] for k = 1 .. K with P = D^-1 A, A[r, c] = the number of
// listed edges r -> c (duplicates sum, self loops kept), D the out-degree, a row without out-edges all zero.
//
// The walk is evaluated on column vectors: q_0 = e_i, q_{t+1}[r] = (1 / deg[r]) * sum_{c in row r} q_t[c] over the
// source-keyed CSR (row r lists the targets of r), rw[i, t] = q_{t+1}[i] -- the same diagonal, (P^k)[i, i] =
// e_i^T P^k e_i, from one CSR.
//
// Work unit: (graph g, tile of RW_TILE = 16 start nodes); grid B x ceil(max_n / 16), both known on the host.  A tile
// past its graph's node count returns at once, so a launch lasts as long as one tile of its largest graph, not as long
// as that whole graph.  The tile's 16 vectors of length n live in LDS as a ping-pong pair, node-major q[node][16]: the
// 16 lanes that gather neighbour c of one row read the 16 consecutive words q[c][0 .. 15] (64 bytes, 16 banks), a
// wave covers four rows, and a row's CSR words are one broadcast load for its 16 lanes.  The pair is 2 * n * 64 bytes:
// 64 KB at n = 512, which is the default limit of a launch (no opt-in) and leaves room for two workgroups per CU.
// One workgroup barrier per step.  The graph's CSR slice is read from global memory in every step; it is a few KB and
// stays in L2 (the tiles of one graph share it).  A thread's chain per row is rowptr -> col -> LDS -> add: the col words
// of a row are fetched four at a time, then their four LDS words, and only the adds run one after the other, in CSR
// order.  Up to 1 024 threads per workgroup (one per (row, start node) while that fits, strided beyond): four columns
// in flight and 1 024 threads were 1.15x (PCQM-Contact, Peptides) to 1.65x (PascalVOC-SP) ahead of one column and 512
// threads, measured; eight columns in flight were behind four.
//
// Sums run in CSR order with plain float32 adds, then one reciprocal and one multiply.  Only non-negative terms: an
// entry whose exact value is 0 (no closed walk of that length) is exactly 0.  No float atomics: same input, same bits.
#include "hscn_common.h"

namespace {

constexpr int RW_TILE = 16;
constexpr int RW_MAX_N = 512;
constexpr int RW_MAX_K = 64;
constexpr int RW_FLAG_EDGE = 2, RW_FLAG_GRAPH = 4;
constexpr int RW_THREADS = 1024;               // 16 waves: with two or three workgroups per CU by LDS, they hide the loads
constexpr int RW_UNROLL = 4;                   // CSR words (then LDS words) in flight per thread; the adds stay in CSR order

struct RwArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* nptr;
  int64_t N;
  int max_n, K;
  float* rw;
  int32_t* flag;
};

__global__ void __launch_bounds__(RW_THREADS) k_rwse_stats(RwArgs a) {
  extern __shared__ __align__(16) float rw_q[];
  const int g = blockIdx.x, tile = blockIdx.y;
  const int t = threadIdx.x, NT = blockDim.x;
  const int64_t n0 = a.nptr[g], n1 = a.nptr[g + 1];
  if (n0 < 0 || n1 > a.N || n1 < n0 || n1 - n0 > a.max_n) {       // a graph beyond what the launch was sized for
    if (tile == 0 && t == 0) atomicOr(a.flag, RW_FLAG_GRAPH);
    const int64_t lo = n0 < 0 ? 0 : n0, hi = n1 > a.N ? a.N : n1;
    const float nanv = __uint_as_float(0x7fc00000u);
    const int64_t per = (int64_t)RW_TILE * a.K, stride = (int64_t)gridDim.y * per;
    for (int64_t base = lo * a.K + tile * per; base < hi * a.K; base += stride)      // the tiles share the rows
      for (int64_t o = base + t; o < base + per && o < hi * a.K; o += NT) a.rw[o] = nanv;
    return;
  }
  const int n = (int)(n1 - n0), i0 = tile * RW_TILE;
  if (i0 >= n) return;
  const int base = (int)n0, K = a.K, work = n * RW_TILE;
  float* src = rw_q;
  float* dst = rw_q + (size_t)a.max_n * RW_TILE;
  for (int idx = t; idx < work; idx += NT) src[idx] = (idx / RW_TILE) == i0 + (idx % RW_TILE) ? 1.f : 0.f;
  __syncthreads();
  bool bad = false;
  for (int step = 0; step < K; ++step) {
    for (int idx = t; idx < work; idx += NT) {
      const int r = idx / RW_TILE, j = idx % RW_TILE;
      const int e0 = a.rowptr[base + r], e1 = a.rowptr[base + r + 1];
      float s = 0.f;
      for (int e = e0; e < e1; e += RW_UNROLL) {
        int c[RW_UNROLL];
        float v[RW_UNROLL];
#pragma unroll
        for (int u = 0; u < RW_UNROLL; ++u) c[u] = e + u < e1 ? a.col[e + u] - base : 0;
#pragma unroll
        for (int u = 0; u < RW_UNROLL; ++u) {
          const bool in = (unsigned)c[u] < (unsigned)n;
          v[u] = in ? src[c[u] * RW_TILE + j] : 0.f;
          if (!in) bad = true;
        }
#pragma unroll
        for (int u = 0; u < RW_UNROLL; ++u)
          if (e + u < e1) s += v[u];
      }
      const float v = e1 > e0 ? (1.f / (float)(e1 - e0)) * s : 0.f;
      dst[idx] = v;
      if (r == i0 + j) a.rw[(int64_t)(base + r) * K + step] = v;
    }
    __syncthreads();
    float* sw = src; src = dst; dst = sw;
  }
  if (bad) atomicOr(a.flag, RW_FLAG_EDGE);
}

}  // namespace

extern "C" {

int hscn_rwse_supported(int max_n, int ksteps) {
  return max_n >= 1 && max_n <= RW_MAX_N && ksteps >= 1 && ksteps <= RW_MAX_K;
}

int hscn_rwse_tile(void) { return RW_TILE; }

int hscn_rwse_stats(const int32_t* rowptr, const int32_t* col, const int32_t* nptr, int64_t N, int64_t B, int max_n,
                    int ksteps, float* rw, int32_t* flag, void* stream_) {
  if (!rowptr || !col || !nptr || !rw || !flag || N < 0 || B < 0 || max_n < 0 || ksteps < 1 || B > 0x7fffffff ||
      N > 0x7fffffff)
    return HSCN_E_BADARG;
  if (B == 0 || N == 0) return 0;
  if (!hscn_rwse_supported(max_n, ksteps)) return HSCN_E_UNSUPPORTED;
  RwArgs a;
  a.rowptr = rowptr; a.col = col; a.nptr = nptr; a.N = N; a.max_n = max_n; a.K = ksteps; a.rw = rw; a.flag = flag;
  const int tiles = (max_n + RW_TILE - 1) / RW_TILE;
  int threads = (max_n * RW_TILE + 63) / 64 * 64;                  // one (row, start node) per thread up to 64 rows
  if (threads > RW_THREADS) threads = RW_THREADS;
  const size_t lds = 2 * (size_t)max_n * RW_TILE * sizeof(float);
  k_rwse_stats<<<dim3((unsigned)B, (unsigned)tiles), threads, lds, hscn_stream(stream_)>>>(a);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
