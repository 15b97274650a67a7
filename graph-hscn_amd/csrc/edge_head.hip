// The pair decoder of a link-level model and its ranking metric.
//
//   score[p] = <z[u_p], z[v_p]>                     hscn_pair_dot_fwd: one gather-dot per candidate pair
//   g_z[i]   = sum_{p: u_p = i} g_p z[v_p] + sum_{p: v_p = i} g_p z[u_p]
//                                                   hscn_pair_dot_bwd: one ordered gather-accumulate per node
//   rank of every positive pair (u, v) among the other nodes w of its graph, by the scores s(u, w)
//                                                   hscn_pair_rank (+ hscn_pair_rank_reduce: MRR, Hits@1/3/10)
//
// Mapping.  Rows of z [N, D] (D a multiple of 4, 4 <= D <= 64) move as float4.  A LANE GROUP of LG = D / 4 rounded up
// to a power of two lanes (1, 2, 4, 8 or 16) owns a pair (forward, rank) or a node (backward); lane q of the group owns
// the columns 4q .. 4q + 3, so a wave holds 64 / LG pairs.  `pd_score` is the ONE dot product of the file: the lane's
// product, three fmaf in column order, then an xor-shuffle tree over the group, widest offset first.  Its order of
// operations depends on D alone -- not on the pair, not on where the group sits in the wave -- and the metric kernel
// calls the same function, so equal embeddings give equal scores bit for bit and a tie is a property of the data.
//
// The backward walks a node's by-source list and then its by-target list (two stable CSRs over the pair list: ascending
// pair id inside a row), one fmaf per incidence and column: a fixed order, no float atomics, and g_z is written, not
// accumulated -- a node without incidences gets an exact zero row.
//
// The metric kernel takes one workgroup per graph (a loop over graphs beyond the grid) and stages the graph's rows in
// LDS at a row stride of 4 LG floats (rows of D = 12, 20, ... are padded to the lane group's width): lane l of a wave
// then reads the 16-byte slot l of the staged image, 64 consecutive slots per wave, and each of ds_read_b128's four
// 16-lane groups ({0-3, 12-15, 20-27}, ...) covers sixteen distinct slots of the 256-byte bank row -- no conflicts,
// and for D = 4, 8, 16, 32, 64 no padding at all.  The launch sizes the staged image by the batch's largest graph
// (dynamic LDS: 3.4 KB for a PCQM-Contact batch at D = 16, not the whole budget); a graph beyond it, or beyond the
// 60 KB budget, reads its rows from global memory through the same code.  Bad input (an id outside its range, a label outside {0, 1}, a NaN score, inconsistent
// segment tables) is checked on the integers before any address is formed, sets a bit of the flag word and is left out.
#include "hscn_common.h"

namespace {

constexpr int PD_THREADS = 256;
constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_LDS_BYTES = 60 * 1024;     // staged rows at most; with the tail's 3 KB the kernel stays below 64 KB
constexpr int PR_MAX_WG = 1024;

inline bool pd_supported(int D) { return D >= 4 && D <= 64 && (D & 3) == 0; }
inline int pd_lanes(int D) {
  int l = 1;
  while (4 * l < D) l <<= 1;
  return l;
}
inline bool pd_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int pr_lds_max_nodes(int D) { return PR_LDS_BYTES / (16 * pd_lanes(D)); }

// the dot product of two rows over a lane group of LG lanes: a and b are the lane's four columns (`live`: the lane has
// columns and the rows exist; a lane without contributes +0).  Every lane of the group returns the same bits.  All
// lanes of the wave must call it together.
__device__ __forceinline__ float pd_score(const float4 a, const float4 b, bool live, int LG) {
  float s = 0.f;
  if (live) {
    s = __fmul_rn(a.x, b.x);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    s = fmaf(a.w, b.w, s);
  }
  for (int o = LG >> 1; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
  return s;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(PD_THREADS) k_pair_dot_fwd(const float* __restrict__ z,
                                                             const int32_t* __restrict__ pair_index, int64_t N,
                                                             int64_t P, int D, int LG, float* __restrict__ score,
                                                             int32_t* __restrict__ flags) {
  const int per_wg = PD_THREADS / LG;
  const int64_t p = (int64_t)blockIdx.x * per_wg + threadIdx.x / LG;
  const int q = threadIdx.x & (LG - 1);
  const bool in = p < P;
  int u = 0, v = 0;
  bool ok = false;
  if (in) {
    u = pair_index[p];
    v = pair_index[P + p];
    ok = u >= 0 && u < N && v >= 0 && v < N;          // on the integers, before any address is formed
  }
  const bool live = ok && 4 * q < D;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (live) {
    const int D4 = D >> 2;
    a = reinterpret_cast<const float4*>(z)[(size_t)u * D4 + q];
    b = reinterpret_cast<const float4*>(z)[(size_t)v * D4 + q];
  }
  const float s = pd_score(a, b, live, LG);
  if (in && q == 0) {
    score[p] = ok ? s : 0.f;
    if (!ok) atomicOr(flags, HSCN_PAIR_ID_OUT_OF_RANGE);
  }
}

__global__ void __launch_bounds__(PD_THREADS) k_pair_dot_bwd(const float* __restrict__ z,
                                                             const int32_t* __restrict__ pair_index,
                                                             const float* __restrict__ g_score,
                                                             const float* __restrict__ scale,
                                                             const int32_t* __restrict__ src_rowptr,
                                                             const int32_t* __restrict__ src_perm,
                                                             const int32_t* __restrict__ dst_rowptr,
                                                             const int32_t* __restrict__ dst_perm, int64_t N, int64_t P,
                                                             int D, int LG, float* __restrict__ g_z) {
  const int per_wg = PD_THREADS / LG;
  const int64_t i = (int64_t)blockIdx.x * per_wg + threadIdx.x / LG;
  const int q = threadIdx.x & (LG - 1);
  if (i >= N || 4 * q >= D) return;
  const int D4 = D >> 2;
  const float4* __restrict__ z4 = reinterpret_cast<const float4*>(z);
  const float sc = scale ? scale[0] : 1.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int side = 0; side < 2; ++side) {              // the by-source list, then the by-target list
    const int32_t* __restrict__ rowptr = side ? dst_rowptr : src_rowptr;
    const int32_t* __restrict__ perm = side ? dst_perm : src_perm;
    const int32_t* __restrict__ other = side ? pair_index : pair_index + P;
    int64_t b = rowptr[i], e = rowptr[i + 1];
    if (b < 0) b = 0;
    if (e > P) e = P;
    for (int64_t j = b; j < e; ++j) {
      const int p = perm[j];
      if (p < 0 || p >= P) continue;
      const int o = other[p];
      if (o < 0 || o >= N) continue;
      const float g = scale ? sc * g_score[p] : g_score[p];
      const float4 r = z4[(size_t)o * D4 + q];
      acc.x = fmaf(g, r.x, acc.x);
      acc.y = fmaf(g, r.y, acc.y);
      acc.z = fmaf(g, r.z, acc.z);
      acc.w = fmaf(g, r.w, acc.w);
    }
  }
  reinterpret_cast<float4*>(g_z)[(size_t)i * D4 + q] = acc;
}

__global__ void __launch_bounds__(PR_THREADS) k_pair_rank(const float* __restrict__ z, const int32_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ pair_ptr,
                                                          const int32_t* __restrict__ pair_index,
                                                          const float* __restrict__ label,
                                                          const int32_t* __restrict__ pos_rowptr,
                                                          const int32_t* __restrict__ pos_perm, int B, int64_t N,
                                                          int64_t P, int D, int LG, int filter, int lds_rows,
                                                          int32_t* __restrict__ rank2, double* __restrict__ per_graph,
                                                          int32_t* __restrict__ flags) {
  extern __shared__ float4 rows[];                    // lds_rows * LG slots: sized by the launch from max_nodes
  __shared__ double terms[PR_THREADS];
  __shared__ int code[PR_THREADS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wl = lane / LG, q = lane & (LG - 1), per = 64 / LG;
  const int D4 = D >> 2;
  const bool liveq = 4 * q < D;
  const float4* __restrict__ z4 = reinterpret_cast<const float4*>(z);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int bits = 0;
  for (int g = blockIdx.x; g < B; g += gridDim.x) {
    const int nb = ptr[g], ne = ptr[g + 1], pb = pair_ptr[g], pe = pair_ptr[g + 1];
    double* __restrict__ out = per_graph + (size_t)g * 5;
    if (nb < 0 || ne < nb || ne > N || pb < 0 || pe < pb || pe > P) {       // (uniform over the workgroup)
      if (tid < 5) out[tid] = 0.0;
      bits |= HSCN_PAIR_BAD_SEGMENT;
      continue;
    }
    const int n = ne - nb;
    const bool in_lds = n <= lds_rows;
    __syncthreads();                                  // the previous graph's rows have been read
    if (in_lds)
      for (int idx = tid; idx < n * LG; idx += PR_THREADS) {
        const int r = idx / LG, c = idx & (LG - 1);
        rows[idx] = 4 * c < D ? z4[(size_t)(nb + r) * D4 + c] : zero4;
      }
    __syncthreads();
    // row of node `node` (inside [nb, ne)), this lane's four columns
#define PR_ROW(node) (in_lds ? rows[((node) - nb) * LG + q] : z4[(size_t)(node) * D4 + q])
    double sum = 0.0;                                 // thread 0: the graph's totals, in pair order
    int h1 = 0, h3 = 0, h10 = 0, npos = 0;
    for (int64_t c0 = pb; c0 < pe; c0 += PR_THREADS) {                      // a chunk of 256 pairs
      for (int t = wave; t < PR_THREADS && c0 + t < pe; t += PR_WAVES) {    // a wave per pair
        const int64_t p = c0 + t;
        const float lab = label[p];
        const int u = pair_index[p], v = pair_index[P + p];
        int r2 = -1;
        if (!(lab == 0.f || lab == 1.f)) {
          bits |= HSCN_PAIR_LABEL_NOT_BINARY;
        } else if (u < nb || u >= ne || v < nb || v >= ne) {
          bits |= HSCN_PAIR_ID_OUT_OF_RANGE;
        } else if (lab == 1.f) {
          const float4 zu = liveq ? PR_ROW(u) : zero4;
          const float4 zv = liveq ? PR_ROW(v) : zero4;
          const float spos = pd_score(zu, zv, liveq, LG);
          int gt = 0, eq = 0;
          for (int w0 = 0; w0 < n; w0 += per) {       // every node w of the graph
            const int w = nb + w0 + wl;
            const bool there = w < ne;
            const float4 zw = there && liveq ? PR_ROW(w) : zero4;
            const float s = pd_score(zu, zw, there && liveq, LG);
            if (there && q == 0 && w != v && (filter < 2 || w != u)) {
              gt += s > spos;
              eq += s == spos;
              if (s != s) bits |= HSCN_PAIR_NAN_SCORE;
            }
          }
          if (filter >= 1) {                          // minus the other positive partners of u
            int64_t b = pos_rowptr[u], e = pos_rowptr[u + 1];
            if (b < 0) b = 0;
            if (e > P) e = P;
            for (int64_t j0 = b; j0 < e; j0 += per) {
              const int64_t j = j0 + wl;
              int w = -1;
              if (j < e) {
                const int pp = pos_perm[j];
                if (pp >= 0 && pp < P && label[pp] == 1.f && pair_index[pp] == u) w = pair_index[P + pp];
              }
              const bool there = w >= nb && w < ne && w != v && (filter < 2 || w != u);
              const float4 zw = there && liveq ? PR_ROW(w) : zero4;
              const float s = pd_score(zu, zw, there && liveq, LG);
              if (there && q == 0) {
                gt -= s > spos;
                eq -= s == spos;
              }
            }
          }
          gt = wave_sum_int(gt);
          eq = wave_sum_int(eq);
          if (spos != spos) {
            bits |= HSCN_PAIR_NAN_SCORE;              // not ranked, not counted
          } else {
            r2 = 2 * gt + eq;
            if (r2 < 0) r2 = 0;                       // (duplicate candidates: outside the contract)
          }
        }
        if (lane == 0) {
          code[t] = r2;
          if (rank2) rank2[p] = r2;
        }
      }
      __syncthreads();
      const int64_t left = pe - c0;
      const int cnt = left < PR_THREADS ? (int)left : PR_THREADS;
      if (tid < cnt) terms[tid] = code[tid] >= 0 ? 2.0 / (double)(code[tid] + 2) : 0.0;
      __syncthreads();
      if (tid == 0)
        for (int t = 0; t < cnt; ++t) {
          const int r2 = code[t];
          if (r2 < 0) continue;
          sum += terms[t];
          npos += 1;
          h1 += r2 + 2 <= 2;
          h3 += r2 + 2 <= 6;
          h10 += r2 + 2 <= 20;
        }
      __syncthreads();                                // code / terms are free again
    }
    if (tid == 0) {
      out[0] = sum;
      out[1] = (double)h1;
      out[2] = (double)h3;
      out[3] = (double)h10;
      out[4] = (double)npos;
    }
#undef PR_ROW
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, 64);
  if (bits && lane == 0) atomicOr(flags, bits);
}

// MRR, Hits@1, Hits@3, Hits@10 from the per-graph table: thread k adds column k in graph order, starting from the
// running accumulator when there is one
__global__ void __launch_bounds__(64) k_pair_rank_reduce(const double* __restrict__ per_graph, int B, int pooled,
                                                         double* __restrict__ acc_sum, int64_t* __restrict__ acc_count,
                                                         double* __restrict__ result, int32_t* __restrict__ flags) {
  const int k = threadIdx.x;
  double s = 0.0;
  int64_t c = 0;
  if (k < 4) {
    if (acc_sum) {
      s = acc_sum[k];
      c = acc_count[0];
    }
    for (int g = 0; g < B; ++g) {
      const double np = per_graph[(size_t)g * 5 + 4];
      if (!(np > 0.0)) continue;                      // a graph without positives is left out
      const double v = per_graph[(size_t)g * 5 + k];
      if (pooled) {
        s += v;
        c += (int64_t)np;
      } else {
        s += v / np;
        c += 1;
      }
    }
  }
  __syncthreads();                                    // every thread has read the running count
  if (k < 4) {
    if (acc_sum) acc_sum[k] = s;
    if (acc_sum && k == 0) acc_count[0] = c;
    result[k] = c > 0 ? s / (double)c : 0.0;
    // the bit speaks of THIS result: a running total that has met a positive by now takes it back
    if (k == 0) {
      if (c == 0) atomicOr(flags, HSCN_PAIR_NO_POSITIVE);
      else atomicAnd(flags, ~HSCN_PAIR_NO_POSITIVE);
    }
  }
}

}  // namespace

extern "C" {

int hscn_pair_dot_supported(int D) { return pd_supported(D) ? 1 : 0; }

int hscn_pair_dot_pairs_per_workgroup(int D) { return pd_supported(D) ? PD_THREADS / pd_lanes(D) : 0; }

int hscn_pair_dot_fwd(const float* z, const int32_t* pair_index, int64_t N, int64_t P, int D, float* score,
                      int32_t* flags, void* stream_) {
  if (N < 0 || N > 0x7fffffffLL || P < 0 || P > 0x7fffffffLL || !flags || (P > 0 && (!z || !pair_index || !score)) ||
      !pd_aligned(z))
    return HSCN_E_BADARG;
  if (!pd_supported(D)) return HSCN_E_UNSUPPORTED;
  if (P == 0) return 0;
  const int LG = pd_lanes(D);
  k_pair_dot_fwd<<<hscn_blocks(P, PD_THREADS / LG), PD_THREADS, 0, hscn_stream(stream_)>>>(z, pair_index, N, P, D, LG,
                                                                                          score, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pair_dot_bwd(const float* z, const int32_t* pair_index, const float* g_score, const float* scale,
                      const int32_t* src_rowptr, const int32_t* src_perm, const int32_t* dst_rowptr,
                      const int32_t* dst_perm, int64_t N, int64_t P, int D, float* g_z, void* stream_) {
  if (N < 1 || N > 0x7fffffffLL || P < 0 || P > 0x7fffffffLL || !z || !g_z || !src_rowptr || !dst_rowptr ||
      (P > 0 && (!pair_index || !g_score || !src_perm || !dst_perm)) || !pd_aligned(z) || !pd_aligned(g_z))
    return HSCN_E_BADARG;
  if (!pd_supported(D)) return HSCN_E_UNSUPPORTED;
  const int LG = pd_lanes(D);
  k_pair_dot_bwd<<<hscn_blocks(N, PD_THREADS / LG), PD_THREADS, 0, hscn_stream(stream_)>>>(
      z, pair_index, g_score, scale, src_rowptr, src_perm, dst_rowptr, dst_perm, N, P, D, LG, g_z);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pair_rank_supported(int max_nodes, int D) {
  if (!pd_supported(D) || max_nodes < 0) return 0;
  return max_nodes <= pr_lds_max_nodes(D) ? 1 : 2;
}

int hscn_pair_rank_lds_max_nodes(int D) { return pd_supported(D) ? pr_lds_max_nodes(D) : 0; }

int hscn_pair_rank_max_workgroups(void) { return PR_MAX_WG; }

int hscn_pair_rank(const float* z, const int32_t* ptr, const int32_t* pair_ptr, const int32_t* pair_index,
                   const float* edge_label, const int32_t* pos_rowptr, const int32_t* pos_perm, int64_t B, int64_t N,
                   int64_t P, int D, int filter, int max_nodes, int32_t* rank2, double* per_graph, int32_t* flags,
                   void* stream_) {
  if (B < 0 || B > 0x7fffffffLL || N < 0 || N > 0x7fffffffLL || P < 0 || P > 0x7fffffffLL || filter < 0 ||
      filter > 2 || !flags || (B > 0 && (!ptr || !pair_ptr || !per_graph)) ||
      (P > 0 && (!z || !pair_index || !edge_label)) || (filter > 0 && P > 0 && (!pos_rowptr || !pos_perm)) || !pd_aligned(z))
    return HSCN_E_BADARG;
  if (!pd_supported(D)) return HSCN_E_UNSUPPORTED;
  if (B == 0) return 0;
  const int grid = B < PR_MAX_WG ? (int)B : PR_MAX_WG;
  const int LG = pd_lanes(D);
  // rows staged per workgroup: the batch's largest graph when the caller knows it, the whole budget otherwise; a
  // graph with more nodes than that reads its rows from global memory
  int lds_rows = pr_lds_max_nodes(D);
  if (max_nodes > 0 && max_nodes < lds_rows) lds_rows = max_nodes;
  const size_t lds = (size_t)lds_rows * LG * sizeof(float4);
  k_pair_rank<<<grid, PR_THREADS, lds, hscn_stream(stream_)>>>(z, ptr, pair_ptr, pair_index, edge_label, pos_rowptr,
                                                               pos_perm, (int)B, N, P, D, LG, filter, lds_rows, rank2,
                                                               per_graph, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pair_rank_reduce(const double* per_graph, int64_t B, int averaging, double* acc_sum, int64_t* acc_count,
                          double* result, int32_t* flags, void* stream_) {
  if (B < 0 || B > 0x7fffffffLL || (B > 0 && !per_graph) || !result || !flags ||
      (averaging != HSCN_PAIR_AVG_GRAPH && averaging != HSCN_PAIR_AVG_POOLED) || ((acc_sum == nullptr) != (acc_count == nullptr)))
    return HSCN_E_BADARG;
  k_pair_rank_reduce<<<1, 64, 0, hscn_stream(stream_)>>>(per_graph, (int)B, averaging == HSCN_PAIR_AVG_POOLED, acc_sum,
                                                         acc_count, result, flags);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
