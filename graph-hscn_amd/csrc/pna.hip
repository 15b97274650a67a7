// PNAConv's aggregate (PyG PNAConv, towers = 1, one pre and one post Linear): several reductions of a node's in-edge
// messages side by side, each multiplied by degree scalers.
//
//   m_k = a[dst_k] + b[src_k] + t_k                       the message is linear in its three parts (t may be absent)
//   mean, min, max, sum over {k: dst_k = i};  std = sqrt(relu(mean(m^2) - mean(m)^2) + 1e-5)
//   out[i, (s A + x) F + f] = scaler_s(deg_i) * aggregator_x(i, f)          scaler-major, then aggregator-major, then F
//   scalers with d = max(deg_i, 1):  identity 1,  amplification log(d + 1) / avg_deg_log,  attenuation the inverse
//
// a_i is constant within a row, so the walk reduces r_k = b[src_k] + t_k alone and the row's finish adds a_i to mean,
// min and max and deg_i a_i to sum; the variance is that of r (a shift leaves it unchanged).  A node without in-edges
// gets 0 for mean, min, max and sum and sqrt(1e-5) for std.  The [E, F] message matrix is never written.
//
// Forward (k_pna_fwd): ONE launch over the target-keyed CSR with the conventions of csrc/row_walk.h as k_gine_walk
// spells them.  Per (node, column) a lane keeps the sum, the sum of squares, the min, the max and the edge ids of the
// argmin and the argmax.  Ties go to the FIRST slot in CSR order (strict comparisons while walking in slot order);
// across the chunks of a long row the earlier chunk wins (strict comparisons while merging in chunk order).  The sums
// of chunk partials are added in chunk order with a separately rounded add.
//
// Backward, no float atomics, the same bits on every run:
//   k_pna_fold      elementwise: the scalers folded into the cotangent, per (node, column) the four weights
//                   gw = {G_mean / deg + G_sum, G_min, G_max, [var > 0] G_std / (deg std)} and
//                   g_a = G_mean + G_min + G_max + deg G_sum  (the std part sums to zero over a row)
//   dm_k = gw0[i] + [k = argmin_i] gw1[i] + [k = argmax_i] gw2[i] + gw3[i] (r_k - mean_i)            i = dst_k
//   k_pna_src_walk  g_b[j] = sum of dm_k over j's out-edges: an owner-computes walk of the source-keyed CSR that
//                   recomputes r_k = b_j + t_k; long rows as in the forward
//   k_pna_edge_grad g_t[k] = dm_k, edge-parallel, plain stores
// dm_k is one device function (edge_grad) for both, so g_t[k] and the term of g_b are the same bits.
#include "row_walk.h"

namespace {

constexpr int PN_THREADS = 256;
constexpr int PNA_MAX_F = 512;
constexpr int PNA_AGGR = 5;      // mean, min, max, sum, std: the codes below
constexpr int PNA_SCAL = 3;      // identity, amplification, attenuation
enum { AG_MEAN = 0, AG_MIN = 1, AG_MAX = 2, AG_SUM = 3, AG_STD = 4 };
enum { SC_IDENTITY = 0, SC_AMPLIFICATION = 1, SC_ATTENUATION = 2 };
constexpr float PNA_STD_EPS = 1e-5f;

struct PnaSpec {
  int aggr[PNA_AGGR];
  int scal[PNA_SCAL];
  int A, S;
  float avg_deg_log;
};

__device__ __forceinline__ float scaler_of(int code, int deg, float avg_deg_log) {
  if (code == SC_IDENTITY) return 1.f;
  const float l = logf((float)((deg > 1 ? deg : 1) + 1));
  return code == SC_AMPLIFICATION ? l / avg_deg_log : avg_deg_log / l;
}

struct PnaFwdArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const float* a;      // [N, F]
  const float* b;      // [N, F]
  const float* t;      // [E, F] or NULL
  float* out;          // [N, S A F]
  float* mean;         // [N, F] mean of r over the row, or NULL
  float* stdv;         // [N, F] std where var > 0, else 0 (no gradient through the relu), or NULL
  int32_t* arg;        // [N, 2 F] edge ids of argmin | argmax, -1 for an empty row, or NULL
  int64_t N, E;
  int F, LPR, RPB;
  PnaSpec spec;
  int32_t* flag;
};

// what a lane keeps of one (row, VEC columns)
template <int VEC>
struct PnaAcc {
  float s[VEC], q[VEC], mn[VEC], mx[VEC];
  int amn[VEC], amx[VEC];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      s[v] = 0.f;
      q[v] = 0.f;
      mn[v] = INFINITY;
      mx[v] = -INFINITY;
      amn[v] = -1;
      amx[v] = -1;
    }
  }
  // a later partial (the next chunk of the row) joins: the earlier one keeps its ties
  __device__ __forceinline__ void merge(const PnaAcc& p) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      s[v] = add_rn(s[v], p.s[v]);
      q[v] = add_rn(q[v], p.q[v]);
      if (p.mn[v] < mn[v]) { mn[v] = p.mn[v]; amn[v] = p.amn[v]; }
      if (p.mx[v] > mx[v]) { mx[v] = p.mx[v]; amx[v] = p.amx[v]; }
    }
  }
};

// slots [s, t) of one row, columns [f, f + VEC), in slot order, continued in `acc`
template <int VEC>
__device__ __forceinline__ void walk_slots(const PnaFwdArgs& A, int s, int t, int f, PnaAcc<VEC>& acc) {
  using V = GV<VEC>;
#pragma unroll 2
  for (int p = s; p < t; ++p) {
    const int j = A.col[p];
    const int k = A.eid[p];
    if (j < 0 || j >= A.N || k < 0 || k >= A.E) {       // never produced by hscn_csr_build; a foreign CSR is flagged
      atomicOr(A.flag, 2);
      continue;
    }
    const typename V::T bj = V::load(A.b + (size_t)j * A.F + f);
    typename V::T tk = V::zero();
    if (A.t) tk = V::load(A.t + (size_t)k * A.F + f);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float r = A.t ? add_rn(V::get(bj, v), V::get(tk, v)) : V::get(bj, v);
      acc.s[v] = add_rn(acc.s[v], r);
      acc.q[v] = add_rn(acc.q[v], mul_rn(r, r));
      if (r < acc.mn[v]) { acc.mn[v] = r; acc.amn[v] = k; }
      if (r > acc.mx[v]) { acc.mx[v] = r; acc.amx[v] = k; }
    }
  }
}

template <int VEC>
__device__ __forceinline__ void finish_row(const PnaFwdArgs& A, int64_t r, int f, int deg, const PnaAcc<VEC>& acc) {
  using V = GV<VEC>;
  const typename V::T ar = V::load(A.a + (size_t)r * A.F + f);
  float val[PNA_AGGR][VEC], mean[VEC], sd[VEC];
  int amn[VEC], amx[VEC];
  const float fd = (float)deg;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const float av = V::get(ar, v);
    if (deg > 0) {
      const float m = acc.s[v] / fd;
      const float var = add_rn(acc.q[v] / fd, -mul_rn(m, m));
      const float sdv = sqrtf(add_rn(var > 0.f ? var : 0.f, PNA_STD_EPS));
      val[AG_MEAN][v] = add_rn(av, m);
      val[AG_MIN][v] = add_rn(av, acc.mn[v]);
      val[AG_MAX][v] = add_rn(av, acc.mx[v]);
      val[AG_SUM][v] = add_rn(mul_rn(fd, av), acc.s[v]);
      val[AG_STD][v] = sdv;
      mean[v] = m;
      sd[v] = var > 0.f ? sdv : 0.f;
      amn[v] = acc.amn[v];
      amx[v] = acc.amx[v];
    } else {
      val[AG_MEAN][v] = val[AG_MIN][v] = val[AG_MAX][v] = val[AG_SUM][v] = 0.f;
      val[AG_STD][v] = sqrtf(PNA_STD_EPS);
      mean[v] = 0.f;
      sd[v] = 0.f;
      amn[v] = amx[v] = -1;
    }
  }
  float* orow = A.out + (size_t)r * A.spec.S * A.spec.A * A.F + f;
  for (int s = 0; s < A.spec.S; ++s) {
    const float sc = scaler_of(A.spec.scal[s], deg, A.spec.avg_deg_log);
    for (int x = 0; x < A.spec.A; ++x) {
      const int code = A.spec.aggr[x];
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        // (a select chain over the five rows instead of a runtime index: the values stay in registers)
        const float w = code == AG_MEAN ? val[AG_MEAN][v]
                        : code == AG_MIN ? val[AG_MIN][v]
                        : code == AG_MAX ? val[AG_MAX][v]
                        : code == AG_SUM ? val[AG_SUM][v] : val[AG_STD][v];
        o[v] = mul_rn(sc, w);
      }
      V::store(orow + (size_t)(s * A.spec.A + x) * A.F, V::make(o));
    }
  }
  if (A.mean) V::store(A.mean + (size_t)r * A.F + f, V::make(mean));
  if (A.stdv) V::store(A.stdv + (size_t)r * A.F + f, V::make(sd));
  if (A.arg) {
    int32_t* ap = A.arg + (size_t)r * 2 * A.F + f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      ap[v] = amn[v];
      ap[A.F + v] = amx[v];
    }
  }
}

// LDS image of the chunk partials: six fields of PN_THREADS * VEC words, field-major
template <int VEC>
__device__ __forceinline__ void park(float* part, int slot, const PnaAcc<VEC>& acc) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    part[(0 * PN_THREADS + slot) * VEC + v] = acc.s[v];
    part[(1 * PN_THREADS + slot) * VEC + v] = acc.q[v];
    part[(2 * PN_THREADS + slot) * VEC + v] = acc.mn[v];
    part[(3 * PN_THREADS + slot) * VEC + v] = acc.mx[v];
    part[(4 * PN_THREADS + slot) * VEC + v] = __int_as_float(acc.amn[v]);
    part[(5 * PN_THREADS + slot) * VEC + v] = __int_as_float(acc.amx[v]);
  }
}
template <int VEC>
__device__ __forceinline__ void unpark(const float* part, int slot, PnaAcc<VEC>& acc) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    acc.s[v] = part[(0 * PN_THREADS + slot) * VEC + v];
    acc.q[v] = part[(1 * PN_THREADS + slot) * VEC + v];
    acc.mn[v] = part[(2 * PN_THREADS + slot) * VEC + v];
    acc.mx[v] = part[(3 * PN_THREADS + slot) * VEC + v];
    acc.amn[v] = __float_as_int(part[(4 * PN_THREADS + slot) * VEC + v]);
    acc.amx[v] = __float_as_int(part[(5 * PN_THREADS + slot) * VEC + v]);
  }
}

template <int VEC>
__global__ void __launch_bounds__(PN_THREADS) k_pna_fwd(const PnaFwdArgs A) {
  __shared__ __attribute__((aligned(16))) float part[6 * PN_THREADS * VEC];
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  const bool member = rl < A.RPB;                       // (256 % LPR lanes at the end of the block own no row)
  const int span = A.LPR * VEC;                         // columns of one pass
  const int64_t tiles = (A.N + A.RPB - 1) / A.RPB;
  int any_long = 0;
  // ---- rows of at most ROW_WALK_LONG_ROW slots: one lane group each, serially --------------------------------------
  if (member) {
    for (int f = lg * VEC; f < A.F; f += span) {        // (one pass up to 64 * VEC columns)
      for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * A.RPB + rl;
        if (r >= A.N) continue;
        const int s = A.rowptr[r], t = A.rowptr[r + 1];
        if (t - s > ROW_WALK_LONG_ROW) { any_long = 1; continue; }
        PnaAcc<VEC> acc;
        acc.clear();
        walk_slots<VEC>(A, s, t, f, acc);
        finish_row<VEC>(A, r, f, t - s, acc);
      }
    }
  }
  if (!__syncthreads_or(any_long)) return;
  // ---- the long rows among this block's tiles: the whole block per row, chunk partials merged in chunk order ------
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int i = 0; i < A.RPB; ++i) {
      const int64_t r = tile * A.RPB + i;
      if (r >= A.N) break;
      const int s = A.rowptr[r], t = A.rowptr[r + 1];   // block-uniform
      if (t - s <= ROW_WALK_LONG_ROW) continue;
      const int chunks = (t - s + ROW_WALK_CHUNK - 1) / ROW_WALK_CHUNK;
      for (int f0 = 0; f0 < A.F; f0 += span) {
        const int f = f0 + lg * VEC;
        const bool live = member && f < A.F;
        PnaAcc<VEC> total;
        total.clear();
        for (int c0 = 0; c0 < chunks; c0 += A.RPB) {
          const int c = c0 + rl;
          if (live && c < chunks) {
            const int cs = s + c * ROW_WALK_CHUNK;
            const int ct = cs + ROW_WALK_CHUNK < t ? cs + ROW_WALK_CHUNK : t;
            PnaAcc<VEC> acc;
            acc.clear();
            walk_slots<VEC>(A, cs, ct, f, acc);
            park<VEC>(part, threadIdx.x, acc);
          }
          __syncthreads();
          if (live && rl == 0) {
            const int n = chunks - c0 < A.RPB ? chunks - c0 : A.RPB;
            for (int q = 0; q < n; ++q) {
              PnaAcc<VEC> pq;
              unpark<VEC>(part, q * A.LPR + lg, pq);
              total.merge(pq);
            }
          }
          __syncthreads();
        }
        if (live && rl == 0) finish_row<VEC>(A, r, f, t - s, total);
      }
    }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// gw [N, 4, F] and g_a [N, F] from the cotangent g_out [N, S A F]; one thread per (node, column)
__global__ void __launch_bounds__(PN_THREADS)
k_pna_fold(const int32_t* __restrict__ rowptr, const float* __restrict__ g_out, const float* __restrict__ stdv,
           float* __restrict__ gw, float* __restrict__ g_a, int64_t N, int F, PnaSpec spec) {
  const int64_t total = N * F;
  for (int64_t idx = (int64_t)blockIdx.x * PN_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * PN_THREADS) {
    const int64_t i = idx / F;
    const int f = (int)(idx - i * F);
    const int deg = rowptr[i + 1] - rowptr[i];
    float G[PNA_AGGR] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float* grow = g_out + (size_t)i * spec.S * spec.A * F + f;
    for (int s = 0; s < spec.S; ++s) {
      const float sc = scaler_of(spec.scal[s], deg, spec.avg_deg_log);
      for (int x = 0; x < spec.A; ++x) {
        const float g = mul_rn(sc, grow[(size_t)(s * spec.A + x) * F]);
        const int code = spec.aggr[x];
#pragma unroll
        for (int c = 0; c < PNA_AGGR; ++c)
          if (code == c) G[c] = add_rn(G[c], g);
      }
    }
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f, ga = 0.f;
    if (deg > 0) {
      const float fd = (float)deg;
      w0 = add_rn(G[AG_MEAN] / fd, G[AG_SUM]);
      w1 = G[AG_MIN];
      w2 = G[AG_MAX];
      const float sd = stdv ? stdv[idx] : 0.f;
      w3 = sd > 0.f ? G[AG_STD] / mul_rn(fd, sd) : 0.f;
      ga = add_rn(add_rn(add_rn(G[AG_MEAN], G[AG_MIN]), G[AG_MAX]), mul_rn(fd, G[AG_SUM]));
    }
    float* w = gw + (size_t)i * 4 * F + f;
    w[0] = w0;
    w[F] = w1;
    w[2 * F] = w2;
    w[3 * F] = w3;
    if (g_a) g_a[idx] = ga;
  }
}

struct PnaBwdArgs {
  const int32_t* rowptr;     // source-keyed CSR (the walk); unused by the edge kernel
  const int32_t* col;
  const int32_t* eid;
  const int64_t* ei;         // [2, E] (the edge kernel)
  const float* b;            // [N, F]
  const float* t;            // [E, F] or NULL
  const float* gw;           // [N, 4, F]
  const float* mean;         // [N, F] or NULL (no std among the aggregators)
  const int32_t* arg;        // [N, 2 F] or NULL (neither min nor max)
  float* out;                // g_b [N, F] / g_t [E, F]
  int64_t N, E;
  int F, LPR, RPB;
  int32_t* flag;
};

// dm_k for the columns [f, f + VEC) of edge k: source row bj, target i
template <int VEC>
__device__ __forceinline__ void edge_grad(const PnaBwdArgs& A, typename GV<VEC>::T bj, int64_t i, int64_t k, int f,
                                          float (&dm)[VEC]) {
  using V = GV<VEC>;
  const float* w = A.gw + (size_t)i * 4 * A.F + f;
  const typename V::T w0 = V::load(w);
#pragma unroll
  for (int v = 0; v < VEC; ++v) dm[v] = V::get(w0, v);
  if (A.arg) {
    const typename V::T w1 = V::load(w + A.F), w2 = V::load(w + 2 * A.F);
    const int32_t* ap = A.arg + (size_t)i * 2 * A.F + f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (ap[v] == (int32_t)k) dm[v] = add_rn(dm[v], V::get(w1, v));
      if (ap[A.F + v] == (int32_t)k) dm[v] = add_rn(dm[v], V::get(w2, v));
    }
  }
  if (A.mean) {
    const typename V::T w3 = V::load(w + 3 * A.F), mi = V::load(A.mean + (size_t)i * A.F + f);
    typename V::T tk = V::zero();
    if (A.t) tk = V::load(A.t + (size_t)k * A.F + f);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float r = A.t ? add_rn(V::get(bj, v), V::get(tk, v)) : V::get(bj, v);
      dm[v] = add_rn(dm[v], mul_rn(V::get(w3, v), add_rn(r, -V::get(mi, v))));
    }
  }
}

// slots [s, t) of source row j, columns [f, f + VEC): the running sum continued from `acc`
template <int VEC>
__device__ __forceinline__ typename GV<VEC>::T src_slots(const PnaBwdArgs& A, int s, int t, int f,
                                                         typename GV<VEC>::T bj, typename GV<VEC>::T acc) {
  using V = GV<VEC>;
  float a[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) a[v] = V::get(acc, v);
#pragma unroll 2
  for (int p = s; p < t; ++p) {
    const int i = A.col[p];
    const int k = A.eid[p];
    if (i < 0 || i >= A.N || k < 0 || k >= A.E) {       // never produced by hscn_csr_build; a foreign CSR is flagged
      atomicOr(A.flag, 2);
      continue;
    }
    float dm[VEC];
    edge_grad<VEC>(A, bj, i, k, f, dm);
#pragma unroll
    for (int v = 0; v < VEC; ++v) a[v] = add_rn(a[v], dm[v]);
  }
  return V::make(a);
}

template <int VEC>
__global__ void __launch_bounds__(PN_THREADS) k_pna_src_walk(const PnaBwdArgs A) {
  using V = GV<VEC>;
  __shared__ __attribute__((aligned(16))) float part[PN_THREADS * VEC];
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  const bool member = rl < A.RPB;
  const int span = A.LPR * VEC;
  const int64_t tiles = (A.N + A.RPB - 1) / A.RPB;
  int any_long = 0;
  if (member) {
    for (int f = lg * VEC; f < A.F; f += span) {
      for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * A.RPB + rl;
        if (r >= A.N) continue;
        const int s = A.rowptr[r], t = A.rowptr[r + 1];
        if (t - s > ROW_WALK_LONG_ROW) { any_long = 1; continue; }
        const typename V::T bj = V::load(A.b + (size_t)r * A.F + f);
        V::store(A.out + (size_t)r * A.F + f, src_slots<VEC>(A, s, t, f, bj, V::zero()));
      }
    }
  }
  if (!__syncthreads_or(any_long)) return;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int i = 0; i < A.RPB; ++i) {
      const int64_t r = tile * A.RPB + i;
      if (r >= A.N) break;
      const int s = A.rowptr[r], t = A.rowptr[r + 1];   // block-uniform
      if (t - s <= ROW_WALK_LONG_ROW) continue;
      const int chunks = (t - s + ROW_WALK_CHUNK - 1) / ROW_WALK_CHUNK;
      for (int f0 = 0; f0 < A.F; f0 += span) {
        const int f = f0 + lg * VEC;
        const bool live = member && f < A.F;
        typename V::T bj = V::zero();
        if (live) bj = V::load(A.b + (size_t)r * A.F + f);
        typename V::T total = V::zero();
        for (int c0 = 0; c0 < chunks; c0 += A.RPB) {
          const int c = c0 + rl;
          if (live && c < chunks) {
            const int cs = s + c * ROW_WALK_CHUNK;
            const int ct = cs + ROW_WALK_CHUNK < t ? cs + ROW_WALK_CHUNK : t;
            V::store(part + (size_t)threadIdx.x * VEC, src_slots<VEC>(A, cs, ct, f, bj, V::zero()));
          }
          __syncthreads();
          if (live && rl == 0) {
            const int n = chunks - c0 < A.RPB ? chunks - c0 : A.RPB;
            for (int q = 0; q < n; ++q) {
              const typename V::T pq = V::load(part + (size_t)(q * A.LPR + lg) * VEC);
              float a[VEC];
#pragma unroll
              for (int v = 0; v < VEC; ++v) a[v] = add_rn(V::get(total, v), V::get(pq, v));
              total = V::make(a);
            }
          }
          __syncthreads();
        }
        if (live && rl == 0) V::store(A.out + (size_t)r * A.F + f, total);
      }
    }
  }
}

// g_t[k, :] = dm_k, one lane group per edge of the edge list as given; an edge with a node id outside [0, N) -- the
// CSR build skipped it and raised the flag -- gets a zero row
template <int VEC>
__global__ void __launch_bounds__(PN_THREADS) k_pna_edge_grad(const PnaBwdArgs A) {
  using V = GV<VEC>;
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  if (rl >= A.RPB) return;
  const int span = A.LPR * VEC;
  for (int f = lg * VEC; f < A.F; f += span) {
    for (int64_t k = (int64_t)blockIdx.x * A.RPB + rl; k < A.E; k += (int64_t)gridDim.x * A.RPB) {
      const int64_t src = A.ei[k], dst = A.ei[A.E + k];
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = 0.f;
      if (src < 0 || src >= A.N || dst < 0 || dst >= A.N) {
        atomicOr(A.flag, 1);
      } else {
        edge_grad<VEC>(A, V::load(A.b + (size_t)src * A.F + f), dst, k, f, o);
      }
      V::store(A.out + (size_t)k * A.F + f, V::make(o));
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
// 0 = fine, else the code: a list is a non-empty subset of its codes, in the given order
int read_spec(int F, const int32_t* aggr, int A, const int32_t* scal, int S, float avg_deg_log, PnaSpec& spec) {
  if (F < 1 || !aggr || !scal || A < 1 || A > PNA_AGGR || S < 1 || S > PNA_SCAL) return HSCN_E_BADARG;
  unsigned seen = 0;
  for (int x = 0; x < A; ++x) {
    if (aggr[x] < 0 || aggr[x] >= PNA_AGGR || (seen >> aggr[x] & 1u)) return HSCN_E_BADARG;
    seen |= 1u << aggr[x];
    spec.aggr[x] = aggr[x];
  }
  for (int x = A; x < PNA_AGGR; ++x) spec.aggr[x] = -1;
  seen = 0;
  bool degree = false;
  for (int s = 0; s < S; ++s) {
    if (scal[s] < 0 || scal[s] >= PNA_SCAL || (seen >> scal[s] & 1u)) return HSCN_E_BADARG;
    seen |= 1u << scal[s];
    spec.scal[s] = scal[s];
    degree = degree || scal[s] != SC_IDENTITY;
  }
  for (int s = S; s < PNA_SCAL; ++s) spec.scal[s] = -1;
  if (degree && !(avg_deg_log > 0.f && avg_deg_log < INFINITY)) return HSCN_E_BADARG;
  spec.A = A;
  spec.S = S;
  spec.avg_deg_log = degree ? avg_deg_log : 1.f;
  if (F > PNA_MAX_F) return HSCN_E_UNSUPPORTED;
  return 0;
}

bool has(const PnaSpec& spec, int code) {
  for (int x = 0; x < spec.A; ++x)
    if (spec.aggr[x] == code) return true;
  return false;
}

int check_width(int64_t N, int64_t E, int F) {
  if (!check_csr_sizes({N, E}) || F < 1) return HSCN_E_BADARG;
  if (F > PNA_MAX_F) return HSCN_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int hscn_pna_supported(int F, int num_aggregators, int num_scalers) {
  return F >= 1 && F <= PNA_MAX_F && num_aggregators >= 1 && num_aggregators <= PNA_AGGR && num_scalers >= 1 &&
                 num_scalers <= PNA_SCAL
             ? 1
             : 0;
}
int hscn_pna_long_row(void) { return ROW_WALK_LONG_ROW; }
int hscn_pna_chunk(void) { return ROW_WALK_CHUNK; }

int hscn_pna_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* a, const float* b,
                 const float* t, float* out, float* mean, float* stdv, int32_t* arg, int64_t N, int64_t E, int F,
                 const int32_t* aggregators_host, int num_aggregators, const int32_t* scalers_host, int num_scalers,
                 float avg_deg_log, int32_t* flag, void* stream_) {
  if (!check_csr_sizes({N, E})) return HSCN_E_BADARG;
  PnaFwdArgs A{rowptr, col, eid, a, b, t, out, mean, stdv, arg, N, E, F, 0, 0, {}, flag};
  if (int rc = read_spec(F, aggregators_host, num_aggregators, scalers_host, num_scalers, avg_deg_log, A.spec)) return rc;
  if (N == 0) return 0;
  if (!rowptr || !a || !b || !out || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid)) return HSCN_E_BADARG;
  int VEC;
  lane_groups(F, PN_THREADS, VEC, A.LPR, A.RPB);
  const unsigned nb = capped_grid(N, A.RPB, 8192);
  hipStream_t st = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) { k_pna_fwd<decltype(v)::value><<<nb, PN_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pna_bwd_fold(const int32_t* rowptr, const float* g_out, const float* stdv, float* gw, float* g_a, int64_t N,
                      int F, const int32_t* aggregators_host, int num_aggregators, const int32_t* scalers_host,
                      int num_scalers, float avg_deg_log, void* stream_) {
  if (!check_csr_sizes({N})) return HSCN_E_BADARG;
  PnaSpec spec;
  if (int rc = read_spec(F, aggregators_host, num_aggregators, scalers_host, num_scalers, avg_deg_log, spec)) return rc;
  if (N == 0) return 0;
  if (!rowptr || !g_out || !gw) return HSCN_E_BADARG;
  if (has(spec, AG_STD) && !stdv) return HSCN_E_BADARG;
  const unsigned nb = capped_grid(N * F, PN_THREADS, 8192);
  k_pna_fold<<<nb, PN_THREADS, 0, hscn_stream(stream_)>>>(rowptr, g_out, stdv, gw, g_a, N, F, spec);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pna_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* b,
                     const float* t, const float* gw, const float* mean, const int32_t* arg, float* g_b, int64_t N,
                     int64_t E, int F, int32_t* flag, void* stream_) {
  if (int rc = check_width(N, E, F)) return rc;
  if (N == 0) return 0;
  if (!rowptr_t || !b || !gw || !g_b || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t)) return HSCN_E_BADARG;
  PnaBwdArgs A{rowptr_t, col_t, eid_t, nullptr, b, t, gw, mean, arg, g_b, N, E, F, 0, 0, flag};
  int VEC;
  lane_groups(F, PN_THREADS, VEC, A.LPR, A.RPB);
  const unsigned nb = capped_grid(N, A.RPB, 8192);
  hipStream_t st = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) { k_pna_src_walk<decltype(v)::value><<<nb, PN_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_pna_bwd_edge(const int64_t* edge_index, const float* b, const float* t, const float* gw, const float* mean,
                      const int32_t* arg, float* g_t, int64_t N, int64_t E, int F, int32_t* flag, void* stream_) {
  if (int rc = check_width(N, E, F)) return rc;
  if (E == 0) return 0;
  if (!edge_index || !b || !gw || !g_t || !flag) return HSCN_E_BADARG;
  PnaBwdArgs A{nullptr, nullptr, nullptr, edge_index, b, t, gw, mean, arg, g_t, N, E, F, 0, 0, flag};
  int VEC;
  lane_groups(F, PN_THREADS, VEC, A.LPR, A.RPB);
  const unsigned nb = capped_grid(E, A.RPB, 8192);
  hipStream_t st = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) { k_pna_edge_grad<decltype(v)::value><<<nb, PN_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
