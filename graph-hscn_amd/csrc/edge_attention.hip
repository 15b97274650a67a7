// Multi-head scaled dot-product attention over the in-edges of every node: the message / aggregate of PyG's
// TransformerConv (dropout = 0), Hd heads of width C, with optional edge features added to keys and values.
//
//   s_k   = scale * sum_c q[i,h,c] * (k[j,h,c] + e[k,h,c])        j = src_k, i = dst_k, scale = 1 / sqrt(C)
//   a_k   = softmax of s over the in-edges of i, per head
//   out_i = sum_k a_k * (v[j,h,:] + e[k,h,:])                      (0 for a node without in-edges)
//
// q is [Nd, Hd*C], k and v are [Ns, Hd*C] (the relation may be bipartite), e is [E, Hd*C] or absent.  Row k of e / de
// belongs to edge k of the edge list, not to CSR slot k: every slot goes through eid[slot].  Every listed edge counts
// (loops, repeats).
//
// Work unit: one (row, head), owned by G consecutive lanes, in the layout of csrc/row_walk.h's head-unit layer (VEC = 4
// columns per lane and pass where the width and the pointers allow, 8 floats per lane and operand).  With the
// in-degree 2..4 of a molecular graph and C = 16 a wave therefore carries 16 (row, head) units, none of them idle; the
// heads of one row are neighbouring lane groups, so a row of k / v is read by consecutive lanes.  The dot products
// are reduced over the lane group by xor shuffles (every lane of a group ends with the same bits).
//
// One kernel, three walks (k_edge_attn<VEC, MODE>):
//   MODE 0, target-keyed CSR (forward):  online softmax in CSR slot order -- the running maximum is subtracted before
//                                        every exp; stores out and ONE log-sum-exp per (node, head), kept as the pair
//                                        (m_i, log sum_k exp(s_k - m_i)) with m_i the row's largest logit.  No [E, Hd]
//                                        tensor of weights exists: the backward recomputes a_k = exp((s_k - m_i) - log sum)
//                                        from the same logit bits, so a logit of magnitude 10^3 (integer atom features)
//                                        costs the weights nothing -- a single rounded m + log sum would cost them
//                                        2^-24 |lse| relative, 6e-5 there.
//   MODE 1, target-keyed CSR (backward): delta_i = sum_c dout_i out_i per head (stored for MODE 2),
//                                        ds_k = a_k (dout_i . (v_j + e_k) - delta_i),
//                                        dq_i = sum_k scale ds_k (k_j + e_k),
//                                        de_k = a_k dout_i + scale ds_k q_i   stored once at eid[slot] (one writer)
//   MODE 2, source-keyed CSR (backward): dk_j = sum_{k: src_k = j} scale ds_k q_i,   dv_j = sum a_k dout_i
// Owner-computes, sums in CSR slot order, no float atomics: the same input gives the same bits.
//
// Long rows: the two-phase scheme described in csrc/row_walk.h with a (row, head) pair as the unit; the forward's chunk
// partials are (max, sum, accumulator) triples merged in chunk order, the backward's plain sums added in chunk order.
#include "row_walk.h"

namespace {

struct EAArgs {
  const int32_t* rowptr;   // the walked CSR: keyed by target (MODE 0, 1) or by source (MODE 2)
  const int32_t* col;
  const int32_t* eid;
  const float* q;          // [Nd, HC]
  const float* k;          // [Ns, HC]
  const float* v;          // [Ns, HC]
  const float* e;          // [E, HC] or NULL
  const float* go;         // [Nd, HC]   MODE 1, 2: cotangent of out
  float* out;              // [Nd, HC]   MODE 0 out, MODE 1 in
  float* lse;              // [Nd, Hd, 2] (row maximum, log of the shifted sum)   MODE 0 out, MODE 1 / 2 in
  float* delta;            // [Nd, Hd]   MODE 1 out, MODE 2 in
  float* g0;               // MODE 1: dq [Nd, HC] or NULL;  MODE 2: dk [Ns, HC] or NULL
  float* g1;               // MODE 1: de [E, HC] or NULL;   MODE 2: dv [Ns, HC] or NULL
  int64_t rows, cols, E;   // rows of the walked CSR, range of its col, edges
  int Hd, C, HC;
  int G, UPB, NP;          // lanes per unit, units per workgroup, column passes
  float scale;
  int walk;                // MODE 1: 0 = delta alone, every row taken as empty (neither dq nor de is wanted)
  int32_t* flag;
};

// what a lane keeps of its (row, head) while it walks the slots
struct UnitCtx {
  float a[HEAD_NC];    // MODE 0, 1: q_i;  MODE 2: k_j
  float b[HEAD_NC];    // MODE 1: dout_i;  MODE 2: v_j
  float m, logl, delta;  // MODE 1
};

// the running state of a walk: MODE 0 (m, l, acc0) of the online softmax; MODE 1 acc0 = dq; MODE 2 acc0 = dk, acc1 = dv
struct UnitAcc {
  float m, l;
  float acc0[HEAD_NC];
  float acc1[HEAD_NC];
};

__device__ __forceinline__ void acc_clear(UnitAcc& S) {
  S.m = -INFINITY;
  S.l = 0.f;
#pragma unroll
  for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = S.acc1[i] = 0.f;
}

template <int VEC, int MODE>
__device__ __forceinline__ void unit_begin(const EAArgs& A, int64_t r, int h, int lg, UnitCtx& U) {
  const size_t at = (size_t)r * A.HC + (size_t)h * A.C;
  if (MODE == 0) {
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + at, lg, U.a);
  } else if (MODE == 1) {
    float o[HEAD_NC];
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + at, lg, U.a);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.go + at, lg, U.b);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.out + at, lg, o);
    U.delta = group_sum(rw_dot8(U.b, o), A.G);
    U.m = A.lse[2 * ((size_t)r * A.Hd + h)];
    U.logl = A.lse[2 * ((size_t)r * A.Hd + h) + 1];
  } else {
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.k + at, lg, U.a);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.v + at, lg, U.b);
  }
}

// slots [s, t) of one row for head h, the running state continued in S
template <int VEC, int MODE>
__device__ __forceinline__ void walk_slots(const EAArgs& A, const UnitCtx& U, int h, int lg, int s, int t, UnitAcc& S) {
  const size_t hoff = (size_t)h * A.C;
  for (int p = s; p < t; ++p) {
    const int j = A.col[p];
    const int kx = A.eid[p];
    if (j < 0 || j >= A.cols || kx < 0 || kx >= A.E) {   // never produced by hscn_csr_build; a foreign CSR is flagged
      atomicOr(A.flag, 2);
      continue;
    }
    float ee[HEAD_NC];
    if (A.e) {
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.e + (size_t)kx * A.HC + hoff, lg, ee);
    } else {
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) ee[i] = 0.f;
    }
    const size_t nj = (size_t)j * A.HC + hoff;
    if (MODE == 0) {
      float kk[HEAD_NC], vv[HEAD_NC];
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.k + nj, lg, kk);
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.v + nj, lg, vv);
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) kk[i] += ee[i], vv[i] += ee[i];
      const float sc = group_sum(rw_dot8(U.a, kk), A.G) * A.scale;
      if (sc > S.m) {                                    // a new running maximum: rescale what was summed under the old
        const float corr = expf(S.m - sc);
        S.l *= corr;
#pragma unroll
        for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] *= corr;
        S.m = sc;
      }
      const float w = expf(sc - S.m);
      S.l += w;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = fmaf(w, vv[i], S.acc0[i]);
    } else if (MODE == 1) {
      float kk[HEAD_NC], vv[HEAD_NC];
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.k + nj, lg, kk);
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.v + nj, lg, vv);
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) kk[i] += ee[i], vv[i] += ee[i];
      const float sc = group_sum(rw_dot8(U.a, kk), A.G) * A.scale;
      const float dp = group_sum(rw_dot8(U.b, vv), A.G);
      const float a = expf((sc - U.m) - U.logl);
      const float ds = a * (dp - U.delta) * A.scale;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = fmaf(ds, kk[i], S.acc0[i]);
      if (A.g1) {
        float de[HEAD_NC];
#pragma unroll
        for (int i = 0; i < HEAD_NC; ++i) de[i] = fmaf(ds, U.a[i], a * U.b[i]);
        rw_store_cols<VEC>(A.G, A.NP, A.C, A.g1 + (size_t)kx * A.HC + hoff, lg, de);
      }
    } else {
      float qq[HEAD_NC], gg[HEAD_NC], kk[HEAD_NC], vv[HEAD_NC];   // (j is the target here, the row is the source)
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + nj, lg, qq);
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.go + nj, lg, gg);
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) kk[i] = U.a[i] + ee[i], vv[i] = U.b[i] + ee[i];
      const float sc = group_sum(rw_dot8(qq, kk), A.G) * A.scale;
      const float dp = group_sum(rw_dot8(gg, vv), A.G);
      const size_t ih = (size_t)j * A.Hd + h;
      const float a = expf((sc - A.lse[2 * ih]) - A.lse[2 * ih + 1]);
      const float ds = a * (dp - A.delta[ih]) * A.scale;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) {
        S.acc0[i] = fmaf(ds, qq[i], S.acc0[i]);
        S.acc1[i] = fmaf(a, gg[i], S.acc1[i]);
      }
    }
  }
}

template <int VEC, int MODE>
__device__ __forceinline__ void unit_finish(const EAArgs& A, const UnitCtx& U, int64_t r, int h, int lg, const UnitAcc& S) {
  const size_t at = (size_t)r * A.HC + (size_t)h * A.C;
  if (MODE == 0) {
    float o[HEAD_NC];
    const bool any = S.l > 0.f || S.l != S.l;            // (a NaN sum is shown, not hidden)
#pragma unroll
    for (int i = 0; i < HEAD_NC; ++i) o[i] = any ? S.acc0[i] / S.l : 0.f;
    rw_store_cols<VEC>(A.G, A.NP, A.C, A.out + at, lg, o);
    if (lg == 0) {
      A.lse[2 * ((size_t)r * A.Hd + h)] = any ? S.m : 0.f;
      A.lse[2 * ((size_t)r * A.Hd + h) + 1] = any ? logf(S.l) : 0.f;
    }
  } else if (MODE == 1) {
    if (lg == 0) A.delta[(size_t)r * A.Hd + h] = U.delta;
    if (A.g0) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g0 + at, lg, S.acc0);
  } else {
    if (A.g0) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g0 + at, lg, S.acc0);
    if (A.g1) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g1 + at, lg, S.acc1);
  }
}

template <int VEC, int MODE>
__global__ void __launch_bounds__(HEAD_THREADS) k_edge_attn(const EAArgs A) {
  constexpr int NACC = MODE == 2 ? 2 : 1;
  __shared__ float part[NACC * HEAD_THREADS * HEAD_NC];  // chunk partials of a long row, [accumulator][thread][HEAD_NC]
  __shared__ float part_m[HEAD_THREADS], part_l[HEAD_THREADS];
  const bool walk = MODE != 1 || A.walk != 0;
  const int ul = threadIdx.x / A.G;                      // unit of this lane group within the workgroup's tile
  const int lg = threadIdx.x - ul * A.G;
  const int64_t units = A.rows * A.Hd;
  const int64_t tiles = (units + A.UPB - 1) / A.UPB;
  int any_long = 0;
  // ---- rows of at most ROW_WALK_LONG_ROW slots: one lane group per (row, head), serially ------------------------
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t u = tile * A.UPB + ul;
    if (u >= units) continue;
    const int64_t r = u / A.Hd;
    const int h = (int)(u - r * A.Hd);
    const int s = A.rowptr[r], t = walk ? A.rowptr[r + 1] : s;
    if (t - s > ROW_WALK_LONG_ROW) { any_long = 1; continue; }
    UnitCtx U;
    UnitAcc S;
    unit_begin<VEC, MODE>(A, r, h, lg, U);
    acc_clear(S);
    walk_slots<VEC, MODE>(A, U, h, lg, s, t, S);
    unit_finish<VEC, MODE>(A, U, r, h, lg, S);
  }
  if (!__syncthreads_or(any_long)) return;
  // ---- the long rows among this workgroup's tiles: a lane group per chunk, partials merged in chunk order --------
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int i = 0; i < A.UPB; ++i) {
      const int64_t u = tile * A.UPB + i;
      if (u >= units) break;
      const int64_t r = u / A.Hd;
      const int h = (int)(u - r * A.Hd);
      const int s = A.rowptr[r], t = A.rowptr[r + 1];    // workgroup-uniform
      if (t - s <= ROW_WALK_LONG_ROW) continue;
      const int chunks = (t - s + ROW_WALK_CHUNK - 1) / ROW_WALK_CHUNK;
      UnitCtx U;
      UnitAcc T;                                         // the merged state (used by lane group 0)
      unit_begin<VEC, MODE>(A, r, h, lg, U);
      acc_clear(T);
      for (int c0 = 0; c0 < chunks; c0 += A.UPB) {
        const int c = c0 + ul;
        if (c < chunks) {
          const int cs = s + c * ROW_WALK_CHUNK;
          const int ct = cs + ROW_WALK_CHUNK < t ? cs + ROW_WALK_CHUNK : t;
          UnitAcc S;
          acc_clear(S);
          walk_slots<VEC, MODE>(A, U, h, lg, cs, ct, S);
#pragma unroll
          for (int x = 0; x < HEAD_NC; ++x) {
            part[threadIdx.x * HEAD_NC + x] = S.acc0[x];
            if (MODE == 2) part[(HEAD_THREADS + threadIdx.x) * HEAD_NC + x] = S.acc1[x];
          }
          if (MODE == 0) part_m[threadIdx.x] = S.m, part_l[threadIdx.x] = S.l;
        }
        __syncthreads();
        if (ul == 0) {
          const int n = chunks - c0 < A.UPB ? chunks - c0 : A.UPB;
          for (int g = 0; g < n; ++g) {
            const int src = g * A.G + lg;
            float f = 1.f;
            if (MODE == 0) {
              const float pm = part_m[src], pl = part_l[src];
              if (pm > T.m) {
                const float corr = expf(T.m - pm);
                T.l *= corr;
#pragma unroll
                for (int x = 0; x < HEAD_NC; ++x) T.acc0[x] *= corr;
                T.m = pm;
              }
              f = expf(pm - T.m);
              T.l = fmaf(pl, f, T.l);
            }
#pragma unroll
            for (int x = 0; x < HEAD_NC; ++x) {
              if (MODE == 0) T.acc0[x] = fmaf(part[src * HEAD_NC + x], f, T.acc0[x]);
              else T.acc0[x] += part[src * HEAD_NC + x];
              if (MODE == 2) T.acc1[x] += part[(HEAD_THREADS + src) * HEAD_NC + x];
            }
          }
        }
        __syncthreads();
      }
      if (ul == 0) unit_finish<VEC, MODE>(A, U, r, h, lg, T);
    }
  }
}

template <int MODE>
int launch_walk(EAArgs A, hipStream_t st) {
  const int VEC = lane_layout(A.C, {A.q, A.k, A.v, A.e, A.go, A.out, A.g0, A.g1}, A.G, A.UPB, A.NP);
  const unsigned nb = capped_grid(A.rows * A.Hd, A.UPB, 16384);
  dispatch_vec(VEC, [&](auto v) { k_edge_attn<decltype(v)::value, MODE><<<nb, HEAD_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int check_common(int64_t Nd, int64_t Ns, int64_t E, int heads, int head_dim) {
  if (!check_csr_sizes({Nd, Ns, E}) || heads < 1 || head_dim < 1) return HSCN_E_BADARG;
  if (!head_walk_supported(heads, head_dim)) return HSCN_E_UNSUPPORTED;
  return 0;
}

void set_shape(EAArgs& A, int64_t rows, int64_t cols, int64_t E, int heads, int head_dim) {
  A.rows = rows, A.cols = cols, A.E = E;
  A.Hd = heads, A.C = head_dim, A.HC = heads * head_dim;
  A.scale = head_scale(head_dim);
}

}  // namespace

extern "C" {

int hscn_edge_attn_supported(int heads, int head_dim) { return head_walk_supported(heads, head_dim) ? 1 : 0; }
int hscn_edge_attn_long_row(void) { return ROW_WALK_LONG_ROW; }
int hscn_edge_attn_chunk(void) { return ROW_WALK_CHUNK; }

int hscn_edge_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* q, const float* k,
                       const float* v, const float* e, float* out, float* lse, int64_t Nd, int64_t Ns, int64_t E,
                       int heads, int head_dim, int32_t* flag, void* stream_) {
  if (int rc = check_common(Nd, Ns, E, heads, head_dim)) return rc;
  if (!rowptr || !flag || (Nd > 0 && (!q || !out || !lse))) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !k || !v)) return HSCN_E_BADARG;
  if (Nd == 0) return 0;
  EAArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid;
  A.q = q, A.k = k, A.v = v, A.e = E > 0 ? e : nullptr;
  A.out = out, A.lse = lse, A.flag = flag;
  set_shape(A, Nd, Ns, E, heads, head_dim);
  return launch_walk<0>(A, hscn_stream(stream_));
}

int hscn_edge_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* q, const float* k,
                           const float* v, const float* e, const float* out, const float* lse, const float* g_out,
                           float* delta, float* dq, float* de, int64_t Nd, int64_t Ns, int64_t E, int heads,
                           int head_dim, int32_t* flag, void* stream_) {
  if (int rc = check_common(Nd, Ns, E, heads, head_dim)) return rc;
  if (!rowptr || !flag || (Nd > 0 && (!q || !out || !lse || !g_out || !delta))) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !k || !v)) return HSCN_E_BADARG;
  if (de && E > 0 && !e) return HSCN_E_BADARG;           // a gradient for edge features that were not given
  if (Nd == 0) return 0;
  EAArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid;
  A.q = q, A.k = k, A.v = v, A.e = E > 0 ? e : nullptr, A.go = g_out;
  A.out = const_cast<float*>(out), A.lse = const_cast<float*>(lse), A.delta = delta;
  A.g0 = dq, A.g1 = E > 0 ? de : nullptr, A.walk = (dq || de) ? 1 : 0;
  A.flag = flag;
  set_shape(A, Nd, Ns, E, heads, head_dim);
  return launch_walk<1>(A, hscn_stream(stream_));
}

int hscn_edge_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* q,
                           const float* k, const float* v, const float* e, const float* lse, const float* delta,
                           const float* g_out, float* dk, float* dv, int64_t Nd, int64_t Ns, int64_t E, int heads,
                           int head_dim, int32_t* flag, void* stream_) {
  if (int rc = check_common(Nd, Ns, E, heads, head_dim)) return rc;
  if (!rowptr_t || !flag || (Ns > 0 && (!k || !v))) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t || !q || !lse || !delta || !g_out)) return HSCN_E_BADARG;
  if (Ns == 0 || (!dk && !dv)) return 0;
  EAArgs A{};
  A.rowptr = rowptr_t, A.col = col_t, A.eid = eid_t;
  A.q = q, A.k = k, A.v = v, A.e = E > 0 ? e : nullptr, A.go = g_out;
  A.lse = const_cast<float*>(lse), A.delta = const_cast<float*>(delta);
  A.g0 = dk, A.g1 = dv, A.flag = flag;
  set_shape(A, Ns, Nd, E, heads, head_dim);
  return launch_walk<2>(A, hscn_stream(stream_));
}

}  // extern "C"
