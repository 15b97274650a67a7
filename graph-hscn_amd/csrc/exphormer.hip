// Exphormer's sparse attention over a union graph (local edges, expander edges, virtual-node edges) with TYPED edge
// rows: Hd heads of width C, the score multiplicative in the edge feature, clamped, normalised without a softmax shift.
//
//   s_k   = scale * sum_c q[i,h,c] * k[j,h,c] * e_k[h,c]          j = src_k, i = dst_k, scale = 1 / sqrt(C)
//   w_k   = exp(clamp(s_k, -5, 5))
//   Z_i   = sum_k w_k                                             over the in-edges of i, per head
//   out_i = (sum_k w_k v[j,h,:]) / (Z_i + 1e-6)                   (exact zeros for a node without in-edges)
//
// q, k, v are [N, Hd*C] over the same N rows (real nodes, then virtual nodes).  The feature row of union edge x is named
// by erow[x]: a value below El is row erow[x] of e_edge [El, Hd*C] (a local edge's own features), a value El + tau is
// row tau of the table e_type [T, Hd*C] (T <= 10 rows that all expander / virtual edges share; they stay in L1 / L2).
// Every slot goes through eid[slot] first, as in edge_attention.hip.  Every listed edge counts (loops, repeats).
//
// Layout, lane groups, VEC and the 8 floats a lane holds per operand are the head-unit layer of csrc/row_walk.h (shared
// with csrc/edge_attention.hip); long rows use the two-phase scheme of the same file with its two constants (a virtual
// node's in-row is a whole graph: long rows are the normal case here).  The skeleton is spelt here once more, as
// row_walk.h explains.
//
// One kernel, three walks (k_exph_attn<VEC, MODE>):
//   MODE 0, target-keyed CSR (forward):  stores out and ONE float per (row, head), Z_i.  w <= e^5, so a row of 2^20
//                                        edges sums well inside float32 and no shift is needed; the chunk partials of a
//                                        long row are plain (Z, accumulator) sums added in chunk order.
//   MODE 1, target-keyed CSR (backward): r_i = 1 / (Z_i + 1e-6), delta_i = sum_c dout_i out_i (stored for MODE 2 and
//                                        the table pass), ds_k = w_k r_i (dout_i . v_j - delta_i) [-5 < s_k < 5],
//                                        dq_i = scale sum_k ds_k (k_j * e_k),
//                                        de_k = scale ds_k (q_i * k_j) stored at row erow[eid[slot]] for slots whose
//                                        row is an e_edge row (each local edge occurs once in the union: one writer)
//   MODE 2, source-keyed CSR (backward): dk_j = scale sum ds_k (q_i * e_k),   dv_j = sum w_k r_i dout_i
// The weights are recomputed from the same logit bits (the same products in the same order), never stored.
//
// The table gradient de_type[tau] = scale sum over the union edges of type tau of ds_k (q_i * k_j) walks a type-keyed
// list of union edge ids (rowptr [T + 1], item; a stable counting sort by type, so ascending edge ids): a type is cut
// into chunks of EXPH_TYPE_CHUNK slots counted from the type's first slot, each chunk is a serial sum from zero by one
// lane group stored as a partial (k_exph_type_partial), and a second launch adds a type's partials in chunk order
// (k_exph_type_combine).  A type of at most EXPH_TYPE_LONG_ROW slots is a single chunk.  So the bits of de_type[tau]
// depend on the type's slots in list order alone, not on the grid.  A type without slots gets exact zeros.
// Owner-computes everywhere, no float atomics: the same input gives the same bits.
#include "row_walk.h"

namespace {

constexpr int XA_MAX_TYPES = 10;         // 2 + 2 * nv, nv <= 4
constexpr int EXPH_TYPE_LONG_ROW = 64;   // types with MORE slots than this are split (hscn_exph_type_long_row)
constexpr int EXPH_TYPE_CHUNK = 64;      // slots per chunk of a split type (hscn_exph_type_chunk)
static_assert(EXPH_TYPE_LONG_ROW >= EXPH_TYPE_CHUNK, "chunks of all types stay within E / CHUNK + T");
constexpr int XA_AHEAD = 4;              // slots whose loads are in flight together (walk_slots, type_batch)
constexpr float XA_CLAMP = 5.0f;
constexpr float XA_EPS = 1e-6f;

struct XAArgs {
  const int32_t* rowptr;   // the walked CSR: keyed by target (MODE 0, 1) or by source (MODE 2)
  const int32_t* col;
  const int32_t* eid;
  const int32_t* erow;     // [E] feature row of every union edge
  const float* q;          // [N, HC]
  const float* k;          // [N, HC]
  const float* v;          // [N, HC]
  const float* e_edge;     // [El, HC] or NULL (El = 0)
  const float* e_type;     // [T, HC]
  const float* go;         // [N, HC]   MODE 1, 2: cotangent of out
  float* out;              // [N, HC]   MODE 0 out, MODE 1 in
  float* z;                // [N, Hd]   MODE 0 out, MODE 1 / 2 in
  float* delta;            // [N, Hd]   MODE 1 out, MODE 2 in
  float* g0;               // MODE 1: dq or NULL;  MODE 2: dk or NULL
  float* g1;               // MODE 1: de_edge [El, HC] or NULL;  MODE 2: dv or NULL
  int64_t rows, E, El;     // rows of the CSR (= range of its col), union edges, rows of e_edge
  int T;
  int Hd, C, HC;
  int G, UPB, NP;          // lanes per unit, units per workgroup, column passes
  float scale;
  int walk;                // MODE 1: 0 = delta alone, every row taken as empty (neither dq nor de is wanted)
  int32_t* flag;
};

// the logit of one slot from q and (k * e), the product rounded first: every pass and the table kernel call this with
// the same lane layout, so they see the same bits
__device__ __forceinline__ float logit(const float (&q)[HEAD_NC], const float (&ke)[HEAD_NC], int G, float scale) {
  return group_sum(rw_dot8(q, ke), G) * scale;
}
__device__ __forceinline__ float weight_of(float s) { return expf(fminf(fmaxf(s, -XA_CLAMP), XA_CLAMP)); }
__device__ __forceinline__ float gate_of(float s) { return (s > -XA_CLAMP && s < XA_CLAMP) ? 1.f : 0.f; }

// what a lane keeps of its (row, head) while it walks the slots
struct UnitCtx {
  float a[HEAD_NC];    // MODE 0, 1: q_i;  MODE 2: k_j
  float b[HEAD_NC];    // MODE 1: dout_i;  MODE 2: v_j
  float r, delta;    // MODE 1
};

// the running state of a walk: MODE 0 (l = Z, acc0); MODE 1 acc0 = dq; MODE 2 acc0 = dk, acc1 = dv
struct UnitAcc {
  float l;
  float acc0[HEAD_NC];
  float acc1[HEAD_NC];
};

__device__ __forceinline__ void acc_clear(UnitAcc& S) {
  S.l = 0.f;
#pragma unroll
  for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = S.acc1[i] = 0.f;
}

template <int VEC, int MODE>
__device__ __forceinline__ void unit_begin(const XAArgs& A, int64_t r, int h, int lg, UnitCtx& U) {
  const size_t at = (size_t)r * A.HC + (size_t)h * A.C;
  if (MODE == 0) {
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + at, lg, U.a);
  } else if (MODE == 1) {
    float o[HEAD_NC];
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + at, lg, U.a);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.go + at, lg, U.b);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.out + at, lg, o);
    U.delta = group_sum(rw_dot8(U.b, o), A.G);
    U.r = 1.0f / (A.z[(size_t)r * A.Hd + h] + XA_EPS);
  } else {
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.k + at, lg, U.a);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.v + at, lg, U.b);
  }
}

// The walk is latency-bound: a slot's column and edge id, then its feature row's number, then the three rows they name
// are three dependent trips to memory.  So slots are taken XA_AHEAD at a time and the trips of consecutive batches
// overlap (walk_slots): while batch b's rows are in flight, the feature-row numbers of batch b + 1 and the columns and
// edge ids of batch b + 2 are requested; then batch b is accumulated IN SLOT ORDER -- the bits are those of a
// slot-by-slot walk.  A slot that names a column, an edge or a feature row out of range (never produced by
// hscn_csr_build; a foreign CSR) reads row 0, adds nothing and sets bit 1 of the flag word.
template <int AH>
struct SlotIdx {
  int j[AH];       // col of the slot
  int er[AH];      // first its edge id (slot_ids), then that edge's feature row (slot_rows)
  bool ok[AH];
};

template <int AH>
__device__ __forceinline__ void slot_ids(const XAArgs& A, int p, SlotIdx<AH>& I) {
#pragma unroll
  for (int u = 0; u < AH; ++u) I.j[u] = A.col[p + u], I.er[u] = A.eid[p + u];
}

template <int AH>
__device__ __forceinline__ void slot_rows(const XAArgs& A, SlotIdx<AH>& I) {
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    I.ok[u] = I.j[u] >= 0 && I.j[u] < A.rows && I.er[u] >= 0 && I.er[u] < A.E;
    I.er[u] = A.erow[I.ok[u] ? I.er[u] : 0];               // (the value is not looked at before batch_accumulate)
  }
}

// what a lane holds of AH slots: the feature rows, MODE 0 / 1 k_j and v_j, MODE 2 q_i and dout_i with Z_i and delta_i
template <int AH>
struct SlotData {
  float ee[AH][HEAD_NC], x0[AH][HEAD_NC], x1[AH][HEAD_NC], zz[AH], dd[AH];
};

template <int VEC, int MODE, int AH>
__device__ __forceinline__ void batch_load(const XAArgs& A, int h, int lg, SlotIdx<AH>& I, SlotData<AH>& D) {
  const size_t hoff = (size_t)h * A.C;
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    I.ok[u] = I.ok[u] && I.er[u] >= 0 && I.er[u] < A.El + A.T;
    if (!I.ok[u]) I.j[u] = 0, I.er[u] = (int)A.El;         // (row 0 of q / k / v and of the table exist)
    const int er = I.er[u];
    const float* erp = er < A.El ? A.e_edge + (size_t)er * A.HC : A.e_type + (size_t)(er - A.El) * A.HC;
    const size_t nj = (size_t)I.j[u] * A.HC + hoff;
    rw_load_cols<VEC>(A.G, A.NP, A.C, erp + hoff, lg, D.ee[u]);
    rw_load_cols<VEC>(A.G, A.NP, A.C, (MODE == 2 ? A.q : A.k) + nj, lg, D.x0[u]);
    rw_load_cols<VEC>(A.G, A.NP, A.C, (MODE == 2 ? A.go : A.v) + nj, lg, D.x1[u]);
    if (MODE == 2) D.zz[u] = A.z[(size_t)I.j[u] * A.Hd + h], D.dd[u] = A.delta[(size_t)I.j[u] * A.Hd + h];
  }
}

template <int VEC, int MODE, int AH>
__device__ __forceinline__ void batch_accumulate(const XAArgs& A, const UnitCtx& U, int h, int lg, const SlotIdx<AH>& I,
                                                 SlotData<AH>& D, UnitAcc& S) {
  const size_t hoff = (size_t)h * A.C;
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    if (!I.ok[u]) {
      atomicOr(A.flag, 2);
      continue;
    }
    if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) D.x0[u][i] *= D.ee[u][i];
      const float w = weight_of(logit(U.a, D.x0[u], A.G, A.scale));
      S.l += w;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = fmaf(w, D.x1[u][i], S.acc0[i]);
    } else if (MODE == 1) {
      float ke[HEAD_NC];
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) ke[i] = D.x0[u][i] * D.ee[u][i];
      const float sc = logit(U.a, ke, A.G, A.scale);
      const float dp = group_sum(rw_dot8(U.b, D.x1[u]), A.G);
      const float ds = weight_of(sc) * U.r * (dp - U.delta) * gate_of(sc) * A.scale;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) S.acc0[i] = fmaf(ds, ke[i], S.acc0[i]);
      if (A.g1 && I.er[u] < A.El) {                        // a row of e_edge: this slot is its one writer
        float de[HEAD_NC];
#pragma unroll
        for (int i = 0; i < HEAD_NC; ++i) de[i] = ds * (U.a[i] * D.x0[u][i]);
        rw_store_cols<VEC>(A.G, A.NP, A.C, A.g1 + (size_t)I.er[u] * A.HC + hoff, lg, de);
      }
    } else {                                               // (j is the target here, the row is the source)
      float ke[HEAD_NC];
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) ke[i] = U.a[i] * D.ee[u][i];
      const float sc = logit(D.x0[u], ke, A.G, A.scale);
      const float dp = group_sum(rw_dot8(D.x1[u], U.b), A.G);
      const float wr = weight_of(sc) * (1.0f / (D.zz[u] + XA_EPS));
      const float ds = wr * (dp - D.dd[u]) * gate_of(sc) * A.scale;
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) {
        S.acc0[i] = fmaf(ds, D.x0[u][i] * D.ee[u][i], S.acc0[i]);
        S.acc1[i] = fmaf(wr, D.x1[u][i], S.acc1[i]);
      }
    }
  }
}

// slots [s, t) of one row for head h, the running state continued in S
template <int VEC, int MODE>
__device__ __forceinline__ void walk_slots(const XAArgs& A, const UnitCtx& U, int h, int lg, int s, int t, UnitAcc& S) {
  constexpr int AH = XA_AHEAD;
  const int nb = (t - s) / AH;
  int p = s;
  if (nb > 0) {
    SlotIdx<AH> cur{}, nx1{}, nx2{};                       // batch b (rows known), b + 1 (ids known), b + 2
    slot_ids(A, p, cur);
    slot_rows(A, cur);
    if (nb > 1) slot_ids(A, p + AH, nx1);
    for (int b = 0; b < nb; ++b, p += AH) {
      SlotData<AH> D;
      batch_load<VEC, MODE>(A, h, lg, cur, D);
      if (b + 1 < nb) slot_rows(A, nx1);
      if (b + 2 < nb) slot_ids(A, p + 2 * AH, nx2);
      batch_accumulate<VEC, MODE>(A, U, h, lg, cur, D, S);
      cur = nx1;
      nx1 = nx2;
    }
  }
  for (; p < t; ++p) {
    SlotIdx<1> I;
    SlotData<1> D;
    slot_ids(A, p, I);
    slot_rows(A, I);
    batch_load<VEC, MODE>(A, h, lg, I, D);
    batch_accumulate<VEC, MODE>(A, U, h, lg, I, D, S);
  }
}

template <int VEC, int MODE>
__device__ __forceinline__ void unit_finish(const XAArgs& A, const UnitCtx& U, int64_t r, int h, int lg, const UnitAcc& S) {
  const size_t at = (size_t)r * A.HC + (size_t)h * A.C;
  if (MODE == 0) {
    float o[HEAD_NC];
    const float inv = 1.0f / (S.l + XA_EPS);
#pragma unroll
    for (int i = 0; i < HEAD_NC; ++i) o[i] = S.acc0[i] * inv;
    rw_store_cols<VEC>(A.G, A.NP, A.C, A.out + at, lg, o);
    if (lg == 0) A.z[(size_t)r * A.Hd + h] = S.l;
  } else if (MODE == 1) {
    if (lg == 0) A.delta[(size_t)r * A.Hd + h] = U.delta;
    if (A.g0) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g0 + at, lg, S.acc0);
  } else {
    if (A.g0) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g0 + at, lg, S.acc0);
    if (A.g1) rw_store_cols<VEC>(A.G, A.NP, A.C, A.g1 + at, lg, S.acc1);
  }
}

template <int VEC, int MODE>
__global__ void __launch_bounds__(HEAD_THREADS) k_exph_attn(const XAArgs A) {
  constexpr int NACC = MODE == 2 ? 2 : 1;
  __shared__ float part[NACC * HEAD_THREADS * HEAD_NC];  // chunk partials of a long row, [accumulator][thread][HEAD_NC]
  __shared__ float part_l[HEAD_THREADS];
  const bool walk = MODE != 1 || A.walk != 0;
  const int ul = threadIdx.x / A.G;                      // unit of this lane group within the workgroup's tile
  const int lg = threadIdx.x - ul * A.G;
  const int64_t units = A.rows * A.Hd;
  const int64_t tiles = (units + A.UPB - 1) / A.UPB;
  int any_long = 0;
  // A tile's rows lie `tiles` apart in the launch, not side by side: the virtual nodes are the LAST rows and every one
  // of them is a hub, so consecutive rows in one tile would leave a handful of workgroups with all the long walks of
  // the launch while the rest are done; `tiles` apart, a workgroup holds one or two.  The heads of a row stay
  // neighbouring lane groups (a row of q / out is touched by consecutive lanes) where they fill whole tiles.  Which
  // units share a workgroup changes no bit of any of them.
  const int keep = A.UPB % A.Hd == 0 ? A.Hd : 1;
  // ---- rows of at most ROW_WALK_LONG_ROW slots: one lane group per (row, head), serially ------------------------
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t u = ((int64_t)(ul / keep) * tiles + tile) * keep + ul % keep;
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
  // ---- the long rows among this workgroup's tiles: a lane group per chunk, partials added in chunk order --------
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int i = 0; i < A.UPB; ++i) {
      const int64_t u = ((int64_t)(i / keep) * tiles + tile) * keep + i % keep;
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
          if (MODE == 0) part_l[threadIdx.x] = S.l;
        }
        __syncthreads();
        if (ul == 0) {
          const int n = chunks - c0 < A.UPB ? chunks - c0 : A.UPB;
          for (int g = 0; g < n; ++g) {
            const int src = g * A.G + lg;
            if (MODE == 0) T.l += part_l[src];
#pragma unroll
            for (int x = 0; x < HEAD_NC; ++x) {
              T.acc0[x] += part[src * HEAD_NC + x];
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

// ---- the table gradient -----------------------------------------------------------------------------------------------
struct XTArgs {
  const int32_t* trowptr;  // [T + 1] slots of every type in the type-keyed list
  const int32_t* titem;    // union edge ids, ascending within a type
  const int64_t* src;      // [E] edge_index[0]
  const int64_t* dst;      // [E] edge_index[1]
  const float* q;
  const float* k;
  const float* v;
  const float* e_type;     // [T, HC]
  const float* go;
  const float* z;          // [N, Hd]
  const float* delta;      // [N, Hd]
  float* part;             // [max_chunks, HC]
  float* de_type;          // [T, HC]
  int64_t N, E, max_chunks;
  int T, Hd, C, HC, G, UPB, NP;
  float scale;
  int32_t* flag;
};

__device__ __forceinline__ int type_chunks(int n) {
  return n <= 0 ? 0 : (n <= EXPH_TYPE_LONG_ROW ? 1 : (n + EXPH_TYPE_CHUNK - 1) / EXPH_TYPE_CHUNK);
}

// the slots [s, e) of type tau, or an empty range (and bit 1) for a rowptr that is not one of this list
__device__ __forceinline__ void type_range(const XTArgs& A, int tau, int& s, int& e) {
  s = A.trowptr[tau], e = A.trowptr[tau + 1];
  if (s < 0 || e < s || e > A.E) {
    atomicOr(A.flag, 2);
    s = e = 0;
  }
}

// AH consecutive slots of the type-keyed list from p on, accumulated in list order (the look-ahead of walk_slots: the
// edge ids, then their ends, then the four rows of every slot are in flight together).  A slot with an edge id or an
// end out of range reads row 0, adds nothing and sets bit 1 (hscn_csr_build left that edge out of both CSRs as well).
template <int VEC, int AH>
__device__ __forceinline__ void type_batch(const XTArgs& A, int h, int lg, int p, const float (&ee)[HEAD_NC],
                                           float (&acc)[HEAD_NC]) {
  const size_t hoff = (size_t)h * A.C;
  int kx[AH];
  int64_t i[AH], j[AH];
  bool ok[AH];
#pragma unroll
  for (int u = 0; u < AH; ++u) kx[u] = A.titem[p + u];
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    ok[u] = kx[u] >= 0 && kx[u] < A.E;
    j[u] = A.src[ok[u] ? kx[u] : 0], i[u] = A.dst[ok[u] ? kx[u] : 0];
  }
  float qq[AH][HEAD_NC], gg[AH][HEAD_NC], kk[AH][HEAD_NC], vv[AH][HEAD_NC], zz[AH], dd[AH];
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    ok[u] = ok[u] && j[u] >= 0 && j[u] < A.N && i[u] >= 0 && i[u] < A.N;
    if (!ok[u]) i[u] = j[u] = 0;
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.q + (size_t)i[u] * A.HC + hoff, lg, qq[u]);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.go + (size_t)i[u] * A.HC + hoff, lg, gg[u]);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.k + (size_t)j[u] * A.HC + hoff, lg, kk[u]);
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.v + (size_t)j[u] * A.HC + hoff, lg, vv[u]);
    zz[u] = A.z[(size_t)i[u] * A.Hd + h], dd[u] = A.delta[(size_t)i[u] * A.Hd + h];
  }
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    if (!ok[u]) {
      atomicOr(A.flag, 2);
      continue;
    }
    float ke[HEAD_NC];
#pragma unroll
    for (int x = 0; x < HEAD_NC; ++x) ke[x] = kk[u][x] * ee[x];
    const float sc = logit(qq[u], ke, A.G, A.scale);
    const float dp = group_sum(rw_dot8(gg[u], vv[u]), A.G);
    const float ds = weight_of(sc) * (1.0f / (zz[u] + XA_EPS)) * (dp - dd[u]) * gate_of(sc) * A.scale;
#pragma unroll
    for (int x = 0; x < HEAD_NC; ++x) acc[x] = fmaf(ds, qq[u][x] * kk[u][x], acc[x]);
  }
}

// lane group (cu, h): chunk cu of the list's chunks, counted type by type -> one partial [C] at part[cu, h]
template <int VEC>
__global__ void __launch_bounds__(HEAD_THREADS) k_exph_type_partial(const XTArgs A) {
  const int ul = threadIdx.x / A.G;
  const int lg = threadIdx.x - ul * A.G;
  const int64_t units = A.max_chunks * A.Hd;
  for (int64_t u = (int64_t)blockIdx.x * A.UPB + ul; u < units; u += (int64_t)gridDim.x * A.UPB) {
    const int64_t cu = u / A.Hd;
    const int h = (int)(u - cu * A.Hd);
    int tau = -1, cs = 0, ct = 0;
    int64_t base = 0;
    for (int x = 0; x < A.T; ++x) {                       // T <= 10: which type owns chunk cu
      int s, e;
      type_range(A, x, s, e);
      const int nc = type_chunks(e - s);
      if (cu < base + nc) {
        tau = x;
        cs = nc == 1 ? s : s + (int)(cu - base) * EXPH_TYPE_CHUNK;
        ct = nc == 1 ? e : (cs + EXPH_TYPE_CHUNK < e ? cs + EXPH_TYPE_CHUNK : e);
        break;
      }
      base += nc;
    }
    if (tau < 0) continue;                                // past the last chunk of the last type
    const size_t hoff = (size_t)h * A.C;
    float ee[HEAD_NC], acc[HEAD_NC];
    rw_load_cols<VEC>(A.G, A.NP, A.C, A.e_type + (size_t)tau * A.HC + hoff, lg, ee);
#pragma unroll
    for (int i = 0; i < HEAD_NC; ++i) acc[i] = 0.f;
    int p = cs;
    for (; p + XA_AHEAD <= ct; p += XA_AHEAD) type_batch<VEC, XA_AHEAD>(A, h, lg, p, ee, acc);
    for (; p < ct; ++p) type_batch<VEC, 1>(A, h, lg, p, ee, acc);
    rw_store_cols<VEC>(A.G, A.NP, A.C, A.part + (size_t)cu * A.HC + hoff, lg, acc);
  }
}

// lane group (tau, h): the type's partials added in chunk order, from zero
template <int VEC>
__global__ void __launch_bounds__(HEAD_THREADS) k_exph_type_combine(const XTArgs A) {
  const int ul = threadIdx.x / A.G;
  const int lg = threadIdx.x - ul * A.G;
  const int64_t units = (int64_t)A.T * A.Hd;
  for (int64_t u = (int64_t)blockIdx.x * A.UPB + ul; u < units; u += (int64_t)gridDim.x * A.UPB) {
    const int tau = (int)(u / A.Hd);
    const int h = (int)(u - (int64_t)tau * A.Hd);
    int64_t base = 0;
    int nc = 0;
    for (int x = 0; x <= tau; ++x) {
      int s, e;
      type_range(A, x, s, e);
      base += nc;
      nc = type_chunks(e - s);
    }
    if (base + nc > A.max_chunks) {
      atomicOr(A.flag, 2);
      nc = 0;
    }
    const size_t hoff = (size_t)h * A.C;
    float tot[HEAD_NC];
#pragma unroll
    for (int i = 0; i < HEAD_NC; ++i) tot[i] = 0.f;
    int c = 0;
    for (; c + 16 <= nc; c += 16) {                       // sixteen partials in flight, added in chunk order
      float pp[16][HEAD_NC];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        rw_load_cols<VEC>(A.G, A.NP, A.C, A.part + (size_t)(base + c + u) * A.HC + hoff, lg, pp[u]);
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int i = 0; i < HEAD_NC; ++i) tot[i] += pp[u][i];
    }
    for (; c < nc; ++c) {
      float pp[HEAD_NC];
      rw_load_cols<VEC>(A.G, A.NP, A.C, A.part + (size_t)(base + c) * A.HC + hoff, lg, pp);
#pragma unroll
      for (int i = 0; i < HEAD_NC; ++i) tot[i] += pp[i];
    }
    rw_store_cols<VEC>(A.G, A.NP, A.C, A.de_type + (size_t)tau * A.HC + hoff, lg, tot);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
template <int MODE>
int launch_walk(XAArgs A, hipStream_t st) {
  const int VEC = lane_layout(A.C, {A.q, A.k, A.v, A.e_edge, A.e_type, A.go, A.out, A.g0, A.g1}, A.G, A.UPB, A.NP);
  const unsigned nb = capped_grid(A.rows * A.Hd, A.UPB, 16384);
  dispatch_vec(VEC, [&](auto v) { k_exph_attn<decltype(v)::value, MODE><<<nb, HEAD_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int check_common(int64_t N, int64_t E, int64_t El, int T, int heads, int head_dim) {
  if (!check_csr_sizes({N, E, El}) || heads < 1 || head_dim < 1 || T < 1) return HSCN_E_BADARG;
  if (El + T > INT32_MAX) return HSCN_E_BADARG;
  if (!head_walk_supported(heads, head_dim) || T > XA_MAX_TYPES) return HSCN_E_UNSUPPORTED;
  return 0;
}

void set_shape(XAArgs& A, int64_t N, int64_t E, int64_t El, int T, int heads, int head_dim) {
  A.rows = N, A.E = E, A.El = El, A.T = T;
  A.Hd = heads, A.C = head_dim, A.HC = heads * head_dim;
  A.scale = head_scale(head_dim);
}

int64_t type_max_chunks(int64_t E, int T) { return E / EXPH_TYPE_CHUNK + T; }

}  // namespace

extern "C" {

int hscn_exph_attn_supported(int heads, int head_dim) { return head_walk_supported(heads, head_dim) ? 1 : 0; }
int hscn_exph_attn_long_row(void) { return ROW_WALK_LONG_ROW; }
int hscn_exph_attn_chunk(void) { return ROW_WALK_CHUNK; }
int hscn_exph_type_long_row(void) { return EXPH_TYPE_LONG_ROW; }
int hscn_exph_type_chunk(void) { return EXPH_TYPE_CHUNK; }
int hscn_exph_max_types(void) { return XA_MAX_TYPES; }

int hscn_exph_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* erow,
                       const float* q, const float* k, const float* v, const float* e_edge, const float* e_type,
                       float* out, float* z, int64_t N, int64_t E, int64_t El, int T, int heads, int head_dim,
                       int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, El, T, heads, head_dim)) return rc;
  if (!rowptr || !flag || !e_type || (N > 0 && (!q || !out || !z))) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !erow || !k || !v)) return HSCN_E_BADARG;
  if (El > 0 && !e_edge) return HSCN_E_BADARG;
  if (N == 0) return 0;
  XAArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.erow = erow;
  A.q = q, A.k = k, A.v = v, A.e_edge = El > 0 ? e_edge : nullptr, A.e_type = e_type;
  A.out = out, A.z = z, A.flag = flag;
  set_shape(A, N, E, El, T, heads, head_dim);
  return launch_walk<0>(A, hscn_stream(stream_));
}

int hscn_exph_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* erow,
                           const float* q, const float* k, const float* v, const float* e_edge, const float* e_type,
                           const float* out, const float* z, const float* g_out, float* delta, float* dq,
                           float* de_edge, int64_t N, int64_t E, int64_t El, int T, int heads, int head_dim,
                           int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, El, T, heads, head_dim)) return rc;
  if (!rowptr || !flag || !e_type || (N > 0 && (!q || !out || !z || !g_out || !delta))) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !erow || !k || !v)) return HSCN_E_BADARG;
  if (El > 0 && !e_edge) return HSCN_E_BADARG;
  if (N == 0) return 0;
  XAArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.erow = erow;
  A.q = q, A.k = k, A.v = v, A.e_edge = El > 0 ? e_edge : nullptr, A.e_type = e_type, A.go = g_out;
  A.out = const_cast<float*>(out), A.z = const_cast<float*>(z), A.delta = delta;
  A.g0 = dq, A.g1 = El > 0 ? de_edge : nullptr, A.walk = (dq || A.g1) ? 1 : 0;
  A.flag = flag;
  set_shape(A, N, E, El, T, heads, head_dim);
  return launch_walk<1>(A, hscn_stream(stream_));
}

int hscn_exph_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const int32_t* erow,
                           const float* q, const float* k, const float* v, const float* e_edge, const float* e_type,
                           const float* z, const float* delta, const float* g_out, float* dk, float* dv, int64_t N,
                           int64_t E, int64_t El, int T, int heads, int head_dim, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, El, T, heads, head_dim)) return rc;
  if (!rowptr_t || !flag || !e_type || (N > 0 && (!k || !v))) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t || !erow || !q || !z || !delta || !g_out)) return HSCN_E_BADARG;
  if (El > 0 && !e_edge) return HSCN_E_BADARG;
  if (N == 0 || (!dk && !dv)) return 0;
  XAArgs A{};
  A.rowptr = rowptr_t, A.col = col_t, A.eid = eid_t, A.erow = erow;
  A.q = q, A.k = k, A.v = v, A.e_edge = El > 0 ? e_edge : nullptr, A.e_type = e_type, A.go = g_out;
  A.z = const_cast<float*>(z), A.delta = const_cast<float*>(delta);
  A.g0 = dk, A.g1 = dv, A.flag = flag;
  set_shape(A, N, E, El, T, heads, head_dim);
  return launch_walk<2>(A, hscn_stream(stream_));
}

size_t hscn_exph_type_workspace_bytes(int64_t E, int T, int heads, int head_dim) {
  if (E < 0 || T < 1 || heads < 1 || head_dim < 1) return 0;
  return (size_t)type_max_chunks(E, T) * (size_t)heads * (size_t)head_dim * sizeof(float);
}

int hscn_exph_attn_bwd_type(const int32_t* trowptr, const int32_t* titem, const int64_t* edge_index, const float* q,
                            const float* k, const float* v, const float* e_type, const float* z, const float* delta,
                            const float* g_out, float* de_type, int64_t N, int64_t E, int T, int heads, int head_dim,
                            int32_t* flag, void* workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = check_common(N, E, 0, T, heads, head_dim)) return rc;
  if (!trowptr || !flag || !e_type || !de_type || !workspace) return HSCN_E_BADARG;
  if (E > 0 && (!titem || !edge_index || !q || !k || !v || !z || !delta || !g_out)) return HSCN_E_BADARG;
  if (workspace_bytes < hscn_exph_type_workspace_bytes(E, T, heads, head_dim)) return HSCN_E_WORKSPACE;
  XTArgs A{};
  A.trowptr = trowptr, A.titem = titem, A.src = edge_index, A.dst = edge_index ? edge_index + E : nullptr;
  A.q = q, A.k = k, A.v = v, A.e_type = e_type, A.go = g_out, A.z = z, A.delta = delta;
  A.part = static_cast<float*>(workspace), A.de_type = de_type;
  A.N = N, A.E = E, A.max_chunks = type_max_chunks(E, T);
  A.T = T, A.Hd = heads, A.C = head_dim, A.HC = heads * head_dim;
  A.scale = head_scale(head_dim);
  A.flag = flag;
  const int VEC = lane_layout(A.C, {A.q, A.k, A.v, A.e_type, A.go, A.part, A.de_type}, A.G, A.UPB, A.NP);
  hipStream_t st = hscn_stream(stream_);
  const unsigned nb = capped_grid(A.max_chunks * A.Hd, A.UPB, 16384);
  dispatch_vec(VEC, [&](auto v) { k_exph_type_partial<decltype(v)::value><<<nb, HEAD_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  const unsigned nc = capped_grid((int64_t)T * A.Hd, A.UPB, 16384);
  dispatch_vec(VEC, [&](auto v) { k_exph_type_combine<decltype(v)::value><<<nc, HEAD_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
