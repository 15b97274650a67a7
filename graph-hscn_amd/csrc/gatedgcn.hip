// GatedGCN's aggregate (GraphGPS GatedGCNLayer; Bresson & Laurent, residual gated graph ConvNets): the edge-gated
// gather-reduce in which edge features are a state -- every layer reads them, writes new ones and needs their gradient.
//
//   e^_k  = Dx_i + Ex_j + Ce_k            j = src_k, i = dst_k          [E, H]  the new edge features (pre-norm)
//   s_k   = sigmoid(e^_k)                                               H gates per edge
//   num_i = sum_{k: dst_k = i} s_k * Bx_j       den_i = sum_{k: dst_k = i} s_k
//   h_i   = Ax_i + num_i / (den_i + 1e-6)                               [N, H]
//
// The five inputs are already transformed (the dense A..E run through hscn_linear_*).  Row k of Ce / e^ / ge belongs
// to edge k of the edge list, not to CSR slot k: every slot goes through eid[slot].  Conventions of csrc/spmm.hip and
// csrc/gine.hip: a row is owned by LPR consecutive lanes, VEC = 4 (16-byte accesses) where H % 4 == 0 and a scalar
// path otherwise, accumulation in CSR slot order with separately rounded multiply and add; a lane group covers at most
// 64 * VEC columns at a time, wider rows take further column passes over the same slots.  The sigmoid is
// 1 / (1 + expf(-x)) with the library's expf and a correctly rounded division.
//
// One kernel, three walks (k_gated_walk<VEC, MODE>), each with two running sums per row:
//   MODE 0, target-keyed CSR (forward):   num_i, den_i;  stores e^[eid], den_i, h_i
//   MODE 1, target-keyed CSR (backward):  gn_i = gh_i / (den_i + 1e-6), gd_i = -gn_i (h_i - Ax_i);
//                                         ge_k = ge^_k + (gn_i Bx_j + gd_i) s_k (1 - s_k)   stored once at eid (= gCe)
//                                         gDx_i = sum ge_k;  stores gn_i for the source walk
//   MODE 2, source-keyed CSR (backward):  gBx_j = sum_{k: src_k = j} s_k gn_i,   gEx_j = sum ge_k
// s_k is recomputed from the saved e^ (an output, kept anyway) by the same device function in all three.  No float
// atomics: every output row has one owner.
//
// Long rows: the two-phase scheme described in csrc/row_walk.h; both running sums of a chunk are parked, and added in
// chunk order with a separately rounded add.
//
// Edges that hscn_csr_build left out (an endpoint outside [0, N): the flag word is non-zero) own no slot; when the flag
// word is set, MODE 0 / MODE 1 sweep the edge list once and store a zero row of e^ / ge for each of them.
#include "row_walk.h"

namespace {

constexpr int GG_THREADS = 256;
constexpr int GATED_MAX_H = 512;
constexpr float GATED_EPS = 1e-6f;

// the one gate evaluation all three walks share
__device__ __forceinline__ float gate(float x) { return 1.0f / (1.0f + expf(-x)); }

struct GatedArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const int64_t* ei;   // [2, E] edge list (MODE 0 / 1: the sweep for left-out edges)
  const float* Ax;     // [N, H]   MODE 0, 1
  const float* Bx;     // [N, H]   MODE 0, 1
  const float* Dx;     // [N, H]   MODE 0
  const float* Ex;     // [N, H]   MODE 0
  const float* Ce;     // [E, H]   MODE 0
  const float* gh;     // [N, H]   MODE 1
  const float* gein;   // [E, H]   MODE 1: cotangent of e^, or NULL
  float* h;            // [N, H]   MODE 0 out, MODE 1 in
  float* eo;           // [E, H]   MODE 0 out, MODE 1 / 2 in (e^)
  float* den;          // [N, H]   MODE 0 out, MODE 1 in
  float* gn;           // [N, H]   MODE 1 out, MODE 2 in
  float* ge;           // [E, H]   MODE 1 out, MODE 2 in
  float* o0;           // [N, H]   MODE 1: gDx;  MODE 2: gBx (or NULL)
  float* o1;           // [N, H]   MODE 2: gEx (or NULL)
  int64_t N, E;
  int H, LPR, RPB;
  int walk;            // MODE 1: 0 = gn alone, every row taken as empty (only Bx asks for a gradient)
  int32_t* flag;
};

// what a lane keeps of its row while it walks the slots
template <int VEC>
struct RowCtx {
  float a[VEC];   // MODE 0: Dx_i;  MODE 1: gn_i
  float b[VEC];   // MODE 1: gd_i
};

template <int VEC, int MODE>
__device__ __forceinline__ void row_begin(const GatedArgs& A, int64_t r, int f, RowCtx<VEC>& R) {
  using V = GV<VEC>;
  const size_t at = (size_t)r * A.H + f;
  if (MODE == 0) {
    const typename V::T d = V::load(A.Dx + at);
#pragma unroll
    for (int v = 0; v < VEC; ++v) R.a[v] = V::get(d, v);
  } else if (MODE == 1) {
    const typename V::T g = V::load(A.gh + at), dn = V::load(A.den + at), hh = V::load(A.h + at), ax = V::load(A.Ax + at);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      R.a[v] = V::get(g, v) / add_rn(V::get(dn, v), GATED_EPS);
      R.b[v] = -mul_rn(R.a[v], add_rn(V::get(hh, v), -V::get(ax, v)));
    }
  }
}

// slots [s, t) of one row, columns [f, f + VEC): the two running sums continued from acc0 / acc1
template <int VEC, int MODE>
__device__ __forceinline__ void walk_slots(const GatedArgs& A, const RowCtx<VEC>& R, int s, int t, int f,
                                           float (&acc0)[VEC], float (&acc1)[VEC]) {
  using V = GV<VEC>;
#pragma unroll 2
  for (int p = s; p < t; ++p) {
    const int j = A.col[p];
    const int k = A.eid[p];
    if (j < 0 || j >= A.N || k < 0 || k >= A.E) {       // never produced by hscn_csr_build; a foreign CSR is flagged
      atomicOr(A.flag, 2);
      continue;
    }
    const size_t nj = (size_t)j * A.H + f, ek = (size_t)k * A.H + f;
    if (MODE == 0) {
      const typename V::T ex = V::load(A.Ex + nj), bx = V::load(A.Bx + nj), ce = V::load(A.Ce + ek);
      float e[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        e[v] = add_rn(add_rn(R.a[v], V::get(ex, v)), V::get(ce, v));
        const float sg = gate(e[v]);
        acc0[v] = add_rn(acc0[v], mul_rn(sg, V::get(bx, v)));
        acc1[v] = add_rn(acc1[v], sg);
      }
      V::store(A.eo + ek, V::make(e));
    } else if (MODE == 1) {
      const typename V::T bx = V::load(A.Bx + nj), eh = V::load(A.eo + ek);
      typename V::T gi = V::zero();
      if (A.gein) gi = V::load(A.gein + ek);
      float g[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float sg = gate(V::get(eh, v));
        const float ds = mul_rn(sg, add_rn(1.0f, -sg));
        g[v] = mul_rn(add_rn(mul_rn(R.a[v], V::get(bx, v)), R.b[v]), ds);
        if (A.gein) g[v] = add_rn(V::get(gi, v), g[v]);
        acc0[v] = add_rn(acc0[v], g[v]);
      }
      V::store(A.ge + ek, V::make(g));
    } else {
      if (A.o0) {
        const typename V::T eh = V::load(A.eo + ek), gn = V::load(A.gn + nj);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc0[v] = add_rn(acc0[v], mul_rn(gate(V::get(eh, v)), V::get(gn, v)));
      }
      if (A.o1) {
        const typename V::T g = V::load(A.ge + ek);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc1[v] = add_rn(acc1[v], V::get(g, v));
      }
    }
  }
}

template <int VEC, int MODE>
__device__ __forceinline__ void finish_row(const GatedArgs& A, const RowCtx<VEC>& R, int64_t r, int f,
                                           const float (&acc0)[VEC], const float (&acc1)[VEC]) {
  using V = GV<VEC>;
  const size_t at = (size_t)r * A.H + f;
  if (MODE == 0) {
    const typename V::T ax = V::load(A.Ax + at);
    float o[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) o[v] = add_rn(V::get(ax, v), acc0[v] / add_rn(acc1[v], GATED_EPS));
    V::store(A.h + at, V::make(o));
    V::store(A.den + at, V::make(acc1));
  } else if (MODE == 1) {
    V::store(A.gn + at, V::make(R.a));
    if (A.o0) V::store(A.o0 + at, V::make(acc0));
  } else {
    if (A.o0) V::store(A.o0 + at, V::make(acc0));
    if (A.o1) V::store(A.o1 + at, V::make(acc1));
  }
}

template <int VEC, int MODE>
__global__ void __launch_bounds__(GG_THREADS) k_gated_walk(const GatedArgs A) {
  using V = GV<VEC>;
  __shared__ __attribute__((aligned(16))) float part[2 * GG_THREADS * VEC];
  // ---- edges the CSR build left out own no slot: a zero row of e^ (MODE 0) / ge (MODE 1) each --------------------
  if (MODE != 2) {
    float* rows = MODE == 0 ? A.eo : A.ge;
    if ((MODE == 0 || A.walk) && A.E > 0 && *A.flag != 0) {
      for (int64_t k = (int64_t)blockIdx.x * GG_THREADS + threadIdx.x; k < A.E; k += (int64_t)gridDim.x * GG_THREADS) {
        const int64_t src = A.ei[k], dst = A.ei[A.E + k];
        if (src < 0 || src >= A.N || dst < 0 || dst >= A.N)
          for (int f = 0; f < A.H; ++f) rows[(size_t)k * A.H + f] = 0.f;
      }
    }
  }
  const bool walk = MODE != 1 || A.walk != 0;
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  const bool member = rl < A.RPB;                       // (256 % LPR lanes at the end of the block own no row)
  const int span = A.LPR * VEC;                         // columns of one pass
  const int64_t tiles = (A.N + A.RPB - 1) / A.RPB;
  int any_long = 0;
  // ---- rows of at most ROW_WALK_LONG_ROW slots: one lane group each, serially --------------------------------------
  if (member) {
    for (int f = lg * VEC; f < A.H; f += span) {        // (one pass up to 64 * VEC columns)
      for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * A.RPB + rl;
        if (r >= A.N) continue;
        const int s = A.rowptr[r], t = walk ? A.rowptr[r + 1] : s;
        if (t - s > ROW_WALK_LONG_ROW) { any_long = 1; continue; }
        RowCtx<VEC> R;
        row_begin<VEC, MODE>(A, r, f, R);
        float acc0[VEC], acc1[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc0[v] = acc1[v] = 0.f;
        walk_slots<VEC, MODE>(A, R, s, t, f, acc0, acc1);
        finish_row<VEC, MODE>(A, R, r, f, acc0, acc1);
      }
    }
  }
  if (!__syncthreads_or(any_long)) return;
  // ---- the long rows among this block's tiles: the whole block per row, chunk partials added in chunk order ------
  float* part0 = part;
  float* part1 = part + GG_THREADS * VEC;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int i = 0; i < A.RPB; ++i) {
      const int64_t r = tile * A.RPB + i;
      if (r >= A.N) break;
      const int s = A.rowptr[r], t = A.rowptr[r + 1];   // block-uniform
      if (t - s <= ROW_WALK_LONG_ROW) continue;
      const int chunks = (t - s + ROW_WALK_CHUNK - 1) / ROW_WALK_CHUNK;
      for (int f0 = 0; f0 < A.H; f0 += span) {
        const int f = f0 + lg * VEC;
        const bool live = member && f < A.H;
        RowCtx<VEC> R;
        if (live) row_begin<VEC, MODE>(A, r, f, R);
        float tot0[VEC], tot1[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) tot0[v] = tot1[v] = 0.f;
        for (int c0 = 0; c0 < chunks; c0 += A.RPB) {
          const int c = c0 + rl;
          if (live && c < chunks) {
            const int cs = s + c * ROW_WALK_CHUNK;
            const int ct = cs + ROW_WALK_CHUNK < t ? cs + ROW_WALK_CHUNK : t;
            float acc0[VEC], acc1[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc0[v] = acc1[v] = 0.f;
            walk_slots<VEC, MODE>(A, R, cs, ct, f, acc0, acc1);
            V::store(part0 + (size_t)threadIdx.x * VEC, V::make(acc0));
            V::store(part1 + (size_t)threadIdx.x * VEC, V::make(acc1));
          }
          __syncthreads();
          if (live && rl == 0) {
            const int n = chunks - c0 < A.RPB ? chunks - c0 : A.RPB;
            for (int q = 0; q < n; ++q) {
              const typename V::T p0 = V::load(part0 + (size_t)(q * A.LPR + lg) * VEC);
              const typename V::T p1 = V::load(part1 + (size_t)(q * A.LPR + lg) * VEC);
#pragma unroll
              for (int v = 0; v < VEC; ++v) {
                tot0[v] = add_rn(tot0[v], V::get(p0, v));
                tot1[v] = add_rn(tot1[v], V::get(p1, v));
              }
            }
          }
          __syncthreads();
        }
        if (live && rl == 0) finish_row<VEC, MODE>(A, R, r, f, tot0, tot1);
      }
    }
  }
}

bool gated_supported(int H) { return H >= 1 && H <= GATED_MAX_H; }

template <int MODE>
int launch_walk(GatedArgs A, hipStream_t st) {
  int VEC;
  lane_groups(A.H, GG_THREADS, VEC, A.LPR, A.RPB);
  const unsigned nb = capped_grid(A.N, A.RPB, 8192);
  dispatch_vec(VEC, [&](auto v) { k_gated_walk<decltype(v)::value, MODE><<<nb, GG_THREADS, 0, st>>>(A); });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int check_common(int64_t N, int64_t E, int H) {
  if (!check_csr_sizes({N, E}) || H < 1) return HSCN_E_BADARG;
  if (!gated_supported(H)) return HSCN_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int hscn_gatedgcn_supported(int H) { return gated_supported(H) ? 1 : 0; }
int hscn_gatedgcn_long_row(void) { return ROW_WALK_LONG_ROW; }
int hscn_gatedgcn_chunk(void) { return ROW_WALK_CHUNK; }

int hscn_gatedgcn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int64_t* edge_index,
                      const float* Ax, const float* Bx, const float* Dx, const float* Ex, const float* Ce, float* h,
                      float* e_out, float* den, int64_t N, int64_t E, int H, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, H)) return rc;
  if (N == 0) return 0;
  if (!rowptr || !Ax || !Bx || !Dx || !Ex || !h || !den || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !edge_index || !Ce || !e_out)) return HSCN_E_BADARG;
  GatedArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.ei = edge_index;
  A.Ax = Ax, A.Bx = Bx, A.Dx = Dx, A.Ex = Ex, A.Ce = Ce;
  A.h = h, A.eo = e_out, A.den = den;
  A.N = N, A.E = E, A.H = H, A.flag = flag;
  return launch_walk<0>(A, hscn_stream(stream_));
}

int hscn_gatedgcn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int64_t* edge_index,
                          const float* Ax, const float* Bx, const float* h, const float* e_out, const float* den,
                          const float* gh, const float* g_e_out, float* gn, float* ge, float* gDx, int64_t N,
                          int64_t E, int H, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, H)) return rc;
  if (N == 0) return 0;
  if (!rowptr || !Ax || !h || !den || !gh || !gn || !flag) return HSCN_E_BADARG;
  const bool walk = ge != nullptr || gDx != nullptr;                        // the edge walk gives both or neither
  if (walk && (!gDx || (E > 0 && (!ge || !col || !eid || !edge_index || !Bx || !e_out)))) return HSCN_E_BADARG;
  GatedArgs A{};
  A.rowptr = rowptr, A.col = col, A.eid = eid, A.ei = edge_index;
  A.Ax = Ax, A.Bx = Bx, A.gh = gh, A.gein = g_e_out;
  A.h = const_cast<float*>(h), A.eo = const_cast<float*>(e_out), A.den = const_cast<float*>(den);
  A.gn = gn, A.ge = ge, A.o0 = gDx, A.walk = walk ? 1 : 0;
  A.N = N, A.E = E, A.H = H, A.flag = flag;
  return launch_walk<1>(A, hscn_stream(stream_));
}

int hscn_gatedgcn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* e_out,
                          const float* gn, const float* ge, float* gBx, float* gEx, int64_t N, int64_t E, int H,
                          int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, H)) return rc;
  if (N == 0 || (!gBx && !gEx)) return 0;
  if (!rowptr_t || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t)) return HSCN_E_BADARG;
  if (E > 0 && gBx && (!e_out || !gn)) return HSCN_E_BADARG;
  if (E > 0 && gEx && !ge) return HSCN_E_BADARG;
  GatedArgs A{};
  A.rowptr = rowptr_t, A.col = col_t, A.eid = eid_t;
  A.eo = const_cast<float*>(e_out), A.gn = const_cast<float*>(gn), A.ge = const_cast<float*>(ge);
  A.o0 = gBx, A.o1 = gEx;
  A.N = N, A.E = E, A.H = H, A.flag = flag;
  return launch_walk<2>(A, hscn_stream(stream_));
}

}  // extern "C"
