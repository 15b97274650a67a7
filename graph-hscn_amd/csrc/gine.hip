// GINEConv's aggregate (PyG GINEConv, edge_dim given): the edge-aware gather-reduce of the MPNN baseline's "gine".
//
//   t_k = lin.bias + lin.weight e_k                      e_k = edge_attr[k], lin: [F, De]
//   z_i = (1 + eps) x_i + sum_{k: dst_k = i} relu(x[src_k] + t_k)
//
// lin(edge_attr) is evaluated INSIDE the gather: De is small, so the [E, F] message matrix is never written by the
// forward, and the backward recomputes each gate from x and edge_attr with the same device function (edge_lin), so a
// gate is the same bit in all three kernels.  Conventions of csrc/spmm.hip: a row is owned by LPR consecutive lanes,
// VEC = 4 (16-byte accesses) where F % 4 == 0 and a scalar path otherwise, accumulation in CSR slot order with
// separately rounded multiply and add.  A lane group covers at most 64 * VEC columns at a time; wider rows take further
// column passes over the same slots.
//
// One kernel, two directions (k_gine_walk<.., MODE>):
//   MODE 0, target-keyed CSR:  out_i = (1+eps) x_i  + sum_slots relu(x[col] + t_eid)               (forward, z)
//   MODE 1, source-keyed CSR:  out_j = (1+eps) gz_j + sum_slots [x_j + t_eid > 0] gz[col]          (backward, gx)
//
// Long rows: the two-phase scheme described in csrc/row_walk.h; the chunk partials are added in chunk order with a
// separately rounded add.
//
// The parameter gradients go through one [E, F] buffer written once with plain stores (k_gine_msg_grad, edge-parallel,
// gm_k = gate_k * gz[dst_k]) and the existing two-stage ordered hscn_linear_bwd_w(gm, edge_attr): no float atomics.
#include "row_walk.h"

namespace {

constexpr int GI_THREADS = 256;
constexpr int GINE_MAX_F = 512;
constexpr int GINE_MAX_DE = 64;

// The lane's VEC rows of lin.weight and lin.bias.  DREG > 0: De <= DREG, the rows live in registers (columns past De
// are zero and meet a zero edge feature).  DREG == 0: any De, the rows are read through the cache per edge.
template <int VEC, int DREG>
struct EdgeLin {
  float w[VEC][DREG > 0 ? DREG : 1];
  float b[VEC];
  const float* Wrow;
  int De;
  __device__ __forceinline__ void init(const float* __restrict__ W, const float* __restrict__ bias, int f, int De_) {
    De = De_;
    Wrow = W + (size_t)f * De_;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      b[v] = bias[f + v];
      if (DREG > 0) {
#pragma unroll
        for (int d = 0; d < DREG; ++d) w[v][d] = d < De_ ? Wrow[v * De_ + d] : 0.f;
      }
    }
  }
  // t[v] = b[v] + sum_d w[v][d] e[d], d ascending, separately rounded: the one evaluation every kernel here shares
  __device__ __forceinline__ void eval(const float* __restrict__ e, float (&t)[VEC]) const {
#pragma unroll
    for (int v = 0; v < VEC; ++v) t[v] = b[v];
    if (DREG > 0) {
#pragma unroll
      for (int d = 0; d < DREG; ++d) {
        const float ev = d < De ? e[d] : 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = add_rn(t[v], mul_rn(w[v][d], ev));
      }
    } else {
      for (int d = 0; d < De; ++d) {
        const float ev = e[d];
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = add_rn(t[v], mul_rn(Wrow[v * De + d], ev));
      }
    }
  }
};

struct GineArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const float* x;      // [N, F] node features
  const float* ea;     // [E, De]
  const float* W;      // [F, De]
  const float* bias;   // [F]
  const float* g;      // MODE 1: gz [N, F]
  float* out;          // [N, F]
  int64_t N, E;
  int F, De, LPR, RPB;
  float scale;         // 1 + eps
  int32_t* flag;
};

// slots [s, t) of one row, columns [f, f + VEC): the running sum continued from `acc`
template <int VEC, int DREG, int MODE>
__device__ __forceinline__ typename GV<VEC>::T walk_slots(const GineArgs& A, const EdgeLin<VEC, DREG>& L, int s, int t,
                                                          int f, typename GV<VEC>::T xr, typename GV<VEC>::T acc) {
  using V = GV<VEC>;
  const float* G = MODE == 0 ? A.x : A.g;
  float a[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) a[v] = V::get(acc, v);
#pragma unroll 2
  for (int p = s; p < t; ++p) {
    const int j = A.col[p];
    const int k = A.eid[p];
    if (j < 0 || j >= A.N || k < 0 || k >= A.E) {       // never produced by hscn_csr_build; a foreign CSR is flagged
      atomicOr(A.flag, 2);
      continue;
    }
    const typename V::T gj = V::load(G + (size_t)j * A.F + f);
    float tk[VEC];
    L.eval(A.ea + (size_t)k * A.De, tk);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float m;
      if (MODE == 0) {
        const float pre = add_rn(V::get(gj, v), tk[v]);
        m = pre > 0.f ? pre : 0.f;
      } else {
        const float pre = add_rn(V::get(xr, v), tk[v]);
        m = pre > 0.f ? V::get(gj, v) : 0.f;
      }
      a[v] = add_rn(a[v], m);
    }
  }
  return V::make(a);
}

template <int VEC>
__device__ __forceinline__ void finish_row(const GineArgs& A, int MODE, int64_t r, int f, typename GV<VEC>::T acc) {
  using V = GV<VEC>;
  const typename V::T self = V::load((MODE == 0 ? A.x : A.g) + (size_t)r * A.F + f);
  float o[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) o[v] = add_rn(V::get(acc, v), mul_rn(A.scale, V::get(self, v)));
  V::store(A.out + (size_t)r * A.F + f, V::make(o));
}

template <int VEC, int DREG, int MODE>
__global__ void __launch_bounds__(GI_THREADS) k_gine_walk(const GineArgs A) {
  using V = GV<VEC>;
  __shared__ __attribute__((aligned(16))) float part[GI_THREADS * VEC];
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  const bool member = rl < A.RPB;                       // (256 % LPR lanes at the end of the block own no row)
  const int span = A.LPR * VEC;                         // columns of one pass
  const int64_t tiles = (A.N + A.RPB - 1) / A.RPB;
  int any_long = 0;
  // ---- rows of at most ROW_WALK_LONG_ROW slots: one lane group each, serially --------------------------------------
  if (member) {
    for (int f = lg * VEC; f < A.F; f += span) {        // (one pass up to 64 * VEC columns)
      EdgeLin<VEC, DREG> L;
      L.init(A.W, A.bias, f, A.De);
      for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * A.RPB + rl;
        if (r >= A.N) continue;
        const int s = A.rowptr[r], t = A.rowptr[r + 1];
        if (t - s > ROW_WALK_LONG_ROW) { any_long = 1; continue; }
        typename V::T xr = V::zero();
        if (MODE == 1) xr = V::load(A.x + (size_t)r * A.F + f);
        finish_row<VEC>(A, MODE, r, f, walk_slots<VEC, DREG, MODE>(A, L, s, t, f, xr, V::zero()));
      }
    }
  }
  if (!__syncthreads_or(any_long)) return;
  // ---- the long rows among this block's tiles: the whole block per row, chunk partials added in chunk order ------
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
        EdgeLin<VEC, DREG> L;
        typename V::T xr = V::zero();
        if (live) {
          L.init(A.W, A.bias, f, A.De);
          if (MODE == 1) xr = V::load(A.x + (size_t)r * A.F + f);
        }
        typename V::T total = V::zero();
        for (int c0 = 0; c0 < chunks; c0 += A.RPB) {
          const int c = c0 + rl;
          if (live && c < chunks) {
            const int cs = s + c * ROW_WALK_CHUNK;
            const int ct = cs + ROW_WALK_CHUNK < t ? cs + ROW_WALK_CHUNK : t;
            V::store(part + (size_t)threadIdx.x * VEC, walk_slots<VEC, DREG, MODE>(A, L, cs, ct, f, xr, V::zero()));
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
        if (live && rl == 0) finish_row<VEC>(A, MODE, r, f, total);
      }
    }
  }
}

// gm[k, :] = [x[src_k] + t_k > 0] * gz[dst_k], one lane group per edge of the edge list as given; an edge with a node
// id outside [0, N) -- the CSR build skipped it and raised the flag -- contributes a zero row
template <int VEC, int DREG>
__global__ void __launch_bounds__(GI_THREADS)
k_gine_msg_grad(const int64_t* __restrict__ ei, const float* __restrict__ x, const float* __restrict__ ea,
                const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ gz,
                float* __restrict__ gm, int64_t N, int64_t E, int F, int De, int LPR, int RPB, int32_t* flag) {
  using V = GV<VEC>;
  const int rl = threadIdx.x / LPR;
  const int lg = threadIdx.x - rl * LPR;
  if (rl >= RPB) return;
  const int span = LPR * VEC;
  for (int f = lg * VEC; f < F; f += span) {
    EdgeLin<VEC, DREG> L;
    L.init(W, bias, f, De);
    for (int64_t k = (int64_t)blockIdx.x * RPB + rl; k < E; k += (int64_t)gridDim.x * RPB) {
      const int64_t src = ei[k], dst = ei[E + k];
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = 0.f;
      if (src < 0 || src >= N || dst < 0 || dst >= N) {
        atomicOr(flag, 1);
      } else {
        const typename V::T xs = V::load(x + (size_t)src * F + f);
        const typename V::T gd = V::load(gz + (size_t)dst * F + f);
        float tk[VEC];
        L.eval(ea + (size_t)k * De, tk);
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = add_rn(V::get(xs, v), tk[v]) > 0.f ? V::get(gd, v) : 0.f;
      }
      V::store(gm + (size_t)k * F + f, V::make(o));
    }
  }
}

bool gine_supported(int F, int De) { return F >= 1 && F <= GINE_MAX_F && De >= 1 && De <= GINE_MAX_DE; }

// f(VEC, DREG) as integral constants: 16-byte lanes where F allows, lin's rows in 4 or 8 registers where De allows
template <class Fn>
void dispatch_vec_dreg(int VEC, int De, Fn&& f) {
  dispatch_vec(VEC, [&](auto v) {
    if (De <= 4) f(v, std::integral_constant<int, 4>{});
    else if (De <= 8) f(v, std::integral_constant<int, 8>{});
    else f(v, std::integral_constant<int, 0>{});
  });
}

template <int MODE>
int launch_walk(GineArgs A, hipStream_t st) {
  int VEC;
  lane_groups(A.F, GI_THREADS, VEC, A.LPR, A.RPB);
  const unsigned nb = capped_grid(A.N, A.RPB, 8192);
  dispatch_vec_dreg(VEC, A.De, [&](auto v, auto d) {
    k_gine_walk<decltype(v)::value, decltype(d)::value, MODE><<<nb, GI_THREADS, 0, st>>>(A);
  });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int check_common(int64_t N, int64_t E, int F, int De) {
  if (!check_csr_sizes({N, E}) || F < 1 || De < 1) return HSCN_E_BADARG;
  if (!gine_supported(F, De)) return HSCN_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int hscn_gine_supported(int F, int De) { return gine_supported(F, De) ? 1 : 0; }
int hscn_gine_long_row(void) { return ROW_WALK_LONG_ROW; }
int hscn_gine_chunk(void) { return ROW_WALK_CHUNK; }

int hscn_gine_aggregate_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* x,
                            const float* edge_attr, const float* W, const float* bias, float eps, float* z, int64_t N,
                            int64_t E, int F, int De, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, F, De)) return rc;
  if (N == 0) return 0;
  if (!rowptr || !x || !W || !bias || !z || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col || !eid || !edge_attr)) return HSCN_E_BADARG;
  GineArgs A{rowptr, col, eid, x, edge_attr, W, bias, nullptr, z, N, E, F, De, 0, 0, 1.0f + eps, flag};
  return launch_walk<0>(A, hscn_stream(stream_));
}

int hscn_gine_aggregate_bwd_x(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* x,
                              const float* edge_attr, const float* W, const float* bias, float eps, const float* gz,
                              float* gx, int64_t N, int64_t E, int F, int De, int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, F, De)) return rc;
  if (N == 0) return 0;
  if (!rowptr_t || !x || !W || !bias || !gz || !gx || !flag) return HSCN_E_BADARG;
  if (E > 0 && (!col_t || !eid_t || !edge_attr)) return HSCN_E_BADARG;
  GineArgs A{rowptr_t, col_t, eid_t, x, edge_attr, W, bias, gz, gx, N, E, F, De, 0, 0, 1.0f + eps, flag};
  return launch_walk<1>(A, hscn_stream(stream_));
}

int hscn_gine_aggregate_bwd_msg(const int64_t* edge_index, const float* x, const float* edge_attr, const float* W,
                                const float* bias, const float* gz, float* gm, int64_t N, int64_t E, int F, int De,
                                int32_t* flag, void* stream_) {
  if (int rc = check_common(N, E, F, De)) return rc;
  if (E == 0) return 0;
  if (!edge_index || !x || !edge_attr || !W || !bias || !gz || !gm || !flag) return HSCN_E_BADARG;
  int VEC, LPR, RPB;
  lane_groups(F, GI_THREADS, VEC, LPR, RPB);
  const unsigned nb = capped_grid(E, RPB, 8192);
  hipStream_t st = hscn_stream(stream_);
  dispatch_vec_dreg(VEC, De, [&](auto v, auto d) {
    k_gine_msg_grad<decltype(v)::value, decltype(d)::value><<<nb, GI_THREADS, 0, st>>>(
        edge_index, x, edge_attr, W, bias, gz, gm, N, E, F, De, LPR, RPB, flag);
  });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
