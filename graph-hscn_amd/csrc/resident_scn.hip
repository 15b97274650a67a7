// Graph-resident stage A: gcn_norm + SCN.forward + MinCUT/orthogonality losses, and the
// backward, one workgroup per graph with everything in LDS.
//
// Reference: the per-graph body of train/train_clustering.py:37-50 --
//   gcn_norm(edge_index, None, n, add_self_loops=True)                      (:37-42)
//   SCN.forward: GraphConv(F->H) + act, Linear(H->K), to_dense_adj, dense_mincut_pool
//                                                                            (model/hscn.py:56-64)
// for mp_units=[H], mlp_units=[] (the only configuration the reference instantiates,
// main.py:101-105; other shapes use the layered operators).  The reference does this with
// ~60 small tensor ops and a dense [n,n] adjacency per graph; here the self-looped,
// normalised graph never materialises:
//   * rows of the target-keyed CSR give the in-degree, deg = indeg + 1 (the added self loop),
//     w_e = deg_src^-1/2 * 1 * deg_dst^-1/2, loop weight deg_i^-1 -- applied on the fly, loop last
//     (PyG appends the loops after the edges, so edge order = CSR order then loop);
//   * MinCUT uses the BINARY A + I (model/hscn.py:61 drops the weights):
//       tr(S^T A S) = sum_i S_i . ((A S)_i + S_i),  tr(S^T D S) = sum_i (outdeg_i + 1) |S_i|^2.
// Existing self loops in the input (none in LRGB) become the unit self loop, as
// add_remaining_self_loops does for unit weights.
// Ordered reductions only; per-graph parameter-gradient partials + one ordered fold.
#include <cstdlib>
#include <type_traits>
#include "hscn_common.h"
#include "resident_common.h"

namespace {

// the wave's index in the workgroup as a SCALAR: the compiler takes threadIdx.x >> 6 for a per-lane value and turns
// every "tiles of this wave" loop into a divergent loop (exec masks, vector compares, vector addresses)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

constexpr int SRT = 1024;  // threads per workgroup (16 waves: latency hiding for the many short phases)
constexpr int FP = 16;    // input features are zero padded to 16 in LDS

struct ScnArgs {
  const float* x;              // [N,F]
  const int64_t *src, *dst;    // raw COO (no self loops needed)
  const int32_t *nptr, *eptr;  // node / edge ranges per graph
  const float *W_rel, *b_rel, *W_root, *W_mlp, *b_mlp;
  float *S, *y, *stats, *ss;   // outputs: [N,K], [N,H], [B,4], [B,K,K]
  const float *g_mc, *g_o;     // backward only: upstream scalars dL/dmincut, dL/dortho on the device (NULL = 0)
  float* partials;             // backward only: [B,P]
  // both CSRs, the normalised aggregation and the binary out-degree: built by the forward launch,
  // exported (graph g: rowptr at nptr[g] + g, columns at eptr[g]) and loaded by the backward launch
  int32_t *ex_rowptr_d, *ex_col_d, *ex_rowptr_s, *ex_col_s;
  float *ex_agg, *ex_dout;  // [N,FP], [N]
  float* ex_xpad;           // [N,FP] or NULL: the features padded to FP columns as LDS holds them (float4 loads in the cached front)
  int pre;                  // one-launch step: the ex_* arrays hold this batch's structure already (loaded, not built)
  long long visits, visit0; // k_scn_epoch: graph visits of the launch, number of the first one
  int G;                    // k_scn_epoch: graphs of the dataset (B = 1: a visit is a batch of one)
  // forward only: losses [3] = {mean mincut, mean ortho, their sum}; with a ticket counter (zero before
  // the first launch, left at zero) the workgroup that finishes last reduces the per-graph statistics
  float* losses;
  int32_t* ticket;
  int32_t* flag;
  int64_t N;
  int F, K, act, max_n, max_e, B, P;
  // one-launch step with ONE graph: the optimizer step (torch's single-tensor Adam / AdamW, csrc/optim.hip) in the
  // tail of the same launch -- the workgroup holds the whole gradient.  adam_m == NULL: no update.
  float *adam_m, *adam_v, *adam_step;
  double* adam_pows;
  const double* adam_lr;
  double adam_b1, adam_b2, adam_eps, adam_wd;
  int adam_decoupled;
};

// The kernel's argument block read LATE: the compiler loads every argument it finds loop-invariant at the top of the
// kernel and keeps it in scalar registers; fields that only the last phase needs (the optimizer's) or only the first
// (the structure cache's) then cost spills all the way through (each spill is a v_writelane / v_readlane pair on the
// VALU).  The pointer is laundered through an empty asm so their loads stay where they are used.
typedef const __attribute__((address_space(4))) ScnArgs* ScnArgsK;
__device__ __forceinline__ ScnArgsK late_args() { return late_args<ScnArgs>(0); }

// the launch a layout is for: the forward, the backward, or both in one (the one-launch step and the persistent epoch)
enum ScnMode : int { SCN_FWD = 0, SCN_BWD = 1, SCN_STEP = 2 };

struct ScnLayout {
  size_t R1, R2, R3, dinv, dout, wt, red, vecs, rowptr_d, col_d, rowptr_s, col_s, cursor, tmp, cursor2, tmp2, wsum, ek,
      eo, ssl, total;
};
// R1: x | agg  (2 * n * FP), later S (n * K) in the forward; R2: y (n * H); R3 (backward): dS / dlogits (n * K)
__host__ __device__ inline ScnLayout scn_layout(int H, int K, int max_n, int max_e, ScnMode mode) {
  const bool back = mode != SCN_FWD;   // the launch has a backward half
  ScnLayout Y;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += (n + 3) & ~(size_t)3; return r; };
  // (the partial tiles of gram_mfma, 16 waves x 256 words, reuse a buffer that is dead by then: y in the
  // forward; in the backward S, then dlogits -- all kept at least that large)
  // Backward: R1 = S, later x; R3 = dlogits, later agg.  x and agg wait in registers until the buffers
  // they take over are dead, so a Peptides graph of 444 nodes fits (x, agg AND S resident did not).
  constexpr size_t GSCR = 4096;
  const int KF = K > FP ? K : FP;
  const size_t xa = (size_t)2 * max_n * FP, sk0 = (size_t)max_n * (back ? KF : K), sk = (back && sk0 < GSCR) ? GSCR : sk0;
  const size_t sks = (size_t)max_n * K + GSCR;          // the one-launch step: S and, behind it, the tile scratch of S^T S
  // (forward launch: the per-wave S^T S tiles of scn_softmax are parked behind S as well when K <= 16)
  const size_t r1f = (xa > sk ? xa : sk), r1s = (K <= 16 || mode == SCN_STEP) ? (r1f > sks ? r1f : sks) : r1f;
  Y.R1 = take(mode == SCN_BWD ? sk : r1s);
  const size_t st = (size_t)2 * (((size_t)max_e + 3) / 4 * 4);
  const size_t yh0 = (size_t)max_n * H, yh = (!back && yh0 < GSCR) ? GSCR : yh0;
  const size_t bs = (size_t)2 * (max_n + 1) + (size_t)2 * max_e + 16;   // the CSR builders' scratch (step: inside R3)
  Y.R2 = take(yh > st ? yh : st);                      // y; the staged COO slice overlays it first
  Y.ek = Y.R2;
  Y.eo = Y.R2 + ((size_t)max_e + 3) / 4 * 4;
  size_t r3 = mode == SCN_STEP ? (sk > bs ? sk : bs) : mode == SCN_BWD ? sk : 0;
  if (mode == SCN_STEP) {   // S | y | dlogits (contiguous) later hold the 16 waves' gradient partials of scn_bwd_tiles
    const size_t NT = ((size_t)K + 15) / 16, TD = (size_t)H / 16;
    const size_t need = 16 * ((NT * TD + 2 * TD) * 256 + 16 * NT + H), have = (o - Y.R1) + r3;
    if (have < need) r3 += need - have;
  }
  Y.R3 = take(r3);
  Y.dinv = take(max_n);
  Y.dout = take(max_n);
  Y.wt = take((size_t)2 * H * FP + H + (size_t)K * H + K + (size_t)K * K);  // W_rel^T | W_root^T | b_rel | W_mlp^T | b_mlp | Gss
  Y.red = take(1024);        // wave partials, column-sum scratch
  Y.vecs = take(64);
  Y.rowptr_d = take(max_n + 1);
  Y.col_d = take(max_e);
  Y.rowptr_s = take(max_n + 1);
  Y.col_s = take(max_e);
  Y.cursor = take(back ? 0 : max_n + 1);     // the backward loads the CSRs
  Y.tmp = take(back ? 0 : max_e);
  Y.cursor2 = take(back ? 0 : max_n + 1);
  Y.tmp2 = take(back ? 0 : max_e);
  if (mode == SCN_STEP) {   // the step builds them in R3 (dlogits are not live before the backward half)
    size_t q = Y.R3;
    auto sub = [&](size_t n) { size_t r = q; q += (n + 3) & ~(size_t)3; return r; };
    Y.cursor = sub(max_n + 1); Y.tmp = sub(max_e); Y.cursor2 = sub(max_n + 1); Y.tmp2 = sub(max_e);
  }
  Y.wsum = take(32);
  Y.ssl = take(back ? (size_t)K * K : 0);   // the forward's S^T S, fetched with the rest of the front
  Y.total = o;
  return Y;
}

// out[o][k] = sum_j Am[j][o] * Bm[j][k]  (o < O, k < Kc; O, Kc <= 64; k < kmax stored) on
// v_mfma_f32_16x16x4_f32: a wave owns one 16 x 16 tile and a strided set of 4-row chunks of j (operands
// are single LDS words per lane, consecutive lanes on consecutive addresses, ragged edges read as 0);
// the waves that share a tile fold their partial tiles through `scratch` [NW][256] in a fixed order.
// Contains workgroup barriers.  `out` may be LDS or global.
template <int NW>
__device__ void gram_mfma(const float* Am, int lda, int O, const float* Bm, int ldb, int Kc, int n, float* scratch,
                          float* out, int ldo, int kmax) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wave = wave_id(), li = lane & 15, lj = lane >> 4;
  const int TO = (O + 15) >> 4, TK = (Kc + 15) >> 4, NT = TO * TK;
  const int TPP = NT < NW ? NT : NW, RG = NW / TPP;
  for (int t0 = 0; t0 < NT; t0 += TPP) {
    const int tl = wave % TPP, rg = wave / TPP, tile = t0 + tl;
    const bool live = tile < NT && rg < RG;
    if (live) {
      const int o0 = (tile / TK) * 16, k0 = (tile % TK) * 16;
      const bool oa = o0 + li < O, ob = k0 + li < Kc;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int j0 = rg * 4; j0 < n; j0 += 4 * RG) {
        const int j = j0 + lj;
        const bool ok = j < n;
        const float av = (ok && oa) ? Am[(size_t)j * lda + o0 + li] : 0.f;
        const float bv = (ok && ob) ? Bm[(size_t)j * ldb + k0 + li] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) scratch[(rg * TPP + tl) * 256 + (lj * 4 + r) * 16 + li] = acc[r];
    }
    lds_barrier();
    for (int idx = threadIdx.x; idx < TPP * 256; idx += SRT) {
      const int t_ = t0 + idx / 256, e_ = idx & 255;
      if (t_ < NT) {
        float s_ = 0.f;
        for (int r = 0; r < RG; ++r) s_ += scratch[(r * TPP + idx / 256) * 256 + e_];
        const int oo = (t_ / TK) * 16 + (e_ >> 4), kk = (t_ % TK) * 16 + (e_ & 15);
        if (oo < O && kk < kmax) out[(size_t)oo * ldo + kk] = s_;
      }
    }
    lds_barrier();
  }
}

// column sums of M[n][C] -> out[C] (C a multiple of 4, C <= 64): a lane adds float4 pieces of a
// strided row set (consecutive lanes on consecutive 16 B), the slots of a wave fold by shuffles, the
// waves through `scratch` [NW][C] in wave order.  Contains one workgroup barrier.
template <int NW>
__device__ void col_sum(const float* M, int ld, int C, int n, float* out, float* scratch) {
  const int lane = threadIdx.x & 63, wave = wave_id();
  if ((C & 3) != 0 || (64 % (C / 4)) != 0 || (ld & 3) != 0) {   // odd widths: wave per column, lanes split rows
    for (int c = wave; c < C; c += NW) {
      float s_ = 0.f;
      for (int i = lane; i < n; i += 64) s_ += M[(size_t)i * ld + c];
      s_ = wave_sum(s_);
      if (lane == 0) out[c] = s_;
    }
    lds_barrier();
    return;
  }
  const int LQ = C / 4, SQ = 64 / LQ;                 // lanes per row, row slots per wave
  const int slot = lane / LQ, f = (lane % LQ) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = wave * SQ + slot; i < n; i += NW * SQ) {
    const float4 v = *reinterpret_cast<const float4*>(M + (size_t)i * ld + f);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  for (int o_ = 32; o_ >= LQ; o_ >>= 1) {
    acc.x += __shfl_xor(acc.x, o_, 64);
    acc.y += __shfl_xor(acc.y, o_, 64);
    acc.z += __shfl_xor(acc.z, o_, 64);
    acc.w += __shfl_xor(acc.w, o_, 64);
  }
  if (slot == 0) *reinterpret_cast<float4*>(scratch + wave * C + f) = acc;
  lds_barrier();
  for (int c = threadIdx.x; c < C; c += SRT) {
    float s_ = 0.f;
    for (int w = 0; w < NW; ++w) s_ += scratch[w * C + c];
    out[c] = s_;
  }
}

// sum_{p in [s, t)} M[col[p] * ld + k], added in p order; four column reads and four row reads of a
// trip are issued together (the rows have a handful of entries: latency, not bandwidth)
__device__ __forceinline__ float gather_sum(const int* col, int s, int t, const float* M, int ld, int k) {
  float a = 0.f;
  for (int p0 = s; p0 < t; p0 += 4) {
    int j[4];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) j[u] = (p0 + u < t) ? col[p0 + u] : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = M[j[u] * ld + k];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (p0 + u < t) a += v[u];
  }
  return a;
}

// one wave: losses = {mean_g -num_g/den_g, mean_g ortho_g, their sum} from stats [G,4]
__device__ __forceinline__ void scn_losses_wave(const float* stats, float* losses, int G) {
  const int lane = threadIdx.x & 63;
  float mc = 0.f, o = 0.f;
  for (int g = lane; g < G; g += 64) {
    const float num = __hip_atomic_load(stats + (size_t)g * 4 + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float den = __hip_atomic_load(stats + (size_t)g * 4 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mc += -(num / den);
    o += __hip_atomic_load(stats + (size_t)g * 4 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  mc = wave_sum(mc);
  o = wave_sum(o);
  if (lane == 0) {
    const float a = mc / (float)G, b = o / (float)G;
    losses[0] = a;
    losses[1] = b;
    losses[2] = a + b;
  }
}

// ---- forward front end ---------------------------------------------------------------------------
// Every global input of the graph (weights, COO slice, features) is requested before anything is
// consumed: one HBM round trip, not one per array.  Then the two CSRs (target-keyed for GraphConv,
// source-keyed for A S) are built side by side by two wave groups between the same barriers, the
// gcn_norm degrees follow from the row lengths, and agg = A_hat x is reduced in edge order, loop last.
// Weights land transposed: WrT / WoT [FP][H] (rows k >= F zero), brl [H], WmT [H][K], bml [K].
template <int H, typename TS, bool PRE>
__device__ void scn_front(const ScnArgs& A, const ScnLayout& Y, float* fb, int* ib, int n0, int n, int e0, int ne,
                          int g, bool load_w = true) {   // load_w = false: the weights in LDS are current (k_scn_epoch)
  constexpr int NW = SRT / 64;
  const TS* const xg = reinterpret_cast<const TS*>(A.x);   // node features in their storage type (float or half)
  const int K = A.K, F = A.F;
  float *xs = fb + Y.R1, *agg = fb + Y.R1 + (size_t)A.max_n * FP, *dinv = fb + Y.dinv, *dout = fb + Y.dout;
  float* WrT = fb + Y.wt;
  float* WoT = WrT + FP * H;
  float* brl = WoT + FP * H;
  float* WmT = brl + H;
  float* bml = WmT + (size_t)H * K;
  int *ek = ib + Y.ek, *eo = ib + Y.eo;
  int *rowptr_d = ib + Y.rowptr_d, *col_d = ib + Y.col_d, *rowptr_s = ib + Y.rowptr_s, *col_s = ib + Y.col_s;
  const int wave = wave_id();
  const int wbase = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
  // ---- requests ----
  constexpr int WPT = (FP * H + SRT - 1) / SRT;
  constexpr int MPT = (64 * H + SRT - 1) / SRT;   // K <= 64
  constexpr int EPT = 2, XPT = 8;
  float wr[WPT], wo[WPT], wm[MPT], vb = 0.f, vm = 0.f;
  long long rd[EPT], rs[EPT];
  float xr[XPT];
#pragma unroll
  for (int i = 0; i < WPT; ++i) { wr[i] = 0.f; wo[i] = 0.f; }
#pragma unroll
  for (int i = 0; i < MPT; ++i) wm[i] = 0.f;
  if (load_w) {
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int d = threadIdx.x + i * SRT;          // slot k*H + o
      const int k = d / H, o = d - k * H;
      const bool ok = d < FP * H && k < F;
      const float a = A.W_rel[ok ? o * F + k : 0], b = A.W_root[ok ? o * F + k : 0];
      wr[i] = ok ? a : 0.f;
      wo[i] = ok ? b : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MPT; ++i) {
      const int d = threadIdx.x + i * SRT;          // slot h*K + k
      const int h = d / K, k = d - h * K;
      const bool ok = d < H * K;
      if (wbase + i * SRT < H * K) {
        const float t = A.W_mlp[ok ? k * H + h : 0];
        wm[i] = ok ? t : 0.f;
      }
    }
    if (wbase < H) vb = A.b_rel[threadIdx.x < H ? threadIdx.x : 0];
    if (wbase < K) vm = A.b_mlp[(int)threadIdx.x < K ? threadIdx.x : 0];
  }
  ScnArgsK KF = late_args();     // (the structure cache's fields: read here, not carried in scalar registers)
  constexpr bool pre = PRE;   // the structure of an earlier visit of this batch (ex_*): loaded, not rebuilt
  constexpr int RPT = 2;
  int rdp[RPT], rsp[RPT], cdp[EPT], csp[EPT];
  float dop[RPT], agr[XPT];
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = threadIdx.x + i * SRT;
    rd[i] = 0; rs[i] = 0; cdp[i] = 0; csp[i] = 0;
    if (wbase + i * SRT < ne) {
      if (!pre) {
        rd[i] = A.dst[e < ne ? e0 + e : e0];
        rs[i] = A.src[e < ne ? e0 + e : e0];
      } else {
        cdp[i] = KF->ex_col_d[(size_t)e0 + (e < ne ? e : 0)];
        csp[i] = KF->ex_col_s[(size_t)e0 + (e < ne ? e : 0)];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int idx = threadIdx.x + i * SRT;
    rdp[i] = 0; rsp[i] = 0; dop[i] = 0.f;
    if (pre && wbase + i * SRT <= n) {
      rdp[i] = KF->ex_rowptr_d[(size_t)n0 + g + (idx <= n ? idx : 0)];
      rsp[i] = KF->ex_rowptr_s[(size_t)n0 + g + (idx <= n ? idx : 0)];
      dop[i] = KF->ex_dout[(size_t)n0 + (idx < n ? idx : 0)];
    }
  }
  // cached front with padded features: x and A_hat x arrive as 16-byte pieces (n * FP / 4 of them each, at most two
  // per thread for n <= 512) instead of eight words per thread each
  constexpr int QPT = 2;
  const bool wide = pre && KF->ex_xpad != nullptr && n * (FP / 4) <= QPT * SRT;
  float4 xq[QPT], aq[QPT];
#pragma unroll
  for (int i = 0; i < QPT; ++i) {
    xq[i] = make_float4(0.f, 0.f, 0.f, 0.f); aq[i] = xq[i];
    const int i4 = threadIdx.x + i * SRT;
    if (wide && wbase + i * SRT < n * (FP / 4)) {
      const size_t at = (size_t)n0 * (FP / 4) + (i4 < n * (FP / 4) ? i4 : 0);
      xq[i] = reinterpret_cast<const float4*>(KF->ex_xpad)[at];
      aq[i] = reinterpret_cast<const float4*>(KF->ex_agg)[at];
    }
  }
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int idx = threadIdx.x + i * SRT;
    const int r = idx / FP, k = idx - r * FP;
    const bool ok = idx < n * FP && k < F;
    xr[i] = 0.f; agr[i] = 0.f;
    if (!wide && wbase + i * SRT < n * FP) {
      const float t = ldf(xg, ok ? (size_t)(n0 + r) * F + k : 0);
      xr[i] = ok ? t : 0.f;
      if (pre) agr[i] = KF->ex_agg[(size_t)n0 * FP + (idx < n * FP ? idx : 0)];
    }
  }
  // ---- park ----
  bool bad = false;
  auto stage_edge = [&](int e, long long d_, long long s_) {
    int k = (int)(d_ - n0), o = (int)(s_ - n0);
    if (k < 0 || k >= n || o < 0 || o >= n) { bad = true; k = -1; o = -1; }
    if (k == o) { k = -1; o = -1; }  // an existing self loop is replaced by the unit loop gcn_norm appends
    ek[e] = k;
    eo[e] = o;
  };
  if (!pre) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + i * SRT;
      if (e < ne) stage_edge(e, rd[i], rs[i]);
    }
    for (int e = threadIdx.x + EPT * SRT; e < ne; e += SRT) stage_edge(e, A.dst[e0 + e], A.src[e0 + e]);
    if (bad && A.flag) atomicOr(A.flag, 2);
  } else {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + i * SRT;
      if (e < ne) { col_d[e] = cdp[i]; col_s[e] = csp[i]; }
    }
    for (int e = threadIdx.x + EPT * SRT; e < ne; e += SRT) {
      col_d[e] = KF->ex_col_d[(size_t)e0 + e];
      col_s[e] = KF->ex_col_s[(size_t)e0 + e];
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      if (idx <= n) { rowptr_d[idx] = rdp[i]; rowptr_s[idx] = rsp[i]; }
      if (idx < n) dout[idx] = dop[i];
    }
    for (int idx = threadIdx.x + RPT * SRT; idx <= n; idx += SRT) {
      rowptr_d[idx] = KF->ex_rowptr_d[(size_t)n0 + g + idx];
      rowptr_s[idx] = KF->ex_rowptr_s[(size_t)n0 + g + idx];
      if (idx < n) dout[idx] = KF->ex_dout[(size_t)n0 + idx];
    }
    if (!wide) {
#pragma unroll
      for (int i = 0; i < XPT; ++i) {
        const int idx = threadIdx.x + i * SRT;
        if (idx < n * FP) agg[idx] = agr[i];
      }
      for (int idx = threadIdx.x + XPT * SRT; idx < n * FP; idx += SRT) agg[idx] = KF->ex_agg[(size_t)n0 * FP + idx];
    }
  }
  if (wide) {
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
      const int i4 = threadIdx.x + i * SRT;
      if (i4 < n * (FP / 4)) {
        reinterpret_cast<float4*>(xs)[i4] = xq[i];
        reinterpret_cast<float4*>(agg)[i4] = aq[i];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      if (idx < n * FP) xs[idx] = xr[i];
    }
    for (int idx = threadIdx.x + XPT * SRT; idx < n * FP; idx += SRT) {
      const int i = idx / FP, k = idx - i * FP;
      xs[idx] = k < F ? ldf(xg, (size_t)(n0 + i) * F + k) : 0.f;
    }
  }
  if (load_w) {
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int d = threadIdx.x + i * SRT;
      if (d < FP * H) { WrT[d] = wr[i]; WoT[d] = wo[i]; }
    }
#pragma unroll
    for (int i = 0; i < MPT; ++i) {
      const int d = threadIdx.x + i * SRT;
      if (d < H * K) WmT[d] = wm[i];
    }
    if (threadIdx.x < H) brl[threadIdx.x] = vb;
    if ((int)threadIdx.x < K) bml[threadIdx.x] = vm;
  }
  for (int i = threadIdx.x; i <= n; i += SRT) {   // the CSR builds count in these (and hand them back zeroed)
    (ib + Y.cursor)[i] = 0;
    (ib + Y.cursor2)[i] = 0;
  }
  lds_barrier();
  STAMP(1);
  if (pre) { STAMP(2); STAMP(3); return; }   // CSRs, out-degrees and A_hat x are in place
  // ---- structure: the two CSRs side by side (same barrier sequence in both wave groups) ----
  {
    const bool second = wave >= NW / 2;
    const Grp GS{(int)threadIdx.x - (second ? (NW / 2) * 64 : 0), (NW / 2) * 64, wave - (second ? NW / 2 : 0), NW / 2};
    if (!second) build_csr_lds(ek, eo, ne, n, rowptr_d, col_d, ib + Y.cursor, ib + Y.tmp, GS, false);   // rows = targets
    else build_csr_lds(eo, ek, ne, n, rowptr_s, col_s, ib + Y.cursor2, ib + Y.tmp2, GS, false);        // rows = sources
  }
  for (int i = threadIdx.x; i < n; i += SRT) {
    const float deg = (float)(rowptr_d[i + 1] - rowptr_d[i]) + 1.0f;        // scatter_add of unit weights + loop
    dinv[i] = 1.0f / sqrtf(deg);
    dout[i] = (float)(rowptr_s[i + 1] - rowptr_s[i]) + 1.0f;               // row sum of binary A + I
  }
  lds_barrier();
  STAMP(2);
  // agg_i = sum_{j->i} (dinv_j * 1 * dinv_i) x_j  (edge order)  +  (dinv_i * 1 * dinv_i) x_i  (loop last)
  {
    constexpr int LPR = FP / 4;
    const int rl = threadIdx.x / LPR, f = (threadIdx.x % LPR) * 4;
    for (int i = rl; i < n; i += SRT / LPR) {
      const float di = dinv[i];
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int p = rowptr_d[i]; p < rowptr_d[i + 1]; ++p) {
        const int j = col_d[p];
        const float w = mul_rn(mul_rn(dinv[j], 1.0f), di);
        const float4 v = *reinterpret_cast<const float4*>(xs + j * FP + f);
        a.x = add_rn(a.x, mul_rn(w, v.x)); a.y = add_rn(a.y, mul_rn(w, v.y));
        a.z = add_rn(a.z, mul_rn(w, v.z)); a.w = add_rn(a.w, mul_rn(w, v.w));
      }
      const float wl = mul_rn(mul_rn(di, 1.0f), di);
      const float4 v = *reinterpret_cast<const float4*>(xs + i * FP + f);
      a.x = add_rn(a.x, mul_rn(wl, v.x)); a.y = add_rn(a.y, mul_rn(wl, v.y));
      a.z = add_rn(a.z, mul_rn(wl, v.z)); a.w = add_rn(a.w, mul_rn(wl, v.w));
      *reinterpret_cast<float4*>(agg + i * FP + f) = a;
      if (KF->ex_agg) *reinterpret_cast<float4*>(KF->ex_agg + (size_t)(n0 + i) * FP + f) = a;
      if (KF->ex_xpad) *reinterpret_cast<float4*>(KF->ex_xpad + (size_t)(n0 + i) * FP + f) = v;   // (x_i, padded)
    }
  }
  // hand the structure to the backward launch
  if (KF->ex_rowptr_d) {
    for (int i = threadIdx.x; i <= n; i += SRT) {
      KF->ex_rowptr_d[(size_t)n0 + g + i] = rowptr_d[i];
      KF->ex_rowptr_s[(size_t)n0 + g + i] = rowptr_s[i];
    }
    const int cd = rowptr_d[n], cs = rowptr_s[n];
    for (int p = threadIdx.x; p < cd; p += SRT) KF->ex_col_d[(size_t)e0 + p] = col_d[p];
    for (int p = threadIdx.x; p < cs; p += SRT) KF->ex_col_s[(size_t)e0 + p] = col_s[p];
    for (int i = threadIdx.x; i < n; i += SRT) KF->ex_dout[(size_t)n0 + i] = dout[i];
  }
  lds_barrier();
  STAMP(3);
}

// ---- forward middle: shared by the forward launch and the one-launch step -------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// e^x for x <= 0 (softmax arguments, the negative side of ELU) in 6 VALU operations: 2^t off the hardware
// exponential (1 ulp) with t = rn(x log2 e), corrected by the product's rounding error and the low part of
// log2 e, which keeps ~2 ulp over the whole range (the library expf spends ~25 operations, most of them on ranges
// that cannot occur here; a graph's n x K softmax runs on ONE CU, where every VALU operation of the phase costs
// n K / 64 issue slots).  Underflows to 0 below ~ -87.
__device__ __forceinline__ float exp_nonpos(float x) {
  const float L2E = 1.4426950408889634f;
  const float t = x * L2E;
  float e = fmaf(x, L2E, -t);
  e = fmaf(x, 1.925963033500011e-08f, e);             // log2 e - (float)log2 e
  const float p = __builtin_amdgcn_exp2f(t);
  return fmaf(p, e * 0.6931471805599453f, p);         // 2^(t + e) = 2^t (1 + e ln 2 + O(e^2)), |e| < 2^-17
}

// the hidden activation (model/hscn.py: SCN's mp_act).  ELU's negative side is e^x - 1 from exp_nonpos:
// absolute error <= 1 ulp of 1.0 (expm1f is relatively exact near 0 and five times the operations).
__device__ __forceinline__ float scn_act(float v, int act) {
  switch (act) {
    case HSCN_ACT_RELU: return v > 0.f ? v : 0.f;
    case HSCN_ACT_ELU: { const float e = exp_nonpos(fminf(v, 0.f)) - 1.0f; return v > 0.f ? v : e; }   // (branch free: the four rows of a lane interleave)
    case HSCN_ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// One 16 x 16 output tile on v_mfma_f32_16x16x4_f32: acc[r] <-> (tile row 4 * lj + r, tile column li)
//   acc += sum_{k' < Kc} A[li][k'] * B[k'][bcol]
// The contraction index is dealt to the four lane groups in contiguous runs (lane group lj: k' in
// [KSp * lj, KSp * (lj + 1)), KSp = the padded quarter), so a lane's A operands are float4 pieces of ONE row:
// 16 rows x 64 bytes per instruction, conflict free.  Arow = the lane's row (16-byte aligned) or nullptr (a row
// outside the graph: zeros); Kc % 4 == 0.  B[k'][c] = Bm[k' * bsk + c * bsc]; bok: the lane's column exists.
__device__ __forceinline__ f32x4 tile_mm(const float* Arow, int Kc, const float* Bm, int bsk, int bsc, int bcol,
                                         bool bok, f32x4 acc) {
  const int lj = (threadIdx.x & 63) >> 4;
  const int KSp = ((Kc + 15) >> 4) << 2;
  const int kb = KSp * lj;
  for (int q = 0; q < KSp; q += 4) {
    const int k0 = kb + q;
    const bool kok = k0 < Kc;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (Arow && kok) a = *reinterpret_cast<const float4*>(Arow + k0);
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (bok && kok) {
      const float* bp = Bm + (size_t)k0 * bsk + (size_t)bcol * bsc;
      b0 = bp[0]; b1 = bp[bsk]; b2 = bp[2 * bsk]; b3 = bp[3 * bsk];
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);
  }
  return acc;
}

// y = act((agg W_rel^T + b_rel) + x W_root^T) for the 16 rows of tile rt, off the matrix cores.  KEEP: also hand
// back x and agg of the tile as the B operands of the backward's weight-gradient products (xb / ab [s] = element
// (row 4 * lj + s, feature li): the row order tile_mm's accumulators have), so the backward half needs no copy
// of x / agg in LDS.
template <int H, typename TS, bool KEEP>
__device__ __forceinline__ void scn_hidden_tile(const ScnArgs& A, int rt, const float* xs, const float* agg, float* yl,
                                                const float* WrT, const float* WoT, const float* brl, int n0, int n,
                                                float (&xb)[4], float (&ab)[4]) {
  constexpr int TD = H / 16;
  const int lane = threadIdx.x & 63, li = lane & 15, lj = lane >> 4;
  const int r0 = rt * 16;
  const bool rowok = r0 + li < n;
  const float* ar = rowok ? agg + (r0 + li) * FP : nullptr;
  const float* xr = rowok ? xs + (r0 + li) * FP : nullptr;
#pragma unroll
  for (int ct = 0; ct < TD; ++ct) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 a1 = tile_mm(ar, FP, WrT, H, 1, ct * 16 + li, true, z);
    const f32x4 a2 = tile_mm(xr, FP, WoT, H, 1, ct * 16 + li, true, z);
    const float b = brl[ct * 16 + li];
  #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + lj * 4 + r;
      if (row < n) {
        const float v = rnd<TS>(scn_act((a1[r] + b) + a2[r], A.act));   // the hidden activation as its storage type holds it
        yl[row * H + ct * 16 + li] = v;
        if (A.y) stf(reinterpret_cast<TS*>(A.y), (size_t)(n0 + row) * H + ct * 16 + li, v);
      }
    }
  }
  if (KEEP) {
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) {
      const int j = r0 + 4 * lj + s_;
      xb[s_] = j < n ? xs[j * FP + li] : 0.f;
      ab[s_] = j < n ? agg[j * FP + li] : 0.f;
    }
  }
}

// all tiles of the graph, a wave owns tiles wave, wave + NW, ...  Ends without a barrier.
template <int H, typename TS>
__device__ __forceinline__ void scn_hidden(const ScnArgs& A, const float* xs, const float* agg, float* yl,
                                           const float* WrT, const float* WoT, const float* brl, int n0, int n) {
  constexpr int NW = SRT / 64;
  const int ntile = (n + 15) >> 4;
  float d0[4], d1[4];
  for (int rt = wave_id(); rt < ntile; rt += NW)
    scn_hidden_tile<H, TS, false>(A, rt, xs, agg, yl, WrT, WoT, brl, n0, n, d0, d1);
}

// logits = y W_mlp^T + b_mlp off the matrix cores, softmax over the K columns in the accumulators (a row's
// columns sit in the 16 lanes of a DPP row and up to four column tiles).  S may overlay x / agg (dead), never
// y.  No barrier.
// K <= 16 (one column tile): the softmax values are, as they sit in the accumulators, both operands of S^T S =
// sum_rows S[row][a] S[row][b]; the wave adds its tiles' contribution on the spot and parks its 16 x 16 partial
// in ss_part [NW][256] (the caller folds the first min(ntile, NW) of them in wave order behind its next barrier).
template <int H>
__device__ __forceinline__ void scn_softmax(const ScnArgs& A, const float* yl, float* Sl, const float* WmT,
                                            const float* bml, int n0, int n, float* ss_part) {
  constexpr int NW = SRT / 64;
  const int K = A.K, NT = (K + 15) >> 4;
  const int lane = threadIdx.x & 63, li = lane & 15, lj = lane >> 4;
  const int ntile = (n + 15) >> 4;
  f32x4 ssacc = {0.f, 0.f, 0.f, 0.f};
  for (int rt = wave_id(); rt < ntile; rt += NW) {
    const int r0 = rt * 16;
    const float* yr = r0 + li < n ? yl + (r0 + li) * H : nullptr;
    float sc[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = nt * 16 + li;
      const bool cok = nt < NT && col < K;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (nt < NT) acc = tile_mm(yr, H, WmT, K, 1, col, cok, acc);
      const float bk = cok ? bml[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[nt][r] = cok ? acc[r] + bk : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + lj * 4 + r;
      float m = fmaxf(fmaxf(sc[0][r], sc[1][r]), fmaxf(sc[2][r], sc[3][r]));
      m = row16_max(m);
      float ex[4], sum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        ex[nt] = (nt < NT && nt * 16 + li < K) ? exp_nonpos(sc[nt][r] - m) : 0.f;
        sum += ex[nt];
      }
      sum = row16_sum(sum);
      const float rs = __builtin_amdgcn_rcpf(sum);   // (1 ulp; sum in [1, K])
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int col = nt * 16 + li;
        float v = 0.f;
        if (nt < NT && col < K && row < n) {
          v = ex[nt] * rs;
          Sl[row * K + col] = v;
          if (A.S) A.S[(size_t)(n0 + row) * K + col] = v;
        }
        if (nt == 0 && NT == 1) ssacc = __builtin_amdgcn_mfma_f32_16x16x4f32(v, v, ssacc, 0, 0, 0);
      }
    }
  }
  if (NT == 1 && (int)(wave_id()) < ntile) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ss_part[(wave_id()) * 256 + (lj * 4 + r) * 16 + li] = ssacc[r];
  }
}

// sum_{p in [s, t)} of the float4 at M[col[p] * ld], added in p order (four column / row reads of a trip in flight)
__device__ __forceinline__ float4 gather_sum4(const int* col, int s, int t, const float* M, int ld) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p0 = s; p0 < t; p0 += 4) {
    int j[4];
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) j[u] = (p0 + u < t) ? col[p0 + u] : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(M + j[u] * ld);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (p0 + u < t) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
  }
  return a;
}

// sum over idx = lane, lane + 64, ... < KK of f(idx), added in idx order; four terms are evaluated side by side
// (their divisions overlap) before they are added
template <typename Fn>
__device__ __forceinline__ float lane_strided_sum(int KK, Fn f) {
  const int lane = threadIdx.x & 63;
  float v = 0.f;
  for (int base = 0; base < KK; base += 256) {
    float t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + 64 * u + lane;
      t[u] = idx < KK ? f(idx) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) v += t[u];
  }
  return v;
}

// the statistics of graph g to HBM and, with a ticket counter, the batch losses by the workgroup that takes the last
// ticket: it sums the per-graph statistics in graph order (the order, hence the result, does not depend on who it
// is).  Wave 0 only.  The statistics are write-through (sc1) stores drained before the ticket is taken and are read
// back with agent-scope loads (cdna_hip_programming.md Guideline 16), so no agent-scope fence -- an L2 write-back
// and invalidate, microseconds at the end of every workgroup -- is needed on either side.
__device__ __forceinline__ void scn_stats_publish(const ScnArgs& A, int g, float num, float den, float nrm, float o) {
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    stf_sc1(A.stats, (size_t)g * 4 + 0, num);
    stf_sc1(A.stats, (size_t)g * 4 + 1, den);
    stf_sc1(A.stats, (size_t)g * 4 + 2, nrm);
    stf_sc1(A.stats, (size_t)g * 4 + 3, o);
  }
  if (A.ticket) {
    int last = 0;
    if (lane == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      last = __hip_atomic_fetch_add(A.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.B - 1;
    }
    last = __builtin_amdgcn_readfirstlane(last);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the loads below the ticket)
      scn_losses_wave(A.stats, A.losses, A.B);
      if (lane == 0) __hip_atomic_store(A.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// <Gq, ss> of the orthogonality backward (wave 0; every lane receives it)
__device__ __forceinline__ float scn_ortho_inner(const float* ssl, int K, float nrm, float o) {
  const float isk = 1.0f / sqrtf((float)K);
  float v = 0.f;
  if (o > 0.f)
    v = lane_strided_sum(K * K, [&](int i) {
      const int a = i / K, b = i - a * K;
      return ((ssl[i] / nrm - (a == b ? isk : 0.f)) / o) * ssl[i];
    });
  return wave_sum(v);
}

// MinCUT statistics on the binary A + I
//   num = sum_i S_i . (sum_{p in row_s(i)} S[col] + S_i),  den = sum_i dout_i |S_i|^2,  ss = S^T S -> ssl [K][K] (LDS)
// then stats[g] = {num, den, |ss|_F, ortho}.  `scratch`: 16 x 256 words (K <= 16: the tiles scn_softmax parked).
// K % 4 == 0: a wave owns 16-row tiles, lane (li = row, lj = a float4 of columns) walks the row's neighbours once
// for four columns.  STEP (the one-launch step): the backward's neighbour term
//   T = (A S)_i + (A^T S)_i + 2 S_i      (K % 4 == 0; otherwise the raw (A S)_i, the tail adds the rest)
// is kept in as_out [n][K] and the statistics are published by the caller after the backward half.  Every thread
// receives the statistics and the backward's <Gq, ss> in R.  Ends behind a barrier.
struct ScnStats { float num, den, nrm, o, inner; };
template <int NW, bool STEP>
__device__ __forceinline__ void scn_stats(const ScnArgs& A, const float* Sl, const int* rowptr_s, const int* col_s,
                                          const int* rowptr_d, const int* col_d, const float* dout, float* red,
                                          float* scratch, float* ssl, ScnStats& R, float* as_out, int n, int g) {
  const int K = A.K, KK = K * K;
  const int wave = wave_id(), lane = threadIdx.x & 63;
  {
    float num = 0.f, den = 0.f;
    if ((K & 3) == 0) {
      const int li = lane & 15, lj = lane >> 4, CG = K >> 2, ntile = (n + 15) >> 4;
      for (int rt = wave; rt < ntile; rt += NW) {
        const int i = rt * 16 + li;
        if (i < n) {
          const int ps = rowptr_s[i], pe = rowptr_s[i + 1];
          int qs = 0, qe = 0;
          if (STEP) { qs = rowptr_d[i]; qe = rowptr_d[i + 1]; }
          const float di = dout[i];
          for (int cg = lj; cg < CG; cg += 4) {
            const float4 sv = *reinterpret_cast<const float4*>(Sl + i * K + 4 * cg);
            float4 as = gather_sum4(col_s, ps, pe, Sl + 4 * cg, K);
            if (STEP) {
              const float4 ad = gather_sum4(col_d, qs, qe, Sl + 4 * cg, K);
              float4 t = as;
              t.x += ad.x; t.y += ad.y; t.z += ad.z; t.w += ad.w;
              t.x += 2.f * sv.x; t.y += 2.f * sv.y; t.z += 2.f * sv.z; t.w += 2.f * sv.w;
              *reinterpret_cast<float4*>(as_out + i * K + 4 * cg) = t;
            }
            as.x += sv.x; as.y += sv.y; as.z += sv.z; as.w += sv.w;
            num = fmaf(sv.x, as.x, num); num = fmaf(sv.y, as.y, num);
            num = fmaf(sv.z, as.z, num); num = fmaf(sv.w, as.w, num);
            den = fmaf(di, sv.x * sv.x, den); den = fmaf(di, sv.y * sv.y, den);
            den = fmaf(di, sv.z * sv.z, den); den = fmaf(di, sv.w * sv.w, den);
          }
        }
      }
    } else {
      for (int idx = threadIdx.x; idx < n * K; idx += SRT) {
        const int i = idx / K, k = idx - i * K;
        const float sv = Sl[idx];
        float as = gather_sum(col_s, rowptr_s[i], rowptr_s[i + 1], Sl, K, k);
        if (STEP) as_out[idx] = as;
        as += sv;
        num = fmaf(sv, as, num);
        den = fmaf(dout[i], sv * sv, den);
      }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) { red[wave] = num; red[16 + wave] = den; }
  }
  // ss = S^T S: K <= 16 -- the per-wave tiles scn_softmax parked in `scratch`, folded in wave order; otherwise
  // through the tile outer product
  if (K <= 16) {
    const int ntile = (n + 15) >> 4, NWA = ntile < NW ? ntile : NW;
    for (int e = threadIdx.x; e < 256; e += SRT) {
      float v = 0.f;
      for (int w = 0; w < NWA; ++w) v += scratch[w * 256 + e];
      const int a = e >> 4, b = e & 15;
      if (a < K && b < K) ssl[a * K + b] = v;
    }
    lds_barrier();
  } else {
    gram_mfma<NW>(Sl, K, K, Sl, K, K, n, scratch, ssl, K, K);
    lds_barrier();
  }
  STAMP(6);
  if (A.ss)
    for (int idx = threadIdx.x; idx < KK; idx += SRT) A.ss[(size_t)g * KK + idx] = ssl[idx];
  // norms by the whole workgroup, two rounds (|ss|_F, then everything that needs it); every thread ends with
  // the same values (ordered sums of the 16 wave partials)
  {
    float p2 = 0.f;
    for (int idx = threadIdx.x; idx < KK; idx += SRT) p2 += ssl[idx] * ssl[idx];
    p2 = wave_sum(p2);
    if (lane == 0) red[32 + wave] = p2;
  }
  lds_barrier();
  float num = 0.f, den = 0.f, n2 = 0.f;
  for (int w = 0; w < NW; ++w) { num += red[w]; den += red[16 + w]; n2 += red[32 + w]; }
  const float nrm = sqrtf(n2);
  const float isk = 1.0f / sqrtf((float)K);
  {
    float po = 0.f, pw = 0.f;
    for (int idx = threadIdx.x; idx < KK; idx += SRT) {
      const int a = idx / K, b = idx - a * K;
      const float q = ssl[idx] / nrm - (a == b ? isk : 0.f);
      po += q * q;
      pw += q * ssl[idx];
    }
    po = wave_sum(po);
    pw = wave_sum(pw);
    if (lane == 0) { red[48 + wave] = po; red[64 + wave] = pw; }
  }
  lds_barrier();
  float o2 = 0.f, wq = 0.f;
  for (int w = 0; w < NW; ++w) { o2 += red[48 + w]; wq += red[64 + w]; }
  R.num = num; R.den = den; R.nrm = nrm; R.o = sqrtf(o2);
  R.inner = R.o > 0.f ? wq / R.o : 0.f;   // <Gq, ss> of the orthogonality backward: sum_i ((q_i / o) ss_i)
  if (!STEP && threadIdx.x < 64) scn_stats_publish(A, g, R.num, R.den, R.nrm, R.o);
}

template <int H, typename TS>
__global__ void __launch_bounds__(SRT) k_scn_fwd(const ScnArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NW = SRT / 64;
  const int g = blockIdx.x, K = A.K;
  const int n0 = A.nptr[g], n = A.nptr[g + 1] - n0;
  const int e0 = A.eptr[g], ne = A.eptr[g + 1] - e0;
  if (n > A.max_n || ne > A.max_e || n < 0 || ne < 0) {
    if (threadIdx.x == 0 && A.flag) atomicOr(A.flag, 4);
    return;
  }
  const ScnLayout Y = scn_layout(H, K, A.max_n, A.max_e, SCN_FWD);
  float* fb = reinterpret_cast<float*>(smem);
  int* ib = reinterpret_cast<int*>(smem);
  float *xs = fb + Y.R1, *agg = xs + (size_t)A.max_n * FP, *Sl = fb + Y.R1, *yl = fb + Y.R2;
  float *dout = fb + Y.dout, *red = fb + Y.red;
  float* WrT = fb + Y.wt;            // [FP][H]
  float* WoT = WrT + FP * H;         // [FP][H]
  float* brl = WoT + FP * H;         // [H]
  float* WmT = brl + H;              // [H][K]
  float* bml = WmT + (size_t)H * K;  // [K]
  int *rowptr_s = ib + Y.rowptr_s, *col_s = ib + Y.col_s;

  STAMP(0);
  scn_front<H, TS, false>(A, Y, fb, ib, n0, n, e0, ne, g);
  scn_hidden<H, TS>(A, xs, agg, yl, WrT, WoT, brl, n0, n);
  lds_barrier();
  STAMP(4);
  scn_softmax<H>(A, yl, Sl, WmT, bml, n0, n, Sl + (size_t)A.max_n * K);   // x / agg are dead: S overlays them (y lives in R2: no overlap)
  lds_barrier();
  STAMP(5);
  // (K > 16: y is in HBM already, its LDS copy is the scratch of the tile product; ss takes the slot the backward uses for Gss)
  ScnStats R;
  scn_stats<NW, false>(A, Sl, rowptr_s, col_s, nullptr, nullptr, dout, red, K <= 16 ? Sl + (size_t)A.max_n * K : yl, bml + K, R,
                       nullptr, n, g);
  STAMP(63);
}

// ---- backward proper: shared by the backward launch and the one-launch step -----------------------
// In LDS on entry (behind a barrier): S (R1), y (R2), the forward's S^T S (ssl), both CSRs, dout, W_mlp^T; x and
// agg wait in registers (xr / agr, slot idx = thread + i * SRT of the [n][FP] arrays) until the buffers they take
// over are dead: R3 holds dlogits, then agg; R1 holds S, then x.  Rows beyond the register window are re-read
// from pag / A.x (pag NULL: the caller guarantees n * FP <= XPT * SRT).  Writes the parameter-gradient
// partials of this graph to `part` (global).
// STEP: <Gq, ss> (`inner`) and the raw (A S) gather (as_in [n][K], may alias DL) come from the forward half.
constexpr int SCN_XPT = 8;
template <int H, typename TS, bool STEP>
__device__ __forceinline__ void scn_bwd_tail(const ScnArgs& A, int n0, int n, float* Sl, float* yl, float* DL,
                                             const float* dout, float* red, const float* WmT, float* Gss,
                                             const float* ssl, const int* rowptr_d, const int* col_d,
                                             const int* rowptr_s, const int* col_s, const float (&agr)[SCN_XPT],
                                             const float (&xr)[SCN_XPT], const float* pag, float* part, float num,
                                             float den, float nrm, float o, float inner_in, const float* as_in) {
  constexpr int NW = SRT / 64, XPT = SCN_XPT;
  const int K = A.K, KK = A.K * A.K;
  const int lane = threadIdx.x & 63;
  float *xs = Sl, *agg = DL;
  const float gmc = (A.g_mc ? A.g_mc[0] : 0.f) / (float)A.B, go = (A.g_o ? A.g_o[0] : 0.f) / (float)A.B;
  const float isk = 1.0f / sqrtf((float)K);
  const float* ssg = ssl;
  if (!STEP) {
    if (threadIdx.x < 64) {
      const float v = scn_ortho_inner(ssg, K, nrm, o);
      if (lane == 0) red[0] = v;
    }
    lds_barrier();
  }
  STAMP(12);
  const float inner = STEP ? inner_in : red[0];
  for (int i = threadIdx.x; i < KK; i += SRT) {
    const int a = i / K, b = i - a * K;
    const float gq = o > 0.f ? (ssg[i] / nrm - (a == b ? isk : 0.f)) / o : 0.f;
    Gss[i] = (gq - inner / (nrm * nrm) * ssg[i]) / nrm;
  }
  lds_barrier();
  STAMP(13);
  // dS -> DL, then dlogits = S * (dS - <dS, S>) in place (KP lanes per row)
  const float c_num = -gmc / den, c_den = gmc * num / (den * den);
  {
    int KP = 1;
    while (KP < K) KP <<= 1;
    const int k = threadIdx.x % KP, r0 = threadIdx.x / KP;
    float gcol[32];   // this lane's column of Gss (K <= 32)
#pragma unroll
    for (int a = 0; a < 32; ++a) gcol[a] = (a < K && k < K && K <= 32) ? Gss[a * K + k] : 0.f;
    for (int i = r0; i < n; i += SRT / KP) {
      float dS = 0.f, sv = 0.f;
      if (k < K) {
        sv = Sl[i * K + k];
        float as = STEP ? as_in[i * K + k] : gather_sum(col_s, rowptr_s[i], rowptr_s[i + 1], Sl, K, k);   // (A S)_i
        as += gather_sum(col_d, rowptr_d[i], rowptr_d[i + 1], Sl, K, k);                  // (A^T S)_i
        as += 2.f * sv;                                                                   // the two identity terms
        float orth = 0.f;
        if (K <= 32 && (K & 3) == 0) {
#pragma unroll
          for (int a4 = 0; a4 < 8; ++a4) {
            if (4 * a4 < K) {
              const float4 sv4 = *reinterpret_cast<const float4*>(Sl + i * K + 4 * a4);
              orth = fmaf(sv4.x, gcol[4 * a4 + 0], orth); orth = fmaf(sv4.y, gcol[4 * a4 + 1], orth);
              orth = fmaf(sv4.z, gcol[4 * a4 + 2], orth); orth = fmaf(sv4.w, gcol[4 * a4 + 3], orth);
            }
          }
        } else {
          for (int a = 0; a < K; ++a) orth = fmaf(Sl[i * K + a], Gss[a * K + k], orth);
        }
        dS = c_num * as + c_den * 2.f * dout[i] * sv + go * 2.f * orth;
      }
      const float dot = seg_sum(dS * sv, KP);
      if (k < K) DL[i * K + k] = sv * (dS - dot);
    }
  }
  lds_barrier();
  STAMP(14);
  // parameter-gradient partials.  layout: W_rel [H*F], b_rel [H], W_root [H*F], W_mlp [K*H], b_mlp [K]
  const int oWrel = 0, obrel = H * A.F, oWroot = obrel + H, oWmlp = oWroot + H * A.F, obmlp = oWmlp + K * H;
  gram_mfma<NW>(DL, K, K, yl, H, H, n, Sl, part + oWmlp, H, H);   // dW_mlp[k][h] = sum_i DL[i][k] y[i][h]  (S is dead: scratch)
  col_sum<NW>(DL, K, K, n, part + obmlp, red);
  lds_barrier();
  STAMP(15);
  // dz = (DL W_mlp) * act'(y)  in place over y: thread (row, h)
  {
    const int h = threadIdx.x % H, r0 = threadIdx.x / H;
    if (K <= 32 && (K & 3) == 0) {
      float wrow[32];   // row h of W_mlp^T (K <= 32)
#pragma unroll
      for (int k = 0; k < 32; ++k) wrow[k] = k < K ? WmT[h * K + k] : 0.f;
      for (int i = r0; i < n; i += SRT / H) {
        float a = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) {
          if (4 * k4 < K) {
            const float4 d4 = *reinterpret_cast<const float4*>(DL + i * K + 4 * k4);
            a = fmaf(d4.x, wrow[4 * k4 + 0], a); a = fmaf(d4.y, wrow[4 * k4 + 1], a);
            a = fmaf(d4.z, wrow[4 * k4 + 2], a); a = fmaf(d4.w, wrow[4 * k4 + 3], a);
          }
        }
        yl[i * H + h] = a * act_grad_from_output(yl[i * H + h], A.act);
      }
    } else {
      for (int i = r0; i < n; i += SRT / H) {
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = fmaf(DL[i * K + k], WmT[h * K + k], a);
        yl[i * H + h] = a * act_grad_from_output(yl[i * H + h], A.act);
      }
    }
  }
  lds_barrier();
  STAMP(16);
  // dlogits are dead: agg takes their buffer (R3), S's buffer (R1) is the scratch of the first product
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int idx = threadIdx.x + i * SRT;
    if (idx < n * FP) agg[idx] = agr[i];
  }
  if (pag)
    for (int idx = threadIdx.x + XPT * SRT; idx < n * FP; idx += SRT) agg[idx] = pag[idx];
  lds_barrier();
  gram_mfma<NW>(yl, H, H, agg, FP, FP, n, Sl, part + oWrel, A.F, A.F);    // dW_rel[o][k] = sum_i dz[i][o] agg[i][k]
  // x takes S's buffer, agg's is the scratch of the second product
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int idx = threadIdx.x + i * SRT;
    if (idx < n * FP) xs[idx] = xr[i];
  }
  for (int idx = threadIdx.x + XPT * SRT; idx < n * FP; idx += SRT) {
    const int i = idx / FP, k = idx - i * FP;
    xs[idx] = k < A.F ? ldf(reinterpret_cast<const TS*>(A.x), (size_t)(n0 + i) * A.F + k) : 0.f;
  }
  lds_barrier();
  gram_mfma<NW>(yl, H, H, xs, FP, FP, n, agg, part + oWroot, A.F, A.F);   // dW_root[o][k] = sum_i dz[i][o] x[i][k]
  col_sum<NW>(yl, H, H, n, part + obrel, red);
}

// ---- the backward half of the one-launch step as ONE pass over the wave's own 16-row tiles ---------------
// (K % 4 == 0, K <= 16 * NTC, at most two tiles per wave: n <= 512.)  Everything between Gss and the parameter-gradient
// partials stays in the registers of the wave that owns the rows:
//   orth = S Gss (matrix cores) -> dS -> dlogits DL (accumulator layout; also to LDS, own rows, as the A operand
//   of the next product) -> dz = (DL W_mlp) * act'(y) (matrix cores) -> the three weight-gradient products
//   dW_mlp += DL^T y, dW_rel += dz^T agg, dW_root += dz^T x with the accumulators of one product as the A
//   operands of the next (row order 4 * lj + s on both sides), x / agg from the registers the forward half left.
// The per-wave partial tiles and bias sums are parked in the (then dead) S | y | dlogits buffers behind ONE
// barrier and folded in wave order: three barriers for the whole backward half.
// T = as_in [n][K] (aliases DL: an element is read by the lane that overwrites it).
// k_scn_epoch's optimizer state: the thread that folds parameter element p (P <= SRT) keeps its moments in registers
// across the visits, the counters travel as values; the updated weights go to global memory AND to their transposed
// slots in LDS, where the next visit reads them.
// Only the two moments are per-thread; everything uniform lives in a few LDS words (the counters double-buffered by
// visit parity: every thread reads this visit's pair, thread 0 writes the next visit's) -- as registers these eleven
// values were live across every phase of the visit loop and cost 9 - 17 vector spills (scratch reloads inside the loop).
struct ScnEpochState {
  float m, v;
  const double* pows;    // LDS: {beta1^t, beta2^t} as this visit reads them
  double* pows_next;     // LDS: where thread 0 leaves the next visit's pair
  float* f;              // LDS: [0..3] num, den, nrm, o of the last visit  [4] g_mc  [5] g_o  [6] step counter
};
template <int H, typename TS, int NTC>
__device__ __forceinline__ void scn_bwd_tiles(const ScnArgs& A, int n, const float* Sl, const float* yl, float* DL,
                                              const float* dout, const float* WmT, const float* Gss,
                                              const float (&xb)[2][4], const float (&ab)[2][4], float* scratch,
                                              float* part, float num, float den, ScnEpochState* ES = nullptr,
                                              float* wl = nullptr) {
  constexpr int NW = SRT / 64, TD = H / 16;
  const int K = A.K, NT = (K + 15) >> 4;
  const int wave = wave_id(), lane = threadIdx.x & 63, li = lane & 15, lj = lane >> 4;
  const int ntile = (n + 15) >> 4;
  const float gmc = ES ? ES->f[4] : (A.g_mc ? A.g_mc[0] : 0.f) / (float)A.B;
  const float go = ES ? ES->f[5] : (A.g_o ? A.g_o[0] : 0.f) / (float)A.B;
  const float c_num = -gmc / den, c_den = gmc * num / (den * den);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 gWm[NTC][TD], gWr[TD], gWo[TD];
  float dbm[NTC], dbr[TD];
#pragma unroll
  for (int nt = 0; nt < NTC; ++nt) {
    dbm[nt] = 0.f;
#pragma unroll
    for (int ct = 0; ct < TD; ++ct) gWm[nt][ct] = z4;
  }
#pragma unroll
  for (int ct = 0; ct < TD; ++ct) { gWr[ct] = z4; gWo[ct] = z4; dbr[ct] = 0.f; }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int rt = wave + t * NW;
    if (rt < ntile) {
      const int r0 = rt * 16;
      const bool rowok = r0 + li < n;
      const float* Srow = rowok ? Sl + (r0 + li) * K : nullptr;
      float sv[NTC][4], dS[NTC][4], dl[NTC][4];
#pragma unroll
      for (int nt = 0; nt < NTC; ++nt) {
        const int col = nt * 16 + li;
        const bool cok = nt < NT && col < K;
        f32x4 orth = z4;
        if (nt < NT) orth = tile_mm(Srow, K, Gss, K, 1, col, cok, orth);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + lj * 4 + r;
          const bool ok = cok && row < n;
          const float s_ = ok ? Sl[row * K + col] : 0.f;
          const float t_ = ok ? DL[row * K + col] : 0.f;
          const float d_ = ok ? dout[row] : 0.f;
          sv[nt][r] = s_;
          dS[nt][r] = ok ? c_num * t_ + c_den * 2.f * d_ * s_ + go * 2.f * orth[r] : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float dot = 0.f;
#pragma unroll
        for (int nt = 0; nt < NTC; ++nt) dot += dS[nt][r] * sv[nt][r];
        dot = row16_sum(dot);
        const int row = r0 + lj * 4 + r;
#pragma unroll
        for (int nt = 0; nt < NTC; ++nt) {
          const int col = nt * 16 + li;
          dl[nt][r] = sv[nt][r] * (dS[nt][r] - dot);
          if (nt < NT && col < K && row < n) DL[row * K + col] = dl[nt][r];
        }
      }
      float yv[TD][4];
#pragma unroll
      for (int ct = 0; ct < TD; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + lj * 4 + r;
          yv[ct][r] = row < n ? yl[row * H + ct * 16 + li] : 0.f;
        }
      // dW_mlp[k][h] += sum_rows DL[row][k] y[row][h];  db_mlp[k] += sum_rows DL[row][k]
#pragma unroll
      for (int nt = 0; nt < NTC; ++nt)
        if (nt < NT) {
#pragma unroll
          for (int ct = 0; ct < TD; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              gWm[nt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dl[nt][r], yv[ct][r], gWm[nt][ct], 0, 0, 0);
          dbm[nt] += ((dl[nt][0] + dl[nt][1]) + dl[nt][2]) + dl[nt][3];
        }
      // dz = (DL W_mlp) * act'(y): A = the tile's DL rows (this wave's own stores, in order behind them)
      const float* DLrow = rowok ? DL + (r0 + li) * K : nullptr;
#pragma unroll
      for (int ct = 0; ct < TD; ++ct) {
        const f32x4 acc = tile_mm(DLrow, K, WmT, 1, K, ct * 16 + li, true, z4);
        float dz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + lj * 4 + r;
          dz[r] = row < n ? acc[r] * act_grad_from_output(yv[ct][r], A.act) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gWr[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[r], ab[t][r], gWr[ct], 0, 0, 0);
          gWo[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[r], xb[t][r], gWo[ct], 0, 0, 0);
        }
        dbr[ct] += ((dz[0] + dz[1]) + dz[2]) + dz[3];
      }
    }
  }
  // bias sums over the four lane groups (rows 4 * lj + r): every lane ends with the wave's total of its column
#pragma unroll
  for (int nt = 0; nt < NTC; ++nt) { dbm[nt] += __shfl_xor(dbm[nt], 16, 64); dbm[nt] += __shfl_xor(dbm[nt], 32, 64); }
#pragma unroll
  for (int ct = 0; ct < TD; ++ct) { dbr[ct] += __shfl_xor(dbr[ct], 16, 64); dbr[ct] += __shfl_xor(dbr[ct], 32, 64); }
  STAMP(14);
  lds_barrier();   // every wave is done with S, T / DL and y: their buffers take the partials
  // block of wave w: tiles {dW_mlp (nt, ct)}, {dW_rel ct}, {dW_root ct} (256 words each, [m][n]), db_mlp [16 * NT], db_rel [H]
  const int NTL = NT * TD + 2 * TD, WSZ = NTL * 256 + 16 * NT + H;
  const int NWA = ntile < NW ? ntile : NW;   // waves that own a tile
  if (wave < NWA) {
    float* blk = scratch + (size_t)wave * WSZ;
#pragma unroll
    for (int nt = 0; nt < NTC; ++nt)
      if (nt < NT) {
#pragma unroll
        for (int ct = 0; ct < TD; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) blk[(nt * TD + ct) * 256 + (lj * 4 + r) * 16 + li] = gWm[nt][ct][r];
        if (lj == 0) blk[NTL * 256 + nt * 16 + li] = dbm[nt];
      }
#pragma unroll
    for (int ct = 0; ct < TD; ++ct) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        blk[(NT * TD + ct) * 256 + (lj * 4 + r) * 16 + li] = gWr[ct][r];
        blk[(NT * TD + TD + ct) * 256 + (lj * 4 + r) * 16 + li] = gWo[ct][r];
      }
      if (lj == 0) blk[NTL * 256 + 16 * NT + ct * 16 + li] = dbr[ct];
    }
  }
  lds_barrier();
  STAMP(15);
  // fold in wave order.  layout of part: W_rel [H*F], b_rel [H], W_root [H*F], W_mlp [K*H], b_mlp [K]
  ScnArgsK KA = late_args();   // (the optimizer's fields: loaded here, not carried through the kernel)
  const int F = A.F;
  const int obrel = H * F, oWroot = obrel + H, oWmlp = oWroot + H * F, obmlp = oWmlp + K * H;
  for (int p = threadIdx.x; p < A.P; p += SRT) {
    int off;
    if (p < obrel) { const int o_ = p / F, f = p - o_ * F; off = (NT * TD + (o_ >> 4)) * 256 + (o_ & 15) * 16 + f; }
    else if (p < oWroot) off = NTL * 256 + 16 * NT + (p - obrel);
    else if (p < oWmlp) { const int q = p - oWroot, o_ = q / F, f = q - o_ * F; off = (NT * TD + TD + (o_ >> 4)) * 256 + (o_ & 15) * 16 + f; }
    else if (p < obmlp) { const int q = p - oWmlp, k_ = q / H, h = q - k_ * H; off = ((k_ >> 4) * TD + (h >> 4)) * 256 + (k_ & 15) * 16 + (h & 15); }
    else off = NTL * 256 + (p - obmlp);
    float v = 0.f;
    for (int w = 0; w < NWA; ++w) v += scratch[(size_t)w * WSZ + off];
    part[p] = v;
    if (KA->adam_m) {   // B == 1: v IS the gradient of parameter element p -- the Adam step of csrc/optim.hip, same operations
      float* pp = p < obrel ? const_cast<float*>(A.W_rel) + p
                : p < oWroot ? const_cast<float*>(A.b_rel) + (p - obrel)
                : p < oWmlp ? const_cast<float*>(A.W_root) + (p - oWroot)
                : p < obmlp ? const_cast<float*>(A.W_mlp) + (p - oWmlp) : const_cast<float*>(A.b_mlp) + (p - obmlp);
      const double lr = KA->adam_lr[0];
      const double b1t = (ES ? ES->pows[0] : KA->adam_pows[0]) * KA->adam_b1, b2t = (ES ? ES->pows[1] : KA->adam_pows[1]) * KA->adam_b2;
      const float step_size = (float)(lr / (1.0 - b1t)), bc2_sqrt = (float)sqrt(1.0 - b2t);
      const float w1 = (float)(1.0 - KA->adam_b1), w2 = (float)(1.0 - KA->adam_b2), b2f = (float)KA->adam_b2;
      float pv, m, vv;
      const int K_ = A.K;
      int wslot;   // the element's slot in the LDS weight block: WrT [FP*H] | WoT [FP*H] | brl [H] | WmT [H*K] | bml [K]
      if (p < obrel) { const int o_ = p / F, f = p - o_ * F; wslot = f * H + o_; }
      else if (p < oWroot) wslot = 2 * FP * H + (p - obrel);
      else if (p < oWmlp) { const int q = p - oWroot, o_ = q / F, f = q - o_ * F; wslot = FP * H + f * H + o_; }
      else if (p < obmlp) { const int q = p - oWmlp, k_ = q / H, h = q - k_ * H; wslot = 2 * FP * H + H + h * K_ + k_; }
      else wslot = 2 * FP * H + H + H * K_ + (p - obmlp);
      if (ES) { pv = wl[wslot]; m = ES->m; vv = ES->v; }   // weights current in LDS, moments in this thread's registers
      else { pv = *pp; m = KA->adam_m[p]; vv = KA->adam_v[p]; }
      float g_ = v;
      if (KA->adam_wd != 0.0) {
        if (KA->adam_decoupled) pv = pv * (float)(1.0 - lr * KA->adam_wd);
        else g_ = g_ + (float)KA->adam_wd * pv;
      }
      m = m + w1 * (g_ - m);
      vv = vv * b2f;
      vv = vv + (w2 * g_) * g_;
      const float denom = sqrtf(vv) / bc2_sqrt + (float)KA->adam_eps;
      pv = pv + (-step_size) * (m / denom);
      *pp = pv;
      if (ES) { wl[wslot] = pv; ES->m = m; ES->v = vv; }
      else { KA->adam_m[p] = m; KA->adam_v[p] = vv; }
    }
  }
  if (ES) {   // the next visit's counters (the other parity: this visit's pair may still be being read)
    if (threadIdx.x == 0) {
      ES->pows_next[0] = ES->pows[0] * KA->adam_b1;
      ES->pows_next[1] = ES->pows[1] * KA->adam_b2;
      ES->f[6] += 1.0f;
    }
  } else if (KA->adam_m) {
    lds_barrier();   // every thread has read the counters
    if (threadIdx.x == 0) {
      KA->adam_step[0] = KA->adam_step[0] + 1.0f;
      KA->adam_pows[0] = KA->adam_pows[0] * KA->adam_b1;
      KA->adam_pows[1] = KA->adam_pows[1] * KA->adam_b2;
    }
  }
}

template <int H, typename TS>
__global__ void __launch_bounds__(SRT) k_scn_bwd(const ScnArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int g = blockIdx.x, K = A.K, KK = A.K * A.K;
  const int n0 = A.nptr[g], n = A.nptr[g + 1] - n0;
  const int e0 = A.eptr[g], ne = A.eptr[g + 1] - e0;
  float* part = A.partials + (size_t)g * A.P;
  if (n > A.max_n || ne > A.max_e || n < 0 || ne < 0) {
    if (threadIdx.x == 0 && A.flag) atomicOr(A.flag, 4);
    for (int i = threadIdx.x; i < A.P; i += SRT) part[i] = 0.f;
    return;
  }
  const ScnLayout Y = scn_layout(H, K, A.max_n, A.max_e, SCN_BWD);
  float* fb = reinterpret_cast<float*>(smem);
  int* ib = reinterpret_cast<int*>(smem);
  float* Sl = fb + Y.R1;                                   // S, and x once S is dead
  float *yl = fb + Y.R2, *DL = fb + Y.R3, *dout = fb + Y.dout, *red = fb + Y.red;   // dlogits, then agg
  float* WmT = fb + Y.wt + 2 * FP * H + H;   // [H][K] (same offsets as the forward's weight block)
  float* Gss = WmT + (size_t)H * K + K;      // [K][K]
  float* ssl = fb + Y.ssl;                   // [K][K] the forward's S^T S
  int *rowptr_d = ib + Y.rowptr_d, *col_d = ib + Y.col_d, *rowptr_s = ib + Y.rowptr_s, *col_s = ib + Y.col_s;

  STAMP(0);
  // ---- front: everything comes from HBM in one batch of requests -- the CSRs, agg and the binary
  // out-degree the forward launch exported, x, S and y, W_mlp -- then is parked in LDS
  constexpr int XPT = SCN_XPT;
  float agr[XPT], xr[XPT];   // agg and x wait in registers until the LDS buffers they take over are dead
  const float* pag = A.ex_agg + (size_t)n0 * FP;
  {
    const int wbase = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    constexpr int RPT = 2, EPT = 2, MPT = (64 * H + SRT - 1) / SRT;
    int rdp[RPT], rsp[RPT], cdp[EPT], csp[EPT];
    float dop[RPT], sr[XPT], yr[XPT], wm[MPT], ssr[4];
    const int32_t *prd = A.ex_rowptr_d + (size_t)n0 + g, *prs = A.ex_rowptr_s + (size_t)n0 + g;
    const int32_t *pcd = A.ex_col_d + (size_t)e0, *pcs = A.ex_col_s + (size_t)e0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      rdp[i] = 0; rsp[i] = 0; dop[i] = 0.f;
      if (wbase + i * SRT <= n) {
        rdp[i] = prd[idx <= n ? idx : 0];
        rsp[i] = prs[idx <= n ? idx : 0];
        dop[i] = A.ex_dout[(size_t)n0 + (idx < n ? idx : 0)];
      }
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + i * SRT;
      cdp[i] = 0; csp[i] = 0;
      if (wbase + i * SRT < ne) {
        cdp[i] = pcd[e < ne ? e : 0];
        csp[i] = pcs[e < ne ? e : 0];
      }
    }
    const float* pS = A.S + (size_t)n0 * K;
    const TS* py = reinterpret_cast<const TS*>(A.y) + (size_t)n0 * H;
    const TS* xg = reinterpret_cast<const TS*>(A.x);
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      const int r = idx / FP, k = idx - r * FP;
      const bool okx = idx < n * FP && k < A.F;
      agr[i] = 0.f; xr[i] = 0.f; sr[i] = 0.f; yr[i] = 0.f;
      if (wbase + i * SRT < n * FP) {
        agr[i] = pag[idx < n * FP ? idx : 0];
        const float t = ldf(xg, okx ? (size_t)(n0 + r) * A.F + k : 0);
        xr[i] = okx ? t : 0.f;
      }
      if (wbase + i * SRT < n * K) sr[i] = pS[idx < n * K ? idx : 0];
      if (wbase + i * SRT < n * H) yr[i] = ldf(py, idx < n * H ? idx : 0);
    }
#pragma unroll
    for (int i = 0; i < MPT; ++i) {
      const int d = threadIdx.x + i * SRT;          // slot h*K + k
      const int h = d / K, k = d - h * K;
      wm[i] = 0.f;
      if (wbase + i * SRT < H * K) wm[i] = A.W_mlp[d < H * K ? k * H + h : 0];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                   // ss [K,K] of this graph (K <= 64: 4 words per thread)
      const int d = threadIdx.x + i * SRT;
      ssr[i] = 0.f;
      if (wbase + i * SRT < KK) ssr[i] = A.ss[(size_t)g * KK + (d < KK ? d : 0)];
    }
    // ---- park ----
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = threadIdx.x + i * SRT;
      if (d < KK) ssl[d] = ssr[i];
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      if (idx <= n) { rowptr_d[idx] = rdp[i]; rowptr_s[idx] = rsp[i]; }
      if (idx < n) dout[idx] = dop[i];
    }
    for (int idx = threadIdx.x + RPT * SRT; idx <= n; idx += SRT) { rowptr_d[idx] = prd[idx]; rowptr_s[idx] = prs[idx]; }
    for (int idx = threadIdx.x + RPT * SRT; idx < n; idx += SRT) dout[idx] = A.ex_dout[(size_t)n0 + idx];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = threadIdx.x + i * SRT;
      if (e < ne) { col_d[e] = cdp[i]; col_s[e] = csp[i]; }
    }
    for (int e = threadIdx.x + EPT * SRT; e < ne; e += SRT) { col_d[e] = pcd[e]; col_s[e] = pcs[e]; }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = threadIdx.x + i * SRT;
      if (idx < n * K) Sl[idx] = sr[i];
      if (idx < n * H) yl[idx] = yr[i];
    }
    for (int idx = threadIdx.x + XPT * SRT; idx < n * K; idx += SRT) Sl[idx] = pS[idx];
    for (int idx = threadIdx.x + XPT * SRT; idx < n * H; idx += SRT) yl[idx] = ldf(py, idx);
#pragma unroll
    for (int i = 0; i < MPT; ++i) {
      const int d = threadIdx.x + i * SRT;
      if (d < H * K) WmT[d] = wm[i];
    }
  }
  const float num = A.stats[g * 4 + 0], den = A.stats[g * 4 + 1], nrm = A.stats[g * 4 + 2], o = A.stats[g * 4 + 3];
  lds_barrier();   // the front's LDS stores
  STAMP(1);
  scn_bwd_tail<H, TS, false>(A, n0, n, Sl, yl, DL, dout, red, WmT, Gss, ssl, rowptr_d, col_d, rowptr_s, col_s, agr, xr,
                             pag, part, num, den, nrm, o, 0.f, nullptr);
  STAMP(63);
}

// ---- the one-launch step: forward, losses and backward of graph g in one workgroup -----------------
// What the forward launch exported for the backward launch (both CSRs, agg, dout, S, y, S^T S, the statistics)
// simply stays in LDS; x and agg move to registers before S takes their buffer.  Upstream gradients g_mc / g_o
// (device scalars, the reference's loss = mincut + ortho has both = 1) are divided by B as in the backward launch.
// With B == 1 the partials ARE the gradients (A.partials = grads): no fold launch.
template <int H, typename TS, bool PRE>
__global__ void __launch_bounds__(SRT) k_scn_step(const ScnArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NW = SRT / 64;
  const int g = blockIdx.x, K = A.K;
  const int n0 = A.nptr[g], n = A.nptr[g + 1] - n0;
  const int e0 = A.eptr[g], ne = A.eptr[g + 1] - e0;
  float* part = A.partials + (size_t)g * A.P;
  if (n > A.max_n || ne > A.max_e || n < 0 || ne < 0) {
    if (threadIdx.x == 0 && A.flag) atomicOr(A.flag, 4);
    for (int i = threadIdx.x; i < A.P; i += SRT) part[i] = 0.f;
    return;
  }
  const ScnLayout Y = scn_layout(H, K, A.max_n, A.max_e, SCN_STEP);
  float* fb = reinterpret_cast<float*>(smem);
  int* ib = reinterpret_cast<int*>(smem);
  float *xs = fb + Y.R1, *agg = xs + (size_t)A.max_n * FP, *Sl = fb + Y.R1, *yl = fb + Y.R2, *DL = fb + Y.R3;
  float *dout = fb + Y.dout, *red = fb + Y.red;
  float* WrT = fb + Y.wt;
  float* WoT = WrT + FP * H;
  float* brl = WoT + FP * H;
  float* WmT = brl + H;
  float* bml = WmT + (size_t)H * K;
  float* Gss = bml + K;
  float* ssl = fb + Y.ssl;
  int *rowptr_d = ib + Y.rowptr_d, *col_d = ib + Y.col_d, *rowptr_s = ib + Y.rowptr_s, *col_s = ib + Y.col_s;

  STAMP(0);
  scn_front<H, TS, PRE>(A, Y, fb, ib, n0, n, e0, ne, g);
  // (K % 4 == 0: hscn_scn_resident_train_step_supported)
  const int wave = wave_id(), ntile = (n + 15) >> 4;
  float xb[2][4], ab[2][4];    // x / agg of the wave's own tiles as B operands of the backward half
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) { xb[t][s_] = 0.f; ab[t][s_] = 0.f; }
    const int rt = wave + t * NW;
    if (rt < ntile) scn_hidden_tile<H, TS, true>(A, rt, xs, agg, yl, WrT, WoT, brl, n0, n, xb[t], ab[t]);
  }
  lds_barrier();
  STAMP(4);
  scn_softmax<H>(A, yl, Sl, WmT, bml, n0, n, Sl + (size_t)A.max_n * K);
  lds_barrier();
  STAMP(5);
  // the backward's neighbour term is kept in the dlogits buffer (each element is read back by the lane that
  // overwrites it); the tile scratch of S^T S is the part of x | agg behind S
  ScnStats R;
  scn_stats<NW, true>(A, Sl, rowptr_s, col_s, rowptr_d, col_d, dout, red, Sl + (size_t)A.max_n * K, ssl, R, DL, n, g);
  STAMP(7);
  const float num = R.num, den = R.den, nrm = R.nrm, o = R.o;
  {
    const float inner = R.inner;
    const float isk = 1.0f / sqrtf((float)K);
    for (int i = threadIdx.x; i < K * K; i += SRT) {
      const int a = i / K, b = i - a * K;
      const float gq = o > 0.f ? (ssl[i] / nrm - (a == b ? isk : 0.f)) / o : 0.f;
      Gss[i] = (gq - inner / (nrm * nrm) * ssl[i]) / nrm;
    }
  }
  lds_barrier();
  STAMP(13);
  // the statistics go out (write-through stores, drained, then the ticket) from the LAST wave, which owns at most
  // one tile where the first ones own two: the drain hides behind the other waves' second tile
  if (wave == NW - 1) scn_stats_publish(A, g, num, den, nrm, o);
  // (column tiles x hidden tiles <= 2: more accumulators than that do not fit the register file of 16 waves)
  if (H == 32 || K <= 16) scn_bwd_tiles<H, TS, 1>(A, n, Sl, yl, DL, dout, WmT, Gss, xb, ab, fb + Y.R1, part, num, den);
  else if constexpr (H == 16) scn_bwd_tiles<H, TS, 2>(A, n, Sl, yl, DL, dout, WmT, Gss, xb, ab, fb + Y.R1, part, num, den);
  STAMP(63);
}

// ---- the chain of visits as ONE launch of one persistent workgroup -------------------------------------------------
// train/train_clustering.py:34-50 is a chain: every visit needs the weights the previous one left.  One workgroup walks
// `visits` graphs (g = v mod G): the weights live in LDS (the optimizer's tail updates them there, transposed slots
// included), the Adam moments in the registers of the threads that fold the gradient (P <= 1024), the counters as
// values; per visit it loads the graph's features and cached structure and runs exactly the phases of k_scn_step.
// The shape arguments every phase derives its index arithmetic from are laundered at the top of each visit: the
// compiler otherwise hoists all of it out of the visit loop and spills (145 scalar / 130 vector registers, measured).
template <int H, typename TS>
__global__ void __launch_bounds__(SRT) k_scn_epoch(const ScnArgs A0) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NW = SRT / 64;
  ScnArgsK KA = late_args();
  __shared__ double es_pows[4];     // two parities of {beta1^t, beta2^t}
  __shared__ float es_f[8];
  ScnEpochState ES;
  {
    const int p = threadIdx.x;
    ES.m = p < A0.P ? KA->adam_m[p] : 0.f;
    ES.v = p < A0.P ? KA->adam_v[p] : 0.f;
    ES.f = es_f;
    if (p == 0) {
      es_pows[0] = KA->adam_pows[0]; es_pows[1] = KA->adam_pows[1];
      es_f[0] = 0.f; es_f[1] = 1.f; es_f[2] = 0.f; es_f[3] = 0.f;
      es_f[4] = A0.g_mc ? A0.g_mc[0] : 0.f;   // (B = 1: no division)
      es_f[5] = A0.g_o ? A0.g_o[0] : 0.f;
      es_f[6] = KA->adam_step[0];
    }
  }
  lds_barrier();
  int par = 0;      // parity of the counters the next executed visit reads
  bool have_w = false;
  for (long long v = A0.visit0; v < A0.visit0 + A0.visits; ++v) {
    float num, den, nrm, o;
    ES.pows = es_pows + 2 * par;
    ES.pows_next = es_pows + 2 * (par ^ 1);
    ScnArgs A = A0;
    {   // per-visit opaque copies of what the phases' index arithmetic is derived from
      int K_ = A.K, F_ = A.F, mn = A.max_n, me = A.max_e, P_ = A.P;
      asm volatile("" : "+s"(K_), "+s"(F_), "+s"(mn), "+s"(me), "+s"(P_));
      A.K = K_; A.F = F_; A.max_n = mn; A.max_e = me; A.P = P_;
    }
    const int K = A.K;
    const ScnLayout Y = scn_layout(H, K, A.max_n, A.max_e, SCN_STEP);
    float* fb = reinterpret_cast<float*>(smem);
    int* ib = reinterpret_cast<int*>(smem);
    float *xs = fb + Y.R1, *agg = xs + (size_t)A.max_n * FP, *Sl = fb + Y.R1, *yl = fb + Y.R2, *DL = fb + Y.R3;
    float *dout = fb + Y.dout, *red = fb + Y.red;
    float* WrT = fb + Y.wt;
    float* WoT = WrT + FP * H;
    float* brl = WoT + FP * H;
    float* WmT = brl + H;
    float* bml = WmT + (size_t)H * K;
    float* Gss = bml + K;
    float* ssl = fb + Y.ssl;
    int *rowptr_d = ib + Y.rowptr_d, *col_d = ib + Y.col_d, *rowptr_s = ib + Y.rowptr_s, *col_s = ib + Y.col_s;
    const int wave = wave_id();
    const int g = (int)(v % A.G);
    const int n0 = A.nptr[g], n = A.nptr[g + 1] - n0;
    const int e0 = A.eptr[g], ne = A.eptr[g + 1] - e0;
    if (n > A.max_n || ne > A.max_e || n < 1 || ne < 0) {   // (uniform) skipped: no step for this graph
      if (threadIdx.x == 0 && A.flag) atomicOr(A.flag, 4);
      continue;
    }
    scn_front<H, TS, true>(A, Y, fb, ib, n0, n, e0, ne, g, !have_w);
    have_w = true;
    const int ntile = (n + 15) >> 4;
    float xb[2][4], ab[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) { xb[t][s_] = 0.f; ab[t][s_] = 0.f; }
      const int rt = wave + t * NW;
      if (rt < ntile) scn_hidden_tile<H, TS, true>(A, rt, xs, agg, yl, WrT, WoT, brl, n0, n, xb[t], ab[t]);
    }
    lds_barrier();
    scn_softmax<H>(A, yl, Sl, WmT, bml, n0, n, Sl + (size_t)A.max_n * K);
    lds_barrier();
    ScnStats R;
    scn_stats<NW, true>(A, Sl, rowptr_s, col_s, rowptr_d, col_d, dout, red, Sl + (size_t)A.max_n * K, ssl, R, DL, n, g);
    num = R.num; den = R.den; nrm = R.nrm; o = R.o;
    if (threadIdx.x == 0) { es_f[0] = num; es_f[1] = den; es_f[2] = nrm; es_f[3] = o; }
    par ^= 1;
    {
      const float inner = R.inner;
      const float isk = 1.0f / sqrtf((float)K);
      for (int i = threadIdx.x; i < K * K; i += SRT) {
        const int a = i / K, b = i - a * K;
        const float gq = o > 0.f ? (ssl[i] / nrm - (a == b ? isk : 0.f)) / o : 0.f;
        Gss[i] = (gq - inner / (nrm * nrm) * ssl[i]) / nrm;
      }
    }
    lds_barrier();
    if (H == 32 || K <= 16)
      scn_bwd_tiles<H, TS, 1>(A, n, Sl, yl, DL, dout, WmT, Gss, xb, ab, fb + Y.R1, A.partials, num, den, &ES, fb + Y.wt);
    else if constexpr (H == 16)
      scn_bwd_tiles<H, TS, 2>(A, n, Sl, yl, DL, dout, WmT, Gss, xb, ab, fb + Y.R1, A.partials, num, den, &ES, fb + Y.wt);
    lds_barrier();   // the updated weights (LDS) before the next visit reads them; the parked partials are dead
  }
  {
    const int p = threadIdx.x;
    if (p < A0.P) { KA->adam_m[p] = ES.m; KA->adam_v[p] = ES.v; }
    if (p == 0) {
      const float num = es_f[0], den = es_f[1], nrm = es_f[2], o = es_f[3];
      KA->adam_step[0] = es_f[6]; KA->adam_pows[0] = es_pows[2 * par]; KA->adam_pows[1] = es_pows[2 * par + 1];
      if (A0.stats) { A0.stats[0] = num; A0.stats[1] = den; A0.stats[2] = nrm; A0.stats[3] = o; }
      if (A0.losses) { const float a = -(num / den); A0.losses[0] = a; A0.losses[1] = o; A0.losses[2] = a + o; }
    }
  }
}

__global__ void k_scn_losses(const float* __restrict__ stats, float* __restrict__ losses, int G) {
  scn_losses_wave(stats, losses, G);
}

inline int64_t scn_param_count(int F, int H, int K) { return (int64_t)2 * H * F + H + (int64_t)K * H + K; }

inline size_t scn_lds_bytes(int H, int K, int max_n, int max_e, ScnMode mode) {
  return scn_layout(H, K, max_n, max_e, mode).total * 4;
}

// the hidden width and the storage type as template arguments, f(std::integral_constant<int, H>{}, TS{}), for the four
// combinations stage A is instantiated at
template <typename F>
int dispatch_scn(int H, bool f16, F&& f) {
  const std::integral_constant<int, 16> h16;
  const std::integral_constant<int, 32> h32;
  if (H != 16 && H != 32) return HSCN_E_UNSUPPORTED;
  return f16 ? (H == 16 ? f(h16, half_t{}) : f(h32, half_t{})) : (H == 16 ? f(h16, float{}) : f(h32, float{}));
}

// one workgroup per graph of the batch; the step's kernel comes in two forms, structure built or loaded (A.pre)
int launch_scn(const ScnArgs& A, int H, bool f16, ScnMode mode, hipStream_t st) {
  const size_t lds = scn_lds_bytes(H, A.K, A.max_n, A.max_e, mode);
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  return dispatch_scn(H, f16, [&](auto h, auto ts) {
    constexpr int HH = decltype(h)::value;
    using TS = decltype(ts);
    const auto k = mode == SCN_FWD   ? k_scn_fwd<HH, TS>
                   : mode == SCN_BWD ? k_scn_bwd<HH, TS>
                   : A.pre           ? k_scn_step<HH, TS, true>
                                     : k_scn_step<HH, TS, false>;
    return launch_with_lds(k, (unsigned)A.B, SRT, lds, st, A);
  });
}

// the fields every entry point sets (NULL where a launch has no use for one); each adds what is its own
ScnArgs scn_args(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr, const int32_t* eptr,
                 const float* W_rel, const float* b_rel, const float* W_root, const float* W_mlp, const float* b_mlp,
                 int64_t N, int64_t B, int F, int H, int K, int act, int max_n, int max_e, float* stats, float* losses,
                 int32_t* ticket, int32_t* flag) {
  ScnArgs A{};
  A.x = (const float*)x; A.src = edge_index; A.dst = edge_index ? edge_index + E : nullptr; A.nptr = nptr; A.eptr = eptr;
  A.W_rel = W_rel; A.b_rel = b_rel; A.W_root = W_root; A.W_mlp = W_mlp; A.b_mlp = b_mlp;
  A.N = N; A.F = F; A.K = K; A.act = act; A.max_n = max_n; A.max_e = max_e; A.B = (int)B;
  A.P = (int)scn_param_count(F, H, K);
  A.stats = stats; A.losses = losses; A.ticket = ticket; A.flag = flag;
  return A;
}

bool adam_ok(const hscn_adam* opt) {
  return opt->exp_avg && opt->exp_avg_sq && opt->step && opt->beta_pows && opt->lr && opt->beta1 >= 0.0 &&
         opt->beta1 < 1.0 && opt->beta2 >= 0.0 && opt->beta2 < 1.0 && opt->eps >= 0.0 && opt->weight_decay >= 0.0;
}
void set_adam(ScnArgs& A, const hscn_adam* opt) {
  A.adam_m = opt->exp_avg; A.adam_v = opt->exp_avg_sq; A.adam_step = opt->step; A.adam_pows = opt->beta_pows;
  A.adam_lr = opt->lr; A.adam_b1 = opt->beta1; A.adam_b2 = opt->beta2; A.adam_eps = opt->eps;
  A.adam_wd = opt->weight_decay; A.adam_decoupled = opt->decoupled;
}

// a structure block has its arrays; the column arrays may be missing only where the caller says so (no edges)
bool structure_ok(const hscn_scn_structure* c, bool cols_may_be_null) {
  return c->rowptr_d && c->rowptr_s && c->agg && c->dout && (cols_may_be_null || (c->col_d && c->col_s));
}
void set_structure(ScnArgs& A, const hscn_scn_structure* c) {
  A.ex_rowptr_d = c->rowptr_d; A.ex_col_d = c->col_d; A.ex_rowptr_s = c->rowptr_s; A.ex_col_s = c->col_s;
  A.ex_agg = c->agg; A.ex_dout = c->dout; A.ex_xpad = c->xpad;
  A.pre = c->ready != 0;   // ready: load the structure an earlier visit exported; else build it and export
}

}  // namespace

extern "C" {

#ifdef HSCN_STAMPS
int hscn_diag_set_stamp_buffer_scn(long long* buf) {   // this translation unit's copy of the stamp pointer
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf));
}
#endif

int hscn_scn_resident_supported(int F, int H, int K, int max_n, int max_e) {
  if (!(H == 16 || H == 32) || F < 1 || F > FP || K < 1 || K > 64 || max_n < 0 || max_e < 0) return 0;
  if (SRT % H != 0) return 0;
  if (scn_lds_bytes(H, K, max_n, max_e, SCN_FWD) > LDS_CU_BYTES) return 0;
  if (scn_lds_bytes(H, K, max_n, max_e, SCN_BWD) > LDS_CU_BYTES) return 0;
  return 1;
}

int64_t hscn_scn_resident_param_count(int F, int H, int K) { return scn_param_count(F, H, K); }

int hscn_scn_resident_train_step_supported(int F, int H, int K, int max_n, int max_e) {
  if (!hscn_scn_resident_supported(F, H, K, max_n, max_e)) return 0;
  // float4 rows of S; at most two 16-row tiles per wave; at most two accumulator tiles of dW_mlp per wave
  if ((K & 3) != 0 || max_n > 512 || ((K + 15) / 16) * (H / 16) > 2) return 0;
  if (scn_lds_bytes(H, K, max_n, max_e, SCN_STEP) > LDS_CU_BYTES) return 0;
  return 1;
}

// HSCN_STORE_F16 (all four launches below): IEEE-half storage of the node features x and of the saved hidden
// activation y (include/hscn.h); S, the statistics, the exported aggregation A_hat x (an accumulator output) and every
// gradient stay float.  ScnArgs types both as float*; the kernels read them as TS.
int hscn_scn_resident_train_step(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                                 const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                                 const float* W_rel, const float* b_rel, const float* W_root, const float* W_mlp,
                                 const float* b_mlp, const float* g_mc, const float* g_o, int max_n, int max_e,
                                 float* S, float* stats, float* losses, int32_t* ticket, float* partials,
                                 float* grads, int32_t* flag, const hscn_adam* opt,
                                 const hscn_scn_structure* cache, int flags, void* stream_) {
  if (flags & ~HSCN_STORE_F16) return HSCN_E_BADARG;
  if (B < 1 || N < 0 || E < 0) return HSCN_E_BADARG;
  if (cache && !structure_ok(cache, E == 0)) return HSCN_E_BADARG;
  if (opt && (B != 1 || !adam_ok(opt))) return HSCN_E_BADARG;
  if (!hscn_scn_resident_train_step_supported(F, H, K, max_n, max_e)) return HSCN_E_UNSUPPORTED;
  if (!x || !nptr || !eptr || !W_rel || !b_rel || !W_root || !W_mlp || !b_mlp || !stats || !losses || !grads ||
      (B > 1 && !partials) || (E > 0 && !edge_index))
    return HSCN_E_BADARG;
  ScnArgs A = scn_args(x, edge_index, E, nptr, eptr, W_rel, b_rel, W_root, W_mlp, b_mlp, N, B, F, H, K, act, max_n,
                       max_e, stats, losses, ticket, flag);
  A.S = S; A.g_mc = g_mc; A.g_o = g_o;
  A.partials = B == 1 ? grads : partials;   // one graph: its partials are the gradients
  if (cache) set_structure(A, cache);
  if (opt) set_adam(A, opt);
  hipStream_t st = hscn_stream(stream_);
  if (int rc = launch_scn(A, H, flags & HSCN_STORE_F16, SCN_STEP, st)) return rc;
  if (!ticket) {
    k_scn_losses<<<1, 64, 0, st>>>(stats, losses, (int)B);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  if (B > 1) {
    launch_param_fold(partials, grads, (int)B, A.P, -1, 0.f, nullptr, false, st);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

int hscn_scn_resident_fwd(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                          const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                          const float* W_rel, const float* b_rel, const float* W_root, const float* W_mlp,
                          const float* b_mlp, int max_n, int max_e, float* S, void* y, float* stats, float* ss,
                          float* losses, int32_t* ticket, int32_t* ex_rowptr_d, int32_t* ex_col_d,
                          int32_t* ex_rowptr_s, int32_t* ex_col_s, float* ex_agg, float* ex_dout, int32_t* flag,
                          int flags, void* stream_) {
  if (flags & ~HSCN_STORE_F16) return HSCN_E_BADARG;
  if (B < 1 || N < 0 || E < 0) return HSCN_E_BADARG;
  if (!hscn_scn_resident_supported(F, H, K, max_n, max_e)) return HSCN_E_UNSUPPORTED;
  if (!x || !nptr || !eptr || !W_rel || !b_rel || !W_root || !W_mlp || !b_mlp || !S || !y || !stats || !ss ||
      !losses || (E > 0 && !edge_index))
    return HSCN_E_BADARG;
  {
    const int have = (ex_rowptr_d != nullptr) + (ex_col_d != nullptr) + (ex_rowptr_s != nullptr) +
                     (ex_col_s != nullptr) + (ex_agg != nullptr) + (ex_dout != nullptr);
    if (have != 0 && have != 6) return HSCN_E_BADARG;   // the structure is exported whole or not at all
  }
  ScnArgs A = scn_args(x, edge_index, E, nptr, eptr, W_rel, b_rel, W_root, W_mlp, b_mlp, N, B, F, H, K, act, max_n,
                       max_e, stats, losses, ticket, flag);
  A.S = S; A.y = (float*)y; A.ss = ss;
  A.ex_rowptr_d = ex_rowptr_d; A.ex_col_d = ex_col_d; A.ex_rowptr_s = ex_rowptr_s; A.ex_col_s = ex_col_s;
  A.ex_agg = ex_agg; A.ex_dout = ex_dout;
  hipStream_t st = hscn_stream(stream_);
  if (int rc = launch_scn(A, H, flags & HSCN_STORE_F16, SCN_FWD, st)) return rc;
  if (!ticket) {   // no ticket counter: the statistics are reduced by a launch of their own
    k_scn_losses<<<1, 64, 0, st>>>(stats, losses, (int)B);
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

int hscn_scn_resident_bwd(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                          const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                          const float* W_mlp, const float* S, const void* y, const float* stats, const float* ss,
                          const float* g_mc, const float* g_o, const int32_t* ex_rowptr_d, const int32_t* ex_col_d,
                          const int32_t* ex_rowptr_s, const int32_t* ex_col_s, const float* ex_agg,
                          const float* ex_dout, int max_n, int max_e, float* partials, float* grads, int32_t* flag,
                          int flags, void* stream_) {
  if (flags & ~HSCN_STORE_F16) return HSCN_E_BADARG;
  if (B < 1 || N < 0 || E < 0) return HSCN_E_BADARG;
  if (!hscn_scn_resident_supported(F, H, K, max_n, max_e)) return HSCN_E_UNSUPPORTED;
  if (!x || !nptr || !eptr || !W_mlp || !S || !y || !stats || !ss || !partials || !grads ||
      !ex_rowptr_d || !ex_rowptr_s || !ex_agg || !ex_dout || (E > 0 && (!ex_col_d || !ex_col_s)))
    return HSCN_E_BADARG;
  ScnArgs A = scn_args(x, edge_index, E, nptr, eptr, nullptr, nullptr, nullptr, W_mlp, nullptr, N, B, F, H, K, act,
                       max_n, max_e, const_cast<float*>(stats), nullptr, nullptr, flag);
  A.S = const_cast<float*>(S); A.y = (float*)const_cast<void*>(y); A.ss = const_cast<float*>(ss);
  A.g_mc = g_mc; A.g_o = g_o; A.partials = partials;
  A.ex_rowptr_d = const_cast<int32_t*>(ex_rowptr_d); A.ex_col_d = const_cast<int32_t*>(ex_col_d);
  A.ex_rowptr_s = const_cast<int32_t*>(ex_rowptr_s); A.ex_col_s = const_cast<int32_t*>(ex_col_s);
  A.ex_agg = const_cast<float*>(ex_agg); A.ex_dout = const_cast<float*>(ex_dout);
  hipStream_t st = hscn_stream(stream_);
  if (int rc = launch_scn(A, H, flags & HSCN_STORE_F16, SCN_BWD, st)) return rc;
  launch_param_fold(partials, grads, (int)B, A.P, -1, 0.f, nullptr, false, st);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

// A whole run of the reference's stage-A loop (train/train_clustering.py:34-50) from ONE call: `visits` graph visits
// in dataset order, each the one-launch step of ONE graph with the optimizer in its tail and the cached structure
// (hscn_scn_resident_train_step(B = 1, opt, cache) on graph v mod G of a dataset laid out as one batch), issued
// back to back by this host loop -- no Python between two visits -- or, when the model has at most 1024 parameters,
// walked by ONE persistent workgroup (k_scn_epoch: weights in LDS, Adam moments in registers).
int hscn_scn_resident_train_epoch(const void* x, const int32_t* nptr, const int32_t* eptr, int64_t N, int64_t G,
                                  int64_t visits, int F, int H, int K, int act, float* W_rel, float* b_rel,
                                  float* W_root, float* W_mlp, float* b_mlp, const float* g_mc, const float* g_o,
                                  int max_n, int max_e, const hscn_scn_structure* cache, const hscn_adam* opt,
                                  float* grads, float* stats, float* losses, int32_t* ticket, int32_t* flag,
                                  int flags, void* stream_) {
  if (flags & ~HSCN_STORE_F16) return HSCN_E_BADARG;
  const bool f16 = flags & HSCN_STORE_F16;
  if (G < 1 || N < 0 || visits < 0) return HSCN_E_BADARG;
  if (!hscn_scn_resident_train_step_supported(F, H, K, max_n, max_e)) return HSCN_E_UNSUPPORTED;
  if (!x || !nptr || !eptr || !W_rel || !b_rel || !W_root || !W_mlp || !b_mlp || !grads || !stats || !losses || !ticket ||
      !cache || !opt)
    return HSCN_E_BADARG;
  if (!cache->ready || !structure_ok(cache, false)) return HSCN_E_BADARG;
  if (!adam_ok(opt)) return HSCN_E_BADARG;
  // a batch of ONE graph; nptr, eptr and the structure's row pointers stand at graph 0, where the persistent
  // workgroup starts its walk of the dataset
  ScnArgs A = scn_args(x, nullptr, 0, nptr, eptr, W_rel, b_rel, W_root, W_mlp, b_mlp, N, 1, F, H, K, act, max_n, max_e,
                       stats, losses, ticket, flag);
  A.g_mc = g_mc; A.g_o = g_o; A.partials = grads;
  set_structure(A, cache);
  set_adam(A, opt);
  hipStream_t st = hscn_stream(stream_);
  // the chain as launches of ONE persistent workgroup (k_scn_epoch; P <= 1024: a thread per parameter element), in
  // slices of 32 768 visits (~0.5 s) so that no launch runs long enough to look hung; HSCN_PERSISTENT_EPOCH=0 keeps the
  // launch per visit below (the same arithmetic, bit for bit)
  const char* pe = getenv("HSCN_PERSISTENT_EPOCH");
  if (A.P <= SRT && !(pe && pe[0] == '0')) {
    A.G = (int)G;
    const size_t lds = scn_lds_bytes(H, K, max_n, max_e, SCN_STEP);
    for (int64_t v0 = 0; v0 < visits; v0 += 32768) {
      A.visit0 = v0;
      A.visits = visits - v0 < 32768 ? visits - v0 : 32768;
      const int rc = dispatch_scn(H, f16, [&](auto h, auto ts) {
        return launch_with_lds(k_scn_epoch<decltype(h)::value, decltype(ts)>, 1u, SRT, lds, st, A);
      });
      if (rc) return rc;
    }
    return 0;
  }
  for (int64_t v = 0; v < visits; ++v) {
    const int64_t g = v % G;
    // the kernel sees a batch of one graph whose ranges are entries g, g + 1 of the dataset's; the dataset-level
    // structure keeps graph g's row pointers at nptr[g] + g: the + g travels in the base pointers
    A.nptr = nptr + g; A.eptr = eptr + g;
    A.ex_rowptr_d = cache->rowptr_d + g; A.ex_rowptr_s = cache->rowptr_s + g;
    if (int rc = launch_scn(A, H, f16, SCN_STEP, st)) return rc;
  }
  return 0;
}

}  // extern "C"
