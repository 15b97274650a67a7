// One-launch training step of the MPNN baseline (reference model/mpnn.py:46-62 with conv = GCNConv,
// configs/GCN/peptides_func_GCN.yaml; train/train.py:73-95): workgroup g runs the forward of graph g, its row of the
// loss and d loss / d pred, and the backward, with the graph's structure and every activation resident in LDS.  The
// output is one row of per-graph gradient partials [B, P + 1] (loss column last) that k_param_reduce{,_acc} folds in
// a fixed order; that fold also advances the step counter the dropout seeds are derived from.
//
// Semantics (model/mpnn.py; nn/conv.py GCNConv(add_self_loops=True)):
//   hidden layer l < L-1:  a = dropout(act(relu(A_hat a_prev W_l^T + b_l)))
//   last layer:           pred = mean_i (A_hat a W_{L-1}^T + b_{L-1})_i
// A_hat = D^-1/2 (A + I) D^-1/2 over the edge list with its own loops dropped (structure.with_self_loops): the loop
// stays implicit -- rows of the two stable CSRs hold the real neighbours in ascending edge order and the loop term
// dinv_i^2 x_i is added after them, the order the layered kernels sum the appended loop in.
//
// Dropout (nn/functional.py: dropout, csrc/dropout.hip): Philox-4x32-10 keyed by the seed of hidden layer l at step
// t, seed0 + (L-1) t + l, counter = quad index of the element in the batch's row-major [N, H] tensor (global row =
// ptr32[g] + local row), keep iff the draw is >= p 2^32, kept values times 1 / (1 - p).  t is the device step word,
// read when the workgroup starts and advanced by the fold behind this launch.
// The backward does not redraw the mask: with a = keep s act(relu(z)), [a > 0] = keep && z > 0 for every supported
// activation (relu / elu / identity are the identity on relu output, tanh keeps the sign).  tanh's derivative
// 1 - t^2 takes t = a / s (a / 1 = a exactly when p = 0): a = fl(t s), so a / s is t or one of its float neighbours.
//
// LDS (words; RT = 256 threads): per layer Wt [fin][fout] | W [fout][fin] | b [fout] (H x H slots), the degree norm,
// both CSRs (target-keyed rowptr / col for the forward, source-keyed rowptr_t / col_t for A_hat^T), a small scratch
// and L + 1 buffers of n x H words: B0 = features of layer 0 in the forward, the node gradient G in the backward; B1
// = X W^T in the forward, A_hat^T G in the backward; B2 .. BL = a_1 .. a_{L-1}.  The last layer's node output goes to
// B0.  Layer 0's input is loaded again into B2 for its weight gradient (a_1 is dead by then).  The CSR build stages
// its edge lists, counters and slot lists in the buffers, which are not live yet.
#include "resident_common.h"

namespace {

constexpr int MPNN_MAXL = 8;
constexpr int MPNN_RT = 256;

struct MpnnArgs {
  const float* x;             // [N][F]
  const int64_t* ei;          // [2][E] batch node ids, graph g's edges at [eptr[g], eptr[g+1])
  int64_t E, N;
  const int32_t *nptr, *eptr; // [B + 1]
  const float* W[MPNN_MAXL];  // [fout][fin]
  const float* b[MPNN_MAXL];  // [fout]
  const float* target;        // [B][C] or NULL (forward-only without a loss)
  float *pred, *score;        // [B][C] (score optional)
  float* partials;            // TRAIN: [B][P + 1]; forward-only: [B] per-graph summed loss terms (or NULL)
  const uint32_t* step;       // device step counter (NULL: 0)
  int32_t* flag;
  uint64_t seed0;
  uint32_t threshold;         // keep iff draw >= threshold
  float scale;                // 1 / (1 - p)
  int dropout;                // p > 0 (TRAIN only)
  int F, H, L, C, act, max_n, max_ell, P, loss_kind;
  float inv_count;
};

struct MpnnLayout {
  size_t w, dinv, rowptr, col, rowptr_t, col_t, misc, red, buf, bufw, total;
  size_t ek, eo, tmp, cursor;   // CSR build staging (inside the buffers)
};

__host__ __device__ inline MpnnLayout mpnn_layout(int H, int L, int max_n, int max_ell) {
  MpnnLayout Y;
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  size_t o = 0;
  Y.w = o; o += (size_t)L * up4(2 * (size_t)H * H + H);
  Y.dinv = o; o += up4(max_n);
  Y.rowptr = o; o += up4((size_t)max_n + 1);
  Y.col = o; o += up4(max_ell);
  Y.rowptr_t = o; o += up4((size_t)max_n + 1);
  Y.col_t = o; o += up4(max_ell);
  Y.misc = o; o += 4 * 64;                         // pred row | g_pred row | loss terms | target row
  Y.red = o; o += (size_t)MPNN_RT;                 // column-sum partials
  size_t bufw = up4((size_t)max_n * H);
  const size_t stage = 3 * up4(max_ell) + up4((size_t)max_n + 1);
  const size_t nb = (size_t)L + 1;
  if (stage > bufw * nb) bufw = up4((stage + nb - 1) / nb);
  Y.bufw = bufw;
  Y.buf = o; o += bufw * nb;
  Y.ek = Y.buf;
  Y.eo = Y.ek + up4(max_ell);
  Y.tmp = Y.eo + up4(max_ell);
  Y.cursor = Y.tmp + up4(max_ell);
  Y.total = o;
  return Y;
}

inline size_t mpnn_lds_bytes(int H, int L, int max_n, int max_ell) { return mpnn_layout(H, L, max_n, max_ell).total * 4; }

// out[c] = sum_i X[i][c] for c < ncols (ncols <= 16 or <= 32): RT / 16 (or / 32) contiguous row chunks, each summed
// in row order, chunks folded in chunk order -- a fixed summation tree.  Results are valid in threads c < ncols
// after the call (returned); two workgroup barriers.
template <int CP>
__device__ __forceinline__ float mpnn_colsum(const float* X, int n, int ncols, float* red) {
  constexpr int NCH = MPNN_RT / CP;
  const int t = threadIdx.x;
  const int c = t % CP, ch = t / CP;
  const int per = (n + NCH - 1) / NCH;
  const int i0 = ch * per, i1 = i0 + per < n ? i0 + per : n;
  float s = 0.f;
  if (c < ncols)
    for (int i = i0; i < i1; ++i) s += X[i * ncols + c];
  red[t] = s;
  lds_barrier();
  float r = 0.f;
  if (t < ncols)
    for (int q = 0; q < NCH; ++q) r += red[q * CP + t];
  lds_barrier();
  return r;
}

// h[i][o] = sum_k X[i][k] W[o][k] (k ascending), W given transposed: Wt[k][o]
__device__ __forceinline__ void mpnn_transform(const float* X, const float* Wt, float* h, int n, int fin, int fout) {
  for (int idx = threadIdx.x; idx < n * fout; idx += MPNN_RT) {
    const int i = idx / fout, o = idx - i * fout;
    float acc = 0.f;
    for (int k = 0; k < fin; ++k) acc = fmaf(X[i * fin + k], Wt[k * fout + o], acc);
    h[idx] = acc;
  }
}

// y[i][o] = sum_{j in row i} (dinv_j dinv_i) v[j][o] in row order, then + (dinv_i dinv_i) v[i][o]
__device__ __forceinline__ float mpnn_gather(const int* rp, const int* col, const float* dinv, const float* v, int i,
                                             int o, int ncols) {
  const float di = dinv[i];
  float acc = 0.f;
  for (int q = rp[i], e = rp[i + 1]; q < e; ++q) {
    const int j = col[q];
    acc += (dinv[j] * di) * v[j * ncols + o];
  }
  acc += (di * di) * v[i * ncols + o];
  return acc;
}

template <int H, bool TRAIN>
__global__ void __launch_bounds__(MPNN_RT) k_mpnn_step(const MpnnArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* sm = reinterpret_cast<float*>(smem);
  int* si = reinterpret_cast<int*>(smem);
  const int g = blockIdx.x;
  const int t = threadIdx.x;
  const int L = A.L, F = A.F, C = A.C;
  const MpnnLayout Y = mpnn_layout(H, L, A.max_n, A.max_ell);
  const int base = A.nptr[g];
  const int n = A.nptr[g + 1] - base;
  const int e0 = A.eptr[g];
  const int ne = A.eptr[g + 1] - e0;
  const int Ptot = A.P + 1;
  if (base < 0 || n < 0 || n > A.max_n || (int64_t)base + n > A.N || e0 < 0 || ne < 0 || ne > A.max_ell ||
      (int64_t)e0 + ne > A.E) {
    // a graph beyond the capacities this launch was sized for: flagged, its row written as zeros
    if (t == 0 && A.flag) atomicOr(A.flag, 2);
    if (TRAIN) {
      for (int p = t; p < Ptot; p += MPNN_RT) A.partials[(size_t)g * Ptot + p] = 0.f;
    } else if (A.partials && t == 0) {
      A.partials[g] = 0.f;
    }
    for (int c = t; c < C; c += MPNN_RT) {
      A.pred[(size_t)g * C + c] = 0.f;
      if (A.score) A.score[(size_t)g * C + c] = 0.f;
    }
    return;
  }
  const uint32_t step = (TRAIN && A.step) ? A.step[0] : 0u;
  float* buf0 = sm + Y.buf;
  float* buf1 = buf0 + Y.bufw;
  auto xbuf = [&](int l) { return buf0 + (size_t)(l + 1) * Y.bufw; };   // a_l, l = 1 .. L-1
  float* dinv = sm + Y.dinv;
  int* rp = si + Y.rowptr;
  int* col = si + Y.col;
  int* rpt = si + Y.rowptr_t;
  int* colt = si + Y.col_t;
  float* misc = sm + Y.misc;
  float* red = sm + Y.red;
  int* ek = si + Y.ek;
  int* eo = si + Y.eo;
  int* tmp = si + Y.tmp;
  int* cursor = si + Y.cursor;

  // ---- weights (Wt and W per layer), edge staging (loops and out-of-graph ids dropped) ----
  for (int l = 0; l < L; ++l) {
    const int fin = l == 0 ? F : H, fout = l == L - 1 ? C : H;
    float* w = sm + Y.w + (size_t)l * ((2 * H * H + H + 3) & ~3);
    for (int q = t; q < fout * fin; q += MPNN_RT) {
      const int o = q / fin, k = q - o * fin;
      const float v = A.W[l][q];
      w[k * fout + o] = v;
      w[H * H + q] = v;
    }
    for (int o = t; o < fout; o += MPNN_RT) w[2 * H * H + o] = A.b[l][o];
  }
  for (int e = t; e < ne; e += MPNN_RT) {
    const int64_t s = A.ei[e0 + e] - base, d = A.ei[A.E + e0 + e] - base;
    const bool ok = s >= 0 && s < n && d >= 0 && d < n;
    if (!ok && A.flag) atomicOr(A.flag, 1);
    const bool keep = ok && s != d;
    ek[e] = keep ? (int)d : -1;
    eo[e] = keep ? (int)s : -1;
  }
  for (int i = t; i <= n; i += MPNN_RT) cursor[i] = 0;
  lds_barrier();
  const Grp G{t, MPNN_RT, t >> 6, MPNN_RT / 64};
  build_csr_lds(ek, eo, ne, n, rp, col, cursor, tmp, G, false);     // keyed by target: the forward's rows
  build_csr_lds(eo, ek, ne, n, rpt, colt, cursor, tmp, G, false);   // keyed by source: rows of A_hat^T
  for (int i = t; i < n; i += MPNN_RT) {
    const int d = rp[i + 1] - rp[i] + 1;                                // + the loop
    dinv[i] = 1.0f / sqrtf((float)d);
  }
  // ---- layer 0's input ----
  for (int q = t; q < n * F; q += MPNN_RT) buf0[q] = A.x[(size_t)base * F + q];
  lds_barrier();

  // ---- forward ----
  for (int l = 0; l < L; ++l) {
    const int fin = l == 0 ? F : H, fout = l == L - 1 ? C : H;
    const float* w = sm + Y.w + (size_t)l * ((2 * H * H + H + 3) & ~3);
    const float* X = l == 0 ? buf0 : xbuf(l);
    mpnn_transform(X, w, buf1, n, fin, fout);
    lds_barrier();
    if (l < L - 1) {
      float* out = xbuf(l + 1);
      const uint64_t seed = A.seed0 + (uint64_t)(L - 1) * step + (uint64_t)l;
      for (int idx = t; idx < n * H; idx += MPNN_RT) {
        const int i = idx / H, o = idx - i * H;
        const float z = mpnn_gather(rp, col, dinv, buf1, i, o, H) + w[2 * H * H + o];
        float a = z > 0.f ? z : 0.f;
        if (A.act == HSCN_ACT_TANH) a = tanhf(a);
        if (TRAIN && A.dropout) {
          const uint64_t gi = (uint64_t)(base + i) * H + o;
          uint32_t c[4];
          philox4x32_10(seed, gi >> 2, c);
          const int k = (int)(gi & 3);
          const uint32_t r = k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3];
          a = r >= A.threshold ? a * A.scale : 0.f;
        }
        out[idx] = a;
      }
    } else {
      for (int idx = t; idx < n * C; idx += MPNN_RT) {
        const int i = idx / C, o = idx - i * C;
        buf0[idx] = mpnn_gather(rp, col, dinv, buf1, i, o, C) + w[2 * H * H + o];
      }
    }
    lds_barrier();
  }

  // ---- mean pool, loss row ----
  const float cnt = (float)(n > 0 ? n : 1);
  const float psum = mpnn_colsum<16>(buf0, n, C, red);   // (C <= H; H = 32 checks C <= 16 on the host)
  float* gp = misc + 64;
  float* lt_row = misc + 128;
  if (t < C) {
    const float pc = psum / cnt;
    A.pred[(size_t)g * C + t] = pc;
    float lt = 0.f, sg = 1.0f / (1.0f + expf(-pc)), gg = 0.f;
    if (A.target) criterion_elem(A.loss_kind, pc, A.target[(size_t)g * C + t], A.inv_count, lt, sg, gg);
    if (A.score) A.score[(size_t)g * C + t] = sg;
    gp[t] = gg;
    lt_row[t] = lt;
  }
  lds_barrier();
  if (t == 0 && A.target && (TRAIN || A.partials)) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += lt_row[c];                       // loss terms in class order
    if (TRAIN) A.partials[(size_t)g * Ptot + A.P] = s;
    else A.partials[g] = s;
  }
  if (!TRAIN) return;

  // ---- backward ----
  // d loss / d (last layer's node output): g_pred / n at every node
  for (int idx = t; idx < n * C; idx += MPNN_RT) {
    const int o = idx % C;
    buf0[idx] = gp[o] / cnt;
  }
  lds_barrier();
  float* part = A.partials + (size_t)g * Ptot;
  int off = A.P;
  for (int l = L - 1; l >= 0; --l) {
    const int fin = l == 0 ? F : H, fout = l == L - 1 ? C : H;
    const float* w = sm + Y.w + (size_t)l * ((2 * H * H + H + 3) & ~3);
    off -= fout * fin + fout;
    // Gh = A_hat^T G
    for (int idx = t; idx < n * fout; idx += MPNN_RT) {
      const int j = idx / fout, o = idx - j * fout;
      buf1[idx] = mpnn_gather(rpt, colt, dinv, buf0, j, o, fout);
    }
    if (l == 0)   // layer 0's input again (a_1, which B2 held, is dead)
      for (int q = t; q < n * F; q += MPNN_RT) xbuf(1)[q] = A.x[(size_t)base * F + q];
    // bias gradient: column sums of G (barriers inside)
    const float gb = H == 16 || fout <= 16 ? mpnn_colsum<16>(buf0, n, fout, red) : mpnn_colsum<32>(buf0, n, fout, red);
    if (t < fout) part[off + fout * fin + t] = gb;
    // weight gradient gW[o][k] = sum_j Gh[j][o] X[j][k]
    const float* X = xbuf(l == 0 ? 1 : l);
    for (int q = t; q < fout * fin; q += MPNN_RT) {
      const int o = q / fin, k = q - o * fin;
      float acc = 0.f;
      for (int j = 0; j < n; ++j) acc = fmaf(buf1[j * fout + o], X[j * fin + k], acc);
      part[off + q] = acc;
    }
    if (l == 0) break;
    // input gradient through W, then dropout, activation and ReLU: G = (Gh W) s [a > 0] act'
    const float* Wl = w + H * H;   // W [fout][fin]
    const bool tanh_act = A.act == HSCN_ACT_TANH;
    for (int idx = t; idx < n * H; idx += MPNN_RT) {
      const int j = idx / H, k = idx - j * H;
      float acc = 0.f;
      for (int o = 0; o < fout; ++o) acc = fmaf(buf1[j * fout + o], Wl[o * fin + k], acc);
      const float a = X[idx];
      float v = 0.f;
      if (a > 0.f) {
        v = A.dropout ? acc * A.scale : acc;
        if (tanh_act) {
          const float tv = A.dropout ? a / A.scale : a;
          v = v * (1.f - tv * tv);
        }
      }
      buf0[idx] = v;
    }
    lds_barrier();
  }
}

template <int H, bool TRAIN>
int launch_mpnn(const MpnnArgs& A, int64_t B, hipStream_t st) {
  const size_t lds = mpnn_lds_bytes(H, A.L, A.max_n, A.max_ell);
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  return launch_with_lds(k_mpnn_step<H, TRAIN>, (unsigned)B, MPNN_RT, lds, st, A);
}

int fill_mpnn_args(MpnnArgs& A, const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                   const int32_t* eptr32, int64_t N, int F, int H, int L, int C, int act,
                   const void* const* params_host, int max_n, int max_ell, const float* target, int loss_kind,
                   float inv_count, float* pred, float* score, int32_t* flag);

}  // namespace

extern "C" {

int hscn_mpnn_supported(int F, int H, int L, int C, int max_n, int max_ell) {
  if (!(H == 16 || H == 32) || F < 1 || F > H || L < 2 || L > MPNN_MAXL || C < 1 || C > H || C > 16) return 0;
  if (max_n < 0 || max_ell < 0 || max_n > (1 << 20) || max_ell > (1 << 22)) return 0;
  return mpnn_lds_bytes(H, L, max_n, max_ell) <= LDS_CU_BYTES ? 1 : 0;
}

int64_t hscn_mpnn_param_count(int F, int H, int L, int C) {
  int64_t P = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t fin = l == 0 ? F : H, fout = l == L - 1 ? C : H;
    P += fout * fin + fout;
  }
  return P;
}

}  // extern "C"

namespace {

int fill_mpnn_args(MpnnArgs& A, const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                   const int32_t* eptr32, int64_t N, int F, int H, int L, int C, int act,
                   const void* const* params_host, int max_n, int max_ell, const float* target, int loss_kind,
                   float inv_count, float* pred, float* score, int32_t* flag) {
  if (N < 0 || E < 0 || !ptr32 || !eptr32 || !params_host || !pred || (N > 0 && !x) || (E > 0 && !edge_index))
    return HSCN_E_BADARG;
  if (act != HSCN_ACT_IDENTITY && act != HSCN_ACT_RELU && act != HSCN_ACT_ELU && act != HSCN_ACT_TANH)
    return HSCN_E_BADARG;
  if (target && loss_kind != 0 && loss_kind != 1) return HSCN_E_BADARG;
  if (!hscn_mpnn_supported(F, H, L, C, max_n, max_ell)) return HSCN_E_UNSUPPORTED;
  A = MpnnArgs{};
  A.x = x; A.ei = edge_index; A.E = E; A.N = N; A.nptr = ptr32; A.eptr = eptr32;
  for (int l = 0; l < L; ++l) {
    if (!params_host[2 * l] || !params_host[2 * l + 1]) return HSCN_E_BADARG;
    A.W[l] = (const float*)params_host[2 * l];
    A.b[l] = (const float*)params_host[2 * l + 1];
  }
  A.target = target; A.pred = pred; A.score = score; A.flag = flag;
  A.F = F; A.H = H; A.L = L; A.C = C; A.act = act; A.max_n = max_n; A.max_ell = max_ell;
  A.P = (int)hscn_mpnn_param_count(F, H, L, C);
  A.loss_kind = loss_kind; A.inv_count = inv_count;
  return 0;
}

}  // namespace

extern "C" {

int hscn_mpnn_train_step(const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                         const int32_t* eptr32, int64_t N, int64_t B, int F, int H, int L, int C, int act,
                         const void* const* params_host, int max_n, int max_ell, const float* target, int loss_kind,
                         float inv_count, float* pred, float* score, float* partials, float* grads, uint32_t* step,
                         float p, uint64_t seed0, int32_t* flag, int flags, void* stream_) {
  if (flags & ~HSCN_GRAD_ACCUMULATE) return HSCN_E_BADARG;
  if (B < 0 || !target || !partials || !grads || !(p >= 0.f && p < 1.f)) return HSCN_E_BADARG;
  if (B == 0) return 0;
  MpnnArgs A;
  if (int rc = fill_mpnn_args(A, x, edge_index, E, ptr32, eptr32, N, F, H, L, C, act, params_host, max_n, max_ell,
                              target, loss_kind, inv_count, pred, score, flag))
    return rc;
  A.partials = partials; A.step = step; A.seed0 = seed0;
  A.dropout = p > 0.f ? 1 : 0;
  dropout_keep_rule(p, A.threshold, A.scale);
  hipStream_t st = hscn_stream(stream_);
  const int rc = H == 16 ? launch_mpnn<16, true>(A, B, st) : launch_mpnn<32, true>(A, B, st);
  if (rc) return rc;
  launch_param_fold(partials, grads, (int)B, A.P + 1, A.P, inv_count, step, flags & HSCN_GRAD_ACCUMULATE, st);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_mpnn_forward(const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                      const int32_t* eptr32, int64_t N, int64_t B, int F, int H, int L, int C, int act,
                      const void* const* params_host, int max_n, int max_ell, const float* target, int loss_kind,
                      float inv_count, float* pred, float* score, float* loss_rows, float* loss, int32_t* flag,
                      void* stream_) {
  if (B < 0 || (loss && (!loss_rows || !target))) return HSCN_E_BADARG;
  if (B == 0) return 0;
  MpnnArgs A;
  if (int rc = fill_mpnn_args(A, x, edge_index, E, ptr32, eptr32, N, F, H, L, C, act, params_host, max_n, max_ell,
                              target, loss_kind, inv_count, pred, score, flag))
    return rc;
  A.partials = target ? loss_rows : nullptr;
  hipStream_t st = hscn_stream(stream_);
  const int rc = H == 16 ? launch_mpnn<16, false>(A, B, st) : launch_mpnn<32, false>(A, B, st);
  if (rc) return rc;
  if (loss) k_param_reduce<<<1, 256, 0, st>>>(loss_rows, loss, (int)B, 1, 0, inv_count, nullptr);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
