// One-launch forward of the SignNet node encoder (graph_hscn/encoder/signnet.py: SignNetNodeEncoder with the
// DeepSet model, use_bn = False, gradients off): workgroup g encodes graph g with its structure in LDS and writes
// its rows of the new feature tensor [linear_x(x) | pe].
//
// Semantics.  phi = GIN(1, Hd, Od, layers) is Lc = max(layers, 2) GINConv's, y = nn(x_i + sum_{j -> i} x_j) over the
// edge list as given (duplicates and loops count as edges, nothing is added); their nn's are Linear(1, Hd),
// Lc - 2 times Linear(Hd, Hd), and Linear(Hd, Hd) -> ReLU -> Linear(Hd, Od).  No activation, normalisation or
// dropout sits between the convolutions, so everything in front of that one ReLU is linear in the scalar input of a
// channel.  With P = I + A (A[i][j] = number of edges j -> i):
//     pre_i = (P^Lc v)_i U + sum_l (P^(Lc-1-l) 1)_i V_l,    U = W_(Lc-1) .. W_1 w_0,   V_l = W_(Lc-1) .. W_(l+1) b_l
// for an eigenvector v (one channel of eigvecs_sn, NaN padding read as 0).  The V part, c_i [Hd], does not depend
// on the channel or its sign; phi(v) + phi(-v) = Wb (relu(c + q U) + relu(c - q U)) + 2 bb with q = P^Lc v.  The
// DeepSet sum over the frequencies k < min(K, n) moves in front of Wb:
//     acc_i = sum_k relu(c_i + q_ik U) + relu(c_i - q_ik U),   enc_i = Wb acc_i + 2 min(K, n) bb,
// then rho (post_layers Linear's, ReLU between them) gives pe_i, and out_i = [Wx x_i + bx | pe_i].
// What the layered path walks as 2 K passes over [n, Hd] activations is here Lc gathers over [n, K] scalars, one
// [n, Hd] table and small dense tails; the result differs from the layered one by the association of the products
// only (tests hold it to the float64 evaluation of the chain).
//
// LDS (words; SN_RT = 256 threads): the two vector tables {U, V_0 ..}, target-keyed CSR (rowptr / col), two scalar
// fields P^j 1, two [n, K] channel fields, the rho tile buffers, and c / acc [n, Hd].  The CSR build stages its
// edge lists, counters and slot lists in the c buffer, which is not live yet.
#include "resident_common.h"

namespace {

constexpr int SN_RT = 256;
constexpr int SN_MAXC = 8;      // GINConv's
constexpr int SN_MAXR = 8;      // rho layers
constexpr int SN_MAXW = 64;     // widest hidden / output vector
constexpr int SN_TR = 32;       // rows per tile of the dense tail

struct SnArgs {
  const float* x;               // [N][F]
  const float* vec;             // [N][K] eigvecs_sn
  const int64_t* ei;            // [2][E] batch node ids, graph g's edges at [eptr[g], eptr[g+1])
  int64_t E, N;
  const int32_t *nptr, *eptr;   // [B + 1]
  const float* Ws[SN_MAXC];     // Ws[0] = w_0 [Hd][1]; then [Hd][Hd]
  const float* bs[SN_MAXC];     // [Hd]
  const float *Wb, *bb;         // [Od][Hd], [Od]
  const float* Wr[SN_MAXR];     // rho: [fout][fin]
  const float* br[SN_MAXR];
  const float *Wx, *bx;         // [dx][F], [dx]; NULL: x is copied (dx = F)
  float *out, *pe;              // [N][dx + dim_pe]; [N][dim_pe] or NULL
  int32_t* flag;
  int F, K, Hd, Od, Lc, R, dim_pe, dx, max_n, max_e;
};

struct SnLayout {
  size_t vecA, vecB, rowptr, col, f0, f1, q0, q1, tile, c, total;
  size_t ek, eo, tmp, cursor;   // CSR build staging (inside c)
  int tw;                       // row stride of a tile buffer
};

__host__ __device__ inline SnLayout sn_layout(int K, int Hd, int Od, int Lc, int dim_pe, int max_n, int max_e) {
  SnLayout Y;
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  size_t o = 0;
  Y.vecA = o; o += up4((size_t)(Lc + 1) * Hd);
  Y.vecB = o; o += up4((size_t)(Lc + 1) * Hd);
  Y.rowptr = o; o += up4((size_t)max_n + 1);
  Y.col = o; o += up4(max_e);
  Y.f0 = o; o += up4(max_n);
  Y.f1 = o; o += up4(max_n);
  Y.q0 = o; o += up4((size_t)max_n * K);
  Y.q1 = o; o += up4((size_t)max_n * K);
  int tw = Hd > Od ? Hd : Od;
  if (dim_pe > tw) tw = dim_pe;
  Y.tw = tw;
  Y.tile = o; o += 2 * (size_t)SN_TR * tw;
  const size_t stage = 3 * up4(max_e) + up4((size_t)max_n + 1);
  size_t cw = up4((size_t)max_n * Hd);
  if (stage > cw) cw = stage;
  Y.c = o; o += cw;
  Y.ek = Y.c;
  Y.eo = Y.ek + up4(max_e);
  Y.tmp = Y.eo + up4(max_e);
  Y.cursor = Y.tmp + up4(max_e);
  Y.total = o;
  return Y;
}

inline size_t sn_lds_bytes(int K, int Hd, int Od, int Lc, int dim_pe, int max_n, int max_e) {
  return sn_layout(K, Hd, Od, Lc, dim_pe, max_n, max_e).total * 4;
}

__global__ void __launch_bounds__(SN_RT) k_signnet_encode(const SnArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* sm = reinterpret_cast<float*>(smem);
  int* si = reinterpret_cast<int*>(smem);
  const int g = blockIdx.x;
  const int t = threadIdx.x;
  const int K = A.K, Hd = A.Hd, Od = A.Od, Lc = A.Lc, F = A.F, dx = A.dx, dpe = A.dim_pe;
  const int ow = dx + dpe;
  const SnLayout Y = sn_layout(K, Hd, Od, Lc, dpe, A.max_n, A.max_e);
  const int base = A.nptr[g];
  const int n = A.nptr[g + 1] - base;
  const int e0 = A.eptr[g];
  const int ne = A.eptr[g + 1] - e0;
  if (base < 0 || n < 0 || n > A.max_n || (int64_t)base + n > A.N || e0 < 0 || ne < 0 || ne > A.max_e ||
      (int64_t)e0 + ne > A.E) {
    // a graph beyond the capacities this launch was sized for: flagged, the rows it names inside the arrays are zeros
    if (t == 0 && A.flag) atomicOr(A.flag, 2);
    const int64_t lo = base > 0 ? base : 0;
    int64_t hi = (int64_t)base + (n > 0 ? n : 0);
    if (hi > A.N) hi = A.N;
    for (int64_t r = lo; r < hi; ++r) {
      for (int c = t; c < ow; c += SN_RT) A.out[r * ow + c] = 0.f;
      if (A.pe)
        for (int c = t; c < dpe; c += SN_RT) A.pe[r * dpe + c] = 0.f;
    }
    return;
  }
  int* rp = si + Y.rowptr;
  int* col = si + Y.col;
  int* ek = si + Y.ek;
  int* eo = si + Y.eo;
  int* tmp = si + Y.tmp;
  int* cursor = si + Y.cursor;
  float* cb = sm + Y.c;

  // ---- edge staging (ids outside the graph dropped and flagged; loops and repeats stay), target-keyed CSR ----
  for (int e = t; e < ne; e += SN_RT) {
    const int64_t s = A.ei[e0 + e] - base, d = A.ei[A.E + e0 + e] - base;
    const bool ok = s >= 0 && s < n && d >= 0 && d < n;
    if (!ok && A.flag) atomicOr(A.flag, 1);
    ek[e] = ok ? (int)d : -1;
    eo[e] = ok ? (int)s : -1;
  }
  for (int i = t; i <= n; i += SN_RT) cursor[i] = 0;
  lds_barrier();
  const Grp G{t, SN_RT, t >> 6, SN_RT / 64};
  build_csr_lds(ek, eo, ne, n, rp, col, cursor, tmp, G, false);

  // ---- the vector table {U, V_0 .. V_(Lc-1)}, the channel fields q = v and the scalar field 1 ----
  float* vcur = sm + Y.vecA;
  float* vnxt = sm + Y.vecB;
  for (int o = t; o < Hd; o += SN_RT) {
    vcur[o] = A.Ws[0][o];
    vcur[Hd + o] = A.bs[0][o];
  }
  float* q = sm + Y.q0;
  float* qn = sm + Y.q1;
  float* f = sm + Y.f0;
  float* fn = sm + Y.f1;
  for (int idx = t; idx < n * K; idx += SN_RT) {
    const float v = A.vec[(size_t)base * K + idx];
    q[idx] = v != v ? 0.f : v;
  }
  for (int i = t; i < n; i += SN_RT) f[i] = 1.f;
  lds_barrier();
  for (int l = 1; l < Lc; ++l) {
    const float* W = A.Ws[l];
    const int nv = l + 1;
    for (int idx = t; idx < nv * Hd; idx += SN_RT) {
      const int v = idx / Hd, o = idx - v * Hd;
      float acc = 0.f;
      for (int k = 0; k < Hd; ++k) acc = fmaf(W[o * Hd + k], vcur[v * Hd + k], acc);
      vnxt[idx] = acc;
    }
    for (int o = t; o < Hd; o += SN_RT) vnxt[nv * Hd + o] = A.bs[l][o];
    lds_barrier();
    float* sw = vcur; vcur = vnxt; vnxt = sw;
  }
  const float* U = vcur;

  // ---- Lc aggregation steps: c += (P^s 1) V_(Lc-1-s);  q <- P q;  1-field <- P (1-field) ----
  for (int s = 0; s < Lc; ++s) {
    const float* V = vcur + (size_t)(1 + (Lc - 1 - s)) * Hd;
    for (int idx = t; idx < n * Hd; idx += SN_RT) {
      const int i = idx / Hd, h = idx - i * Hd;
      const float add = f[i] * V[h];
      cb[idx] = s == 0 ? add : cb[idx] + add;
    }
    for (int idx = t; idx < n * K; idx += SN_RT) {
      const int i = idx / K, k = idx - i * K;
      float acc = q[idx];
      for (int p = rp[i], pe = rp[i + 1]; p < pe; ++p) acc += q[col[p] * K + k];
      qn[idx] = acc;
    }
    if (s + 1 < Lc)
      for (int i = t; i < n; i += SN_RT) {
        float acc = f[i];
        for (int p = rp[i], pe = rp[i + 1]; p < pe; ++p) acc += f[col[p]];
        fn[i] = acc;
      }
    lds_barrier();
    float* sw = q; q = qn; qn = sw;
    sw = f; f = fn; fn = sw;
  }

  // ---- acc_i = sum over the graph's frequencies of relu(c + q U) + relu(c - q U)   (in place of c) ----
  const int cnt = K < n ? K : n;
  for (int idx = t; idx < n * Hd; idx += SN_RT) {
    const int i = idx / Hd, h = idx - i * Hd;
    const float cc = cb[idx], u = U[h];
    float acc = 0.f;
    for (int k = 0; k < cnt; ++k) {
      const float a = q[i * K + k] * u;
      const float zp = cc + a, zm = cc - a;
      acc += (zp > 0.f ? zp : 0.f) + (zm > 0.f ? zm : 0.f);
    }
    cb[idx] = acc;
  }
  lds_barrier();

  // ---- dense tail in tiles of SN_TR rows: enc = Wb acc + 2 cnt bb, rho, pe written behind linear_x's columns ----
  const int tw = Y.tw;
  const float bscale = 2.f * (float)cnt;
  for (int r0 = 0; r0 < n; r0 += SN_TR) {
    const int rows = n - r0 < SN_TR ? n - r0 : SN_TR;
    float* in = sm + Y.tile;
    float* ot = in + (size_t)SN_TR * tw;
    for (int idx = t; idx < rows * Od; idx += SN_RT) {
      const int r = idx / Od, o = idx - r * Od;
      const float* a = cb + (size_t)(r0 + r) * Hd;
      float acc = 0.f;
      for (int k = 0; k < Hd; ++k) acc = fmaf(a[k], A.Wb[o * Hd + k], acc);
      in[r * tw + o] = acc + bscale * A.bb[o];
    }
    lds_barrier();
    for (int l = 0; l < A.R; ++l) {
      const int fin = l == 0 ? Od : Hd, fout = l == A.R - 1 ? dpe : Hd;
      const float* W = A.Wr[l];
      const float* b = A.br[l];
      const bool last = l == A.R - 1;
      for (int idx = t; idx < rows * fout; idx += SN_RT) {
        const int r = idx / fout, o = idx - r * fout;
        float acc = 0.f;
        for (int k = 0; k < fin; ++k) acc = fmaf(in[r * tw + k], W[o * fin + k], acc);
        acc += b[o];
        if (last) {
          const size_t row = (size_t)base + r0 + r;
          A.out[row * ow + dx + o] = acc;
          if (A.pe) A.pe[row * dpe + o] = acc;
        } else {
          ot[r * tw + o] = acc > 0.f ? acc : 0.f;
        }
      }
      lds_barrier();
      float* sw = in; in = ot; ot = sw;
    }
  }

  // ---- linear_x into the leading columns ----
  for (int idx = t; idx < n * dx; idx += SN_RT) {
    const int i = idx / dx, o = idx - i * dx;
    const float* xr = A.x + ((size_t)base + i) * F;
    float v;
    if (A.Wx) {
      float acc = 0.f;
      for (int k = 0; k < F; ++k) acc = fmaf(xr[k], A.Wx[o * F + k], acc);
      v = acc + A.bx[o];
    } else {
      v = xr[o];
    }
    A.out[((size_t)base + i) * ow + o] = v;
  }
}

}  // namespace

extern "C" {

int hscn_signnet_supported(int model, int use_bn, int F, int K, int hidden, int phi_out, int layers, int post_layers,
                           int dim_pe, int dim_x, int max_n, int max_e) {
  if (model != HSCN_SIGNNET_DEEPSET || use_bn) return 0;
  if (F < 1 || F > 1024 || dim_x < 1 || dim_x > 1024 || K < 1 || K > 64) return 0;
  if (hidden < 1 || hidden > SN_MAXW || phi_out < 1 || phi_out > SN_MAXW || dim_pe < 1 || dim_pe > SN_MAXW) return 0;
  if (layers < 1 || layers > SN_MAXC || post_layers < 1 || post_layers > SN_MAXR) return 0;
  if (max_n < 0 || max_e < 0 || max_n > (1 << 20) || max_e > (1 << 22)) return 0;
  const int Lc = layers < 2 ? 2 : layers;
  return sn_lds_bytes(K, hidden, phi_out, Lc, dim_pe, max_n, max_e) <= LDS_CU_BYTES ? 1 : 0;
}

int hscn_signnet_encode(const float* x, const float* eigvecs, const int64_t* edge_index, int64_t E,
                        const int32_t* ptr32, const int32_t* eptr32, int64_t N, int64_t B, int F, int K, int hidden,
                        int phi_out, int layers, int post_layers, int dim_pe, int dim_x, int expand_x,
                        const void* const* params_host, int max_n, int max_e, float* out, float* pe, int32_t* flag,
                        void* stream_) {
  if (N < 0 || E < 0 || B < 0 || !ptr32 || !eptr32 || !params_host || (N > 0 && (!x || !eigvecs || !out)) ||
      (E > 0 && !edge_index))
    return HSCN_E_BADARG;
  if (F < 1 || K < 1 || hidden < 1 || phi_out < 1 || layers < 1 || post_layers < 1 || dim_pe < 1 || dim_x < 1 ||
      max_n < 0 || max_e < 0 || (!expand_x && dim_x != F))
    return HSCN_E_BADARG;
  if (!hscn_signnet_supported(HSCN_SIGNNET_DEEPSET, 0, F, K, hidden, phi_out, layers, post_layers, dim_pe, dim_x,
                              max_n, max_e))
    return HSCN_E_UNSUPPORTED;
  SnArgs A{};
  const int Lc = layers < 2 ? 2 : layers;
  int p = 0;
  for (int l = 0; l < Lc; ++l) {
    A.Ws[l] = (const float*)params_host[p++];
    A.bs[l] = (const float*)params_host[p++];
    if (!A.Ws[l] || !A.bs[l]) return HSCN_E_BADARG;
  }
  A.Wb = (const float*)params_host[p++];
  A.bb = (const float*)params_host[p++];
  if (!A.Wb || !A.bb) return HSCN_E_BADARG;
  for (int l = 0; l < post_layers; ++l) {
    A.Wr[l] = (const float*)params_host[p++];
    A.br[l] = (const float*)params_host[p++];
    if (!A.Wr[l] || !A.br[l]) return HSCN_E_BADARG;
  }
  if (expand_x) {
    A.Wx = (const float*)params_host[p++];
    A.bx = (const float*)params_host[p++];
    if (!A.Wx || !A.bx) return HSCN_E_BADARG;
  }
  if (B == 0 || N == 0) return 0;
  A.x = x; A.vec = eigvecs; A.ei = edge_index; A.E = E; A.N = N; A.nptr = ptr32; A.eptr = eptr32;
  A.out = out; A.pe = pe; A.flag = flag;
  A.F = F; A.K = K; A.Hd = hidden; A.Od = phi_out; A.Lc = Lc; A.R = post_layers; A.dim_pe = dim_pe; A.dx = dim_x;
  A.max_n = max_n; A.max_e = max_e;
  const size_t lds = sn_lds_bytes(K, hidden, phi_out, Lc, dim_pe, max_n, max_e);
  return launch_with_lds(k_signnet_encode, (unsigned)B, SN_RT, lds, hscn_stream(stream_), A);
}

}  // extern "C"
