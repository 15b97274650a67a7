// One-launch training step of HSCN with the opt-in virtual -> local relation (graph_hscn.model.hscn.HSCN(vl_conv="GAT")):
// workgroup g runs the forward of graph g on BOTH node types, its row of the loss and d loss / d pred, and the backward
// through all four relations, with the graph's structure in LDS.  The output is one row of per-graph gradient partials
// [B, P + 1] (loss column last) that k_param_reduce{,_acc} folds in graph order.
//
// Semantics (model/hscn.py with the fourth HeteroConv entry; nn/conv.py GCNConv / GATConv, add_self_loops=False):
//   x_l' = relu((A_ll (x_l W_ll^T) + b_ll) + ((x_v W_vl,src^T)[c(i)] + b_vl))
//   x_v' = relu((A_vv (x_v W_vv^T) + b_vv) + (sum_{i in v} alpha_i (x_l W_lv,src^T)_i + b_lv))
// A_* = D^-1/2 A D^-1/2 over the edge list as given (in-degree; loops and repeated edges are ordinary edges; in-degree
// 0 gives dinv = 0).  alpha = segment softmax over the members of cluster v of leaky_relu(a_src[i] + a_dst[v], slope),
// a_src = (x_l W_lv,src^T) . att_src, a_dst = (x_v W_lv,dst^T) . att_dst (max subtracted, + 1e-16 in the denominator).
// c(i) = the target of local node i's ONE local -> virtual edge: the virtual -> local relation is that edge reversed, its
// softmax runs over one score, alpha = 1, so the relation is lin_src(x_v)[c(i)] + b_vl and its lin_dst / att_src /
// att_dst receive exactly zero gradients.  A node without such an edge receives b_vl only; a node with several is
// flagged (bit 16).  The last layer's virtual update does not reach the prediction: the step skips it and writes zeros
// into its parameters' columns (the Python step leaves those parameters' .grad at None, as autograd does).
//
// Parameter pointers, per layer (fin = F for layer 0, else H): W_ll [H,fin], b_ll, W_vv, b_vv, lv {W_src, W_dst,
// att_src, att_dst, b}, vl {W_src, W_dst, att_src, att_dst, b}; then W1, b1, W2, b2.  The gradient columns follow that
// order except that the last layer's dead part (vv, lv) comes after the head, so that the live gradients tile the
// front of the flat buffer (what optim.FlatAdam takes).
//
// LDS (words; RT = 256 threads): the current layer's weights (six H x H slots + vectors, reloaded per layer: the
// forward takes them transposed, the backward as stored), both degree norms, the ll and vv CSRs by target and by source,
// the cluster id per local node and the member list per cluster, per layer alpha and the leaky slope factor per local
// node, per layer the virtual input features, four V x H work arrays, and three buffers of n x H words:
//   forward:  B0 = x_l (then x_l' in place), B1 = x_l W_ll^T, B2 = x_l W_lv,src^T
//   backward: B0 = node gradient, B1 = A_ll^T G, then the recomputed x_l W_lv,src^T and its gradient, B2 = x_l
// The local activations x_1 .. x_{L-1} the backward reads again go to an HBM workspace [(L-1), N, H]; x_L stays in B0.
// Every sum has a fixed order (rows in edge order, members in edge order, chunked column sums); no float atomics.
#include "resident_common.h"

namespace {

constexpr int VL_MAXL = 8;
constexpr int VL_RT = 256;
constexpr int VL_NP = 14;   // parameters per layer
enum { VP_WLL, VP_BLL, VP_WVV, VP_BVV, VP_LVS, VP_LVD, VP_LVAS, VP_LVAD, VP_LVB, VP_VLS, VP_VLD, VP_VLAS, VP_VLAD, VP_VLB };

struct VlArgs {
  const float *xl, *xv;                       // [N][F], [V][F]
  const int64_t *ei_ll, *ei_vv, *ei_lv;       // [2][E_*] batch node ids
  int64_t E_ll, E_vv, E_lv, N, V;
  const int32_t *lptr, *vptr, *eptr_ll, *eptr_vv, *eptr_lv;   // [B + 1]
  const float* p[VL_MAXL][VL_NP];
  const float *W1, *b1, *W2, *b2;
  const float* target;                        // [B][C] or NULL (forward-only without a loss)
  float *pred, *score;                        // [B][C] (score optional)
  float* partials;                            // TRAIN: [B][P + 1]; forward-only: [B] summed loss terms (or NULL)
  float* ws;                                  // TRAIN: [(L-1)][N][H]
  float* xv_out;                              // [V][H] final virtual features (or NULL)
  int32_t* flag;
  int F, H, L, C, act, max_n, max_v, max_ell, max_evv, P, loss_kind;
  float slope, inv_count;
};

struct VlLayout {
  size_t w, vec, dinv_l, dinv_v, rp, col, rpt, colt, vrp, vcol, vrpt, vcolt, cl, mrp, mcol, alpha, lk, xvs, va, vb, vc,
      vd, asrc, tmpn, adst, misc, red, buf, bufw, total;
  size_t ek, eo, tmp, cursor;   // CSR build staging (inside the buffers)
};

__host__ __device__ inline VlLayout vl_layout(int H, int L, int max_n, int max_v, int max_ell, int max_evv) {
  VlLayout Y;
  auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  size_t o = 0;
  Y.w = o; o += 6 * (size_t)H * H;
  Y.vec = o; o += 8 * (size_t)H;
  Y.dinv_l = o; o += up4(max_n);
  Y.dinv_v = o; o += up4(max_v);
  Y.rp = o; o += up4((size_t)max_n + 1);
  Y.col = o; o += up4(max_ell);
  Y.rpt = o; o += up4((size_t)max_n + 1);
  Y.colt = o; o += up4(max_ell);
  Y.vrp = o; o += up4((size_t)max_v + 1);
  Y.vcol = o; o += up4(max_evv);
  Y.vrpt = o; o += up4((size_t)max_v + 1);
  Y.vcolt = o; o += up4(max_evv);
  Y.cl = o; o += up4(max_n);
  Y.mrp = o; o += up4((size_t)max_v + 1);
  Y.mcol = o; o += up4(max_n);
  Y.alpha = o; o += (size_t)L * up4(max_n);
  Y.lk = o; o += (size_t)L * up4(max_n);
  Y.xvs = o; o += (size_t)L * up4((size_t)max_v * H);
  Y.va = o; o += up4((size_t)max_v * H);
  Y.vb = o; o += up4((size_t)max_v * H);
  Y.vc = o; o += up4((size_t)max_v * H);
  Y.vd = o; o += up4((size_t)max_v * H);
  Y.asrc = o; o += up4(max_n);
  Y.tmpn = o; o += up4(max_n);
  Y.adst = o; o += 2 * up4(max_v);
  Y.misc = o; o += 8 * 64;
  Y.red = o; o += (size_t)VL_RT;
  size_t se = (size_t)max_ell;
  if ((size_t)max_evv > se) se = (size_t)max_evv;
  if ((size_t)max_n > se) se = (size_t)max_n;
  const size_t rows = (size_t)(max_n > max_v ? max_n : max_v) + 1;
  const size_t stage = 3 * up4(se) + up4(rows);
  size_t bufw = up4((size_t)max_n * H);
  if (stage > 3 * bufw) bufw = up4((stage + 2) / 3);
  Y.bufw = bufw;
  Y.buf = o; o += 3 * bufw;
  Y.ek = Y.buf;
  Y.eo = Y.ek + up4(se);
  Y.tmp = Y.eo + up4(se);
  Y.cursor = Y.tmp + up4(se);
  Y.total = o;
  return Y;
}

inline size_t vl_lds_bytes(int H, int L, int max_n, int max_v, int max_ell, int max_evv) {
  return vl_layout(H, L, max_n, max_v, max_ell, max_evv).total * 4;
}

// out[c] = sum_i w[i] X[i][c] (w = NULL: ones) for c < CP columns: RT / CP contiguous row chunks, each summed in row
// order, chunks folded in chunk order -- a fixed summation tree.  Valid in threads c < CP after the call; two barriers.
template <int CP>
__device__ __forceinline__ float vl_colsum(const float* X, const float* w, int n, float* red) {
  constexpr int NCH = VL_RT / CP;
  const int t = threadIdx.x;
  const int c = t % CP, ch = t / CP;
  const int per = (n + NCH - 1) / NCH;
  const int i0 = ch * per, i1 = i0 + per < n ? i0 + per : n;
  float s = 0.f;
  if (w) {
    for (int i = i0; i < i1; ++i) s = fmaf(w[i], X[i * CP + c], s);
  } else {
    for (int i = i0; i < i1; ++i) s += X[i * CP + c];
  }
  red[t] = s;
  lds_barrier();
  float r = 0.f;
  if (t < CP)
    for (int q = 0; q < NCH; ++q) r += red[q * CP + t];
  lds_barrier();
  return r;
}

// dst = the [rows][cols] matrix src as stored, or transposed ([cols][rows])
__device__ __forceinline__ void vl_load_w(float* dst, const float* src, int rows, int cols, bool transposed) {
  for (int q = threadIdx.x; q < rows * cols; q += VL_RT) {
    const int o = q / cols, k = q - o * cols;
    dst[transposed ? k * rows + o : q] = src[q];
  }
}

// h[i][o] = sum_k X[i][k] W[o][k] (k ascending); WT: W given transposed (Wt[k][o]), else as stored (W[o][k])
template <bool WT>
__device__ __forceinline__ void vl_transform(const float* X, const float* W, float* h, int n, int fin, int fout) {
  for (int idx = threadIdx.x; idx < n * fout; idx += VL_RT) {
    const int i = idx / fout, o = idx - i * fout;
    float acc = 0.f;
    for (int k = 0; k < fin; ++k) acc = fmaf(X[i * fin + k], WT ? W[k * fout + o] : W[o * fin + k], acc);
    h[idx] = acc;
  }
}

// out[j][k] (+)= sum_o G[j][o] W[o][k] (o ascending)
template <bool ADD>
__device__ __forceinline__ void vl_input_grad(const float* G, const float* W, float* out, int n, int fin, int fout) {
  for (int idx = threadIdx.x; idx < n * fin; idx += VL_RT) {
    const int j = idx / fin, k = idx - j * fin;
    float acc = 0.f;
    for (int o = 0; o < fout; ++o) acc = fmaf(G[j * fout + o], W[o * fin + k], acc);
    out[idx] = ADD ? out[idx] + acc : acc;
  }
}

// part[o][k] = sum_j G[j][o] X[j][k] (j ascending)
__device__ __forceinline__ void vl_weight_grad(const float* G, const float* X, float* part, int n, int fin, int fout) {
  for (int q = threadIdx.x; q < fout * fin; q += VL_RT) {
    const int o = q / fin, k = q - o * fin;
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = fmaf(G[j * fout + o], X[j * fin + k], acc);
    part[q] = acc;
  }
}

// sum_{j in row i} (dinv_j dinv_i) v[j][o] in row order
__device__ __forceinline__ float vl_gather(const int* rp, const int* col, const float* dinv, const float* v, int i, int o,
                                           int ncols) {
  const float di = dinv[i];
  float acc = 0.f;
  for (int q = rp[i], e = rp[i + 1]; q < e; ++q) {
    const int j = col[q];
    acc += (dinv[j] * di) * v[j * ncols + o];
  }
  return acc;
}

__device__ __forceinline__ void vl_zero(float* p, int n) {
  for (int q = threadIdx.x; q < n; q += VL_RT) p[q] = 0.f;
}

// edges [e0, e0 + ne) of ei as graph-local (target, source) pairs; an end outside its graph drops the edge (flag 2)
__device__ __forceinline__ void vl_stage(const int64_t* ei, int64_t E, int e0, int ne, int sbase, int ns, int dbase, int nd,
                                         int* ek, int* eo, int32_t* flag) {
  for (int e = threadIdx.x; e < ne; e += VL_RT) {
    const int64_t s = ei[e0 + e] - sbase, d = ei[E + e0 + e] - dbase;
    const bool ok = s >= 0 && s < ns && d >= 0 && d < nd;
    if (!ok && flag) atomicOr(flag, 2);
    ek[e] = ok ? (int)d : -1;
    eo[e] = ok ? (int)s : -1;
  }
}

template <int H, bool TRAIN>
__global__ void __launch_bounds__(VL_RT) k_vl_step(const VlArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* sm = reinterpret_cast<float*>(smem);
  int* si = reinterpret_cast<int*>(smem);
  const int g = blockIdx.x;
  const int t = threadIdx.x;
  const int L = A.L, F = A.F, C = A.C;
  const VlLayout Y = vl_layout(H, L, A.max_n, A.max_v, A.max_ell, A.max_evv);
  const int lb = A.lptr[g], n = A.lptr[g + 1] - lb;
  const int vb = A.vptr[g], nv = A.vptr[g + 1] - vb;
  const int e0l = A.eptr_ll[g], nel = A.eptr_ll[g + 1] - e0l;
  const int e0v = A.eptr_vv[g], nev = A.eptr_vv[g + 1] - e0v;
  const int e0c = A.eptr_lv[g], nec = A.eptr_lv[g + 1] - e0c;
  const int Ptot = A.P + 1;
  if (lb < 0 || n < 0 || n > A.max_n || (int64_t)lb + n > A.N || vb < 0 || nv < 0 || nv > A.max_v ||
      (int64_t)vb + nv > A.V || e0l < 0 || nel < 0 || nel > A.max_ell || (int64_t)e0l + nel > A.E_ll || e0v < 0 ||
      nev < 0 || nev > A.max_evv || (int64_t)e0v + nev > A.E_vv || e0c < 0 || nec < 0 || nec > A.max_n ||
      (int64_t)e0c + nec > A.E_lv) {
    // a graph beyond the capacities this launch was sized for: flagged, its rows written as zeros
    if (t == 0 && A.flag) atomicOr(A.flag, 4);
    if (TRAIN) {
      for (int p = t; p < Ptot; p += VL_RT) A.partials[(size_t)g * Ptot + p] = 0.f;
    } else if (A.partials && t == 0) {
      A.partials[g] = 0.f;
    }
    for (int c = t; c < C; c += VL_RT) {
      A.pred[(size_t)g * C + c] = 0.f;
      if (A.score) A.score[(size_t)g * C + c] = 0.f;
    }
    return;
  }
  float* W = sm + Y.w;                 // six H x H slots
  float* Wll = W, *Wvv = W + H * H, *Wlvs = W + 2 * H * H, *Wlvd = W + 3 * H * H, *Wvls = W + 4 * H * H;
  float* vec = sm + Y.vec;             // b_ll | b_vv | b_lv | b_vl | att_src | att_dst
  float *b_ll = vec, *b_vv = vec + H, *b_lv = vec + 2 * H, *b_vl = vec + 3 * H, *att_s = vec + 4 * H, *att_d = vec + 5 * H;
  float* dinv_l = sm + Y.dinv_l;
  float* dinv_v = sm + Y.dinv_v;
  int *rp = si + Y.rp, *col = si + Y.col, *rpt = si + Y.rpt, *colt = si + Y.colt;
  int *vrp = si + Y.vrp, *vcol = si + Y.vcol, *vrpt = si + Y.vrpt, *vcolt = si + Y.vcolt;
  int *cl = si + Y.cl, *mrp = si + Y.mrp, *mcol = si + Y.mcol;
  const size_t nstride = ((size_t)A.max_n + 3) & ~(size_t)3;
  const size_t vstride = ((size_t)A.max_v * H + 3) & ~(size_t)3;
  auto alpha = [&](int l) { return sm + Y.alpha + (size_t)l * nstride; };
  auto lkf = [&](int l) { return sm + Y.lk + (size_t)l * nstride; };
  auto xvs = [&](int l) { return sm + Y.xvs + (size_t)l * vstride; };
  float *vA = sm + Y.va, *vB = sm + Y.vb, *vC = sm + Y.vc, *vD = sm + Y.vd;
  float* asrc = sm + Y.asrc;
  float* tmpn = sm + Y.tmpn;
  int* cnt = si + Y.tmpn;
  float* adst = sm + Y.adst;
  float* dadst = adst + (((size_t)A.max_v + 3) & ~(size_t)3);
  float* misc = sm + Y.misc;
  float* red = sm + Y.red;
  float* buf0 = sm + Y.buf;
  float* buf1 = buf0 + Y.bufw;
  float* buf2 = buf1 + Y.bufw;
  int *ek = si + Y.ek, *eo = si + Y.eo, *tmp = si + Y.tmp, *cursor = si + Y.cursor;
  const Grp G{t, VL_RT, t >> 6, VL_RT / 64};
  const int nrows_max = (A.max_n > A.max_v ? A.max_n : A.max_v);

  // ---- structure: ll and vv CSRs by target and by source, degree norms, clusters and member lists ----
  for (int i = t; i <= nrows_max; i += VL_RT) cursor[i] = 0;
  vl_stage(A.ei_ll, A.E_ll, e0l, nel, lb, n, lb, n, ek, eo, A.flag);
  lds_barrier();
  build_csr_lds(ek, eo, nel, n, rp, col, cursor, tmp, G, false);
  build_csr_lds(eo, ek, nel, n, rpt, colt, cursor, tmp, G, false);
  dinv_from_rowptr(rp, n, dinv_l, G);
  vl_stage(A.ei_vv, A.E_vv, e0v, nev, vb, nv, vb, nv, ek, eo, A.flag);
  lds_barrier();
  build_csr_lds(ek, eo, nev, nv, vrp, vcol, cursor, tmp, G, false);
  build_csr_lds(eo, ek, nev, nv, vrpt, vcolt, cursor, tmp, G, false);
  dinv_from_rowptr(vrp, nv, dinv_v, G);
  vl_stage(A.ei_lv, A.E_lv, e0c, nec, lb, n, vb, nv, ek, eo, A.flag);
  for (int i = t; i < n; i += VL_RT) {
    cl[i] = -1;
    cnt[i] = 0;
  }
  lds_barrier();
  for (int e = t; e < nec; e += VL_RT) {
    if (ek[e] < 0) continue;
    atomicMax(&cl[eo[e]], ek[e]);
    if (atomicAdd(&cnt[eo[e]], 1) >= 1 && A.flag) atomicOr(A.flag, 16);   // several local -> virtual edges at one node
  }
  build_csr_lds(ek, eo, nec, nv, mrp, mcol, cursor, tmp, G, false);      // members of every cluster in edge order
  // ---- the input features ----
  for (int q = t; q < n * F; q += VL_RT) buf0[q] = A.xl[(size_t)lb * F + q];
  for (int q = t; q < nv * F; q += VL_RT) xvs(0)[q] = A.xv[(size_t)vb * F + q];
  lds_barrier();

  // ---- forward ----
  for (int l = 0; l < L; ++l) {
    const int fin = l == 0 ? F : H;
    const bool upd_v = l < L - 1 || A.xv_out != nullptr;
    const float* xv = xvs(l);
    vl_load_w(Wll, A.p[l][VP_WLL], H, fin, true);
    vl_load_w(Wvls, A.p[l][VP_VLS], H, fin, true);
    if (upd_v) {
      vl_load_w(Wvv, A.p[l][VP_WVV], H, fin, true);
      vl_load_w(Wlvs, A.p[l][VP_LVS], H, fin, true);
      vl_load_w(Wlvd, A.p[l][VP_LVD], H, fin, true);
    }
    for (int o = t; o < H; o += VL_RT) {
      b_ll[o] = A.p[l][VP_BLL][o];
      b_vl[o] = A.p[l][VP_VLB][o];
      b_vv[o] = A.p[l][VP_BVV][o];
      b_lv[o] = A.p[l][VP_LVB][o];
      att_s[o] = A.p[l][VP_LVAS][o];
      att_d[o] = A.p[l][VP_LVAD][o];
    }
    lds_barrier();
    vl_transform<true>(buf0, Wll, buf1, n, fin, H);
    vl_transform<true>(xv, Wvls, vA, nv, fin, H);
    if (upd_v) {
      vl_transform<true>(buf0, Wlvs, buf2, n, fin, H);
      vl_transform<true>(xv, Wvv, vB, nv, fin, H);
      vl_transform<true>(xv, Wlvd, vC, nv, fin, H);
    }
    lds_barrier();
    if (upd_v) {
      float* al = alpha(l);
      float* lk = lkf(l);
      for (int i = t; i < n; i += VL_RT) {
        float acc = 0.f;
        for (int o = 0; o < H; ++o) acc = fmaf(buf2[i * H + o], att_s[o], acc);
        asrc[i] = acc;
        al[i] = 0.f;
        lk[i] = 0.f;
      }
      for (int v = t; v < nv; v += VL_RT) {
        float acc = 0.f;
        for (int o = 0; o < H; ++o) acc = fmaf(vC[v * H + o], att_d[o], acc);
        adst[v] = acc;
      }
      lds_barrier();
      for (int v = t; v < nv; v += VL_RT) {   // segment softmax over the cluster's members, in edge order
        const int q0 = mrp[v], q1 = mrp[v + 1];
        const float ad = adst[v];
        float m = -INFINITY;
        for (int q = q0; q < q1; ++q) m = fmaxf(m, leaky(asrc[mcol[q]] + ad, A.slope));
        float den = 0.f;
        for (int q = q0; q < q1; ++q) den += expf(leaky(asrc[mcol[q]] + ad, A.slope) - m);
        den += 1e-16f;
        for (int q = q0; q < q1; ++q) {
          const int i = mcol[q];
          const float raw = asrc[i] + ad;
          al[i] = expf(leaky(raw, A.slope) - m) / den;
          lk[i] = raw > 0.f ? 1.f : A.slope;
        }
      }
      lds_barrier();
      float* xvn = l < L - 1 ? xvs(l + 1) : vD;
      for (int idx = t; idx < nv * H; idx += VL_RT) {
        const int v = idx / H, o = idx - v * H;
        float gat = 0.f;
        for (int q = mrp[v], e = mrp[v + 1]; q < e; ++q) {
          const int i = mcol[q];
          gat += al[i] * buf2[i * H + o];
        }
        const float z = (vl_gather(vrp, vcol, dinv_v, vB, v, o, H) + b_vv[o]) + (gat + b_lv[o]);
        const float a = z > 0.f ? z : 0.f;
        xvn[idx] = a;
        if (l == L - 1) A.xv_out[(size_t)vb * H + idx] = a;
      }
    }
    for (int idx = t; idx < n * H; idx += VL_RT) {
      const int i = idx / H, o = idx - i * H;
      const int c = cl[i];
      const float z = (vl_gather(rp, col, dinv_l, buf1, i, o, H) + b_ll[o]) + ((c >= 0 ? vA[c * H + o] : 0.f) + b_vl[o]);
      const float a = z > 0.f ? z : 0.f;
      buf0[idx] = a;
      if (TRAIN && l < L - 1) A.ws[((size_t)l * A.N + lb) * H + idx] = a;
    }
    lds_barrier();
  }

  // ---- mean pool, head, loss row ----
  const float cnt_n = (float)(n > 0 ? n : 1);
  float* pooled = misc;            // [H]
  float* hact = misc + 64;         // [H] act(lin_1)
  float* gp = misc + 128;          // [C] d loss / d pred
  float* lt_row = misc + 192;      // [C]
  float* gz1 = misc + 256;         // [H]
  float* gpool = misc + 320;       // [H]
  {
    const float ps = vl_colsum<H>(buf0, nullptr, n, red);
    if (t < H) pooled[t] = ps / cnt_n;
    lds_barrier();
    if (t < H) {
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fmaf(pooled[k], A.W1[t * H + k], acc);
      hact[t] = apply_act(acc + A.b1[t], A.act);
    }
    lds_barrier();
    if (t < C) {
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fmaf(hact[k], A.W2[t * H + k], acc);
      const float pc = acc + A.b2[t];
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
  }
  if (!TRAIN) return;

  // ---- backward: head ----
  float* part = A.partials + (size_t)g * Ptot;
  // flat order: layers 0 .. L-2 whole, the last layer's live part (ll, vl), the head, the last layer's dead part (vv, lv)
  auto layer_off = [&](int l) { return l == 0 ? 0 : (6 * H * F + 8 * H) + (l - 1) * (6 * H * H + 8 * H); };
  const int head = layer_off(L - 1) + 3 * H * (L == 1 ? F : H) + 4 * H;
  const int dead = head + H * H + H + C * H + C;
  if (t < H) {
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc = fmaf(gp[c], A.W2[c * H + t], acc);
    const float v = acc * act_grad_from_output(hact[t], A.act);
    gz1[t] = v;
    part[head + H * H + t] = v;                                          // b1
  }
  if (t < C) part[head + H * H + H + C * H + t] = gp[t];                 // b2
  lds_barrier();
  for (int q = t; q < H * H; q += VL_RT) part[head + q] = gz1[q / H] * pooled[q % H];                   // W1
  for (int q = t; q < C * H; q += VL_RT) part[head + H * H + H + q] = gp[q / H] * hact[q % H];           // W2
  if (t < H) {
    float acc = 0.f;
    for (int h = 0; h < H; ++h) acc = fmaf(gz1[h], A.W1[h * H + t], acc);
    gpool[t] = acc / cnt_n;
  }
  lds_barrier();
  // d loss / d (pre-ReLU output of the last layer): the pooled gradient at every node, through the ReLU
  for (int idx = t; idx < n * H; idx += VL_RT) buf0[idx] = buf0[idx] > 0.f ? gpool[idx % H] : 0.f;
  lds_barrier();

  // ---- backward: layers.  buf0 = gradient at the layer's local pre-activation, vD = at its virtual pre-activation ----
  for (int l = L - 1; l >= 0; --l) {
    const int fin = l == 0 ? F : H;
    const bool upd_v = l < L - 1;          // the last layer's virtual update is dead
    const float* xv = xvs(l);
    const int HF = H * fin;
    float* pl = part + layer_off(l);
    float *g_wll = pl, *g_bll = pl + HF;
    float* g_wvv = upd_v ? g_bll + H : part + dead;
    float *g_bvv = g_wvv + HF, *g_lvs = g_bvv + H, *g_lvd = g_lvs + HF;
    float *g_lvas = g_lvd + HF, *g_lvad = g_lvas + H, *g_lvb = g_lvad + H;
    float* g_vls = upd_v ? g_lvb + H : g_bll + H;
    float *g_vld = g_vls + HF, *g_vlas = g_vld + HF, *g_vlad = g_vlas + H, *g_vlb = g_vlad + H;
    vl_load_w(Wll, A.p[l][VP_WLL], H, fin, false);
    vl_load_w(Wvls, A.p[l][VP_VLS], H, fin, false);
    if (upd_v) {
      vl_load_w(Wvv, A.p[l][VP_WVV], H, fin, false);
      vl_load_w(Wlvs, A.p[l][VP_LVS], H, fin, false);
      vl_load_w(Wlvd, A.p[l][VP_LVD], H, fin, false);
      for (int o = t; o < H; o += VL_RT) {
        att_s[o] = A.p[l][VP_LVAS][o];
        att_d[o] = A.p[l][VP_LVAD][o];
      }
    }
    // the layer's input again
    const float* xsrc = l == 0 ? A.xl + (size_t)lb * F : A.ws + ((size_t)(l - 1) * A.N + lb) * H;
    for (int q = t; q < n * fin; q += VL_RT) buf2[q] = xsrc[q];
    // B1: A_ll^T G, the member sums of G (what the virtual -> local relation hands its cluster), bias gradients
    for (int idx = t; idx < n * H; idx += VL_RT) buf1[idx] = vl_gather(rpt, colt, dinv_l, buf0, idx / H, idx % H, H);
    for (int idx = t; idx < nv * H; idx += VL_RT) {
      const int v = idx / H, o = idx - v * H;
      float acc = 0.f;
      for (int q = mrp[v], e = mrp[v + 1]; q < e; ++q) acc += buf0[mcol[q] * H + o];
      vA[idx] = acc;
    }
    {
      const float gb = vl_colsum<H>(buf0, nullptr, n, red);   // (barriers inside)
      if (t < H) {
        g_bll[t] = gb;
        g_vlb[t] = gb;
      }
    }
    // B2: weight gradients of ll and vl, the gradient at the layer's inputs
    vl_weight_grad(buf1, buf2, g_wll, n, fin, H);
    vl_weight_grad(vA, xv, g_vls, nv, fin, H);
    vl_zero(g_vld, HF);
    vl_zero(g_vlas, 2 * H);
    if (!upd_v) {
      vl_zero(g_wvv, HF + H);
      vl_zero(g_lvs, 2 * HF + 3 * H);
    }
    if (l > 0) {
      vl_input_grad<false>(buf1, Wll, buf0, n, fin, H);
      vl_input_grad<false>(vA, Wvls, vB, nv, fin, H);
    }
    lds_barrier();
    if (upd_v) {
      float* al = alpha(l);
      float* lk = lkf(l);
      // B3: A_vv^T Gv, the local -> virtual transforms again, bias gradients of vv and lv
      for (int idx = t; idx < nv * H; idx += VL_RT) vA[idx] = vl_gather(vrpt, vcolt, dinv_v, vD, idx / H, idx % H, H);
      vl_transform<false>(buf2, Wlvs, buf1, n, fin, H);
      vl_transform<false>(xv, Wlvd, vC, nv, fin, H);
      if (t < H) {
        float acc = 0.f;
        for (int v = 0; v < nv; ++v) acc += vD[v * H + t];
        g_bvv[t] = acc;
        g_lvb[t] = acc;
      }
      lds_barrier();
      // B4: vv weight / input gradients; d alpha_i = Gv[c(i)] . hs_i
      vl_weight_grad(vA, xv, g_wvv, nv, fin, H);
      if (l > 0) vl_input_grad<true>(vA, Wvv, vB, nv, fin, H);
      for (int i = t; i < n; i += VL_RT) {
        const int c = cl[i];
        float acc = 0.f;
        if (c >= 0)
          for (int o = 0; o < H; ++o) acc = fmaf(vD[c * H + o], buf1[i * H + o], acc);
        tmpn[i] = acc;
        asrc[i] = 0.f;
      }
      lds_barrier();
      // B5: softmax and leaky-ReLU backward per cluster: asrc[i] = d raw score_i, dadst[v] = their sum
      for (int v = t; v < nv; v += VL_RT) {
        const int q0 = mrp[v], q1 = mrp[v + 1];
        float s = 0.f;
        for (int q = q0; q < q1; ++q) s = fmaf(al[mcol[q]], tmpn[mcol[q]], s);
        float tot = 0.f;
        for (int q = q0; q < q1; ++q) {
          const int i = mcol[q];
          const float d = al[i] * (tmpn[i] - s) * lk[i];
          asrc[i] = d;
          tot += d;
        }
        dadst[v] = tot;
      }
      lds_barrier();
      // B6: attention vector gradients, then the gradients of the two transforms in place
      if (t < H) {
        float acc = 0.f;
        for (int v = 0; v < nv; ++v) acc = fmaf(dadst[v], vC[v * H + t], acc);
        g_lvad[t] = acc;
      }
      {
        const float ga = vl_colsum<H>(buf1, asrc, n, red);   // (barriers inside)
        if (t < H) g_lvas[t] = ga;
      }
      for (int idx = t; idx < n * H; idx += VL_RT) {
        const int i = idx / H, o = idx - i * H;
        const int c = cl[i];
        buf1[idx] = (c >= 0 ? al[i] * vD[c * H + o] : 0.f) + asrc[i] * att_s[o];
      }
      for (int idx = t; idx < nv * H; idx += VL_RT) vC[idx] = dadst[idx / H] * att_d[idx % H];
      lds_barrier();
      // B7: weight gradients of lv's transforms, their share of the input gradients
      vl_weight_grad(buf1, buf2, g_lvs, n, fin, H);
      vl_weight_grad(vC, xv, g_lvd, nv, fin, H);
      if (l > 0) {
        vl_input_grad<true>(buf1, Wlvs, buf0, n, fin, H);
        vl_input_grad<true>(vC, Wlvd, vB, nv, fin, H);
      }
      lds_barrier();
    }
    if (l == 0) break;
    // through the ReLU that produced this layer's inputs
    for (int idx = t; idx < n * H; idx += VL_RT) buf0[idx] = buf2[idx] > 0.f ? buf0[idx] : 0.f;
    for (int idx = t; idx < nv * H; idx += VL_RT) vD[idx] = xv[idx] > 0.f ? vB[idx] : 0.f;
    lds_barrier();
  }
}

template <int H, bool TRAIN>
int launch_vl(const VlArgs& A, int64_t B, hipStream_t st) {
  const size_t lds = vl_lds_bytes(H, A.L, A.max_n, A.max_v, A.max_ell, A.max_evv);
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  return launch_with_lds(k_vl_step<H, TRAIN>, (unsigned)B, VL_RT, lds, st, A);
}

}  // namespace

extern "C" {

int hscn_vl_supported(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv) {
  if (!(H == 16 || H == 32) || F < 1 || F > H || L < 1 || L > VL_MAXL || C < 1 || C > H || C > 16) return 0;
  if (max_n < 0 || max_v < 0 || max_ell < 0 || max_evv < 0 || max_n > (1 << 20) || max_v > (1 << 20) ||
      max_ell > (1 << 22) || max_evv > (1 << 22))
    return 0;
  return vl_lds_bytes(H, L, max_n, max_v, max_ell, max_evv) <= LDS_CU_BYTES ? 1 : 0;
}

int64_t hscn_vl_param_count(int F, int H, int L, int C) {
  int64_t P = (int64_t)H * H + H + (int64_t)C * H + C;
  for (int l = 0; l < L; ++l) {
    const int64_t fin = l == 0 ? F : H;
    P += 6 * H * fin + 8 * H;
  }
  return P;
}

}  // extern "C"

namespace {

int fill_vl_args(VlArgs& A, const float* x_local, const float* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                 const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr,
                 const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv, int64_t N,
                 int64_t V, int F, int H, int L, int C, int head_act, float slope, const void* const* layer_params_host,
                 const float* W1, const float* b1, const float* W2, const float* b2, int max_n, int max_v, int max_ell,
                 int max_evv, const float* target, int loss_kind, float inv_count, float* pred, float* score,
                 int32_t* flag) {
  if (N < 0 || V < 0 || E_ll < 0 || E_vv < 0 || E_lv < 0 || !lptr || !vptr || !eptr_ll || !eptr_vv || !eptr_lv ||
      !layer_params_host || !W1 || !b1 || !W2 || !b2 || !pred || (N > 0 && !x_local) || (V > 0 && !x_virtual) ||
      (E_ll > 0 && !ei_ll) || (E_vv > 0 && !ei_vv) || (E_lv > 0 && !ei_lv))
    return HSCN_E_BADARG;
  if (head_act != HSCN_ACT_IDENTITY && head_act != HSCN_ACT_RELU && head_act != HSCN_ACT_ELU && head_act != HSCN_ACT_TANH)
    return HSCN_E_BADARG;
  if (target && loss_kind != 0 && loss_kind != 1) return HSCN_E_BADARG;
  if (!hscn_vl_supported(F, H, L, C, max_n, max_v, max_ell, max_evv)) return HSCN_E_UNSUPPORTED;
  A = VlArgs{};
  A.xl = x_local; A.xv = x_virtual; A.ei_ll = ei_ll; A.ei_vv = ei_vv; A.ei_lv = ei_lv;
  A.E_ll = E_ll; A.E_vv = E_vv; A.E_lv = E_lv; A.N = N; A.V = V;
  A.lptr = lptr; A.vptr = vptr; A.eptr_ll = eptr_ll; A.eptr_vv = eptr_vv; A.eptr_lv = eptr_lv;
  for (int l = 0; l < L; ++l)
    for (int k = 0; k < VL_NP; ++k) {
      if (!layer_params_host[l * VL_NP + k]) return HSCN_E_BADARG;
      A.p[l][k] = (const float*)layer_params_host[l * VL_NP + k];
    }
  A.W1 = W1; A.b1 = b1; A.W2 = W2; A.b2 = b2;
  A.target = target; A.pred = pred; A.score = score; A.flag = flag;
  A.F = F; A.H = H; A.L = L; A.C = C; A.act = head_act; A.max_n = max_n; A.max_v = max_v; A.max_ell = max_ell;
  A.max_evv = max_evv;
  A.P = (int)hscn_vl_param_count(F, H, L, C);
  A.loss_kind = loss_kind; A.slope = slope; A.inv_count = inv_count;
  return 0;
}

}  // namespace

extern "C" {

int hscn_vl_train_step(const float* x_local, const float* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                       const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr,
                       const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv,
                       int64_t N, int64_t V, int64_t B, int F, int H, int L, int C, int head_act, float slope,
                       const void* const* layer_params_host, const float* W1, const float* b1, const float* W2,
                       const float* b2, int max_n, int max_v, int max_ell, int max_evv, const float* target,
                       int loss_kind, float inv_count, float* pred, float* score, float* partials, float* grads,
                       float* workspace, int32_t* flag, int accumulate, void* stream_) {
  if (B < 0) return HSCN_E_BADARG;
  if (B == 0) return 0;
  if (!target || !partials || !grads || (L > 1 && N > 0 && !workspace)) return HSCN_E_BADARG;
  VlArgs A;
  if (int rc = fill_vl_args(A, x_local, x_virtual, ei_ll, E_ll, ei_vv, E_vv, ei_lv, E_lv, lptr, vptr, eptr_ll, eptr_vv,
                            eptr_lv, N, V, F, H, L, C, head_act, slope, layer_params_host, W1, b1, W2, b2, max_n, max_v,
                            max_ell, max_evv, target, loss_kind, inv_count, pred, score, flag))
    return rc;
  A.partials = partials; A.ws = workspace;
  hipStream_t st = hscn_stream(stream_);
  const int rc = H == 16 ? launch_vl<16, true>(A, B, st) : launch_vl<32, true>(A, B, st);
  if (rc) return rc;
  launch_param_fold(partials, grads, (int)B, A.P + 1, A.P, inv_count, nullptr, accumulate != 0, st);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_vl_forward(const float* x_local, const float* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                    const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr,
                    const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv, int64_t N,
                    int64_t V, int64_t B, int F, int H, int L, int C, int head_act, float slope,
                    const void* const* layer_params_host, const float* W1, const float* b1, const float* W2,
                    const float* b2, int max_n, int max_v, int max_ell, int max_evv, const float* target, int loss_kind,
                    float inv_count, float* pred, float* score, float* loss_rows, float* loss, float* xv_out,
                    int32_t* flag, void* stream_) {
  if (B < 0 || (loss && (!loss_rows || !target))) return HSCN_E_BADARG;
  if (B == 0) return 0;
  VlArgs A;
  if (int rc = fill_vl_args(A, x_local, x_virtual, ei_ll, E_ll, ei_vv, E_vv, ei_lv, E_lv, lptr, vptr, eptr_ll, eptr_vv,
                            eptr_lv, N, V, F, H, L, C, head_act, slope, layer_params_host, W1, b1, W2, b2, max_n, max_v,
                            max_ell, max_evv, target, loss_kind, inv_count, pred, score, flag))
    return rc;
  A.partials = target ? loss_rows : nullptr;
  A.xv_out = xv_out;
  hipStream_t st = hscn_stream(stream_);
  const int rc = H == 16 ? launch_vl<16, false>(A, B, st) : launch_vl<32, false>(A, B, st);
  if (rc) return rc;
  if (loss) k_param_reduce<<<1, 256, 0, st>>>(loss_rows, loss, (int)B, 1, 0, inv_count, nullptr);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
