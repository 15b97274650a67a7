// GATConv attention part on a HOMOGENEOUS graph with one implicit self loop per node (heads=1; PyG
// GATConv(in, out) with add_self_loops=True, what the MPNN baseline builds: reference model/mpnn.py:29-32,52,59).
//
// Narrow rows: a molecule batch has tens of thousands of target rows with two or three neighbours each, where
// the wave-per-row kernels of gat.hip leave 60 of 64 lanes idle.  Here a row is owned by a group of G consecutive
// lanes (G = the power of two >= width/4 at 16-byte access when width % 4 == 0, >= width at scalar access
// otherwise; G <= 64), a wave covers 64/G rows, and the group walks its row's neighbours serially: max, exp-sum
// and weighted sum stay in registers, nothing crosses a wave, nothing goes through LDS.  The only fold is the
// g . h dot of the two backward kernels, a __shfl_xor butterfly inside the group.
//
// Self loops: the kernels take the stable CSRs of the RAW edge list.  Entries with col == row are skipped
// (remove_self_loops), the node's own term is added LAST (add_self_loops appends the loops after the remaining
// edges): the summation order of PyG's scatter over structure.with_self_loops(edge_index), with no boolean-mask
// indexing on the host -- every shape is host-known and the launches can be captured.
//
// Nothing is stored per edge.  The forward leaves stat[v] = {row max, exp-sum + 1e-16}; both backward kernels
// recompute alpha from it, and the source side recomputes the g . h dot it shares with the target side, which
// hands over tsum[v] = sum_e alpha_e (g_v . h_e) and g_a_dst[v] only.
//
// DISPATCH RULE (nn/functional.py: GATLoopFn): per call, by the relation's maximum raw in-degree.  These kernels
// are correct for rows of any degree (every loop is bounded by rowptr), but a group walks its row serially, so
// one hub row holds its wave for deg gathers in a row; a relation whose largest in-degree exceeds
// GAT_NARROW_MAX_DEGREE goes to the wave-per-row kernels of gat.hip over the explicit-loop relation instead.
#include "row_walk.h"

namespace {

constexpr int GL_THREADS = 256;

// G lanes per row, RPB = GL_THREADS / G rows per block
template <int VEC>
__global__ void __launch_bounds__(GL_THREADS)
k_gat_loop_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ a_src,
               const float* __restrict__ a_dst, const float* __restrict__ h, const float* __restrict__ bias,
               float* __restrict__ stat, float* __restrict__ out, int64_t n, int width, float slope, int act, int G) {
  const int RPB = GL_THREADS / G;
  const int rl = threadIdx.x / G;
  const int fl = threadIdx.x - rl * G;
  const int f = fl * VEC;
  const bool flive = f < width;
  for (int64_t v = (int64_t)blockIdx.x * RPB + rl; v < n; v += (int64_t)gridDim.x * RPB) {
    const int s = rowptr[v], t = rowptr[v + 1];
    const float ad = a_dst[v];
    const float zself = rw_leaky(a_src[v] + ad, slope);
    float m = zself;
    for (int p = s; p < t; ++p) {
      const int j = col[p];
      if (j != (int)v) m = fmaxf(m, rw_leaky(a_src[j] + ad, slope));
    }
    float sum = 0.f;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int p = s; p < t; ++p) {
      const int j = col[p];
      if (j == (int)v) continue;
      const float e = expf(rw_leaky(a_src[j] + ad, slope) - m);
      sum += e;
      if (flive) {
        float hv[VEC];
        rw_load<VEC>(h + (size_t)j * width + f, hv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(e, hv[k], acc[k]);
      }
    }
    const float es = expf(zself - m);
    sum += es;
    const float denom = sum + 1e-16f;
    if (fl == 0) {
      stat[2 * v] = m;
      stat[2 * v + 1] = denom;
    }
    if (flive) {
      float hv[VEC], o[VEC];
      rw_load<VEC>(h + (size_t)v * width + f, hv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(es, hv[k], acc[k]) / denom;
      if (bias) {
        float b[VEC];
        rw_load<VEC>(bias + f, b);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += b[k];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = apply_act(acc[k], act);
      rw_store<VEC>(out + (size_t)v * width + f, o);
    }
  }
}

// target side: tsum[v] = sum_e alpha_e (g_v . h_e) and g_a[2v+1] = sum_e dL/d(a_src[e] + a_dst[v]), e over the
// row's kept entries and the loop
template <int VEC>
__global__ void __launch_bounds__(GL_THREADS)
k_gat_loop_bwd_dst(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                   const float* __restrict__ a_src, const float* __restrict__ a_dst, const float* __restrict__ h,
                   const float* __restrict__ stat, const float* __restrict__ g, float* __restrict__ tsum,
                   float* __restrict__ g_a, int64_t n, int width, float slope, int G) {
  const int RPB = GL_THREADS / G;
  const int rl = threadIdx.x / G;
  const int fl = threadIdx.x - rl * G;
  const int f = fl * VEC;
  const bool flive = f < width;
  for (int64_t v = (int64_t)blockIdx.x * RPB + rl; v < n; v += (int64_t)gridDim.x * RPB) {
    const int s = rowptr[v], t = rowptr[v + 1];
    const float ad = a_dst[v];
    const float m = stat[2 * v], denom = stat[2 * v + 1];
    float gv[VEC], hv[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) gv[k] = 0.f, hv[k] = 0.f;
    if (flive) rw_load<VEC>(g + (size_t)v * width + f, gv);
    // pass 1: the alpha-weighted mean of the dots
    float ts = 0.f;
    for (int p = s; p < t; ++p) {
      const int j = col[p];
      if (j == (int)v) continue;
      if (flive) rw_load<VEC>(h + (size_t)j * width + f, hv);
      const float d = group_sum(rw_dot<VEC>(gv, hv), G);
      const float a = expf(rw_leaky(a_src[j] + ad, slope) - m) / denom;
      ts = fmaf(a, d, ts);
    }
    const float pre_self = a_src[v] + ad;
    const float a_self = expf(rw_leaky(pre_self, slope) - m) / denom;
    if (flive) rw_load<VEC>(h + (size_t)v * width + f, hv);
    const float d_self = group_sum(rw_dot<VEC>(gv, hv), G);
    ts = fmaf(a_self, d_self, ts);
    // pass 2: softmax and leaky-ReLU derivatives per entry (the rows are L1/L2-resident from pass 1)
    float gad = 0.f;
    for (int p = s; p < t; ++p) {
      const int j = col[p];
      if (j == (int)v) continue;
      if (flive) rw_load<VEC>(h + (size_t)j * width + f, hv);
      const float d = group_sum(rw_dot<VEC>(gv, hv), G);
      const float pre = a_src[j] + ad;
      const float gl = expf(rw_leaky(pre, slope) - m) / denom * (d - ts);
      gad += pre > 0.f ? gl : gl * slope;
    }
    const float gls = a_self * (d_self - ts);
    gad += pre_self > 0.f ? gls : gls * slope;
    if (fl == 0) {
      tsum[v] = ts;
      g_a[2 * v + 1] = gad;
    }
  }
}

// source side over the source-keyed CSR: g_a[2j] = sum over out-entries (and the loop) of dL/d(a_src[j] + a_dst[v]),
// g_h[j,:] = sum alpha g[v,:] + g_a[2j] att_src + g_a[2j+1] att_dst  (the shared transform: h feeds both dots)
template <int VEC>
__global__ void __launch_bounds__(GL_THREADS)
k_gat_loop_bwd_src(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t,
                   const float* __restrict__ a_src, const float* __restrict__ a_dst, const float* __restrict__ h,
                   const float* __restrict__ stat, const float* __restrict__ tsum, const float* __restrict__ g,
                   const float* __restrict__ att_src, const float* __restrict__ att_dst, float* __restrict__ g_a,
                   float* __restrict__ g_h, int64_t n, int width, float slope, int G) {
  const int RPB = GL_THREADS / G;
  const int rl = threadIdx.x / G;
  const int fl = threadIdx.x - rl * G;
  const int f = fl * VEC;
  const bool flive = f < width;
  for (int64_t j = (int64_t)blockIdx.x * RPB + rl; j < n; j += (int64_t)gridDim.x * RPB) {
    const int s = rowptr_t[j], t = rowptr_t[j + 1];
    const float as = a_src[j];
    float hv[VEC], gv[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) hv[k] = 0.f, gv[k] = 0.f, acc[k] = 0.f;
    if (flive) rw_load<VEC>(h + (size_t)j * width + f, hv);
    float gas = 0.f;
    for (int q = s; q <= t; ++q) {           // q == t: the loop j -> j, last
      const int v = q < t ? col_t[q] : (int)j;
      if (q < t && v == (int)j) continue;
      if (flive) rw_load<VEC>(g + (size_t)v * width + f, gv);
      const float d = group_sum(rw_dot<VEC>(gv, hv), G);
      const float pre = as + a_dst[v];
      const float a = expf(rw_leaky(pre, slope) - stat[2 * (size_t)v]) / stat[2 * (size_t)v + 1];
      const float gl = a * (d - tsum[v]);
      gas += pre > 0.f ? gl : gl * slope;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(a, gv[k], acc[k]);
    }
    if (flive) {
      float at[VEC];
      rw_load<VEC>(att_src + f, at);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(gas, at[k], acc[k]);
      const float gad = g_a[2 * j + 1];
      rw_load<VEC>(att_dst + f, at);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = fmaf(gad, at[k], acc[k]);
      rw_store<VEC>(g_h + (size_t)j * width + f, acc);
    }
    if (fl == 0) g_a[2 * j] = gas;
  }
}

}  // namespace

extern "C" {

int hscn_gat_loop_fwd(const int32_t* rowptr, const int32_t* col, const float* a_src, const float* a_dst,
                      const float* h, const float* bias, float* stat, float* out, int64_t num_nodes, int width,
                      float slope, int act, void* stream_) {
  if (num_nodes < 0 || width < 1 || act < HSCN_ACT_IDENTITY || act > HSCN_ACT_TANH) return HSCN_E_BADARG;
  if (num_nodes == 0) return 0;
  if (!rowptr || !col || !a_src || !a_dst || !h || !stat || !out) return HSCN_E_BADARG;
  const int VEC = (width % 4 == 0) ? 4 : 1;
  const int G = pow2_lanes((width + VEC - 1) / VEC, false);      // lanes per row; wider than a wave is refused
  if (G == 0) return HSCN_E_UNSUPPORTED;
  const unsigned nb = capped_grid(num_nodes, GL_THREADS / G, 8192);
  hipStream_t stt = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) {
    k_gat_loop_fwd<decltype(v)::value><<<nb, GL_THREADS, 0, stt>>>(rowptr, col, a_src, a_dst, h, bias, stat, out,
                                                                  num_nodes, width, slope, act, G);
  });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_gat_loop_bwd_dst(const int32_t* rowptr, const int32_t* col, const float* a_src, const float* a_dst,
                          const float* h, const float* stat, const float* g, float* tsum, float* g_a,
                          int64_t num_nodes, int width, float slope, void* stream_) {
  if (num_nodes < 0 || width < 1) return HSCN_E_BADARG;
  if (num_nodes == 0) return 0;
  if (!rowptr || !col || !a_src || !a_dst || !h || !stat || !g || !tsum || !g_a) return HSCN_E_BADARG;
  const int VEC = (width % 4 == 0) ? 4 : 1;
  const int G = pow2_lanes((width + VEC - 1) / VEC, false);      // lanes per row; wider than a wave is refused
  if (G == 0) return HSCN_E_UNSUPPORTED;
  const unsigned nb = capped_grid(num_nodes, GL_THREADS / G, 8192);
  hipStream_t stt = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) {
    k_gat_loop_bwd_dst<decltype(v)::value><<<nb, GL_THREADS, 0, stt>>>(rowptr, col, a_src, a_dst, h, stat, g, tsum, g_a,
                                                                      num_nodes, width, slope, G);
  });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

int hscn_gat_loop_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const float* a_src, const float* a_dst,
                          const float* h, const float* stat, const float* tsum, const float* g,
                          const float* att_src, const float* att_dst, float* g_a, float* g_h, int64_t num_nodes,
                          int width, float slope, void* stream_) {
  if (num_nodes < 0 || width < 1) return HSCN_E_BADARG;
  if (num_nodes == 0) return 0;
  if (!rowptr_t || !col_t || !a_src || !a_dst || !h || !stat || !tsum || !g || !att_src || !att_dst || !g_a || !g_h)
    return HSCN_E_BADARG;
  const int VEC = (width % 4 == 0) ? 4 : 1;
  const int G = pow2_lanes((width + VEC - 1) / VEC, false);      // lanes per row; wider than a wave is refused
  if (G == 0) return HSCN_E_UNSUPPORTED;
  const unsigned nb = capped_grid(num_nodes, GL_THREADS / G, 8192);
  hipStream_t stt = hscn_stream(stream_);
  dispatch_vec(VEC, [&](auto v) {
    k_gat_loop_bwd_src<decltype(v)::value><<<nb, GL_THREADS, 0, stt>>>(rowptr_t, col_t, a_src, a_dst, h, stat, tsum, g,
                                                                      att_src, att_dst, g_a, g_h, num_nodes, width,
                                                                      slope, G);
  });
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
