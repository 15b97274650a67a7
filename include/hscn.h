/*
 * hscn.h -- C ABI of the MI355X (gfx950) hot path of Graph-HSCN.
 *
 * The reference (camille-004/Graph-HSCN) has no FFI layer: its hot path is
 * Python that calls un-vendored torch_geometric / torch_scatter operators
 * (reference graph_hscn/model/hscn.py:6-14).  This header is the boundary a
 * replacement shared library must export; every entry point names the
 * reference call site (file:line under /root/reference) whose arithmetic it
 * replaces.  The Python mirror in graph-hscn_amd/graph_hscn binds it with
 * ctypes.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     the parameter name ends in _host;
 *   - the caller allocates every output and workspace; nothing is allocated,
 *     freed or synchronised inside (safe under hipGraph stream capture);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - return 0 on success, a positive hipError_t from the launch, or a
 *     negative HSCN_E_* for bad arguments; never throws;
 *   - node features are row-major fp32 [rows, width]; CSR indices are int32,
 *     COO inputs are int64 [2,E] as torch_geometric stores them;
 *   - stateless and re-entrant; no global handles (the hscn_comm_* set-up helpers of the data-parallel exchange
 *     are the one documented exception: they allocate / map peer memory, host-synchronously, once per job);
 *   - all reductions are ordered: results are bitwise reproducible run to run
 *     (no floating-point atomics anywhere).
 */
#ifndef HSCN_H
#define HSCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSCN_ABI_VERSION 24

#define HSCN_E_BADARG (-1)   /* null pointer, negative size, unsupported width */
#define HSCN_E_WORKSPACE (-2) /* workspace too small */
#define HSCN_E_UNSUPPORTED (-3)

/* `flags` of the resident entry points (ABI 23; the last parameter before `stream`).  An entry point takes the bits
 * its comment names and answers HSCN_E_BADARG for any other, before any launch.
 *   HSCN_STORE_F16       node features and activations are IEEE half ("half storage", below at hscn_half)
 *   HSCN_GRAD_ACCUMULATE the gradient fold adds to `grads` ("gradient accumulation", below) */
#define HSCN_STORE_F16 1
#define HSCN_GRAD_ACCUMULATE 2

/* activation codes (reference graph_hscn/config/config.py:13-18 ACT_DICT) */
#define HSCN_ACT_IDENTITY 0
#define HSCN_ACT_RELU 1
#define HSCN_ACT_ELU 2
#define HSCN_ACT_TANH 3

int hscn_abi_version(void);
const char* hscn_strerror(int code);

/* ------------------------------------------------------------------------- *
 * Graph structure: COO(int64) -> CSR(int32), stable.
 * Replaces the per-call index bookkeeping inside PyG MessagePassing.propagate
 * (gather by edge_index[0], scatter by edge_index[1]) for every conv at
 * reference model/hscn.py:32,40,85-93.
 *   key[e]   : row of edge e in the CSR being built (target for a forward
 *              CSR, source for the transposed one)
 *   other[e] : column stored for edge e
 * Rows keep their edges in ascending e (the order torch's CPU index_add_
 * accumulates in).  eid[p] is the original edge number of CSR slot p.
 * Edges whose key/other fall outside [0,num_rows)/[0,num_cols) are skipped and
 * flag[0] is set to 1 (flag may be NULL).
 * ------------------------------------------------------------------------- */
size_t hscn_csr_workspace_bytes(int64_t num_edges, int64_t num_rows);
int hscn_csr_build(const int64_t* key, const int64_t* other, int64_t num_edges,
                   int64_t num_rows, int64_t num_cols,
                   int32_t* rowptr /*[num_rows+1]*/, int32_t* col /*[E]*/, int32_t* eid /*[E]*/,
                   int32_t* flag /*[1] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);
/* ABI 17: BOTH stable CSRs of one edge list in one go -- keyed by target (what the forward gathers through: rowptr / col /
 * eid, num_dst rows) and keyed by source (what the backward of the same MessagePassing.propagate call gathers through:
 * rowptr_t / col_t / eid_t, num_src rows) -- with 7 launches instead of the 16 of two hscn_csr_build calls (one zeroing
 * launch, one histogram and one fill pass that serve both keys, the scans and the in-row ranking of the two sides as the
 * two halves of one grid).  Results are bit-identical to hscn_csr_build(dst, src, ...) and hscn_csr_build(src, dst, ...).
 * An edge with an endpoint out of range is skipped on both sides and raises flag[0]. */
size_t hscn_csr_pair_workspace_bytes(int64_t num_edges, int64_t num_src, int64_t num_dst);
int hscn_csr_build_pair(const int64_t* src, const int64_t* dst, int64_t num_edges, int64_t num_src, int64_t num_dst,
                        int32_t* rowptr /*[num_dst+1]*/, int32_t* col /*[E]*/, int32_t* eid /*[E]*/,
                        int32_t* rowptr_t /*[num_src+1]*/, int32_t* col_t /*[E]*/, int32_t* eid_t /*[E]*/,
                        int32_t* flag /*[1] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* inv_pos[eid[p]] = p  and  pos_t[q] = inv_pos[eid_t[q]]: CSR slot of the edge
 * at slot q of the transposed CSR (used by backward passes that stored
 * per-edge values in forward-CSR order). */
int hscn_csr_cross_positions(const int32_t* eid, const int32_t* eid_t, int64_t num_edges,
                             int32_t* inv_pos_scratch /*[E]*/, int32_t* pos_t /*[E]*/, void* stream);

/* PyG gcn_norm(add_self_loops=False) degree part, unit edge weights
 * (reference model/hscn.py:88-93 via GCNConv): dinv[i] = indeg(i)^-1/2, 0 if
 * indeg(i)==0, with indeg read off rowptr. */
int hscn_gcn_dinv(const int32_t* rowptr, int64_t num_rows, float* dinv, void* stream);

/* PyG gcn_norm with explicit edge weights (reference
 * train/train_clustering.py:37-42): deg[i] = sum of w over CSR row i in edge
 * order; dinv = deg^-1/2 (inf -> 0); w_norm[e] = dinv[src]*w[e]*dinv[dst].
 * rowptr/col/eid: CSR keyed by target. */
int hscn_gcn_norm_weights(const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                          const float* w /*[E] by edge id, or NULL = ones*/, int64_t num_rows,
                          float* dinv_scratch /*[num_rows]*/, float* w_norm /*[E] by edge id*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Dense feature transform  y = act( x W^T + b  [+ x2 W2^T] ), optional row
 * dot a[r] = sum_o (x W^T)[r,o] * att[o]  (pre-bias, pre-activation).
 * Replaces torch_geometric.nn.Linear inside GraphConv/GCNConv/GATConv and the
 * head (reference model/hscn.py:51,54,99,100,112-113) and GATConv's
 * (x*att).sum(-1).
 *   w_layout 0: W is [out,in] (nn.Linear layout);  1: W is [in,out].
 * ------------------------------------------------------------------------- */
int hscn_linear_fwd(const float* x, const float* W, const float* bias /*or NULL*/,
                    const float* x2 /*or NULL*/, const float* W2 /*or NULL*/,
                    const float* att /*[out] or NULL*/, float* a_out /*[rows] or NULL*/,
                    float* y, int64_t rows, int in_f, int out_f, int w_layout, int act, void* stream);

/* gy <- gy * act'(y) in place is NOT done here; see hscn_act_bwd.
 * gW[out,in] = sum_r gy[r,:]^T x[r,:],  gb[out] = sum_r gy[r,:]  (either may be
 * NULL).  Two ordered stages through `partials`
 * (hscn_linear_bwd_w_workspace_bytes). */
size_t hscn_linear_bwd_w_workspace_bytes(int64_t rows, int in_f, int out_f);
int hscn_linear_bwd_w(const float* gy, const float* x, float* gW, float* gb,
                      int64_t rows, int in_f, int out_f, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);

/* y = act(x) elementwise (reference config/config.py:13-18 ACT_DICT; the
 * inter-layer ReLU at model/hscn.py:110 when it is not fused into a conv). */
int hscn_act_fwd(const float* x, float* y, int64_t count, int act, void* stream);

/* g[r,:] = gy[r,:] * act'(y[r,:]) using the forward OUTPUT y (relu: y>0;
 * elu: y>0 ? 1 : y+1; tanh: 1-y^2).  g may alias gy. */
int hscn_act_bwd(const float* gy, const float* y, float* g, int64_t count, int act, void* stream);

/* Inverted dropout (reference model/mpnn.py:58, F.dropout(x, p, training) of the MPNN baseline):
 * y[i] = keep(seed, i) ? x[i] / (1 - p) : 0, keep drawn per element from Philox-4x32-10 keyed by
 * `seed` with the element number as counter (P(keep) = 1 - p).  The mask is a pure function of
 * (seed, i): the backward is the same entry on the incoming gradient with the same seed.
 * 0 <= p < 1; y may alias x. */
int hscn_dropout(const float* x, float* y, int64_t count, float p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------- *
 * a12  GCNConv propagate, unit weights, no self loops
 * (reference model/hscn.py:88-93):
 *   out[i,:] = act( sum_{p in row i} (dinv_c[col[p]] * dinv_r[i]) * h[col[p],:]  + bias
 *                   [+ out_prev[i,:] if accumulate] )
 * summed in slot order with separately rounded multiply and add (the CPU
 * reference's index_add_ order).  The backward w.r.t. h is the same entry
 * point on the transposed CSR with bias=NULL, act=identity.
 * ------------------------------------------------------------------------- */
int hscn_spmm_csr_gcn(const int32_t* rowptr, const int32_t* col,
                      const float* dinv_r /*[num_rows]*/, const float* dinv_c /*[num_cols]*/,
                      const float* h, const float* bias /*or NULL*/, float* out,
                      int64_t num_rows, int width, int accumulate, int act, void* stream);

/* a3  GraphConv propagate with per-edge weights (reference model/hscn.py:32,40;
 * SURVEY.md A.2): out[i,:] = sum_{p in row i} w[eid[p]] * x[col[p],:]
 * (w NULL = unit weights; eid NULL = weights already in slot order). */
int hscn_spmm_csr_weighted(const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                           const float* w, const float* x, float* out,
                           int64_t num_rows, int width, void* stream);

/* ------------------------------------------------------------------------- *
 * a13  GATConv (heads=1, bipartite, add_self_loops=False) attention part
 * (reference model/hscn.py:85-87).  CSR keyed by target v:
 *   e_p    = leaky_relu(a_src[col[p]] + a_dst[v], slope)
 *   alpha_p= exp(e_p - max_row) / (sum_row exp(e_p - max_row) + 1e-16)
 *   out[v,:] = act( sum_p alpha_p * h_src[col[p],:] + bias [+ out_prev[v,:]] )
 * alpha (slot order) is kept for the backward.
 * ------------------------------------------------------------------------- */
int hscn_gat_segment_fwd(const int32_t* rowptr, const int32_t* col,
                         const float* a_src, const float* a_dst, const float* h_src,
                         const float* bias /*or NULL*/, float* alpha /*[E]*/, float* out,
                         int64_t num_dst, int width, float slope, int accumulate, int act, void* stream);

/* Backward, target side: given g = dL/d(pre-activation out) [num_dst,width]
 *   g_pre[p]  = dL/d(a_src[col[p]] + a_dst[v])   (slot order)
 *   g_a_dst[v]= sum_p g_pre[p] */
int hscn_gat_segment_bwd_dst(const int32_t* rowptr, const int32_t* col,
                             const float* a_src, const float* a_dst, const float* h_src,
                             const float* alpha, const float* g,
                             float* g_pre /*[E]*/, float* g_a_dst /*[num_dst]*/,
                             int64_t num_dst, int width, float slope, void* stream);

/* Backward, source side over the transposed CSR (keyed by source j):
 *   g_a_src[j]   = sum_q g_pre[pos_t[q]]
 *   g_h_src[j,:] = sum_q alpha[pos_t[q]] * g[col_t[q],:]  +  g_a_src[j] * att_src[:] */
int hscn_gat_segment_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* pos_t,
                             const float* alpha, const float* g_pre, const float* g,
                             const float* att_src /*[width]*/,
                             float* g_a_src /*[num_src]*/, float* g_h_src /*[num_src,width]*/,
                             int64_t num_src, int width, void* stream);

/* ------------------------------------------------------------------------- *
 * ABI 21: GATConv(in, out) of the MPNN baseline -- heads=1, homogeneous, add_self_loops=True, ONE shared
 * transform h = x W^T feeding both attention dots (reference model/mpnn.py:29-32,52,59 with
 * config/config.py:19-23 CONV_DICT["gat"]; PyG 2.2/2.3 GATConv).  Narrow-row kernels (csrc/gat_loops.hip): a row is
 * owned by a lane group sized to the width, a wave covers several rows, each group walks its row serially.
 *
 * rowptr / col (and rowptr_t / col_t) are the stable CSRs of the RAW edge list keyed by target (by source), as
 * hscn_csr_build_pair makes them, num_nodes rows each.  Entries with col == row are skipped in the kernel and the
 * node's own term is added last: the result and the summation order are those of the bipartite operator over
 * remove_self_loops + add_self_loops(edge_index), with nothing of data-dependent shape on the host.  Per target v,
 * e over its kept in-entries followed by the loop v -> v:
 *   z_e      = leaky_relu(a_src[src_e] + a_dst[v], slope)
 *   alpha_e  = exp(z_e - max_v) / (sum_v exp(z_e - max_v) + 1e-16)
 *   out[v,:] = act( sum_e alpha_e h[src_e,:] + bias )
 * Nothing is kept per edge.  Caller-allocated hand-over buffers:
 *   stat [num_nodes,2]  forward -> both backwards: {max_v, sum_v exp + 1e-16}; alpha is recomputed from it
 *   tsum [num_nodes]    bwd_dst -> bwd_src: sum_e alpha_e (g[v,:] . h[src_e,:])
 *   g_a  [num_nodes,2]  {dL/da_src[j], dL/da_dst[j]} interleaved: bwd_dst writes column 1, bwd_src reads it and
 *                       writes column 0 (one [N,2]^T [N,width] product then gives both attention-vector gradients)
 * Call order in the backward: hscn_gat_loop_bwd_dst, then hscn_gat_loop_bwd_src on the same stream.
 *   g      = dL/d(pre-activation out) [num_nodes,width]
 *   g_h[j,:] = sum_{e: src_e = j} alpha_e g[dst_e,:] + g_a[j,0] att_src + g_a[j,1] att_dst   (= dL/dh, complete)
 * Rows of any in-degree are correct; width <= 256 when width % 4 == 0 (16-byte access), width <= 64 otherwise
 * (HSCN_E_UNSUPPORTED beyond).  bias may be NULL.  Null pointers / negative sizes / an unknown act: HSCN_E_BADARG.
 * ------------------------------------------------------------------------- */
int hscn_gat_loop_fwd(const int32_t* rowptr, const int32_t* col,
                      const float* a_src /*[num_nodes]*/, const float* a_dst /*[num_nodes]*/, const float* h,
                      const float* bias /*or NULL*/, float* stat /*[num_nodes,2]*/, float* out,
                      int64_t num_nodes, int width, float slope, int act, void* stream);
int hscn_gat_loop_bwd_dst(const int32_t* rowptr, const int32_t* col,
                          const float* a_src, const float* a_dst, const float* h, const float* stat,
                          const float* g, float* tsum /*[num_nodes]*/, float* g_a /*[num_nodes,2], column 1*/,
                          int64_t num_nodes, int width, float slope, void* stream);
int hscn_gat_loop_bwd_src(const int32_t* rowptr_t, const int32_t* col_t,
                          const float* a_src, const float* a_dst, const float* h, const float* stat,
                          const float* tsum, const float* g,
                          const float* att_src /*[width]*/, const float* att_dst /*[width]*/,
                          float* g_a /*[num_nodes,2], column 0 written, column 1 read*/,
                          float* g_h /*[num_nodes,width]*/,
                          int64_t num_nodes, int width, float slope, void* stream);

/* ------------------------------------------------------------------------- *
 * a14  global_mean_pool (reference model/hscn.py:111).
 * Segments given as CSR over graphs: out[g,:] = mean_{p in seg g} x[node[p],:]
 * (node NULL = identity, i.e. sorted batch vector with ptr = rowptr);
 * empty segments give 0.  Backward: g_x[i,:] = g_out[batch[i],:] / count. */
int hscn_segment_mean_fwd(const int32_t* rowptr, const int32_t* node, const float* x, float* out,
                          int64_t num_segments, int width, void* stream);
int hscn_segment_mean_bwd(const int32_t* rowptr, const int64_t* batch /*[num_nodes]*/, const float* g_out,
                          float* g_x, int64_t num_nodes, int width, void* stream);

/* ------------------------------------------------------------------------- *
 * DMoN modularity pooling (Tsitsulin et al., "Graph Clustering with Graph Neural Networks"; PyG dense_dmon_pool)
 * on the same edge-list route and with the same operands as a6: A = the edge list with multiplicities, never
 * densified; d_i = out-degree of i (|row i| of the CSR keyed by edge ROW), 2m = sum_i d_i, S = softmax(logits).
 *   spectral_g = -( sum_i S_i . (A S)_i - sum_k (d^T S)_k^2 / 2m ) / 2m     (0 for a graph with 2m = 0)
 *   ortho_g    = | S^T S / |S^T S|_F - I / sqrt(K) |_F                       (a6's term)
 *   cluster_g  = | sum_i S_i |_2 sqrt(K) / n - 1
 * Per graph outputs (pooled_x / pooled_adj may be NULL):
 *   S        [N,K]
 *   stats    [G,8]   {sum_i S_i.(A S)_i, 2m, sum_k (d^T S)_k^2 / 2m, |S^T S|_F, ortho_g, |sum_i S_i|_2,
 *                     spectral_g, cluster_g}
 *   ss       [G,K,K] S^T S
 *   vec      [G,2,K] {d^T S, sum_i S_i}, kept for the backward
 *   pooled_x [G,K,Fx] selu(S^T X)
 *   pooled_adj[G,K,K] normalised S^T A S (zero diagonal, d^-1/2 scaling)
 *   losses   [3]     means over the graphs {spectral, ortho, cluster}
 * K in [1,256]; HSCN_E_UNSUPPORTED when one graph's accumulators exceed a CU's LDS:
 *   forward  (2 K^2 + K Fx + 35 K + 16 Fx + 20) * 4 bytes,  backward (K^2 + 34 K + 20) * 4 bytes.
 * Every check precedes the first launch.  A graph without nodes is outside the contract.
 * ------------------------------------------------------------------------- */
int hscn_dmon_sparse_fwd(const float* logits, const float* x /*or NULL*/,
                         const int32_t* rowptr, const int32_t* col, const int32_t* node_ptr,
                         float* S, float* stats, float* ss, float* vec, float* pooled_x, float* pooled_adj,
                         float* losses, int64_t num_nodes, int64_t num_graphs, int K, int Fx, void* stream);

/* dL/dlogits [N,K] (written once, plain stores) given g_losses = {dL/dspectral, dL/dortho, dL/dcluster} on the
 * device.  rowptr/col keyed by ROW, rowptr_t/col_t keyed by COL: A need not be symmetric. */
int hscn_dmon_sparse_bwd(const float* S, const float* stats, const float* ss, const float* vec,
                         const int32_t* rowptr, const int32_t* col,
                         const int32_t* rowptr_t, const int32_t* col_t, const int32_t* node_ptr,
                         const float* g_losses /*[3] device*/, float* g_logits,
                         int64_t num_nodes, int64_t num_graphs, int K, void* stream);

/* ------------------------------------------------------------------------- *
 * a6  dense_mincut_pool on the sparse (edge list) route
 * (reference model/hscn.py:61-63).  A = sum_e E[row_e, col_e]
 * is never densified: tr(S^T A S) = sum_e s_row . s_col,
 * tr(S^T D S) = sum_i d_i |s_i|^2, d_i = out-degree of i in the edge list.
 * Graph g owns nodes [node_ptr[g], node_ptr[g+1]).  CSR keyed by edge ROW.
 * Per graph outputs (any of pooled_x / pooled_adj may be NULL):
 *   S        [N,K]   softmax(logits)                 (hscn.py:64 first return)
 *   stats    [G,4]   {num, den, |S^T S|_F, ortho_g}
 *   ss       [G,K,K] S^T S
 *   pooled_x [G,K,Fx] S^T X                          (A.4 `out`)
 *   pooled_adj[G,K,K] normalised S^T A S (zero diagonal, d^-1/2 scaling)
 *   losses   [2]     {mean_g(-num/den), mean_g(ortho_g)}
 * ------------------------------------------------------------------------- */
int hscn_mincut_sparse_fwd(const float* logits, const float* x /*or NULL*/,
                           const int32_t* rowptr, const int32_t* col, const int32_t* node_ptr,
                           float* S, float* stats, float* ss, float* pooled_x, float* pooled_adj,
                           float* losses, int64_t num_nodes, int64_t num_graphs, int K, int Fx, void* stream);

/* dL/dlogits [N,K] given upstream scalars g_losses_host = {dL/dmincut, dL/dortho}
 * passed BY VALUE (host floats).  rowptr/col keyed by ROW, rowptr_t/col_t keyed by COL. */
int hscn_mincut_sparse_bwd(const float* S, const float* stats, const float* ss,
                           const int32_t* rowptr, const int32_t* col,
                           const int32_t* rowptr_t, const int32_t* col_t, const int32_t* node_ptr,
                           const float* g_losses /*[2] device*/, float* g_logits,
                           int64_t num_nodes, int64_t num_graphs, int K, void* stream);

/* The same for a batch of graphs of DIFFERENT sizes (BASELINE.json configs[3]: PascalVOC-SP, n in [395, 500]; the
 * reference's own call is one graph at a time, model/hscn.py:61-63, so any n per call must work): node-indexed
 * operands (logits, x, S, AS, deg, AtS, sg_ws, g_logits) are flat [N, width] arrays -- graph b owns rows
 * [nptr[b], nptr[b + 1]) -- the adjacency is [B, nmax, nmax] with zeros beyond a graph's n_b (nmax = the largest n_b),
 * the per-graph results (stats [B,4], ss / pooled_adj [B,K,K], pooled_x [B,K,F]) keep their shapes.  gid [N] int32 = graph
 * of every node.  Values per graph identical to the uniform entry points on that graph alone; losses = mean over graphs.
 * adj_elem_bytes = 4: float adjacency [B, nmax, nmax]; = 1: the same counts as bytes, [B, nmax, lda8] with
 * lda8 = nmax rounded up to 32 (hscn_to_dense_adj_ragged_u8): the A S / A^T S products stream the adjacency, a quarter
 * of the bytes, converted exactly on the way to the matrix cores (v_mfma_f32_32x32x2_f32, 128-row tiles). */
int hscn_mincut_dense_ragged_fwd(const float* x /*[N,F] or NULL*/, const void* adj, int adj_elem_bytes,
                                 const float* logits /*[N,K]*/, const int32_t* nptr /*[B+1]*/, int64_t N, int64_t B,
                                 int nmax, int K, int F, float* S, float* AS, float* deg /*[N]*/, float* stats,
                                 float* ss, float* pooled_x, float* pooled_adj, float* losses /*[2]*/, void* stream);
int hscn_mincut_dense_ragged_bwd(const void* adj, int adj_elem_bytes, const float* S, const float* AS, const float* deg,
                                 const float* stats, const float* ss, const float* g_losses /*[2]*/,
                                 const int32_t* nptr, const int32_t* gid /*[N]*/, int64_t N, int64_t B, int nmax, int K,
                                 float* AtS, float* sg_ws, float* gss_ws /*[B,K,K]*/, float* g_logits, void* stream);
/* ABI 18: undirected graphs -- the norm in the reference's datasets -- have A^T = A, so the backward's A^T S is the forward's
 * A S.  hscn_dense_adj_asymmetry_u8 sets asym[b] (int32 [B], ZERO on entry) to 1 for every graph of a ragged byte
 * adjacency ([B, nmax, lda8], hscn_to_dense_adj_ragged_u8) that is NOT symmetric (one pass of 64 x 64 tile pairs);
 * hscn_mincut_dense_ragged_bwd_sym = hscn_mincut_dense_ragged_bwd with those flags (asym may be NULL = the general
 * form): graphs with asym[b] == 0 skip the A^T S product -- the largest launch of the backward -- and read AS.
 * Same gradients bit for bit (A^T S and A S are the same sums over the same entries in the same order). */
int hscn_dense_adj_asymmetry_u8(const void* adj8, int64_t B, int nmax, int32_t* asym /*[B]*/, void* stream);
int hscn_mincut_dense_ragged_bwd_sym(const void* adj, int adj_elem_bytes, const float* S, const float* AS, const float* deg,
                                     const float* stats, const float* ss, const float* g_losses /*[2] device*/,
                                     const int32_t* nptr, const int32_t* gid, int64_t N, int64_t B, int nmax, int K,
                                     float* AtS, float* sg_ws, float* gss_ws, float* g_logits,
                                     const int32_t* asym /*[B] or NULL*/, void* stream);

/* ABI 17: the adjacency product of the dense route by itself -- out [N,K] = op(A) S per graph of a ragged batch (the
 * A S of dense_mincut_pool, reference model/hscn.py:63 -> PyG dense_mincut_pool's `torch.matmul(adj, s)`; transA = 1: the
 * A^T S its backward needs), deg [N] (optional, transA = 0) = row sums of A.  The launch hscn_mincut_dense_ragged_fwd /
 * _bwd issue for it; exposed so the route's dominant kernel can be timed alone (bench.py's stage_a_dense roofline). */
int hscn_dense_adj_s(const void* adj, int adj_elem_bytes, const float* S /*[N,K]*/, const int32_t* nptr /*[B+1]*/,
                     int64_t B, int nmax, int K, int transA, float* out /*[N,K]*/, float* deg /*[N] or NULL*/,
                     void* stream);


/* ------------------------------------------------------------------------- *
 * a6  dense_mincut_pool, dense route on the matrix cores (reference model/hscn.py:61-63
 * with the dense [B,n,n] adjacency PyG's to_dense_adj builds; BASELINE config 4).
 * hscn_bgemm_f32: C[b] (M x N) = op(A[b]) * B[b] with exact-fp32 MFMA
 * (v_mfma_f32_16x16x4_f32), N <= 64, transA: A stored [Kd, M].
 * hscn_mincut_dense_fwd runs softmax, deg = A 1, A S, S^T(A S), S^T S, S^T X, the two
 * losses and the normalised coarse adjacency; AS [B,n,K] and deg [B,n] are kept for the
 * backward, which adds A^T S and returns dL/dlogits given g_losses = {dL/dmincut, dL/dortho}.
 * ------------------------------------------------------------------------- */
int hscn_bgemm_f32(const float* A, const float* B, float* C, int64_t batch, int M, int N, int Kd,
                   int64_t lda, int64_t ldb, int64_t ldc, int64_t strideA, int64_t strideB, int64_t strideC,
                   int transA, void* stream);
int hscn_mincut_dense_fwd(const float* x /*[B,n,F] or NULL*/, const float* adj /*[B,n,n]*/,
                          const float* logits /*[B,n,K]*/, int64_t B, int n, int K, int F,
                          float* S, float* AS, float* deg, float* stats /*[B,4]*/, float* ss /*[B,K,K]*/,
                          float* pooled_x /*[B,K,F] or NULL*/, float* pooled_adj /*[B,K,K]*/, float* losses /*[2]*/,
                          void* stream);
int hscn_mincut_dense_bwd(const float* adj, const float* S, const float* AS, const float* deg, const float* stats,
                          const float* ss, const float* g_losses /*[2] device*/, int64_t B, int n, int K,
                          float* AtS_workspace /*[B,n,K]*/, float* SG_workspace /*[B,n,K]*/,
                          float* Gss_workspace /*[B,K,K]*/, float* g_logits /*[B,n,K]*/, void* stream);

/* a7  cluster assignment (reference train/train_clustering.py:68):
 * ids[i] = first index of the row maximum of S[i,:]. */
int hscn_assign_argmax(const float* S, int64_t* ids, int64_t num_nodes, int K, void* stream);

/* ------------------------------------------------------------------------- *
 * a8  generate_hetero_data + PyG collate on the device (reference
 * loader/hetero_data.py:42-87; SURVEY.md B.1 quirks kept, bit-exact).
 * A batch of graphs (node ranges nptr) with raw cluster ids per node (K <= 64):
 *   count: U[g] = distinct ids, lvl[i] = remapped id of node i (np.unique order),
 *          means[g,v,:] = float32(float64 mean, node order) of remapped cluster (v+1) mod U[g]
 *   scan : vptr = exclusive cumsum(U), evptr = exclusive cumsum(U(U+1)/2) as int64 [B+1] (PyG ptr) and
 *          int32 [B+1] (resident kernels), totals [4] = {V, E_vv, flag word, max U}: the one thing the host
 *          reads back, because the outputs have data-dependent sizes
 *   emit : virtual_x [V,F]; ei_lv [2,N] = {node, vptr[g] + lvl}; ei_vv [2,Evv] = {(i -> j): i+j <= U-1}
 *          in the reference's order, offset by vptr; vbatch [V] (or NULL) = graph id of every virtual node.
 * x is int64 (atom features) or fp32; flag bit 8: a cluster id outside [0,K).
 * ------------------------------------------------------------------------- */
int hscn_build_hetero_count(const void* x, int x_is_int64, const int64_t* clusters, const int32_t* nptr,
                            int64_t B, int F, int K, int32_t* U /*[B]*/, int32_t* lvl /*[N]*/,
                            float* means /*[B,K,F]*/, int32_t* flag, void* stream);
int hscn_build_hetero_scan(const int32_t* U, int64_t B, const int32_t* flag /*or NULL*/, int64_t* vptr /*[B+1]*/,
                           int64_t* evptr /*[B+1]*/, int32_t* vptr32 /*[B+1]*/, int32_t* evptr32 /*[B+1]*/,
                           int64_t* totals /*[4]*/, void* stream);
int hscn_build_hetero_emit(const int32_t* U, const int64_t* vptr /*[B+1]*/, const int64_t* evptr /*[B+1]*/,
                           const int32_t* nptr, const int32_t* lvl, const float* means, int64_t B, int F, int K,
                           int64_t N, int64_t Evv, float* virtual_x, int64_t* ei_lv, int64_t* ei_vv,
                           int64_t* vbatch /*[V] or NULL*/, void* stream);

/* a5  to_dense_adj (reference model/hscn.py:61): adj must be
 * zero-filled by the caller's stream order; adj[row_e*n + col_e] += 1. */
int hscn_to_dense_adj(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t n,
                      float* adj /*[n,n]*/, void* stream);
/* the same for a block-diagonal batch of B graphs with n nodes each: adj [B,n,n] (zero on entry); what
 * to_dense_adj(edge_index, batch) gives for equally sized graphs -- the input of the dense MinCUT route */
int hscn_to_dense_adj_batched(const int64_t* row, const int64_t* col, int64_t E, int64_t B, int64_t n, float* adj,
                              void* stream);
/* to_dense_adj(edge_index, batch) for graphs of different sizes: adj [B, nmax, nmax], ZERO on entry.  mode 0: every
 * edge of the list counts (to_dense_adj on the list as given, reference model/hscn.py:61); mode 1: the list's self
 * loops are skipped and the identity added -- what gcn_norm's add_remaining_self_loops followed by to_dense_adj
 * (train/train_clustering.py:37-42 then model/hscn.py:61) yields from RAW edges. */
int hscn_to_dense_adj_ragged(const int64_t* row, const int64_t* col, int64_t E, const int32_t* nptr /*[B+1]*/,
                             const int32_t* gid /*[N]*/, int64_t N, int64_t B, int64_t nmax, int mode, float* adj,
                             void* stream);
/* ... as bytes: adj8 [B, nmax, lda8], lda8 = nmax rounded up to 32, ZERO on entry (4-byte aligned); flag (optional) gets
 * bit 16 when an entry would pass 255. */
int hscn_to_dense_adj_ragged_u8(const int64_t* row, const int64_t* col, int64_t E, const int32_t* nptr,
                                const int32_t* gid, int64_t N, int64_t B, int64_t nmax, int mode, uint8_t* adj8,
                                int32_t* flag, void* stream);
/* gcn_norm's self-loop bookkeeping (PyG add_remaining_self_loops; train/train_clustering.py:37-42) with a STATIC output
 * shape [E + N] -- capturable, no data-dependent size: the E input edges keep their slots (an input self loop stays
 * in place with weight 0, its weight moves to the node's loop), then one loop per node (weight = the moved one or
 * `fill`).  Degrees and aggregations over this list equal PyG's over its shorter one. */
int hscn_gcn_norm_self_loops(const int64_t* row, const int64_t* col, const float* w /*[E] or NULL = ones*/, int64_t E,
                             int64_t N, float fill, int64_t* row_out /*[E+N]*/, int64_t* col_out, float* w_out,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * Collate on the device (reference: the PyG DataLoader collates HeteroData on the host for every step,
 * loader/hetero_data.py:91-106, loader/loader.py:48-60).  The hetero dataset stays in HBM as
 * concatenated arrays with per-graph LOCAL node ids; hscn_collate_gather writes the batch made of graphs
 * ids[0..B) -- features, batch vectors, targets, edge lists re-based to batch numbering (int64 [2, ecap] as the
 * reference's edge_index), int64 / int32 per-graph segment tables -- into fixed-capacity buffers, bit for bit
 * what Batch.from_data_list produces for that list of graphs.  One launch, no host synchronisation.
 * Relations in the order ll, vv, lv (source type local, virtual, local; target type local, virtual, virtual).
 * flag bit 8: an id outside [0, G) or a batch beyond a capacity (the offending part is not written).
 * cursor (optional, device int32): the batch is ids[cursor[0]*B .. +B) -- `ids` is then a whole epoch's
 * permutation -- and a one-thread launch behind the gather increments it, so a captured sequence of launches
 * walks through the epoch by itself, one slice per replay (the caller re-fills `ids` and zeroes the cursor
 * between epochs and must not replay past the permutation's end). */
typedef struct hscn_hetero_dataset {
  const float* x_local;    /* [N,F] */
  const float* x_virtual;  /* [V,F] */
  const float* y;          /* [G,C] or NULL */
  const int64_t* nptr;     /* [G+1] local-node ranges */
  const int64_t* vptr;     /* [G+1] virtual-node ranges */
  const int32_t* src[3];   /* per relation: source ids local to the graph */
  const int32_t* dst[3];   /* per relation: target ids local to the graph */
  const int64_t* eptr[3];  /* per relation: [G+1] edge ranges */
  int64_t G;
  int32_t F, C;
} hscn_hetero_dataset;
typedef struct hscn_hetero_batch_out {
  float *x_local, *x_virtual, *y;                /* [ncap,F] [vcap,F] [B,C] (y NULL iff the dataset has none) */
  int64_t *ptr_local, *ptr_virtual;              /* [B+1] */
  int32_t *ptr32_local, *ptr32_virtual;          /* [B+1] */
  int64_t *batch_local, *batch_virtual;          /* [ncap] [vcap] graph slot of every node */
  int64_t* ei[3];                                /* [2, ecap[r]] */
  int32_t* eptr32[3];                            /* [B+1] */
  int64_t ncap, vcap, ecap[3];
} hscn_hetero_batch_out;
int hscn_collate_gather(const hscn_hetero_dataset* dataset, const int64_t* ids /*[B] device*/, int64_t B,
                        const hscn_hetero_batch_out* out, int32_t* flag, int32_t* cursor /*device [1] or NULL*/,
                        const int32_t* cursor_base /*device [1] or NULL*/, void* stream);
/* cursor_base != NULL: `cursor` is a counter that somebody else advances once per training step -- word 0 of the
 * sync buffer of hscn_resident_train_step -- and the slice taken is cursor[0] - cursor_base[0]; the call then issues
 * no launch of its own to advance anything (cursor_base is set to the counter's value when an epoch starts). */

/* ------------------------------------------------------------------------- *
 * Loss tail (reference graph_hscn/loss.py:6-19, called at train/train.py:82) on the
 * [B,C] prediction, kind 0 = BCEWithLogits(mean), 1 = L1(mean):
 *   loss[0] = mean loss, score = sigmoid(pred) (may be NULL), grad = dloss/dpred.
 * hscn_scale: y = g[0] * x (the backward of the loss given the upstream scalar).
 * ------------------------------------------------------------------------- */
int hscn_criterion_fwd(const float* pred, const float* target, int64_t count, int kind,
                       float* loss /*[1]*/, float* score /*[count] or NULL*/, float* grad /*[count]*/,
                       void* stream);
int hscn_scale(const float* g /*[1]*/, const float* x, float* y, int64_t count, void* stream);

/* The multiclass branch of the same criterion (loss.py:11-14: nll_loss(log_softmax(pred, -1), true), class-index
 * targets, mean reduction; class weights and ignore_index: hscn_softmax_nll_fwd_ex below), csrc/loss.hip.  Purely additive to ABI 23.
 *   pred [R, C] f32 row-major, target [R] i64;  1 <= C <= 1024 (HSCN_E_BADARG beyond: a row is held by one 64-lane
 *   group, 16 columns per lane), R >= 1 is not bounded by a workgroup (a per-node [N, C] prediction is served).
 *   logp [R, C] (may be NULL) = pred - max - log sum exp(pred - max), the "score" the reference returns;
 *   loss [1] = -(1/R) sum_r logp[r, target[r]];  grad [R, C] = (exp(logp) - onehot(target)) / R = dloss/dpred.
 *   flags [1] i32: the call ORs bits IN (the caller zeroes the word when it wants a fresh reading):
 *     bit 0 = a target outside [0, C) -- that row adds nothing to the loss, its gradient row is zero, its logp row
 *     is still written, nothing is read out of bounds; bit 1 = a NaN in pred.
 *   Rows map to aligned lane groups of the smallest power of two >= C (64 for C > 64); a workgroup owns 256 rows.
 *   R <= 256 is ONE launch.  Beyond, every workgroup writes its partial sum to `workspace`
 *   (hscn_softmax_nll_workspace_bytes(R, C) bytes: 4 per workgroup, 0 for R <= 256 -- workspace may then be NULL;
 *   0 also for arguments the call refuses) and a one-workgroup launch adds them in index order.  No float atomics:
 *   two calls on the same input give the same bits.  HSCN_E_BADARG for R < 1, C outside [1, 1024], a NULL pred,
 *   target, loss, grad or flags, or a NULL workspace where one is needed; HSCN_E_WORKSPACE for one too small; all
 *   before any launch. */
size_t hscn_softmax_nll_workspace_bytes(int64_t R, int C);
int hscn_softmax_nll_fwd(const float* pred, const int64_t* target, int64_t R, int C, float* loss /*[1]*/,
                         float* logp /*[R,C] or NULL*/, float* grad /*[R,C]*/, int32_t* flags /*[1]*/,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Class weights and ignore_index of the multiclass criterion (F.cross_entropy(pred, true, weight=w, ignore_index=i);
 * LRGB's weighted_cross_entropy), csrc/loss.hip.  Two calls; nothing is read back by the host.  Purely additive to
 * ABI 23.
 *
 * hscn_class_weights: target [R] i64, 1 <= R < 2^31, 1 <= C <= 1024.  A row equal to ignore_index is not counted and
 *   raises no flag; any other row outside [0, C) ORs bit 0 into flags (the word of hscn_softmax_nll_fwd) and is not
 *   counted.
 *     counts [C] i32 (zeroed by the call): rows per class -- a per-workgroup LDS histogram, then integer adds: any
 *       order gives the same bits;
 *     weight [C] f32: mode HSCN_CW_NONE = ones; HSCN_CW_GIVEN = weight_in [C] copied; HSCN_CW_BATCH = with V the
 *       number of counted rows and n_c = counts[c]: (float)(V - n_c) / (float)V where n_c > 0, else 0 (float32
 *       division, round to nearest: torch's (V - n).float() / V);
 *     denom [1] f64 = sum_c n_c * weight[c], added in double in class order by one thread.
 *   Three launches on the stream (zero, count, finish).  HSCN_E_BADARG for null pointers (weight_in may be NULL
 *   unless mode is HSCN_CW_GIVEN), R or C outside their ranges or an unknown mode, before any launch.
 *
 * hscn_softmax_nll_fwd_ex: hscn_softmax_nll_fwd with weight [C] f32 (or NULL: ones), ignore_index and denom [1] f64,
 *   the DEVICE value hscn_class_weights wrote for the same targets:
 *     loss = sum over the counted rows of weight[target] * (-logp[r, target]) / denom;
 *     grad row = weight[target] * (exp(logp) - onehot(target)) / denom for a counted row, zero for an ignored row or
 *       one whose target is out of range (bit 0 of flags; an ignored row raises nothing); logp is written for every
 *       row.
 *   The same row mapping, workspace (hscn_softmax_nll_workspace_bytes) and ordered fold.  With weight = NULL and no
 *   row ignored denom is R and loss, logp and grad are hscn_softmax_nll_fwd's, bit for bit.
 *   denom == 0 (every row ignored, or every class present has weight 0 -- HSCN_CW_BATCH with one class present) is
 *   what torch computes on the CPU, 0 / 0: the loss is NaN, the gradient of a counted row is NaN (0 * inf) and that
 *   of an ignored row 0.
 *   HSCN_E_BADARG / HSCN_E_WORKSPACE as hscn_softmax_nll_fwd, and HSCN_E_BADARG for a NULL denom. */
#define HSCN_CW_NONE 0
#define HSCN_CW_GIVEN 1
#define HSCN_CW_BATCH 2
int hscn_class_weights(const int64_t* target, int64_t R, int C, int64_t ignore_index, int mode,
                       const float* weight_in /*[C] or NULL*/, int32_t* counts /*[C]*/, float* weight /*[C]*/,
                       double* denom /*[1]*/, int32_t* flags /*[1]*/, void* stream);
int hscn_softmax_nll_fwd_ex(const float* pred, const int64_t* target, int64_t R, int C,
                            const float* weight /*[C] or NULL*/, int64_t ignore_index, const double* denom /*[1]*/,
                            float* loss /*[1]*/, float* logp /*[R,C] or NULL*/, float* grad /*[R,C]*/,
                            int32_t* flags /*[1]*/, void* workspace, size_t workspace_bytes, void* stream);

/* The per-node head of a node-level model, pred = lin_2(act(lin_1(x))) on every row of x [N, H]
 * (graph_hscn.nn.head.NodeHead; csrc/node_head.hip).  Purely additive to ABI 23.
 *   x [N, H], W1 [H, H], b1 [H], W2 [C, H], b2 [C], pred / g_pred [N, C], all f32 row-major; act: HSCN_ACT_*.
 * hscn_node_head_supported: the envelope, H in {16, 32, 64} and 1 <= C <= 64 (the single source of truth: the two
 *   launches answer HSCN_E_UNSUPPORTED outside it).
 * hscn_node_head_fwd: ONE launch, a lane per row, hscn_node_head_rows_per_workgroup() = 256 rows per workgroup; the
 *   hidden row stays in registers, only pred is written.  N = 0 launches nothing.
 * hscn_node_head_bwd: one launch plus one ordered fold.  scale [1] (or NULL = 1): a device scalar g_pred is multiplied
 *   by on the way in (a loss.LazyScaled gradient is consumed unmultiplied).  The hidden row is recomputed from x.
 *   g_x [N, H] (or NULL: not wanted); gW1 [H, H], gb1 [H], gW2 [C, H], gb2 [C].  Every workgroup (at most 256; a
 *   workgroup strides over the 256-row tiles) sums its rows' parameter terms in row order and writes them to its row
 *   of `workspace` (hscn_node_head_workspace_bytes(N, H, C) = workgroups * (H + C) * (H + 1) * 4; 0 for arguments the
 *   call refuses); a one-workgroup launch adds the rows in workgroup order and stores the four gradients, or with
 *   accumulate = 1 adds the sum last into what they hold.  No float atomics: the same input gives the same bits.
 *   x and g_x are read and written as float4: both must be 16-byte aligned (rows of H floats keep the alignment).
 * HSCN_E_BADARG: null pointers, an x or g_x that is not 16-byte aligned, an unknown act, accumulate outside {0, 1},
 *   N < 0 (fwd) / N < 1 (bwd) or N > 2^31; HSCN_E_UNSUPPORTED outside the envelope, or where the device refuses the
 *   backward's LDS (up to 97 KB at H = C = 64); HSCN_E_WORKSPACE for a workspace too small; all before any launch. */
int hscn_node_head_supported(int H, int C);
int hscn_node_head_rows_per_workgroup(void);
size_t hscn_node_head_workspace_bytes(int64_t N, int H, int C);
int hscn_node_head_fwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2, int64_t N,
                       int H, int C, int act, float* pred, void* stream);
int hscn_node_head_bwd(const float* x, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* g_pred, const float* scale /*[1] or NULL*/, int64_t N, int H, int C, int act,
                       float* g_x /*[N,H] or NULL*/, float* gW1, float* gb1, float* gW2, float* gb2, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * a10  HSCN.forward / backward, graph-resident engine
 * (reference model/hscn.py:102-114 with lv=GAT, ll=GCN, vv=GCN; the loop
 * train/train.py:76,87 drives it).  The batch must be block-diagonal with graph
 * g owning local nodes [lptr[g],lptr[g+1]), virtual nodes [vptr[g],vptr[g+1])
 * and the edge slices [eptr_*[g],eptr_*[g+1]) of each relation's int64 [2,E]
 * COO list (what PyG's collate produces).  One workgroup per graph keeps the
 * graph's features and CSR in LDS for all L layers.
 *   layer_params_host: HOST array of L x 9 device pointers per layer
 *     {W_ll[H,fin], b_ll[H], W_vv[H,fin], b_vv[H], W_src[H,fin], W_dst[H,fin],
 *      att_src[H], att_dst[H], b_gat[H]},  fin = F for layer 0, else H
 *   acts [L,N,H]: post-ReLU local features of every layer (kept for backward)
 *   pooled [B,H], z [B,H] (head hidden, post-activation), pred [B,C]
 *   xv_out [V,H] or NULL: final virtual features (never used by the prediction
 *     in the reference architecture; exposed so the virtual branch is testable)
 *   compute_virtual: 1 = both branches in one launch; 0 = local chain + head only (the virtual
 *     branch cannot change pred); 2 = virtual branch only: `acts` is an INPUT holding what a mode-0
 *     launch of the same batch stored, xv_out is required, pooled / z / pred / head weights / CSR
 *     export are not touched (may be NULL).  Modes 0 + 2 on two streams give the results of mode 1
 *     with the virtual branch off the critical path of the step.
 *   csr_rowptr_t / csr_col_t / dinv: the local->local CSR keyed by SOURCE (graph g: rowptr at
 *     lptr[g]+g, columns at eptr_ll[g]) and in-degree^-1/2, built in LDS by the forward launch and
 *     handed to the backward launch, which does not rebuild them (all three NULL = do not export)
 *   flag: bit 2 = an edge left its graph's node range, bit 4 = a graph exceeds
 *     max_n / max_v / max_ell / max_evv (the LDS budget the launch was sized for)
 *   g_scale: optional device scalar; the upstream gradient is g_scale[0] * g_pred (the factor
 *     the loss node would otherwise apply with a launch of its own, hscn_scale); NULL = 1
 *   score (forward, optional [B,C]): sigmoid(pred), the score loss.py:9-10,17-19 returns beside the loss
 *   tail (backward, optional): the loss tail of the step (loss.py:6-19 on this prediction, mean over
 *     B*C elements) rides on the backward launch: workgroup g derives its upstream gradient row
 *     g_scale[0] * d(mean loss)/dpred[g,:] from (tail->pred, tail->target) itself -- g_pred is ignored
 *     and may be NULL -- and adds the graph's loss terms as one more column of its partials row;
 *     `partials` is then [B, P+1], `grads` [P+1], and grads[P] receives the mean loss.  Same
 *     per-element arithmetic as hscn_criterion_fwd (gradients bit-identical to the three-call route).
 * hscn_resident_bwd returns dL/d{W_ll, b_ll per layer, W1, b1, W2, b2} packed in
 * that order in grads[P] (P = hscn_resident_param_count); the virtual-branch
 * parameters receive no gradient, exactly as in the reference's autograd graph.
 * ------------------------------------------------------------------------- */
typedef struct hscn_loss_tail {
  const float* pred;    /* [B,C] what the forward launch of this step wrote */
  const float* target;  /* [B,C] float32 */
  int32_t kind;         /* 0 = BCE with logits, 1 = L1 (both mean-reduced) */
} hscn_loss_tail;
int hscn_resident_supported(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv);
int64_t hscn_resident_param_count(int F, int H, int L, int C);
/* The size-dependent choices hscn_resident_fwd (compute_virtual 0 or 1) and hscn_resident_bwd make for these
 * maxima (ABI 24): host arithmetic only, no stream and no launch, through the same functions the launches take
 * them from.  want_export != 0: the forward is asked for the source-keyed CSR (csr_rowptr_t != NULL).  Fills
 * plan_host[HSCN_PLAN_COUNT]; returns 0, HSCN_E_UNSUPPORTED where hscn_resident_supported answers 0, HSCN_E_BADARG
 * for a NULL plan_host.  (The first seven fields of hscn_resident_launch_plan_ex(HSCN_LAUNCH_PAIR, ...).)
 *   HSCN_PLAN_THREADS     threads per workgroup of both launches: 256 (max_n <= 64) or 1024
 *   HSCN_PLAN_FWD_DB      1 = the forward keeps two weight buffers in LDS (H <= 32 and they fit)
 *   HSCN_PLAN_FWD_EXP     1 = the forward launch builds and exports the source-keyed CSR itself
 *   HSCN_PLAN_CSR_LAUNCH  1 = the export was wanted and did not fit: a light launch of its own builds it
 *   HSCN_PLAN_BWD_TWO     1 = the backward works in two n x H buffers instead of three
 *   HSCN_PLAN_FWD_LDS / HSCN_PLAN_BWD_LDS   dynamic LDS bytes of the two launches */
#define HSCN_PLAN_THREADS 0
#define HSCN_PLAN_FWD_DB 1
#define HSCN_PLAN_FWD_EXP 2
#define HSCN_PLAN_CSR_LAUNCH 3
#define HSCN_PLAN_BWD_TWO 4
#define HSCN_PLAN_FWD_LDS 5
#define HSCN_PLAN_BWD_LDS 6
#define HSCN_PLAN_COUNT 7
int hscn_resident_launch_plan(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv,
                              int want_export, int32_t* plan_host);
/* The same query over every stage-C launch shape (additive to ABI 24), `launch` one of
 *   HSCN_LAUNCH_PAIR          hscn_resident_fwd + hscn_resident_bwd
 *   HSCN_LAUNCH_PAIR_VIRTUAL  hscn_resident_fwd_with_virtual + hscn_resident_bwd_with_virtual (max_v / max_evv: the
 *                             job's; the forward is taken to be handed a non-NULL ei_ll; L >= 2 is the entry point's
 *                             own check, not looked at here)
 *   HSCN_LAUNCH_STEP          hscn_resident_train_step without a job (max_v, max_evv and want_export are ignored)
 *   HSCN_LAUNCH_STEP_VIRTUAL  hscn_resident_train_step with a job (want_export is ignored)
 * Fills plan_host[HSCN_PLAN_EX_COUNT] (zeros where the launch shape is refused): the seven fields above, where the forward fields describe the LOCAL workgroup's
 * argument block and the one-launch step reports its single launch as the forward (HSCN_PLAN_BWD_LDS = 0), then
 *   HSCN_PLAN_CSR_LDS        dynamic LDS bytes of the light CSR launch (0 without it)
 *   HSCN_PLAN_V_DB           the virtual workgroup of the forward / of the step keeps two weight buffers
 *   HSCN_PLAN_V_EXP          1 = the forward's VIRTUAL workgroup builds and exports the source-keyed CSR
 *   HSCN_PLAN_V_ACQ          1 = the step's virtual workgroup acquires the local activations (4-wave workgroups)
 *   HSCN_PLAN_BWD_V_DB       the virtual workgroup of the backward keeps two weight buffers
 *   HSCN_PLAN_LOCAL_FIXED / HSCN_PLAN_VIRTUAL_FIXED   the step's instantiation: 1 = that program takes its LDS layout
 *                            at compile time (the local one only when the virtual one does too, or there is no job)
 *   HSCN_PLAN_FWD_LOCAL_NEED / _FWD_VIRTUAL_NEED / _BWD_LOCAL_NEED / _BWD_VIRTUAL_NEED   bytes each workgroup program
 *                            lays out in LDS for the argument block it is handed (0: no such program in the launch);
 *                            a launch's LDS is at least both of its programs'.
 * Returns 0; HSCN_E_UNSUPPORTED where hscn_resident_supported (pair) / hscn_resident_train_step_supported (step, with
 * max_v = max_evv = 0 when there is no job) answers 0; HSCN_E_BADARG for a NULL plan_host or an unknown launch. */
#define HSCN_LAUNCH_PAIR 0
#define HSCN_LAUNCH_PAIR_VIRTUAL 1
#define HSCN_LAUNCH_STEP 2
#define HSCN_LAUNCH_STEP_VIRTUAL 3
#define HSCN_PLAN_CSR_LDS 7
#define HSCN_PLAN_V_DB 8
#define HSCN_PLAN_V_EXP 9
#define HSCN_PLAN_V_ACQ 10
#define HSCN_PLAN_BWD_V_DB 11
#define HSCN_PLAN_LOCAL_FIXED 12
#define HSCN_PLAN_VIRTUAL_FIXED 13
#define HSCN_PLAN_FWD_LOCAL_NEED 14
#define HSCN_PLAN_FWD_VIRTUAL_NEED 15
#define HSCN_PLAN_BWD_LOCAL_NEED 16
#define HSCN_PLAN_BWD_VIRTUAL_NEED 17
#define HSCN_PLAN_EX_COUNT 18
int hscn_resident_launch_plan_ex(int launch, int F, int H, int L, int C, int max_n, int max_v, int max_ell,
                                 int max_evv, int want_export, int32_t* plan_host);
int hscn_resident_fwd(const void* x_local, const void* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                      const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv,
                      const int32_t* lptr, const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv,
                      const int32_t* eptr_lv, int64_t N, int64_t V, int64_t B, int F, int H, int L, int C,
                      int head_act, float slope, const void* const* layer_params_host,
                      const float* W1, const float* b1, const float* W2, const float* b2, int max_n, int max_v,
                      int max_ell, int max_evv, int compute_virtual, void* acts, float* pooled, float* z,
                      float* pred, float* score /*[B,C] or NULL*/, void* xv_out, int32_t* csr_rowptr_t /*[N+B]*/,
                      int32_t* csr_col_t /*[E_ll]*/, float* dinv /*[N]*/, int32_t* flag,
                      int flags /*HSCN_STORE_F16*/, void* stream);
int hscn_resident_bwd(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                      const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C, int head_act,
                      const void* const* W_ll_host, const float* W1, const float* W2, const void* acts,
                      const float* pooled, const float* z, const float* g_pred, const float* g_scale /*[1] or NULL*/,
                      const int32_t* csr_rowptr_t, const int32_t* csr_col_t, const float* dinv, int max_n,
                      int max_ell, float* partials /*[B,P]*/, float* grads /*[P]*/, int32_t* flag,
                      const hscn_loss_tail* tail /*or NULL*/, int flags /*HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE*/,
                      void* stream);

/* hscn_resident_bwd that also carries the virtual branch of the SAME step's forward: one launch
 * of 2B workgroups, even ones run the backward of graph g, odd ones what a compute_virtual = 2
 * hscn_resident_fwd launch would do for graph g (job->xv_out receives the final virtual features).
 * The forward of the step is then a compute_virtual = 0 launch: the virtual branch (which the
 * reference evaluates although nothing consumes it, model/hscn.py:106-111) leaves the step's
 * critical path and runs on the CUs a 128-graph batch does not occupy.  Gradients are identical
 * to hscn_resident_bwd, xv_out to the one-launch forward.  Fields as in hscn_resident_fwd. */
typedef struct hscn_virtual_job {
  const float* x_virtual;              /* [V,F] */
  const int64_t* ei_vv; int64_t E_vv;  /* [2,E_vv] */
  const int64_t* ei_lv; int64_t E_lv;  /* [2,E_lv] */
  const int32_t* vptr;                 /* [B+1] */
  const int32_t* eptr_vv;              /* [B+1] */
  const int32_t* eptr_lv;              /* [B+1] */
  const void* const* layer_params_host;/* L x 9 device pointers (host array) */
  float* xv_out;                       /* [V,H] */
  int64_t V;
  int32_t max_v, max_evv;
  float slope;                         /* GAT leaky-ReLU slope */
  /* Optional split of the virtual branch over the two launches of a step (all six NULL = the
   * backward launch runs the whole branch).  hscn_resident_fwd_with_virtual builds the virtual
   * relations' CSRs and runs layer 0 (which reads only input features) beside the local chain and
   * leaves this state; hscn_resident_bwd_with_virtual resumes at layer 1 from it. */
  int32_t* st_rowptr_lv;               /* [V+B]  (graph g: at vptr[g]+g) */
  int32_t* st_col_lv;                  /* [E_lv] local node ids, graph g at eptr_lv[g] */
  int32_t* st_rowptr_vv;               /* [V+B] */
  int32_t* st_col_vv;                  /* [E_vv] */
  float* st_dinv_v;                    /* [V] in-degree^-1/2 of the vv relation */
  float* st_xv;                        /* [V,H] virtual features after layer 0 */
} hscn_virtual_job;
/* hscn_resident_fwd with compute_virtual = 0 (local chain + head, CSR export) whose launch also
 * carries, as odd workgroups, the first part of the virtual branch described by `job` (state
 * pointers required, L >= 2).  Pair it with hscn_resident_bwd_with_virtual on the same job. */
int hscn_resident_fwd_with_virtual(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                                   const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C,
                                   int head_act, const void* const* layer_params_host, const float* W1,
                                   const float* b1, const float* W2, const float* b2, int max_n, int max_ell,
                                   void* acts, float* pooled, float* z, float* pred, float* score /*or NULL*/,
                                   int32_t* csr_rowptr_t, int32_t* csr_col_t, float* dinv, int32_t* flag,
                                   const hscn_virtual_job* job, int flags /*HSCN_STORE_F16*/, void* stream);
int hscn_resident_bwd_with_virtual(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                                   const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C,
                                   int head_act, const void* const* W_ll_host, const float* W1, const float* W2,
                                   const void* acts, const float* pooled, const float* z, const float* g_pred,
                                   const float* g_scale /*[1] or NULL*/, const int32_t* csr_rowptr_t,
                                   const int32_t* csr_col_t, const float* dinv, int max_n, int max_ell,
                                   float* partials /*[B,P]*/, float* grads /*[P]*/, int32_t* flag,
                                   const hscn_loss_tail* tail /*or NULL*/, const hscn_virtual_job* job,
                                   int flags /*HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE*/, void* stream);

/* ------------------------------------------------------------------------- *
 * structure_build = "dataset-resident".  The reference rebuilds nothing because it has no structure to build
 * (PyG scatters over the COO list every call, model/hscn.py:108-110); the resident launches build four stable CSRs
 * and two degree norms per graph in LDS every step.  Graph structure is epoch-invariant, so it can be built ONCE:
 * hscn_resident_structure fills an hscn_structure for every graph of a block-diagonal hetero batch -- or of a whole
 * dataset laid out as one batch -- with the same device functions the launches use (graph-LOCAL int32 ids; rows keep
 * ascending edge order), hscn_collate_gather_structure gathers the chosen graphs' slices next to hscn_collate_gather,
 * and hscn_resident_train_step(structure != NULL) loads instead of building.  Bit-identical results either way.
 *   graph g: ll_rowptr_* at lptr[g] + g (n+1 entries), ll_col_* at eptr_ll[g], ll_dinv at lptr[g];
 *            lv_rowptr / vv_rowptr at vptr[g] + g (nv+1), lv_col at eptr_lv[g], vv_col at eptr_vv[g], vv_dinv at vptr[g].
 * ------------------------------------------------------------------------- */
typedef struct hscn_structure {
  int32_t *ll_rowptr_d, *ll_col_d;   /* local->local keyed by target  [N+B] [E_ll] */
  int32_t *ll_rowptr_s, *ll_col_s;   /* local->local keyed by source  [N+B] [E_ll] */
  float* ll_dinv;                    /* in-degree^-1/2                [N]          */
  int32_t *lv_rowptr, *lv_col;       /* local->virtual keyed by target (cluster)  [V+B] [E_lv] */
  int32_t *vv_rowptr, *vv_col;       /* virtual->virtual keyed by target          [V+B] [E_vv] */
  float* vv_dinv;                    /* [V] */
} hscn_structure;
int hscn_resident_structure(const int64_t* ei_ll, int64_t E_ll, const int64_t* ei_vv, int64_t E_vv,
                            const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr, const int32_t* vptr,
                            const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv, int64_t B,
                            int max_n, int max_v, int max_ell, int max_evv, const hscn_structure* out,
                            int32_t* flag, void* stream);
/* gather of the structure slices of graphs ids[0..B) of a dataset (ds_structure built over the dataset as one batch
 * of ds->G graphs) into batch-level arrays with the capacities of `out_batch`; same ids / cursor convention as
 * hscn_collate_gather, which must be called AFTER it when a cursor is used (that call advances the cursor). */
int hscn_collate_gather_structure(const hscn_hetero_dataset* dataset, const hscn_structure* ds_structure,
                                  const int64_t* ids, int64_t B, const hscn_hetero_batch_out* out_batch,
                                  const hscn_structure* out_structure, int32_t* flag, const int32_t* cursor,
                                  const int32_t* cursor_base, void* stream);

/* ------------------------------------------------------------------------- *
 * a10 + f3  the whole training iteration of stage C in ONE launch (+ the ordered parameter reduction):
 * reference train/train.py:73-95 -- pred = model(x_dict, edge_index_dict, batch) (model/hscn.py:102-114);
 * loss, score = criterion(loss_fn, pred, true) (loss.py:6-19); loss.backward().  Workgroup g runs forward, its row
 * of d(mean loss)/d pred and backward of graph g with structure and every activation resident in LDS; nothing is
 * exported between "forward" and "backward" (csrc/resident_step.h).  Prediction, score, loss and virtual features
 * are bit-identical to hscn_resident_fwd_with_virtual + hscn_resident_bwd_with_virtual(tail); the parameter
 * gradients agree with theirs to float rounding (H = 16 groups the weight gradient's partial sums by row tile);
 * every output is bitwise reproducible from run to run.
 *   target [B,C], loss_kind 0 = BCE-with-logits / 1 = L1 (mean over B*C); pred, score [B,C] outputs;
 *   partials [B,P+1], grads [P+1], P = hscn_resident_param_count: grads[0..P) = parameter gradients in the order
 *   {W_ll, b_ll} per layer, W1, b1, W2, b2; grads[P] = the mean loss.
 *   job (or NULL = no virtual branch): the virtual branch runs as B more workgroups of the same launch; it needs
 *   job->xv_out (final virtual features [V,H]), acts [max(L-1,1),N,H] (the local activations handed over inside
 *   the launch) and sync: 32 + B uint32 words, ZERO when first used and never touched by the caller afterwards
 *   ([0] = step epoch, advanced by the reduction; [32+g] = graph g's publish counter).  The job's st_* are unused.
 *   H in {16, 32}; hscn_resident_train_step_supported says whether the graphs fit (H = 16: n <= ~450).
 *   flag bit 8: a virtual workgroup gave up waiting for its local activations (virtual features invalid;
 *   prediction, loss and gradients unaffected).
 * ------------------------------------------------------------------------- */
int hscn_resident_train_step_supported(int F, int H, int L, int C, int max_n, int max_ell, int max_v, int max_evv);
/* workgroups of that launch one CU holds at a time (0 = unsupported): the virtual branch rides as B more workgroups
 * while 2B <= number of CUs x this figure (1 for 16-wave workgroups; up to 4 for the 4-wave workgroups of small graphs).
 * Beyond that the launch is still CORRECT at any B -- block ids [0, B) are the local programs, so every producer is
 * dispatched before its consumer and no local program waits on anybody -- and, for 16-wave workgroups at H = 16, faster
 * than the launch pair (the caller's choice: graph_hscn/step.py takes it there). */
int hscn_resident_train_step_wgs_per_cu(int F, int H, int L, int C, int max_n, int max_ell, int max_v, int max_evv);
int hscn_resident_train_step(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                             const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C, int head_act,
                             const void* const* layer_params_host /* L x 9 */, const float* W1, const float* b1,
                             const float* W2, const float* b2, int max_n, int max_ell, const float* target,
                             int loss_kind, float* pred, float* score /*or NULL*/, float* partials /*[B,P+1]*/,
                             float* grads /*[P+1]*/, void* acts /*or NULL*/, uint32_t* sync /*or NULL*/,
                             int32_t* flag, const hscn_virtual_job* job /*or NULL*/,
                             const hscn_structure* structure /*or NULL: build per step*/,
                             int flags /*HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Half storage (HSCN_STORE_F16; BASELINE.json configs[4], "fp16 feat + bf16 accum", PCQM-Contact): the launches
 * above and the stage-A launches below with IEEE-half STORAGE of node features and inter-layer activations.  The
 * reference has no reduced-precision mode (no autocast / half anywhere); the flag serves the same call
 * sites (model/hscn.py:102-114, train/train.py:76-87, train/train_clustering.py:37-50) for a caller that keeps `x`
 * in half.  The arrays whose element type the flag selects are declared `void*`:
 *   hscn_resident_*: x_local, x_virtual, acts, xv_out, and in `job`: x_virtual, xv_out, st_xv (declared float*
 *     there; they point to hscn_half arrays under the flag);
 *   hscn_scn_resident_*: x [N,F] and the saved hidden activation y [N,H].
 *   float either way: parameters, pooled, z, pred, score, degree norms, S, stats, ss, losses, the exported
 *   aggregation ex_agg, partials, grads.  Every sum accumulates in float registers (a superset of bf16
 *   accumulation); an activation is rounded to half once, where it is produced.
 *   H in {16, 32} (HSCN_E_UNSUPPORTED otherwise); everything else as documented without the flag.
 * ------------------------------------------------------------------------- */
typedef uint16_t hscn_half; /* the 16 bits of an IEEE binary16 */

/* ------------------------------------------------------------------------- *
 * Gradient accumulation over micro-batches (HSCN_GRAD_ACCUMULATE; reference train/train.py:89-95:
 * `batch_accumulation`, the optimizer steps every k-th batch on the SUM of their gradients).  hscn_resident_bwd,
 * hscn_resident_bwd_with_virtual, hscn_resident_train_step and hscn_mpnn_train_step issue the same launches under
 * the flag, except that the final fold ADDS each parameter column to `grads`:
 *   grads[p] = grads[p] + sum_g partials[g][p]   (p < P: the sum formed exactly as without the flag, added
 *                                                  last -- autograd's `p.grad += new`, rounding for rounding)
 * The loss column grads[P] (with a loss tail) is still overwritten: it is the loss of THIS micro-batch.  The caller
 * zeroes `grads` where the reference calls optimizer.zero_grad() (hscn_adam_step_ex can do it in its launch).
 * ------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------- *
 * a2/a4/a6  stage A, graph-resident engine: the body of the reference's clustering loop
 * (train/train_clustering.py:37-47) for a batch of RAW graphs in one launch --
 * gcn_norm(add_self_loops=True) folded into the CSR walk, SCN.forward for
 * mp_units=[H], mlp_units=[] (GraphConv + act, Linear -> K logits, softmax), MinCUT and
 * orthogonality losses on the binary A + I (model/hscn.py:56-64), one workgroup per graph.
 *   edge_index: int64 [2,E] raw COO (self loops, if any, are replaced by the unit loop);
 *   graph g owns nodes [nptr[g],nptr[g+1]) and edges [eptr[g],eptr[g+1]);
 *   outputs S [N,K] (= softmax, the reference's first return), y [N,H] (post-activation
 *   GraphConv output, kept for the backward), stats [B,4] {num, den, |S^T S|_F, ortho},
 *   ss [B,K,K], losses [3] = {mean mincut, mean ortho, their sum (what the training loop minimises,
 *   train/train_clustering.py:48)}.  ticket: a device int32 that is zero before the first launch; with
 *   it the workgroup that finishes last reduces the per-graph statistics inside the launch (and leaves
 *   the counter at zero), without it a one-wave launch does.  Same summation order either way.
 * hscn_scn_resident_bwd: grads packed as {W_rel [H,F], b_rel [H], W_root [H,F], W_mlp [K,H],
 * b_mlp [K]} given the upstream scalars g_mc = dL/dmincut, g_o = dL/dortho as two device pointers
 * (the two losses are separate autograd outputs; NULL = that loss received no gradient).
 *   ex_*: both CSRs of the self-loop-free graph (target-keyed d, source-keyed s; graph g: rowptr at
 *   nptr[g] + g, columns at eptr[g]), the normalised aggregation agg = A_hat x (16 columns, zero
 *   padded) and the binary out-degree + 1: built in LDS by the forward launch, exported (all six or
 *   none) and loaded by the backward launch, which does not rebuild them.
 * ------------------------------------------------------------------------- */
int hscn_scn_resident_supported(int F, int H, int K, int max_n, int max_e);
int64_t hscn_scn_resident_param_count(int F, int H, int K);
int hscn_scn_resident_fwd(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                          const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                          const float* W_rel, const float* b_rel, const float* W_root, const float* W_mlp,
                          const float* b_mlp, int max_n, int max_e, float* S, void* y, float* stats, float* ss,
                          float* losses /*[3]*/, int32_t* ticket /*[1] or NULL*/, int32_t* ex_rowptr_d /*[N+B]*/,
                          int32_t* ex_col_d /*[E]*/,
                          int32_t* ex_rowptr_s /*[N+B]*/, int32_t* ex_col_s /*[E]*/, float* ex_agg /*[N,16]*/,
                          float* ex_dout /*[N]*/, int32_t* flag, int flags /*HSCN_STORE_F16*/, void* stream);
int hscn_scn_resident_bwd(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                          const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                          const float* W_mlp, const float* S, const void* y, const float* stats, const float* ss,
                          const float* g_mc /*[1] or NULL*/, const float* g_o /*[1] or NULL*/,
                          const int32_t* ex_rowptr_d, const int32_t* ex_col_d, const int32_t* ex_rowptr_s,
                          const int32_t* ex_col_s, const float* ex_agg, const float* ex_dout, int max_n, int max_e,
                          float* partials /*[B,P]*/, float* grads /*[P]*/, int32_t* flag,
                          int flags /*HSCN_STORE_F16*/, void* stream);

/* State and hyper-parameters of torch's Adam / AdamW for the one-launch optimizer step (hscn_adam_step, below) and for
 * the stage-A step that applies it in its own tail: exp_avg / exp_avg_sq [P] (flat parameter order, zero before the
 * first step), step: device float counter, beta_pows: device double [2] = {1, 1} before the first step (beta1^t,
 * beta2^t as running products), lr: device double; decoupled != 0: AdamW. */
typedef struct hscn_adam {
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  double* beta_pows;
  const double* lr;
  double beta1, beta2, eps, weight_decay;
  int decoupled;
} hscn_adam;

/* What a stage-A step derives from a batch's graphs and INPUT features alone -- both CSRs of the self-loop-free graph
 * (graph g: row pointers at nptr[g] + g, columns at eptr[g]), the gcn_norm aggregation A_hat x [N,16] and the binary
 * out-degree + 1 [N] (the ex_* arrays of hscn_scn_resident_fwd) -- kept across the cluster_epochs visits of the same
 * batch (train/train_clustering.py:34: neither the graphs nor x change between epochs).  ready == 0: the launch builds
 * the structure and stores it here; ready != 0: it loads it instead (no COO read, no CSR build, no aggregation).
 * Bit-identical results either way. */
typedef struct hscn_scn_structure {
  int32_t* rowptr_d; /* [N + B] */
  int32_t* col_d;    /* [E] */
  int32_t* rowptr_s; /* [N + B] */
  int32_t* col_s;    /* [E] */
  float* agg;        /* [N, 16] */
  float* dout;       /* [N] */
  float* xpad;       /* [N, 16] or NULL: the input features zero-padded to 16 columns (16-byte loads on later visits) */
  int ready;
} hscn_scn_structure;

/* The stage-A step in ONE launch: optimizer.zero_grad(); S, mc, o = model(x, ei, adj); (mc + o).backward() of
 * train/train_clustering.py:37-49 for a batch of raw graphs -- hscn_scn_resident_fwd and hscn_scn_resident_bwd with
 * everything the first exported for the second (CSRs, agg, y, S, S^T S, statistics) staying in the workgroup's LDS.
 * Bit-identical to the pair of launches.  S [N,K] may be NULL (a training step does not need the assignments);
 * stats [B,4], losses [3], ticket as in hscn_scn_resident_fwd; g_mc / g_o as in hscn_scn_resident_bwd.  With
 * B == 1 (the reference's trajectory, one graph per optimizer step) the workgroup writes grads [P] itself and
 * partials may be NULL; with B > 1 the ordered fold of partials [B,P] is the launch behind it.
 * opt != NULL (B == 1 only): optimizer.step() of train/train_clustering.py:50 in the tail of the same launch -- the
 * workgroup holds the whole gradient; W_rel .. b_mlp are then UPDATED IN PLACE (same operations as hscn_adam_step).
 * cache != NULL: see hscn_scn_structure.
 * hscn_scn_resident_train_step_supported: the pair's conditions, K % 4 == 0, K <= 32 (H = 16) and max_n <= 512. */
int hscn_scn_resident_train_step_supported(int F, int H, int K, int max_n, int max_e);
int hscn_scn_resident_train_step(const void* x, const int64_t* edge_index, int64_t E, const int32_t* nptr,
                                 const int32_t* eptr, int64_t N, int64_t B, int F, int H, int K, int act,
                                 const float* W_rel, const float* b_rel, const float* W_root, const float* W_mlp,
                                 const float* b_mlp, const float* g_mc /*[1] or NULL*/, const float* g_o /*[1] or NULL*/,
                                 int max_n, int max_e, float* S /*[N,K] or NULL*/, float* stats /*[B,4]*/,
                                 float* losses /*[3]*/, int32_t* ticket /*[1] or NULL*/, float* partials /*[B,P]*/,
                                 float* grads /*[P]*/, int32_t* flag, const hscn_adam* opt /*or NULL*/,
                                 const hscn_scn_structure* cache /*or NULL*/, int flags /*HSCN_STORE_F16*/,
                                 void* stream);
/* A whole run of the reference's stage-A loop (train/train_clustering.py:34-50: one optimizer step per graph, graph
 * after graph, epoch after epoch) from ONE call: `visits` graph visits in dataset order (visit v takes graph v mod G
 * of a dataset laid out as one block-diagonal batch: nptr / eptr [G+1]), each the launch of
 * hscn_scn_resident_train_step(B = 1, opt, cache) on that graph -- walked by ONE persistent workgroup with the weights
 * in LDS and the Adam moments in registers when the model has at most 1024 parameters (slices of 32 768 visits per
 * launch), else issued launch by launch by the library; no host language between two visits either way.
 * cache: REQUIRED and ready -- the structure of ALL G graphs in the batch layout (one
 * hscn_scn_resident_fwd launch over the dataset with its ex_* outputs builds it); opt: REQUIRED; W_rel .. b_mlp and
 * opt's state are updated in place by every visit; g_mc / g_o: the upstream gradients of the two losses (device
 * scalars; the loop's loss mincut + ortho has both = 1); grads [P], stats [4], losses [3]: the last visit's; ticket:
 * a zeroed device int32.  hscn_scn_resident_train_step_supported says whether the shapes qualify. */
int hscn_scn_resident_train_epoch(const void* x, const int32_t* nptr, const int32_t* eptr, int64_t N, int64_t G,
                                  int64_t visits, int F, int H, int K, int act, float* W_rel, float* b_rel,
                                  float* W_root, float* W_mlp, float* b_mlp, const float* g_mc /*[1]*/,
                                  const float* g_o /*[1]*/, int max_n, int max_e,
                                  const hscn_scn_structure* cache, const hscn_adam* opt, float* grads /*[P]*/,
                                  float* stats /*[4]*/, float* losses /*[3]*/, int32_t* ticket, int32_t* flag,
                                  int flags /*HSCN_STORE_F16*/, void* stream);

/* ---------------------------------------------------------------------------
 * The optimizer step behind a resident training step as ONE launch: torch.optim.Adam / AdamW (the optimizers
 * train/train.py:82 and train/train_clustering.py:30-33 build from config.py's OPTIM_DICT), single-tensor formulas
 * operation for operation (torch/optim/adam.py::_single_tensor_adam), on parameters whose gradients lie in one flat
 * buffer (what the resident steps produce).  params_host: HOST array of the nseg device pointers of the parameter
 * tensors in flat order, seg_off_host: HOST int32 [nseg + 1] element offsets (0 .. P; both travel in the kernel
 * arguments); exp_avg / exp_avg_sq [P] zero before the first step;
 * step_dev: device float counter (incremented here); beta_pows_dev: device double [2] = {1, 1} before the first step
 * (beta1^t, beta2^t, kept as running products); lr_dev: device double (a scheduler may rewrite it);
 * decoupled != 0: AdamW's p *= 1 - lr * weight_decay instead of Adam's g += weight_decay * p.
 * nseg <= 64; one workgroup (the model family has a few thousand parameters in ~10 tensors).
 * ------------------------------------------------------------------------- */
int hscn_adam_step(float* const* params_host, const int32_t* seg_off_host, int nseg, const float* grads,
                   float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev, double* beta_pows_dev,
                   const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, int decoupled, void* stream);

/* ABI 19: hscn_adam_step with, in the same launch, the two optimizer-side settings of the reference's loop
 * (train/train.py:89-95):
 *   max_norm > 0: torch.nn.utils.clip_grad_norm_(params, max_norm) over the flat gradient first -- the 2-norm as a
 *     sum of g^2 in double in a fixed order (bitwise reproducible), then torch's formulas from the norm on:
 *     norm = (float)sqrt(sum), coef = min(reciprocal(norm + 1e-6f) * max_norm, 1), g = g * coef for every element
 *     (coef == 1 included; a non-finite norm propagates as in torch).  The clipped gradient is written back to
 *     `grads` (what p.grad holds after torch's clip) and, if norm_out != NULL, the pre-clip norm to norm_out[0]
 *     (clip_grad_norm_'s return value).  max_norm == 0: no clip.
 *   zero_grads != 0: grads[0 .. P) = 0 after the update (optimizer.zero_grad(): the next micro-batch accumulates
 *     onto zeros).
 * hscn_clip_grad_norm_flat: the same norm and in-place scaling as a launch of its own (one workgroup), for
 * optimizers that are not hscn_adam_step; max_norm > 0. */
int hscn_adam_step_ex(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                      float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev, double* beta_pows_dev,
                      const double* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                      int decoupled, float max_norm, float* norm_out /*[1] or NULL*/, int zero_grads, void* stream);
int hscn_clip_grad_norm_flat(float* grads, int64_t P, float max_norm, float* norm_out /*[1] or NULL*/, void* stream);

/* A learning-rate schedule evaluated INSIDE the optimizer launch (additive to ABI 23): the record travels by value in
 * the kernel arguments, the launch reads the device step counter it is about to increment (s = optimizer steps
 * completed so far) and uses lr(s) = base_lr * f(s), f in double as Python would form it:
 *   HSCN_LR_CONSTANT       no record: the launch reads the device lr word (the entry points treat it like NULL).
 *   HSCN_LR_WARMUP_COSINE  s < warmup_steps: f = max(1e-6, s / max(1, warmup_steps)); else, with s clamped to
 *                          total_steps: f = max(min_factor, 0.5 * (1 + cos(pi * (s - warmup_steps) / max(1, total_steps -
 *                          warmup_steps)))).
 *   HSCN_LR_WARMUP_LINEAR  the same warm-up, then f = max(min_factor, (total_steps - s) / max(1, total_steps -
 *                          warmup_steps)), s clamped likewise.
 *   HSCN_LR_STEP           f = gamma ^ floor(s / period), kept as a running product in sched_state_dev[0] (a device
 *                          double, 1 before the first step; the launch multiplies it when s + 1 reaches a period).
 * The launch writes the rate it used into the device lr word (behind its closing barrier, beside the counter), so the
 * word always holds the last step's rate.  HSCN_E_BADARG: an unknown kind, base_lr or warmup_steps negative,
 * total_steps < warmup_steps, period < 1, gamma outside (0, 1], min_factor negative or NaN. */
#define HSCN_LR_CONSTANT 0
#define HSCN_LR_WARMUP_COSINE 1
#define HSCN_LR_WARMUP_LINEAR 2
#define HSCN_LR_STEP 3
typedef struct hscn_lr_schedule {
  int kind;
  double base_lr;
  int64_t warmup_steps, total_steps, period;
  double gamma, min_factor;
} hscn_lr_schedule;

/* hscn_adam_step_ex with a schedule: sched (HOST pointer; NULL or kind HSCN_LR_CONSTANT: exactly hscn_adam_step_ex),
 * sched_state_dev: device double [1] (required with a schedule), lr_dev: written. */
int hscn_adam_step_sched(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                         float* exp_avg, float* exp_avg_sq, int64_t P, float* step_dev, double* beta_pows_dev,
                         double* lr_dev, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                         float max_norm, float* norm_out /*[1] or NULL*/, int zero_grads,
                         const hscn_lr_schedule* sched /*or NULL*/, double* sched_state_dev /*[1]*/, void* stream);

/* torch.optim.Adagrad (the third member of config.py's OPTIM_DICT) as ONE launch on the same flat layout, with the
 * same optional clip in front (max_norm > 0) and zeroing behind (zero_grads != 0) and the same optional schedule:
 * torch/optim/adagrad.py::_single_tensor_adagrad, operation for operation --
 *   t = step + 1;  [weight_decay] g = g + wd * p;  clr = lr / (1 + (t - 1) * lr_decay)  (double, rounded to float once)
 *   sum = sum + g * g;  std = sqrtf(sum) + eps;  p = p + (-clr) * (g / std)
 * state_sum [P]: filled with initial_accumulator_value before the first step; step_dev: device float counter
 * (incremented here); lr_dev: device double (written only with a schedule). */
int hscn_adagrad_step(float* const* params_host, const int32_t* seg_off_host, int nseg, float* grads,
                      float* state_sum, int64_t P, float* step_dev, double* lr_dev, double lr_decay, double eps,
                      double weight_decay, float max_norm, float* norm_out /*[1] or NULL*/, int zero_grads,
                      const hscn_lr_schedule* sched /*or NULL*/, double* sched_state_dev /*[1] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------
 * Normalisation layers of the MPNN baseline: torch.nn.LayerNorm(H) / torch.nn.BatchNorm1d(H) on [N, H] activations,
 * reference graph_hscn/model/mpnn.py:34-44 (construction) and :53-56 (use after every hidden convolution).
 * LayerNorm: per row, biased variance, eps inside the root; mean / rstd [N] are saved for the backward.
 * BatchNorm1d, training != 0: batch statistics per column (two passes), running_mean / running_var (either may be
 *   NULL) updated with `momentum` (unbiased variance), save_mean / save_rstd [H] for the backward; training == 0:
 *   running statistics (save_* receive them).  Parameter gradients and column statistics are ordered sums over row
 *   chunks (workspace: hscn_norm_workspace_bytes(N, H)); no float atomics.
 * ------------------------------------------------------------------------- */
size_t hscn_norm_workspace_bytes(int64_t N, int H);
int hscn_layer_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                        int64_t N, int H, float eps, void* stream);
int hscn_layer_norm_bwd(const float* gy, const float* x, const float* gamma, const float* mean, const float* rstd,
                        float* gx, float* g_gamma, float* g_beta, int64_t N, int H, void* workspace,
                        size_t workspace_bytes, void* stream);
int hscn_batch_norm_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float* y, float* save_mean, float* save_rstd, int64_t N, int H, float eps, float momentum,
                        int training, void* workspace, size_t workspace_bytes, void* stream);
int hscn_batch_norm_bwd(const float* gy, const float* x, const float* gamma, const float* save_mean,
                        const float* save_rstd, float* gx, float* g_gamma, float* g_beta, int64_t N, int H,
                        int training, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Data-parallel exchange: one-shot peer-to-peer all-reduce of the flat gradient buffer.
 * The reference is single process; the exchange slots in between loss.backward() and
 * optimizer.step() of the training iteration, reference graph_hscn/train/train.py:87-94.
 * At 4.6 KB - 640 KB the collective is pure latency and the 8 GPUs of a node are one xGMI hop apart, so instead of
 * a ring (2(G-1) dependent hops) every rank stores its buffer into slot `rank` of every rank's slot buffer, raises
 * a per-source epoch flag there (system-scope release), waits for its own G flags (bounded spin), and adds its G
 * slots in RANK ORDER: flat = scale * (slot_0 + slot_1 + ... + slot_{G-1}), separately rounded adds, the same order
 * on every rank, so replicas stay bit-identical.  One launch; capturable (the epoch is device state advanced by the
 * kernel).  Slots are double-buffered by epoch parity (csrc/allreduce.hip explains why two suffice).  Buffers of up
 * to 16 384 floats travel as 8-byte {value, epoch} granules (64-bit relaxed system-scope atomics: no flag, no fence,
 * one fabric round trip); larger ones as 16-byte slabs with per-chunk flags and one release / acquire per workgroup.
 *
 * Set-up (host-synchronous, once per job; the only entry points that allocate):
 *   hscn_comm_alloc      zero-filled device memory that peers may write while a kernel polls it.
 *                        kind 0 = fine-grained (hipDeviceMallocFinegrained: what the memory model requires for
 *                        system-scope synchronisation inside a kernel), 1 = uncached, 2 = plain hipMalloc.
 *   hscn_comm_ipc_export / _open / _close   hipIpcGetMemHandle / hipIpcOpenMemHandle / hipIpcCloseMemHandle on a
 *                        64-byte handle (dmabuf IPC: HSA_ENABLE_IPC_MODE_LEGACY=0).
 * Every rank allocates slot_bytes + flag_bytes, exports both, opens its peers', and passes the G mapped addresses
 * (its own allocation at index `rank`) as HOST arrays; they travel in the kernel arguments.
 *   epoch  [hscn_allreduce_oneshot_chunks(count)] uint32 local device words, zero before the first call;
 *   status [2] uint32 local device words, zero: [0] bit 0 = a wait timed out (that chunk of `flat` is then left
 *          unreduced), [1] = bit mask of the sources whose flag never arrived;
 *   spin_limit: polls (each followed by a short sleep) before a wait gives up; 0 = default (~1 s).
 * count <= 2 Mi floats (every workgroup of a launch must be resident at once).
 * ------------------------------------------------------------------------- */
int hscn_comm_alloc(size_t bytes, int kind, void** out_ptr_host);
int hscn_comm_free(void* ptr);
int hscn_comm_ipc_export(void* ptr, void* handle64_host);
int hscn_comm_ipc_open(const void* handle64_host, void** out_ptr_host);
int hscn_comm_ipc_close(void* ptr);
size_t hscn_allreduce_oneshot_slot_bytes(int64_t count, int G);
size_t hscn_allreduce_oneshot_flag_bytes(int64_t count, int G);
int64_t hscn_allreduce_oneshot_chunks(int64_t count);
int hscn_allreduce_oneshot(float* flat, int64_t count, void* const* peer_slots_host /*[G]*/,
                           void* const* peer_flags_host /*[G]*/, uint32_t* epoch, uint32_t* status, int rank, int G,
                           float scale, uint32_t spin_limit, void* stream);

/* ------------------------------------------------------------------------- *
 * ABI 20: the MPNN baseline (reference model/mpnn.py:13-62 with conv = GCNConv, configs/GCN/peptides_func_GCN.yaml)
 * as ONE training-step launch: workgroup g runs the forward of graph g, its loss row and the backward with the
 * structure and every activation in LDS, then the fold (k_param_reduce) sums the per-graph partials.
 *   hidden layer l < L-1: a = dropout(act(relu(A_hat a W_l^T + b_l))); last layer: pred = mean_i (A_hat a W^T + b)_i;
 *   A_hat: GCN normalisation WITH self loops (the edge list's own loops are replaced, not doubled; isolated nodes
 *   keep their own row).  act: HSCN_ACT_* (relu, elu, identity, tanh).
 *   x [N,F] f32, edge_index int64 [2,E] batch numbering, graph g owns nodes [ptr32[g], ptr32[g+1]) and edges
 *   [eptr32[g], eptr32[g+1]); params_host: HOST array of L x 2 device pointers {W_l [fout,fin], b_l [fout]}
 *   (fin = F for l = 0 else H, fout = C for l = L-1 else H), the parameter order of graph_hscn.model.mpnn.MPNN.
 *   target [B,C], loss_kind 0 = BCE with logits (multilabel), 1 = L1; inv_count = 1 / (B C).
 *   pred, score (sigmoid, optional) [B,C]; partials [B, P+1]; grads [P+1]: dL/d params packed in parameter order,
 *   grads[P] = the mean loss (P = hscn_mpnn_param_count).
 *   Dropout p in [0, 1): the mask of hidden layer l is bitwise that of hscn_dropout over the batch's [N, H]
 *   activation with seed seed0 + (L-1) t + l, t = step[0] (device word, read at launch, advanced by one by the fold:
 *   a captured step draws new masks on every replay).  step may be NULL when p = 0 (t = 0; nothing advanced).
 *   flag bit 1: an edge with an end outside its graph (dropped); bit 2: a graph beyond max_n / max_ell or the
 *   arrays (its partials row is zeros).
 *   flags: HSCN_GRAD_ACCUMULATE = the same launches, the fold ADDS every parameter column to grads (as for the
 *   hscn_resident_* entry points; grads[P] is still the loss of this call).
 * hscn_mpnn_forward: the forward alone (no dropout: evaluation / inference): pred, score (optional), and with a
 *   target the per-graph loss-term sums loss_rows [B] and, if loss != NULL, the mean loss loss[0].
 * hscn_mpnn_supported: H in {16, 32}, 1 <= F <= H, C <= min(H, 16), 2 <= L <= 8, and a layout of the largest graph
 *   within 160 KB of LDS (H = 16: Peptides' 444 nodes).  Normalisation layers, other convolutions and class-index
 *   targets are not this launch's (the Python layer reports them).
 * ------------------------------------------------------------------------- */
int hscn_mpnn_supported(int F, int H, int L, int C, int max_n, int max_ell);
int64_t hscn_mpnn_param_count(int F, int H, int L, int C);
int hscn_mpnn_train_step(const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                         const int32_t* eptr32, int64_t N, int64_t B, int F, int H, int L, int C, int act,
                         const void* const* params_host /* L x 2 */, int max_n, int max_ell, const float* target,
                         int loss_kind, float inv_count, float* pred, float* score /*or NULL*/,
                         float* partials /*[B,P+1]*/, float* grads /*[P+1]*/, uint32_t* step /*or NULL if p = 0*/,
                         float p, uint64_t seed0, int32_t* flag, int flags /*HSCN_GRAD_ACCUMULATE*/, void* stream);
int hscn_mpnn_forward(const float* x, const int64_t* edge_index, int64_t E, const int32_t* ptr32,
                      const int32_t* eptr32, int64_t N, int64_t B, int F, int H, int L, int C, int act,
                      const void* const* params_host, int max_n, int max_ell, const float* target /*or NULL*/,
                      int loss_kind, float inv_count, float* pred, float* score /*or NULL*/,
                      float* loss_rows /*[B] or NULL*/, float* loss /*[1] or NULL*/, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------- *
 * ABI 22: the SignNet node encoder's forward (graph_hscn/encoder/signnet.py: SignNetNodeEncoder; reference
 * encoder/signnet.py:296-381, run once per batch under no_grad by compute_posenc) as ONE launch: workgroup g encodes
 * graph g with its structure in LDS (csrc/signnet.hip).
 *   eigvecs [N,K] f32 (NaN padding is read as 0), K independent channels of width 1;
 *   phi = GIN(1, hidden, phi_out, layers): Lc = max(layers, 2) GINConv's, nn(x_i + sum_{j -> i} x_j) over the edge
 *   list as given (repeated edges and loops count, nothing is added), nn = Linear(1, hidden), Lc - 2 times
 *   Linear(hidden, hidden), then Linear(hidden, hidden) -> ReLU -> Linear(hidden, phi_out);
 *   DeepSet: enc = sum over the frequencies k < min(K, n_graph) of phi(v_k) + phi(-v_k);
 *   rho: post_layers Linear's with ReLU between them (phi_out -> hidden -> .. -> dim_pe; one layer: phi_out -> dim_pe);
 *   out [N, dim_x + dim_pe] = [ x Wx^T + bx | pe ]  (expand_x = 0: the leading columns are x itself, dim_x = F);
 *   pe [N, dim_pe]: optional second copy of the encoding (pass_as_var).
 *   x [N,F] f32, edge_index int64 [2,E] batch numbering, graph g owns nodes [ptr32[g], ptr32[g+1]) and edges
 *   [eptr32[g], eptr32[g+1]).  params_host: HOST array of device pointers {W, b} per Linear in module order: the Lc
 *   Linear's in front of the ReLU, the one behind it, rho's post_layers, then (expand_x) linear_x.
 *   flag bit 1: an edge with an end outside its graph (dropped); bit 2: a graph beyond max_n / max_e or the arrays
 *   (the rows it names inside [0, N) are zeros).
 * hscn_signnet_supported: model = HSCN_SIGNNET_DEEPSET (HSCN_SIGNNET_MLP, the concatenation over k, is refused),
 *   use_bn = 0 (BatchNorm in training mode takes statistics across the whole batch), 1 <= F, dim_x <= 1024,
 *   1 <= K <= 64, hidden, phi_out, dim_pe in [1, 64], layers and post_layers in [1, 8], and a layout of the largest
 *   graph within 160 KB of LDS.  hscn_signnet_encode: HSCN_E_BADARG for null pointers / non-positive widths,
 *   HSCN_E_UNSUPPORTED outside the envelope, both before any launch; B = 0 or N = 0 launches nothing.
 * ------------------------------------------------------------------------- */
#define HSCN_SIGNNET_DEEPSET 0
#define HSCN_SIGNNET_MLP 1
int hscn_signnet_supported(int model, int use_bn, int F, int K, int hidden, int phi_out, int layers, int post_layers,
                           int dim_pe, int dim_x, int max_n, int max_e);
int hscn_signnet_encode(const float* x, const float* eigvecs, const int64_t* edge_index, int64_t E,
                        const int32_t* ptr32, const int32_t* eptr32, int64_t N, int64_t B, int F, int K, int hidden,
                        int phi_out, int layers, int post_layers, int dim_pe, int dim_x, int expand_x,
                        const void* const* params_host, int max_n, int max_e, float* out, float* pe /*or NULL*/,
                        int32_t* flag, void* stream);

/* ------------------------------------------------------------------------- *
 * Epoch metrics of the training / evaluation loop (reference graph_hscn/metrics.py:6-36, called on the whole
 * epoch's [G, C] labels and scores at train/train.py:109-144) where the tensors live (csrc/metrics.hip).  Purely
 * additive to ABI 23.
 *
 * hscn_average_precision: metrics.py:6-27 eval_ap = the mean over the valid classes of sklearn's
 *   average_precision_score.  y_true, y_score [G, C] f32 row-major.  Per class c: rows whose label is NaN are
 *   ignored; the class is VALID iff the remaining labels hold at least one 1 and at least one 0 (a label counts as
 *   positive iff it equals 1).  A valid class's rows are ordered by score, descending; scores that compare equal
 *   form one threshold run (-0.0 ties +0.0); AP = the float64 sum over runs of (recall_run - recall_prev) *
 *   precision_run with precision = tp / n and recall = tp / P at the last row of the run.
 *     ap [C] f64 (0 where the class is not valid), valid [C] i32,
 *     result [2] f64 = { mean of ap over the valid classes, summed in class order; number of valid classes },
 *     flags [1] i32: bit 0 = no valid class (result[0] is then 0), bit 1 = a NaN score in a labelled row of a valid
 *     class (an invalid class takes no part in the metric, its scores are not examined).
 *   One workgroup per class: 64-bit keys (inverted order-preserving image of the score << 1 | label bit), a
 *   bitonic sort and a scan of the label bits in LDS for G <= 16384 (8 B per row, 128 KB of the CU's 160 KB), in
 *   `workspace` (global memory, slower) beyond; then a one-wave launch folds the classes.  No atomics: the same
 *   input gives the same bits.  hscn_average_precision_workspace_bytes(G, C): 256 bytes for G <= 16384.
 *   HSCN_E_BADARG for null pointers, G < 1, C < 1 or G > 2^30; HSCN_E_WORKSPACE for a workspace too small; both
 *   before any launch.
 *
 * hscn_mean_absolute_error: metrics.py:30-36 eval_mae = the float64 mean of |y_true - y_pred| over [G, C] (one
 *   workgroup, per-thread strided sums folded by a fixed tree).  result [2] f64 = { mean, G * C },
 *   flags [1] i32: bit 1 = a NaN prediction.
 *
 * hscn_multiclass_metrics: accuracy and macro-F1 of class-index targets (the metrics of the criterion's multiclass
 *   branch; scikit-learn's accuracy_score and f1_score(average="macro")).  target [G] i64, score [G, C] f32
 *   row-major (any score that ranks the classes: logits, log-probabilities), 1 <= C <= 128 (the confusion matrix
 *   fits 64 KB of LDS), G <= 2^30.  The predicted class of a row is its FIRST maximal column (numpy's argmax).
 *     confusion [C, C] i32, rows = true class, columns = predicted class (zeroed by the call; integer adds, in LDS
 *       per workgroup, then into this matrix: deterministic),
 *     per_class [C] f64 = F1 of each class = 2 tp / (rows with that target + rows with that prediction), 0 where tp
 *       is 0,
 *     result [2] f64 = { accuracy = trace / G; macro-F1 = the mean of per_class over the classes that occur among
 *       the targets or the predictions, added in class order },
 *     flags [1] i32 (written by the call): bit 1 = a NaN score; bit 2 = a target outside [0, C) (the row is left
 *       out of the matrix, G still divides).
 *   Three launches on the stream (zero, count, finish).  HSCN_E_BADARG for null pointers, G < 1, G > 2^30 or C
 *   outside [1, 128], before any launch.
 * ------------------------------------------------------------------------- */
size_t hscn_average_precision_workspace_bytes(int64_t G, int C);
int hscn_average_precision(const float* y_true, const float* y_score, int64_t G, int C, double* ap, int32_t* valid,
                           double* result, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream);
int hscn_mean_absolute_error(const float* y_true, const float* y_pred, int64_t G, int C, double* result,
                             int32_t* flags, void* stream);
int hscn_multiclass_metrics(const int64_t* target, const float* score, int64_t G, int C, int32_t* confusion /*[C,C]*/,
                            double* result /*[2]*/, double* per_class /*[C]*/, int32_t* flags /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Laplacian statistics of the SignNet positional encoding (reference transform/posenc.py:14-107:
 * compute_posenc_stats, get_lap_decomp_stats, eigvec_normalizer) for a collated batch as ONE launch, one workgroup
 * per graph (csrc/lap_eig.hip).  Purely additive to ABI 23.
 *
 * hscn_lap_eig_stats: edge_index int64 [2, E] in batch numbering; graph g owns nodes [nptr[g], nptr[g+1]) and edges
 *   [eptr[g], eptr[g+1]) (int32, B + 1 entries each); max_n >= the largest graph's node count.
 *   Laplacian: self loops dropped; is_undirected != 0: every listed edge adds 1 to A[row, col] (duplicates sum),
 *   is_undirected = 0: A[r, c] = A[c, r] = 1 for every listed pair; degree = row sum; lap_norm HSCN_LAP_NONE: D - A,
 *   HSCN_LAP_SYM: I - D^-1/2 A D^-1/2, HSCN_LAP_RW: I - D^-1 A (1/0 -> 0), in float32; the matrix decomposed is its
 *   lower triangle mirrored (what numpy's eigh reads).  Decomposition: two-sided cyclic Jacobi in round-robin order
 *   until the off-diagonal mass is at most 1e-15 of the squared Frobenius norm, at most 30 sweeps.
 *   eigvecs [N, max_freqs] f32: per graph the max_freqs smallest eigenpairs in ascending order, each vector divided
 *   by its HSCN_VECNORM_L1 / _L2 / _ABSMAX norm over the graph's nodes (clamped at 1e-12); eigvals [N, max_freqs]
 *   f32: the eigenvalues clamped at 0, the same row for every node of the graph; columns from the graph's node count
 *   on are NaN in both.
 *   flag [1] i32, zeroed by the caller, only ever OR-ed into: bit 0 = a graph reached the sweep cap, bit 1 = an edge
 *   with an end outside its graph (dropped), bit 2 = a graph larger than max_n or outside [0, N) (its rows are NaN).
 *   Graphs of at most hscn_lap_eig_lds_max_n() nodes are decomposed in LDS, larger ones (up to 512) in their slab of
 *   `workspace`: hscn_lap_eig_workspace_bytes(B, max_n) bytes, 0 when max_n fits LDS.  A workspace with 4 * B more
 *   bytes than that receives every graph's sweep count (int32) in those last words.
 *   No float atomics: the same input gives the same bits.
 *   HSCN_E_BADARG for null pointers, negative sizes, max_freqs < 1, an unknown lap_norm / eigvec_norm or a workspace
 *   smaller than asked; HSCN_E_UNSUPPORTED where hscn_lap_eig_supported is 0 (max_n > 512 or max_freqs > 64); both
 *   before any launch.  B = 0 or N = 0 launches nothing.
 * ------------------------------------------------------------------------- */
#define HSCN_LAP_NONE 0
#define HSCN_LAP_SYM 1
#define HSCN_LAP_RW 2
#define HSCN_VECNORM_L1 0
#define HSCN_VECNORM_L2 1
#define HSCN_VECNORM_ABSMAX 2
int hscn_lap_eig_supported(int max_n, int max_freqs);
int hscn_lap_eig_lds_max_n(void);
size_t hscn_lap_eig_workspace_bytes(int64_t B, int max_n);
int hscn_lap_eig_stats(const int64_t* edge_index, int64_t E, const int32_t* nptr, const int32_t* eptr, int64_t N,
                       int64_t B, int max_n, int lap_norm, int is_undirected, int max_freqs, int eigvec_norm,
                       float* eigvals, float* eigvecs, int32_t* flag, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------- *
 * HSCN with the opt-in virtual -> local relation (graph_hscn.model.hscn.HSCN(vl_conv="GAT"): a fourth HeteroConv
 * entry the reference never wired up, with which the virtual branch reaches the prediction) as ONE training-step
 * launch, one workgroup per graph, plus the gradient fold (csrc/resident_vl.hip).  Purely additive to ABI 23.
 *   layer:  x_l' = relu((A_ll (x_l W_ll^T) + b_ll) + ((x_v W_vl,src^T)[c(i)] + b_vl))
 *           x_v' = relu((A_vv (x_v W_vv^T) + b_vv) + (sum_{i in v} alpha_i (x_l W_lv,src^T)_i + b_lv))
 *   A_* = GCN normalisation WITHOUT self loops over the edge list as given (in-degree; in-degree 0: the bias only);
 *   alpha = GATConv's segment softmax of leaky_relu(a_src[i] + a_dst[v], slope) over the members of cluster v;
 *   c(i) = the target of local node i's one local -> virtual edge (the virtual -> local edge list is that list
 *   reversed, so its attention weight is exactly 1 and its lin_dst / att_src / att_dst get exactly zero gradients);
 *   then the mean pool over local nodes, lin_1 -> head_act -> lin_2 and the loss row (loss_kind 0 = BCE with logits,
 *   1 = L1; inv_count = 1 / (B C)).
 *   x_local [N,F], x_virtual [V,F] f32; ei_* int64 [2,E_*] batch numbering; graph g owns local nodes
 *   [lptr[g], lptr[g+1]), virtual nodes [vptr[g], ...) and the edge ranges eptr_*[g] .. eptr_*[g+1] (int32, B + 1).
 *   layer_params_host: HOST array of L x 14 device pointers {W_ll, b_ll, W_vv, b_vv, lv: W_src, W_dst, att_src,
 *   att_dst, b, vl: W_src, W_dst, att_src, att_dst, b} (W [H,fin], fin = F for layer 0 else H); W1, b1, W2, b2.
 *   partials [B, P+1]; grads [P+1] = dL/d params, grads[P] = the mean loss (P = hscn_vl_param_count: every
 *   parameter).  Column order: layers 0 .. L-2 in pointer order, the last layer's {W_ll, b_ll, vl: five}, W1, b1, W2,
 *   b2, then the last layer's {W_vv, b_vv, lv: five} -- those do not reach the prediction, their columns are zeros,
 *   and the live gradients tile the front of the buffer.  workspace: (L-1) N H floats (the local activations the backward reads again).
 *   accumulate != 0: the fold ADDS every parameter column to grads (grads[P] is still the loss of this call).
 *   flag: bit 2 = an edge with an end outside its graph (dropped), bit 4 = a graph beyond max_n / max_v / max_ell /
 *   max_evv (or more local -> virtual edges than max_n) or the arrays (its rows are zeros), bit 16 = a local node with
 *   more than one local -> virtual edge.  Fixed summation orders, no float atomics: the same input gives the same bits.
 *   B = 0 launches nothing (0); a NULL target, partials or grads is HSCN_E_BADARG.
 * hscn_vl_forward: the forward alone: pred, score (optional), with a target the per-graph loss-term sums loss_rows
 *   [B] and, if loss != NULL, the mean loss; xv_out [V,H] (optional): the final virtual features (without it the last
 *   layer's virtual update is skipped).
 * hscn_vl_supported: H in {16, 32}, 1 <= F <= H, C <= min(H, 16), 1 <= L <= 8 and a layout of the largest graph within
 *   160 KB of LDS (H = 16, L = 3: Peptides' 444 nodes with 16 clusters).
 * ------------------------------------------------------------------------- */
int hscn_vl_supported(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv);
int64_t hscn_vl_param_count(int F, int H, int L, int C);
int hscn_vl_train_step(const float* x_local, const float* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                       const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr,
                       const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv,
                       int64_t N, int64_t V, int64_t B, int F, int H, int L, int C, int head_act, float slope,
                       const void* const* layer_params_host /* L x 14 */, const float* W1, const float* b1,
                       const float* W2, const float* b2, int max_n, int max_v, int max_ell, int max_evv,
                       const float* target, int loss_kind, float inv_count, float* pred, float* score /*or NULL*/,
                       float* partials /*[B,P+1]*/, float* grads /*[P+1]*/, float* workspace /*[(L-1) N H]*/,
                       int32_t* flag, int accumulate, void* stream);
int hscn_vl_forward(const float* x_local, const float* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                    const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr,
                    const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv,
                    int64_t N, int64_t V, int64_t B, int F, int H, int L, int C, int head_act, float slope,
                    const void* const* layer_params_host /* L x 14 */, const float* W1, const float* b1,
                    const float* W2, const float* b2, int max_n, int max_v, int max_ell, int max_evv,
                    const float* target /*or NULL*/, int loss_kind, float inv_count, float* pred,
                    float* score /*or NULL*/, float* loss_rows /*[B] or NULL*/, float* loss /*[1] or NULL*/,
                    float* xv_out /*[V,H] or NULL*/, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------- *
 * Link-level tasks: the pair decoder and the per-graph ranking metric (graph_hscn.nn.head.pair_dot,
 * graph_hscn.metrics; csrc/edge_head.hip).  Purely additive to ABI 23.
 *   z [N, D] f32 row-major, 16-byte aligned (rows move as float4); pair_index [2, P] i32, row 0 the source u, row 1
 *   the target v, ids into z; N, P < 2^31.
 * hscn_pair_dot_supported: the envelope, D a multiple of 4 with 4 <= D <= 64 (the single source of truth: the
 *   launches answer HSCN_E_UNSUPPORTED outside it).  A lane group of D / 4 lanes rounded up to a power of two owns a
 *   pair; hscn_pair_dot_pairs_per_workgroup(D) = 256 / that (0 outside the envelope).
 * hscn_pair_dot_fwd: ONE launch, score[p] = sum_k z[u_p, k] z[v_p, k]: per lane a product and three fmaf over its four
 *   columns in column order, then an xor-shuffle tree over the lane group, widest offset first -- an order that depends
 *   on D alone.  A pair with an id outside [0, N) is not dereferenced: its score is 0 and HSCN_PAIR_ID_OUT_OF_RANGE is
 *   ORed into flags [1] (the caller zeroes the word).  P = 0 launches nothing.
 * hscn_pair_dot_bwd: ONE launch, g_z[i] = sum_{p: u_p = i} g_p z[v_p] + sum_{p: v_p = i} g_p z[u_p] with
 *   g_p = g_score[p] (times scale [1], a device scalar, unless NULL): the node's by-source list first, then its
 *   by-target list, one fmaf per incidence.  src_rowptr / dst_rowptr [N + 1] and src_perm / dst_perm [P] are the
 *   stable CSRs of the pair list keyed by source / by target (perm = pair ids, ascending inside a row;
 *   hscn_csr_build_pair's rowptr_t / eid_t and rowptr / eid); an entry outside [0, P), or whose other endpoint lies
 *   outside [0, N), is skipped.  A pair (i, i) contributes 2 g z[i].  g_z [N, D] is written, not accumulated: a node
 *   without incidences gets an exact zero row.  No float atomics: the same input gives the same bits.
 *
 * hscn_pair_rank: for every positive pair (edge_label[p] == 1) of every graph, its rank among the scores s(u, w) of
 *   the graph's other nodes w, each score evaluated exactly as hscn_pair_dot_fwd evaluates it.  One workgroup per
 *   graph (hscn_pair_rank_max_workgroups() at most, a workgroup strides over the graphs).
 *     ptr [B + 1] i32 node ranges, pair_ptr [B + 1] i32 pair ranges, edge_label [P] f32;
 *     pos_rowptr [N + 1] / pos_perm: the stable CSR of the POSITIVE pairs keyed by source (read for filter >= 1);
 *     filter: HSCN_PAIR_FILTER_NONE     Neg(u, v) = every node w != v of the graph (u itself and u's other positive
 *                                       partners included);
 *             HSCN_PAIR_FILTER_POSITIVES  additionally without any w != v such that (u, w) is a positive candidate
 *                                       (counted over all nodes, then subtracted over u's positive list: candidates
 *                                       are distinct within a graph);
 *             HSCN_PAIR_FILTER_POSITIVES_SELF  additionally without w == u.
 *     With g = #{w in Neg: s(u, w) > s(u, v)} and e = #{... == ...}: rank2 [P] i32 (or NULL) = 2 g + e, that is
 *     rank = 1 + g + e / 2, the mean of the optimistic and the pessimistic rank; -1 for every pair that is not ranked.
 *     per_graph [B, 5] f64 = { sum 2 / (rank2 + 2) added in ascending pair id, #(rank <= 1), #(rank <= 3),
 *     #(rank <= 10) as the integer comparisons rank2 + 2 <= 2 K, the number of ranked positives }.
 *   flags [1] i32, ORed into (the caller zeroes the word): HSCN_PAIR_ID_OUT_OF_RANGE = a pair with an endpoint outside
 *   its graph's node range; HSCN_PAIR_NAN_SCORE = a NaN score (a positive whose own score is NaN is not ranked, a NaN
 *   competitor counts neither as greater nor as equal); HSCN_PAIR_LABEL_NOT_BINARY = a label outside {0, 1};
 *   HSCN_PAIR_BAD_SEGMENT = a graph whose ptr / pair_ptr entries are not ascending inside [0, N] / [0, P] (its row of
 *   per_graph is zeros).  None of these is dereferenced or counted.
 *   hscn_pair_rank_supported(max_nodes, D): 0 outside hscn_pair_dot_supported's envelope; 1 when a graph of max_nodes
 *   nodes is staged in LDS (up to hscn_pair_rank_lds_max_nodes(D) = 60 KB / (16 B * lane-group width) rows, row stride
 *   = 4 * lane-group width floats); 2 when the same kernel reads its rows from global memory.  No workspace.
 *   max_nodes: the node count of the batch's largest graph, which sizes the launch's LDS (16 B * lane-group width per
 *   node instead of the whole 60 KB budget); 0 or less = unknown, the whole budget.  A graph with more nodes than
 *   max_nodes is still served, from global memory.  A pair outside every graph's [pair_ptr[g], pair_ptr[g + 1]), or
 *   of a graph flagged HSCN_PAIR_BAD_SEGMENT, is not visited: the caller presets rank2 (graph_hscn.metrics: -1).
 * hscn_pair_rank_reduce: one small launch, result [4] f64 = { MRR, Hits@1, Hits@3, Hits@10 }.  HSCN_PAIR_AVG_GRAPH:
 *   per graph the mean over its positives, then the mean over the graphs that have at least one, in graph order;
 *   HSCN_PAIR_AVG_POOLED: one mean over all positives.  acc_sum [4] f64 / acc_count [1] i64 (both or neither): running
 *   sums and count of an epoch -- the launch adds this table's graphs to them, in order, and divides the totals, so
 *   several batches cost one host copy at the end and give the bits of one call on their union.  No positive at all:
 *   result is 0 and HSCN_PAIR_NO_POSITIVE is ORed into flags; a call whose total holds a positive clears that one bit
 *   (so an epoch's leading batches without positives leave nothing behind), every other bit is only ever ORed.
 * HSCN_E_BADARG for null pointers, sizes negative or beyond 2^31 - 1, a misaligned z or g_z, an unknown filter or
 * averaging; HSCN_E_UNSUPPORTED outside the envelope; both before any launch.
 * ------------------------------------------------------------------------- */
#define HSCN_PAIR_ID_OUT_OF_RANGE 1
#define HSCN_PAIR_NAN_SCORE 2
#define HSCN_PAIR_LABEL_NOT_BINARY 4
#define HSCN_PAIR_BAD_SEGMENT 8
#define HSCN_PAIR_NO_POSITIVE 16
#define HSCN_PAIR_FILTER_NONE 0
#define HSCN_PAIR_FILTER_POSITIVES 1
#define HSCN_PAIR_FILTER_POSITIVES_SELF 2
#define HSCN_PAIR_AVG_GRAPH 0
#define HSCN_PAIR_AVG_POOLED 1
int hscn_pair_dot_supported(int D);
int hscn_pair_dot_pairs_per_workgroup(int D);
int hscn_pair_dot_fwd(const float* z, const int32_t* pair_index, int64_t N, int64_t P, int D, float* score /*[P]*/,
                      int32_t* flags /*[1]*/, void* stream);
int hscn_pair_dot_bwd(const float* z, const int32_t* pair_index, const float* g_score /*[P]*/,
                      const float* scale /*[1] or NULL*/, const int32_t* src_rowptr, const int32_t* src_perm,
                      const int32_t* dst_rowptr, const int32_t* dst_perm, int64_t N, int64_t P, int D,
                      float* g_z /*[N,D]*/, void* stream);
int hscn_pair_rank_supported(int max_nodes, int D);
int hscn_pair_rank_lds_max_nodes(int D);
int hscn_pair_rank_max_workgroups(void);
int hscn_pair_rank(const float* z, const int32_t* ptr, const int32_t* pair_ptr, const int32_t* pair_index,
                   const float* edge_label, const int32_t* pos_rowptr, const int32_t* pos_perm, int64_t B, int64_t N,
                   int64_t P, int D, int filter, int max_nodes, int32_t* rank2 /*[P] or NULL*/,
                   double* per_graph /*[B,5]*/, int32_t* flags /*[1]*/, void* stream);
int hscn_pair_rank_reduce(const double* per_graph, int64_t B, int averaging, double* acc_sum /*[4] or NULL*/,
                          int64_t* acc_count /*[1] or NULL*/, double* result /*[4]*/, int32_t* flags /*[1]*/,
                          void* stream);

/* ------------------------------------------------------------------------- *
 * Random-walk structural encoding (RWSE) of a collated batch as ONE launch (graph_hscn.transform.rwse;
 * csrc/rwse.hip): the eigensolver-free positional statistics.  Purely additive to ABI 23.
 *
 * hscn_rwse_stats: rowptr [N + 1] / col: the stable CSR of the batch's edge list keyed by SOURCE, in batch numbering
 *   (hscn_csr_build(src, dst), or hscn_csr_build_pair's rowptr_t / col_t): row r lists the targets of r.  Graph g owns
 *   nodes [nptr[g], nptr[g+1]) (int32, B + 1 entries); max_n >= the largest graph's node count.
 *   A[r, c] = the number of listed edges r -> c (duplicates sum, self loops are KEPT -- the Laplacian launch drops
 *   them); deg[r] = rowptr[r+1] - rowptr[r], the out-degree; P = D^-1 A, a row with deg 0 all zero.
 *   rw [N, ksteps] f32: rw[i, k-1] = (P^k)[i, i], k = 1 .. ksteps; a node without out-edges gets zeros.
 *   Evaluated on column vectors, q_0 = e_i, q_{t+1}[r] = (1 / deg[r]) * sum_{c in row r} q_t[c], rw[i, t] = q_{t+1}[i]:
 *   the sum in CSR order with plain float32 adds, then one reciprocal and one multiply.  All terms are non-negative:
 *   an entry whose exact value is 0 is exactly 0.  No float atomics: the same input gives the same bits.
 *   One workgroup per (graph, tile of hscn_rwse_tile() start nodes), grid B x ceil(max_n / tile): the tile's vectors
 *   live in LDS as a ping-pong pair q[node][tile], 2 * max_n * tile * 4 bytes (64 KB at 512 nodes), one barrier per
 *   step; a tile past its graph's node count returns at once.  No workspace.
 *   flag [1] i32, zeroed by the caller, only ever OR-ed into: bit 1 = a CSR entry outside its graph's node range (it
 *   adds nothing to its sum), bit 2 = a graph larger than max_n or outside [0, N) (its rows are NaN); bit 0 is unused,
 *   so the bits read as hscn_lap_eig_stats's.
 *   HSCN_E_BADARG for null pointers, negative sizes or ksteps < 1; HSCN_E_UNSUPPORTED where hscn_rwse_supported is 0
 *   (max_n outside [1, 512] or ksteps > 64); both before any launch.  B = 0 or N = 0 launches nothing.
 * ------------------------------------------------------------------------- */
int hscn_rwse_supported(int max_n, int ksteps);
int hscn_rwse_tile(void);
int hscn_rwse_stats(const int32_t* rowptr, const int32_t* col, const int32_t* nptr, int64_t N, int64_t B, int max_n,
                    int ksteps, float* rw /*[N, ksteps]*/, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * GINEConv's aggregate with edge features (PyG GINEConv with edge_dim; csrc/gine.hip).  Purely additive to ABI 23.
 *
 *   t_k = bias + W e_k                     e_k = edge_attr[k] (row k belongs to edge k of the edge list),  W [F, De]
 *   z_i = (1 + eps) x_i + sum_{k: dst_k = i} relu(x[src_k] + t_k)        every listed edge counts (loops, repeats)
 *
 * hscn_gine_aggregate_fwd: ONE launch, z [N, F] from the target-keyed stable CSR (hscn_csr_build(dst, src), or
 *   hscn_csr_build_pair's rowptr / col / eid): slot p of row i gathers x[col[p]] and the edge-feature row
 *   edge_attr[eid[p]].  t_k is evaluated inside the gather; no [E, F] buffer is written.  Sums run in CSR slot order
 *   with separately rounded multiply and add.  Rows of more than hscn_gine_long_row() slots are summed by a whole
 *   workgroup in chunks of hscn_gine_chunk() slots, the chunk partials added in chunk order: the same input gives the
 *   same bits.
 * hscn_gine_aggregate_bwd_x: gx_j = (1 + eps) gz_j + sum_{k: src_k = j} [x_j + t_k > 0] gz[dst_k], ONE launch over the
 *   source-keyed CSR (rowptr_t / col_t / eid_t); the gates are recomputed, nothing is kept by the forward.
 * hscn_gine_aggregate_bwd_msg: gm [E, F], gm_k = [x[src_k] + t_k > 0] gz[dst_k] in edge order (edge_index int64
 *   [2, E]), written once with plain stores.  d W = hscn_linear_bwd_w(gm, edge_attr), d bias its gb: ordered, no
 *   float atomics.  An edge with a node id outside [0, N) gives a zero row and flag bit 0.
 *   flag [1] i32, only ever OR-ed into (the CSR build's flag word serves): bit 0 as above, bit 1 = a CSR column
 *   outside [0, N) or an eid outside [0, E) (the slot adds nothing; hscn_csr_build never produces one).
 *   HSCN_E_BADARG for null pointers (col / eid / edge_attr may be NULL when E == 0) and negative sizes;
 *   HSCN_E_UNSUPPORTED where hscn_gine_supported is 0 (F outside [1, 512] or De outside [1, 64]); both before any
 *   launch.  N = 0 launches nothing.  No workspace, no host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_gine_supported(int F, int De);
int hscn_gine_long_row(void);
int hscn_gine_chunk(void);
int hscn_gine_aggregate_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* x,
                            const float* edge_attr, const float* W, const float* bias, float eps, float* z /*[N, F]*/,
                            int64_t N, int64_t E, int F, int De, int32_t* flag /*[1]*/, void* stream);
int hscn_gine_aggregate_bwd_x(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* x,
                              const float* edge_attr, const float* W, const float* bias, float eps, const float* gz,
                              float* gx /*[N, F]*/, int64_t N, int64_t E, int F, int De, int32_t* flag /*[1]*/,
                              void* stream);
int hscn_gine_aggregate_bwd_msg(const int64_t* edge_index, const float* x, const float* edge_attr, const float* W,
                                const float* bias, const float* gz, float* gm /*[E, F]*/, int64_t N, int64_t E, int F,
                                int De, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Global attention: block-diagonal multi-head self-attention over a collated batch (csrc/attention.hip), the global
 * half of a GPS layer.  Purely additive to ABI 24.
 *
 *   qkv [N, 3D] f32 row-major, the packed input projection: Q = columns [0, D), K = [D, 2D), V = [2D, 3D); head h owns
 *   columns [h dh, (h + 1) dh) of each third (torch.nn.MultiheadAttention's layout); D = heads * dh; scale = dh^-1/2.
 *   Node i of graph g attends to the nodes [ptr32[g], ptr32[g + 1]) of its graph, itself included:
 *     out_i = sum_j p_ij v_j,   p_ij = exp(scale <q_i, k_j> - lse_i),   lse_i = log sum_j exp(scale <q_i, k_j>)
 *
 * hscn_attention_fwd: ONE launch; out [N, D], lse [N, heads].  A workgroup takes hscn_attention_tile() query rows of
 *   one (graph, head) and streams the graph's keys and values through LDS in chunks of hscn_attention_chunk() keys with
 *   an online softmax.  Nothing padded is ever written: memory is O(N D), and a graph may have any number of nodes.
 *   A row depends on its own graph's rows only, in key and chunk order from the graph's first node: the same bits
 *   wherever the graph stands in the batch.  A graph of one node gives out = v and lse = s_00 exactly.
 * hscn_attention_bwd_q: ONE launch, query-keyed; recomputes p from lse.  Writes delta [N, heads], delta_i =
 *   sum_d g_out_id out_id, and the Q third of g_qkv [N, 3D]: gQ_i = scale sum_j p_ij (<g_out_i, v_j> - delta_i) k_j.
 * hscn_attention_bwd_kv: ONE launch, key-keyed, after hscn_attention_bwd_q (it reads delta).  Writes the K and V thirds
 *   of g_qkv: gV_j = sum_i p_ij g_out_i, gK_j = scale sum_i p_ij (<g_out_i, v_j> - delta_i) q_i, i in row order.
 *   g_qkv is written once with plain stores, no float atomics; it feeds hscn_linear_bwd_w and the input-gradient linear.
 *   max_nodes sizes the grid (ceil(max_nodes / tile) workgroups per graph and head).  flag [1] i32, only ever OR-ed
 *   into: bit 2 = a graph with more than max_nodes nodes, whose rows of every output are NaN.  Graph ranges are clamped
 *   to [0, N].  An empty graph owns no rows.
 *   HSCN_E_BADARG for negative sizes, N or B beyond 2^31 - 1, null pointers, or a qkv / out / g_out / g_qkv that is not
 *   16-byte aligned; HSCN_E_UNSUPPORTED where hscn_attention_supported is 0 (it wants heads >= 1, dh % 4 == 0,
 *   4 <= dh <= 64, heads * dh <= 512); both before any launch.  N = 0 or B = 0 launches nothing (0).  No workspace, no
 *   host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_attention_supported(int heads, int dh);
int hscn_attention_tile(void);
int hscn_attention_chunk(void);
int hscn_attention_fwd(const float* qkv, const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh,
                       float* out /*[N, D]*/, float* lse /*[N, heads]*/, int32_t* flag /*[1]*/, void* stream);
int hscn_attention_bwd_q(const float* qkv, const float* out, const float* lse, const float* g_out,
                         const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh,
                         float* g_qkv /*[N, 3D]*/, float* delta /*[N, heads]*/, int32_t* flag /*[1]*/, void* stream);
int hscn_attention_bwd_kv(const float* qkv, const float* lse, const float* delta, const float* g_out,
                          const int32_t* ptr32, int64_t N, int64_t B, int max_nodes, int heads, int dh,
                          float* g_qkv /*[N, 3D]*/, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * GatedGCN's aggregate (GraphGPS GatedGCNLayer, residual gated graph ConvNets; csrc/gatedgcn.hip).  Purely additive
 * to ABI 24.  With j = src_k, i = dst_k and Ax, Bx, Dx, Ex [N, H], Ce [E, H] already transformed (row k of Ce, e_out
 * and ge belongs to edge k of the edge list, not to a CSR slot):
 *
 *   e_out_k = Dx_i + Ex_j + Ce_k        s_k = 1 / (1 + exp(-e_out_k))
 *   h_i     = Ax_i + (sum_{k: dst_k = i} s_k * Bx_j) / (den_i + 1e-6),   den_i = sum_{k: dst_k = i} s_k
 *
 * Every listed edge counts (loops, repeats).  Sums run in CSR slot order with separately rounded multiply and add; rows
 * of more than hscn_gatedgcn_long_row() slots are summed by a whole workgroup in chunks of hscn_gatedgcn_chunk()
 * slots, the partials added in chunk order: a row depends on the row alone, the same input gives the same bits.
 *
 * hscn_gatedgcn_fwd: ONE launch over the target-keyed stable CSR; writes h, den [N, H] and e_out [E, H] (plain stores
 *   at row eid[slot]).  A node without edges gets h_i = Ax_i bit for bit.
 * hscn_gatedgcn_bwd_dst: ONE launch over the same CSR.  gn_i = gh_i / (den_i + 1e-6) is stored ([N, H]).  With ge and
 *   gDx given it also walks the edges: ge_k = g_e_out_k + (gn_i Bx_j - gn_i (h_i - Ax_i)) s_k (1 - s_k), stored once
 *   (the gradient of Ce), and gDx_i = sum ge_k.  g_e_out may be NULL (no cotangent for e_out).  ge = gDx = NULL: gn
 *   alone (only Bx asks for a gradient).
 * hscn_gatedgcn_bwd_src: ONE launch over the source-keyed CSR: gBx_j = sum_{k: src_k = j} s_k gn_i and
 *   gEx_j = sum ge_k; either output may be NULL and is then not computed.  The gradient of Ax is gh itself.
 *   No float atomics anywhere: every output row has one owner.
 * flag [1] i32: the CSR's flag word.  It is read: when it is non-zero (hscn_csr_build left an edge out because a node
 *   id lies outside [0, N)), fwd / bwd_dst store a ZERO row of e_out / ge for every such edge of edge_index, so no
 *   row of either is left unwritten.  Bit 1 is OR-ed in for a slot with a column outside [0, N) or an eid outside
 *   [0, E) (the slot adds nothing; hscn_csr_build never produces one).
 *   HSCN_E_BADARG for null pointers (col / eid / edge_index / Ce / e_out / ge may be NULL when E == 0) and negative
 *   sizes; HSCN_E_UNSUPPORTED where hscn_gatedgcn_supported is 0 (H outside [1, 512]); both before any launch.
 *   N = 0 launches nothing.  No workspace, no host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_gatedgcn_supported(int H);
int hscn_gatedgcn_long_row(void);
int hscn_gatedgcn_chunk(void);
int hscn_gatedgcn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int64_t* edge_index,
                      const float* Ax, const float* Bx, const float* Dx, const float* Ex, const float* Ce,
                      float* h /*[N, H]*/, float* e_out /*[E, H]*/, float* den /*[N, H]*/, int64_t N, int64_t E, int H,
                      int32_t* flag /*[1]*/, void* stream);
int hscn_gatedgcn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int64_t* edge_index,
                          const float* Ax, const float* Bx, const float* h, const float* e_out, const float* den,
                          const float* gh, const float* g_e_out, float* gn /*[N, H]*/, float* ge /*[E, H]*/,
                          float* gDx /*[N, H]*/, int64_t N, int64_t E, int H, int32_t* flag /*[1]*/, void* stream);
int hscn_gatedgcn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* e_out,
                          const float* gn, const float* ge, float* gBx /*[N, H]*/, float* gEx /*[N, H]*/, int64_t N,
                          int64_t E, int H, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Categorical encoders (OGB AtomEncoder / BondEncoder; csrc/catenc.hip).  Purely additive to ABI 24.  F integer
 * columns share ONE table W [R, D] float32, R = sum_c card_c; column c owns rows off_c .. off_c + card_c - 1 with
 * off_c = card_0 + .. + card_{c-1}.  idx is int64 [n, F], row-major.  card_host [F] is read on the HOST during the
 * call (it travels as a launch argument), every other pointer is device memory.
 *
 * hscn_catenc_supported: 1 for D a multiple of 4 in [4, 512], 1 <= F <= 16, F <= R <= 4096.
 * hscn_catenc_fwd: ONE launch.  out[i] = ((0 + W[off_0 + idx[i,0]]) + W[off_1 + idx[i,1]]) + ..., the adds in column
 *   order, each rounded separately.  An index outside [0, card_c) is never dereferenced: its term is skipped and bit 0
 *   of flag is OR-ed in.  n = 0 launches nothing.
 * hscn_catenc_index_build: four launches, a stable counting sort of the n F items (i, c) by table row
 *   off_c + idx[i, c]: rowptr [R + 1] (rowptr[R] = the items kept) and item [n F], the ids i of each table row in
 *   ascending order.  Items with an index outside its column are left out and bit 0 of flag is OR-ed in; item beyond
 *   rowptr[R] is left unwritten.  Work O(n F + chunks R) with chunks = ceil(n F / hscn_catenc_sort_chunk()); counts
 *   are integers, nothing depends on an arrival order.  n = 0: rowptr is zeroed.
 * hscn_catenc_bwd: two launches.  dW[r] = sum over slots p in [rowptr[r], rowptr[r+1]) of dOut[item[p]], every row of
 *   dW written (a row without items gets exact zeros).  A row of at most hscn_catenc_long_row() slots is summed in
 *   slot order from zero; a longer one is cut into chunks of hscn_catenc_chunk() slots counted from its first slot,
 *   each summed in slot order from zero -- by whichever workgroup takes it -- and the partials are added in chunk order
 *   from zero.  No float atomics: the bits of a row depend on its values in slot order alone, not on the launch
 *   geometry or on the rest of the batch.  A slot with an id outside [0, n), or a rowptr outside [0, n F], adds
 *   nothing and ORs bit 1 into flag (hscn_catenc_index_build produces neither).
 * Workspaces: hscn_catenc_index_workspace_bytes (the per-chunk histograms, R ints per chunk) and
 *   hscn_catenc_bwd_workspace_bytes = (ceil(n F / chunk) + R) * D floats; neither needs initialising.
 * HSCN_E_BADARG for null pointers, negative sizes, an empty column or n F beyond INT32_MAX; HSCN_E_UNSUPPORTED outside
 *   the envelope; HSCN_E_WORKSPACE for a workspace that is too small; all before any launch.  No host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_catenc_supported(int D, int F, int R);
int hscn_catenc_long_row(void);
int hscn_catenc_chunk(void);
int hscn_catenc_sort_chunk(void);
int hscn_catenc_fwd(const float* W /*[R, D]*/, const int64_t* idx /*[n, F]*/, const int32_t* card_host /*[F], host*/,
                    float* out /*[n, D]*/, int64_t n, int F, int D, int32_t* flag /*[1]*/, void* stream);
size_t hscn_catenc_index_workspace_bytes(int64_t n, int F, int R);
int hscn_catenc_index_build(const int64_t* idx /*[n, F]*/, const int32_t* card_host /*[F], host*/, int64_t n, int F,
                            int32_t* rowptr /*[R + 1]*/, int32_t* item /*[n F]*/, int32_t* flag /*[1]*/,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t hscn_catenc_bwd_workspace_bytes(int64_t n, int F, int R, int D);
int hscn_catenc_bwd(const int32_t* rowptr /*[R + 1]*/, const int32_t* item /*[n F]*/, const float* dOut /*[n, D]*/,
                    float* dW /*[R, D]*/, int64_t n, int F, int R, int D, int32_t* flag /*[1]*/, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Edge attention: the message / aggregate of PyG's TransformerConv with dropout = 0 (csrc/edge_attention.hip).  Purely
 * additive to ABI 24.  `heads` heads of width `head_dim` (HC = heads * head_dim), q [Nd, HC], k and v [Ns, HC], e
 * [E, HC] or NULL; with j = src_k, i = dst_k and scale = 1 / sqrt(head_dim), per head h:
 *
 *   s_k   = scale * sum_c q[i,h,c] * (k[j,h,c] + e[k,h,c])
 *   a_k   = exp(s_k - lse_i),   lse_i = log sum_{k: dst_k = i} exp(s_k) = m_i + log sum_k exp(s_k - m_i),  m_i = max_k s_k
 *   out_i = sum_{k: dst_k = i} a_k * (v[j,h,:] + e[k,h,:])                  (exact zeros for a node without in-edges)
 *
 * Every listed edge counts (loops, repeats); row k of e and de belongs to edge k of the edge list, not to a CSR slot
 * (every slot goes through eid).  The relation may be bipartite.  Sums run in CSR slot order; a row of more than
 * hscn_edge_attn_long_row() slots is taken by a whole workgroup in chunks of hscn_edge_attn_chunk() slots whose
 * partials -- (max, sum, accumulator) triples in the forward, plain sums in the backward -- are merged in chunk
 * order: a row depends on the row alone, the same input gives the same bits.  No float atomics, no [E, heads] tensor.
 *
 * hscn_edge_attn_supported: 1 for heads >= 1, head_dim >= 1, heads * head_dim <= 512.  16-byte accesses are used where
 *   head_dim % 4 == 0 and every tensor is 16-byte aligned, 4-byte accesses otherwise.
 * hscn_edge_attn_fwd: ONE launch over the target-keyed stable CSR; writes out [Nd, HC] and lse [Nd, heads, 2]: the one
 *   log-sum-exp per (node, head) as its two summands (m_i, log sum_k exp(s_k - m_i)), so that the backward's
 *   exp((s_k - m_i) - log sum) loses nothing to the magnitude of the logits; (0, 0) for a node without in-edges.
 * hscn_edge_attn_bwd_dst: ONE launch over the same CSR.  delta_i = sum_c g_out_i out_i per head is stored
 *   ([Nd, heads]).  With ds_k = a_k (g_out_i . (v_j + e_k) - delta_i):  dq_i = sum_k scale ds_k (k_j + e_k) and
 *   de_k = a_k g_out_i + scale ds_k q_i, the latter stored once at row eid[slot].  dq, de may each be NULL and are
 *   then not computed (both NULL: delta alone).  de needs e.
 * hscn_edge_attn_bwd_src: ONE launch over the source-keyed CSR: dk_j = sum_{k: src_k = j} scale ds_k q_i and
 *   dv_j = sum a_k g_out_i; either may be NULL and is then not computed (both NULL: nothing is launched).
 * flag [1] i32: the CSR's flag word; bit 1 is OR-ed in for a slot with a column outside its range or an eid outside
 *   [0, E) (the slot adds nothing; hscn_csr_build never produces one).
 *   HSCN_E_BADARG for null pointers (col / eid / k / v may be NULL when E == 0, e always) and negative sizes;
 *   HSCN_E_UNSUPPORTED where hscn_edge_attn_supported is 0; both before any launch.  No workspace, no host
 *   synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_edge_attn_supported(int heads, int head_dim);
int hscn_edge_attn_long_row(void);
int hscn_edge_attn_chunk(void);
int hscn_edge_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* q, const float* k,
                       const float* v, const float* e, float* out /*[Nd, HC]*/, float* lse /*[Nd, heads, 2]*/, int64_t Nd,
                       int64_t Ns, int64_t E, int heads, int head_dim, int32_t* flag /*[1]*/, void* stream);
int hscn_edge_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* q,
                           const float* k, const float* v, const float* e, const float* out, const float* lse,
                           const float* g_out, float* delta /*[Nd, heads]*/, float* dq /*[Nd, HC]*/,
                           float* de /*[E, HC]*/, int64_t Nd, int64_t Ns, int64_t E, int heads, int head_dim,
                           int32_t* flag /*[1]*/, void* stream);
int hscn_edge_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* q,
                           const float* k, const float* v, const float* e, const float* lse, const float* delta,
                           const float* g_out, float* dk /*[Ns, HC]*/, float* dv /*[Ns, HC]*/, int64_t Nd, int64_t Ns,
                           int64_t E, int heads, int head_dim, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Shortest-path buckets (csrc/spd.hip) and the self-attention they bias (csrc/attention.hip, BiasArgs): Graphormer's
 * spatial encoding inside the global attention above.  Purely additive to ABI 24; the unbiased entry points are
 * unchanged.
 *
 * hscn_spd_buckets: ONE launch, one workgroup per graph.  d(i, j) = the fewest edges on a directed path i -> j inside
 *   graph g, following edge_index [2, E] i64 as source -> target (the edges of graph g are the columns
 *   [eptr32[g], eptr32[g + 1]), its nodes [ptr32[g], ptr32[g + 1])); d(i, i) = 0; self-loops and parallel edges change
 *   nothing.  bucket(i, j) = d(i, j) where d(i, j) < max_dist and max_dist otherwise (farther and unreachable alike):
 *   max_dist + 1 values, uint8, graph g's [n_g, n_g] matrix row-major (row = query i, column = key j) at
 *   bucket + spd_ptr[g]; spd_ptr [B + 1] i64 and total = the bucket tensor's length come from the caller (the running
 *   sums of n_g^2).  Adjacency and two reachability matrices are bitsets in LDS, breadth-first levels run one word (32
 *   targets) at a time for up to max_dist - 1 levels and stop when a level finds nothing.  Integers: the same result
 *   on every run, wherever the graph stands.  flag [1] i32, only ever OR-ed into: bit 0 = an edge with an end outside
 *   its graph (skipped), bit 1 = a graph with more than max_nodes nodes (all its buckets are max_dist) or whose range
 *   [spd_ptr[g], spd_ptr[g] + n_g^2) leaves [0, total) (not written).
 * hscn_spd_supported: 1 for max_dist in [1, 63] and 3 * max_nodes * ceil(max_nodes / 32) * 4 bytes + 1 KB within a
 *   CU's 160 KB of LDS (max_nodes <= 646).
 *   HSCN_E_BADARG for null pointers (edge_index may be NULL when E == 0), negative sizes, N, E or B beyond 2^31 - 1;
 *   HSCN_E_UNSUPPORTED where hscn_spd_supported is 0; both before any launch.  N = 0 or B = 0 launches nothing.
 *
 * hscn_attention_bias_fwd / _bwd_q / _bwd_kv: hscn_attention_fwd / _bwd_q / _bwd_kv with
 *     s_ij = scale <q_i, k_j> + table[bucket_ij, h]
 *   table [num_buckets, heads] f32, num_buckets <= 64; bucket / spd_ptr / total as above (a bucket value >=
 *   num_buckets is read as num_buckets - 1).  The same tiles, chunks, online softmax, lse and determinism; the logit is
 *   computed as the unbiased kernels compute it and the bias is added to it, so an all-zero table gives out, lse and
 *   g_qkv bit-equal to the unbiased entry points'.  The bucket bytes of a tile x chunk are staged through LDS by the
 *   whole wave along the key index.
 *   hscn_attention_bias_bwd_q also gives g_table [num_buckets, heads] (or NULL: not wanted): g_table[b, h] = sum over
 *   the pairs with bucket_ij = b of p_ij (<g_out_i, v_j> - delta_i).  No float atomics: a lane sums its row's terms per
 *   bucket in key order, a tile sums its lanes in lane order into workspace [B * tiles, heads, num_buckets] f32
 *   (tiles = max(1, ceil(max_nodes / hscn_attention_tile())); workspace_floats says how many floats it holds), and a
 *   second launch adds the tiles in tile order: bit-identical between runs.  g_qkv may be NULL there (the Q third is
 *   then not written; g_table must be given).  N = 0 or B = 0 with a g_table writes zeros to it.
 *   flag: the attention operator's word; bit 2 as above, bit 3 = a graph whose bucket range leaves [0, total): its
 *   rows are NaN too, and g_table with them.
 *   HSCN_E_BADARG / HSCN_E_UNSUPPORTED as the unbiased entry points, with hscn_attention_bias_supported =
 *   hscn_attention_supported and 1 <= num_buckets <= 64; HSCN_E_WORKSPACE for a workspace that is too small; all before
 *   any launch.  No host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_spd_supported(int max_nodes, int max_dist);
int hscn_spd_buckets(const int64_t* edge_index, const int32_t* ptr32, const int32_t* eptr32, const int64_t* spd_ptr,
                     int64_t N, int64_t E, int64_t B, int64_t total, int max_nodes, int max_dist,
                     uint8_t* bucket /*[total]*/, int32_t* flag /*[1]*/, void* stream);
int hscn_attention_bias_supported(int heads, int dh, int num_buckets);
int hscn_attention_bias_fwd(const float* qkv, const float* table, const uint8_t* bucket, const int64_t* spd_ptr,
                            const int32_t* ptr32, int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh,
                            int num_buckets, float* out /*[N, D]*/, float* lse /*[N, heads]*/, int32_t* flag /*[1]*/,
                            void* stream);
int hscn_attention_bias_bwd_q(const float* qkv, const float* out, const float* lse, const float* g_out,
                              const float* table, const uint8_t* bucket, const int64_t* spd_ptr, const int32_t* ptr32,
                              int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh, int num_buckets,
                              float* g_qkv /*[N, 3D]*/, float* delta /*[N, heads]*/, float* g_table, float* workspace,
                              int64_t workspace_floats, int32_t* flag /*[1]*/, void* stream);
int hscn_attention_bias_bwd_kv(const float* qkv, const float* lse, const float* delta, const float* g_out,
                               const float* table, const uint8_t* bucket, const int64_t* spd_ptr, const int32_t* ptr32,
                               int64_t N, int64_t B, int64_t total, int max_nodes, int heads, int dh, int num_buckets,
                               float* g_qkv /*[N, 3D]*/, int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * Exphormer: expander edges (csrc/expander.hip) and typed sparse attention (csrc/exphormer.hip).  Purely additive to
 * ABI 24.
 *
 * hscn_expander_build: ONE launch, one workgroup per graph.  degree is even, in [2, hscn_expander_max_degree() = 32].
 *   Graph g of n nodes gets degree / 2 random Hamiltonian cycles, each in both directions: n * degree edges at column
 *   degree * ptr32[g] of edge_index i64 [2, degree * N].  Cycle r: node t (local id) has the key
 *   (philox4x32_10(seed, ctr)[0] << 32) | t with ctr = (gid << 32) | (r << 16) | t, gid = graph_ids[g] (i32 [B]) or g
 *   when graph_ids is NULL; pi = the local ids in ascending key order (bitonic sort in LDS); block r holds
 *   pi[i] -> pi[(i + 1) mod n] for i = 0 .. n - 1 and then their reverses.  n = 1 gives loops, n = 2 repeats; nothing
 *   is rejected.  flag [1] i32, only OR-ed into: bit 0 = a graph with more than max_nodes nodes (its edges are -1) or
 *   a ptr32 that leaves [0, N] (nothing written for that graph).  max_nodes <= hscn_expander_max_nodes() = 2048.
 *   HSCN_E_BADARG for null pointers, negative sizes, an odd degree or one below 2; HSCN_E_UNSUPPORTED beyond the two
 *   limits; both before any launch.  N = 0 or B = 0 launches nothing.
 *
 * hscn_exph_attn_*: per head, over the in-edges of row i of a union graph with N rows and E edges,
 *     s_k = scale <q_i, k_j * e_k>,  w_k = exp(clamp(s_k, -5, 5)),  Z_i = sum_k w_k,
 *     out_i = (sum_k w_k v_j) / (Z_i + 1e-6)              scale = 1 / sqrt(head_dim), j = src_k
 *   e_k is row erow[k] of e_edge [El, HC] where erow[k] < El and row erow[k] - El of the table e_type [T, HC] otherwise
 *   (erow i32 [E], indexed by the union edge, reached from a CSR slot through eid; T <= hscn_exph_max_types() = 10;
 *   e_edge may be NULL with El = 0).  The CSR conventions, lane layout, long-row scheme and its two constants
 *   (hscn_exph_attn_long_row / _chunk) are those of hscn_edge_attn_*; q, k, v share the N rows.
 * hscn_exph_attn_fwd: ONE launch; out [N, HC] and z [N, heads] = Z_i (no shift: w <= e^5); zeros for an empty row.
 * hscn_exph_attn_bwd_dst: ONE launch over the same CSR; stores delta_i = sum_c g_out_i out_i [N, heads], and with
 *   ds_k = w_k (g_out_i . v_j - delta_i) / (Z_i + 1e-6) [-5 < s_k < 5]:  dq_i = scale sum_k ds_k (k_j * e_k) and, for
 *   slots with erow < El, de_edge[erow] = scale ds_k (q_i * k_j) (one writer: the caller lists each e_edge row once).
 *   dq, de_edge may be NULL (both NULL: delta alone).
 * hscn_exph_attn_bwd_src: ONE launch over the source-keyed CSR: dk_j = scale sum ds_k (q_i * e_k), dv_j =
 *   sum w_k g_out_i / (Z_i + 1e-6); either may be NULL (both: nothing is launched).
 * hscn_exph_attn_bwd_type: TWO launches; de_type[tau] = scale sum ds_k (q_i * k_j) over the union edges listed for
 *   type tau in trowptr [T + 1] / titem (edge ids in list order; edge_index i64 [2, E] names their ends).  A type of
 *   more than hscn_exph_type_long_row() slots is cut into chunks of hscn_exph_type_chunk() slots from its first
 *   slot; every chunk is a serial sum from zero stored as a partial, the second launch adds a type's partials in chunk
 *   order: the bits depend on the type's slots in list order alone.  A type without slots gets zeros.  workspace:
 *   hscn_exph_type_workspace_bytes = (E / chunk + T) * HC floats, not initialised by the caller.
 * No float atomics anywhere.  flag [1] i32: bit 1 is OR-ed in for a slot whose column, edge id, feature row or list
 *   range is out of range (the slot adds nothing).  HSCN_E_BADARG for null pointers and negative sizes,
 *   HSCN_E_UNSUPPORTED where hscn_exph_attn_supported is 0 (heads * head_dim > 512) or T > 10, HSCN_E_WORKSPACE for a
 *   short workspace; all before any launch.  No host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_expander_max_nodes(void);
int hscn_expander_max_degree(void);
int hscn_expander_build(const int32_t* ptr32 /*[B + 1]*/, const int32_t* graph_ids /*[B] or NULL*/, int64_t N, int64_t B,
                        int degree, uint64_t seed, int max_nodes, int64_t* edge_index /*[2, degree N]*/,
                        int32_t* flag /*[1]*/, void* stream);
int hscn_exph_attn_supported(int heads, int head_dim);
int hscn_exph_attn_long_row(void);
int hscn_exph_attn_chunk(void);
int hscn_exph_type_long_row(void);
int hscn_exph_type_chunk(void);
int hscn_exph_max_types(void);
int hscn_exph_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* erow /*[E]*/,
                       const float* q, const float* k, const float* v, const float* e_edge /*[El, HC] or NULL*/,
                       const float* e_type /*[T, HC]*/, float* out /*[N, HC]*/, float* z /*[N, heads]*/, int64_t N,
                       int64_t E, int64_t El, int T, int heads, int head_dim, int32_t* flag /*[1]*/, void* stream);
int hscn_exph_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* erow,
                           const float* q, const float* k, const float* v, const float* e_edge, const float* e_type,
                           const float* out, const float* z, const float* g_out, float* delta /*[N, heads]*/,
                           float* dq /*[N, HC]*/, float* de_edge /*[El, HC]*/, int64_t N, int64_t E, int64_t El, int T,
                           int heads, int head_dim, int32_t* flag /*[1]*/, void* stream);
int hscn_exph_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const int32_t* erow,
                           const float* q, const float* k, const float* v, const float* e_edge, const float* e_type,
                           const float* z, const float* delta, const float* g_out, float* dk /*[N, HC]*/,
                           float* dv /*[N, HC]*/, int64_t N, int64_t E, int64_t El, int T, int heads, int head_dim,
                           int32_t* flag /*[1]*/, void* stream);
size_t hscn_exph_type_workspace_bytes(int64_t E, int T, int heads, int head_dim);
int hscn_exph_attn_bwd_type(const int32_t* trowptr /*[T + 1]*/, const int32_t* titem, const int64_t* edge_index /*[2, E]*/,
                            const float* q, const float* k, const float* v, const float* e_type, const float* z,
                            const float* delta, const float* g_out, float* de_type /*[T, HC]*/, int64_t N, int64_t E,
                            int T, int heads, int head_dim, int32_t* flag /*[1]*/, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * LapPE node encoder, DeepSet model (csrc/lappe.hip).  Purely additive to ABI 24.
 *
 * vec, val f32 [N, K] (K = max_freqs): eigenvector entry and eigenvalue per node and frequency, what
 * hscn_lap_eig_stats writes; a NaN in vec[i, k] marks padding.  params_host: a HOST array of 2 * layers device
 * pointers W_0, b_0, W_1, b_1, ... with W_l f32 [H_l, H_{l-1}] row-major, b_l [H_l], H_{-1} = 2, H_l = 2 * dim_pe
 * for l < layers - 1 and H_{layers-1} = dim_pe (layers = 1: one 2 -> dim_pe Linear).
 *     u_ik = (s_k vec[i,k], val[i,k])                          NaN entries read as 0
 *     a^0 = relu(W_0 u + b_0),  a^l = relu(W_l a^{l-1} + b_l)
 *     out[i] = sum over the k with vec[i,k] not NaN of a^{layers-1}_ik        [N, dim_pe]; all NaN: zeros
 *   s_k = -1 iff flip != 0 and word 0 of philox4x32_10(seed, ctr = k) is >= 2^31, else +1: one sign per frequency
 *   column for the whole call, computed in the kernels from seed (no sign tensor).
 * hscn_lappe_fwd: ONE launch; a workgroup is four waves over the same hscn_lappe_tile() = 64 nodes, one node per lane,
 *   wave q taking the frequencies k = q, q + 4, ...; the parameters are staged in LDS and read as broadcasts, the chain
 *   stays in registers (widths are template parameters): no [N, K, H] tensor exists.  Every pre-activation starts at
 *   the bias and takes fmaf(input_i, W[o][i], .) for i ascending; a lane adds its frequencies in ascending k and wave 0
 *   adds the four waves' sums in wave order.  out[i] depends on row i of vec / val and the parameters alone: bitwise
 *   independent of N, of the row's place and of the grid.  out must be 16-byte aligned.
 * hscn_lappe_bwd: TWO launches; gradients for the parameters only (the statistics are constants).  g_params f32
 *   [sum_l (H_{l-1} + 1) H_l], flat in the order W_0, b_0, W_1, b_1, ... as the tensors are laid out.  The first launch
 *   recomputes the chain from vec, val and seed in the forward's order (the ReLU gates are the forward's) and stores
 *   one partial gradient per workgroup to workspace -- a workgroup walks a contiguous range of the N * K (node,
 *   frequency) samples, up to 256 per pass in sample order, parameters and activations of the pass in LDS -- and the
 *   second adds the partials in workgroup order in a fixed tree.  No float atomics: two runs give the same bits.
 *   workspace: hscn_lappe_workspace_floats(N, max_freqs, dim_pe, layers) floats (min(512, ceil(N K / 256)) partials),
 *   not initialised by the caller.
 * hscn_lappe_supported: 1 for 1 <= max_freqs <= 64, dim_pe a multiple of 4 in [4, 32], 1 <= layers <= 4.
 *   HSCN_E_BADARG for null pointers and negative N, HSCN_E_UNSUPPORTED where hscn_lappe_supported is 0,
 *   HSCN_E_WORKSPACE for a short workspace; all before any launch.  N = 0 launches nothing (g_params is then not
 *   written).  No host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_lappe_supported(int max_freqs, int dim_pe, int layers);
int hscn_lappe_tile(void);
int64_t hscn_lappe_workspace_floats(int64_t N, int max_freqs, int dim_pe, int layers);
int hscn_lappe_fwd(const float* vec, const float* val, const void* const* params_host, int64_t N, int max_freqs,
                   int dim_pe, int layers, int flip, uint64_t seed, float* out /*[N, dim_pe]*/, void* stream);
int hscn_lappe_bwd(const float* vec, const float* val, const float* g_out /*[N, dim_pe]*/,
                   const void* const* params_host, int64_t N, int max_freqs, int dim_pe, int layers, int flip,
                   uint64_t seed, float* g_params, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------- *
 * PNAConv's aggregate: mean / min / max / sum / std of a node's in-edge messages under degree scalers
 * (PyG PNAConv with towers = 1; csrc/pna.hip).  Purely additive to ABI 24.
 *
 * The message of edge k (j = src_k -> i = dst_k) is m_k = a[i] + b[j] + t[k]: a, b f32 [N, F], t f32 [E, F] in the
 * order of the edge list, or NULL (no edge features).  aggregators_host / scalers_host: HOST arrays of codes, each a
 * non-empty list without repeats, in the order of the output's column blocks:
 *     aggregators  0 mean, 1 min, 2 max, 3 sum, 4 std = sqrt(relu(mean(m^2) - mean(m)^2) + 1e-5)
 *     scalers      0 identity, 1 amplification log(d + 1) / avg_deg_log, 2 attenuation avg_deg_log / log(d + 1),
 *                  d = max(deg_i, 1); avg_deg_log is read (and must be finite and positive) only beside a code 1 or 2
 *     out[i, (s A + x) F + f] = scaler_s(i) * aggregator_x(i, f)                    f32 [N, S A F]
 *   A node without in-edges: 0 for mean, min, max and sum, sqrt(1e-5) for std.
 * hscn_pna_fwd: ONE launch over the target-keyed stable CSR.  A row is owned by a lane group (4 columns a lane where
 *   F % 4 == 0), reduces r_k = b[j] + t[k] in slot order and adds a[i] at the end (deg a[i] to sum, nothing to std).
 *   min / max ties go to the first slot in CSR order.  Rows of more than hscn_pna_long_row() slots are cut into
 *   chunks of hscn_pna_chunk() slots merged in chunk order (sums by a separately rounded add, min / max by comparison,
 *   the earlier chunk keeping a tie): a row's result depends on its own slots alone.  Optional outputs for the
 *   backward, each may be NULL: mean [N, F] (mean of r), stdv [N, F] (the std where the variance is positive, else 0),
 *   arg int32 [N, 2 F] (edge id of the argmin | argmax, -1 for an empty row).
 * hscn_pna_bwd_fold: ONE elementwise launch.  g_out f32 [N, S A F] -> gw f32 [N, 4, F] = {G_mean / deg + G_sum, G_min,
 *   G_max, [var > 0] G_std / (deg std)} (G_x: the cotangent of aggregator x with the scalers folded in; zeros for an
 *   empty row) and g_a [N, F] = G_mean + G_min + G_max + deg G_sum (may be NULL).  rowptr: the target-keyed CSR's; stdv:
 *   what the forward wrote (required with aggregator 4).
 *   Then, for edge k:  dm_k = gw0[i] + [k = argmin_i] gw1[i] + [k = argmax_i] gw2[i] + gw3[i] (r_k - mean_i).
 * hscn_pna_bwd_src: g_b [N, F], g_b[j] = sum of dm_k over the out-edges of j: ONE launch over the source-keyed stable
 *   CSR, slot order, long rows as in the forward.  mean may be NULL without aggregator 4, arg without 1 and 2.
 * hscn_pna_bwd_edge: g_t [E, F], g_t[k] = dm_k in edge order (edge_index int64 [2, E]); plain stores.
 *   No float atomics anywhere: two runs give the same bits.  flag: the relation's flag word; an edge with a node id
 *   outside [0, N) is in no CSR row, gets a zero row of g_t and raises bit 0; a foreign CSR entry raises bit 1.
 * hscn_pna_supported: 1 for 1 <= F <= 512, 1 <= num_aggregators <= 5, 1 <= num_scalers <= 3.
 *   HSCN_E_BADARG for null pointers (col / eid may be NULL when E == 0, t always), negative sizes, F < 1, a list that
 *   is empty, too long, repeats a code or holds an unknown one, or an avg_deg_log that is needed and not positive;
 *   HSCN_E_UNSUPPORTED for F > 512; both before any launch.  No workspace, no host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_pna_supported(int F, int num_aggregators, int num_scalers);
int hscn_pna_long_row(void);
int hscn_pna_chunk(void);
int hscn_pna_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* a, const float* b,
                 const float* t, float* out, float* mean, float* stdv, int32_t* arg, int64_t N, int64_t E, int F,
                 const int32_t* aggregators_host, int num_aggregators, const int32_t* scalers_host, int num_scalers,
                 float avg_deg_log, int32_t* flag /*[1]*/, void* stream);
int hscn_pna_bwd_fold(const int32_t* rowptr, const float* g_out, const float* stdv, float* gw, float* g_a, int64_t N,
                      int F, const int32_t* aggregators_host, int num_aggregators, const int32_t* scalers_host,
                      int num_scalers, float avg_deg_log, void* stream);
int hscn_pna_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const float* b,
                     const float* t, const float* gw, const float* mean, const int32_t* arg, float* g_b, int64_t N,
                     int64_t E, int F, int32_t* flag /*[1]*/, void* stream);
int hscn_pna_bwd_edge(const int64_t* edge_index, const float* b, const float* t, const float* gw, const float* mean,
                      const int32_t* arg, float* g_t, int64_t N, int64_t E, int F, int32_t* flag /*[1]*/,
                      void* stream);

/* ------------------------------------------------------------------------- *
 * SAN's attention over real and fake edges (csrc/san.hip).  Purely additive to ABI 24.
 *
 * q, k, v, q2, k2e f32 [N, HC] (HC = heads * head_dim = heads * C), e f32 [E, HC] in the order of the edge list, ptr32
 * int32 [B + 1] the graph boundaries, (rowptr, col, eid) the target-keyed stable CSR of the edge list
 * (hscn_csr_build), (rowptr_t, col_t, eid_t) the source-keyed one.  Per head, target i of graph g, scale = 1/sqrt(C):
 *     real  every listed edge x = (j -> i) with both ends in g, in CSR order:
 *             w_x   = a exp(clamp(scale sum_c q[i,c] (k[j,c] e[x,c]), -5, 5))
 *     fake  every node j of g, j = i included, without a listed edge j -> i, in key order:
 *             w2_ij = b exp(clamp(scale sum_c q2[i,c] k2e[j,c], -5, 5))
 *     a = 1 / (1 + gamma), b = gamma / (1 + gamma) (computed in double, rounded once)
 *     z[i] = sum w_x + sum w2_ij      out[i] = (sum w_x v[j] + sum w2_ij v[j]) / (z[i] + 1e-6)
 *   full_graph = 0: the real term alone with a = 1 (q2, k2e, dq2, dk2e NULL, gamma not read); a node without
 *   in-edges gets zeros.  The relation is directed.
 * hscn_san_attn_fwd: ONE launch, one wave per 64 rows of one (graph, head), a row per lane; the tile's adjacency is a
 *   bitset in LDS filled from the CSR, k2e and v stream through LDS in chunks of 32 rows.  Writes out [N, HC] and
 *   z [N, heads]; no weight, no [n, n] and no [E, heads] tensor exists.
 * hscn_san_attn_bwd_dst: ONE launch keyed by query: delta [N, heads] = sum_c g_out out (always), dq [N, HC], de [E, HC]
 *   (one writer per edge; rows of skipped edges are not written: hand in zeros), dq2 [N, HC]; each may be NULL.
 * hscn_san_attn_bwd_src: ONE launch keyed by key over the source-keyed CSR: dk, dv, dk2e [N, HC], each may be NULL
 *   (all NULL: nothing is launched).  The gradient through the clamp is zero outside (-5, 5).
 *   No float atomics, plain stores: two runs give the same bits, and a graph's rows have the same bits wherever the
 *   graph stands in the batch.
 * flag: bit 0 = a slot whose other end lies outside its row's graph or whose edge id lies outside [0, E): left out of
 *   the real term and of the bitset (the pair counts as fake); bit 1 = a graph with more than max_nodes nodes: NaN in
 *   all its rows of every output of the launch but de.
 * hscn_san_attn_supported: 1 for head_dim a multiple of 4 in [4, 64], heads >= 1, heads * head_dim <= 512 and
 *   0 <= max_nodes <= 4096 (the bitset row of a lane: ceil(max_nodes / 32) | 1 words, 32.3 KB a tile at 4096).
 *   HSCN_E_BADARG for null or misaligned (16 bytes) pointers, negative sizes, N or E beyond int32, and with
 *   full_graph a gamma that is negative or not finite; HSCN_E_UNSUPPORTED where hscn_san_attn_supported is 0; both
 *   before any launch.  N = 0 or B = 0 launches nothing.  No workspace, no host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_san_attn_supported(int heads, int head_dim, int max_nodes);
int hscn_san_attn_fwd(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* ptr32,
                      const float* q, const float* k, const float* v, const float* e, const float* q2,
                      const float* k2e, float* out /*[N, HC]*/, float* z /*[N, heads]*/, int64_t N, int64_t E,
                      int64_t B, int max_nodes, int heads, int head_dim, double gamma, int full_graph,
                      int32_t* flag /*[1]*/, void* stream);
int hscn_san_attn_bwd_dst(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const int32_t* ptr32,
                          const float* q, const float* k, const float* v, const float* e, const float* q2,
                          const float* k2e, const float* out, const float* z, const float* g_out,
                          float* delta /*[N, heads]*/, float* dq /*[N, HC]*/, float* de /*[E, HC]*/,
                          float* dq2 /*[N, HC]*/, int64_t N, int64_t E, int64_t B, int max_nodes, int heads,
                          int head_dim, double gamma, int full_graph, int32_t* flag /*[1]*/, void* stream);
int hscn_san_attn_bwd_src(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t, const int32_t* ptr32,
                          const float* q, const float* k, const float* v, const float* e, const float* q2,
                          const float* k2e, const float* z, const float* delta, const float* g_out,
                          float* dk /*[N, HC]*/, float* dv /*[N, HC]*/, float* dk2e /*[N, HC]*/, int64_t N, int64_t E,
                          int64_t B, int max_nodes, int heads, int head_dim, double gamma, int full_graph,
                          int32_t* flag /*[1]*/, void* stream);

/* ------------------------------------------------------------------------- *
 * GCNII's layer, PyG GCN2Conv (csrc/gcn2.hip).  Purely additive to ABI 24.
 *
 * x, x0, out, h f32 [N, H]; W1, W2 f32 [H, H] in PyG's layout (h @ W1, no transpose), W2 NULL = shared weights;
 * (rowptr, col) the target-keyed stable CSR of the edge list WITH one loop per node appended
 * (structure.self_loop_relation_of) and dinv f32 [N] its in-degree^-1/2 (hscn_gcn_dinv): unit edge weights, symmetric
 * normalisation, a graph's repeated edges count as often as they occur.  alpha in [0, 1], beta in (0, 1].
 *     p_i = sum over the row's CSR slots j of (dinv_i dinv_j) x_j      slot order, product and sum rounded separately
 *     W2 == NULL:  h = (1 - alpha) p + alpha x0,  y = (1 - beta) h + beta (h W1)                       saved: h
 *     else:        pa = (1 - alpha) p, xa = alpha x0,  y = (1 - beta) (pa + xa) + beta (pa W1 + xa W2)  saved: pa
 *     out = act(y)     act: HSCN_ACT_IDENTITY or HSCN_ACT_RELU
 * hscn_gcn2_fwd: ONE launch.  A workgroup owns a tile of rows (hscn_gcn2_plan: 32; 16 with two weights), gathers it
 *   into LDS, multiplies it by the weight on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per element) and writes
 *   out and the saved tile `h`; no other [N, H] value reaches memory.  The weight stays in LDS where tile and weight fit
 *   96 KB (H <= 128; H <= 96 with two weights); wider, it passes through LDS in column panels of 64 / 32 / 16 columns
 *   inside the same launch.
 * hscn_gcn2_bwd: ONE launch over gy = act'(out) g: gyb = beta gy [N, H] (the cotangent the weight gradients multiply),
 *   gp = (1 - alpha) ((1 - beta) gy + beta gy W1^T) [N, H] (whose gather over the source-keyed CSR,
 *   hscn_spmm_csr_gcn, is the gradient of x) and gx0 = alpha ((1 - beta) gy + beta gy Wx^T), Wx = W1 shared, W2 else;
 *   each may be NULL and is then not computed.
 * hscn_gcn2_bwd_w: gW1 [H, H] = h^T gyb and, with two weights, gW2 = alpha x0^T gyb, each through hscn_linear_bwd_w's
 *   ordered two-stage reduction (row chunks in row order, chunks folded in a fixed tree), either may be NULL.
 *   No float atomics: two runs give the same bits.
 * hscn_gcn2_supported: 1 for H a multiple of 4 in [4, 512].  hscn_gcn2_plan: plan[4] = {rows per tile of the forward,
 *   weight columns in LDS at a time, 1 if the weight stays in LDS, LDS bytes} (host arithmetic).
 *   HSCN_E_BADARG for null or misaligned (16 bytes) pointers, N negative or beyond int32, alpha or beta out of range;
 *   HSCN_E_UNSUPPORTED for a width outside the envelope or another act; both before any launch.  N = 0 launches
 *   nothing.  No host synchronisation.
 * ------------------------------------------------------------------------- */
int hscn_gcn2_supported(int H);
int hscn_gcn2_plan(int H, int two_weights, int32_t* plan /*[4]*/);
int hscn_gcn2_fwd(const int32_t* rowptr, const int32_t* col, const float* dinv, const float* x, const float* x0,
                  const float* W1, const float* W2, float* out /*[N, H]*/, float* h /*[N, H]*/, int64_t N, int H,
                  double alpha, double beta, int act, void* stream);
int hscn_gcn2_bwd(const float* g, const float* out, const float* W1, const float* W2, float* gyb /*[N, H]*/,
                  float* gp /*[N, H]*/, float* gx0 /*[N, H]*/, int64_t N, int H, double alpha, double beta, int act,
                  void* stream);
size_t hscn_gcn2_bwd_w_workspace_bytes(int64_t N, int H);
int hscn_gcn2_bwd_w(const float* gyb, const float* h, const float* x0, float* gW1 /*[H, H]*/, float* gW2 /*[H, H]*/,
                    int64_t N, int H, double alpha, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSCN_H */
