// What the row-walk kernels share: k_gine_walk (gine.hip), k_gated_walk (gatedgcn.hip), k_edge_attn
// (edge_attention.hip) and the two GAT families (gat.hip, gat_loops.hip).  The long-row scheme of the first three is
// described here once, with its two constants; below it, the small device helpers and the host-side launch geometry.
//
// Geometry: a row (edge attention: a (row, head) pair) is owned by a group of consecutive lanes, a workgroup holds
// several groups and grid-strides over tiles of that many rows.
// Short rows: every lane group walks the slots of its row serially, in CSR slot order.
// Long rows: a hub of thousands of edges would hold its wave while every other row is done, so rows of MORE than
// ROW_WALK_LONG_ROW slots are left out of the serial walk and taken by the WHOLE workgroup afterwards: the row is cut
// into chunks of ROW_WALK_CHUNK slots, the lane groups walk one chunk each (slot order, from a cleared accumulator) and
// park their partials in LDS, and lane group 0 merges them in chunk order (a separately rounded add, or the online
// softmax's rescale) and finishes the row.  A row of more chunks than lane groups takes further rounds, merged into
// the same total in order.
// Reproducibility: which rows are split, where the chunks are cut and the order of the merge depend on the row's slot
// count alone -- not on the grid, the lane groups per workgroup or the rows that share a tile -- so a row's result is
// the same bits wherever it stands in a batch.
// Barriers: every thread of the workgroup reaches __syncthreads_or and, for a long row, both barriers of every round,
// whatever its membership: the loops around them run over workgroup-uniform values only (the tile, the row's index
// in the tile, rowptr of that row, the pass, the round), and everything lane-dependent (member, live, c < chunks,
// lane group 0) is tested inside them.
//
// Each of the three kernels, and k_exph_attn (exphormer.hip) as the fourth, spells this skeleton itself: as one inlined
// function template the same statements reach the backend in another order, and it then allocates
// k_gine_walk<4, 4, 1> 73 VGPRs instead of 71, one occupancy step less (profiles/row_walk_driver_resources.txt).
// What k_edge_attn and k_exph_attn do share is the head-unit layer at the end of this file: the constants, the column
// helpers and the lane layout of a (row, head) unit (profiles/head_walk_resources.txt: all their kernels unchanged).
// csrc/catenc.hip has a LONG_ROW / CHUNK pair of its own for a different scheme (a second combine kernel, a look-ahead
// window).
#pragma once
#include "hscn_common.h"
#include <initializer_list>
#include <math.h>
#include <type_traits>

constexpr int ROW_WALK_LONG_ROW = 256;   // rows with MORE slots than this are split (hscn_*_long_row)
constexpr int ROW_WALK_CHUNK = 64;       // slots per chunk of a split row (hscn_*_chunk)

// ---- device helpers shared with gat.hip and gat_loops.hip ---------------------------------------------------------
__device__ __forceinline__ float rw_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// VEC columns between memory and a lane's array, through GV<VEC> (16 bytes at once for VEC = 4)
template <int VEC>
__device__ __forceinline__ void rw_load(const float* p, float (&v)[VEC]) {
  const typename GV<VEC>::T t = GV<VEC>::load(p);
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k] = GV<VEC>::get(t, k);
}
template <int VEC>
__device__ __forceinline__ void rw_store(float* p, const float (&v)[VEC]) { GV<VEC>::store(p, GV<VEC>::make(v)); }

template <int VEC>
__device__ __forceinline__ float rw_dot(const float (&a)[VEC], const float (&b)[VEC]) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < VEC; ++k) d = fmaf(a[k], b[k], d);
  return d;
}

// ---- launch geometry (host) ---------------------------------------------------------------------------------------
// every count that indexes a CSR is a non-negative int32
static inline bool check_csr_sizes(std::initializer_list<int64_t> counts) {
  for (int64_t n : counts)
    if (n < 0 || n > INT32_MAX) return false;
  return true;
}

// lanes of a group for `need` lanes' worth of columns: the power of two >= need; past a wave 64 if `clamp`, else 0
static inline int pow2_lanes(int need, bool clamp) {
  int G = 1;
  while (G < need && G < HSCN_WAVE) G <<= 1;
  return G >= need || clamp ? G : 0;
}

// the lane layout of gine.hip and gatedgcn.hip: VEC = 4 where the width allows, a lane per VEC columns up to a wave
static inline void lane_groups(int width, int threads, int& VEC, int& LPR, int& RPB) {
  VEC = (width % 4 == 0) ? 4 : 1;
  LPR = (width + VEC - 1) / VEC;
  if (LPR > HSCN_WAVE) LPR = HSCN_WAVE;
  RPB = threads / LPR;
}

// workgroups for `work` items at `per_block` each, at most `cap` (the kernels grid-stride)
static inline unsigned capped_grid(int64_t work, int per_block, int64_t cap) {
  const int64_t nb = (work + per_block - 1) / per_block;
  return (unsigned)(nb > cap ? cap : nb);
}

// f(std::integral_constant<int, VEC>) for VEC = 4 or 1: the VEC ladder of every entry point
template <class F>
static inline void dispatch_vec(int VEC, F&& f) {
  if (VEC == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 1>{});
}

// ---- the head-unit layer: a (row, head) unit walked by a lane group (edge_attention.hip, exphormer.hip) -----------
// One (row, head) is owned by G consecutive lanes (G a power of two, at most 64), VEC = 4 columns per lane and pass
// (16-byte accesses) where C % 4 == 0 and every pointer is 16-byte aligned, VEC = 1 otherwise; a head wider than
// G * VEC takes NP <= HEAD_NC / VEC passes, all of them held in registers.
constexpr int HEAD_THREADS = 256;
constexpr int HEAD_MAX_WIDTH = 512;  // heads * head_dim
constexpr int HEAD_NC = 8;           // floats a lane holds of one operand row: (8 / VEC) passes of VEC columns

// pass p gives lane lg of a group the columns [c, c + VEC), c = (p * G + lg) * VEC; only p < NP is visited and a lane
// with c >= C idles (C % VEC == 0, so a vector never straddles the end of a head)
template <int VEC>
__device__ __forceinline__ void rw_load_cols(int G, int NP, int C, const float* row, int lg, float (&x)[HEAD_NC]) {
  using V = GV<VEC>;
#pragma unroll
  for (int i = 0; i < HEAD_NC; ++i) x[i] = 0.f;
#pragma unroll
  for (int p = 0; p < HEAD_NC / VEC; ++p) {
    const int c = (p * G + lg) * VEC;
    if (p < NP && c < C) {
      const typename V::T t = V::load(row + c);
#pragma unroll
      for (int u = 0; u < VEC; ++u) x[p * VEC + u] = V::get(t, u);
    }
  }
}

template <int VEC>
__device__ __forceinline__ void rw_store_cols(int G, int NP, int C, float* row, int lg, const float (&x)[HEAD_NC]) {
  using V = GV<VEC>;
#pragma unroll
  for (int p = 0; p < HEAD_NC / VEC; ++p) {
    const int c = (p * G + lg) * VEC;
    if (p < NP && c < C) V::store(row + c, V::make(&x[p * VEC]));
  }
}

__device__ __forceinline__ float rw_dot8(const float (&a)[HEAD_NC], const float (&b)[HEAD_NC]) {
  float s = 0.f;                     // (columns a lane does not own hold zeros)
#pragma unroll
  for (int i = 0; i < HEAD_NC; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// the envelope of both operators (hscn_edge_attn_supported, hscn_exph_attn_supported)
static inline bool head_walk_supported(int heads, int head_dim) {
  return heads >= 1 && head_dim >= 1 && (int64_t)heads * head_dim <= HEAD_MAX_WIDTH;
}

// VEC, G, UPB, NP for a head of width C: `ptrs` are the float tensors the launch touches (NULL counts as aligned)
static inline int lane_layout(int C, std::initializer_list<const void*> ptrs, int& G, int& UPB, int& NP) {
  bool vec = C % 4 == 0;
  for (const void* p : ptrs) vec = vec && aligned16(p);
  const int VEC = vec ? 4 : 1;
  const int need = (C + VEC - 1) / VEC;                  // lanes a head asks for
  G = pow2_lanes(need, true);
  UPB = HEAD_THREADS / G;
  NP = (need + G - 1) / G;                               // <= 2 (VEC = 4), <= 8 (VEC = 1) for C <= 512
  return VEC;
}

// the logits' scale 1 / sqrt(C)
static inline float head_scale(int head_dim) { return 1.0f / sqrtf((float)head_dim); }
