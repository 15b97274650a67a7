// Categorical encoders (OGB's AtomEncoder / BondEncoder): F integer columns, one embedding block per column in ONE
// table W [R, D], R = sum_c card_c, column c owning rows off_c .. off_c + card_c - 1;  idx is int64 [n, F], row-major.
//
//   forward     out[i] = ((0 + W[off_0 + idx[i,0]]) + W[off_1 + idx[i,1]]) + ...      separately rounded adds, column order
//   index       a stable counting sort of the n * F items by table row: rowptr [R + 1], item [n * F] = the node / edge
//               ids of every table row, ascending (a table row belongs to one column, so its items are distinct ids)
//   backward    dW[r] = sum over the row's slots of dOut[item[p]], in slot order
//
// Conventions of csrc/spmm.hip and csrc/gatedgcn.hip: a row of D floats is owned by LPR = min(D / 4, 64) consecutive
// lanes with 16-byte accesses; wider rows take further column passes.  No float atomics anywhere.
//
// The sort.  Each WAVE owns CATENC_SORT_CHUNK consecutive items (a "chunk"; four chunks per workgroup):
//   k_hist    the chunk's histogram over the R table rows in LDS (integer LDS atomics: a count has no order), stored
//             as hist[r][chunk];
//   k_scan    one wave per table row: exclusive scan of hist[r][.] over the chunks in place, the row's total aside;
//   k_rowptr  one workgroup: exclusive scan of the R totals = rowptr;
//   k_place   the chunk again, 64 items a round in item order: a lane's rank among the lanes of its round with the same
//             key comes from ballots over the key's bits, its slot is cursor[key] + rank, and the last lane of each key
//             advances the cursor.  Nothing depends on an arrival order.
// Work is O(n F + chunks R); the histograms take 4 R ints of LDS per workgroup (R <= 4096: 64 KB).
//
// The reduce.  A row of at most CATENC_LONG_ROW slots is one serial sum by one lane group.  A longer row is cut into
// chunks of CATENC_CHUNK slots counted from the ROW's first slot; each chunk is a serial sum from zero by one lane group
// (of any workgroup) stored as a partial, and a second launch adds a row's partials in chunk order.  So the bits of a
// row depend on the row's values in slot order alone: not on the launch geometry, not on where the row sits in the
// table or what else the batch holds.  Lane groups find their work without a host round trip: group g < R takes table
// row g (short rows; a long row is left to the chunks), group R + t takes the chunks that START in slots
// [t C, (t + 1) C) -- at most two, because a long row is longer than C: one of the row that holds slot t C, and the
// first chunk of the row that holds the tile's last slot.  Chunk k of row r is stored at partial rowptr[r] / C + r + k,
// which is unique and below ceil(n F / C) + R.
//
// An index outside [0, card_c) is never dereferenced: its term is skipped (forward), its item left out (index), and
// bit 0 of the flag word is set.  A slot whose id is outside [0, n), or a rowptr that leaves [0, n F], adds nothing
// and sets bit 1 (hscn_catenc_index_build never produces either).
#include "hscn_common.h"

namespace {

constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / HSCN_WAVE;
constexpr int CATENC_LONG_ROW = 128;     // rows with MORE slots than this are split (hscn_catenc_long_row)
constexpr int CATENC_CHUNK = 128;        // slots per chunk of a split row (hscn_catenc_chunk)
constexpr int CATENC_SORT_CHUNK = 512;   // items per wave of the counting sort (hscn_catenc_sort_chunk)
constexpr int CATENC_MAX_D = 512;
constexpr int CATENC_MAX_F = 16;
constexpr int CATENC_MAX_R = 4096;
static_assert(CATENC_LONG_ROW >= CATENC_CHUNK, "a tile of CATENC_CHUNK slots must hold at most two chunk starts");
static_assert(CATENC_SORT_CHUNK % HSCN_WAVE == 0, "a chunk is whole rounds of one wave");
static_assert((size_t)CE_WAVES * CATENC_MAX_R * sizeof(int) <= LDS_NO_OPT_IN_BYTES, "the histograms need no opt-in");

struct Cols {
  int F;
  int off[CATENC_MAX_F + 1];   // off[c] = first table row of column c; off[F] = R
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(add_rn(a.x, b.x), add_rn(a.y, b.y), add_rn(a.z, b.z), add_rn(a.w, b.w));
}

// ---- forward ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CE_THREADS) k_catenc_fwd(const float* __restrict__ W, const int64_t* __restrict__ idx,
                                                           const Cols C, float* __restrict__ out, int64_t n, int D,
                                                           int LPR, int RPB, int32_t* flag) {
  const int rl = threadIdx.x / LPR;
  const int lg = threadIdx.x - rl * LPR;
  if (rl >= RPB) return;                                  // (256 % LPR lanes at the end of the block own no row)
  const int span = LPR * 4;
  const int64_t tiles = (n + RPB - 1) / RPB;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * RPB + rl;
    if (i >= n) continue;
    const int64_t* row = idx + i * C.F;
    bool bad = false;
    for (int f = lg * 4; f < D; f += span) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int c = 0; c < C.F; ++c) {
        const int64_t v = row[c];
        const bool ok = v >= 0 && v < (int64_t)(C.off[c + 1] - C.off[c]);
        const float4 w = ld4(W + (size_t)(ok ? C.off[c] + (int)v : 0) * D + f);      // (row 0 exists: R >= 1)
        if (ok) acc = add4(acc, w);
        else bad = true;
      }
      st4(out + (size_t)i * D + f, acc);
    }
    if (bad && lg == 0) atomicOr(flag, 1);
  }
}

// ---- the counting sort ----------------------------------------------------------------------------------------------
// table row of item p (column p % F of node p / F), or -1 for an index outside its column
__device__ __forceinline__ int key_of(const int64_t* __restrict__ idx, const int* s_off, int F, int64_t p) {
  const int c = (int)(p % F);
  const int64_t v = idx[p];
  const int lo = s_off[c];
  return (v >= 0 && v < (int64_t)(s_off[c + 1] - lo)) ? lo + (int)v : -1;
}

extern __shared__ __attribute__((aligned(16))) int ce_smem[];      // [CE_WAVES][R] ints, then F + 1 column offsets

__global__ void __launch_bounds__(CE_THREADS) k_catenc_hist(const int64_t* __restrict__ idx, const Cols C, int64_t items,
                                                            int R, int chunks, int32_t* __restrict__ hist,
                                                            int32_t* flag) {
  int* s_off = ce_smem + CE_WAVES * R;
  for (int k = threadIdx.x; k < CE_WAVES * R; k += CE_THREADS) ce_smem[k] = 0;
  if (threadIdx.x <= C.F) s_off[threadIdx.x] = C.off[threadIdx.x];
  __syncthreads();
  const int wave = threadIdx.x / HSCN_WAVE, lane = threadIdx.x % HSCN_WAVE;
  const int ch = blockIdx.x * CE_WAVES + wave;
  int* h = ce_smem + wave * R;
  const int64_t base = (int64_t)ch * CATENC_SORT_CHUNK;
  bool bad = false;
  for (int rd = 0; rd < CATENC_SORT_CHUNK / HSCN_WAVE; ++rd) {
    const int64_t p = base + rd * HSCN_WAVE + lane;
    if (p < items) {
      const int key = key_of(idx, s_off, C.F, p);
      if (key >= 0) atomicAdd(&h[key], 1);
      else bad = true;
    }
  }
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  if (ch < chunks)
    for (int r = lane; r < R; r += HSCN_WAVE) hist[(size_t)r * chunks + ch] = h[r];
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < HSCN_WAVE; o <<= 1) {
    const int u = __shfl_up(v, o, HSCN_WAVE);
    if (lane >= o) v += u;
  }
  return v;
}

// one wave per table row: hist[r][.] becomes its exclusive scan over the chunks, total[r] the row's length
__global__ void __launch_bounds__(CE_THREADS) k_catenc_scan(int32_t* __restrict__ hist, int32_t* __restrict__ total,
                                                            int R, int chunks) {
  const int wave = threadIdx.x / HSCN_WAVE, lane = threadIdx.x % HSCN_WAVE;
  const int r = blockIdx.x * CE_WAVES + wave;
  if (r >= R) return;
  int32_t* h = hist + (size_t)r * chunks;
  int carry = 0;
  for (int t = 0; t < chunks; t += HSCN_WAVE) {
    const int v = t + lane < chunks ? h[t + lane] : 0;
    const int inc = wave_inclusive_scan(v, lane);
    if (t + lane < chunks) h[t + lane] = carry + inc - v;
    carry += __shfl(inc, HSCN_WAVE - 1, HSCN_WAVE);
  }
  if (lane == 0) total[r] = carry;
}

// one workgroup: rowptr = exclusive scan of the R <= CATENC_MAX_R totals (a contiguous run of rows per thread)
__global__ void __launch_bounds__(CE_THREADS) k_catenc_rowptr(const int32_t* __restrict__ total,
                                                              int32_t* __restrict__ rowptr, int R) {
  __shared__ int wsum[CE_WAVES];
  const int per = (R + CE_THREADS - 1) / CE_THREADS;
  const int lo = threadIdx.x * per, hi = lo + per < R ? lo + per : R;
  int s = 0;
  for (int r = lo; r < hi; ++r) s += total[r];
  const int wave = threadIdx.x / HSCN_WAVE, lane = threadIdx.x % HSCN_WAVE;
  const int inc = wave_inclusive_scan(s, lane);
  if (lane == HSCN_WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  int run = inc - s;
  for (int w = 0; w < wave; ++w) run += wsum[w];
  for (int r = lo; r < hi; ++r) {
    rowptr[r] = run;
    run += total[r];
  }
  if (threadIdx.x == CE_THREADS - 1) rowptr[R] = run;     // (threads past the last row carry the grand total)
}

__global__ void __launch_bounds__(CE_THREADS) k_catenc_place(const int64_t* __restrict__ idx, const Cols C, int64_t items,
                                                             int R, int chunks, int nbits,
                                                             const int32_t* __restrict__ hist,
                                                             const int32_t* __restrict__ rowptr,
                                                             int32_t* __restrict__ item) {
  int* s_off = ce_smem + CE_WAVES * R;
  const int wave = threadIdx.x / HSCN_WAVE, lane = threadIdx.x % HSCN_WAVE;
  const int ch = blockIdx.x * CE_WAVES + wave;
  int* cur = ce_smem + wave * R;
  if (ch < chunks)
    for (int r = lane; r < R; r += HSCN_WAVE) cur[r] = rowptr[r] + hist[(size_t)r * chunks + ch];
  if (threadIdx.x <= C.F) s_off[threadIdx.x] = C.off[threadIdx.x];
  __syncthreads();
  const int64_t base = (int64_t)ch * CATENC_SORT_CHUNK;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int rd = 0; rd < CATENC_SORT_CHUNK / HSCN_WAVE; ++rd) {          // (uniform over the workgroup: barriers inside)
    const int64_t p = base + rd * HSCN_WAVE + lane;
    const int key = p < items ? key_of(idx, s_off, C.F, p) : -1;
    const bool ok = key >= 0;
    unsigned long long same = __ballot(ok);                            // lanes of this round with this lane's key
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (key >> b) & 1;
      const unsigned long long set = __ballot(bit);
      same &= bit ? set : ~set;
    }
    const int rank = __popcll(same & below), cnt = __popcll(same);
    if (ok) {
      const int64_t pos = (int64_t)cur[key] + rank;
      if (pos >= 0 && pos < items) item[pos] = (int32_t)(p / C.F);
    }
    __syncthreads();
    if (ok && rank == cnt - 1) cur[key] += cnt;
    __syncthreads();
  }
}

// ---- the segment reduce ---------------------------------------------------------------------------------------------
struct BwdArgs {
  const int32_t* rowptr;   // [R + 1]
  const int32_t* item;     // [items]
  const float* g;          // dOut [n, D]
  float* dW;               // [R, D]
  float* part;             // [tiles + R, D] chunk partials of the long rows
  int64_t n, items, tiles;
  int R, D, LPR, RPB;
  int32_t* flag;
};

// slots [s, t) in slot order, columns [f, f + 4), from zero.  The walk is latency-bound (an id, then the row it names),
// so CE_AHEAD ids and then CE_AHEAD rows are in flight before the ordered adds; a foreign id reads row 0 and adds +0.
constexpr int CE_AHEAD = 8;

__device__ __forceinline__ float4 sum_slots(const BwdArgs& A, int s, int t, int f) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* __restrict__ g = A.g + f;
  const int32_t* __restrict__ item = A.item;
  const uint32_t n = (uint32_t)A.n;                       // (n <= INT32_MAX; a negative id compares as a large one)
  bool bad = false;
  int p = s;
  for (; p + CE_AHEAD <= t; p += CE_AHEAD) {
    uint32_t j[CE_AHEAD];
    float4 v[CE_AHEAD];
#pragma unroll
    for (int u = 0; u < CE_AHEAD; ++u) j[u] = (uint32_t)item[p + u];
#pragma unroll
    for (int u = 0; u < CE_AHEAD; ++u) v[u] = ld4(g + (size_t)(j[u] < n ? j[u] : 0u) * A.D);
#pragma unroll
    for (int u = 0; u < CE_AHEAD; ++u) {
      const bool ok = j[u] < n;                           // (selects, not a branch: the loads above stay together)
      bad |= !ok;
      acc = add4(acc, make_float4(ok ? v[u].x : 0.f, ok ? v[u].y : 0.f, ok ? v[u].z : 0.f, ok ? v[u].w : 0.f));
    }
  }
  for (; p < t; ++p) {
    const uint32_t j = (uint32_t)item[p];
    const bool ok = j < n;
    const float4 v = ld4(g + (size_t)(ok ? j : 0u) * A.D);
    bad |= !ok;
    acc = add4(acc, make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f));
  }
  if (bad) atomicOr(A.flag, 2);
  return acc;
}

// the slots [s, e) of table row r, or false (and bit 1) for a rowptr that is not one of this index
__device__ __forceinline__ bool row_range(const BwdArgs& A, int r, int& s, int& e) {
  s = A.rowptr[r], e = A.rowptr[r + 1];
  if (s < 0 || e < s || e > A.items) {
    atomicOr(A.flag, 2);
    return false;
  }
  return true;
}

__device__ __forceinline__ void store_chunk(const BwdArgs& A, int r, int s, int e, int k, int f0, int span) {
  const int64_t q = (int64_t)(s / CATENC_CHUNK) + r + k;
  if (q >= A.tiles + A.R) {
    atomicOr(A.flag, 2);
    return;
  }
  const int cs = s + k * CATENC_CHUNK;
  const int ct = cs + CATENC_CHUNK < e ? cs + CATENC_CHUNK : e;
  for (int f = f0; f < A.D; f += span) st4(A.part + (size_t)q * A.D + f, sum_slots(A, cs, ct, f));
}

__global__ void __launch_bounds__(CE_THREADS) k_catenc_bwd(const BwdArgs A) {
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  if (rl >= A.RPB) return;
  const int span = A.LPR * 4, f0 = lg * 4;
  const int64_t groups = A.R + A.tiles;
  for (int64_t G = (int64_t)blockIdx.x * A.RPB + rl; G < groups; G += (int64_t)gridDim.x * A.RPB) {
    if (G < A.R) {                                        // a table row of at most CATENC_LONG_ROW slots
      const int r = (int)G;
      int s, e;
      if (!row_range(A, r, s, e)) e = s = 0;
      if (e - s > CATENC_LONG_ROW) continue;
      for (int f = f0; f < A.D; f += span) st4(A.dW + (size_t)r * A.D + f, sum_slots(A, s, e, f));
      continue;
    }
    // the chunks of long rows that start in slots [a, b)
    const int total = A.rowptr[A.R];
    const int64_t a64 = (G - A.R) * CATENC_CHUNK;
    if (total < 0 || total > A.items || a64 >= total) continue;
    const int a = (int)a64;
    const int b = a + CATENC_CHUNK < total ? a + CATENC_CHUNK : total;
    int r1 = 0, r2 = 0;
    for (int pass = 0; pass < 2; ++pass) {                // the rows that hold slot a and slot b - 1
      const int want = pass == 0 ? a : b - 1;
      int lo = 0, hi = A.R;                               // rowptr[lo] <= want < rowptr[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.rowptr[mid] <= want) lo = mid;
        else hi = mid;
      }
      (pass == 0 ? r1 : r2) = lo;
    }
    int s, e;
    if (row_range(A, r1, s, e) && e - s > CATENC_LONG_ROW && s <= a) {
      const int k = (a - s + CATENC_CHUNK - 1) / CATENC_CHUNK;
      const int64_t st = (int64_t)s + (int64_t)k * CATENC_CHUNK;
      if (st < b && st < e) store_chunk(A, r1, s, e, k, f0, span);
    }
    if (r2 != r1 && row_range(A, r2, s, e) && e - s > CATENC_LONG_ROW && s > a && s < b)
      store_chunk(A, r2, s, e, 0, f0, span);
  }
}

// the long rows: their partials added in chunk order
__global__ void __launch_bounds__(CE_THREADS) k_catenc_bwd_combine(const BwdArgs A) {
  const int rl = threadIdx.x / A.LPR;
  const int lg = threadIdx.x - rl * A.LPR;
  if (rl >= A.RPB) return;
  const int span = A.LPR * 4;
  for (int64_t G = (int64_t)blockIdx.x * A.RPB + rl; G < A.R; G += (int64_t)gridDim.x * A.RPB) {
    const int r = (int)G;
    const int s = A.rowptr[r], e = A.rowptr[r + 1];
    if (s < 0 || e < s || e > A.items || e - s <= CATENC_LONG_ROW) continue;
    const int chunks = (e - s + CATENC_CHUNK - 1) / CATENC_CHUNK;
    const int64_t q0 = (int64_t)(s / CATENC_CHUNK) + r;
    for (int f = lg * 4; f < A.D; f += span) {
      float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q0 + chunks <= A.tiles + A.R) {
#pragma unroll 8
        for (int k = 0; k < chunks; ++k) tot = add4(tot, ld4(A.part + (size_t)(q0 + k) * A.D + f));
      }
      st4(A.dW + (size_t)r * A.D + f, tot);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
bool catenc_supported(int D, int F, int R) {
  return D >= 4 && D <= CATENC_MAX_D && D % 4 == 0 && F >= 1 && F <= CATENC_MAX_F && R >= F && R <= CATENC_MAX_R;
}

// `card` [F] on the host -> the column offsets; HSCN_E_BADARG for an empty column, HSCN_E_UNSUPPORTED outside the envelope
int make_cols(const int32_t* card, int F, int D, Cols& C) {
  if (F < 1 || D < 1) return HSCN_E_BADARG;
  if (F > CATENC_MAX_F) return HSCN_E_UNSUPPORTED;
  if (!card) return HSCN_E_BADARG;
  C.F = F;
  int64_t R = 0;
  for (int c = 0; c < F; ++c) {
    if (card[c] < 1) return HSCN_E_BADARG;
    C.off[c] = (int)R;
    R += card[c];
    if (R > CATENC_MAX_R) return HSCN_E_UNSUPPORTED;
  }
  for (int c = F; c <= CATENC_MAX_F; ++c) C.off[c] = (int)R;
  return catenc_supported(D, F, (int)R) ? 0 : HSCN_E_UNSUPPORTED;
}

void lane_groups(int D, int& LPR, int& RPB) {
  LPR = D / 4 < HSCN_WAVE ? D / 4 : HSCN_WAVE;
  RPB = CE_THREADS / LPR;
}

int64_t sort_chunks(int64_t items) { return (items + CATENC_SORT_CHUNK - 1) / CATENC_SORT_CHUNK; }
int64_t reduce_tiles(int64_t items) { return (items + CATENC_CHUNK - 1) / CATENC_CHUNK; }
size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int hscn_catenc_supported(int D, int F, int R) { return catenc_supported(D, F, R) ? 1 : 0; }
int hscn_catenc_long_row(void) { return CATENC_LONG_ROW; }
int hscn_catenc_chunk(void) { return CATENC_CHUNK; }
int hscn_catenc_sort_chunk(void) { return CATENC_SORT_CHUNK; }

int hscn_catenc_fwd(const float* W, const int64_t* idx, const int32_t* card_host, float* out, int64_t n, int F, int D,
                    int32_t* flag, void* stream_) {
  if (n < 0) return HSCN_E_BADARG;
  Cols C{};
  if (int rc = make_cols(card_host, F, D, C)) return rc;
  if (n > INT32_MAX / F) return HSCN_E_BADARG;            // items are int32
  if (n == 0) return 0;
  if (!W || !idx || !out || !flag) return HSCN_E_BADARG;
  int LPR, RPB;
  lane_groups(D, LPR, RPB);
  int64_t nb = (n + RPB - 1) / RPB;
  if (nb > 65536) nb = 65536;
  k_catenc_fwd<<<(unsigned)nb, CE_THREADS, 0, hscn_stream(stream_)>>>(W, idx, C, out, n, D, LPR, RPB, flag);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

size_t hscn_catenc_index_workspace_bytes(int64_t n, int F, int R) {
  if (n < 0 || F < 1 || R < 1 || n > INT32_MAX / F) return 0;
  const int64_t chunks = sort_chunks(n * F);
  return align16((size_t)R * (size_t)chunks * sizeof(int32_t)) + align16((size_t)R * sizeof(int32_t));
}

int hscn_catenc_index_build(const int64_t* idx, const int32_t* card_host, int64_t n, int F, int32_t* rowptr,
                            int32_t* item, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream_) {
  if (n < 0) return HSCN_E_BADARG;
  Cols C{};
  if (int rc = make_cols(card_host, F, 4, C)) return rc;
  if (n > INT32_MAX / F) return HSCN_E_BADARG;
  const int R = C.off[F];
  if (!rowptr || !flag) return HSCN_E_BADARG;
  hipStream_t st = hscn_stream(stream_);
  const int64_t items = n * F;
  if (items == 0) {
    if (hipMemsetAsync(rowptr, 0, (size_t)(R + 1) * sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
    return 0;
  }
  if (!idx || !item || !workspace) return HSCN_E_BADARG;
  if (workspace_bytes < hscn_catenc_index_workspace_bytes(n, F, R)) return HSCN_E_WORKSPACE;
  const int chunks = (int)sort_chunks(items);
  int32_t* hist = static_cast<int32_t*>(workspace);
  int32_t* total = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) +
                                              align16((size_t)R * (size_t)chunks * sizeof(int32_t)));
  int nbits = 0;
  while ((1 << nbits) < R) ++nbits;
  const unsigned nb = hscn_blocks(chunks, CE_WAVES);
  const size_t lds = ((size_t)CE_WAVES * R + CATENC_MAX_F + 1) * sizeof(int);
  if (int rc = launch_with_lds(k_catenc_hist, nb, CE_THREADS, lds, st, idx, C, items, R, chunks, hist, flag)) return rc;
  k_catenc_scan<<<hscn_blocks(R, CE_WAVES), CE_THREADS, 0, st>>>(hist, total, R, chunks);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  k_catenc_rowptr<<<1, CE_THREADS, 0, st>>>(total, rowptr, R);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return launch_with_lds(k_catenc_place, nb, CE_THREADS, lds, st, idx, C, items, R, chunks, nbits,
                         (const int32_t*)hist, (const int32_t*)rowptr, item);
}

size_t hscn_catenc_bwd_workspace_bytes(int64_t n, int F, int R, int D) {
  if (n < 0 || F < 1 || R < 1 || D < 1 || n > INT32_MAX / F) return 0;
  return (size_t)(reduce_tiles(n * F) + R) * (size_t)D * sizeof(float);
}

int hscn_catenc_bwd(const int32_t* rowptr, const int32_t* item, const float* dOut, float* dW, int64_t n, int F, int R,
                    int D, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream_) {
  if (n < 0 || F < 1 || R < 1 || D < 1) return HSCN_E_BADARG;
  if (!catenc_supported(D, F, R)) return HSCN_E_UNSUPPORTED;
  if (n > INT32_MAX / F) return HSCN_E_BADARG;
  const int64_t items = n * F;
  if (!rowptr || !dW || !flag || !workspace) return HSCN_E_BADARG;
  if (items > 0 && (!item || !dOut)) return HSCN_E_BADARG;
  if (workspace_bytes < hscn_catenc_bwd_workspace_bytes(n, F, R, D)) return HSCN_E_WORKSPACE;
  BwdArgs A{};
  A.rowptr = rowptr, A.item = item, A.g = dOut, A.dW = dW, A.part = static_cast<float*>(workspace);
  A.n = n, A.items = items, A.tiles = reduce_tiles(items);
  A.R = R, A.D = D, A.flag = flag;
  lane_groups(D, A.LPR, A.RPB);
  hipStream_t st = hscn_stream(stream_);
  k_catenc_bwd<<<hscn_blocks(A.R + A.tiles, A.RPB), CE_THREADS, 0, st>>>(A);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  k_catenc_bwd_combine<<<hscn_blocks(A.R, A.RPB), CE_THREADS, 0, st>>>(A);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
