// All-pairs shortest-path buckets per graph of a collated batch (Graphormer's spatial encoding, the index of the
// attention bias of csrc/attention.hip).
//
//   d(i, j) = the fewest edges on a directed path i -> j inside graph g (edge_index = [source; target]), d(i, i) = 0;
//   bucket(i, j) = d(i, j) where d(i, j) < max_dist, max_dist otherwise ("farther" and "unreachable" alike):
//   max_dist + 1 values, one uint8 each, row-major [n_g, n_g] (row = query, column = key) at bucket + spd_ptr[g].
//
// Work split: ONE workgroup per graph.  Three bitset matrices of n rows x W = ceil(n / 32) words live in LDS:
//   adj  bit j of row i: an edge i -> j                               (LDS integer atomicOr while the edges are read)
//   cur  bit j of row i: d(i, j) <= k - 1                             (starts as the identity)
//   nxt  cur[i] | OR over the successors s of i of cur[s]:  d(i, j) <= k
// One item = one word (i, w): it walks the set bits of adj[i] and ORs the same word w of those rows, so a level costs
// E W word operations whatever the frontier; the bits that are new in nxt are the pairs at distance exactly k, and the
// item writes k to their bytes.  Levels k = 1 .. max_dist - 1, or until a level finds nothing new anywhere.
// The matrix is first filled with max_dist by the whole workgroup (dword stores between the unaligned ends), a barrier
// later the diagonal and the levels overwrite single bytes: every byte is written at most once after the fill.
//
// LDS: 3 * max_nodes * ceil(max_nodes / 32) * 4 bytes of dynamic LDS (96 KB at 512 nodes) asked through
// launch_with_lds, beside SPD_STATIC_LDS = 1 KB kept for the kernel's own static words (the barrier's vote);
// hscn_spd_supported: the two within a CU's 160 KB, up to 646 nodes.  The result is integers: the same on every run, wherever the graph stands in the batch.
//
// Flag word (only ever OR-ed): bit 0 = an edge with an end outside its graph (skipped); bit 1 = a graph with more than
// max_nodes nodes (its buckets are all max_dist), or one whose [spd_ptr[g], spd_ptr[g] + n^2) leaves the bucket
// tensor (nothing of it is written).
#include "hscn_common.h"

namespace {

constexpr int SPD_THREADS = 512;
constexpr int SPD_MIN_DIST = 1, SPD_MAX_DIST = 63;
constexpr int SPD_FLAG_BAD_EDGE = 1;      // bit 0
constexpr int SPD_FLAG_OVERFLOW = 2;      // bit 1
constexpr size_t SPD_STATIC_LDS = 1024;   // room for what the kernel declares beside its dynamic LDS

struct SpdArgs {
  const int64_t* ei;     // [2, E]
  const int32_t* ptr;    // [B + 1]
  const int32_t* eptr;   // [B + 1]
  const int64_t* sptr;   // [B + 1]
  uint8_t* bucket;       // [total]
  int64_t N, E, total;
  int max_nodes, max_dist;
  int32_t* flag;
};

size_t spd_lds_bytes(int max_nodes) {
  const size_t n = max_nodes < 1 ? 1 : (size_t)max_nodes;
  return 3 * n * ((n + 31) / 32) * sizeof(uint32_t);
}

bool spd_supported(int max_nodes, int max_dist) {
  return max_nodes >= 0 && max_dist >= SPD_MIN_DIST && max_dist <= SPD_MAX_DIST &&
         spd_lds_bytes(max_nodes) + SPD_STATIC_LDS <= LDS_CU_BYTES;
}

// p[0, count) := v by the whole workgroup: dword stores between the ends that are not 4-byte aligned
__device__ __forceinline__ void fill_bytes(uint8_t* p, int64_t count, uint8_t v) {
  int64_t head = (int64_t)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3);
  if (head > count) head = count;
  const int64_t words = (count - head) >> 2;
  uint32_t* w = reinterpret_cast<uint32_t*>(p + head);
  const uint32_t vv = (uint32_t)v * 0x01010101u;
  for (int64_t k = threadIdx.x; k < head; k += SPD_THREADS) p[k] = v;
  for (int64_t k = threadIdx.x; k < words; k += SPD_THREADS) w[k] = vv;
  for (int64_t k = head + (words << 2) + threadIdx.x; k < count; k += SPD_THREADS) p[k] = v;
}

__global__ void __launch_bounds__(SPD_THREADS) k_spd(const SpdArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t spd_lds[];
  const int g = blockIdx.x;
  int64_t a = A.ptr[g], b = A.ptr[g + 1];
  a = a < 0 ? 0 : (a > A.N ? A.N : a);
  b = b < a ? a : (b > A.N ? A.N : b);
  const int n = (int)(b - a);
  if (n == 0) return;
  const int64_t base = A.sptr[g], nn = (int64_t)n * n;
  if (base < 0 || nn > A.total || base > A.total - nn) {          // workgroup-uniform: nowhere to write
    if (threadIdx.x == 0) atomicOr(A.flag, SPD_FLAG_OVERFLOW);
    return;
  }
  uint8_t* out = A.bucket + base;
  fill_bytes(out, nn, (uint8_t)A.max_dist);
  if (n > A.max_nodes) {                                          // the LDS was sized for max_nodes
    if (threadIdx.x == 0) atomicOr(A.flag, SPD_FLAG_OVERFLOW);
    return;
  }
  const int W = (n + 31) >> 5, words = n * W;
  uint32_t* adj = spd_lds;
  uint32_t* cur = adj + words;
  uint32_t* nxt = cur + words;
  for (int it = threadIdx.x; it < words; it += SPD_THREADS) {
    const int i = it / W, w = it - i * W;
    adj[it] = 0u;
    cur[it] = (i >> 5) == w ? 1u << (i & 31) : 0u;
  }
  __syncthreads();
  int64_t e0 = A.eptr[g], e1 = A.eptr[g + 1];
  e0 = e0 < 0 ? 0 : (e0 > A.E ? A.E : e0);
  e1 = e1 < e0 ? e0 : (e1 > A.E ? A.E : e1);
  bool bad = false;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += SPD_THREADS) {
    const int64_t s = A.ei[e] - a, t = A.ei[A.E + e] - a;
    if (s < 0 || s >= n || t < 0 || t >= n) bad = true;
    else atomicOr(&adj[(int)s * W + (int)(t >> 5)], 1u << (int)(t & 31));
  }
  if (bad) atomicOr(A.flag, SPD_FLAG_BAD_EDGE);
  __syncthreads();                                                // adj is whole; the fill lies before the byte stores
  for (int i = threadIdx.x; i < n; i += SPD_THREADS) out[(int64_t)i * n + i] = 0;
  for (int k = 1; k < A.max_dist; ++k) {
    int any = 0;
    for (int it = threadIdx.x; it < words; it += SPD_THREADS) {
      const int i = it / W, w = it - i * W;
      const uint32_t old = cur[it];
      uint32_t r = old;
      for (int aw = 0; aw < W; ++aw) {
        uint32_t bits = adj[i * W + aw];
        while (bits) {
          const int s = (aw << 5) + __ffs((int)bits) - 1;
          bits &= bits - 1;
          r |= cur[s * W + w];
        }
      }
      nxt[it] = r;
      uint32_t fresh = r & ~old;                                  // columns j of word w with d(i, j) == k
      any |= fresh != 0u;
      uint8_t* row = out + (int64_t)i * n + (w << 5);
      while (fresh) {
        const int c = __ffs((int)fresh) - 1;
        fresh &= fresh - 1;
        row[c] = (uint8_t)k;
      }
    }
    if (!__syncthreads_or(any)) break;                            // (a barrier) no pair at distance k: none farther
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
}

}  // namespace

extern "C" {

int hscn_spd_supported(int max_nodes, int max_dist) { return spd_supported(max_nodes, max_dist) ? 1 : 0; }

int hscn_spd_buckets(const int64_t* edge_index, const int32_t* ptr32, const int32_t* eptr32, const int64_t* spd_ptr,
                     int64_t N, int64_t E, int64_t B, int64_t total, int max_nodes, int max_dist, uint8_t* bucket,
                     int32_t* flag, void* stream_) {
  if (N < 0 || E < 0 || B < 0 || total < 0 || max_nodes < 0) return HSCN_E_BADARG;
  if (N > INT32_MAX || E > INT32_MAX || B >= INT32_MAX) return HSCN_E_BADARG;     // ptr32 / eptr32 are int32
  if (!spd_supported(max_nodes, max_dist)) return HSCN_E_UNSUPPORTED;
  if (N == 0 || B == 0) return 0;
  if (!ptr32 || !eptr32 || !spd_ptr || !flag || (E > 0 && !edge_index) || (total > 0 && !bucket)) return HSCN_E_BADARG;
  const SpdArgs A{edge_index, ptr32, eptr32, spd_ptr, bucket, N, E, total, max_nodes, max_dist, flag};
  return launch_with_lds<SPD_STATIC_LDS>(k_spd, (unsigned)B, SPD_THREADS, spd_lds_bytes(max_nodes), hscn_stream(stream_), A);
}

}  // extern "C"
