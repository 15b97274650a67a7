// Exphormer's expander edges, built on the device: every graph g of n nodes gets degree / 2 random Hamiltonian cycles,
// each emitted in both directions -- n * degree directed edges at offset degree * ptr32[g] of an int64 [2, degree * N]
// edge list.  No scan, no host round trip.  The published construction regenerates until the expander is simple; this
// one keeps what the permutations give: n = 1 yields self loops, n = 2 repeats, and repeats and loops count.
//
// Cycle r of graph g (tests/exphormer_oracle.py restates this bit for bit):
//   gid   = graph_ids[g], or g without graph_ids
//   ctr   = (uint64(gid) << 32) | (r << 16) | t          for the node with local id t
//           (t < 2048 < 2^16 and r < 16, so r << 16 | t < 2^20: no two (gid, r, t) of the envelope share a counter)
//   key_t = (uint64(philox4x32_10(seed, ctr)[0]) << 32) | t
//   pi    = the local ids in ascending order of their keys (the low word breaks ties: keys are distinct)
//   block r = the edges pi[i] -> pi[(i + 1) mod n], i = 0 .. n - 1, then their reverses in the same order,
//             at offset degree * ptr32[g] + 2 n r
// Because of graph_ids a graph's expander does not depend on where the graph stands in a batch.
//
// One workgroup per graph; the keys are sorted by a bitonic network in LDS, padded to a power of two with all-ones keys
// (which no node has: t < 2^32 - 1).  EXPANDER_MAX_NODES = 2048 keys are 16 KB: no LDS opt-in.  A graph of more than
// max_nodes nodes (or a ptr32 that is not ascending inside [0, N]) emits -1 for the edges that lie inside the output
// and ORs bit 0 into the flag word.  Integers only: the same bits on every run.  One launch; no launch besides it.
#include "hscn_common.h"

namespace {

constexpr int EXPANDER_THREADS = 256;
constexpr int EXPANDER_MAX_NODES = 2048;
constexpr int EXPANDER_MAX_DEGREE = 32;
static_assert(EXPANDER_MAX_NODES * sizeof(uint64_t) <= LDS_NO_OPT_IN_BYTES, "the keys need no opt-in");
static_assert(EXPANDER_MAX_NODES <= (1 << 16) && EXPANDER_MAX_DEGREE / 2 <= 16, "the counter packing");

__global__ void __launch_bounds__(EXPANDER_THREADS) k_expander(const int32_t* __restrict__ ptr32,
                                                               const int32_t* __restrict__ graph_ids, int64_t N, int B,
                                                               int degree, uint64_t seed, int max_nodes,
                                                               int64_t* __restrict__ out, int32_t* flag) {
  __shared__ uint64_t keys[EXPANDER_MAX_NODES];
  const int g = blockIdx.x;
  if (g >= B) return;
  const int64_t lo = ptr32[g], hi = ptr32[g + 1];
  const int64_t total = (int64_t)degree * N;
  if (lo < 0 || hi < lo || hi > N) {                       // not a batch's ptr: nothing of this graph can be placed
    if (threadIdx.x == 0) atomicOr(flag, 1);
    return;
  }
  const int64_t n64 = hi - lo;
  if (n64 > max_nodes) {                                   // outside the envelope: no valid edge (the range is inside out)
    if (threadIdx.x == 0) atomicOr(flag, 1);
    for (int64_t p = threadIdx.x; p < n64 * degree; p += EXPANDER_THREADS) {
      out[degree * lo + p] = -1;
      out[total + degree * lo + p] = -1;
    }
    return;
  }
  const int n = (int)n64;
  if (n == 0) return;
  int P = 1;
  while (P < n) P <<= 1;
  const uint32_t gid = (uint32_t)(graph_ids ? graph_ids[g] : g);
  for (int r = 0; r < degree / 2; ++r) {                   // (uniform over the workgroup: barriers inside)
    for (int t = threadIdx.x; t < P; t += EXPANDER_THREADS) {
      uint64_t key = ~0ull;
      if (t < n) {
        uint32_t c[4];
        philox4x32_10(seed, ((uint64_t)gid << 32) | ((uint64_t)r << 16) | (uint64_t)t, c);
        key = ((uint64_t)c[0] << 32) | (uint64_t)t;
      }
      keys[t] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < P; t += EXPANDER_THREADS) {
          const int x = t ^ j;
          if (x > t) {
            const uint64_t a = keys[t], b = keys[x];
            const bool up = (t & k) == 0;
            if ((a > b) == up) keys[t] = b, keys[x] = a;
          }
        }
        __syncthreads();
      }
    }
    const int64_t base = degree * lo + 2 * (int64_t)n * r;
    for (int i = threadIdx.x; i < n; i += EXPANDER_THREADS) {
      const int64_t a = lo + (int64_t)(uint32_t)keys[i];
      const int64_t b = lo + (int64_t)(uint32_t)keys[i + 1 < n ? i + 1 : 0];
      out[base + i] = a, out[total + base + i] = b;
      out[base + n + i] = b, out[total + base + n + i] = a;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int hscn_expander_max_nodes(void) { return EXPANDER_MAX_NODES; }
int hscn_expander_max_degree(void) { return EXPANDER_MAX_DEGREE; }

int hscn_expander_build(const int32_t* ptr32, const int32_t* graph_ids, int64_t N, int64_t B, int degree, uint64_t seed,
                        int max_nodes, int64_t* edge_index, int32_t* flag, void* stream_) {
  if (N < 0 || B < 0 || N > INT32_MAX || B > INT32_MAX || max_nodes < 0) return HSCN_E_BADARG;
  if (degree < 2 || degree % 2) return HSCN_E_BADARG;
  if (degree > EXPANDER_MAX_DEGREE || max_nodes > EXPANDER_MAX_NODES) return HSCN_E_UNSUPPORTED;
  if (N > INT64_MAX / (2 * EXPANDER_MAX_DEGREE)) return HSCN_E_BADARG;
  if (!ptr32 || !flag || (N > 0 && !edge_index)) return HSCN_E_BADARG;
  if (N == 0 || B == 0) return 0;
  k_expander<<<(unsigned)B, EXPANDER_THREADS, 0, hscn_stream(stream_)>>>(ptr32, graph_ids, N, (int)B, degree, seed,
                                                                         max_nodes, edge_index, flag);
  HSCN_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

}  // extern "C"
