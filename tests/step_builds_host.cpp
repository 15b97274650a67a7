// Host check of csrc/row_sort6.h (tests/test_step_builds_host.py compiles and runs this file):
//   1. the comparator network sorts all 64 zero-one inputs (hence every input);
//   2. on 10^4 random rows of 0 .. 6 packed keys in random slot order, the ids of mask-after-sort equal those of the
//      rank-and-route form the row records were built with before (edge numbers and neighbours read apart, the edge
//      numbers ranked pairwise, every neighbour routed to the slot of its rank);
//   3. the degree norm's seven values carry the bits of 1.0f / sqrtf((float)c).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "row_sort6.h"

// the earlier form, from its inputs: ev = the edge numbers in the row's slots, other[e] = edge e's neighbour
static void rank_and_route(const int (&ell)[6], const int* other, int c, uint32_t r, uint32_t (&id)[6]) {
  int ev[6], ov[6];
  for (int j = 0; j < 6; ++j) ev[j] = j < c ? ell[j] : 0x7fffffff;
  for (int j = 0; j < 6; ++j) ov[j] = other[j < c ? ev[j] : 0];
  for (int j = 0; j < 6; ++j) id[j] = r;
  for (int j = 0; j < 6; ++j) {
    int rank = 0;
    for (int m = 0; m < 6; ++m) rank += ev[m] < ev[j] ? 1 : 0;
    for (int q = 0; q < 6; ++q)
      if (j < c && rank == q) id[q] = (uint32_t)ov[j];
  }
}

int main() {
  for (unsigned bits = 0; bits < 64; ++bits) {
    uint32_t k[6];
    for (int j = 0; j < 6; ++j) k[j] = (bits >> j) & 1u;
    row_sort6(k);
    for (int j = 0; j + 1 < 6; ++j)
      if (k[j] > k[j + 1]) { std::printf("zero-one input %u is not sorted\n", bits); return 1; }
  }
  std::mt19937 gen(20240611u);
  constexpr int NE = 65535;                       // edge numbers 0 .. 65 534, ids 0 .. 65 534: the fields' whole range
  static int other[NE];
  for (int e = 0; e < NE; ++e) other[e] = (int)(gen() % 65535u);
  other[NE - 1] = 65534;
  for (int row = 0; row < 10000; ++row) {
    const int c = (int)(gen() % 7u);
    const uint32_t r = gen() % 65535u;
    int ell[6];
    uint32_t slot[6];
    for (int j = 0; j < 6; ++j) {
      bool fresh;
      do {                                        // distinct edge numbers, the extremes among them now and then
        const unsigned pick = gen() % 16u;
        ell[j] = pick == 0 ? 0 : (pick == 1 ? NE - 1 : (int)(gen() % (unsigned)NE));
        fresh = true;
        for (int m = 0; m < j; ++m) fresh = fresh && ell[m] != ell[j];
      } while (!fresh);
      slot[j] = ((uint32_t)ell[j] << 16) | (uint32_t)other[ell[j]];
    }
    for (int j = c; j < 6; ++j) slot[j] = gen();  // an unused slot holds anything
    uint32_t want[6], got[6];
    rank_and_route(ell, other, c, r, want);
    row_record_ids(slot, c, r, got);
    if (std::memcmp(want, got, sizeof want) != 0) { std::printf("row %d (c = %d) differs\n", row, c); return 1; }
  }
  for (int c = 0; c <= 6; ++c) {
    const float want = c > 0 ? 1.0f / sqrtf((float)c) : 0.f, got = row_degree_norm6(c);
    if (std::memcmp(&want, &got, sizeof want) != 0) { std::printf("norm of c = %d differs\n", c); return 1; }
  }
  std::printf("row_sort6 ok\n");
  return 0;
}
