// Six unsigned keys in ascending order through a 12-comparator network, and the row-record words built from them.
// Plain C++: a host program includes this file as it stands (tests/test_step_builds_host.py compiles one).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROW_SORT6_FN __host__ __device__ inline
#else
#define ROW_SORT6_FN inline
#endif

// one comparator: (a, b) -> (min, max)  (v_min_u32 / v_max_u32 on the device)
ROW_SORT6_FN void row_sort6_cx(uint32_t& a, uint32_t& b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// k[0] <= k[1] <= ... <= k[5] on return.  The network is the 12-comparator, depth-6 one
// (1,2)(4,5) (0,2)(3,5) (0,1)(3,4) (2,5) (0,3)(1,4) (2,4)(1,3) (2,3); all 64 zero-one inputs sort.
ROW_SORT6_FN void row_sort6(uint32_t (&k)[6]) {
  row_sort6_cx(k[1], k[2]); row_sort6_cx(k[4], k[5]);
  row_sort6_cx(k[0], k[2]); row_sort6_cx(k[3], k[5]);
  row_sort6_cx(k[0], k[1]); row_sort6_cx(k[3], k[4]);
  row_sort6_cx(k[2], k[5]);
  row_sort6_cx(k[0], k[3]); row_sort6_cx(k[1], k[4]);
  row_sort6_cx(k[2], k[4]); row_sort6_cx(k[1], k[3]);
  row_sort6_cx(k[2], k[3]);
}

// A row's record from the c <= 6 packed keys (edge number << 16 | neighbour id) its edges left in slot[0 .. c) in any
// order; slot[c .. 6) may hold anything.  id[q] = the neighbour of the row's q-th edge in ascending edge order for
// q < c, the row itself beyond.  Edge numbers are at most 65 534, so no real key is 0xffffffff and the c real keys are
// the first c after the sort.
ROW_SORT6_FN void row_record_ids(const uint32_t (&slot)[6], int c, uint32_t r, uint32_t (&id)[6]) {
  uint32_t k[6];
  for (int j = 0; j < 6; ++j) k[j] = j < c ? slot[j] : 0xffffffffu;
  row_sort6(k);
  for (int j = 0; j < 6; ++j) id[j] = j < c ? (k[j] & 0xffffu) : r;
}

// 1 / sqrt(c) for a row of c = 0 .. 6 edges (0 for an empty row): the bits of 1.0f / sqrtf((float)c) with both
// operations correctly rounded, as the general build computes them.
ROW_SORT6_FN float row_degree_norm6(int c) {
  float v = 0.f;
  v = c == 1 ? 1.0f : v;
  v = c == 2 ? 0x1.6a09e6p-1f : v;
  v = c == 3 ? 0x1.279a74p-1f : v;
  v = c == 4 ? 0.5f : v;
  v = c == 5 ? 0x1.c9f25cp-2f : v;
  v = c == 6 ? 0x1.a20bd6p-2f : v;
  return v;
}
