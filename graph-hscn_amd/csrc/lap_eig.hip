// Laplacian statistics of the SignNet positional encoding (reference transform/posenc.py:14-107; the host restatement
// is graph_hscn/transform/posenc.py) as ONE launch: workgroup g takes graph g from the batch's edge list to its rows
// of eigvecs / eigvals [N, max_freqs].  No dense Laplacian in HBM, no padding to the largest graph, no host loop.
//
// Assemble.  The matrix has ne = n rounded up to even rows of ld = ne + 1 floats.  Edges are counted with INTEGER
// atomics in the matrix storage (is_undirected: every listed edge adds 1, duplicates sum; otherwise both directions
// are stored as 1, duplicates merged), self loops dropped; the degree is the row sum (lane i walks row i: ld is odd,
// so 32 consecutive rows fall on 32 different LDS banks); then every pair i >= c is turned into the float32 entry of
// D - A, I - D^-1/2 A D^-1/2 or I - D^-1 A taken from the LOWER triangle and written to both triangles -- the matrix
// np.linalg.eigh decomposes (for "rw" that is not the matrix as written).  With an odd n, index n is a zero row and
// column: its pivots are exactly 0, every rotation with it is the identity, and it takes no part in the selection.
//
// Decompose: two-sided cyclic Jacobi, round-robin ordering.  Round r of the ne - 1 rounds of a sweep pairs
// (i0 + k, i0 - k) mod (ne - 1) for k = 1 .. ne/2 - 1 and (i0, ne - 1), i0 = r * ne/2 mod (ne - 1): ne/2 disjoint
// pivots whose row and column indices are consecutive in k.  Phase 1: thread k takes (c, s) of pivot k from a_pp,
// a_qq, a_pq, updates the two diagonal entries and zeroes a_pq.  Barrier.  Phase 2: the column step A J and the row
// step J^T A are one pass -- thread (k1, k2) owns the 2 x 2 block rows {p1, q1} x columns {p2, q2}, reads it once and
// writes J1^T block J2; every entry is read and written by exactly one thread, and lanes run over k2, i.e. over
// consecutive columns of one row (ascending for p2, descending for q2): conflict-free in LDS, coalesced in global
// memory.  The four results are summed as (a-term + d-term) + (b-term + c-term), which is the same expression for
// a block and its transpose, so A stays symmetric bit for bit.  V is kept transposed (row j = vector j) and takes
// the row step V^T <- J^T V^T, lanes along the row.  Barrier.
// The diagonal lives in float64 (4 KB of LDS): a diagonal entry is updated ne * sweeps times and in float32 those
// roundings, not the rotations, would set the eigenvalue error.  Rotation angles are computed in float64 as well
// (ne/2 per round); the matrix, the vectors and (c, s) are float32.
// A sweep starts with sum_{i != j} a_ij^2 (fixed-order block sum): at most 1e-15 * ||A||_F^2 ends the loop, and so
// does the sweep cap (flag bit 1).  Jacobi's off-diagonal roundings are relative to the off-diagonal entries
// themselves, so the threshold is reached, not approached.
//
// Storage: n <= hscn_lap_eig_lds_max_n() keeps A and V^T in dynamic LDS; a larger graph (up to 512) uses its slab of
// the caller's workspace through the same code (the workgroup's own global stores are visible to it behind
// __syncthreads, as in metrics.hip).  The choice is per graph, inside one launch.
//
// Tail (get_lap_decomp_stats, eigvec_normalizer): rank the n eigenvalues (ties by index), keep the max_freqs
// smallest, clamp at 0, one wave per kept vector for the L1 / L2 / abs-max denominator (clamped at 1e-12), write
// both outputs at the graph's node offset, NaN in the columns from n on.  No float atomics: same input, same bits.
#include "hscn_common.h"

namespace {

constexpr int LE_MAX_N = 512;
constexpr int LE_MAX_FREQS = 64;
constexpr int LE_SWEEP_CAP = 30;
constexpr double LE_TOL2 = 1e-15;              // off^2 <= LE_TOL2 * fro^2
constexpr int LE_FLAG_CAP = 1, LE_FLAG_EDGE = 2, LE_FLAG_GRAPH = 4;

struct LeScratch {
  double d[LE_MAX_N];                          // the diagonal
  float f[LE_MAX_N];                           // assembly: degree weights; sweeps: c [0, 256), s [256, 512)
  int p[LE_MAX_N / 2], q[LE_MAX_N / 2];        // the round's pivots
  double red[16];
  int sel[LE_MAX_FREQS];
  float den[LE_MAX_FREQS];
};

__host__ __device__ inline int le_even(int n) { return n + (n & 1); }
__host__ __device__ inline size_t le_matrix_floats(int n) { return (size_t)le_even(n) * (size_t)(le_even(n) + 1); }

int le_lds_max_n() {
  int n = 0;
  while (n < LE_MAX_N && 2 * le_matrix_floats(n + 1) * 4 + sizeof(LeScratch) <= LDS_CU_BYTES) ++n;
  return n;
}

struct LeArgs {
  const int64_t* ei;
  int64_t E, N;
  const int32_t* nptr;
  const int32_t* eptr;
  int max_n, lds_max_n, lap_norm, undirected, K, vec_norm;
  float* eigvals;
  float* eigvecs;
  int32_t* flag;
  float* ws;
  int32_t* sweeps;                             // or NULL
};

// sum over the workgroup in a fixed order, returned to every thread
__device__ __forceinline__ double le_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; ++w) t += red[w];
  return t;
}

__device__ __forceinline__ void le_graph(float* A, float* Vt, LeScratch& S, const LeArgs& a, int g, int n0, int n,
                                         int64_t e0, int64_t e1) {
  const int t = threadIdx.x, NT = blockDim.x;
  const int ne = le_even(n), ld = ne + 1, h = ne >> 1, m = ne - 1;
  int* Ai = reinterpret_cast<int*>(A);

  // ---- assemble ----
  for (int idx = t; idx < ne * ld; idx += NT) {
    const int i = idx / ld, j = idx - i * ld;
    Ai[idx] = 0;
    Vt[idx] = i == j ? 1.f : 0.f;
  }
  __syncthreads();
  bool bad = false;
  for (int64_t e = e0 + t; e < e1; e += NT) {
    const int64_t r = a.ei[e] - n0, c = a.ei[a.E + e] - n0;
    if (r < 0 || r >= n || c < 0 || c >= n) { bad = true; continue; }
    if (r == c) continue;
    if (a.undirected) {
      atomicAdd(&Ai[(int)r * ld + (int)c], 1);
    } else {
      Ai[(int)r * ld + (int)c] = 1;
      Ai[(int)c * ld + (int)r] = 1;
    }
  }
  if (bad) atomicOr(a.flag, LE_FLAG_EDGE);
  __syncthreads();
  for (int i = t; i < ne; i += NT) {
    int s = 0;
    if (i < n)
      for (int c = 0; c < n; ++c) s += Ai[i * ld + c];
    float w = (float)s;
    if (a.lap_norm == 1) w = s > 0 ? (float)(1.0 / sqrt((double)s)) : 0.f;
    if (a.lap_norm == 2) w = s > 0 ? 1.f / (float)s : 0.f;
    S.f[i] = w;
  }
  __syncthreads();
  for (int idx = t; idx < ne * ne; idx += NT) {
    const int i = idx / ne, c = idx - i * ne;
    if (c > i) continue;
    float v = 0.f;
    if (i < n) {
      const float cnt = (float)Ai[i * ld + c];
      const float eye = i == c ? 1.f : 0.f;
      if (a.lap_norm == 0) v = (i == c ? S.f[i] : 0.f) - cnt;
      else if (a.lap_norm == 1) v = eye - (S.f[i] * cnt) * S.f[c];
      else v = eye - S.f[i] * cnt;
    }
    if (i == c) S.d[i] = (double)v;
    A[i * ld + c] = v;
    A[c * ld + i] = v;
  }
  __syncthreads();

  // ---- decompose ----
  float* rc = S.f;
  float* rs = S.f + LE_MAX_N / 2;
  double fro2 = 0.0;
  int sweeps = 0;
  bool capped = false;
  for (;;) {
    double part = 0.0;
    for (int idx = t; idx < ne * ne; idx += NT) {
      const int i = idx / ne, j = idx - i * ne;
      if (i != j) {
        const double v = (double)A[i * ld + j];
        part += v * v;
      }
    }
    const double off2 = le_block_sum(part, S.red);
    if (sweeps == 0) {
      double dp = 0.0;
      for (int i = t; i < ne; i += NT) dp += S.d[i] * S.d[i];
      fro2 = off2 + le_block_sum(dp, S.red);
    }
    if (off2 <= LE_TOL2 * fro2) break;
    if (sweeps == LE_SWEEP_CAP) { capped = true; break; }
    for (int r = 0; r < m; ++r) {
      const int i0 = (int)(((int64_t)r * h) % m);
      for (int k = t; k < h; k += NT) {
        int p = i0, q = m;
        if (k > 0) {
          p = i0 + k; if (p >= m) p -= m;
          q = i0 - k; if (q < 0) q += m;
        }
        const float apq = A[p * ld + q];
        float c = 1.f, s = 0.f;
        if (apq != 0.f) {
          const double dp = S.d[p], dq = S.d[q], x = (double)apq;
          const double th = (dq - dp) / (2.0 * x);
          const double tt = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
          const double cc = 1.0 / sqrt(tt * tt + 1.0);
          c = (float)cc;
          s = (float)(tt * cc);
          S.d[p] = dp - tt * x;
          S.d[q] = dq + tt * x;
          A[p * ld + q] = 0.f;
          A[q * ld + p] = 0.f;
        }
        S.p[k] = p; S.q[k] = q; rc[k] = c; rs[k] = s;
      }
      __syncthreads();
      for (int idx = t; idx < h * h; idx += NT) {
        const int k1 = idx / h, k2 = idx - k1 * h;
        if (k1 == k2) continue;
        const int p1 = S.p[k1] * ld, q1 = S.q[k1] * ld, p2 = S.p[k2], q2 = S.q[k2];
        const float c1 = rc[k1], s1 = rs[k1], c2 = rc[k2], s2 = rs[k2];
        const float cc = c1 * c2, cs = c1 * s2, sc = s1 * c2, ss = s1 * s2;
        const float xa = A[p1 + p2], xb = A[p1 + q2], xc = A[q1 + p2], xd = A[q1 + q2];
        A[p1 + p2] = (cc * xa + ss * xd) - (cs * xb + sc * xc);
        A[p1 + q2] = (cs * xa - sc * xd) + (cc * xb - ss * xc);
        A[q1 + p2] = (sc * xa - cs * xd) + (cc * xc - ss * xb);
        A[q1 + q2] = (ss * xa + cc * xd) + (sc * xb + cs * xc);
      }
      for (int idx = t; idx < h * ne; idx += NT) {
        const int k = idx / ne, j = idx - k * ne;
        const int pj = S.p[k] * ld + j, qj = S.q[k] * ld + j;
        const float c = rc[k], s = rs[k];
        const float x = Vt[pj], y = Vt[qj];
        Vt[pj] = c * x - s * y;
        Vt[qj] = s * x + c * y;
      }
      __syncthreads();
    }
    ++sweeps;
  }
  if (t == 0) {
    if (capped) atomicOr(a.flag, LE_FLAG_CAP);
    if (a.sweeps) a.sweeps[g] = sweeps;
  }

  // ---- select, normalise, write ----
  const int K = a.K, kk = K < n ? K : n;
  for (int j = t; j < n; j += NT) {
    const double dj = S.d[j];
    int rk = 0;
    for (int i = 0; i < n; ++i) {
      const double di = S.d[i];
      rk += (di < dj) || (di == dj && i < j);
    }
    if (rk < K) S.sel[rk] = j;
  }
  __syncthreads();
  const int lane = t & 63, nw = NT >> 6;
  for (int r = t >> 6; r < kk; r += nw) {
    const float* v = Vt + S.sel[r] * ld;
    float acc = 0.f;
    for (int i = lane; i < n; i += 64) {
      const float x = v[i];
      if (a.vec_norm == 0) acc += fabsf(x);
      else if (a.vec_norm == 1) acc += x * x;
      else acc = fmaxf(acc, fabsf(x));
    }
    acc = a.vec_norm == 2 ? wave_max(acc) : wave_sum(acc);
    if (a.vec_norm == 1) acc = sqrtf(acc);
    if (lane == 0) S.den[r] = fmaxf(acc, 1e-12f);
  }
  __syncthreads();
  const float nanv = __uint_as_float(0x7fc00000u);
  for (int idx = t; idx < n * K; idx += NT) {
    const int i = idx / K, r = idx - i * K;
    float ve = nanv, va = nanv;
    if (r < kk) {
      const int j = S.sel[r];
      ve = Vt[j * ld + i] / S.den[r];
      va = fmaxf((float)S.d[j], 0.f);
    }
    const int64_t o = (int64_t)(n0 + i) * K + r;
    a.eigvecs[o] = ve;
    a.eigvals[o] = va;
  }
}

__global__ void __launch_bounds__(1024) k_lap_eig_stats(LeArgs a) {
  extern __shared__ __align__(16) float le_dyn[];
  __shared__ LeScratch S;
  const int g = blockIdx.x;
  const int64_t n0 = a.nptr[g], n1 = a.nptr[g + 1];
  int64_t e0 = a.eptr[g], e1 = a.eptr[g + 1];
  if (n0 < 0 || n1 > a.N || n1 - n0 > a.max_n || n1 < n0) {       // a graph beyond what the launch was sized for
    if (threadIdx.x == 0) atomicOr(a.flag, LE_FLAG_GRAPH);
    const int64_t lo = n0 < 0 ? 0 : n0, hi = n1 > a.N ? a.N : n1;
    const float nanv = __uint_as_float(0x7fc00000u);
    for (int64_t o = lo * a.K + threadIdx.x; o < hi * a.K; o += blockDim.x) {
      a.eigvecs[o] = nanv;
      a.eigvals[o] = nanv;
    }
    return;
  }
  if (e0 < 0) e0 = 0;
  if (e1 > a.E) e1 = a.E;
  const int n = (int)(n1 - n0);
  if (n == 0) return;
  if (n <= a.lds_max_n) {
    le_graph(le_dyn, le_dyn + le_matrix_floats(n), S, a, g, (int)n0, n, e0, e1);
  } else {
    float* slab = a.ws + (size_t)g * 2 * le_matrix_floats(a.max_n);
    le_graph(slab, slab + le_matrix_floats(n), S, a, g, (int)n0, n, e0, e1);
  }
}

}  // namespace

extern "C" {

int hscn_lap_eig_supported(int max_n, int max_freqs) {
  return max_n >= 1 && max_n <= LE_MAX_N && max_freqs >= 1 && max_freqs <= LE_MAX_FREQS;
}

int hscn_lap_eig_lds_max_n(void) {
  static const int v = le_lds_max_n();
  return v;
}

size_t hscn_lap_eig_workspace_bytes(int64_t B, int max_n) {
  if (B < 1 || max_n <= hscn_lap_eig_lds_max_n() || max_n > LE_MAX_N) return 0;
  return (size_t)B * 2 * le_matrix_floats(max_n) * sizeof(float);
}

int hscn_lap_eig_stats(const int64_t* edge_index, int64_t E, const int32_t* nptr, const int32_t* eptr, int64_t N,
                       int64_t B, int max_n, int lap_norm, int is_undirected, int max_freqs, int eigvec_norm,
                       float* eigvals, float* eigvecs, int32_t* flag, void* workspace, size_t workspace_bytes,
                       void* stream_) {
  if (E < 0 || N < 0 || B < 0 || max_n < 0 || max_freqs < 1 || lap_norm < 0 || lap_norm > 2 || eigvec_norm < 0 ||
      eigvec_norm > 2 || !nptr || !eptr || !eigvals || !eigvecs || !flag || (E > 0 && !edge_index) ||
      B > 0x7fffffff || N > 0x7fffffff)
    return HSCN_E_BADARG;
  if (B == 0 || N == 0) return 0;
  if (!hscn_lap_eig_supported(max_n, max_freqs)) return HSCN_E_UNSUPPORTED;
  const size_t need = hscn_lap_eig_workspace_bytes(B, max_n);
  if (workspace_bytes < need || (need > 0 && !workspace)) return HSCN_E_BADARG;
  LeArgs a;
  a.ei = edge_index; a.E = E; a.N = N; a.nptr = nptr; a.eptr = eptr;
  a.max_n = max_n; a.lds_max_n = hscn_lap_eig_lds_max_n(); a.lap_norm = lap_norm; a.undirected = is_undirected != 0;
  a.K = max_freqs; a.vec_norm = eigvec_norm;
  a.eigvals = eigvals; a.eigvecs = eigvecs; a.flag = flag;
  a.ws = static_cast<float*>(workspace);
  // a workspace with room for B more words behind what was asked receives the sweep count of every graph there
  a.sweeps = workspace && workspace_bytes >= need + (size_t)B * 4
                 ? reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + need) : nullptr;
  const int n_lds = max_n < a.lds_max_n ? max_n : a.lds_max_n;
  const size_t lds = 2 * le_matrix_floats(n_lds) * sizeof(float);
  const int threads = max_n <= 64 ? 256 : 1024;
  return launch_with_lds<sizeof(LeScratch)>(k_lap_eig_stats, (unsigned)B, threads, lds, hscn_stream(stream_), a);
}

}  // extern "C"
