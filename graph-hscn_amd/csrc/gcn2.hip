// GCNII's layer (PyG GCN2Conv) as one launch forward: gather -> mix with x0 -> weight product -> epilogue.
//
//   p_i = sum over row i's CSR slots j of (dinv_i dinv_j) x_j      slot order, multiply and add rounded separately
//   shared weights:  h = (1 - alpha) p + alpha x0                   y = (1 - beta) h + beta (h W1)
//   two weights:     pa = (1 - alpha) p, xa = alpha x0, h = pa + xa  y = (1 - beta) h + beta (pa W1 + xa W2)
//   out = act(y)
//
// A workgroup owns a tile of rows (32; 16 with two weights, which keep two tiles).  It gathers the tile's rows into
// LDS, multiplies the tile by the weight on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per element, exact f32)
// and writes out and the saved tile (h; pa with two weights: what the weight gradient multiplies).  The weight stays in
// LDS where tile + weight fit G2_RESIDENT_BYTES (the workgroup then walks several tiles); wider, it passes through LDS
// in column panels of 64 / 32 / 16 columns, every panel over the full k range, inside the same launch.
//
// Backward: hscn_gcn2_bwd is the same structure over gy = act'(out) g with the TRANSPOSED weight(s); the weight
// gradients go through hscn_linear_bwd_w's ordered two-stage reduction; the gradient of x is hscn_spmm_csr_gcn over the
// source-keyed CSR.  No float atomics anywhere.
#include "hscn_common.h"

namespace {

constexpr int G2_THREADS = 256;
constexpr int G2_MIN_WIDTH = 4;
constexpr int G2_MAX_WIDTH = 512;
constexpr int G2_ROWS = 32;          // rows of a tile where the workgroup keeps one tile
constexpr int G2_ROWS_TWO = 16;      // ... two tiles (forward with two weights)
constexpr size_t G2_RESIDENT_BYTES = 96 * 1024;   // tile(s) + whole weight(s) within this: the weight stays in LDS
constexpr size_t G2_TWO_WG_BYTES = 80 * 1024;     // a streamed panel is chosen to leave room for two workgroups a CU

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Plan {
  int rt;         // rows per tile
  int hs;         // floats per tile row: H + 2 (2 x odd: the 16 rows x 2 k of an MFMA A read fall on 32 banks)
  int pw;         // weight columns in LDS at a time (a multiple of 16; of 32 from 32 up: the bank swizzle needs it)
  int np;         // panels
  int resident;
  size_t lds;
};

inline bool width_ok(int H) { return H >= G2_MIN_WIDTH && H <= G2_MAX_WIDTH && H % 4 == 0; }

// ntiles LDS tiles and nw weight images
inline bool plan_of(int H, int ntiles, int nw, Plan& p) {
  if (!width_ok(H)) return false;
  p.rt = ntiles == 2 ? G2_ROWS_TWO : G2_ROWS;
  p.hs = H + 2;
  const size_t tiles = (size_t)ntiles * p.rt * p.hs * 4;
  const int hp32 = (H + 31) / 32 * 32;
  const size_t whole = tiles + (size_t)nw * H * hp32 * 4;
  if (whole <= G2_RESIDENT_BYTES) {
    p.pw = hp32; p.np = 1; p.resident = 1; p.lds = whole;
    return true;
  }
  p.resident = 0;
  p.pw = 0;
  const int cand[3] = {64, 32, 16};
  for (int c = 0; c < 3 && !p.pw; ++c)
    if (tiles + (size_t)nw * H * cand[c] * 4 <= G2_TWO_WG_BYTES) p.pw = cand[c];
  for (int c = 0; c < 3 && !p.pw; ++c)
    if (tiles + (size_t)nw * H * cand[c] * 4 <= LDS_CU_BYTES) p.pw = cand[c];
  if (!p.pw) return false;
  p.np = (H + p.pw - 1) / p.pw;
  p.lds = tiles + (size_t)nw * H * p.pw * 4;
  return true;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// a tile row starts 8-byte aligned (hs = H + 2)
__device__ __forceinline__ void st_tile(float* p, float4 v) {
  *reinterpret_cast<float2*>(p) = make_float2(v.x, v.y);
  *reinterpret_cast<float2*>(p + 2) = make_float2(v.z, v.w);
}
__device__ __forceinline__ float4 scale4(float s, float4 v) {
  return make_float4(mul_rn(s, v.x), mul_rn(s, v.y), mul_rn(s, v.z), mul_rn(s, v.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(add_rn(a.x, b.x), add_rn(a.y, b.y), add_rn(a.z, b.z), add_rn(a.w, b.w));
}

// Panel pn of W [H][H] (row = k, PyG's layout) into Wl [H][PW]: column c = pn PW + cc at cc ^ (16 if k is odd, from
// PW = 32 up), zeros past H.  TRANS: the panel of W^T, Wl[k][cc] = W[c][k].
template <bool TRANS>
__device__ __forceinline__ void load_panel(const float* __restrict__ W, float* __restrict__ Wl, int H, int PW, int pn) {
  const int swz = PW >= 32 ? 16 : 0;
  if (!TRANS) {
    const int P4 = PW >> 2;
    for (int idx = threadIdx.x; idx < H * P4; idx += G2_THREADS) {
      const int k = idx / P4, cc = (idx - k * P4) * 4;
      const int c = pn * PW + cc;
      const float4 v = c < H ? ld4(W + (size_t)k * H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      st4(Wl + (size_t)k * PW + (cc ^ ((k & 1) ? swz : 0)), v);
    }
  } else {
    const int H4 = H >> 2;
    for (int idx = threadIdx.x; idx < H4 * PW; idx += G2_THREADS) {
      const int k4 = idx / PW, cc = idx - k4 * PW;
      const int c = pn * PW + cc;
      const float4 v = c < H ? ld4(W + (size_t)c * H + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* d = Wl + (size_t)(4 * k4) * PW;
      d[cc] = v.x;
      d[PW + (cc ^ swz)] = v.y;
      d[2 * PW + cc] = v.z;
      d[3 * PW + (cc ^ swz)] = v.w;
    }
  }
}

// acc[rb] += T[16 rb .. +16][0 .. H) x Wl[0 .. H)[16 ct .. +16]: lane (li = lane & 15, lk = lane >> 4) feeds
// A[li][lk] = T[16 rb + li][k0 + lk] and B[lk][li] = Wl[k0 + lk][16 ct + li]; k0 + lk is odd exactly when lk is.
// The k range is summed in blocks of G2_KBLOCK: a block is one k-ordered fmaf chain from zero, the block sums are
// added in block order (one chain over 2 x 512 terms sat at the edge of what the float64 referee allows).
constexpr int G2_KBLOCK = 64;
template <int RB>
__device__ __forceinline__ void tile_times_panel(const float* __restrict__ T, const float* __restrict__ Wl, int H, int HS,
                                                 int PW, int ct, int li, int lk, f32x4 (&acc)[RB]) {
  const int swz = PW >= 32 ? 16 : 0;
  const float* ap = T + li * HS + lk;
  const float* bp = Wl + (size_t)lk * PW + ((ct * 16 + li) ^ ((lk & 1) ? swz : 0));
  for (int kb = 0; kb < H; kb += G2_KBLOCK) {
    const int ke = kb + G2_KBLOCK < H ? kb + G2_KBLOCK : H;
    f32x4 part[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) part[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k0 = kb; k0 < ke; k0 += 4) {
      const float bv = bp[(size_t)k0 * PW];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        part[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[rb * 16 * HS + k0], bv, part[rb], 0, 0, 0);
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] += part[rb];
  }
}

template <int RB, bool TWO>
__global__ void __launch_bounds__(G2_THREADS)
k_gcn2_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ dinv,
           const float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ W1,
           const float* __restrict__ W2, float* __restrict__ out, float* __restrict__ hsave, int64_t N, int H, int HS,
           int PW, int NP, float a, float oma, float b, float omb, int act, int64_t tiles) {
  extern __shared__ __align__(16) float lds[];
  constexpr int RT = 16 * RB;
  float* T = lds;                                        // [RT][HS]: h; pa with two weights
  float* T2 = lds + (TWO ? RT * HS : 0);                 // [RT][HS]: xa
  float* Wl = lds + (TWO ? 2 : 1) * RT * HS;             // [H][PW]
  float* Wl2 = Wl + (TWO ? (size_t)H * PW : 0);
  const int H4 = H >> 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  bool loaded = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * RT;
    // ---- gather + mix: a lane owns four columns of one row ----
    for (int idx = threadIdx.x; idx < RT * H4; idx += G2_THREADS) {
      const int rl = idx / H4, f = (idx - rl * H4) * 4;
      const int64_t r = r0 + rl;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f), xv = p;
      if (r < N) {
        const int s = rowptr[r], t = rowptr[r + 1];
        const float dr = dinv[r];
#pragma unroll 2
        for (int q = s; q < t; ++q) {
          const int j = col[q];
          const float w = mul_rn(dinv[j], dr);
          const float4 v = ld4(x + (size_t)j * H + f);
          p = make_float4(add_rn(p.x, mul_rn(w, v.x)), add_rn(p.y, mul_rn(w, v.y)), add_rn(p.z, mul_rn(w, v.z)),
                          add_rn(p.w, mul_rn(w, v.w)));
        }
        xv = ld4(x0 + (size_t)r * H + f);
      }
      const float4 pa = scale4(oma, p), xa = scale4(a, xv);
      if (TWO) {
        st_tile(T + rl * HS + f, pa);
        st_tile(T2 + rl * HS + f, xa);
        if (r < N) st4(hsave + (size_t)r * H + f, pa);
      } else {
        const float4 hv = add4(pa, xa);
        st_tile(T + rl * HS + f, hv);
        if (r < N) st4(hsave + (size_t)r * H + f, hv);
      }
    }
    __syncthreads();
    // ---- y = (1 - beta) h + beta (tile x weight), panel by panel ----
    for (int pn = 0; pn < NP; ++pn) {
      if (NP > 1 || !loaded) {
        load_panel<false>(W1, Wl, H, PW, pn);
        if (TWO) load_panel<false>(W2, Wl2, H, PW, pn);
        loaded = true;
        __syncthreads();
      }
      for (int ct = wave; ct * 16 < PW; ct += 4) {
        const int c0 = pn * PW + ct * 16;
        if (c0 >= H) break;
        f32x4 acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        tile_times_panel<RB>(T, Wl, H, HS, PW, ct, li, lk, acc);
        if (TWO) tile_times_panel<RB>(T2, Wl2, H, HS, PW, ct, li, lk, acc);
        const int c = c0 + li;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rl = rb * 16 + 4 * lk + q;
            const int64_t r = r0 + rl;
            if (r < N && c < H) {
              float hv = T[rl * HS + c];
              if (TWO) hv = add_rn(hv, T2[rl * HS + c]);
              out[(size_t)r * H + c] = apply_act(add_rn(mul_rn(omb, hv), mul_rn(b, acc[rb][q])), act);
            }
          }
      }
      if (NP > 1) __syncthreads();          // the next panel overwrites Wl
    }
    if (NP == 1) __syncthreads();           // the next tile overwrites T
  }
}

// gy = act'(out) g;  gyb = beta gy (what the weight gradients multiply);
// shared:  gh = (1 - beta) gy + beta gy W1^T          gp = (1 - alpha) gh,  gx0 = alpha gh
// two:     gp = (1 - alpha) ((1 - beta) gy + beta gy W1^T),  gx0 = alpha ((1 - beta) gy + beta gy W2^T)
// gyb, gp, gx0 may each be NULL.
template <bool TWO>
__global__ void __launch_bounds__(G2_THREADS)
k_gcn2_bwd(const float* __restrict__ g, const float* __restrict__ out, const float* __restrict__ W1,
           const float* __restrict__ W2, float* __restrict__ gyb, float* __restrict__ gp, float* __restrict__ gx0,
           int64_t N, int H, int HS, int PW, int NP, float a, float oma, float b, float omb, int act, int64_t tiles) {
  extern __shared__ __align__(16) float lds[];
  constexpr int RB = 2, RT = 32;
  float* T = lds;                                        // [RT][HS]: gy
  float* Wl = lds + RT * HS;                             // [H][PW]: a panel of W1^T
  float* Wl2 = Wl + (TWO ? (size_t)H * PW : 0);          //          ... of W2^T
  const int H4 = H >> 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const bool do1 = gp != nullptr || (!TWO && gx0 != nullptr);
  const bool do2 = TWO && gx0 != nullptr;
  bool loaded = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * RT;
    for (int idx = threadIdx.x; idx < RT * H4; idx += G2_THREADS) {
      const int rl = idx / H4, f = (idx - rl * H4) * 4;
      const int64_t r = r0 + rl;
      float4 gy = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < N) {
        const float4 gv = ld4(g + (size_t)r * H + f), ov = ld4(out + (size_t)r * H + f);
        gy = make_float4(gv.x * act_grad_from_output(ov.x, act), gv.y * act_grad_from_output(ov.y, act),
                         gv.z * act_grad_from_output(ov.z, act), gv.w * act_grad_from_output(ov.w, act));
        if (gyb) st4(gyb + (size_t)r * H + f, scale4(b, gy));
      }
      st_tile(T + rl * HS + f, gy);
    }
    __syncthreads();
    if (do1 || do2) {
      for (int pn = 0; pn < NP; ++pn) {
        if (NP > 1 || !loaded) {
          if (do1) load_panel<true>(W1, Wl, H, PW, pn);
          if (do2) load_panel<true>(W2, Wl2, H, PW, pn);
          loaded = true;
          __syncthreads();
        }
        for (int ct = wave; ct * 16 < PW; ct += 4) {
          const int c0 = pn * PW + ct * 16;
          if (c0 >= H) break;
          f32x4 acc1[RB], acc2[RB];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) acc1[rb] = acc2[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (do1) tile_times_panel<RB>(T, Wl, H, HS, PW, ct, li, lk, acc1);
          if (do2) tile_times_panel<RB>(T, Wl2, H, HS, PW, ct, li, lk, acc2);
          const int c = c0 + li;
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int rl = rb * 16 + 4 * lk + q;
              const int64_t r = r0 + rl;
              if (r < N && c < H) {
                const float base = mul_rn(omb, T[rl * HS + c]);
                const float gh1 = add_rn(base, mul_rn(b, acc1[rb][q]));
                const float gh2 = TWO ? add_rn(base, mul_rn(b, acc2[rb][q])) : gh1;
                if (gp) gp[(size_t)r * H + c] = mul_rn(oma, gh1);
                if (gx0) gx0[(size_t)r * H + c] = mul_rn(a, gh2);
              }
            }
        }
        if (NP > 1) __syncthreads();
      }
    }
    if (NP == 1 || !(do1 || do2)) __syncthreads();
  }
}

__global__ void k_gcn2_scale(float* __restrict__ v, float s, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) v[i] = mul_rn(s, v[i]);
}

inline unsigned grid_for(const Plan& p, int64_t tiles) {
  // a resident weight is loaded once per workgroup: as many workgroups as the chip holds at once, each walking tiles
  int64_t per_cu = (int64_t)(LDS_CU_BYTES / p.lds);
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 4) per_cu = 4;
  const int64_t cap = p.resident ? 256 * per_cu : 16384;
  return (unsigned)(tiles < cap ? tiles : cap);
}

inline bool coeffs_ok(double alpha, double beta) { return alpha >= 0.0 && alpha <= 1.0 && beta > 0.0 && beta <= 1.0; }
inline bool act_ok(int act) { return act == HSCN_ACT_IDENTITY || act == HSCN_ACT_RELU; }

}  // namespace

extern "C" {

int hscn_gcn2_supported(int H) { return width_ok(H) ? 1 : 0; }

int hscn_gcn2_plan(int H, int two_weights, int32_t* plan) {
  if (!plan) return HSCN_E_BADARG;
  Plan p;
  if (!plan_of(H, two_weights ? 2 : 1, two_weights ? 2 : 1, p)) return HSCN_E_UNSUPPORTED;
  plan[0] = p.rt; plan[1] = p.pw; plan[2] = p.resident; plan[3] = (int32_t)p.lds;
  return 0;
}

int hscn_gcn2_fwd(const int32_t* rowptr, const int32_t* col, const float* dinv, const float* x, const float* x0,
                  const float* W1, const float* W2, float* out, float* h, int64_t N, int H, double alpha, double beta,
                  int act, void* stream_) {
  if (N < 0 || N > INT32_MAX || !coeffs_ok(alpha, beta)) return HSCN_E_BADARG;
  if (!width_ok(H) || !act_ok(act)) return HSCN_E_UNSUPPORTED;
  if (N == 0) return 0;
  if (!rowptr || !col || !dinv || !x || !x0 || !W1 || !out || !h) return HSCN_E_BADARG;
  if (!aligned16(x) || !aligned16(x0) || !aligned16(W1) || !aligned16(W2) || !aligned16(out) || !aligned16(h))
    return HSCN_E_BADARG;
  const bool two = W2 != nullptr;
  Plan p;
  if (!plan_of(H, two ? 2 : 1, two ? 2 : 1, p)) return HSCN_E_UNSUPPORTED;
  const int64_t tiles = (N + p.rt - 1) / p.rt;
  const float a = (float)alpha, oma = (float)(1.0 - alpha), b = (float)beta, omb = (float)(1.0 - beta);
  hipStream_t st = hscn_stream(stream_);
  if (two)
    return launch_with_lds(k_gcn2_fwd<1, true>, grid_for(p, tiles), G2_THREADS, p.lds, st, rowptr, col, dinv, x, x0, W1,
                           W2, out, h, N, H, p.hs, p.pw, p.np, a, oma, b, omb, act, tiles);
  return launch_with_lds(k_gcn2_fwd<2, false>, grid_for(p, tiles), G2_THREADS, p.lds, st, rowptr, col, dinv, x, x0, W1,
                         W2, out, h, N, H, p.hs, p.pw, p.np, a, oma, b, omb, act, tiles);
}

int hscn_gcn2_bwd(const float* g, const float* out, const float* W1, const float* W2, float* gyb, float* gp, float* gx0,
                  int64_t N, int H, double alpha, double beta, int act, void* stream_) {
  if (N < 0 || N > INT32_MAX || !coeffs_ok(alpha, beta)) return HSCN_E_BADARG;
  if (!width_ok(H) || !act_ok(act)) return HSCN_E_UNSUPPORTED;
  if (N == 0 || (!gyb && !gp && !gx0)) return 0;
  if (!g || !out || !W1) return HSCN_E_BADARG;
  if (!aligned16(g) || !aligned16(out) || !aligned16(W1) || !aligned16(W2) || !aligned16(gyb) || !aligned16(gp) ||
      !aligned16(gx0))
    return HSCN_E_BADARG;
  const bool two = W2 != nullptr;
  Plan p;
  if (!plan_of(H, 1, two ? 2 : 1, p)) return HSCN_E_UNSUPPORTED;
  const int64_t tiles = (N + p.rt - 1) / p.rt;
  const float a = (float)alpha, oma = (float)(1.0 - alpha), b = (float)beta, omb = (float)(1.0 - beta);
  hipStream_t st = hscn_stream(stream_);
  if (two)
    return launch_with_lds(k_gcn2_bwd<true>, grid_for(p, tiles), G2_THREADS, p.lds, st, g, out, W1, W2, gyb, gp, gx0, N,
                           H, p.hs, p.pw, p.np, a, oma, b, omb, act, tiles);
  return launch_with_lds(k_gcn2_bwd<false>, grid_for(p, tiles), G2_THREADS, p.lds, st, g, out, W1, W2, gyb, gp, gx0, N, H,
                         p.hs, p.pw, p.np, a, oma, b, omb, act, tiles);
}

size_t hscn_gcn2_bwd_w_workspace_bytes(int64_t N, int H) { return hscn_linear_bwd_w_workspace_bytes(N, H, H); }

int hscn_gcn2_bwd_w(const float* gyb, const float* h, const float* x0, float* gW1, float* gW2, int64_t N, int H,
                    double alpha, void* workspace, size_t workspace_bytes, void* stream_) {
  if (N < 0 || !(alpha >= 0.0 && alpha <= 1.0) || !workspace) return HSCN_E_BADARG;
  if (!width_ok(H)) return HSCN_E_UNSUPPORTED;
  if ((gW2 != nullptr) && N > 0 && !x0) return HSCN_E_BADARG;
  if (N > 0 && (!gyb || (gW1 && !h))) return HSCN_E_BADARG;
  if (workspace_bytes < hscn_gcn2_bwd_w_workspace_bytes(N, H)) return HSCN_E_WORKSPACE;
  // gW[i][o] = sum_r left[r][i] gyb[r][o]: hscn_linear_bwd_w's "gy" is the left factor, its "x" the cotangent, so its
  // [O][I] result is PyG's [in][out] layout; chunk partials in row order, chunks folded in a fixed tree
  if (gW1)
    if (int rc = hscn_linear_bwd_w(h, gyb, gW1, nullptr, N, H, H, 0, workspace, workspace_bytes, stream_)) return rc;
  if (gW2) {
    if (int rc = hscn_linear_bwd_w(x0, gyb, gW2, nullptr, N, H, H, 0, workspace, workspace_bytes, stream_)) return rc;
    const int64_t n = (int64_t)H * H;
    k_gcn2_scale<<<hscn_blocks(n, 256), 256, 0, hscn_stream(stream_)>>>(gW2, (float)alpha, n);   // xa = alpha x0
    HSCN_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

}  // extern "C"
