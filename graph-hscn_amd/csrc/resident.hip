// Graph-resident HSCN engine, float32 storage: the C entry points of include/hscn.h over the kernels in
// resident_kernels.h (which holds the design notes).  resident_f16.hip instantiates the same kernels for IEEE-half
// feature / activation storage; the entry points here dispatch to it under HSCN_STORE_F16.
#include "resident_kernels.h"

extern "C" {


#ifdef HSCN_STAMPS
int hscn_diag_set_stamp_buffer(long long* buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf));
}
#endif

int hscn_resident_supported(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv) {
  if (!(H == 16 || H == 32 || H == 64) || F < 1 || F > H || L < 1 || L > MAXL || C < 1 || C > 4096) return 0;
  if (max_n < 0 || max_v < 0 || max_ell < 0 || max_evv < 0) return 0;
  if (fwd_lds_bytes(H, C, max_n, max_v, max_ell, max_evv, 0, 0) > LDS_CU_BYTES) return 0;
  if (bwd_lds_bytes(H, C, max_n, max_ell, 1) > LDS_CU_BYTES) return 0;
  return 1;
}

// the LDS a virtual (or both-branch) program lays out for the block it is handed, as hscn_fwd_body computes it
static int32_t fwd_need(const FwdArgs& A, int H, bool fixed = false) {
  if (fixed) return (int32_t)fwd_lds_bytes(H, 1, StepVCaps::N, StepVCaps::V, 0, StepVCaps::EVV, 1, 0);
  return (int32_t)fwd_lds_bytes(H, A.C, A.max_n, A.max_v, A.max_ell, A.max_evv, A.db, A.exp);
}

// Host arithmetic only: argument blocks that hold nothing but the size fields go through the planners of
// resident_kernels.h, the functions every launch_* takes its choices from.
int hscn_resident_launch_plan_ex(int launch, int F, int H, int L, int C, int max_n, int max_v, int max_ell,
                                 int max_evv, int want_export, int32_t* plan_host) {
  if (!plan_host || launch < HSCN_LAUNCH_PAIR || launch > HSCN_LAUNCH_STEP_VIRTUAL) return HSCN_E_BADARG;
  const bool step = launch == HSCN_LAUNCH_STEP || launch == HSCN_LAUNCH_STEP_VIRTUAL;
  const bool virt = launch == HSCN_LAUNCH_PAIR_VIRTUAL || launch == HSCN_LAUNCH_STEP_VIRTUAL;
  const bool want = want_export != 0;
  for (int i = 0; i < HSCN_PLAN_EX_COUNT; ++i) plan_host[i] = 0;
  FwdArgs Al{};
  Al.F = F; Al.L = L; Al.C = C; Al.max_n = max_n; Al.max_v = max_v; Al.max_ell = max_ell; Al.max_evv = max_evv;
  Al.l_end = L;
  FwdArgs Av = Al;          // a job's block (virtual_job_args): virtual-only, sized without ll edges
  Av.compute_virtual = 2; Av.max_ell = 0;
  if (step) {
    if (!hscn_resident_train_step_supported(F, H, L, C, max_n, max_ell, virt ? max_v : 0, virt ? max_evv : 0))
      return HSCN_E_UNSUPPORTED;
    StepArgs S{};
    S.F = F; S.L = L; S.C = C; S.max_n = max_n; S.max_ell = max_ell;
    LaunchPlan P;
    if (int rc = plan_step(S, virt ? &Av : nullptr, H, P)) return rc;
    plan_host[HSCN_PLAN_THREADS] = P.threads;
    plan_host[HSCN_PLAN_FWD_LDS] = (int32_t)P.lds;
    plan_host[HSCN_PLAN_LOCAL_FIXED] = P.local_fixed;
    plan_host[HSCN_PLAN_VIRTUAL_FIXED] = P.virtual_fixed;
    plan_host[HSCN_PLAN_FWD_LOCAL_NEED] =
        (int32_t)(P.local_fixed ? STEP_LFIX_LDS_BYTES : step_lds_bytes(H, L, C, max_n, max_ell));
    if (virt) {
      plan_host[HSCN_PLAN_V_DB] = Av.db;
      plan_host[HSCN_PLAN_V_ACQ] = Av.acq;
      plan_host[HSCN_PLAN_FWD_VIRTUAL_NEED] = fwd_need(Av, H, P.virtual_fixed);
    }
  } else {
    if (!hscn_resident_supported(F, H, L, C, max_n, max_v, max_ell, max_evv)) return HSCN_E_UNSUPPORTED;
    BwdArgs Ab{};
    Ab.F = F; Ab.L = L; Ab.C = C; Ab.max_n = max_n; Ab.max_ell = max_ell;
    FwdArgs Avb = Av;       // the job's block in the backward launch
    LaunchPlan Pf, Pb;
    // (the forward's virtual workgroup is taken to have been handed the ll edges whenever the export is wanted)
    if (int rc = virt ? plan_fwd_pair(Al, Av, H, want, want, Pf) : plan_fwd(Al, H, want, Pf)) return rc;
    if (int rc = virt ? plan_bwd_virtual(Ab, Avb, H, Pb) : plan_bwd(Ab, H, Pb)) return rc;
    if (Pf.threads != Pb.threads) return HSCN_E_UNSUPPORTED;   // (one rule, resident_threads: cannot happen)
    plan_host[HSCN_PLAN_THREADS] = Pf.threads;
    plan_host[HSCN_PLAN_FWD_DB] = Al.db;
    plan_host[HSCN_PLAN_FWD_EXP] = Al.exp;
    plan_host[HSCN_PLAN_CSR_LAUNCH] = Pf.csr_launch;
    plan_host[HSCN_PLAN_BWD_TWO] = Ab.two;
    plan_host[HSCN_PLAN_FWD_LDS] = (int32_t)Pf.lds;
    plan_host[HSCN_PLAN_BWD_LDS] = (int32_t)Pb.lds;
    plan_host[HSCN_PLAN_CSR_LDS] = (int32_t)Pf.csr_lds;
    plan_host[HSCN_PLAN_FWD_LOCAL_NEED] = fwd_need(Al, H);
    plan_host[HSCN_PLAN_BWD_LOCAL_NEED] = (int32_t)bwd_lds_bytes(H, C, max_n, max_ell, Ab.two);
    if (virt) {
      plan_host[HSCN_PLAN_V_DB] = Av.db;
      plan_host[HSCN_PLAN_V_EXP] = Av.exp;
      plan_host[HSCN_PLAN_BWD_V_DB] = Avb.db;
      plan_host[HSCN_PLAN_FWD_VIRTUAL_NEED] = fwd_need(Av, H);
      plan_host[HSCN_PLAN_BWD_VIRTUAL_NEED] = fwd_need(Avb, H);
    }
  }
  return 0;
}

// the plain pair's seven fields of the query above
int hscn_resident_launch_plan(int F, int H, int L, int C, int max_n, int max_v, int max_ell, int max_evv,
                              int want_export, int32_t* plan_host) {
  int32_t plan[HSCN_PLAN_EX_COUNT];
  if (!plan_host) return HSCN_E_BADARG;
  if (int rc = hscn_resident_launch_plan_ex(HSCN_LAUNCH_PAIR, F, H, L, C, max_n, max_v, max_ell, max_evv, want_export,
                                            plan))
    return rc;
  for (int i = 0; i < HSCN_PLAN_COUNT; ++i) plan_host[i] = plan[i];
  return 0;
}

int64_t hscn_resident_param_count(int F, int H, int L, int C) {
  int64_t P = 0;
  for (int l = 0; l < L; ++l) P += (int64_t)H * (l == 0 ? F : H) + H;
  return P + (int64_t)H * H + H + (int64_t)C * H + C;
}

// Each of the five launches: refuse a flag it has no variant for (and half storage at a width it is not instantiated
// at), then hand the exported argument list to the float instantiation or, under HSCN_STORE_F16, to the half one
// (resident_f16.hip).
static int check_flags(int flags, int valid, int H) {
  if (flags & ~valid) return HSCN_E_BADARG;
  return ((flags & HSCN_STORE_F16) && !hscn_resident_f16_takes(H)) ? HSCN_E_UNSUPPORTED : 0;
}
int hscn_resident_fwd(const void* x_local, const void* x_virtual, const int64_t* ei_ll, int64_t E_ll,
                      const int64_t* ei_vv, int64_t E_vv, const int64_t* ei_lv, int64_t E_lv,
                      const int32_t* lptr, const int32_t* vptr, const int32_t* eptr_ll, const int32_t* eptr_vv,
                      const int32_t* eptr_lv, int64_t N, int64_t V, int64_t B, int F, int H, int L, int C,
                      int head_act, float slope, const void* const* layer_params_host /* L x 9 */,
                      const float* W1, const float* b1, const float* W2, const float* b2, int max_n, int max_v,
                      int max_ell, int max_evv, int compute_virtual, void* acts, float* pooled, float* z,
                      float* pred, float* score, void* xv_out, int32_t* csr_rowptr_t, int32_t* csr_col_t,
                      float* dinv_out, int32_t* flag, int flags, void* stream_) {
  if (int rc = check_flags(flags, HSCN_STORE_F16, H)) return rc;
  return ((flags & HSCN_STORE_F16) ? hscn_resident_f16().fwd : impl_resident_fwd<float>)(
      x_local, x_virtual, ei_ll, E_ll, ei_vv, E_vv, ei_lv, E_lv, lptr, vptr, eptr_ll, eptr_vv, eptr_lv, N, V, B, F, H,
      L, C, head_act, slope, layer_params_host, W1, b1, W2, b2, max_n, max_v, max_ell, max_evv, compute_virtual, acts,
      pooled, z, pred, score, xv_out, csr_rowptr_t, csr_col_t, dinv_out, flag, flags, stream_);
}

int hscn_resident_bwd(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                      const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C, int head_act,
                      const void* const* W_ll_host /* L */, const float* W1, const float* W2, const void* acts,
                      const float* pooled, const float* z, const float* g_pred, const float* g_scale,
                      const int32_t* csr_rowptr_t, const int32_t* csr_col_t, const float* dinv, int max_n,
                      int max_ell, float* partials /*[B][P]*/, float* grads /*[P]*/, int32_t* flag,
                      const hscn_loss_tail* tail, int flags, void* stream_) {
  if (int rc = check_flags(flags, HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE, H)) return rc;
  return ((flags & HSCN_STORE_F16) ? hscn_resident_f16().bwd : impl_resident_bwd<float>)(
      x_local, ei_ll, E_ll, lptr, eptr_ll, N, B, F, H, L, C, head_act, W_ll_host, W1, W2, acts, pooled, z, g_pred,
      g_scale, csr_rowptr_t, csr_col_t, dinv, max_n, max_ell, partials, grads, flag, tail, flags, stream_);
}

int hscn_resident_bwd_with_virtual(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                                   const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C,
                                   int head_act, const void* const* W_ll_host, const float* W1, const float* W2,
                                   const void* acts, const float* pooled, const float* z, const float* g_pred,
                                   const float* g_scale, const int32_t* csr_rowptr_t, const int32_t* csr_col_t,
                                   const float* dinv, int max_n, int max_ell, float* partials, float* grads,
                                   int32_t* flag, const hscn_loss_tail* tail, const hscn_virtual_job* job,
                                   int flags, void* stream_) {
  if (int rc = check_flags(flags, HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE, H)) return rc;
  return ((flags & HSCN_STORE_F16) ? hscn_resident_f16().bwd_with_virtual : impl_resident_bwd_with_virtual<float>)(
      x_local, ei_ll, E_ll, lptr, eptr_ll, N, B, F, H, L, C, head_act, W_ll_host, W1, W2, acts, pooled, z, g_pred,
      g_scale, csr_rowptr_t, csr_col_t, dinv, max_n, max_ell, partials, grads, flag, tail, job, flags, stream_);
}

int hscn_resident_fwd_with_virtual(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                                   const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C,
                                   int head_act, const void* const* layer_params_host, const float* W1,
                                   const float* b1, const float* W2, const float* b2, int max_n, int max_ell,
                                   void* acts, float* pooled, float* z, float* pred, float* score,
                                   int32_t* csr_rowptr_t, int32_t* csr_col_t, float* dinv_out, int32_t* flag,
                                   const hscn_virtual_job* job, int flags, void* stream_) {
  if (int rc = check_flags(flags, HSCN_STORE_F16, H)) return rc;
  return ((flags & HSCN_STORE_F16) ? hscn_resident_f16().fwd_with_virtual : impl_resident_fwd_with_virtual<float>)(
      x_local, ei_ll, E_ll, lptr, eptr_ll, N, B, F, H, L, C, head_act, layer_params_host, W1, b1, W2, b2, max_n,
      max_ell, acts, pooled, z, pred, score, csr_rowptr_t, csr_col_t, dinv_out, flag, job, flags, stream_);
}

int hscn_resident_structure(const int64_t* ei_ll, int64_t E_ll, const int64_t* ei_vv, int64_t E_vv,
                            const int64_t* ei_lv, int64_t E_lv, const int32_t* lptr, const int32_t* vptr,
                            const int32_t* eptr_ll, const int32_t* eptr_vv, const int32_t* eptr_lv, int64_t B,
                            int max_n, int max_v, int max_ell, int max_evv, const hscn_structure* out,
                            int32_t* flag, void* stream_) {
  if (B < 0 || !out || max_n < 0 || max_v < 0 || max_ell < 0 || max_evv < 0) return HSCN_E_BADARG;
  if (B == 0) return 0;
  if (!lptr || !vptr || !eptr_ll || !eptr_vv || !eptr_lv || (E_ll > 0 && !ei_ll) || (E_vv > 0 && !ei_vv) ||
      (E_lv > 0 && !ei_lv))
    return HSCN_E_BADARG;
  if (!out->ll_rowptr_d || !out->ll_rowptr_s || !out->ll_dinv || !out->lv_rowptr || !out->vv_rowptr || !out->vv_dinv ||
      (E_ll > 0 && (!out->ll_col_d || !out->ll_col_s)) || (E_lv > 0 && !out->lv_col) || (E_vv > 0 && !out->vv_col))
    return HSCN_E_BADARG;
  StructArgs A;
  A.ll_src = ei_ll; A.ll_dst = ei_ll ? ei_ll + E_ll : nullptr;
  A.vv_src = ei_vv; A.vv_dst = ei_vv ? ei_vv + E_vv : nullptr;
  A.lv_src = ei_lv; A.lv_dst = ei_lv ? ei_lv + E_lv : nullptr;
  A.lptr = lptr; A.vptr = vptr; A.eptr_ll = eptr_ll; A.eptr_vv = eptr_vv; A.eptr_lv = eptr_lv;
  A.out = *out; A.flag = flag; A.max_n = max_n; A.max_v = max_v; A.max_ell = max_ell; A.max_evv = max_evv;
  const size_t lds = struct_lds_words(max_n, max_v, max_ell, max_evv) * 4;
  if (lds > LDS_CU_BYTES) return HSCN_E_UNSUPPORTED;
  return launch_with_lds(k_structure, (unsigned)B, 256, lds, hscn_stream(stream_), A);
}

// the step's envelope; the virtual program is sized without ll edges (max_v = 0: no virtual job)
int hscn_resident_train_step_supported(int F, int H, int L, int C, int max_n, int max_ell, int max_v, int max_evv) {
  if (!step_takes_widths(F, H, L, C)) return 0;
  if (max_n < 0 || max_ell < 0 || max_v < 0 || max_evv < 0) return 0;
  if (step_lds_bytes(H, L, C, max_n, max_ell) > LDS_CU_BYTES) return 0;
  if (max_v > 0 && fwd_lds_bytes(H, C, max_n, max_v, 0, max_evv, 0, 0) > LDS_CU_BYTES) return 0;
  return 1;
}

// workgroups of the one-launch step that one CU takes at a time: 1 for 16-wave workgroups (they are not made to
// share a CU), up to 4 for the 4-wave workgroups of small graphs (PCQM-Contact: n <= 64) when LDS allows
int hscn_resident_train_step_wgs_per_cu(int F, int H, int L, int C, int max_n, int max_ell, int max_v, int max_evv) {
  if (!hscn_resident_train_step_supported(F, H, L, C, max_n, max_ell, max_v, max_evv)) return 0;
  if (max_n > 64) return 1;
  size_t lds = step_lds_bytes(H, L, C, max_n, max_ell);
  if (max_v > 0) {
    const size_t lv = fwd_lds_bytes(H, C, max_n, max_v, 0, max_evv, 1, 0);
    if (lv > lds) lds = lv;
  }
  if (lds == 0) return 4;
  const int by_lds = (int)(LDS_CU_BYTES / lds);
  return by_lds < 1 ? 1 : (by_lds > 4 ? 4 : by_lds);
}

// (the step checks H itself, after its argument checks: no width check ahead of the half instantiation)
int hscn_resident_train_step(const void* x_local, const int64_t* ei_ll, int64_t E_ll, const int32_t* lptr,
                             const int32_t* eptr_ll, int64_t N, int64_t B, int F, int H, int L, int C, int head_act,
                             const void* const* layer_params_host, const float* W1, const float* b1, const float* W2,
                             const float* b2, int max_n, int max_ell, const float* target, int loss_kind, float* pred,
                             float* score, float* partials, float* grads, void* acts, uint32_t* sync, int32_t* flag,
                             const hscn_virtual_job* job, const hscn_structure* structure, int flags, void* stream_) {
  if (flags & ~(HSCN_STORE_F16 | HSCN_GRAD_ACCUMULATE)) return HSCN_E_BADARG;
  return ((flags & HSCN_STORE_F16) ? hscn_resident_f16().train_step : impl_resident_train_step<float>)(
      x_local, ei_ll, E_ll, lptr, eptr_ll, N, B, F, H, L, C, head_act, layer_params_host, W1, b1, W2, b2, max_n,
      max_ell, target, loss_kind, pred, score, partials, grads, acts, sync, flag, job, structure, flags, stream_);
}

}  // extern "C"
