// engine_run.hip -- C ABI (include/admm_engine.h), part 2: run() = admm.m:252-767.  The entry point with its prologue
// (option checks, histories, start iterates, objective wiring, kernel argument blocks), what every loop shares (the CG
// x-solve, the control-block poll, B, the epilogue) and the setters.  The loops themselves: engine_run_general.hip,
// engine_run_tv.hip, engine_run_consensus.hip.
#include "engine_internal.h"

#include <array>

namespace admm {

static int cg_apply(admm_engine* e, const double* v, const double** qin, int32_t* nchunk, int64_t* ldq) {
  if (e->problem == ADMM_PROB_TV2D) {  // operator I + rho*D'D: the stencil part here, the identity via shift = 1
    TimerScope ts(e, ADMM_K_GEMV_N);
    launch_tv2d_laplace(e->tv2_H, e->tv2_W, e->last_opts.rho, v, e->cg_tmp, e->ctrl, e->stream);
    *qin = e->cg_tmp;
    *nchunk = 1;
    *ldq = 0;
    return ADMM_OK;
  }
  const Ctrl* sk = e->cg_skip;  // no-ops once this solve has converged (or the run has stopped)
  if (e->sparse) {  // D'(D v) as two sparse products, each row summed in its fixed order (spmv.hip)
    {
      TimerScope ts(e, ADMM_K_GEMV_N);
      launch_spmv(e->sp.n, v, e->tmpA, sk, e->stream);
    }
    {
      TimerScope ts(e, ADMM_K_GEMV_T);
      launch_spmv(e->sp.t, e->tmpA, e->cg_tmp, sk, e->stream);
    }
    *qin = e->cg_tmp;
    *nchunk = 1;
    *ldq = 0;
    return ADMM_OK;
  }
  {
    TimerScope ts(e, ADMM_K_GEMV_N);
    launch_gemv_n(e->planDN, e->D, v, e->partDN, sk, e->stream);
  }
  launch_sum_partials(e->partDN, e->planDN.nchunk, e->planDN.ldy, e->m, e->tmpA, sk, e->stream);
  {
    TimerScope ts(e, ADMM_K_GEMV_T);
    launch_gemv_t(e->planDT, e->D, e->tmpA, nullptr, nullptr, 1, e->partDT, sk, e->stream);
  }
  *qin = e->partDT;
  *nchunk = e->planDT.nchunk;
  *ldq = e->planDT.ldg;
  if (e->comm && comm_nranks(e->comm) > 1) {  // sum_g D_g'(D_g v): n doubles per inner iteration
    launch_sum_partials_t(e->planDT, e->partDT, 1, e->cg_tmp, round_up(e->n, 2), e->ctrl, e->stream);
    ADMM_TRY(comm_allreduce_device(e->comm, e->cg_tmp, static_cast<size_t>(e->n), e->stream));
    *qin = e->cg_tmp;
    *nchunk = 1;
    *ldq = 0;
  }
  return ADMM_OK;
}

// x <- solve of (D'D + shift I) x = y by warm-started CG (cg.hip); one poll of the device per solve
int cg_solve(admm_engine* e, const double* y) {
  if (e->problem == ADMM_PROB_TV2D) return cg_solve_tv2d(e, y);
  CgArgs a{};
  a.n = e->n;
  a.shift = e->cg_shift_is_rho ? e->last_opts.rho : 0.0;
  a.tol = e->cg_tol;
  a.maxit = e->cg_maxit;
  a.y = y;
  a.x = e->x;
  a.r = e->cg_r;
  a.p = e->cg_p;
  a.q = e->cg_q;
  a.part = e->cg_part;
  a.st = e->cg_st;
  a.ctrl = e->ctrl;
  a.skip = &e->cg_skip->stop;
  // clear iters/done of the previous solve (total keeps counting) and re-arm the operator kernels
  ADMM_HIP_TRY(hipMemsetAsync(&e->cg_st->iters, 0, 2 * sizeof(int32_t), e->stream));
  ADMM_HIP_TRY(hipMemsetAsync(&e->cg_skip->stop, 0, sizeof(int32_t), e->stream));
  const double* qin;
  int32_t nchunk;
  int64_t ldq;
  ADMM_TRY(cg_apply(e, e->x, &qin, &nchunk, &ldq));
  CgArgs a0 = a;
  a0.p = e->x;  // q = D'D x + shift*x
  launch_cg_q(a0, qin, nchunk, ldq, false, e->stream);
  launch_cg_init(a, e->stream);
  // everything enqueued after convergence is a no-op (operator kernels included), so a chunk can be as long as
  // the previous solve was: one or two polls of the device per solve instead of one per 4 iterations
  const int chunk = e->cg_chunk;
  for (int done_it = 0; done_it < e->cg_maxit;) {
    const int k = (e->cg_maxit - done_it < chunk) ? e->cg_maxit - done_it : chunk;
    for (int c = 0; c < k; ++c) {
      ADMM_TRY(cg_apply(e, e->cg_p, &qin, &nchunk, &ldq));
      launch_cg_q(a, qin, nchunk, ldq, true, e->stream);
      launch_cg_step_tail(a, e->stream);
    }
    done_it += k;
    ADMM_HIP_TRY(hipMemcpyAsync(e->cg_st_host, e->cg_st, sizeof(CgState), hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->cg_st_host->done || e->ctrl_host->stop) break;
  }
  e->cg_chunk = std::min(64, std::max(4, static_cast<int>(e->cg_st_host->iters) + 2));
  return ADMM_OK;
}

// e->ctrl_host <- the device's control block, once everything enqueued so far has run
int poll_ctrl(admm_engine* e) {
  ADMM_HIP_TRY(hipMemcpyAsync(e->ctrl_host, e->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  return ADMM_OK;
}

// End of a run: launch errors, kernel timers, the summary with the objective at the last executed iteration
// (admm.m:752-754).  e->ctrl_host holds the device's final control block.
int finish_run(admm_engine* e, const admm_options& o, int32_t N, double runtime, admm_run_summary* summary) {
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(ADMM_E_DEVICE, std::string("kernel launch: ") + hipGetErrorString(le));
  if (e->profiling) collect_timers(e);
  const int32_t steps = e->ctrl_host->steps;
  e->last = admm_run_summary{};
  e->last.steps = steps;
  e->last.stopped_early = (steps < N) ? 1 : 0;
  e->last.convtest_failed_at = e->ctrl_host->convfail;
  e->last.runtime_s = runtime;
  e->last.objopt = NAN;
  if (o.objevals && steps > 0) {
    double v = NAN;
    ADMM_HIP_TRY(hipMemcpy(&v, e->objv + (steps - 1), sizeof(double), hipMemcpyDeviceToHost));
    e->last.objopt = v;
  }
  e->has_run = true;
  if (summary) *summary = e->last;
  return ADMM_OK;
}

admm_comm* engine_comm(admm_engine* e) { return e ? e->comm : nullptr; }

// w[len] = -B*z[nBz]   (admm.m:536 Bz = B(z); the loop carries w so that B = -1 is the identity)
int apply_b(admm_engine* e, const double* zin, double* wout) {
  if (e->bcb) {
    if (e->bcb(e->buser, zin, e->nBz, e->btmp, e->len, static_cast<void*>(e->stream)) != 0)
      return fail(ADMM_E_INVALID, "the B operator callback reported a failure");
    launch_combine(e->btmp, 1, 0, -1.0, nullptr, 0.0, nullptr, wout, e->len, e->ctrl, e->stream);
  } else if (e->Bmat) {
    launch_gemv_n(e->planBN, e->Bmat, zin, e->partBN, e->ctrl, e->stream);
    launch_combine(e->partBN, e->planBN.nchunk, e->planBN.ldy, -1.0, nullptr, 0.0, nullptr, wout, e->len, e->ctrl,
                   e->stream);
  } else {
    launch_combine(zin, 1, 0, -e->bscalar, nullptr, 0.0, nullptr, wout, e->len, e->ctrl, e->stream);
  }
  return ADMM_OK;
}

// ---- the prologue of admm_engine_run, one job each

static int check_run_options(admm_engine* e, const admm_options* opts, admm_options& o) {
  if (!e || !opts) return fail(ADMM_E_INVALID, "engine/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_options)))
    return fail(ADMM_E_INVALID, "admm_options.struct_size mismatch (ABI version skew)");
  ADMM_HIP_TRY(hipSetDevice(e->device));
  o = *opts;
  if (!(o.rho > 0.0)) return fail(ADMM_E_INVALID, "options.rho must be positive");
  if (o.maxiters <= 0) o.maxiters = 1000;  // admm.m:334-339
  if (o.restart <= 0.0 || o.restart >= 1.0) o.restart = 0.999;  // admm.m:285-287
  if (o.fast != ADMM_FAST_OFF && o.fast != ADMM_FAST_WEAK && o.fast != ADMM_FAST_STRONG)
    return fail(ADMM_E_INVALID, "bad options.fast");
  if (o.rho != e->rho_factor && !o.stale_factor_ok && (e->F || e->has_zfac || e->Kmat) && e->problem != ADMM_PROB_LAD && e->problem != ADMM_PROB_HUBERFIT &&
      e->problem != ADMM_PROB_LINEARSVM)
    return fail(ADMM_E_INVALID, "options.rho differs from the rho the cached factor was built for");
  if (e->problem == ADMM_PROB_LASSO_CONSENSUS && o.rho != e->rho_factor)
    return fail(ADMM_E_INVALID, "options.rho differs from the rho the cached slice factors were built for");
  if (e->xsolve == ADMM_XSOLVE_CALLBACK && !e->xcb)
    return fail(ADMM_E_INVALID, "this engine was created with xsolve=callback: set the xminf callback before running");
  if (!e->a_identity && !e->D && e->axbuf && (!e->acb || !e->atcb))
    return fail(ADMM_E_INVALID, "this engine has no constraint matrix: set the A and At operator callbacks "
                                "(admm_engine_set_operators) before running");
  if (o.relax != 1.0 && (e->problem == ADMM_PROB_LINEARSVM))
    return fail(ADMM_E_INVALID,
                "relaxation with the linear SVM prox is a dimension error in the reference (getProxOps.m:1088)");
  // (relaxation with LAD / Huber: lad.m:124-126 switches to the userelax closures, which take Axhat directly: same
  // fused formula, nothing to check)
  if (e->problem == ADMM_PROB_MODEL) {
    if (!e->has_xfac && !e->xcb)
      return fail(ADMM_E_INVALID, "no x-update: the model was created without PtP/Ptr and no xminf callback is set");
    if (!e->has_zfac && !e->zcb)
      return fail(ADMM_E_INVALID, "no z-update: the model was created without QtQ/Qts and no zming callback is set");
  }
  if (e->bgen && !(e->xcb && e->zcb))
    return fail(ADMM_E_INVALID, "an engine with a general B needs both the xminf and the zming callback");
  e->last_opts = o;
  return ADMM_OK;
}

static std::array<double**, 9> scalar_histories(admm_engine* e) {
  return {&e->pnorm, &e->dnorm, &e->perr, &e->derr, &e->objv, &e->hnorm, &e->avals, &e->dvals, &e->restarted};
}

// (a run with the shape of the previous one keeps its buffers: hipFree synchronises the device and nine hipMallocs
// cost ~0.1 ms -- 7 % of a 20-iteration run of the headline loop)
static int prepare_histories(admm_engine* e, const admm_options& o, int alg) {
  const int64_t len = e->len, nA = e->nA;
  const int32_t N = o.maxiters;
  const bool same_shape = e->hist_cap == N && e->hist_cap > 0 && e->hist_vectors == (o.record_history != 0) &&
                          e->hist_fast == (alg != 0) && e->hist_bgen == e->bgen && e->pnorm != nullptr;
  if (!same_shape) free_hist(e);
  e->hist_cap = N;
  e->hist_vectors = o.record_history != 0;
  e->hist_fast = alg != 0;
  e->hist_bgen = e->bgen;
  if (!same_shape && e->hist_vectors) {
    ADMM_TRY(hist_alloc(e, &e->xhist, static_cast<size_t>(nA) * N));
    ADMM_TRY(hist_alloc(e, &e->zhist, static_cast<size_t>(len) * N));
    ADMM_TRY(hist_alloc(e, &e->uhist, static_cast<size_t>(len) * N));
    if (alg != 0) {
      ADMM_TRY(hist_alloc(e, &e->vhist, static_cast<size_t>(len) * N));
      ADMM_TRY(hist_alloc(e, &e->uhathist, static_cast<size_t>(len) * N));
    }
    if (e->bgen) {  // results.zvals / vvals hold the caller's z (nB elements), not w = -B*z
      ADMM_TRY(hist_alloc(e, &e->zthist, static_cast<size_t>(e->nBz) * N));
      if (alg != 0) ADMM_TRY(hist_alloc(e, &e->vthist, static_cast<size_t>(e->nBz) * N));
    }
  }
  for (double** p : scalar_histories(e))
    if (!same_shape) ADMM_TRY(hist_alloc(e, p, N));
  return ADMM_OK;
}

// the start iterates (admm.m:252-254, 269-270), zeroed scalar histories, the control block; timers and CG state reset
static int start_iterates(admm_engine* e, const admm_options& o) {
  const int64_t len = e->len, nA = e->nA;
  const int32_t N = o.maxiters;
  const auto scal = scalar_histories(e);
  Ctrl c0{};
  c0.acurr = 1.0;
  c0.aprev = 1.0;
  c0.d = INFINITY;
  c0.dprev = INFINITY;
  *e->ctrl_host = c0;
  if (!o.x0 && !o.z0 && !o.u0 && !e->bgen) {
    // zero start (admm.m:252-254): the iterates, v = z, uhat = u (admm.m:269-270), the nine scalar histories and the
    // control block in ONE launch -- fifteen memset / memcpy calls cost ~60 us of host time per run, the price of
    // four iterations of a 20-iteration run of the headline loop
    RunInitArgs ia{};
    ia.x = e->x;
    ia.nA = nA;
    ia.z = e->z;
    ia.u = e->u;
    ia.v = e->v;
    ia.uhat = e->uhat;
    ia.len = len;
    static_assert(sizeof(ia.scal) / sizeof(ia.scal[0]) == std::tuple_size<decltype(scalar_histories(e))>::value,
                  "RunInitArgs::scal holds one slot per scalar history");
    int k = 0;
    for (double** p : scal) ia.scal[k++] = *p;
    ia.N = N;
    ia.ctrl = e->ctrl;
    ia.c0 = c0;
    launch_run_init(ia, e->stream);
  } else {
    for (double** p : scal) ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * N, e->stream));
    // ---- initial iterates (admm.m:252-254) and control block
    auto init_vec = [&](double* dst, const double* src, int64_t cnt) -> int {
      if (src) ADMM_HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice, e->stream));
      else ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * cnt, e->stream));
      return ADMM_OK;
    };
    ADMM_TRY(init_vec(e->x, o.x0, nA));
    if (e->bgen) ADMM_TRY(init_vec(e->zt, o.z0, e->nBz));
    else ADMM_TRY(init_vec(e->z, o.z0, len));
    ADMM_TRY(init_vec(e->u, o.u0, len));
    ADMM_HIP_TRY(hipMemcpyAsync(e->v, e->z, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));     // admm.m:269
    ADMM_HIP_TRY(hipMemcpyAsync(e->uhat, e->u, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));  // admm.m:270
    ADMM_HIP_TRY(hipMemcpyAsync(e->ctrl, e->ctrl_host, sizeof(Ctrl), hipMemcpyHostToDevice, e->stream));
  }
  if (e->bgen) {  // w0 = -B*z0; v starts as z (admm.m:269)
    ADMM_TRY(apply_b(e, e->zt, e->z));
    ADMM_HIP_TRY(hipMemcpyAsync(e->v, e->z, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));
    ADMM_HIP_TRY(hipMemcpyAsync(e->vt, e->zt, sizeof(double) * e->nBz, hipMemcpyDeviceToDevice, e->stream));
    ADMM_HIP_TRY(hipMemcpyAsync(e->ztprev, e->zt, sizeof(double) * e->nBz, hipMemcpyDeviceToDevice, e->stream));
  }
  if (o.x0 || o.z0 || o.u0 || e->bgen) ADMM_HIP_TRY(hipStreamSynchronize(e->stream));  // (host buffers were read)
  for (auto& t : e->timers) {
    t.used = 0;
    t.total_ms = 0.0;
    t.launches = 0;
  }
  if (e->cg_st) ADMM_HIP_TRY(hipMemsetAsync(e->cg_st, 0, sizeof(CgState), e->stream));
  return ADMM_OK;
}

// objective wiring (solver-supplied handles: lasso.m:227, lad.m:148, huberfit.m:180, linearsvm.m:231-236,
// quadraticprogram.m:242, basispursuit.m:140)
static int wire_objective(admm_engine* e, const admm_options& o, ProxArgs& pa, FinArgs& fa, ObjForm& obj) {
  fa.obj_scale_part = 0.0;
  pa.objz = OBJZ_NONE;
  pa.objx = OBJX_NONE;
  if (o.objevals && e->ocb) {  // options.obj is the caller's handle (admm.m:603-605)
    fa.obj_scale_part = 1.0;
  } else if (o.objevals) {
    switch (e->problem) {
      case ADMM_PROB_LASSO:
        if (!e->s)
          return fail(ADMM_E_INVALID, "objevals on a lasso engine created from args.Dts alone: the objective "
                                      "0.5*||D*x - s||^2 (lasso.m:227) needs s (or an objective callback)");
        obj.obj_lasso_gemv = true;
        fa.obj_scale_part = 0.5;  // (the Gram form sets its own scale and constant per iteration)
        pa.objz = OBJZ_ABS;
        fa.obj_scale_z = e->lambda;
        break;
      case ADMM_PROB_LAD:
        pa.objz = OBJZ_ABS;
        fa.obj_scale_z = 1.0;
        break;
      case ADMM_PROB_HUBERFIT:
        pa.objz = OBJZ_HUBER;
        fa.obj_scale_z = 0.5;
        break;
      case ADMM_PROB_LINEARSVM:
        // (ADMM_LOSS_SQHINGE always runs the cost form, which sums its own objective: any value but OBJX_NONE asks for it)
        pa.objx = (e->loss == ADMM_LOSS_HINGE)      ? OBJX_HINGE
                  : (e->loss == ADMM_LOSS_LOGISTIC) ? OBJX_LOGISTIC
                                                    : OBJX_ZEROONE;  // linearsvm.m:231-237
        fa.obj_scale_x = e->C;
        fa.obj_half_xnorm = 0.5;
        break;
      case ADMM_PROB_QP_BOUNDED:
      case ADMM_PROB_QP_STANDARD:
        obj.obj_qp_gemv = true;
        fa.obj_scale_part = 1.0;
        fa.obj_const = e->rconst;
        break;
      case ADMM_PROB_LINEARPROGRAM:  // b'*x   (linearprogram.m:178)
        pa.objx = OBJX_DOT;
        fa.obj_scale_x = 1.0;
        break;
      case ADMM_PROB_BASISPURSUIT:
        pa.objx = OBJX_ABS;
        fa.obj_scale_x = 1.0;
        break;
      case ADMM_PROB_COVSEL:  // trace(S*x) - log(det(x)) + lambda*norm(z(:),1)   (covarianceselection.m:169)
        pa.objx = OBJX_DOT;   // sum S_ij X_ij = trace(S*X): X is symmetric
        fa.obj_scale_x = 1.0;
        pa.objz = OBJZ_ABS;
        fa.obj_scale_z = e->lambda;
        obj.obj_covsel = true;  // -log det X = -sum log f(lambda_i), from the x-update's own eigenvalues (q27)
        fa.obj_scale_part = 1.0;
        break;
      case ADMM_PROB_MODEL:  // 1/2||P*x - r||^2 + 1/2||Q*z - s||^2   (model.m:133-134)
        if (!e->D || !e->D2)
          return fail(ADMM_E_INVALID, "objevals on the model problem needs the matrices P, Q and vectors r, s "
                                      "(or an objective callback)");
        obj.obj_model_gemv = true;
        fa.obj_scale_part = 0.5;
        break;
      default:
        break;
    }
  }
  return ADMM_OK;
}

// the static parts of the kernel argument blocks
static void fill_arg_blocks(admm_engine* e, const admm_options& o, int alg, bool use_h, bool split_z, ProxArgs& pa,
                            FinArgs& fa, ExtrapArgs& xa) {
  const int64_t len = e->len, nA = e->nA;
  const int32_t N = o.maxiters;
  pa.len = len;
  pa.c = e->c;
  pa.ell = e->ell;
  pa.lb = e->lb;
  pa.ub = e->ub;
  pa.z = e->z;
  pa.u = e->u;
  pa.uhat = e->uhat;
  pa.v = e->v;
  pa.zprev = e->zprev;
  pa.uprev = e->uprev;
  pa.dz = e->dz;
  pa.rhs = e->rhs;
  pa.rhs_add = e->rhs_add;
  pa.zhist = e->zhist;
  pa.uhist = e->uhist;
  pa.xhist = e->a_identity ? e->xhist : nullptr;
  pa.vhist = e->vhist;
  pa.uhathist = e->uhathist;
  pa.part = e->part;
  pa.rho = o.rho;
  pa.rho_solve = e->rho_factor;
  pa.relax = o.relax;
  pa.prox = split_z ? PROX_GIVEN : e->prox;
  pa.zgiven = e->zext;
  pa.rhs_kind = e->xcb ? RHS_NONE : e->rhs_kind;
  pa.alg = alg;
  pa.a_identity = e->a_identity ? 1 : 0;
  switch (e->prox) {
    case PROX_SOFT:
      pa.t = (e->problem == ADMM_PROB_LASSO || e->problem == ADMM_PROB_COVSEL) ? e->lambda / o.rho
                                                                              : 1.0 / o.rho;  // getProxOps.m:455, 750 | 810, 142
      break;
    case PROX_HINGE:
    case PROX_LOGISTIC:
      pa.t = e->C / o.rho;  // getProxOps.m:1096
      break;
    case PROX_01:
      pa.t = o.rho / e->C;  // getProxOps.m:1100
      break;
    default:
      pa.t = 0.0;
      break;
  }

  fa.len = len;
  fa.nA = nA;
  fa.part = e->part;
  fa.g = e->a_identity ? nullptr : e->g;
  fa.ldg = e->ldg;
  fa.x = e->a_identity ? nullptr : e->x;
  fa.xhist = e->a_identity ? nullptr : e->xhist;
  fa.cnorm = e->cnorm;
  fa.rho = o.rho;
  fa.rhoH = o.rho;
  fa.abstol = o.abstol;
  fa.reltol = o.reltol;
  fa.Hnormtol = o.Hnormtol;
  fa.convtol = o.convtol;
  fa.restart = o.restart;
  fa.dvaltol = o.dvaltol;
  fa.alg = alg;
  fa.a_identity = pa.a_identity;
  fa.nodualerror = o.nodualerror;
  fa.objevals = o.objevals;
  fa.use_h = use_h ? 1 : 0;
  fa.convtest = o.convtest;
  fa.stopcond = o.stopcond;
  fa.domaxiters = o.domaxiters;
  fa.maxiters = N;
  fa.pnorm = e->pnorm;
  fa.dnorm = e->dnorm;
  fa.perr = e->perr;
  fa.derr = e->derr;
  fa.objv = e->objv;
  fa.hnorm = e->hnorm;
  fa.avals = e->avals;
  fa.dvals = e->dvals;
  fa.restarted = e->restarted;
  fa.ctrl = e->ctrl;

  xa.len = len;
  xa.z = e->z;
  xa.u = e->u;
  xa.zprev = e->zprev;
  xa.uprev = e->uprev;
  xa.c = e->c;
  xa.v = e->v;
  xa.uhat = e->uhat;
  xa.rhs = e->rhs;
  xa.rhs_add = e->rhs_add;
  xa.vhist = e->vhist;
  xa.uhathist = e->uhathist;
  xa.rho = o.rho;
  xa.rhs_kind = e->xcb ? RHS_NONE : e->rhs_kind;
}

// The device copy of a setter's weight vector (host == null: none) into *slot, the last step of a call that has
// validated everything else: upload, synchronise, free the old copy, store -- a refused call has changed nothing.
static int replace_device_weights(admm_engine* e, double** slot, const double* host, int64_t len) {
  ADMM_HIP_TRY(hipSetDevice(e->device));
  double* w = nullptr;
  if (host) {
    ADMM_TRY(e->mem.alloc(&w, static_cast<size_t>(len)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, host, sizeof(double) * len, hipMemcpyHostToDevice, e->stream));
  }
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));  // (the caller's weights are read until here; no run uses the old ones)
  if (*slot) e->mem.free_one(*slot);
  *slot = w;
  return ADMM_OK;
}

}  // namespace admm

extern "C" {

int admm_engine_set_callbacks(admm_engine* e, admm_prox_callback xmin, void* xuser, admm_prox_callback zmin,
                              void* zuser, admm_obj_callback obj, void* objuser) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  const bool a1 = e->problem == ADMM_PROB_MODEL || e->problem == ADMM_PROB_QP_BOUNDED ||
                  e->problem == ADMM_PROB_BASISPURSUIT || e->problem == ADMM_PROB_LINEARPROGRAM ||
                  e->problem == ADMM_PROB_QP_STANDARD || (e->problem == ADMM_PROB_LASSO && !e->fat);
  const bool ad = e->problem == ADMM_PROB_LAD || e->problem == ADMM_PROB_HUBERFIT || e->problem == ADMM_PROB_LINEARSVM;
  if ((xmin || zmin || obj) && !((a1 || ad) && e->xsolve != ADMM_XSOLVE_CG))
    return fail(ADMM_E_UNSUPPORTED,
                "prox callbacks are supported for the A = 1 problems (model/generic, tall lasso, QP, LP, basis pursuit) "
                "and the A = D problems (LAD, Huber, linear SVM / unwrapped ADMM) with a cached-factor x-solve");
  if ((xmin || zmin || obj) && e->comm && comm_nranks(e->comm) > 1)
    return fail(ADMM_E_UNSUPPORTED, "prox callbacks are not supported on row-sharded engines");
  ADMM_HIP_TRY(hipSetDevice(e->device));
  const int64_t n2 = round_up(e->len, 2);
  if (!e->xext) ADMM_TRY(e->mem.alloc(&e->xext, round_up(e->nA, 2)));
  if (!e->zext) ADMM_TRY(e->mem.alloc(&e->zext, n2));
  if (!e->xh) ADMM_TRY(e->mem.alloc(&e->xh, n2));
  e->xcb = xmin;
  e->xuser = xuser;
  e->zcb = zmin;
  e->zuser = zuser;
  e->ocb = obj;
  e->ouser = objuser;
  return ADMM_OK;
}

int admm_engine_set_hooks(admm_engine* e, admm_altu_callback altu, void* altu_user, admm_norms_callback norms,
                          void* norms_user) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (altu || norms) {
    if (e->problem == ADMM_PROB_LASSO_CONSENSUS || e->problem == ADMM_PROB_TOTALVARIATION || e->problem == ADMM_PROB_TV2D)
      return fail(ADMM_E_UNSUPPORTED, "caller-supplied options.altu / options.specialnorms: not for the consensus-lasso "
                                      "and total-variation loops (consensus lasso's own hooks are engine-native)");
    if (e->comm && comm_nranks(e->comm) > 1)
      return fail(ADMM_E_UNSUPPORTED, "caller-supplied options.altu / options.specialnorms are not supported on "
                                      "row-sharded engines");
    ADMM_HIP_TRY(hipSetDevice(e->device));
    const int64_t n2 = round_up(e->len, 2);
    if (!e->xh) ADMM_TRY(e->mem.alloc(&e->xh, n2));
    if (!e->hk_uold) {
      ADMM_TRY(e->mem.alloc(&e->hk_uold, n2));
      ADMM_TRY(e->mem.alloc(&e->hk_bz, n2));
      ADMM_TRY(e->mem.alloc(&e->hk_unew, n2));
      ADMM_TRY(e->mem.alloc(&e->hk_zero, n2));
      ADMM_TRY(e->mem.alloc(&e->hk_norms, 2));
      ADMM_HIP_TRY(hipMemsetAsync(e->hk_zero, 0, sizeof(double) * n2, e->stream));
    }
  }
  e->altucb = altu;
  e->altuuser = altu_user;
  e->normscb = norms;
  e->normsuser = norms_user;
  return ADMM_OK;
}

int admm_engine_set_operators(admm_engine* e, admm_operator_callback A, void* Auser, admm_operator_callback At,
                              void* Atuser) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (e->D || e->a_identity || e->xsolve != ADMM_XSOLVE_CALLBACK)
    return fail(ADMM_E_UNSUPPORTED, "operator callbacks belong to an engine created without a matrix "
                                    "(ADMM_PROB_LAD, ADMM_XSOLVE_CALLBACK, desc.D = NULL)");
  e->acb = A;
  e->auser = Auser;
  e->atcb = At;
  e->atuser = Atuser;
  return ADMM_OK;
}

int admm_engine_set_constraint_b(admm_engine* e, const double* B, int64_t ldB, int64_t nB, int32_t memkind,
                                 double scalar, admm_operator_callback Bop, void* Buser) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  const bool generic = (e->problem == ADMM_PROB_MODEL && !e->has_xfac && !e->has_zfac) ||
                       (e->problem == ADMM_PROB_LAD && e->xsolve == ADMM_XSOLVE_CALLBACK);
  if (!generic)
    return fail(ADMM_E_UNSUPPORTED, "a general B belongs to an engine whose two prox operators are both the caller's "
                                    "(the library's operators are written for B = -1)");
  if (e->comm && comm_nranks(e->comm) > 1) return fail(ADMM_E_UNSUPPORTED, "a general B is not supported on row-sharded engines");
  if (e->bgen && Bop && e->bcb && nB == e->nBz) {  // a fresh thunk for the same operator (host bindings re-create them per run)
    e->bcb = Bop;
    e->buser = Buser;
    return ADMM_OK;
  }
  if (e->bgen) return fail(ADMM_E_INVALID, "the constraint operator B of this engine is already set");
  const int64_t len = e->len;
  if (!Bop && !B) {  // a scalar: B = scalar*I, z has as many elements as the constraint
    if (nB != 0 && nB != len) return fail(ADMM_E_INVALID, "a scalar B needs nB equal to the constraint length m");
    nB = len;
  } else if (nB <= 0) {
    return fail(ADMM_E_INVALID, "nB (the length of z) must be positive");
  }
  if (B && !Bop && ldB < len) ldB = len;
  ADMM_HIP_TRY(hipSetDevice(e->device));
  const int64_t np = round_up(nB, 64) + 64;  // the streaming kernels read whole 16-byte pairs
  for (double** p : {&e->zt, &e->ztprev, &e->ztnew, &e->vt}) {
    ADMM_TRY(e->mem.alloc(p, np));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * np, e->stream));
  }
  ADMM_TRY(e->mem.alloc(&e->btmp, round_up(len, 2)));
  if (Bop) {
    e->bcb = Bop;
    e->buser = Buser;
  } else if (B) {
    ADMM_TRY(upload_matrix(e->mem, &e->Bmat, &e->ldB, B, len, nB, ldB, memkind, e->stream));
    e->planBN = gemv_n_plan(len, nB, e->ldB);
    ADMM_TRY(e->mem.alloc(&e->partBN, e->planBN.part_elems()));
  }
  e->bscalar = scalar;
  e->nBz = nB;
  e->bgen = true;
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  return ADMM_OK;
}

int admm_engine_set_groups(admm_engine* e, const int64_t* sizes, int32_t ngroups, const double* weights) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (ngroups < 0) return fail(ADMM_E_INVALID, "groups: a negative group count");
  if (e->problem != ADMM_PROB_LASSO)
    return fail(ADMM_E_UNSUPPORTED, "groups belong to the serial lasso (ADMM_PROB_LASSO): the block soft threshold "
                                    "replaces its l1 prox");
  if (e->comm) return fail(ADMM_E_UNSUPPORTED, "groups are not supported on row-sharded engines");
  GroupPlanHost h;
  const bool on = sizes && ngroups > 0;
  if (on) ADMM_TRY(group_plan_build(sizes, ngroups, weights, e->len, &h));  // (a refused call changes nothing)
  ADMM_HIP_TRY(hipSetDevice(e->device));
  if (e->grp_blob) {
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    e->mem.free_one(e->grp_blob);
    e->grp_blob = nullptr;
  }
  e->ngroups = 0;
  e->grp = GroupPlan{};
  if (!on) return ADMM_OK;
  ADMM_TRY(e->mem.alloc(&e->grp_blob, h.blob.size()));
  ADMM_HIP_TRY(hipMemcpyAsync(e->grp_blob, h.blob.data(), sizeof(double) * h.blob.size(), hipMemcpyHostToDevice, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));  // (h is read until here)
  e->grp = h.bind(e->grp_blob);
  e->ngroups = ngroups;
  return ADMM_OK;
}

int admm_engine_set_penalty(admm_engine* e, const admm_penalty_desc* d) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (e->problem != ADMM_PROB_LASSO)
    return fail(ADMM_E_UNSUPPORTED, "the penalty family belongs to the serial lasso (ADMM_PROB_LASSO): it replaces the "
                                    "l1 prox of its z-update");
  if (e->comm) return fail(ADMM_E_UNSUPPORTED, "the penalty family is not supported on row-sharded engines");
  if (d) {  // (a refused call changes nothing)
    if (!finite_nonneg(d->l1)) return fail(ADMM_E_INVALID, "penalty: l1 must be finite and >= 0");
    if (!finite_nonneg(d->ridge)) return fail(ADMM_E_INVALID, "penalty: ridge must be finite and >= 0");
    if (d->nonnegative != 0 && d->nonnegative != 1) return fail(ADMM_E_INVALID, "penalty: nonnegative must be 0 or 1");
    if (d->l1weights)
      for (int64_t i = 0; i < e->len; ++i)
        if (!finite_nonneg(d->l1weights[i]))
          return fail(ADMM_E_INVALID, "penalty: l1 weight " + std::to_string(i) + " is negative or not finite");
  }
  ADMM_TRY(replace_device_weights(e, &e->pen_w, d ? d->l1weights : nullptr, e->len));
  e->pen_l1 = d ? d->l1 : 0.0;
  e->pen_ridge = d ? d->ridge : 0.0;
  e->pen_nonneg = d ? d->nonnegative : 0;
  return ADMM_OK;
}

int admm_engine_get_penalty(admm_engine* e, admm_penalty_desc* out, int32_t* has_l1weights) {
  if (!e || !out) return fail(ADMM_E_INVALID, "NULL argument");
  out->l1weights = nullptr;
  out->l1 = e->pen_l1;
  out->ridge = e->pen_ridge;
  out->nonnegative = e->pen_nonneg;
  if (has_l1weights) *has_l1weights = e->pen_w ? 1 : 0;
  return ADMM_OK;
}

int admm_engine_set_loss(admm_engine* e, const admm_loss_desc* d) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (e->problem != ADMM_PROB_LAD && e->problem != ADMM_PROB_HUBERFIT)
    return fail(ADMM_E_INVALID, "the loss family belongs to ADMM_PROB_LAD and ADMM_PROB_HUBERFIT: it replaces the prox of "
                                "their z-update");
  if (e->comm) return fail(ADMM_E_UNSUPPORTED, "the loss family is not supported on row-sharded engines");
  if (e->xsolve == ADMM_XSOLVE_CALLBACK)
    return fail(ADMM_E_UNSUPPORTED, "the loss family is not supported on the generic callback engine");
  if (d) ADMM_TRY(check_loss_desc(e->problem, *d, e->len));  // (a refused call changes nothing)
  ADMM_TRY(replace_device_weights(e, &e->loss_w, d ? d->weights : nullptr, e->len));
  e->loss_a = d ? d->slope_pos : 1.0;
  e->loss_b = d ? d->slope_neg : 1.0;
  e->loss_eps = d ? d->epsilon : 0.0;
  e->loss_delta = d ? d->delta : 1.0;
  return ADMM_OK;
}

int admm_engine_get_loss(admm_engine* e, admm_loss_desc* out, int32_t* has_weights) {
  if (!e || !out) return fail(ADMM_E_INVALID, "NULL argument");
  out->weights = nullptr;
  out->slope_pos = e->loss_a;
  out->slope_neg = e->loss_b;
  out->epsilon = e->loss_eps;
  out->delta = e->loss_delta;
  if (has_weights) *has_weights = e->loss_w ? 1 : 0;
  return ADMM_OK;
}

int admm_engine_set_svm_cost(admm_engine* e, const admm_svm_cost_desc* d) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (e->problem != ADMM_PROB_LINEARSVM)
    return fail(ADMM_E_INVALID, "the costs belong to ADMM_PROB_LINEARSVM: they enter the prox of its z-update");
  if (e->comm) return fail(ADMM_E_UNSUPPORTED, "the costs of the linear SVM are not supported on row-sharded engines");
  if (d) {  // (a refused call changes nothing)
    const double costs[2] = {d->cost_pos, d->cost_neg};
    ADMM_TRY(check_svm_cost(d->weights, e->len, costs, 2));
  }
  ADMM_TRY(replace_device_weights(e, &e->svm_w, d ? d->weights : nullptr, e->len));
  e->svm_cost_pos = d ? d->cost_pos : 1.0;
  e->svm_cost_neg = d ? d->cost_neg : 1.0;
  return ADMM_OK;
}

int admm_engine_get_svm_cost(admm_engine* e, admm_svm_cost_desc* out, int32_t* has_weights) {
  if (!e || !out) return fail(ADMM_E_INVALID, "NULL argument");
  out->weights = nullptr;
  out->cost_pos = e->svm_cost_pos;
  out->cost_neg = e->svm_cost_neg;
  if (has_weights) *has_weights = e->svm_w ? 1 : 0;
  return ADMM_OK;
}

int admm_engine_set_tv2d_isotropic(admm_engine* e, int32_t on) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  if (e->problem != ADMM_PROB_TV2D)
    return fail(ADMM_E_INVALID, "the isotropic norm belongs to 2-D total variation (ADMM_PROB_TV2D)");
  if (on != 0 && on != 1) return fail(ADMM_E_INVALID, "isotropic must be 0 or 1");
  e->tv2_isotropic = on;  // read by the next run (engine_run_tv.hip: run_total_variation_2d)
  return ADMM_OK;
}

int admm_engine_run(admm_engine* e, const admm_options* opts, admm_run_summary* summary) {
  RunState rs{};
  admm_options& o = rs.o;
  ADMM_TRY(check_run_options(e, opts, o));
  if (e->problem == ADMM_PROB_COVSEL) {  // every run starts its eigen-steps from V = I: no state from the previous run
    launch_jacobi_identity(e->cov_V, e->cov_ld, e->n, e->stream);
    ADMM_HIP_TRY(hipMemsetAsync(e->cov_cnt, 0, sizeof(int32_t), e->stream));
    e->cov_sweeps_host = 0;
  }
  rs.alg = o.fast;  // 0, 1 (strong), 2 (weak)
  rs.N = o.maxiters;
  rs.len = e->len;
  rs.split_z = e->zcb != nullptr || e->problem == ADMM_PROB_MODEL;  // z is computed between two kernels
  rs.check_every = o.check_every > 0 ? o.check_every : (o.domaxiters ? 64 : 8);
  const bool use_h = o.convtest || o.stopcond == ADMM_STOP_HNORM || o.stopcond == ADMM_STOP_BOTH;
  ADMM_TRY(prepare_histories(e, o, rs.alg));
  ADMM_TRY(start_iterates(e, o));
  ADMM_TRY(wire_objective(e, o, rs.pa, rs.fa, rs.obj));
  fill_arg_blocks(e, o, rs.alg, use_h, rs.split_z, rs.pa, rs.fa, rs.xa);
  if (e->problem == ADMM_PROB_LASSO_CONSENSUS) {
    ADMM_TRY(run_consensus_lasso(e, rs, summary));
    return comm_check_error(e->comm, e->stream);
  }
  if (e->problem == ADMM_PROB_TV2D) return run_total_variation_2d(e, rs, summary);
  if (e->problem == ADMM_PROB_TOTALVARIATION) return run_total_variation(e, rs, summary);
  return run_general(e, rs, summary);
}

}  // extern "C"
