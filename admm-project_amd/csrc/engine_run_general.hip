// engine_run_general.hip -- the general loop of admm_engine_run (admm.m:315-756): every problem but total variation
// and consensus lasso.  The x-update dispatch, the choice of the iteration form for a run (GeneralLoop::plan), the
// iteration sequences themselves, the batch / graph / poll loop and the calibration of the lasso objective's form.
#include "engine_internal.h"

namespace admm {
namespace {

// where the element update finds A*x: one vector, or the partial rows the x-solve / the D*x pass left for it to sum
struct AxSource {
  const double* src;
  const double* t;
  int32_t npart, tri;
  int64_t ld;
};

int factor_x_update(admm_engine* e, AxSource* ax, bool leave_partials);

// the one-block triangular solves (trsv.hip: tri1_*) leave the backward pass's partial rows to the one-launch tail
bool xsolve_tri1_partials(const admm_engine* e) {
  return e->xfac.mode == ADMM_XSOLVE_TRSV && e->xfac.trsv.one && !e->xcb && e->xsolve != ADMM_XSOLVE_CG && !e->fat &&
         (e->problem == ADMM_PROB_LASSO || e->problem == ADMM_PROB_QP_BOUNDED);
}

// the lower-triangle x-solve may hand its partial rows to the one-launch tail instead of reducing them itself
bool xsolve_has_partials(const admm_engine* e) {
  if (xsolve_tri1_partials(e)) return true;
  return e->xfac.mode == ADMM_XSOLVE_INVERSE && e->xfac.Minv && e->xfac.n >= kSymvHalfMin && !e->sy_split && !e->xcb &&
         e->xsolve == ADMM_XSOLVE_INVERSE && !e->fat &&
         (e->problem == ADMM_PROB_LASSO || e->problem == ADMM_PROB_QP_BOUNDED);
}

// one x-update (admm.m:501-511) from e->rhs into e->x, or into chunk partials for the fused consumer
int x_update(admm_engine* e, AxSource* ax, bool leave_partials) {
  TimerScope ts(e, ADMM_K_XSOLVE);
  *ax = AxSource{e->x, nullptr, 1, 0, 0};
  if (e->xcb) {  // x = xminf(x, z, u, rho), fast ADMM: xminf(x, v, uhat, rho)   (admm.m:502, 506)
    const bool fastalg = e->last_opts.fast != ADMM_FAST_OFF;
    const double* zarg = e->bgen ? (fastalg ? e->vt : e->zt) : (fastalg ? e->v : e->z);
    if (e->xcb(e->xuser, e->x, zarg, fastalg ? e->uhat : e->u, e->last_opts.rho, e->xext, e->nA,
               static_cast<void*>(e->stream)) != 0)
      return fail(ADMM_E_INVALID, "the xminf callback reported a failure");
    if (e->a_identity) {
      ax->src = e->xext;  // the fused kernel stores it into x (guarded by the device stop flag)
    } else {  // A = D: D*x follows; copy through a kernel that honours the stop flag
      launch_combine(e->xext, 1, 0, 1.0, nullptr, 0.0, nullptr, e->x, e->nA, e->ctrl, e->stream);
    }
    return ADMM_OK;
  }
  if (e->xsolve == ADMM_XSOLVE_CG) return cg_solve(e, e->a_identity ? e->rhs : e->g);
  switch (e->problem) {
    case ADMM_PROB_LASSO:
      if (!e->fat) {
        ADMM_TRY(factor_x_update(e, ax, leave_partials));
      } else {
        // getProxOps.m:1204  x = y/rho - D'*(U\(L\(D*y)))/rho^2
        launch_gemv_n(e->planDN, e->D, e->rhs, e->partDN, e->ctrl, e->stream);
        launch_sum_partials(e->partDN, e->planDN.nchunk, e->planDN.ldy, e->m, e->tmpA, e->ctrl, e->stream);
        ADMM_TRY(solve_factor(e, e->tmpA, e->tmpB));
        launch_gemv_t(e->planDT, e->D, e->tmpB, nullptr, nullptr, 1, e->partDT, e->ctrl, e->stream);
        const double rho = e->last_opts.rho;
        launch_combine(e->partDT, e->planDT.nchunk, e->planDT.ldg, -1.0 / (rho * rho), e->rhs, 1.0 / rho, nullptr,
                       e->x, e->n, e->ctrl, e->stream);
      }
      break;
    case ADMM_PROB_QP_BOUNDED:  // planSq/partSq are shared with the objective GEMV; the x-update consumes them first
    case ADMM_PROB_MODEL:
      ADMM_TRY(factor_x_update(e, ax, leave_partials));
      break;
    case ADMM_PROB_LINEARPROGRAM:
    case ADMM_PROB_QP_STANDARD:  // x = K*y + k0: the KKT solve of getProxOps.m:1363 / 1410, reduced once
      launch_gemv_t(e->planK, e->Kmat, e->rhs, nullptr, nullptr, 1, e->partK, e->ctrl, e->stream);
      launch_combine(e->partK, e->planK.nchunk, e->planK.ldg, 1.0, nullptr, 0.0, e->k0, e->x, e->n, e->ctrl,
                     e->stream);
      break;
    case ADMM_PROB_BASISPURSUIT:
      launch_gemv_t(e->planSq, e->Pmat, e->rhs, nullptr, nullptr, 1, e->partSq, e->ctrl, e->stream);
      launch_combine(e->partSq, e->planSq.nchunk, e->planSq.ldg, 1.0, nullptr, 0.0, e->q, e->x, e->n, e->ctrl,
                     e->stream);
      break;
    case ADMM_PROB_COVSEL:  // getProxOps.m:1487-1495: X = f(rho*(Z - U) - S) by a symmetric eigen-step (covsel.hip)
      if (e->n <= kCovselSmallMax) {
        CovselArgs ca{e->n, e->last_opts.rho, e->rhs, e->cov_S, e->x, e->cov_V, e->cov_ld, e->objpart, e->cov_cnt};
        launch_covsel_small(ca, e->ctrl, e->stream);
      } else {
        ADMM_TRY(covsel_large_x_update(e->cov_big, e->last_opts.rho, e->rhs, e->cov_S, e->x, e->objpart, e->ctrl,
                                       e->ctrl_host, &e->cov_sweeps_host, e->stream));
      }
      break;
    default:  // LAD / Huber / SVM: rhs already holds D'*(c + z - u) (row 0 of g)
      if (e->DplusT)  // row 0 of g is Dplus*(z - u) already (getProxOps.m:1067)
        launch_combine(e->g, 1, 0, 1.0, nullptr, 0.0, nullptr, e->x, e->nA, e->ctrl, e->stream);
      else
        ADMM_TRY(solve_factor(e, e->g, e->x));
      break;
  }
  return ADMM_OK;
}

// the cached-factor x-update shared by lasso (tall), bounded QP and the model problem
int factor_x_update(admm_engine* e, AxSource* ax, bool leave_partials) {
  if (leave_partials && xsolve_tri1_partials(e)) {  // x = sum of the backward pass's rows from the diagonal tile on
    const TrsvPlan& t = e->xfac.trsv;
    launch_tri1_pair(t, e->rhs, nullptr, e->dfin, e->dfin && e->dfin_pending, e->ctrl, e->stream);
    *ax = AxSource{t.tp1, t.tp1, t.ntile, 1, t.ldp};
    return ADMM_OK;
  }
  if (leave_partials && xsolve_has_partials(e)) {  // x = sum of these rows, taken by prox_fin_kernel
    const SliceFactor& f = e->xfac;
    if (e->dfin && f.planSy.packed)
      launch_symv_lower_fin(f.planSy, f.Minv, e->rhs, e->syN, e->syT, *e->dfin, e->dfin_pending, e->ctrl, e->stream);
    else
      launch_symv_lower(f.planSy, f.Minv, f.ldM, e->rhs, e->syN, e->syT, e->x, e->ctrl, e->stream, 0, 1, false);
    *ax = AxSource{e->syN, e->syT, f.planSy.ntile, 0, f.planSy.ldp};
    return ADMM_OK;
  }
  return solve_factor(e, e->rhs, e->x);
}

// One run of the general loop: what the lambda of the former one-function run captured, as members.
struct GeneralLoop {
  admm_engine* e;
  const admm_options& o;
  const int alg;
  const int32_t N;
  const int64_t len, nA;
  ProxArgs& pa;
  FinArgs& fa;
  ExtrapArgs& xa;
  const ObjForm obj;
  const int check_every;

  // ---- fixed for the run (plan)
  bool sharded = false, hooks = false, split_z = false;
  int nrhs_dual = 3;
  bool uw_fused = false, onepass = false, use_graph = false;
  bool alt_qp = false, alt_ok = false;
  double alt_const = 0.0;
  bool gram_guard = false, split_symv = false;
  bool grouped = false;  // group lasso: the grouped element update wherever the lasso's own runs (a zming callback wins)
  // the family a non-default setter (admm_engine_set_penalty / _set_loss / _set_svm_cost, or the squared hinge) puts in
  // force wherever the problem's own element update runs; each belongs to another problem, so at most one is planned
  ProxFamily fam{};

  // ---- may change at a batch boundary (after_batch: nothing is pending there, so the launch sequence may change)
  bool gram_now = false, gram_calibrating = false, obj_kernels = false;
  bool fuse_tail = false, defer_fin = false, defer_fin_ad = false;

  // ---- carried between iterations
  UwArgs ua{};           // .iter, .fin_pending: the two-launch unwrapped iteration's parity and its pending finalize
  OnePassArgs opa{};
  GemvTPlan op_plan{};
  FinArgs dff{};         // the finalize that rides along with a later launch (e->dfin points here while one is pending)
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int32_t gbatch = 0;
  bool polled = false;   // ctrl_host is what the device holds (nothing was enqueued since the last poll)
  std::chrono::steady_clock::time_point tstart;

  GeneralLoop(admm_engine* eng, RunState& rs)
      : e(eng), o(rs.o), alg(rs.alg), N(rs.N), len(rs.len), nA(eng->nA), pa(rs.pa), fa(rs.fa), xa(rs.xa), obj(rs.obj),
        check_every(rs.check_every), split_z(rs.split_z) {}

  int run(admm_run_summary* summary) {
    ADMM_TRY(plan());
    ADMM_TRY(prime());
    if (use_graph) ADMM_TRY(capture_graph());
    const int rc = run_batches();
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    ADMM_TRY(rc);
    return finish(summary);
  }

  int plan() {
    nrhs_dual = o.nodualerror ? 1 : 3;
    sharded = e->comm && comm_nranks(e->comm) > 1;
    hooks = e->altucb != nullptr || e->normscb != nullptr;
    grouped = e->ngroups > 0 && !split_z;
    ADMM_TRY(plan_penalty());
    plan_loss();
    plan_svm_cost();
    if (hooks && alg != 0)
      return fail(ADMM_E_UNSUPPORTED, "caller-supplied options.altu / options.specialnorms with fast ADMM: not supported "
                                      "(admm.m:614 overwrites fast ADMM's v with the norms: q5)");
    if (hooks && sharded) return fail(ADMM_E_UNSUPPORTED, "options.altu / options.specialnorms on a row-sharded engine");
    fa.norms_given = e->normscb ? e->hk_norms : nullptr;
    fa.len_global = e->len_global;
    tstart = std::chrono::steady_clock::now();  // ---- loop (admm.m:315 tic .. 756 toc)
    // The unwrapped iteration with an explicit pseudo-inverse (linear SVM, unwrappedadmm.m:76-92) runs as TWO launches per
    // iteration (unwrapped.hip) when nothing outside the fused element update is asked for: plain ADMM, no recorded dual
    // residual (unwrappedadmm.m:92 sets nodualerror), library operators, library objective, one rank.
    uw_fused = e->Dp && e->problem == ADMM_PROB_LINEARSVM && alg == 0 && o.relax == 1.0 && o.nodualerror && !sharded &&
               !hooks && !e->xcb && !e->zcb && !e->ocb;
    // One iteration = a fixed sequence of launches with iteration-independent arguments (the iteration
    // index lives in ctrl->iter), and iterations past a stop condition or past maxiters are no-ops on the
    // device, so a batch of iterations CAN be captured once into a hipGraph and replayed.  Measured on
    // MI355X / ROCm 7.x (profiles/svm_bench.py, profiles/trsv_graph_bench.py) replay is never faster than
    // eager launches on one stream -- SVM 6000x400: 23.0k vs 23.9k it/s -- so eager is the default and
    // ADMM_HIP_GRAPH=1 opts in.  Never used when collectives or host callbacks sit inside the iteration, for
    // the CG x-solve (which polls the device between inner iterations), or with event timing on
    // (hipEventElapsedTime rejects events recorded by graph nodes: "invalid resource handle").
    const int64_t heavy = std::max<int64_t>(e->m * e->n, e->nF * e->nF);
    use_graph = env_switches().graph && !sharded && e->profiling == 0 && !uw_fused && e->xsolve != ADMM_XSOLVE_CG &&
                heavy <= (int64_t{32} << 20) && !e->xcb && !e->zcb && !e->ocb && !hooks &&
                !(e->problem == ADMM_PROB_COVSEL && e->n > kCovselSmallMax);  // (host checks per sweep)
    plan_objective_form();
    plan_tail();
    return ADMM_OK;
  }

  // the penalty family.  Every field at its default leaves today's kernels in place, bit for bit; l1 is
  // read only beside groups, where lambda is the groups' weight.  The finalize takes the whole of g(z) from S_OBJZ.
  int plan_penalty() {
    const bool penalized = e->problem == ADMM_PROB_LASSO && !split_z &&
                           (e->pen_w || e->pen_ridge != 0.0 || e->pen_nonneg || (grouped && e->pen_l1 != 0.0));
    if (!penalized) return ADMM_OK;
    if (!grouped && len > int64_t{128} * kMaxPartBlocks)
      return fail(ADMM_E_UNSUPPORTED, "a penalised lasso of more than " + std::to_string(128 * kMaxPartBlocks) +
                                          " coefficients is not supported");
    const double l1 = grouped ? e->pen_l1 : e->lambda;
    PenaltyArgs& pen = fam.pen;
    fam.kind = FAM_PENALTY;
    pen.w = e->pen_w;
    pen.tau = l1 / o.rho;
    pen.kappa = o.rho / (o.rho + e->pen_ridge);
    pen.l1 = l1;
    pen.lam_group = grouped ? e->lambda : 0.0;
    pen.half_mu = 0.5 * e->pen_ridge;
    pen.nonneg = e->pen_nonneg;
    if (pa.objz == OBJZ_ABS) fa.obj_scale_z = 1.0;
    return ADMM_OK;
  }

  // the loss family.  Every field at its default leaves today's kernels in place, bit for bit; a zming
  // callback (split_z) replaces the z-update as before.  The finalize takes the whole of g(z) from S_OBJZ.
  void plan_loss() {
    const bool huber = e->problem == ADMM_PROB_HUBERFIT;
    const bool lossy = (huber || e->problem == ADMM_PROB_LAD) && !split_z &&
                       (e->loss_w || e->loss_a != 1.0 || e->loss_b != 1.0 || e->loss_eps != 0.0 || e->loss_delta != 1.0);
    if (!lossy) return;
    fam.kind = FAM_LOSS;
    fam.loss = LossArgs{e->loss_w, e->loss_a, e->loss_b, e->loss_eps, e->loss_delta, o.rho, huber ? 1 : 0, 0};
    if (pa.objz != OBJZ_NONE) fa.obj_scale_z = 1.0;
  }

  // the costs of the linear SVM.  Defaults leave today's kernels in place, bit for bit; the squared hinge
  // exists in the cost form only; a zming callback (split_z) replaces the z-update as before.  S_OBJX and its scale C in
  // the finalize stay.
  void plan_svm_cost() {
    const bool costly = e->problem == ADMM_PROB_LINEARSVM && !split_z &&
                        (e->svm_w || e->svm_cost_pos != 1.0 || e->svm_cost_neg != 1.0 || e->loss == ADMM_LOSS_SQHINGE);
    if (!costly) return;
    fam.kind = FAM_COST;
    fam.cost = SvmCostArgs{e->svm_w, e->svm_cost_pos, e->svm_cost_neg, e->C, o.rho, e->loss, 0};
  }

  void plan_objective_form() {
    // the lasso objective through the cached Gram matrix: always (obj_gram = 1), or once the calibration of the first
    // batch has shown it agrees with the literal D*x form to 1e-11 (obj_gram = 0; admm_engine.h)
    // (the form: 1/2*x'(y - rho*x) - x'D's + 1/2*s's with y the right-hand side x was solved from -- OBJX_SOLVE, summed by
    // the element update itself: no objective kernel at all, and the one-launch tail stays available with objevals = 1)
    alt_qp = obj.obj_qp_gemv && e->problem == ADMM_PROB_QP_BOUNDED && e->rhs_kind == RHS_RHO_MINUS_Q;
    alt_ok = ((obj.obj_lasso_gemv && e->rhs_kind == RHS_RHO_DTS) || alt_qp) && e->obj_alt && e->a_identity && !e->xcb &&
             e->xsolve != ADMM_XSOLVE_CG;
    alt_const = alt_qp ? e->rconst : e->half_ssq;
    gram_now = alt_ok && (!e->obj_auto || e->obj_gram_ok);
    gram_calibrating = alt_ok && e->obj_auto && !e->obj_gram_ok && !e->obj_gram_bad;
    if (use_graph || sharded) gram_calibrating = false;  // (a captured batch cannot switch; shards would have to agree)
    if (gram_now || gram_calibrating) pa.objx = alt_qp ? OBJX_SOLVE_QP : OBJX_SOLVE;
    if (gram_now) {
      fa.obj_scale_part = 0.0;
      fa.obj_scale_x = 1.0;
      fa.obj_const = alt_const;
    }
    // the cancellation bound of that form (finalize_device.h) is tracked whenever the engine chose it itself
    // (obj_gram = 0): past 1e-10 the run goes back to the literal pass at the next batch boundary (after_batch)
    gram_guard = alt_ok && e->obj_auto && !use_graph && !sharded;
    fa.obj_track_bound = (gram_guard && (gram_now || gram_calibrating)) ? 1 : 0;
    obj_kernels = o.objevals &&
                  (((obj.obj_lasso_gemv || obj.obj_qp_gemv) && !gram_now) || obj.obj_model_gemv || e->ocb);
  }

  void plan_tail() {
    // A = I iterations whose finalize depends on nothing but the prox kernel's partial sums end in ONE launch
    // (prox_fin_kernel): no accelerated-ADMM decision, no split z-update, no objective kernels behind the prox, one rank
    // ... and so do A = D iterations that record no dual residual (unwrappedadmm.m:92 sets nodualerror for the SVM):
    // without it the finalize logic needs none of the D' products that follow the prox kernel
    // (row-sharded A = I engines keep x, z, u replicated and exchange nothing per iteration unless the x-solve's tiles
    // are split over the ranks -- symv_apply's one all-reduce, before this tail: they run the same tail as one rank)
    fuse_tail = (e->a_identity || o.nodualerror) && alg != 2 && !split_z && (!sharded || e->a_identity) && !obj_kernels &&
                !hooks && len <= int64_t{128} * kMaxPartBlocks;
    // With the packed lower-triangle x-solve in front of it, the finalize logic of an A = I iteration is deferred: the
    // element update stores its block partials and ends; the next iteration's x-solve carries the finalize in one extra
    // workgroup (symv_lower_fin_kernel), where its ~6 us of serial work overlap with 60 us of streaming, and the element
    // update after that starts with the decision in ctrl.  A batch's last iteration gets a stand-alone finalize.
    // (also with the x-solve's tiles split over the ranks: symv_apply hands the same passenger to its launch)
    split_symv = sharded && e->sy_split && e->xfac.mode == ADMM_XSOLVE_INVERSE && e->xfac.Minv && !e->xcb &&
                 (e->problem == ADMM_PROB_LASSO || e->problem == ADMM_PROB_QP_BOUNDED) && !e->fat;
    defer_fin = fuse_tail && e->a_identity &&
                (((xsolve_has_partials(e) || split_symv) && e->xfac.planSy.packed) || xsolve_tri1_partials(e)) &&
                !use_graph;
    // A = D iterations without a dual residual (fuse_tail): the finalize logic leaves the element update's launch too and
    // runs as one extra workgroup of the partial-sum launch of D'*(c + z - u) that follows it (gemv.hip)
    defer_fin_ad = fuse_tail && !e->a_identity && e->D && !(e->atcb && !e->D) && !use_graph;
    // A = D iterations without a dual residual on a tall, narrow D (config 3 at MNIST's full size): ONE pass over D per
    // iteration instead of two (unwrapped.hip: ad_onepass_kernel) -- x-solve, the pass (D*x, element update, the partial
    // rows of D'*(c + z - u)), their sum with the iteration's finalize as passenger.
    onepass = fuse_tail && defer_fin_ad && !uw_fused && alg == 0 && o.relax == 1.0 && o.nodualerror && e->D &&
              !e->DplusT && !sharded && !hooks && !e->xcb && !e->zcb && !e->ocb && !e->acb && !e->atcb && !e->bgen &&
              !split_z && !use_graph && e->xsolve != ADMM_XSOLVE_CG && onepass_supported(e->m, e->n);
  }

  // D'*[t1, z - zprev, u] in one pass over D (getProxOps.m:1514; admm.m:624, 654).  With the caller's pseudo-inverse
  // (args.Dplus, linearsvm.m:185-186) row 0 is Dplus*t1 = the x-update itself (getProxOps.m:1067) and only the two
  // dual-residual products still stream D.  fin: a finalize for the first partial-sum launch to carry, or null.
  int transposed_products(int nrhs, const FinArgs* fin) {
    TimerScope ts(e, ADMM_K_GEMV_T);
    auto sum_t = [&](int nr, double* gout) {
      if (fin) launch_sum_partials_t_fin(e->planDT, e->partDT, nr, gout, e->ldg, *fin, e->ctrl, e->stream);
      else launch_sum_partials_t(e->planDT, e->partDT, nr, gout, e->ldg, e->ctrl, e->stream);
      fin = nullptr;
    };
    if (e->atcb && !e->D) {  // options.At as a function handle (admm.m:165-167): one call per right-hand side
      const double* vecs[3] = {e->rhs, e->dz, e->u};
      for (int r = 0; r < nrhs; ++r)
        if (e->atcb(e->atuser, vecs[r], len, e->g + r * e->ldg, nA, static_cast<void*>(e->stream)) != 0)
          return fail(ADMM_E_INVALID, "the At operator callback reported a failure");
    } else if (e->DplusT) {
      launch_gemv_t(e->planDT, e->DplusT, e->rhs, nullptr, nullptr, 1, e->partDT, e->ctrl, e->stream);
      sum_t(1, e->g);
      if (nrhs > 1) {
        launch_gemv_t(e->planDT, e->D, e->dz, e->u, nullptr, 2, e->partDT, e->ctrl, e->stream);
        sum_t(2, e->g + e->ldg);
      }
    } else {
      launch_gemv_t(e->planDT, e->D, e->rhs, e->dz, e->u, nrhs, e->partDT, e->ctrl, e->stream);
      sum_t(nrhs, e->g);
    }
    return ADMM_OK;
  }

  // what has to be on the stream before the first iteration
  int prime() {
    // rhs of the first x-update from the initial iterates (zx = v = z0, ux = uhat = u0)
    launch_initial_rhs(len, e->rhs_kind, o.rho, e->z, e->u, e->c, e->rhs_add, e->rhs, e->stream);
    if (uw_fused) {
      ua.D = e->D;
      ua.ldD = e->ldD;
      ua.Dp = e->Dp;
      ua.ldP = e->ldDp;
      ua.m = e->m;
      ua.n = e->n;
      ua.R = e->uwR;
      ua.nblk = e->uwnblk;
      ua.G = e->uwG;
      ua.ldg = e->uwldg;
      ua.axpart = e->uwAx;
      ua.ldax = e->uwldax;
      ua.nchunk = e->uwnchunk;
      ua.xbuf = e->uwX;
      ua.ldx = e->uwldg;
      ua.iter = 0;
      ua.fin_pending = 0;
      ua.init = 1;  // partial rows of Dplus*(z0 - u0): what the first iteration sums into its x
      launch_uw_prox(ua, pa, e->ctrl, e->stream, &fam);
      ua.init = 0;
    } else if (!e->a_identity) {
      ADMM_TRY(transposed_products(1, nullptr));
      if (sharded) ADMM_TRY(comm_allreduce_device(e->comm, e->g, static_cast<size_t>(e->ldg), e->stream));
    }
    if (gram_calibrating)
      ADMM_HIP_TRY(hipMemsetAsync(e->gobjpart + kMaxPartBlocks, 0, sizeof(double), e->stream));
    if (onepass) {
      const int nwg = onepass_workgroups(e->m);
      if (!e->opG) ADMM_TRY(e->mem.alloc(&e->opG, static_cast<size_t>(nwg) * static_cast<size_t>(e->ldg)));
      opa.D = e->D;
      opa.ldD = e->ldD;
      opa.m = e->m;
      opa.n = e->n;
      opa.x = e->x;
      opa.gpart = e->opG;
      opa.ldg = e->ldg;
      op_plan = e->planDT;
      op_plan.nchunk = nwg;
      op_plan.ldg = e->ldg;
    }
    return ADMM_OK;
  }

  int iterate() {
    if (onepass) return iterate_onepass();
    if (uw_fused) return iterate_unwrapped();
    return iterate_general();
  }

  int iterate_onepass() {
    {
      TimerScope ts(e, ADMM_K_XSOLVE);
      ADMM_TRY(solve_factor(e, e->g, e->x));  // (row 0 of g: D'*(c + z - u) of the previous pass)
    }
    int nblk = 1;
    {
      TimerScope ts(e, ADMM_K_PROX);
      pa.axsrc = nullptr;
      pa.ax_t = nullptr;
      pa.ax_tri = 0;
      pa.x_out = nullptr;
      launch_ad_onepass(opa, pa, e->ctrl, &nblk, e->stream, &fam);
    }
    dff = prox_fin_args(pa, fa);
    dff.nblk = nblk;
    TimerScope ts(e, ADMM_K_GEMV_T);
    launch_sum_partials_t_fin(op_plan, e->opG, 1, e->g, e->ldg, dff, e->ctrl, e->stream);
    return ADMM_OK;
  }

  int iterate_unwrapped() {
    TimerScope ts(e, ADMM_K_PROX);
    pa.axsrc = nullptr;
    pa.ax_t = nullptr;
    pa.x_out = nullptr;
    FinArgs fprev = fa;  // the previous iteration's finalize rides along with this iteration's first launch
    fprev.x = e->uwX + ((ua.iter + 1) & 1) * e->uwldg;
    launch_uw_ax(ua, fprev, e->ctrl, e->stream);
    launch_uw_prox(ua, pa, e->ctrl, e->stream, &fam);
    ua.iter += 1;
    ua.fin_pending = 1;
    return ADMM_OK;
  }

  int iterate_general() {
    AxSource ax{};
    ADMM_TRY(x_update_and_ax(&ax));
    if (split_z) ADMM_TRY(split_z_update(ax));
    int nblk = 1;
    bool done = false;
    ADMM_TRY(element_update(ax, &nblk, &done));
    if (done) return ADMM_OK;
    // A = D: only the next x-update's right-hand side D'*(c + z - u) is left to do (its partial sums carry the finalize)
    if (fuse_tail) return transposed_products(1, defer_fin_ad ? &dff : nullptr);
    fa.nblk = nblk;
    const bool shard_rows = sharded && !e->a_identity;  // z, u and the residual sums are row-local
    if (alg == 2) ADMM_TRY(weak_fast_step(nblk, shard_rows));
    if (!e->a_identity) ADMM_TRY(dual_products(nblk, shard_rows));
    ADMM_TRY(objective_terms(nblk));
    TimerScope ts(e, ADMM_K_FINALIZE);
    launch_finalize(fa, e->stream);
    return ADMM_OK;
  }

  int x_update_and_ax(AxSource* ax) {
    ADMM_TRY(x_update(e, ax, fuse_tail));
    if (!e->a_identity && !e->D) {  // Ax = A(x) with options.A a function handle (admm.m:117-120, 535)
      TimerScope ts(e, ADMM_K_GEMV_N);
      if (e->acb(e->auser, e->x, nA, e->axbuf, len, static_cast<void*>(e->stream)) != 0)
        return fail(ADMM_E_INVALID, "the A operator callback reported a failure");
      ax->src = e->axbuf;
      ax->npart = 1;
      ax->ld = 0;
    } else if (!e->a_identity) {  // Ax = D*x (admm.m:535), summed inside the prox kernel
      TimerScope ts(e, ADMM_K_GEMV_N);
      launch_gemv_n(e->planDN, e->D, e->x, e->partDN, e->ctrl, e->stream);
      ax->src = e->partDN;
      ax->npart = e->planDN.nchunk;
      ax->ld = e->planDN.ldy;
    }
    return ADMM_OK;
  }

  // xh = Ax (or the relaxed Axhat) as a vector, and optionally the right-hand side of zminModel
  void launch_prez_for(const AxSource& ax, const double* uo, const double* add, double* rz) {
    PreZArgs za{};
    za.len = len;
    za.axsrc = ax.src;
    za.naxpart = ax.npart;
    za.axld = ax.ld;
    za.c = e->c;
    za.z = e->z;
    za.uo = uo;
    za.add = add;
    za.xh = e->xh;
    za.rz = rz;
    za.rho = o.rho;
    za.relax = o.relax;
    launch_prez(za, e->ctrl, e->stream);
  }

  // z = zming(x or Axhat, z, u or uhat, rho) between the two halves of the fused kernel
  int split_z_update(const AxSource& ax) {
    TimerScope ts(e, ADMM_K_PROX);
    const double* uo = (alg == 0) ? e->u : e->uhat;
    launch_prez_for(ax, uo, e->qz, e->zcb ? nullptr : e->rz);
    if (!e->zcb) {  // zminModel: (QtQ + rho I) \ (Qts + rho*(x + u))   getProxOps.m:1012
      apply_slice_factor(e, e->zfac, e->rz, e->zext);
      return ADMM_OK;
    }
    // admm.m:521-530: zming is called with x itself, or with the relaxed Axhat when relax != 1; with A = 1
    // the two have the same length (xh), with A = D the un-relaxed call passes the n-vector x
    const double* zarg = (e->a_identity || o.relax != 1.0) ? e->xh : e->x;
    if (e->bgen) {  // z = zming(., z, u, rho) in the caller's own space, then w = -B*z for the fused kernel
      if (e->zcb(e->zuser, zarg, e->zt, uo, o.rho, e->ztnew, e->nBz, static_cast<void*>(e->stream)) != 0)
        return fail(ADMM_E_INVALID, "the zming callback reported a failure");
      ADMM_TRY(apply_b(e, e->ztnew, e->zext));
      ZStateArgs zs{e->nBz, e->zt, e->ztprev, e->vt, e->ztnew, e->zthist, e->vthist, alg, 0};
      launch_zstate(zs, e->ctrl, e->stream);
    } else if (e->zcb(e->zuser, zarg, e->z, uo, o.rho, e->zext, len, static_cast<void*>(e->stream)) != 0) {
      return fail(ADMM_E_INVALID, "the zming callback reported a failure");
    }
    return ADMM_OK;
  }

  // the element update (z, u, the next right-hand side, the block partials of the residual sums) in one of its four
  // tails.  *done: the iteration ends with this launch
  int element_update(const AxSource& ax, int* nblk, bool* done) {
    fa.slots_reduced = nullptr;
    fa.objp_reduced = nullptr;
    fa.objpart = obj.obj_covsel ? e->objpart : nullptr;  // (written by this iteration's x-update)
    fa.nobjpart = obj.obj_covsel ? 1 : 0;
    TimerScope ts(e, ADMM_K_PROX);
    pa.axsrc = ax.src;
    pa.ax_t = ax.t;
    pa.ax_tri = ax.tri;
    pa.naxpart = ax.npart;
    pa.axld = ax.ld;
    pa.x_out = e->a_identity ? e->x : nullptr;
    if (defer_fin) {  // the element update alone; the finalize rides along with the next x-solve
      launch_tail(nblk, true);
      dff = tail_fin_args(*nblk);
      e->dfin = &dff;
      e->dfin_pending = true;
      *done = true;
    } else if (fuse_tail && defer_fin_ad) {  // A = D without a dual residual: the finalize rides along with the partial
      launch_tail(nblk, true);  // sums of the next right-hand side (iterate_general)
      dff = tail_fin_args(*nblk);
    } else if (fuse_tail) {  // z/u update + finalize in one launch
      launch_tail(nblk, false);
      *done = e->a_identity;  // the iteration ends here
    } else {
      ADMM_TRY(element_update_plain(ax, nblk));
    }
    return ADMM_OK;
  }

  // the one-launch tail with the run's family: the lasso's, or the grouped one of group lasso (its block partials: one per
  // workgroup of the plan)
  void launch_tail(int* nblk, bool defer) {
    if (grouped) launch_group_prox_fin(pa, fa, e->grp, e->ctrl, nblk, e->stream, defer, &fam);
    else launch_prox_fin(pa, fa, e->ctrl, nblk, e->stream, defer, &fam);
  }
  FinArgs tail_fin_args(int nblk) {
    FinArgs d = prox_fin_args(pa, fa);
    if (grouped) d.nblk = nblk;
    return d;
  }

  // the element update on its own, with the caller's options.altu / options.specialnorms around it
  int element_update_plain(const AxSource& ax, int* nblk) {
    if (e->altucb) {  // options.altu needs the old u and Ax (or the relaxed Axhat) as vectors: admm.m:553-559
      ADMM_HIP_TRY(hipMemcpyAsync(e->hk_uold, e->u, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));
      if (!split_z) launch_prez_for(ax, e->u, nullptr, nullptr);
    }
    // A grouped or penalised run keeps the tail kernel here, deferred (the block partials stored plainly: launch_finalize
    // follows): a prox_kernel form of them would sum the block partials over other blocks, in another order, and change
    // the bits.
    if (grouped || fam.kind == FAM_PENALTY) launch_tail(nblk, true);
    else launch_prox(pa, e->ctrl, nblk, e->stream, &fam);
    if (e->altucb) {
      launch_negate(e->z, e->hk_bz, len, e->ctrl, e->stream);
      if (e->altucb(e->altuuser, e->hk_uold, e->xh, e->hk_bz, e->c ? e->c : e->hk_zero, len, e->hk_unew,
                    static_cast<void*>(e->stream)) != 0)
        return fail(ADMM_E_INVALID, "the altu callback reported a failure");
      UFixArgs ux{};
      ux.len = len;
      ux.unew = e->hk_unew;
      ux.uold = e->hk_uold;
      ux.z = e->z;
      ux.c = e->c;
      ux.rhs_add = e->rhs_add;
      ux.u = e->u;
      ux.uhist = e->uhist;
      ux.rhs = pa.rhs;
      ux.part = e->part;
      ux.nblk = *nblk;
      ux.rhs_kind = pa.rhs_kind;
      ux.rho = o.rho;
      launch_ufix(ux, e->ctrl, e->stream);
    }
    if (e->normscb) {  // v = options.specialnorms(x, z, u, rho)   admm.m:612-616
      if (e->normscb(e->normsuser, e->x, nA, e->bgen ? e->zt : e->z, e->bgen ? e->nBz : len, e->u, len, o.rho,
                     e->hk_norms, static_cast<void*>(e->stream)) != 0)
        return fail(ADMM_E_INVALID, "the specialnorms callback reported a failure");
    }
    return ADMM_OK;
  }

  // weak fast ADMM: the restart decision and the extrapolation (admm.m:572-600)
  int weak_fast_step(int nblk, bool shard_rows) {
    if (shard_rows) {  // the restart decision needs the global ||u-uhat||^2, ||z-v||^2 (admm.m:572-573)
      launch_pack_slots(e->part, nblk, e->red, e->ctrl, e->stream);
      ADMM_TRY(comm_allreduce_device(e->comm, e->red, 16, e->stream));
      fa.slots_reduced = e->red;
    }
    launch_fast_decide(fa, e->stream);
    launch_extrapolate(xa, e->ctrl, e->stream);
    if (e->bgen) {
      ZStateArgs zs{e->nBz, e->zt, e->ztprev, e->vt, nullptr, nullptr, e->vthist, alg, 1};
      launch_zstate(zs, e->ctrl, e->stream);
    }
    return ADMM_OK;
  }

  // D'*[c+zx-ux, z-zprev, u]  (getProxOps.m:1514; admm.m:624, 654) in ONE pass
  int dual_products(int nblk, bool shard_rows) {
    ADMM_TRY(transposed_products(nrhs_dual, nullptr));
    if (!shard_rows) return ADMM_OK;
    // ONE all-reduce per iteration: d = sum_g D_g'(...) (unwrappedadmm.m:135-137) for up to
    // three right-hand sides plus the 16 residual/objective partial sums (X3 + X6)
    double* slots = e->g + 3 * e->ldg;
    if (alg == 2) ADMM_HIP_TRY(hipMemcpyAsync(slots, e->red, 16 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    else launch_pack_slots(e->part, nblk, slots, e->ctrl, e->stream);
    if (alg == 2) {  // slots were already reduced: only the vectors travel
      ADMM_TRY(comm_allreduce_device(e->comm, e->g, static_cast<size_t>(3 * e->ldg), e->stream));
    } else {
      ADMM_TRY(comm_allreduce_device(e->comm, e->g, static_cast<size_t>(3 * e->ldg + 16), e->stream));
    }
    fa.slots_reduced = slots;
    return ADMM_OK;
  }

  // the objective's data term for the finalize: already in the element update's slots, or by its own kernels
  int objective_terms(int nblk) {
    fa.objpart = nullptr;
    fa.nobjpart = 0;
    if ((obj.obj_lasso_gemv || obj.obj_qp_gemv) && gram_now) {  // the element update's S_OBJX slot holds the data term already
      fa.obj_scale_part = 0.0;
      fa.obj_scale_x = 1.0;
      fa.obj_const = alt_const;
    } else if (obj.obj_lasso_gemv) {  // 0.5*||D*x - s||^2  (lasso.m:227)
      TimerScope ts(e, ADMM_K_GEMV_N);
      int nob = 0;
      if (e->sparse) {  // D*x by the sparse product into the length-m scratch of the CG operator: one finished chunk
        launch_spmv(e->sp.n, e->x, e->tmpA, e->ctrl, e->stream);
        launch_residual_sq(e->tmpA, 1, 0, e->s, e->m, e->objpart, &nob, e->ctrl, e->stream);
      } else {
        launch_gemv_n(e->planDN, e->D, e->x, e->partDN, e->ctrl, e->stream);
        launch_residual_sq(e->partDN, e->planDN.nchunk, e->planDN.ldy, e->s, e->m, e->objpart, &nob, e->ctrl, e->stream);
      }
      fa.obj_scale_part = 0.5;
      fa.obj_const = 0.0;
      fa.objpart = e->objpart;
      fa.nobjpart = nob;
      if (gram_calibrating)  // the solve-identity form beside it (slot partials of the element update): how far apart?
        launch_obj_compare(e->objpart, nob, 0.5, 0.0, e->part + static_cast<size_t>(S_OBJX) * kMaxPartBlocks, nblk, 1.0,
                           e->half_ssq, e->gobjpart + kMaxPartBlocks, e->ctrl, e->stream);
      if (sharded) {  // sum over the row shards of ||D_g*x - s_g||^2
        launch_pack_sum(e->objpart, nob, e->red + 16, e->ctrl, e->stream);
        ADMM_TRY(comm_allreduce_device(e->comm, e->red + 16, 1, e->stream));
        fa.objp_reduced = e->red + 16;
      }
    } else if (o.objevals && e->ocb) {  // objevals(i) = obj(x, z) with the caller's handle (admm.m:604)
      if (e->ocb(e->ouser, e->x, nA, e->bgen ? e->zt : e->z, e->bgen ? e->nBz : len, e->objpart,
                 static_cast<void*>(e->stream)) != 0)
        return fail(ADMM_E_INVALID, "the objective callback reported a failure");
      fa.objpart = e->objpart;
      fa.nobjpart = 1;
    } else if (obj.obj_covsel) {
      fa.objpart = e->objpart;
      fa.nobjpart = 1;
    } else if (obj.obj_model_gemv) {
      TimerScope ts(e, ADMM_K_GEMV_N);
      int nob1 = 0, nob2 = 0;
      launch_gemv_n(e->planDN, e->D, e->x, e->partDN, e->ctrl, e->stream);
      launch_residual_sq(e->partDN, e->planDN.nchunk, e->planDN.ldy, e->ell, e->m, e->objpart, &nob1, e->ctrl,
                         e->stream);
      launch_gemv_n(e->planD2N, e->D2, e->z, e->partD2N, e->ctrl, e->stream);
      launch_residual_sq(e->partD2N, e->planD2N.nchunk, e->planD2N.ldy, e->s2, e->m2, e->objpart + nob1, &nob2, e->ctrl,
                         e->stream);
      fa.objpart = e->objpart;
      fa.nobjpart = nob1 + nob2;
    } else if (obj.obj_qp_gemv) {  // 1/2 x'Px + q'x + r  (quadraticprogram.m:242)
      int nob = 0;
      const GemvTPlan& p = e->planSq;  // P is symmetric
      launch_gemv_t(p, e->Pmat, e->x, nullptr, nullptr, 1, e->partSq, e->ctrl, e->stream);
      launch_qp_objective(e->partSq, p.nchunk, p.ldg, e->x, e->q, e->n, e->objpart, &nob, e->ctrl, e->stream);
      fa.objpart = e->objpart;
      fa.nobjpart = nob;
      if (gram_calibrating)  // the right-hand-side form beside it
        launch_obj_compare(e->objpart, nob, 1.0, e->rconst, e->part + static_cast<size_t>(S_OBJX) * kMaxPartBlocks, nblk,
                           1.0, e->rconst, e->gobjpart + kMaxPartBlocks, e->ctrl, e->stream);
    }
    return ADMM_OK;
  }

  int capture_graph() {
    gbatch = (N < check_every) ? N : check_every;
    hipError_t ge = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    int rc_cap = ADMM_OK;
    if (ge == hipSuccess) {
      for (int32_t b = 0; b < gbatch && rc_cap == ADMM_OK; ++b) rc_cap = iterate();
      ge = hipStreamEndCapture(e->stream, &graph);
    }
    if (ge == hipSuccess && rc_cap == ADMM_OK) ge = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
    if (ge != hipSuccess || rc_cap != ADMM_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      graph = nullptr;
      return fail(ADMM_E_DEVICE, std::string("hipGraph capture of the iteration failed: ") + hipGetErrorString(ge));
    }
    return ADMM_OK;
  }

  int run_batches() {
    int32_t enq = 0;
    bool stopped = false;
    while (enq < N && !stopped) {
      polled = false;
      int32_t batch = (N - enq < check_every) ? N - enq : check_every;
      if (gexec) {
        batch = gbatch;  // a full batch; iterations beyond maxiters are device-side no-ops
        if (hipGraphLaunch(gexec, e->stream) != hipSuccess) return fail(ADMM_E_DEVICE, "hipGraphLaunch failed");
      } else {
        for (int32_t b = 0; b < batch; ++b) ADMM_TRY(iterate());
      }
      enq += batch;
      if (defer_fin && e->dfin_pending) {  // the batch's last iteration
        launch_finalize(dff, e->stream);
        e->dfin_pending = false;
      }
      if (uw_fused && ua.fin_pending) {  // the last enqueued iteration's finalize, on its own
        FinArgs flast = uw_fin_args(ua, fa);
        flast.x = e->uwX + ((ua.iter + 1) & 1) * e->uwldg;
        launch_finalize(flast, e->stream);
        ua.fin_pending = 0;
      }
      // the host polls after EVERY batch, domaxiters runs included: an unbounded run of launches without a host
      // sync (6000 for a 1000-iteration SVM run) overruns a buffer inside rocprofv3's counter-collection mode
      // (SIGSEGV in the launch path of the profiler, r2 record in DESIGN section 6); one 64-byte read-back per 64
      // iterations costs < 1 %
      if (poll_ctrl(e) != ADMM_OK) return fail(ADMM_E_DEVICE, "polling the device control block failed");
      polled = true;
      if (e->ctrl_host->stop) stopped = true;
      ADMM_TRY(after_batch());
    }
    return ADMM_OK;
  }

  // ctrl_host holds the batch's last control block: the two decisions about the objective's form
  int after_batch() {
    // The right-hand-side form of the objective cancels terms of the size of 1/2*s's down to the data misfit: once
    // eps * |terms| / |objective| (the device keeps the run's maximum in ctrl) leaves 1e-10 -- a near-interpolating fit,
    // small lambda, little noise -- the engine goes back to the literal D*x pass (lasso.m:227), for the rest of this
    // run and for every later one.  Nothing is pending at a batch boundary, so the launch sequence may change here.
    if (gram_guard && gram_now && e->ctrl_host->obj_bound > 1e-10) {
      e->obj_gram_ok = false;
      e->obj_gram_bad = true;
      gram_now = false;
      obj_kernels = true;
      fuse_tail = false;
      defer_fin = false;
      defer_fin_ad = false;
      fa.obj_track_bound = 0;
      pa.objx = OBJX_NONE;
      fa.obj_scale_x = 0.0;
      fa.obj_const = 0.0;
      fa.obj_scale_part = alt_qp ? 1.0 : 0.5;
      if (alt_qp) fa.obj_const = e->rconst;
    }
    if (e->ctrl_host->obj_bound > e->obj_bound_seen) e->obj_bound_seen = e->ctrl_host->obj_bound;
    int rc = ADMM_OK;
    if (gram_calibrating) {  // the batch evaluated both forms of the lasso objective
      double disc = 1.0;
      if (hipMemcpy(&disc, e->gobjpart + kMaxPartBlocks, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(ADMM_E_DEVICE, "reading the objective calibration failed");
      gram_calibrating = false;
      if (disc <= 1e-11 && !(e->ctrl_host->obj_bound > 1e-10)) {
        e->obj_gram_ok = true;
        gram_now = true;
      } else {
        e->obj_gram_bad = true;
      }
    }
    return rc;
  }

  int finish(admm_run_summary* summary) {
    if (!polled) ADMM_TRY(poll_ctrl(e));
    if (uw_fused && e->ctrl_host->steps > 0) {  // the x of the last completed iteration (double-buffered on its parity)
      ADMM_HIP_TRY(hipMemcpyAsync(e->x, e->uwX + ((e->ctrl_host->steps - 1) & 1) * e->uwldg, sizeof(double) * e->n,
                                  hipMemcpyDeviceToDevice, e->stream));
      ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    }
    const double runtime = std::chrono::duration<double>(std::chrono::steady_clock::now() - tstart).count();
    if (e->problem == ADMM_PROB_COVSEL) {
      int32_t sw = 0;
      ADMM_HIP_TRY(hipMemcpy(&sw, e->cov_cnt, sizeof(int32_t), hipMemcpyDeviceToHost));
      e->cov_sweeps = sw + e->cov_sweeps_host;
    }
    if (e->cg_st) {
      ADMM_HIP_TRY(hipMemcpy(e->cg_st_host, e->cg_st, sizeof(CgState), hipMemcpyDeviceToHost));
      e->cg_total_last = e->cg_st_host->total;
      e->cg_capped_last = e->cg_st_host->capped;
    }
    ADMM_TRY(finish_run(e, o, N, runtime, nullptr));
    // (the TV and consensus runs leave a failed profiled run's unread timer events in place: only this loop drops them)
    for (auto& t : e->timers) t.used = 0;
    e->last.obj_gram_used = (o.objevals && gram_now) ? 1 : 0;
    if (summary) *summary = e->last;
    return comm_check_error(e->comm, e->stream);
  }
};

}  // namespace

int run_general(admm_engine* e, RunState& rs, admm_run_summary* summary) {
  GeneralLoop loop(e, rs);
  const int rc = loop.run(summary);
  // the one place, on every way out: the deferred finalize pointed into the loop object
  e->dfin = nullptr;
  e->dfin_pending = false;
  return rc;
}

}  // namespace admm
