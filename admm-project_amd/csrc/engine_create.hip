// engine_create.hip -- C ABI (include/admm_engine.h): admm_engine_create = the reference solvers' one-time setup +
// getproxops (lasso.m:160-192, lad.m:129-137, huberfit.m:161-169, linearsvm.m:183-217 + unwrappedadmm.m:76-92,
// quadraticprogram.m:210-232, basispursuit.m:116-127), one setup_<problem> function per problem.  The factor machinery
// they call is engine.hip.  Within a problem the order of device allocations, uploads, launches and collectives is
// fixed: the ranks of a sharded engine must issue the same collectives in the same order.
#include "engine_internal.h"

namespace {

struct CreateCtx {  // what create's option checks compute and the setup functions read
  int xs;             // the x-solve asked for, after the per-problem defaults (2-D TV: always CG)
  int mk;             // desc->mem: where the caller's arrays live
  bool sharded;       // a communicator with more than one rank
  int64_t m_global;   // rows of D over all ranks (the local m when not sharded)
  bool tv2_want_dct;  // 2-D TV: build the tables of the spectral x-update
  const admm_sparse_desc* sparse;  // admm_engine_create_sparse: the checked matrix in HOST arrays, else null
};

struct SideStream {  // a second stream and the event that orders it behind the engine's, released on every path
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;
  ~SideStream() {
    if (ev) (void)hipEventDestroy(ev);
    if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace

static int64_t src_ld(const admm_problem_desc* desc) { return desc->ldD ? desc->ldD : desc->m; }

// A big host matrix whose Gram matrix is needed anyway: upload it in row chunks and accumulate D_c'*D_c of the chunk
// that has arrived on a second stream while the next chunk crosses PCIe (the copy from pageable memory keeps the host
// busy, the GEMM does not): create() drops from upload + Gram to about the longer of the two.
// *W (ldW x n) = D'*D, lower triangle (lasso.m:168 before the rho shift).
static int upload_with_gram(admm_engine* e, const admm_problem_desc* desc, double** W, int64_t ldW) {
  const int64_t m = desc->m, n = desc->n;
  e->ldD = round_up(m, 512);
  ADMM_TRY(e->mem.alloc(&e->D, static_cast<size_t>(e->ldD) * n));
  if (e->ldD != m) ADMM_HIP_TRY(hipMemsetAsync(e->D, 0, sizeof(double) * e->ldD * n, e->stream));
  ADMM_TRY(e->mem.alloc(W, static_cast<size_t>(ldW) * n));
  ADMM_HIP_TRY(hipMemsetAsync(*W, 0, sizeof(double) * ldW * n, e->stream));
  SideStream side;
  ADMM_HIP_TRY(hipStreamCreateWithFlags(&side.s, hipStreamNonBlocking));
  ADMM_HIP_TRY(hipEventCreateWithFlags(&side.ev, hipEventDisableTiming));
  const int64_t chunk = round_up(ceil_div(m, int64_t{8}), 512);
  for (int64_t r0 = 0; r0 < m; r0 += chunk) {
    const int64_t rows = (m - r0 < chunk) ? m - r0 : chunk;
    ADMM_HIP_TRY(hipMemcpy2DAsync(e->D + r0, e->ldD * sizeof(double), desc->D + r0, src_ld(desc) * sizeof(double),
                                  rows * sizeof(double), n, hipMemcpyHostToDevice, e->stream));
    ADMM_HIP_TRY(hipEventRecord(side.ev, e->stream));
    ADMM_HIP_TRY(hipStreamWaitEvent(side.s, side.ev, 0));
    launch_gemm(1, 0, n, n, rows, 1.0, e->D + r0, e->ldD, e->D + r0, e->ldD, 1.0, *W, ldW, true, side.s);
  }
  ADMM_HIP_TRY(hipStreamSynchronize(side.s));
  return ADMM_OK;
}

// A device copy of desc->D (and of desc->s when with_s) that lives only while build(D, ld, s) makes something of it
template <class Build>
static int with_data_copy(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx, bool with_s,
                          Build&& build) {
  double *Dd = nullptr, *sd = nullptr;
  int64_t ldd = 0;
  ADMM_TRY(upload_matrix(e->mem, &Dd, &ldd, desc->D, desc->m, desc->n, src_ld(desc), cx.mk, e->stream));
  if (with_s) ADMM_TRY(upload(e->mem, &sd, desc->s, desc->m, cx.mk, e->stream));
  ADMM_TRY(build(Dd, ldd, sd));
  e->mem.free_one(Dd);
  e->mem.free_one(sd);
  return ADMM_OK;
}

// the pivot ratio of the factor just built says D'D is singular to rounding (n * eps)
static bool gram_singular(const admm_engine* e, int64_t n) {
  return !(e->xfac.cond_diag < 1.0 / (static_cast<double>(n) * 2.220446049250313e-16));
}

static int setup_lasso(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const int mk = cx.mk;
  if (!desc->D || (!desc->s && !desc->Dts) || m <= 0 || n <= 0)
    return fail(ADMM_E_INVALID, "lasso needs D (m x n) and s (or D'*s)");
  if (desc->lambda < 0) return fail(ADMM_E_INVALID, "lambda must be a nonnegative real (lasso.m:132)");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_RHO_DTS;
  e->fat = cx.m_global < n;
  if (cx.sharded && e->fat) return fail(ADMM_E_UNSUPPORTED, "row-sharded lasso needs a tall matrix (global m >= n)");
  double* Wpre = nullptr;  // D'*D when the upload has already accumulated it
  const int64_t ldW = round_up(e->fat ? m : n, 16);
  if (mk == ADMM_MEM_HOST && !e->fat && !desc->L && e->xsolve != ADMM_XSOLVE_CG && m >= 32768 &&
      static_cast<double>(m) * n >= 1e8)
    ADMM_TRY(upload_with_gram(e, desc, &Wpre, ldW));
  else
    ADMM_TRY(upload_matrix(e->mem, &e->D, &e->ldD, desc->D, m, n, src_ld(desc), mk, e->stream));
  if (desc->s) ADMM_TRY(upload(e->mem, &e->s, desc->s, m, mk, e->stream));
  e->planDN = gemv_n_plan(m, n, e->ldD);
  e->planDT = gemv_t_plan(m, n, e->ldD);
  ADMM_TRY(e->mem.alloc(&e->partDN, e->planDN.part_elems()));
  ADMM_TRY(e->mem.alloc(&e->partDT, e->planDT.part_elems(3)));
  // Dts = D'*s   lasso.m:160 (or handed in: args.Dts, getProxOps.m:446)
  ADMM_TRY(e->mem.alloc(&e->rhs_add, round_up(n, 2)));
  if (desc->Dts) {
    if (cx.sharded) return fail(ADMM_E_UNSUPPORTED, "args.Dts on a row-sharded engine: pass the local rows of s");
    ADMM_HIP_TRY(hipMemcpyAsync(e->rhs_add, desc->Dts, sizeof(double) * n,
                                mk == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
  } else {
    launch_gemv_t(e->planDT, e->D, e->s, nullptr, nullptr, 1, e->partDT, nullptr, e->stream);
    launch_sum_partials_t(e->planDT, e->partDT, 1, e->rhs_add, round_up(n, 2), nullptr, e->stream);
  }
  if (cx.sharded) ADMM_TRY(comm_allreduce_device(e->comm, e->rhs_add, n, e->stream));  // sum_g D_g'*s_g
  if (e->xsolve == ADMM_XSOLVE_CG) {  // matrix-free: nothing n x n is ever formed
    if (e->fat) return fail(ADMM_E_UNSUPPORTED, "xsolve=cg needs a tall matrix (m >= n)");
    e->cg_shift_is_rho = true;
    return e->mem.alloc(&e->tmpA, round_up(m, 2));
  }
  const int64_t nF = e->fat ? m : n;
  double* W = Wpre;
  if (!W) ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ldW) * nF));
  if (!desc->L) {
    if (!e->fat) {  // lasso.m:168  chol(D'*D + rho*I)
      if (!Wpre) ADMM_TRY(gram_lower(e, e->D, e->ldD, m, n, false, 1.0, W, ldW));
      // W = sum_g D_g'*D_g  (unwrappedadmm.m:118-122); one-time, bandwidth-bound all-reduce
      if (cx.sharded) ADMM_TRY(comm_allreduce_device(e->comm, W, static_cast<size_t>(ldW) * n, e->stream));
      launch_add_diag(W, n, ldW, desc->rho, e->stream);
    } else {  // lasso.m:172  chol(1/rho*(D*D') + I)
      ADMM_TRY(gram_lower(e, e->D, e->ldD, m, n, true, 1.0 / desc->rho, W, ldW));
      launch_add_diag(W, m, ldW, 1.0, e->stream);
    }
    if (desc->obj_gram >= 0 && e->s) {  // (0 = automatic: the form costs nothing, and is calibrated first)
      // The objective's data term without a pass over D: x solves (G + rho*I) x = y (directly, or through the
      // matrix-inversion lemma of the fat case, lasso.m:172), so G x = y - rho*x and
      // 1/2*||D x - s||^2 = 1/2*x'(y - rho*x) - x'D's + 1/2*s's comes out of the element update's own operands
      // (OBJX_SOLVE, prox_device.h).  Needs 1/2*s's, over all shards, once.
      e->obj_alt = true;
      e->obj_auto = desc->obj_gram == 0;
      ADMM_TRY(e->mem.alloc(&e->gobjpart, kMaxPartBlocks + 2));
      double ssq = 0.0;
      ADMM_TRY(device_sumsq_host(e, e->s, m, &ssq));
      ADMM_TRY(allreduce_scalar(e, &ssq, e->gobjpart));
      e->half_ssq = 0.5 * ssq;
    }
  }
  ADMM_TRY(factorize(e, W, nF, ldW, desc->L, mk));
  if (e->fat) {
    ADMM_TRY(e->mem.alloc(&e->tmpA, round_up(m, 2)));
    ADMM_TRY(e->mem.alloc(&e->tmpB, round_up(m, 2)));
  }
  return ADMM_OK;
}

// The lasso on a sparse design matrix: both orientations of D on the device, D'*s by the sparse
// product, the matrix-free x-update.  e->D stays null: cg_apply and the literal objective run launch_spmv, and every
// other reader of D belongs to a factor path or to an A = D problem.
static int setup_lasso_sparse(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  if (!desc->s && !desc->Dts) return fail(ADMM_E_INVALID, "lasso needs s (or D'*s)");
  if (desc->lambda < 0) return fail(ADMM_E_INVALID, "lambda must be a nonnegative real (lasso.m:132)");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_RHO_DTS;
  e->fat = false;  // (D'D + rho I) is positive definite for every shape: one x-update form
  e->sparse = true;
  ADMM_TRY(sparse_device_build(cx.sparse, &e->sp, e->stream));
  if (desc->s) ADMM_TRY(upload(e->mem, &e->s, desc->s, m, cx.mk, e->stream));
  ADMM_TRY(e->mem.alloc(&e->rhs_add, round_up(n, 2)));
  ADMM_HIP_TRY(hipMemsetAsync(e->rhs_add, 0, sizeof(double) * round_up(n, 2), e->stream));
  if (desc->Dts)
    ADMM_HIP_TRY(hipMemcpyAsync(e->rhs_add, desc->Dts, sizeof(double) * n,
                                cx.mk == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
  else
    launch_spmv(e->sp.t, e->s, e->rhs_add, nullptr, e->stream);  // Dts = D'*s   lasso.m:160
  e->cg_shift_is_rho = true;
  ADMM_TRY(e->mem.alloc(&e->tmpA, round_up(m, 2)));
  ADMM_HIP_TRY(hipMemsetAsync(e->tmpA, 0, sizeof(double) * round_up(m, 2), e->stream));
  return ADMM_OK;
}

// options.A / options.At are function handles (admm.m:117-158): no matrix, both operators are callbacks
static int setup_operator_form(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m;
  if (!desc->s) return fail(ADMM_E_INVALID, "the operator form needs the constraint vector c (as s)");
  if (cx.sharded) return fail(ADMM_E_UNSUPPORTED, "operator callbacks are not supported on row-sharded engines");
  e->a_identity = false;
  e->nA = desc->n;
  e->len = m;
  e->len_global = m;
  e->rhs_kind = RHS_T1;
  e->prox = PROX_SOFT;
  ADMM_TRY(upload(e->mem, &e->s, desc->s, m, cx.mk, e->stream));
  e->c = e->s;
  return e->mem.alloc(&e->axbuf, round_up(m, 2));
}

// args.Dplus = pinv(D) from the caller (linearsvm.m:185-186): x = Dplus*(z-u) is one pass over its transpose with the
// column-dot kernel (the same bytes as D'*v); nothing is factored
static int setup_svm_given_pinv(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  double *Dp = nullptr, *Dpt = nullptr;
  ADMM_TRY(upload(e->mem, &Dp, desc->Dplus, static_cast<size_t>(n) * m, cx.mk, e->stream));
  ADMM_TRY(e->mem.alloc(&Dpt, static_cast<size_t>(m) * n));
  launch_transpose(Dp, Dpt, n, m, nullptr, e->stream);  // (n x m) -> (m x n)
  ADMM_TRY(e->mem.alloc(&e->DplusT, static_cast<size_t>(e->ldD) * n));
  ADMM_HIP_TRY(hipMemsetAsync(e->DplusT, 0, sizeof(double) * e->ldD * n, e->stream));
  ADMM_HIP_TRY(hipMemcpy2DAsync(e->DplusT, e->ldD * sizeof(double), Dpt, m * sizeof(double), m * sizeof(double), n,
                                hipMemcpyDeviceToDevice, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  ADMM_TRY(build_unwrapped_pinv(e, Dp));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->mem.free_one(Dp);
  e->mem.free_one(Dpt);
  e->xsolve = ADMM_XSOLVE_PINV;
  return ADMM_OK;
}

// LAD, Huber fit and the linear SVM: the generic A = D iteration
static int setup_lad_huber_svm(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const int mk = cx.mk;
  const bool svm = desc->problem == ADMM_PROB_LINEARSVM;
  if (!desc->D && cx.xs == ADMM_XSOLVE_CALLBACK && desc->problem == ADMM_PROB_LAD && m > 0 && n > 0)
    return setup_operator_form(e, desc, cx);
  if (!desc->D || m <= 0 || n <= 0) return fail(ADMM_E_INVALID, "problem needs D (m x n)");
  if (!svm && !desc->s) return fail(ADMM_E_INVALID, "LAD/Huber need the signal vector s");
  if (svm && !desc->ell) return fail(ADMM_E_INVALID, "linear SVM needs the label vector ell");
  // (the linear SVM's x-update is pinv(D)*(z-u), linearsvm.m:185: it exists for a wide D too -- the rank-deficient
  // D'D falls through to the pseudo-inverse below; lad.m:134 / huberfit.m:166 call chol, which errors)
  if (cx.m_global < n && cx.xs != ADMM_XSOLVE_CALLBACK && !(svm && !cx.sharded))
    return fail(ADMM_E_INVALID, "D must have full column rank (m >= n) for chol(D'*D) (lad.m:134)");
  e->a_identity = false;
  e->nA = n;
  e->len = m;
  e->len_global = cx.m_global;
  e->rhs_kind = RHS_T1;
  if (desc->problem == ADMM_PROB_LAD) e->prox = PROX_SOFT;
  else if (desc->problem == ADMM_PROB_HUBERFIT) e->prox = PROX_HUBER;
  else e->prox = (desc->loss == ADMM_LOSS_01) ? PROX_01 : (desc->loss == ADMM_LOSS_LOGISTIC) ? PROX_LOGISTIC : PROX_HINGE;
  ADMM_TRY(upload_matrix(e->mem, &e->D, &e->ldD, desc->D, m, n, src_ld(desc), mk, e->stream));
  if (!svm) {
    ADMM_TRY(upload(e->mem, &e->s, desc->s, m, mk, e->stream));
    e->c = e->s;  // lad.m:142  options.c = s
  } else {
    ADMM_TRY(upload(e->mem, &e->ell, desc->ell, m, mk, e->stream));
  }
  e->planDN = gemv_n_plan(m, n, e->ldD);
  e->planDT = gemv_t_plan(m, n, e->ldD);
  ADMM_TRY(e->mem.alloc(&e->partDN, e->planDN.part_elems()));
  ADMM_TRY(e->mem.alloc(&e->partDT, e->planDT.part_elems(3)));
  if (e->xsolve == ADMM_XSOLVE_CG) {  // matrix-free normal equations D'D x = D'(c + z - u)
    e->cg_shift_is_rho = false;
    return e->mem.alloc(&e->tmpA, round_up(m, 2));
  }
  if (e->xsolve == ADMM_XSOLVE_CALLBACK) return ADMM_OK;  // the caller's xminf is the x-update: nothing to factor
  if (svm && desc->Dplus) return setup_svm_given_pinv(e, desc, cx);
  const int64_t ld = round_up(n, 16);
  double* W = nullptr;
  ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ld) * n));
  if (!desc->L) {  // lad.m:134  chol(D'*D,'lower') (un-shifted; also D^+ = (D'D)^-1 D' for the SVM)
    ADMM_TRY(gram_lower(e, e->D, e->ldD, m, n, false, 1.0, W, ld));
    // W = sum_g D_g'*D_g  (unwrappedadmm.m:96-123)
    if (cx.sharded) ADMM_TRY(comm_allreduce_device(e->comm, W, static_cast<size_t>(ld) * n, e->stream));
  }
  if (!svm || desc->L) {  // lad.m:134 / huberfit.m:166: chol errors on a rank-deficient D, and so does the engine
    ADMM_TRY(factorize(e, W, n, ld, desc->L, mk));
    // exactly dependent columns leave a pivot at the rounding level of D'D, of either sign: where MATLAB's chol
    // may or may not error, the engine always refuses (the iterates would be noise amplified by 1/pivot)
    if (!desc->L && gram_singular(e, n))
      return fail(ADMM_E_NUMERIC, "Cholesky failed: D'*D is numerically singular (pivot ratio " +
                                      std::to_string(e->xfac.cond_diag) + "): D must have full column rank (lad.m:134)");
    return ADMM_OK;
  }
  // linear SVM: the reference's x-update is pinv(D)*(z-u) (linearsvm.m:185, unwrappedadmm.m:76-78), which exists
  // for every D.  Full column rank: (D'D)^-1 D' through the Cholesky factor (same map, to rounding).  Rank
  // deficient -- Cholesky breaks down, or its pivots fall to the rounding level of D'D -- or on request
  // (xsolve = pinv): the pseudo-inverse of D'D from its eigen-decomposition.
  double* Wkeep = nullptr;  // the Gram matrix survives the in-place factorisation attempt
  ADMM_TRY(e->mem.alloc(&Wkeep, static_cast<size_t>(ld) * n));
  ADMM_HIP_TRY(hipMemcpyAsync(Wkeep, W, sizeof(double) * ld * n, hipMemcpyDeviceToDevice, e->stream));
  bool need_pinv = cx.xs == ADMM_XSOLVE_PINV;
  if (!need_pinv) {
    const int rc = factorize(e, W, n, ld, nullptr, mk);
    if (rc != ADMM_OK && rc != ADMM_E_NUMERIC) return rc;
    need_pinv = rc == ADMM_E_NUMERIC || gram_singular(e, n);
    if (need_pinv) {
      release_slice_factor(e, e->xfac);
      e->mem.free_one(W);
    }
  }
  if (need_pinv) ADMM_TRY(factorize_pinv(e, Wkeep, n, ld));
  else e->mem.free_one(Wkeep);
  return build_unwrapped_pinv(e, nullptr);
}

static int setup_qp_bounded(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t n = desc->n;
  const int mk = cx.mk;
  if (!desc->P || !desc->q || !desc->lb || !desc->ub || n <= 0)
    return fail(ADMM_E_INVALID, "bounded QP needs P (n x n), q, lb, ub");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_BOX;
  e->rhs_kind = RHS_RHO_MINUS_Q;
  ADMM_TRY(upload_matrix(e->mem, &e->Pmat, &e->ldP, desc->P, n, n, n, mk, e->stream));
  ADMM_TRY(upload(e->mem, &e->q, desc->q, n, mk, e->stream));
  ADMM_TRY(upload(e->mem, &e->lb, desc->lb, n, mk, e->stream));
  ADMM_TRY(upload(e->mem, &e->ub, desc->ub, n, mk, e->stream));
  e->rhs_add = e->q;
  const int64_t ld = e->ldP;
  double* W = nullptr;
  ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ld) * n));
  if (!desc->L) {  // getProxOps.m:640-641  chol(P + rho*I)
    ADMM_HIP_TRY(hipMemcpyAsync(W, e->Pmat, sizeof(double) * ld * n, hipMemcpyDeviceToDevice, e->stream));
    launch_add_diag(W, n, ld, desc->rho, e->stream);
  }
  ADMM_TRY(factorize(e, W, n, ld, desc->L, mk));
  // the objective 1/2 x'Px + q'x + r needs P*x
  e->planSq = gemv_t_plan(n, n, ld);
  ADMM_TRY(e->mem.alloc(&e->partSq, e->planSq.part_elems(1)));
  // ... or, with the engine's own factor, nothing: P x = y - rho*x from the right-hand side the x-update solved
  // with (OBJX_SOLVE_QP), calibrated against the P*x form in the first batch like the lasso objective
  if (!desc->L && desc->obj_gram >= 0) {
    e->obj_alt = true;
    e->obj_auto = desc->obj_gram == 0;
    ADMM_TRY(e->mem.alloc(&e->gobjpart, kMaxPartBlocks + 2));
  }
  return ADMM_OK;
}

static int setup_basis_pursuit(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const bool from_data = !desc->P && desc->D && desc->s && m > 0 && n > m;
  if (!from_data && (!desc->P || !desc->q || n <= 0))
    return fail(ADMM_E_INVALID, "basis pursuit needs the projector P (n x n) and q, or a fat D (m < n) and s");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_DIFF;
  if (from_data) {  // basispursuit.m:116-120 on the device
    ADMM_TRY(with_data_copy(e, desc, cx, true, [&](const double* D, int64_t ld, const double* s) {
      return build_bp_projector(e, D, m, n, ld, s);
    }));
    e->m = n;
  } else {
    ADMM_TRY(upload_matrix(e->mem, &e->Pmat, &e->ldP, desc->P, n, n, n, cx.mk, e->stream));
    ADMM_TRY(upload(e->mem, &e->q, desc->q, n, cx.mk, e->stream));
  }
  e->planSq = gemv_t_plan(n, n, e->ldP);
  ADMM_TRY(e->mem.alloc(&e->partSq, e->planSq.part_elems(1)));
  e->xsolve = ADMM_XSOLVE_INVERSE;  // x = P*(z-u) + q is a GEMV by construction
  return ADMM_OK;
}

// model.m:111-128 + getProxOps.m:83-95: x - z = c with quadratic f and g given by their Gram data.
// Either half may be left out (NULL): it must then be supplied by admm_engine_set_callbacks.
static int setup_model(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const int mk = cx.mk;
  if (n <= 0) return fail(ADMM_E_INVALID, "the model / generic problem needs n (args.n, getProxOps.m:89)");
  if ((desc->P != nullptr) != (desc->q != nullptr) || (desc->Q != nullptr) != (desc->qz != nullptr))
    return fail(ADMM_E_INVALID, "model: PtP comes with Ptr and QtQ with Qts (getProxOps.m:83-88)");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_GIVEN;
  e->rhs_kind = RHS_RHO_DTS;  // y = rho*(z-u) + Ptr   (getProxOps.m:978)
  if (cx.xs == ADMM_XSOLVE_CG) return fail(ADMM_E_UNSUPPORTED, "xsolve=cg needs a data matrix");
  if (desc->c) {
    ADMM_TRY(upload(e->mem, &e->s, desc->c, n, mk, e->stream));
    e->c = e->s;
  }
  e->has_xfac = desc->P != nullptr;
  if (desc->P) {
    ADMM_TRY(upload(e->mem, &e->q, desc->q, n, mk, e->stream));
    e->rhs_add = e->q;
    double* W = nullptr;
    int64_t ld = 0;
    ADMM_TRY(upload_matrix(e->mem, &W, &ld, desc->P, n, n, n, mk, e->stream));
    launch_add_diag(W, n, ld, desc->rho, e->stream);  // getProxOps.m:972-975
    ADMM_TRY(factorize(e, W, n, ld, nullptr, mk));
  } else {
    e->rhs_kind = RHS_NONE;
  }
  if (desc->Q) {
    ADMM_TRY(upload(e->mem, &e->qz, desc->qz, n, mk, e->stream));
    double* W = nullptr;
    int64_t ld = 0;
    ADMM_TRY(upload_matrix(e->mem, &W, &ld, desc->Q, n, n, n, mk, e->stream));
    launch_add_diag(W, n, ld, desc->rho, e->stream);  // getProxOps.m:1005-1008
    ADMM_TRY(build_slice_factor(e, e->zfac, W, n, ld, e->xsolve_requested, nullptr, mk));
    e->has_zfac = true;
  }
  // optional: the matrices of the objective 1/2||P*x-r||^2 + 1/2||Q*z-s||^2 (model.m:133-134)
  if (desc->D && desc->s && desc->D2 && desc->s2 && m > 0 && desc->m2 > 0) {
    ADMM_TRY(upload_matrix(e->mem, &e->D, &e->ldD, desc->D, m, n, src_ld(desc), mk, e->stream));
    ADMM_TRY(upload(e->mem, &e->ell, desc->s, m, mk, e->stream));  // r (kept apart from the constraint vector)
    e->planDN = gemv_n_plan(m, n, e->ldD);
    ADMM_TRY(e->mem.alloc(&e->partDN, e->planDN.part_elems()));
    e->m2 = desc->m2;
    ADMM_TRY(upload_matrix(e->mem, &e->D2, &e->ldD2, desc->D2, e->m2, n, desc->ldD2 ? desc->ldD2 : e->m2, mk,
                           e->stream));
    ADMM_TRY(upload(e->mem, &e->s2, desc->s2, e->m2, mk, e->stream));
    e->planD2N = gemv_n_plan(e->m2, n, e->ldD2);
    ADMM_TRY(e->mem.alloc(&e->partD2N, e->planD2N.part_elems()));
  }
  const int64_t n2 = round_up(n, 2);
  for (double** p : {&e->xext, &e->zext, &e->xh, &e->rz}) ADMM_TRY(e->mem.alloc(p, n2));
  return ADMM_OK;
}

// linear program and standard-form QP: the x-update is the affine map x = K*y + k0 (build_kkt_map)
static int setup_lp_qp_standard(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const int mk = cx.mk;
  const bool qp = desc->problem == ADMM_PROB_QP_STANDARD;
  const bool from_data = !desc->K && desc->D && desc->s && m > 0 && m < n;
  if ((!from_data && (!desc->K || !desc->k0)) || !desc->q || n <= 0 || (qp && !desc->P))
    return fail(ADMM_E_INVALID, qp ? "standard-form QP needs P, q and either the reduced KKT map K, k0 or D, s"
                                   : "linear program needs b (as q) and either the reduced KKT map K, k0 or D, s");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_POS;             // getProxOps.m:1381, 1425
  e->rhs_kind = RHS_RHO_MINUS_Q;  // y = rho*(z-u) - b   (getProxOps.m:1363, 1410)
  if (qp) ADMM_TRY(upload_matrix(e->mem, &e->Pmat, &e->ldP, desc->P, n, n, n, mk, e->stream));
  if (from_data) {  // the KKT elimination on the device, for desc.rho
    ADMM_TRY(with_data_copy(e, desc, cx, true, [&](const double* D, int64_t ld, const double* s) {
      return build_kkt_map(e, D, m, n, ld, s, qp ? e->Pmat : nullptr, e->ldP, desc->rho);
    }));
    e->m = n;
  } else {
    ADMM_TRY(upload_matrix(e->mem, &e->Kmat, &e->ldK, desc->K, n, n, n, mk, e->stream));
    ADMM_TRY(upload(e->mem, &e->k0, desc->k0, n, mk, e->stream));
  }
  ADMM_TRY(upload(e->mem, &e->q, desc->q, n, mk, e->stream));
  e->rhs_add = e->q;
  e->ell = e->q;  // objective b'*x (linearprogram.m:178) reads it as the dot vector
  e->planK = gemv_t_plan(n, n, e->ldK);
  ADMM_TRY(e->mem.alloc(&e->partK, e->planK.part_elems(1)));
  if (qp) {  // the objective 1/2 x'Px + q'x + r needs P*x
    e->planSq = gemv_t_plan(n, n, e->ldP);
    ADMM_TRY(e->mem.alloc(&e->partSq, e->planSq.part_elems(1)));
  }
  e->xsolve = ADMM_XSOLVE_INVERSE;  // a GEMV by construction
  return ADMM_OK;
}

// device tables of the column / row transform of length len (dct.h): the power-of-two network, or for any other length
// the chirp form -- an FFT of length M >= 2*len - 1 behind every column pair.  (Also behind the stand-alone operators
// of ops.hip, with a memory owner of their own.)
int admm::dct_tables_create(DevMem& mem, hipStream_t stream, int64_t len, DctTables* t) {
  const int32_t L = static_cast<int32_t>(len);
  const bool chirp = !dct_length_ok(L);
  const int32_t M = chirp ? dct_chirp_fft_length(L) : L;  // length of the FFT network
  std::vector<admm_double2> tw(static_cast<size_t>(M / 2)), c4(static_cast<size_t>(chirp ? L : L / 2 + 1)),
      ch(static_cast<size_t>(chirp ? L : 0)), hb(static_cast<size_t>(chirp ? M : 0));
  std::vector<double> lam(static_cast<size_t>(L));
  if (chirp) dct_fill_chirp_tables(L, tw.data(), c4.data(), lam.data(), ch.data(), hb.data());
  else dct_fill_tables(L, tw.data(), c4.data(), lam.data());
  auto bind = [&](const std::vector<admm_double2>& host, const admm_double2** dev) -> int {
    double* d = nullptr;
    ADMM_TRY(upload(mem, &d, reinterpret_cast<const double*>(host.data()), 2 * host.size(), ADMM_MEM_HOST, stream));
    *dev = reinterpret_cast<const admm_double2*>(d);
    return ADMM_OK;
  };
  *t = DctTables{};
  t->odd_pair = -1;
  t->n = L;
  double* dlam = nullptr;
  ADMM_TRY(bind(tw, &t->tw));
  ADMM_TRY(bind(c4, &t->c4));
  ADMM_TRY(upload(mem, &dlam, lam.data(), L, ADMM_MEM_HOST, stream));
  t->lam = dlam;
  if (chirp) {
    ADMM_TRY(bind(ch, &t->chirp));
    ADMM_TRY(bind(hb, &t->hbr));
    t->bm = M;
  }
  int32_t& log2len = chirp ? t->log2bm : t->log2n;
  while ((1 << log2len) < M) ++log2len;
  ADMM_HIP_TRY(hipStreamSynchronize(stream));  // the host vectors go out of scope
  return ADMM_OK;
}

// 2-D anisotropic TV of an m x n image (column-major): z, u have 2*m*n entries ([vertical; horizontal])
static int setup_tv2d(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  if (!desc->s || m <= 0 || n <= 0) return fail(ADMM_E_INVALID, "2-D total variation needs the m x n image in s");
  if (desc->lambda < 0) return fail(ADMM_E_INVALID, "Given lambda parameter is not a nonnegative number!");
  const int64_t N = m * n;
  e->tv2_H = m;
  e->tv2_W = n;
  e->m = 2 * N;
  e->n = N;  // length of the CG vectors
  e->a_identity = false;
  e->nA = N;
  e->len = 2 * N;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_NONE;
  if (desc->cg_tol <= 0 || desc->cg_tol == 1e-12) e->cg_tol = 1e-11;
  if (desc->cg_maxit <= 0 || desc->cg_maxit == 200) {
    e->cg_maxit = 500;
    e->cg_maxit_auto = true;  // (raised per run to what rho needs: engine_run_tv.hip)
  }
  ADMM_TRY(upload(e->mem, &e->s, desc->s, N, cx.mk, e->stream));
  ADMM_TRY(e->mem.alloc(&e->tv_zB, round_up(2 * N, 2)));
  ADMM_TRY(e->mem.alloc(&e->tv_uB, round_up(2 * N, 2)));
  if (cx.tv2_want_dct) {
    ADMM_TRY(dct_tables_create(e->mem, e->stream, m, &e->dctH));
    e->tv2_rows_dct = dct_length_ok(n);
    if (e->tv2_rows_dct) ADMM_TRY(dct_tables_create(e->mem, e->stream, n, &e->dctW));
    e->tv2_dct = true;
  }
  return ADMM_OK;
}

// totalvariation.m:122-157: s is the (column) signal, D = spdiags([1 -1],0:1,n,n) is implicit
static int setup_total_variation(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t nn = desc->n > 0 ? desc->n : desc->m;
  if (!desc->s || nn <= 0) return fail(ADMM_E_INVALID, "Argument s is not a vector! (totalvariation.m:197)");
  if (desc->lambda < 0) return fail(ADMM_E_INVALID, "Given lambda parameter is not a nonnegative number!");
  e->m = e->n = nn;
  e->a_identity = false;
  e->nA = nn;
  e->len = nn;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_NONE;
  ADMM_TRY(upload(e->mem, &e->s, desc->s, nn, cx.mk, e->stream));
  ADMM_TRY(e->mem.alloc(&e->tv_y, round_up(nn, 2)));
  ADMM_TRY(e->mem.alloc(&e->tv_y2, round_up(nn, 2)));
  ADMM_TRY(alloc_zeroed_block(e, &e->ctrl_idle));
  ADMM_TRY(e->mem.alloc(&e->tv_zB, round_up(nn, 2)));
  ADMM_TRY(e->mem.alloc(&e->tv_uB, round_up(nn, 2)));
  return ADMM_OK;
}

// consensus lasso, after the slice factors: the exchange buffers, and what lets the K x-solves share launches
static int consensus_exchange_buffers(admm_engine* e, int64_t n) {
  e->cldn = round_up(n, 2);
  const size_t K = e->cslices.size();
  ADMM_TRY(e->mem.alloc(&e->cX, K * e->cldn));
  ADMM_TRY(e->mem.alloc(&e->cU, K * e->cldn));
  ADMM_TRY(e->mem.alloc(&e->csums, 2 * e->cldn + 2));  // + the packed scalar of the one-collective exchange
  for (double** p : {&e->czc, &e->cxave, &e->cxaveprev, &e->cubar}) ADMM_TRY(e->mem.alloc(p, e->cldn));
  // every slice applies an explicit inverse through the lower-triangle kernel: keep one set of partial rows per
  // slice, summed by the exchange kernel itself (launch_cons_gather_sum) instead of K symv_reduce launches
  bool all_half = n >= kSymvHalfMin;
  for (const ConsSlice& sl : e->cslices) all_half = all_half && !sl.fat && sl.fac.mode == ADMM_XSOLVE_INVERSE;
  if (all_half && ceil_div(n, 128) <= kMaxPartBlocks) {
    e->cpstride = static_cast<int64_t>(e->cslices[0].fac.planSy.npart_elems());
    for (double** p : {&e->csyN, &e->csyT}) ADMM_TRY(e->mem.alloc(p, K * static_cast<size_t>(e->cpstride)));
    ADMM_HIP_TRY(hipMemsetAsync(e->csyN, 0, sizeof(double) * K * e->cpstride, e->stream));
    ADMM_HIP_TRY(hipMemsetAsync(e->csyT, 0, sizeof(double) * K * e->cpstride, e->stream));
  }
  // the K slice inverses are each read once per iteration: they share the Infinity-Cache budget of the split policy
  for (ConsSlice& sl : e->cslices)
    if (sl.fac.Minv) sl.fac.planSy.ncached = symv_cached_tiles(sl.fac.planSy, kSymvCacheBytes / K);
  if (e->csyN) {  // all slices packed and of one size: their x-solves run as ONE launch
    bool packed = true;
    std::vector<const double*> hp;
    for (const ConsSlice& sl : e->cslices) {
      packed = packed && sl.fac.planSy.packed;
      hp.push_back(sl.fac.Minv);
    }
    if (packed) {
      double* raw = nullptr;
      ADMM_TRY(e->mem.alloc(&raw, hp.size()));  // K pointers in K doubles
      ADMM_HIP_TRY(hipMemcpyAsync(raw, hp.data(), sizeof(double*) * hp.size(), hipMemcpyHostToDevice, e->stream));
      ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
      e->cMptr = reinterpret_cast<const double**>(raw);
    }
  }
  ADMM_TRY(e->mem.alloc(&e->cY, K * e->cldn));
  ADMM_TRY(e->mem.alloc(&e->cDts, K * e->cldn));
  ADMM_HIP_TRY(hipMemsetAsync(e->cDts, 0, sizeof(double) * K * e->cldn, e->stream));
  for (size_t k = 0; k < K; ++k)
    ADMM_HIP_TRY(hipMemcpyAsync(e->cDts + k * e->cldn, e->cslices[k].Dts, sizeof(double) * n, hipMemcpyDeviceToDevice,
                                e->stream));
  return e->mem.alloc(&e->cobjpart, K * kMaxPartBlocks);
}

// lasso.m:193-224 + getProxOps.m:383-442: one (D_k, D_k's_k, chol(D_k'D_k + rho*I)) per row slice
static int setup_consensus_lasso(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  const int mk = cx.mk;
  if (!desc->D || !desc->s || m <= 0 || n <= 0) return fail(ADMM_E_INVALID, "lasso needs D (m x n) and s");
  if (desc->lambda < 0) return fail(ADMM_E_INVALID, "lambda must be a nonnegative real (lasso.m:132)");
  if (desc->nslices < 1 || !desc->slices) return fail(ADMM_E_INVALID, "consensus lasso needs args.slices");
  int64_t tot = 0;
  for (int32_t k = 0; k < desc->nslices; ++k) {
    if (desc->slices[k] <= 0) return fail(ADMM_E_INVALID, "empty slice");
    tot += desc->slices[k];
  }
  if (tot != m)
    return fail(ADMM_E_INVALID, "The number of parallel slices does not match length of x! (errorcheck.m:264)");
  e->a_identity = true;
  e->nA = n;
  e->len = n;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_NONE;
  double slices_all = static_cast<double>(desc->nslices);  // slicenum over all ranks
  ADMM_TRY(allreduce_scalar(e, &slices_all));
  e->cons_total = static_cast<int32_t>(slices_all + 0.5);
  const int64_t ld = round_up(n, 16);
  e->cslices.resize(desc->nslices);
  int64_t r0 = 0;
  for (int32_t k = 0; k < desc->nslices; ++k) {
    ConsSlice& sl = e->cslices[k];
    sl.m = desc->slices[k];
    ADMM_TRY(upload_matrix(e->mem, &sl.D, &sl.ld, desc->D + r0, sl.m, n, src_ld(desc), mk, e->stream));
    ADMM_TRY(upload(e->mem, &sl.s, desc->s + r0, sl.m, mk, e->stream));
    sl.planN = gemv_n_plan(sl.m, n, sl.ld);
    sl.planT = gemv_t_plan(sl.m, n, sl.ld);
    if (k == 0 || sl.planN.part_elems() > e->planDN.part_elems()) e->planDN = sl.planN;  // largest = buffer size
    if (k == 0 || sl.planT.part_elems(1) > e->planDT.part_elems(1)) e->planDT = sl.planT;
    r0 += sl.m;
  }
  ADMM_TRY(e->mem.alloc(&e->partDN, e->planDN.part_elems()));
  ADMM_TRY(e->mem.alloc(&e->partDT, e->planDT.part_elems(1)));
  int64_t fat_rows = 0;
  for (ConsSlice& sl : e->cslices) {
    ADMM_TRY(e->mem.alloc(&sl.Dts, round_up(n, 2)));
    launch_gemv_t(sl.planT, sl.D, sl.s, nullptr, nullptr, 1, e->partDT, nullptr, e->stream);
    launch_sum_partials_t(sl.planT, e->partDT, 1, sl.Dts, round_up(n, 2), nullptr, e->stream);
    // tall slice: chol(D_k'D_k + rho I) (getProxOps.m:424, 429-435).  Fat slice (rows < columns), documented
    // deviation q12: the reference's branch (getProxOps.m:426-430, 1251) shifts the wrong entries of D_k D_k' and is
    // exact for no rho; the engine applies the serial solver's form, chol(D_k D_k'/rho + I) with
    // x = y/rho - D_k'(U\(L\(D_k y)))/rho^2 (lasso.m:172, getProxOps.m:1204) = the Woodbury identity of
    // (D_k'D_k + rho I)^-1 y
    sl.fat = sl.m < n;
    const int64_t nF = sl.fat ? sl.m : n, ldF = sl.fat ? round_up(sl.m, 16) : ld;
    double* W = nullptr;
    ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ldF) * nF));
    ADMM_TRY(gram_lower(e, sl.D, sl.ld, sl.m, n, sl.fat, sl.fat ? 1.0 / desc->rho : 1.0, W, ldF));
    launch_add_diag(W, nF, ldF, sl.fat ? 1.0 : desc->rho, e->stream);
    ADMM_TRY(build_slice_factor(e, sl.fac, W, nF, ldF, e->xsolve_requested, nullptr, mk));
    if (sl.fat && sl.m > fat_rows) fat_rows = sl.m;
  }
  if (fat_rows > 0) {
    ADMM_TRY(e->mem.alloc(&e->tmpA, round_up(fat_rows, 2)));
    ADMM_TRY(e->mem.alloc(&e->tmpB, round_up(fat_rows, 2)));
  }
  return consensus_exchange_buffers(e, n);
}

// covarianceselection.m:145-172: A = 1, B = -1, c = 0, x/z/u the n x n matrices flattened (every norm of admm.m
// is 'fro', perr uses sqrt(numel)): the vector loop on n^2 elements with the lasso z-prox (getProxOps.m:750)
static int setup_covsel(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  const int64_t m = desc->m, n = desc->n;
  if (n < 1) return fail(ADMM_E_INVALID, "covariance selection needs n >= 1 (S is n x n)");
  if (!(desc->lambda > 0.0))
    return fail(ADMM_E_INVALID, "lambda must be a positive real (covarianceselection.m: errorcheck 'ispositivereal')");
  if (e->comm) return fail(ADMM_E_UNSUPPORTED, "covariance selection runs on one device (desc.comm must be NULL)");
  if (cx.xs != ADMM_XSOLVE_AUTO)
    return fail(ADMM_E_UNSUPPORTED, "covariance selection has one x-update (the eigen-step): desc.xsolve must be AUTO");
  const int64_t nn = n * n;
  e->a_identity = true;
  e->nA = nn;
  e->len = nn;
  e->prox = PROX_SOFT;
  e->rhs_kind = RHS_DIFF;  // the x-update reads z - u (v - uhat in fast ADMM)
  e->cov_ld = round_up(n, 16);
  const int64_t ld = e->cov_ld;
  if (desc->P) {
    ADMM_TRY(upload(e->mem, &e->cov_S, desc->P, static_cast<size_t>(nn), cx.mk, e->stream));
    std::vector<double> h(static_cast<size_t>(nn));
    ADMM_HIP_TRY(hipMemcpyAsync(h.data(), e->cov_S, sizeof(double) * nn, hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    double amax = 0.0, asym = 0.0;
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = j; i < n; ++i) {
        const double a = h[i + j * n], b = h[j + i * n];
        amax = std::max(amax, std::max(std::fabs(a), std::fabs(b)));
        asym = std::max(asym, std::fabs(a - b));
        if (!std::isfinite(a) || !std::isfinite(b)) asym = INFINITY;
      }
    if (!(asym <= 1e-12 * amax))
      return fail(ADMM_E_INVALID, "covariance selection: S must be a finite symmetric matrix (|S - S'| <= "
                                  "1e-12 * max|S|)");
  } else if (desc->D) {  // S = cov(D), covarianceselection.m:150: centre the columns, then the Gram / (m - 1)
    if (m < 2) return fail(ADMM_E_INVALID, "covariance selection: cov(D) needs at least two samples (m >= 2)");
    double* W = nullptr;
    ADMM_TRY(with_data_copy(e, desc, cx, false, [&](double* D, int64_t ldd, const double*) -> int {  // (centred in place)
      ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ld) * n));
      ADMM_TRY(e->mem.alloc(&e->cov_S, static_cast<size_t>(nn)));
      covsel_cov(D, ldd, m, n, W, ld, e->cov_S, e->stream);
      ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
      return ADMM_OK;
    }));
    e->mem.free_one(W);
  } else {
    return fail(ADMM_E_INVALID, "covariance selection needs S (desc.P, n x n) or the samples (desc.D, m x n)");
  }
  e->ell = e->cov_S;  // the weights of trace(S*X) = sum S_ij X_ij (OBJX_DOT)
  ADMM_TRY(e->mem.alloc(&e->cov_V, static_cast<size_t>(ld) * n));
  ADMM_HIP_TRY(hipMemsetAsync(e->cov_V, 0, sizeof(double) * ld * n, e->stream));
  ADMM_TRY(e->mem.alloc(reinterpret_cast<double**>(&e->cov_cnt), 1));
  if (n <= kCovselSmallMax) return covsel_small_prepare();
  CovselLarge& c = e->cov_big;
  c.n = n;
  c.ld = ld;
  c.V = e->cov_V;
  for (double** p : {&c.W, &c.B, &c.T}) {
    ADMM_TRY(e->mem.alloc(p, static_cast<size_t>(ld) * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * ld * n, e->stream));
  }
  ADMM_TRY(e->mem.alloc(&c.lam, static_cast<size_t>(2 * n)));
  ADMM_TRY(e->mem.alloc(&c.sig, static_cast<size_t>(1 + 2 * n)));
  return e->mem.alloc(reinterpret_cast<double**>(&c.rot), 1);
}

// the stream, the fields every problem shares and the x-solve option checks; fills cx
static int check_options(admm_engine* e, const admm_problem_desc* desc, CreateCtx* cx) {
  e->device = desc->device;
  e->comm = desc->comm;
  ADMM_TRY(comm_stream_create(e->comm, &e->stream));
  e->problem = desc->problem;
  e->m = desc->m;
  e->n = desc->n;
  e->lambda = desc->lambda;
  e->C = desc->C;
  e->rconst = desc->r;
  e->loss = desc->loss;
  e->rho_factor = desc->rho;
  if (!(desc->rho > 0.0)) return fail(ADMM_E_INVALID, "rho must be a positive real (lasso.m:138)");

  const int prob = desc->problem;
  const bool data_problem = prob == ADMM_PROB_LASSO || prob == ADMM_PROB_LAD || prob == ADMM_PROB_HUBERFIT ||
                            prob == ADMM_PROB_LINEARSVM;  // the x-update solves with D'D (+ rho I)
  int xs = desc->xsolve;
  if (xs < ADMM_XSOLVE_AUTO || xs > ADMM_XSOLVE_PINV) return fail(ADMM_E_INVALID, "bad desc.xsolve");
  if (xs == ADMM_XSOLVE_PINV && prob != ADMM_PROB_LINEARSVM)
    return fail(ADMM_E_UNSUPPORTED, "xsolve=pinv is the linear SVM / unwrapped ADMM x-update (unwrappedadmm.m:76-78)");
  // AUTO stays AUTO here: build_slice_factor resolves it per factor (the explicit inverse while its accuracy probe
  // holds, else the blocked triangular solves: probe_and_choose)
  e->xsolve_requested = (xs == ADMM_XSOLVE_TRSV || xs == ADMM_XSOLVE_INVERSE) ? xs : ADMM_XSOLVE_AUTO;
  cx->sharded = e->comm && comm_nranks(e->comm) > 1;
  if (xs == ADMM_XSOLVE_CALLBACK && prob != ADMM_PROB_LAD)
    return fail(ADMM_E_UNSUPPORTED, "xsolve=callback is the generic A = D engine: use ADMM_PROB_LAD with D = A, s = c");
  if (xs == ADMM_XSOLVE_CALLBACK && cx->sharded)
    return fail(ADMM_E_UNSUPPORTED, "prox callbacks are not supported on row-sharded engines");
  // 2-D TV: the spectral x-update when the column transform supports the height (a power of two, or the chirp form
  // of dct.hip up to 4096) at any width -- run() picks the row stage, and falls back to CG for a rho where none fits;
  // CG outright on request.  The CG vectors are allocated either way: the spectral solve uses them as scratch.
  cx->tv2_want_dct = prob == ADMM_PROB_TV2D && desc->xsolve != ADMM_XSOLVE_CG &&
                     (dct_length_ok(desc->m) || dct_chirp_length_ok(desc->m));
  if (prob == ADMM_PROB_TV2D) xs = ADMM_XSOLVE_CG;
  if (xs == ADMM_XSOLVE_CG && prob != ADMM_PROB_TV2D && !data_problem)
    return fail(ADMM_E_UNSUPPORTED, "xsolve=cg applies to problems whose x-update solves with D'D (+ rho I)");
  e->xsolve = xs;
  e->cg_tol = desc->cg_tol > 0 ? desc->cg_tol : 1e-12;
  e->cg_maxit = desc->cg_maxit > 0 ? desc->cg_maxit : 200;
  if (cx->sharded && !data_problem && prob != ADMM_PROB_LASSO_CONSENSUS)
    return fail(ADMM_E_UNSUPPORTED, "row sharding applies to problems with a data matrix D (lasso/LAD/Huber/SVM)");
  double rows_all = static_cast<double>(desc->m);  // rows of D over all ranks
  ADMM_TRY(allreduce_scalar(e, &rows_all));
  cx->xs = xs;
  cx->mk = desc->mem;
  cx->m_global = cx->sharded ? static_cast<int64_t>(rows_all + 0.5) : desc->m;
  e->len_global = 0;
  return ADMM_OK;
}

static int setup_problem(admm_engine* e, const admm_problem_desc* desc, const CreateCtx& cx) {
  switch (desc->problem) {
    case ADMM_PROB_LASSO: return cx.sparse ? setup_lasso_sparse(e, desc, cx) : setup_lasso(e, desc, cx);
    case ADMM_PROB_LAD:
    case ADMM_PROB_HUBERFIT:
    case ADMM_PROB_LINEARSVM: return setup_lad_huber_svm(e, desc, cx);
    case ADMM_PROB_QP_BOUNDED: return setup_qp_bounded(e, desc, cx);
    case ADMM_PROB_BASISPURSUIT: return setup_basis_pursuit(e, desc, cx);
    case ADMM_PROB_MODEL: return setup_model(e, desc, cx);
    case ADMM_PROB_LINEARPROGRAM:
    case ADMM_PROB_QP_STANDARD: return setup_lp_qp_standard(e, desc, cx);
    case ADMM_PROB_TV2D: return setup_tv2d(e, desc, cx);
    case ADMM_PROB_TOTALVARIATION: return setup_total_variation(e, desc, cx);
    case ADMM_PROB_LASSO_CONSENSUS: return setup_consensus_lasso(e, desc, cx);
    case ADMM_PROB_COVSEL: return setup_covsel(e, desc, cx);
    default: return fail(ADMM_E_INVALID, "Invalid input for problem - not a solver (getProxOps.m:916)");
  }
}

// what every problem needs after its own setup: iterates and scratch, the CG vectors, the control blocks, ||c||
static int setup_common(admm_engine* e) {
  const int64_t L2 = round_up(e->len, 2), N2 = round_up(e->nA, 2);
  ADMM_TRY(e->mem.alloc(&e->x, N2));
  ADMM_TRY(e->mem.alloc(&e->z, L2));
  ADMM_TRY(e->mem.alloc(&e->u, L2));
  ADMM_TRY(e->mem.alloc(&e->rhs, L2 > N2 ? L2 : N2));
  for (double** p : {&e->v, &e->uhat, &e->zprev, &e->uprev}) ADMM_TRY(e->mem.alloc(p, L2));
  if (!e->a_identity && e->problem != ADMM_PROB_TOTALVARIATION && e->problem != ADMM_PROB_TV2D) {
    ADMM_TRY(e->mem.alloc(&e->dz, L2));
    e->ldg = N2;
    ADMM_TRY(e->mem.alloc(&e->g, 3 * N2 + 16));  // + 16 reduction slots: one all-reduce payload
  }
  ADMM_TRY(e->mem.alloc(&e->red, 32));  // packed scalar payloads of the sharded runs
  if (e->xsolve == ADMM_XSOLVE_CG) {
    for (double** p : {&e->cg_r, &e->cg_p, &e->cg_q, &e->cg_tmp}) ADMM_TRY(e->mem.alloc(p, N2));
    ADMM_TRY(e->mem.alloc(&e->cg_part, 2 * kMaxPartBlocks));
    ADMM_TRY(alloc_zeroed_block(e, &e->cg_st));
    ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->cg_st_host), sizeof(CgState), hipHostMallocDefault));
    ADMM_TRY(alloc_zeroed_block(e, &e->cg_skip));
  }
  e->tv_zA = e->z;
  e->tv_uA = e->u;
  ADMM_TRY(e->mem.alloc(&e->part, static_cast<size_t>(S_COUNT) * kMaxPartBlocks));
  ADMM_TRY(e->mem.alloc(&e->objpart, 2 * kMaxPartBlocks));  // the model objective has two residual terms
  ADMM_TRY(alloc_zeroed_block(e, &e->ctrl));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->ctrl_host), sizeof(Ctrl), hipHostMallocDefault));
  if (e->c) {  // ||c||  (admm.m:650), over the row shards
    double ss = 0.0;
    ADMM_TRY(device_sumsq_host(e, e->c, e->len, &ss));
    ADMM_TRY(allreduce_scalar(e, &ss, e->red));
    e->cnorm = std::sqrt(ss);
  }
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  return ADMM_OK;
}

// sparse: null, or the checked matrix of admm_engine_create_sparse in HOST arrays
static int create_engine(const admm_problem_desc* desc, const admm_sparse_desc* sparse, admm_engine** out,
                         bool keep_fp64 = false) {
  const auto t0 = std::chrono::steady_clock::now();
  admm_engine* e = new admm_engine();
  e->keep_fp64 = keep_fp64;
  CreateCtx cx{};
  cx.sparse = sparse;
  int rc = check_options(e, desc, &cx);
  if (rc == ADMM_OK) rc = setup_problem(e, desc, cx);
  if (rc == ADMM_OK) rc = setup_common(e);
  if (rc != ADMM_OK) {  // the one place a half-built engine is given up
    admm_engine_destroy(e);
    return rc;
  }
  e->setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = e;
  return ADMM_OK;
}

// the checks both create entries make before an engine object exists; selects the device
static int check_device(const admm_problem_desc* desc, admm_engine** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_problem_desc)))
    return fail(ADMM_E_INVALID, "admm_problem_desc.struct_size mismatch (ABI version skew)");
  *out = nullptr;
  int ndev = 0;
  ADMM_TRY(admm_device_count(&ndev));
  if (ndev <= 0) return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  if (desc->device < 0 || desc->device >= ndev) return fail(ADMM_E_INVALID, "bad device ordinal");
  ADMM_HIP_TRY(hipSetDevice(desc->device));
  return ADMM_OK;
}

extern "C" int admm_engine_create(const admm_problem_desc* desc, admm_engine** out) {
  ADMM_TRY(check_device(desc, out));
  return create_engine(desc, nullptr, out);
}

int admm::engine_create_keep_fp64(const admm_problem_desc* desc, admm_engine** out) {
  ADMM_TRY(check_device(desc, out));
  return create_engine(desc, nullptr, out, true);
}

extern "C" int admm_engine_create_sparse(const admm_problem_desc* desc, const admm_sparse_desc* D, admm_engine** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (!D) return fail(ADMM_E_INVALID, "the sparse matrix is NULL");
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_problem_desc)))
    return fail(ADMM_E_INVALID, "admm_problem_desc.struct_size mismatch (ABI version skew)");
  // what a sparse engine does not do, before anything touches the device
  if (desc->problem != ADMM_PROB_LASSO)
    return fail(ADMM_E_UNSUPPORTED, "a sparse design matrix is supported for the lasso only (ADMM_PROB_LASSO)");
  if (desc->D) return fail(ADMM_E_INVALID, "admm_engine_create_sparse: desc.D must be NULL (the matrix is the sparse one)");
  if (desc->m != D->rows || desc->n != D->cols)
    return fail(ADMM_E_INVALID, "admm_engine_create_sparse: desc.m / desc.n differ from the rows / cols of the matrix");
  if (desc->xsolve != ADMM_XSOLVE_AUTO && desc->xsolve != ADMM_XSOLVE_CG)
    return fail(ADMM_E_UNSUPPORTED, "a sparse engine runs the matrix-free x-update only (xsolve = auto or cg): nothing "
                                    "n x n is ever formed");
  if (desc->L) return fail(ADMM_E_UNSUPPORTED, "args.L with a sparse design matrix: no factor is used");
  if (desc->nslices > 1) return fail(ADMM_E_UNSUPPORTED, "consensus lasso on a sparse design matrix");
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, "a sparse design matrix on a row-sharded engine");
  if (D->mem != ADMM_MEM_HOST && D->mem != ADMM_MEM_DEVICE) return fail(ADMM_E_INVALID, "bad admm_sparse_desc.mem");
  if (D->mem == ADMM_MEM_HOST) ADMM_TRY(sparse_csc_check(D));  // (before the device is even looked for)
  ADMM_TRY(check_device(desc, out));
  admm_sparse_desc host;
  std::vector<double> val;
  std::vector<uint64_t> ir, jc;
  ADMM_TRY(sparse_to_host(D, &host, &val, &ir, &jc));
  if (D->mem == ADMM_MEM_DEVICE) ADMM_TRY(sparse_csc_check(&host));
  admm_problem_desc d = *desc;
  d.xsolve = ADMM_XSOLVE_CG;
  return create_engine(&d, &host, out);
}
