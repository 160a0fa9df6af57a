/*
 * admm_engine.h -- C ABI of libadmm_hip.so, the MI355X (gfx950) ADMM iteration engine.
 *
 * Drop-in boundary for the hot path of PeterSutor/ADMM-Project: the loop of
 * `results = admm(xminf, zming, options)` (reference admm.m:24, loop 496-743) when
 * both prox handles come from `getproxops(problem, args)` (getProxOps.m:13).  The
 * reference has no native layer at all; these are the entry points a MEX (or ctypes)
 * binding for that path binds -- see INTEGRATION.md for the reference-side stub.
 *
 * Conventions: plain C, no C++/torch types.  All matrices are column-major fp64
 * (MATLAB layout).  Every function returns 0 on success and a negative ADMM_E_* code
 * on failure; admm_last_error() returns the thread-local message.  An engine handle
 * is not re-entrant; one host thread drives one device.
 *
 * Environment: the library reads five variables and no others (one reader, csrc/common.h: env_switches).  Each makes
 * the engine take a path that it otherwise picks by measurement or by shape; they exist for the tests and for A/B
 * measurements, not as tuning knobs, and every path they reach is a production path.  They are read when the named
 * call runs, never cached.
 *   ADMM_HIP_GRAPH               (run)    replay batches of iterations as a captured hipGraph where the iteration
 *                                         allows it; the default is eager launches (never slower, EXPERIMENTS.md)
 *   ADMM_TRSV_FORM=blocked|one   (create, admm_op_trsv_pair) the form of the triangular solves, overriding the
 *                                         create-time accuracy probe: blocked substitution / one pre-inverted block
 *   ADMM_HIP_XSPLIT=0|1          (create) multi-GPU explicit-inverse x-solve: keep / split the tiles over the ranks,
 *                                         overriding the decision taken from the measured all-reduce latency
 *   ADMM_HIP_NO_UNWRAPPED_FUSED  (create) no explicit pinv(D) is built, so the linear SVM runs the general A = D
 *                                         iteration instead of the two-launch unwrapped one
 *   ADMM_HIP_NO_ONEPASS          (run)    the general A = D iteration instead of the one-pass form for tall, narrow D
 */
#ifndef ADMM_ENGINE_H
#define ADMM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADMM_ABI_VERSION 5

/* ---- error codes ------------------------------------------------------------ */
enum {
  ADMM_OK = 0,
  ADMM_E_INVALID = -1,     /* bad argument (mirrors the reference's error() calls) */
  ADMM_E_UNSUPPORTED = -2, /* valid in the reference, not engine-native (yet) */
  ADMM_E_DEVICE = -3,      /* HIP runtime / no GPU */
  ADMM_E_NUMERIC = -4,     /* Cholesky breakdown (matrix not positive definite; lad.m:134 errors the same way) */
  ADMM_E_COMM = -5,        /* RCCL */
  ADMM_E_CAPACITY = -6     /* destination buffer too small */
};

/* ---- problem kinds: the cases of getproxops' switch (getProxOps.m:52-917) ---- */
enum {
  ADMM_PROB_LASSO = 1,            /* getProxOps.m:313-456 serial; x: 1192-1206, z: 455 */
  ADMM_PROB_LASSO_CONSENSUS = 2,  /* getProxOps.m:383-442, 1217-1343 (args.parallel=1) */
  ADMM_PROB_LAD = 3,              /* getProxOps.m:753-811, x: 1511-1515 */
  ADMM_PROB_HUBERFIT = 4,         /* getProxOps.m:814-912, z: 1529-1539 */
  ADMM_PROB_LINEARSVM = 5,        /* getProxOps.m:202-310, 1062-1180 */
  ADMM_PROB_TOTALVARIATION = 6,   /* getProxOps.m:145-199, 1044-1048 */
  ADMM_PROB_QP_BOUNDED = 7,       /* getProxOps.m:631-641, 1441-1474 */
  ADMM_PROB_BASISPURSUIT = 8,     /* getProxOps.m:98-142, 1027-1032 */
  ADMM_PROB_LINEARPROGRAM = 10,   /* getProxOps.m:459-542, x: 1357-1366 (KKT solve), z: 1378-1382 */
  ADMM_PROB_QP_STANDARD = 11,     /* getProxOps.m:624-630, x: 1397-1412 (KKT solve), z: 1422-1426 */
  ADMM_PROB_TV2D = 12,            /* engine-side extension: 2-D TV of an m x n image (D = [Dv; Dh] forward
                                     differences), anisotropic or -- admm_engine_set_tv2d_isotropic -- isotropic; x-update of I + rho*D'D spectral (column DCT + row stage) where the
                                     height has a column transform, matrix-free CG otherwise or with ADMM_XSOLVE_CG; no
                                     reference counterpart (totalvariation.m is 1-D) -- BASELINE config 5 as literally written */
  ADMM_PROB_COVSEL = 13,          /* getProxOps.m:669-750 (z: soft threshold lambda/rho, 745-750), x: 1487-1495
                                     (eigen-step of rho*(z-u) - S); covarianceselection.m:145-172 on the n^2 entries of
                                     the n x n X: S = desc.P (n x n), or desc.D (m x n samples, S = cov(D) built on the
                                     device), lambda = desc.lambda */
  ADMM_PROB_MODEL = 9             /* getProxOps.m:60-95, x: 952-979, z: 990-1013 (model.m); with both prox
                                     callbacks set and no data it is the generic admm(xminf, zming, options)
                                     of admm.m:24 for A = 1, B = -1 */
};

/* linear-SVM loss (getProxOps.m:1094: anything but '01' runs the hinge prox) */
enum { ADMM_LOSS_HINGE = 0, ADMM_LOSS_01 = 1,
       ADMM_LOSS_HINGE_OBJ01 = 2 /* any other lossfunction string (e.g. linearsvmtest.m:157 passes '0-1'): the hinge
                                    prox runs, but linearsvm.m:231-237 installs the 0-1 objective */,
       ADMM_LOSS_LOGISTIC = 3 /* g(z) = C*sum log(1 + exp(-ell.*z)): not in the reference, whose unwrapped ADMM takes
                                 any separable z-prox (unwrappedadmm.m:76-92); 'logistic'  */,
       /* (4 is unassigned and refused) */
       ADMM_LOSS_SQHINGE = 5 /* g(z) = C*sum max(1 - ell.*z, 0).^2, the L2-loss SVM: not in the reference either;
                                'sqhinge' (DESIGN.md q34).  z = v where ell.*v >= 1, else ell.*(ell.*v + 2t)/(1 + 2t),
                                t = C/rho */ };

/* how the cached-factor x-update is applied every iteration */
enum {
  ADMM_XSOLVE_AUTO = 0,    /* INVERSE if it passes the accuracy probe below, else TRSV */
  ADMM_XSOLVE_TRSV = 1,    /* two triangular solves with the Cholesky factor (reference form: getProxOps.m:1200, 1514),
                              as blocked substitution: 2K + 1 bandwidth-bound launches, K = ceil(n / 2048) */
  ADMM_XSOLVE_INVERSE = 2, /* one symmetric n x n GEMV with the explicit inverse, built once.  Its forward error grows
                              like cond^1.5 * eps, so create() solves a system with a known solution with both forms
                              and keeps the explicit inverse only while it is as accurate as the triangular solves
                              (or below 1e-9); otherwise the triangular solves run (admm_engine_info reports which
                              form is in use and the probe errors) */
  ADMM_XSOLVE_CG = 3,      /* matrix-free conjugate gradients on (D'D + rho I), A-streaming */
  ADMM_XSOLVE_CALLBACK = 4,/* A = D problems (LAD shape: A x - z = c): no factor is built, D may have any shape;
                              every run needs an xminf callback (admm_engine_set_callbacks) -- the generic
                              results = admm(xminf, zming, options) with a matrix options.A (admm.m:117-120) */
  ADMM_XSOLVE_PINV = 5     /* linear SVM only: x = pinv(D)*(z-u) (linearsvm.m:185, unwrappedadmm.m:76-78) through the
                              pseudo-inverse of D'D (Jacobi eigen-decomposition, eigenvalues <= n*eps*max dropped).
                              AUTO / TRSV / INVERSE use chol(D'D) while D has full column rank and switch to this
                              form by themselves when the factorisation breaks down or its pivots reach the
                              rounding level (rank-deficient D: e.g. MNIST pixels that are zero in every sample) */
};

/* where the desc's data pointers live */
enum { ADMM_MEM_HOST = 0, ADMM_MEM_DEVICE = 1 };

/* stopcond (admm.m:69, 710-722) */
enum { ADMM_STOP_STANDARD = 0, ADMM_STOP_HNORM = 1, ADMM_STOP_BOTH = 2,
       ADMM_STOP_NONE = 3 /* any other string: the reference's strcmp chain matches nothing */ };

/* fast ADMM flavour (admm.m:63-64, 267-298) */
enum { ADMM_FAST_OFF = 0, ADMM_FAST_WEAK = 2 /* accelerated, alg 2 */, ADMM_FAST_STRONG = 1 /* alg 1 */ };

typedef struct admm_engine admm_engine; /* opaque */

/*
 * Caller-supplied proximal operators: the `xminf` / `zming` function handles of admm.m:24 when they are
 * NOT the library's own (examples/convergencechecking.m:125-136 mixes both kinds).  All pointers are
 * DEVICE pointers into the engine's state; the callback enqueues its work on `hip_stream` (a hipStream_t)
 * or synchronises before returning, and writes its result to `out` (never aliased with an input).
 *   xmin: out[nA] = xminf(x[nA], z[nB], u[nB], rho)   admm.m:502 (fast ADMM passes v, uhat: 506)
 *   zmin: out[nB] = zming(xh, z[nB], u[nB], rho)      admm.m:521-530; xh is x (nA elements) or, when
 *                                                      options.relax != 1, the relaxed Axhat (nB elements)
 *   obj : *out    = obj(x[nA], z[nB])                 admm.m:603-605
 * A non-zero return aborts the run with ADMM_E_INVALID.  Speculatively enqueued iterations after a stop
 * condition still invoke the callbacks; their outputs are discarded on the device.
 */
typedef int (*admm_prox_callback)(void* user, const double* x, const double* z, const double* u, double rho,
                                  double* out, int64_t nout, void* hip_stream);
typedef int (*admm_obj_callback)(void* user, const double* x, int64_t nA, const double* z, int64_t nB, double* out,
                                 void* hip_stream);
/* The two remaining caller-handle fields of the loop (ABI 4), same conventions (device pointers, hip_stream):
 *   altu : out[m] = options.altu(u[m], Ax[m], Bz[m], c[m])   admm.m:553-559 -- replaces the u-update; Ax is the relaxed
 *          Axhat when options.relax != 1 (admm.m:555), c is a zero vector when the constraint has none
 *   norms: out[0..1] = options.specialnorms(x[nA], z[nB], u[m], rho)   admm.m:612-616 -- replaces pnorm / dnorm (perr / derr
 *          are computed as always, admm.m:640-658) */
typedef int (*admm_altu_callback)(void* user, const double* u, const double* Ax, const double* Bz, const double* c,
                                  int64_t m, double* out, void* hip_stream);
typedef int (*admm_norms_callback)(void* user, const double* x, int64_t nA, const double* z, int64_t nB, const double* u,
                                   int64_t m, double rho, double* out2, void* hip_stream);
/* Caller-supplied constraint operators: options.A / options.At as function handles (admm.m:117-158).
 *   out[nout] = A(in[nin])  or  At(in[nin]);  device pointers, enqueue on hip_stream, non-zero return aborts the run */
typedef int (*admm_operator_callback)(void* user, const double* in, int64_t nin, double* out, int64_t nout,
                                      void* hip_stream);
typedef struct admm_comm admm_comm;     /* opaque RCCL communicator wrapper */

/*
 * Problem description = what lasso.m:181-189 / lad.m:129-134 / huberfit.m:161-166 /
 * linearsvm.m:210-214 / totalvariation.m:139-144 / quadraticprogram.m:212-218 pass to
 * getproxops in `args`, as flat pointers.  Unused pointers are NULL.  With
 * ADMM_MEM_HOST the engine copies everything at create (caller may free afterwards);
 * with ADMM_MEM_DEVICE the big matrix D (or P) is borrowed and must outlive the engine.
 */
typedef struct admm_problem_desc {
  int32_t struct_size; /* sizeof(admm_problem_desc), for ABI evolution */
  int32_t problem;     /* ADMM_PROB_* */
  int64_t m, n;        /* rows / columns of D (local rows when row-sharded); P is n x n */
  const double* D;     /* m x n, column-major */
  int64_t ldD;         /* leading dimension of D (>= m) */
  const double* s;     /* length m (LAD/Huber/lasso) or n (total variation signal) */
  const double* ell;   /* length m, labels +-1 (linear SVM) */
  const double* P;     /* n x n: QP matrix, or basis-pursuit projector */
  const double* q;     /* length n: QP linear term, or basis-pursuit offset */
  const double* lb;    /* length n (QP bounded) */
  const double* ub;    /* length n (QP bounded) */
  const double* L;     /* optional precomputed lower Cholesky factor (args.L, lasso.m:183) */
  double lambda;       /* lasso / TV regularisation */
  double C;            /* SVM regularisation */
  double r;            /* QP constant term */
  double rho;          /* rho the cached factor is built for (args.rho) */
  int32_t loss;        /* ADMM_LOSS_* */
  int32_t userelax;    /* args.userelax (lad.m:124-126) */
  int32_t xsolve;      /* ADMM_XSOLVE_* */
  int32_t mem;         /* ADMM_MEM_* */
  int32_t device;      /* HIP device ordinal */
  int32_t nslices;     /* consensus lasso: number of LOCAL row slices (>=1) */
  const int64_t* slices; /* their sizes (sum == m), slicemaker order (errorcheck.m:216-267) */
  admm_comm* comm;     /* NULL = single device; else rows are sharded across the ranks */
  double cg_tol;       /* ADMM_XSOLVE_CG: relative residual tolerance (default 1e-12) */
  int32_t cg_maxit;    /* ADMM_XSOLVE_CG: iteration cap per x-update (default 200) */
  int32_t obj_gram;    /* lasso (and, in the same way, the bounded QP's 1/2*x'Px + q'x, quadraticprogram.m:242), factor
                          built by the engine: how the objective's 1/2*||D*x - s||^2 (lasso.m:227) is
                          evaluated.  The Gram form is 1/2*x'Gx - x'D's + 1/2*s's with G = D'D; since x solves
                          (G + rho*I) x = y (y = rho*(z - u) + D's, getProxOps.m:1195), G x = y - rho*x and the form
                          is a sum over the element update's own operands -- no pass over D (8mn B) or G at all.  Its
                          absolute error is ~1e-16*||s||^2 plus x'(residual of the x-solve).
                          0 = automatic: the engine
                              evaluates BOTH forms during the first host batch of the first objevals run (the
                              literal values are the ones recorded) and switches to the Gram form only if they agreed
                              to 1e-11 relative; 1 = the Gram form always; -1 = the literal D*x form always */
  /* ADMM_PROB_MODEL (getProxOps.m:83-89): P = args.PtP, q = args.Ptr above; and */
  const double* Q;     /* n x n: args.QtQ */
  const double* qz;    /* length n: args.Qts */
  /* optional data of the model objective 1/2||P*x - r||^2 + 1/2||Q*z - s||^2 (model.m:133-134):
   * D = P (m x n), s = r above; and */
  const double* D2;    /* m2 x n: the matrix Q */
  int64_t m2, ldD2;
  const double* s2;    /* length m2: the vector s */
  const double* c;     /* optional constraint vector (length n) of x - z = c; NULL = 0 (model.m:127) */
  /* ADMM_PROB_LINEARPROGRAM / ADMM_PROB_QP_STANDARD: the KKT solve [M D'; D 0] \ [y; s] of
   * getProxOps.m:1363 / 1410 (M = rho*I or P + rho*I) reduced ONCE by the binding to the affine map
   * x = K*y + k0,  K = inv(M) - inv(M) D' inv(S) D inv(M) (symmetric, n x n),  k0 = inv(M) D' inv(S) s,
   * S = D inv(M) D'  (built for desc.rho).  y = rho*(z-u) - q with q = the linear cost (args.b / args.q). */
  const double* K;
  const double* k0;
  /* ADMM_PROB_LINEARSVM: optional pseudo-inverse computed by the caller, n x m column-major, ld = n
   * (args.Dplus = pinv(D), linearsvm.m:185-186).  When given, the x-update is literally x = Dplus*(z-u)
   * (getProxOps.m:1067): one GEMV with it, nothing is factored.  NULL: the engine forms the map from D'D itself. */
  const double* Dplus;
  /* ADMM_PROB_LASSO: optional D'*s (args.Dts, lasso.m:160, 182); the serial args struct carries no s
   * (getProxOps.m:445-451).  Without s the engine-native objective (objevals) is unavailable. */
  const double* Dts;
} admm_problem_desc;

/* POD mirror of the `options` struct read by admm.m:51-76 (defaults: setopt, 780-971). */
typedef struct admm_options {
  int32_t struct_size;
  int32_t maxiters;     /* default 1000 (admm.m:58, 334-339) */
  double rho;           /* default 1.0 */
  double relax;         /* default 1.0 (admm.m:60, 515-532) */
  double abstol;        /* default 1e-5 */
  double reltol;        /* default 1e-3 */
  double Hnormtol;      /* default 1e-6 (accepts the reference's Hreltol spelling host-side) */
  double convtol;       /* default 1e-10 */
  double restart;       /* default 0.999 */
  double dvaltol;       /* default 1e-8 */
  int32_t domaxiters;   /* default 0 */
  int32_t fast;         /* ADMM_FAST_* */
  int32_t objevals;     /* default 0 */
  int32_t convtest;     /* default 0 */
  int32_t stopcond;     /* ADMM_STOP_* */
  int32_t nodualerror;  /* default 0 */
  int32_t record_history; /* 1 = keep xvals/zvals/uvals like admm.m:608-610; 0 = perf opt-out */
  int32_t check_every;  /* iterations enqueued between host polls of the device stop flag (0 = auto) */
  const double* x0;     /* optional warm start, HOST pointers (admm.m:252-254) */
  const double* z0;
  const double* u0;
  int32_t stale_factor_ok; /* 1 = run with options.rho != the rho the cached factor was built with, as xminLASSO does
                              (getProxOps.m:1192-1206 never re-factors; needed by options.adaptive, admm.m:724-741);
                              0 = refuse the mismatch (default: it is almost always a caller's mistake) */
  int32_t reserved1;
} admm_options;

typedef struct admm_run_summary {
  int32_t steps;               /* results.steps (admm.m:746) */
  int32_t stopped_early;       /* 1 if a stop condition fired before maxiters */
  int32_t convtest_failed_at;  /* >0: iteration where the H-norm monotonicity test aborted (admm.m:686-701) */
  int32_t obj_gram_used;   /* 1: the run ended with the lasso objective in its Gram form (admm_problem_desc.obj_gram) */
  double runtime_s;            /* loop only: tic admm.m:315 .. toc admm.m:756 */
  double objopt;               /* results.objopt (admm.m:752-754), NaN if not evaluated */
} admm_run_summary;

/* result fields for admm_engine_fetch (reference names: admm.m:257-259, 582-616, 648-656, 681-682, 746-754) */
enum {
  ADMM_F_XOPT = 1, ADMM_F_ZOPT = 2, ADMM_F_UOPT = 3,
  ADMM_F_XVALS = 4, ADMM_F_ZVALS = 5, ADMM_F_UVALS = 6, /* len x steps, column-major */
  ADMM_F_PNORM = 7, ADMM_F_DNORM = 8, ADMM_F_PERR = 9, ADMM_F_DERR = 10,
  ADMM_F_OBJEVALS = 11, ADMM_F_HNORMSQ = 12,
  ADMM_F_AVALS = 13, ADMM_F_DVALS = 14, ADMM_F_RESTARTED = 15,
  ADMM_F_VVALS = 16, ADMM_F_UHATVALS = 17,
  ADMM_F_ZCONSENSUS = 18, /* consensus lasso: the true consensus z (the z handed to admm is 0, q9) */
  ADMM_F_FACTOR = 19,     /* n x n (or m x m, fat lasso) lower Cholesky factor */
  ADMM_F_CG_ITERS = 20,   /* matrix-free x-update: [0] inner iterations of the last run in total, [1] (capacity >= 2) the number of
                           * its x-updates that ended on cg_maxit with the residual still above cg_tol (an inexact iterate) */
  ADMM_F_CONS_X = 21,     /* consensus lasso: the local slices' x_k, n x K column-major (closure state xi{k}, getProxOps.m:1247) */
  ADMM_F_CONS_U = 22,     /* consensus lasso: the local slices' u_k (closure state ui{k}, getProxOps.m:1296) */
  ADMM_F_WVALS = 23,      /* (nA + nB + nU) x steps: w = [x; z; rho*u] per iteration, results.wvals of the H-norm runs
                           * (admm.m:678-681); needs the vector histories */
  ADMM_F_COVSEL_S = 24,   /* covariance selection: the n x n S the engine runs with (cov(D) when created from samples);
                           * available before the first run */
  ADMM_F_TV2D_ROW_STAGE = 25,/* 2-D total variation: one value, the ADMM_TV2D_ROWS_* form the row stage of the last run's
                           * spectral x-update took (the three-launch iteration included); 0 when the x-update was CG */
  ADMM_F_SPARSE_NNZ = 26  /* an engine of admm_engine_create_sparse: [0] the stored nonzeros of D, [1] / [2] (capacity >= 3)
                           * the lanes per row of the D*v and of the D'*v product (csrc/spmv.h); available before the
                           * first run.  ADMM_E_INVALID on a dense engine */
};

/* ---- library ---------------------------------------------------------------- */
int admm_abi_version(void);
const char* admm_last_error(void);
int admm_device_count(int* count);
/* name[cap] gets the gcnArchName; hbm_bytes/cus may be NULL */
int admm_device_info(int device, char* name, size_t cap, int64_t* hbm_bytes, int32_t* cus);

/* ---- engine lifecycle --------------------------------------------------------
 * create   = the solver's one-time setup + getproxops (lasso.m:160-192, lad.m:129-137, ...):
 *            uploads data, builds Gram matrix / Cholesky factor / pseudo-inverse on device.
 * run      = admm(minx, minz, options): the iteration loop, entirely on device.
 * fetch    = copy one results.* field into caller memory (MEX: mxGetPr of the output).
 */
void admm_options_default(admm_options* opts);
void admm_problem_desc_default(admm_problem_desc* desc);
int admm_engine_create(const admm_problem_desc* desc, admm_engine** out);
/* A lasso engine on a SPARSE design matrix (engine-side extension: DESIGN.md q35).  D arrives as real double CSC,
 * MATLAB's own storage; its arrays are copied at create whichever memory they live in.  The device keeps D by rows and
 * D' by rows (12 B per nonzero each: int64 row starts, int32 indices, fp64 values); the x-update is the warm-started CG
 * of ADMM_XSOLVE_CG on (D'D + rho I) with two sparse matrix-vector products per inner iteration (csrc/spmv.hip: no
 * atomics, one fixed summation order per row), and the objective's 1/2*||D*x - s||^2 is evaluated literally with the
 * same product.  Nothing n x n is formed, so tall and fat matrices are both accepted.  The z-side -- admm_engine_set_groups,
 * admm_engine_set_penalty -- every option and every history are those of a dense xsolve = cg lasso engine.
 *   desc: problem = ADMM_PROB_LASSO, D = NULL, m = D->rows, n = D->cols, s (or Dts) per desc->mem, lambda, rho, cg_tol,
 *         cg_maxit, device; xsolve ADMM_XSOLVE_AUTO and ADMM_XSOLVE_CG both mean CG; obj_gram is ignored
 * ADMM_E_INVALID (nothing is uploaded, no engine is created; the message names the first offending column): desc->D
 * given, m / n that differ from rows / cols, rows, cols or nnz not below 2^31, jc[0] != 0, a decreasing jc,
 * jc[cols] != nnz, a row index >= rows, row indices not strictly increasing inside a column (unsorted or duplicate
 * entries), a value that is not finite.
 * ADMM_E_UNSUPPORTED: xsolve TRSV / INVERSE / PINV (callback as well), desc->L, nslices > 1, desc->comm, any problem other
 * than the lasso (LAD, Huber and the SVM on sparse data are out of scope). */
typedef struct admm_sparse_desc {
  int32_t struct_size;  /* sizeof(admm_sparse_desc) */
  int32_t mem;          /* ADMM_MEM_HOST or ADMM_MEM_DEVICE: where val / ir / jc live */
  int64_t rows, cols, nnz;
  const double* val;    /* nnz values */
  const uint64_t* ir;   /* their row indices */
  const uint64_t* jc;   /* column starts, cols + 1 entries */
} admm_sparse_desc;
int admm_engine_create_sparse(const admm_problem_desc* desc, const admm_sparse_desc* D, admm_engine** out);
/* replace the x- and/or z-update (and the objective hook) of an A = 1 problem (tall lasso, QP, LP, basis
 * pursuit, model) or an A = D problem (LAD, Huber, linear SVM: the zming handle of
 * unwrappedadmm(zming, D, options), unwrappedadmm.m:1) by caller-supplied callbacks; NULL keeps the
 * engine-native operator.  x has nA = n elements; z, u and zmin's first argument have nB elements (n or m).
 * ADMM_PROB_MODEL created without Gram data REQUIRES the corresponding callback. */
int admm_engine_set_callbacks(admm_engine* eng, admm_prox_callback xmin, void* xuser, admm_prox_callback zmin,
                              void* zuser, admm_obj_callback obj, void* objuser);
/* options.A / options.At as function handles: an engine created as ADMM_PROB_LAD with ADMM_XSOLVE_CALLBACK and
 * desc.D = NULL (desc.m = rows of A = length of z, u, c; desc.n = length of x; desc.s = c) has no matrix at all --
 * A*x, At*(.) of the dual residual / tolerance (admm.m:535, 624, 654) are these callbacks, both required; B = -1. */
int admm_engine_set_operators(admm_engine* eng, admm_operator_callback A, void* Auser, admm_operator_callback At,
                              void* Atuser);
/* options.altu / options.specialnorms as the CALLER's handles (admm.m:553-559, 612-616; the consensus-lasso hooks of
 * getproxops' `extra` are engine-native and need none of this).  Plain ADMM only (the reference never combines them with
 * fast / accelerated ADMM: q5), any engine of the general loop (not consensus lasso / total variation, not row-sharded).
 * With a hook set the iteration leaves the fused one-launch tails: element update, hook, a small fix-up kernel, finalize.
 * NULL, NULL restores the engine's own u-update and norms. */
int admm_engine_set_hooks(admm_engine* eng, admm_altu_callback altu, void* altu_user, admm_norms_callback norms,
                          void* norms_user);
/* options.B other than the shorthand -1 (admm.m:198-245): a scalar (B = NULL, Bop = NULL: B = scalar*I), an m x nB
 * matrix (column-major, leading dimension ldB, host or device pointer per memkind = ADMM_MEM_*), or a function handle
 * Bop(z[nB]) -> out[m].  Only for engines whose two prox operators are BOTH the caller's (ADMM_PROB_MODEL created
 * without Gram data, or ADMM_PROB_LAD with ADMM_XSOLVE_CALLBACK): the library's own operators are written for
 * B = -1.  Afterwards z, v and zming's result have nB elements (callbacks, options.z0, ADMM_F_ZOPT / ZVALS / VVALS);
 * u, c and the relaxed Axhat keep m.  B enters the loop linearly (admm.m:515, 536-552, 573, 621-658, 305), so the
 * device loop carries w = -B*z and runs the same fused kernels. */
int admm_engine_set_constraint_b(admm_engine* eng, const double* B, int64_t ldB, int64_t nB, int32_t memkind,
                                 double scalar, admm_operator_callback Bop, void* Buser);
/* Group lasso (engine-side extension, no reference counterpart: DESIGN.md q30): the z-prox of an ADMM_PROB_LASSO
 * engine becomes the block soft threshold of lambda * sum_g weights[g] * ||z_g||_2 over ngroups contiguous groups of
 * the n coefficients (sizes[g] >= 1, sum == n; weights >= 0, NULL = 1 for every group), and objevals reports
 * 1/2*||D*x - s||^2 + lambda * sum_g weights[g] * ||z_g||.  The x-update, every option and every x-solve form stay the
 * lasso's; a zming callback still replaces the z-update.  sizes == NULL or ngroups == 0 restores the l1 prox.
 * ADMM_E_INVALID: a size below 1, sizes that do not sum to n, a negative or non-finite weight; ADMM_E_UNSUPPORTED: any
 * other problem (consensus lasso included), a row-sharded engine.  One group of n elements is one workgroup walking
 * all of them twice per iteration: correct, slow. */
int admm_engine_set_groups(admm_engine* eng, const int64_t* sizes, int32_t ngroups, const double* weights);
/* The lasso's penalty family (engine-side extension: DESIGN.md q32).  The z-side term of an ADMM_PROB_LASSO engine is
 *   g(z) = lambda1 * sum_i l1weights[i]*|z_i| + lambdaG * sum_g omega_g*||z_g||_2 + ridge/2*||z||^2 + [z >= 0 if nonnegative]
 * Without groups lambda1 is the engine's lambda and the group term is absent; with admm_engine_set_groups in force
 * lambdaG is the engine's lambda with the groups' weights omega_g, as before, and lambda1 is the field l1 (read only
 * then).  Adaptive lasso / an unpenalised intercept (l1weights), elastic net (ridge), non-negative lasso (nonnegative)
 * and the sparse-group lasso (groups + l1) are its members.  Only the z-prox changes, with v = (Ax^ + u) - c:
 *   e_i = sign(v_i)*max(|v_i| - (lambda1/rho)*l1weights[i], 0)      (nonnegative: max(v_i - (lambda1/rho)*l1weights[i], 0))
 *   with groups: e_g *= (||e_g|| > t_g ? 1 - t_g/||e_g|| : 0),  t_g = (lambda/rho)*omega_g
 *   z = rho/(rho + ridge) * e
 * and objevals reports 1/2*||D*x - s||^2 + g(z).  The x-update and its cached factor (ridge never enters it), every
 * option and every x-solve form stay the lasso's, with the plain lasso's launches per iteration; a zming callback still
 * replaces the z-update.  Defaults: l1weights NULL (every weight 1), l1 = 0, ridge = 0, nonnegative = 0 -- with all of
 * them the engine is the plain (or group) lasso, bit for bit.  desc == NULL restores the defaults.  The call is
 * independent of the order of admm_engine_set_groups; l1weights (n HOST values) are copied.
 * ADMM_E_INVALID: a negative or non-finite weight, l1 or ridge; nonnegative outside {0, 1} -- a refused call changes
 * nothing.  ADMM_E_UNSUPPORTED: any other problem (consensus lasso included), a row-sharded engine; at run time, more
 * than 131072 coefficients without groups. */
typedef struct admm_penalty_desc {
  const double* l1weights;
  double l1;
  double ridge;
  int32_t nonnegative;
} admm_penalty_desc;
int admm_engine_set_penalty(admm_engine* eng, const admm_penalty_desc* desc);
/* what is in force (admm_engine_info_t has no reserved field left): l1, ridge, nonnegative into *desc (its l1weights is
 * set to NULL) and whether weights are held into *has_l1weights (nullable) */
int admm_engine_get_penalty(admm_engine* eng, admm_penalty_desc* desc, int32_t* has_l1weights);
/* The loss family of the robust-regression engines (engine-side extension: DESIGN.md q33).  With the constraint
 * D*x - z = s, the z-side term of an ADMM_PROB_LAD or ADMM_PROB_HUBERFIT engine is g(z) = sum_i weights[i]*phi(z_i):
 *   LAD engine:    phi(z) = slope_pos*max(z - epsilon, 0) + slope_neg*max(-z - epsilon, 0)
 *                  (LAD: 1, 1, 0; the tau-quantile: slope_pos = tau, slope_neg = 1 - tau; the epsilon-insensitive loss of
 *                  support vector regression: 1, 1, epsilon > 0)
 *   Huber engine:  phi(z) = (z >= 0 ? slope_pos : slope_neg)*H_delta(z),  H_delta(z) = z^2/2 for |z| <= delta and
 *                  delta*|z| - delta^2/2 beyond (at the defaults the reference's 1/2*huber)
 * Only the z-prox changes, with v = (Ax^ + u) - c, t_a = weights[i]*slope_pos/rho, t_b = weights[i]*slope_neg/rho:
 *   LAD engine:    z = v - t_a (v > epsilon + t_a), epsilon (v >= epsilon), v (v > -epsilon), -epsilon (v >= -epsilon - t_b),
 *                  v + t_b otherwise: the flats are +-epsilon exactly, the dead zone and a zero weight return v itself
 *   Huber engine:  z = v - clamp(alpha*v/(alpha + rho), 0, alpha*delta/rho) for v >= 0 with alpha = weights[i]*slope_pos,
 *                  z = v - clamp(alpha*v/(alpha + rho), -alpha*delta/rho, 0) for v < 0 with alpha = weights[i]*slope_neg
 * and objevals reports g(z).  The cached factor, both products with D, every option and every iteration form stay the
 * engine's, with its launches per iteration; a zming callback still replaces the z-update.  Defaults: weights NULL
 * (every weight 1), slopes 1, epsilon 0, delta 1 -- with all of them the engine launches the kernels it always did, bit
 * for bit.  desc == NULL restores the defaults.  weights (m HOST values) are copied at the call.
 * ADMM_E_INVALID: another problem; a negative or non-finite weight; a slope <= 0; epsilon < 0, or != 0 on a Huber
 * engine; delta <= 0, or != 1 on a LAD engine -- a refused call changes nothing.  ADMM_E_UNSUPPORTED: a row-sharded
 * engine, the generic callback engine (ADMM_PROB_LAD with ADMM_XSOLVE_CALLBACK). */
typedef struct admm_loss_desc {
  const double* weights;
  double slope_pos;
  double slope_neg;
  double epsilon;
  double delta;
} admm_loss_desc;
int admm_engine_set_loss(admm_engine* eng, const admm_loss_desc* desc);
/* what is in force: the four scalars into *desc (its weights is set to NULL) and whether weights are held into
 * *has_weights (nullable) */
int admm_engine_get_loss(admm_engine* eng, admm_loss_desc* desc, int32_t* has_weights);
/* The costs of the linear SVM (engine-side extension: DESIGN.md q34).  With the constraint D*x - z = 0, the z-side term
 * of an ADMM_PROB_LINEARSVM engine is g(z) = C * sum_i c_i*phi(ell_i*z_i) with
 *   c_i = weights[i]*(ell_i > 0 ? cost_pos : cost_neg)
 * and phi the engine's loss: max(1 - s, 0) (hinge), max(1 - s, 0)^2 (ADMM_LOSS_SQHINGE), log(1 + e^-s) (logistic),
 * [s < 1] (0-1).  Only the z-prox changes, with v = (Ax^ + u) - c, s = ell_i*v, t_i = C*c_i/rho:
 *   hinge     z = v + ell_i*max(min(1 - s, t_i), 0)
 *   sqhinge   z = v (s >= 1), ell_i*(s + 2 t_i)/(1 + 2 t_i) otherwise
 *   logistic  z = ell_i*r, r - s = t_i/(1 + e^r)
 *   0-1       z = ell_i*y, y = s if s >= 1 or s < 1 - sqrt(2 t_i), else 1
 * (c_i = 0 returns v itself), and objevals reports 1/2*||x||^2 + C*sum_i c_i*phi(ell_i*(D*x)_i) (linearsvm.m:231-237
 * with the costs inside the sum; the 0-1 objective of ADMM_LOSS_01 / ADMM_LOSS_HINGE_OBJ01 counts c_i per violated row).
 * The x-update Dplus*(z - u) holds neither ell nor C: the cached map, the one read of D per iteration, every option and
 * every iteration form stay the engine's, with its launches per iteration; a zming callback still replaces the
 * z-update.  Defaults: weights NULL (every weight 1), costs 1 -- with them the engine launches the kernels it always
 * did, bit for bit.  desc == NULL restores the defaults.  weights (m HOST values) are copied at the call.
 * ADMM_E_INVALID: another problem; a negative or non-finite weight or cost -- a refused call changes nothing.
 * ADMM_E_UNSUPPORTED: a row-sharded engine. */
typedef struct admm_svm_cost_desc {
  const double* weights;
  double cost_pos;
  double cost_neg;
} admm_svm_cost_desc;
int admm_engine_set_svm_cost(admm_engine* eng, const admm_svm_cost_desc* desc);
/* what is in force: the two costs into *desc (its weights is set to NULL) and whether weights are held into
 * *has_weights (nullable) */
int admm_engine_get_svm_cost(admm_engine* eng, admm_svm_cost_desc* desc, int32_t* has_weights);
/* Isotropic 2-D total variation (engine-side extension: DESIGN.md q31): with on = 1 an ADMM_PROB_TV2D engine minimises
 * 1/2*||x - s||^2 + lambda * sum_k sqrt((Dx)[k]^2 + (Dx)[N+k]^2), k over the N pixels (the Rudin-Osher-Fatemi norm),
 * instead of the anisotropic lambda*||Dx||_1.  Only the z-update changes: for every pixel k -- those of the last image
 * row / column, whose row of D is zero, included -- the pair v = (u + Dx)[k], (u + Dx)[N+k] is shrunk as a block,
 * z = v * (||v|| > t ? 1 - t/||v|| : 0), t = lambda/rho, u+ = v - z; objevals reports the objective above.  D, the
 * x-update (spectral or CG), the residuals, every option and fast / accelerated ADMM stay as they are; relaxation stays
 * the dimension error it is.  on = 0 (the default) restores the anisotropic prox, bit for bit.  ADMM_E_INVALID: any
 * other problem, on outside {0, 1}. */
int admm_engine_set_tv2d_isotropic(admm_engine* eng, int32_t on);
int admm_engine_run(admm_engine* eng, const admm_options* opts, admm_run_summary* summary);
int admm_engine_fetch(admm_engine* eng, int field, double* dst, size_t cap, size_t* written);
/* what create() decided about the x-update factor (first slice for consensus lasso) */
typedef struct admm_engine_info_t {
  int32_t struct_size;       /* sizeof(admm_engine_info_t), set by the caller */
  int32_t xsolve_requested;  /* desc.xsolve as resolved: AUTO, TRSV or INVERSE */
  int32_t xsolve_used;       /* ADMM_XSOLVE_TRSV or ADMM_XSOLVE_INVERSE (CG / CALLBACK / 0 where no factor exists) */
  int32_t pinv_used;         /* 1: the explicit matrix is the pseudo-inverse of a rank-deficient D'D */
  int32_t probed;            /* 1: both forms were built and compared */
  int32_t trsv_blocks;       /* coarse blocks K of the blocked substitution (0 if not in use) */
  int32_t jacobi_sweeps;     /* sweeps of the eigen-solver (pinv; covariance selection: over the last run) */
  int32_t unwrapped_fused;   /* 1: the two-launch unwrapped iteration with an explicit pinv(D) is available (linear SVM) */
  int64_t factor_n;          /* order of the factor (n; m for fat lasso) */
  int64_t rank;              /* numerical rank (== factor_n unless pinv_used) */
  double cond_estimate;      /* (max L_ii / min L_ii)^2, a lower bound of cond(L L'); pinv: lambda_max / lambda_min kept */
  double probe_err_inverse;  /* max-norm relative forward error of each form on (L L') x = L (L' x0); NaN if not probed */
  double probe_err_trsv;
  double probe_diff;         /* max-norm relative difference of the two forms on an unstructured right-hand side */
  /* bytes of the x-solve's matrix operand one iteration reads, split by cache policy (ABI 4): read with default loads
   * (meant to stay in the 256 MB Infinity Cache from one iteration to the next) / streamed non-temporally from HBM.
   * Consensus lasso: summed over the local slices.  0 / 0 where no n x n operand exists. */
  int64_t xsolve_cacheable_bytes;
  int64_t xsolve_stream_bytes;
  /* lasso / bounded-QP objective through the x-update's right-hand side (desc.obj_gram): the largest value of
   * eps * |cancelling terms| / |objective| any recorded objective of this engine has had (0: form never used); past
   * 1e-10 the engine has gone back to the literal form (obj_form_literal = 1) */
  double obj_bound_max;
  int32_t obj_form_literal;
  int32_t ngroups;           /* groups of admm_engine_set_groups in force (0: the plain l1 prox); the former reserved0 */
  /* ABI 5: the triangular solves' one-block form (the whole factor pre-inverted: two passes, two launches per pair;
   * trsv_blocks = 1 when it is in use): its forward error on the probe system next to probe_err_trsv, which is the
   * blocked substitution's (the yardstick); NaN where it was not built (n < 1536, or the explicit inverse runs) */
  double probe_err_trsv_one;
} admm_engine_info_t;
int admm_engine_info(admm_engine* eng, admm_engine_info_t* info);
/* How the explicit inverse of the engine's own x-update factor is stored: fp64 (tile-packed at order >= 1536, a padded
 * square below), or compact -- off-diagonal 128 x 128 tiles as 48-bit fixed point with one power-of-two scale per tile,
 * 3/4 of the bytes the streamed x-solve reads.  create() builds the compact form where the fp64 packed triangle is too
 * large for the caches, probes it against that triangle on the two systems of the x-solve probe and keeps it while
 * admm_xsolve_compact_accept holds.  stored_bytes: what one x-solve reads (0: no explicit inverse in use).  The three
 * probe numbers -- max-norm relative forward error of the compact and of the fp64 product on (L L') x = L (L' x0),
 * their relative difference on an unstructured right-hand side -- are NaN where the compact form was not built.  Any
 * output pointer may be NULL.  ADMM_STORAGE_COMPACT40: the same format with 40-bit tiles, 5/8 of the bytes, tried first
 * (same rule, then the 48-bit form) where the 48-bit store is larger than the cacheable share of the x-solve; the probe
 * numbers are those of the form in use.  ADMM_STORAGE_COMPACT38 / _COMPACT36: 38- and 36-bit tiles, 19/32 and 9/16 of
 * the bytes, tried (36 first) before the 40-bit form where even the 40-bit store is larger than that share.  The ladder
 * is 36, 38, 40, 48, fp64: the first width the rule accepts is kept, the others are freed. */
enum {
  ADMM_STORAGE_FP64 = 0,
  ADMM_STORAGE_COMPACT = 1,
  ADMM_STORAGE_COMPACT40 = 2,
  ADMM_STORAGE_COMPACT38 = 3,
  ADMM_STORAGE_COMPACT36 = 4
};
int admm_engine_xsolve_storage(admm_engine* eng, int32_t* form, int64_t* stored_bytes, double* probe_err_compact,
                               double* probe_err_fp64, double* probe_diff);
/* The rungs of that ladder create() tried and rejected, in the order tried: *count of them (at most 4); the first
 * min(*count, cap) entries of bits (the tile width), err_compact, err_fp64 and diff (the rung's three probe numbers, as
 * above) are filled.  Any array may be NULL.  The rule gives 0 on every entry. */
int admm_engine_xsolve_rejected(admm_engine* eng, int32_t cap, int32_t* count, int32_t* bits, double* err_compact,
                                double* err_fp64, double* diff);
/* the acceptance rule itself (host arithmetic, no device): 1 while
 * err_compact <= max(1e-11, 4 err_fp64) and diff <= max(1e-11, 8 err_fp64); a NaN anywhere gives 0 */
int admm_xsolve_compact_accept(double err_compact, double err_fp64, double diff);
/* The row stage of the spectral x-update of 2-D total variation (csrc/dct.hip).  admm_tv2d_row_stage is the rule the
 * engine runs (host arithmetic, no device): the form an H x W image takes at this rho -- COOP or GREEN while the
 * Toeplitz kernel's truncation admm_tv2d_rows_green_taps(rho) is at most 96 terms and 4 x it fits the width (COOP:
 * truncation <= 64 and W >= 384), else DCT where W is a power of two in 8 .. 8192 and H is even, else THOMAS.
 * ADMM_E_INVALID (negative) for H, W < 1 or a rho that is not finite and > 0. */
enum { ADMM_TV2D_ROWS_AUTO = 0, ADMM_TV2D_ROWS_GREEN = 1, ADMM_TV2D_ROWS_COOP = 2, ADMM_TV2D_ROWS_DCT = 3,
       ADMM_TV2D_ROWS_THOMAS = 4 };
int admm_tv2d_row_stage(int64_t H, int64_t W, double rho);
int admm_tv2d_rows_green_taps(double rho);
/* The host tables of a column / row transform of length n (8 <= n <= 8192 a power of two: the network; any other
 * 8 <= n <= 4096: the chirp form), exactly as the device receives them (no device needed).  counts[0..4] = entries of
 * tw, c4, lam, chirp, hbr (the last two 0 for the network); tw, c4, chirp and hbr are complex, two doubles per entry.
 * With tw == NULL only the counts are returned; otherwise every table with a non-zero count must be given.
 *   tw[k] = e^{-2 pi i k/M}, k < M/2 (M = n, chirp form: the FFT length);  c4[k] = e^{-i pi k/(2n)};
 *   lam[k] = 4 sin^2(pi k/(2n));  chirp[j] = e^{-pi i j^2/n};  hbr[p] = FFT_M(conj chirp, wrapped)[bitrev(p)] / M */
int admm_dct_tables(int64_t n, double* tw, double* c4, double* lam, double* chirp, double* hbr, int64_t counts[5]);
/* seconds spent in create (upload + factorisation); solverruntime = setup + runtime */
int admm_engine_setup_seconds(admm_engine* eng, double* seconds);
/* per-kernel timing of the last run, measured with HIP events on the engine's stream:
 * which = ADMM_K_*; returns total milliseconds and launch count */
enum { ADMM_K_XSOLVE = 0, ADMM_K_GEMV_N = 1, ADMM_K_GEMV_T = 2, ADMM_K_PROX = 3, ADMM_K_FINALIZE = 4, ADMM_K_COUNT = 5 };
int admm_engine_kernel_time(admm_engine* eng, int which, double* total_ms, int64_t* launches);
/* per-kernel event timing for subsequent runs: mask = OR of (1 << ADMM_K_*), 0 = off (default),
 * negative = every class.  Each timed class costs two hipEventRecord per launch group. */
int admm_engine_set_profiling(admm_engine* eng, int mask);
/* time only every stride-th launch group of each selected class (default 1 = all): a sampled measurement costs the
 * loop 2/stride event records per iteration instead of 2 */
int admm_engine_set_profiling_stride(admm_engine* eng, int stride);
void admm_engine_destroy(admm_engine* eng);

/* ---- binding layer (ABI 5): the getproxops / admm argument structs seen through the C ABI -------------------------
 * A host language (the MATLAB MEX gateway, ctypes, ...) flattens its structs into admm_field entries; everything that
 * INTERPRETS them lives behind the ABI (csrc/binding.hip; host code, no GPU needed): which field means what for which
 * problem (getProxOps.m:52-917: the args struct of getproxops), the defaults of admm's options (admm.m:780-971), what
 * admm refuses before its loop, and the layout of the results struct (admm.m:257-767).  A gateway converts containers
 * and stages function handles; it decides nothing. */
enum { ADMM_FIELD_NUMERIC = 0,  /* full real double array: data, rows, cols (column-major) */
       ADMM_FIELD_TEXT = 1,     /* character vector: text */
       ADMM_FIELD_HANDLE = 2,   /* a function handle (its presence is what counts; the gateway keeps the callable) */
       ADMM_FIELD_SPARSE = 3,   /* real double CSC matrix: data = nonzeros, ir = their rows, jc = column starts (cols + 1);
                                   `reserved`, when not 0, is the number of stored values (else jc[cols] is) */
       ADMM_FIELD_OTHER = 4 };
typedef struct admm_field {
  const char* name;
  int32_t kind;
  int32_t reserved;
  const double* data;
  int64_t rows, cols;
  const char* text;
  const uint64_t* ir;
  const uint64_t* jc;
} admm_field;
typedef struct admm_binding admm_binding;
/* problem: the getproxops problem string ('lasso', 'lad', 'huberfit', 'linearsvm', 'totalvariation', 'quadraticprogram',
 * 'linearprogram', 'basispursuit', 'model'; extensions 'totalvariation2d', 'generic' = both prox operators the caller's);
 * args: the struct getproxops receives; handles: the caller's function handles by name (xminf, zming, obj, A, At, B, altu,
 * specialnorms) plus the scalars a solver keeps next to them (s, r, objnative).  The description borrows the numeric
 * arrays of `args`: they must stay valid until admm_engine_create has returned. */
int admm_binding_create(const char* problem, const admm_field* args, int32_t nargs, const admm_field* handles,
                        int32_t nhandles, admm_binding** out);
void admm_binding_destroy(admm_binding* b);
const admm_problem_desc* admm_binding_desc(const admm_binding* b);
typedef struct admm_binding_info {
  int32_t struct_size;  /* sizeof(admm_binding_info), set by the caller */
  int32_t problem;      /* ADMM_PROB_* */
  int64_t nA, nB, nU;   /* lengths of x, of z, and of u / c / A*x (admm.m:252-254) */
  int32_t a_handle;     /* generic: A and At are function handles (admm_engine_set_operators before a run) */
  int32_t b_kind;       /* generic: 0 = B is the shorthand -1, 1 = another scalar, 2 = a matrix, 3 = a function handle */
  double b_scalar;
  const double* b_matrix;
  int64_t b_ld;
} admm_binding_info;
int admm_binding_get_info(const admm_binding* b, admm_binding_info* info);
/* a 'lasso' binding whose args.D is ADMM_FIELD_SPARSE describes the sparse engine: the matrix, checked as
 * admm_engine_create_sparse checks it (ADMM_E_INVALID, on the host), or NULL for every other binding.  A gateway that
 * gets a matrix here calls admm_engine_create_sparse(admm_binding_desc(b), admm_binding_sparse(b), &engine).  s / Dts of
 * the wrong length are ADMM_E_INVALID; a sparse args.D for any other problem, with args.parallel = 1 or with args.L is
 * ADMM_E_UNSUPPORTED */
const admm_sparse_desc* admm_binding_sparse(const admm_binding* b);
/* a 'lasso' binding also takes the penalty family of admm_engine_set_penalty from its args: `l1weights` (one finite
 * value >= 0 per column of D), `ridge`, `l1` (finite, >= 0) and `nonnegative` (0 or 1), checked by admm_binding_create
 * (ADMM_E_INVALID), refused with parallel = 1 (ADMM_E_UNSUPPORTED) and handed to the engine by admm_binding_apply */
/* a 'lad' or 'huberfit' binding also takes the loss family of admm_engine_set_loss from its args: `weights` (one
 * finite value >= 0 per row of D), `slopes` (two values > 0: positive side, negative side) or its shorthand `tau`
 * (strictly inside (0, 1): slopes tau, 1 - tau; refused beside `slopes`), `epsilon` ('lad') and `delta` ('huberfit'),
 * checked by admm_binding_create (ADMM_E_INVALID) and handed to the engine by admm_binding_apply */
/* a 'linearsvm' binding also takes the costs of admm_engine_set_svm_cost from its args: `weights` (one finite value >= 0
 * per row of D) and `classcost` (two finite values >= 0: cost_pos, cost_neg), checked by admm_binding_create
 * (ADMM_E_INVALID), refused with a communicator (ADMM_E_UNSUPPORTED) and handed to the engine by admm_binding_apply;
 * `lossfunction` = 'sqhinge' selects ADMM_LOSS_SQHINGE */
/* after admm_engine_create: a scalar or matrix B goes to the engine (admm_engine_set_constraint_b), and the groups of a
 * 'lasso' binding whose args carry `groups` (group sizes: integers >= 1 that sum to the columns of D) and optionally
 * `groupweights` (one finite value >= 0 per group) go to admm_engine_set_groups.  admm_binding_create checks both vectors
 * and their element counts (ADMM_E_INVALID) and refuses groups together with parallel = 1 (ADMM_E_UNSUPPORTED) */
int admm_binding_apply(const admm_binding* b, admm_engine* eng);
/* options struct -> admm_options (defaults of admm.m:780-971; x0 / z0 / u0 point into the fields) and the checks admm
 * makes before its loop -- callable BEFORE an engine exists, so that a refused call never holds device memory */
int admm_binding_options(const admm_binding* b, const admm_field* options, int32_t nopt, const admm_field* handles,
                         int32_t nhandles, admm_options* out);
/* the fields of results after a run, in the reference's order (admm.m:257-767) */
enum { ADMM_RES_FETCH = 0,   /* admm_engine_fetch(source = ADMM_F_*), rows x cols */
       ADMM_RES_SCALAR = 1,  /* `scalar` */
       ADMM_RES_START = 2 }; /* the start vector the run used: options.x0 / z0 / u0 (source 0 / 1 / 2) or zeros */
typedef struct admm_result_field {
  const char* name;  /* static storage */
  int32_t kind, source;
  int64_t rows, cols;
  double scalar;
} admm_result_field;
int admm_binding_results(admm_binding* b, const admm_options* opts, const admm_run_summary* summary,
                         admm_result_field* out, int32_t cap, int32_t* count);

/* Host <-> device copies on the engine's stream (hip_stream as handed to a callback, NULL = default stream), complete on
 * return.  For bindings whose callbacks live on the host (a MATLAB function handle staged by the MEX gateway): the
 * gateway needs no HIP headers. */
int admm_memcpy_d2h(void* host_dst, const void* device_src, size_t bytes, void* hip_stream);
int admm_memcpy_h2d(void* device_dst, const void* host_src, size_t bytes, void* hip_stream);

/* ---- stand-alone operators (kernel-level entry points; HOST pointers) ---------
 * The building blocks of the loop, callable on their own: used by the parity tests
 * and by bindings that run a user-supplied prox on the host but want the heavy
 * linear algebra on the device.  Each cites the reference op it replaces.
 */
/* y = D*x  (admm.m:120 `A*v`; getProxOps.m:810, 1088) */
int admm_op_gemv_n(const double* D, int64_t m, int64_t n, int64_t ldD, const double* x, double* y);
/* G(:,k) = D'*V(:,k), k < nrhs <= 4  (admm.m:119/167 `At*v`; getProxOps.m:1514) */
int admm_op_gemv_t(const double* D, int64_t m, int64_t n, int64_t ldD, const double* V, int64_t ldV,
                   int32_t nrhs, double* G, int64_t ldG);
/* The forms those two operators run for an m x n matrix, on the host alone (no device is touched): out = {gemv_n column
 * chunks, gemv_n columns per chunk, gemv_t rows per chunk, gemv_t row chunks, 1 if the matrix loads are non-temporal
 * (the matrix is larger than the caches) else 0}, from the launchers' own planners with the leading dimension the
 * operators give the device copy.  For the tests: a shape meant to reach a form says so here. */
int admm_op_gemv_forms(int64_t m, int64_t n, int32_t out[5]);
/* y = D*x (transpose = 0: x has cols, y rows elements) or y = D'*x (x rows, y cols) for a sparse D in host CSC arrays,
 * by the kernel and the plans of the sparse lasso engine (admm_engine_create_sparse, whose checks of D apply): every
 * row's products are added in one fixed order, so a second call returns the same bits; an empty row gives 0.0 */
int admm_op_spmv(const admm_sparse_desc* D, int transpose, const double* x, double* y);
/* Y = D*X (transpose = 0: X is cols x K, Y rows x K) or Y = D'*X, X and Y column-major on the host, by the multi-vector
 * kernel of the sparse linear SVM (admm_sparse_svm_create; csrc/spmm.hip): one read of D per chunk of
 * admm_sparse_svm_chunk() columns, and column k of Y has the bits admm_op_spmv returns for column k of X */
int admm_op_spmm(const admm_sparse_desc* D, int transpose, int K, const double* X, double* Y);
/* Y(:, k) = omega_k o (D*X(:, k)), omega_ik = obsweights[i] * [fold[i] != heldout[k]]: the forward product of the lasso
 * under observations (admm_sparse_lasso_set_observations, whose arguments and refusals these are) on host
 * arrays, X cols x K and Y rows x K column-major.  Column k has admm_op_spmm's bits times obsweights[i] (one rounding),
 * or those bits themselves without obsweights; a held-out row is +0.0 whatever the product holds (a select, not a
 * multiplication by zero).  The operator itself checks that the columns past K of the last chunk stay +0.0
 * (ADMM_E_NUMERIC).  Every refusal fires before a device is touched. */
int admm_op_spmm_weighted(const admm_sparse_desc* D, int32_t K, const double* X, const double* obsweights, int32_t nfolds,
                          const int32_t* fold, const int32_t* heldout, double* Y);
/* X(:, k) = conjugate gradients on (D'D + shift*I) x = Y(:, k) for K right-hand sides in lock-step: ONE solve of the
 * x-update the sparse multi-fit solvers share (csrc/spmm_cg.hip), through the object, the host loop and
 * the kernels of a run.  Y, X0, X and R are cols x K, column-major on the host.  X0 == NULL: from x = 0 (the first solve
 * of a run); otherwise from X0 (every later one).  A fit ends on ||r|| <= tol*||y||, after maxit inner iterations, on a
 * zero right-hand side (x = 0) or on p.q = 0.  batch > 0 sets the inner iterations enqueued between two polls of the
 * host, batch <= 0 leaves a run's first value; *next_batch (nullable) is the value the solve left for the next one.
 * stop (nullable, K values): nonzero freezes the fit as a stopped ADMM run is frozen -- its columns of X and R come back
 * as a fixed pattern the operator wrote in front of the solve.  R (nullable) is the residual of the recurrence.
 * state holds six values per fit: inner iterations of this solve, inner iterations in total, solves that ended above
 * tol, done, the p.q = 0 exit, the zero right-hand side.
 * The operator itself checks that the columns past K of the last chunk of X, R, P and Q are still +0.0 and that a
 * frozen fit's columns of X, R and P and its state hold the bits they held before the solve (ADMM_E_NUMERIC).
 * ADMM_E_INVALID without a device: a NULL D, Y, X or state, K < 1, tol not positive and finite, maxit < 1, shift negative
 * or not finite, D not in host arrays, and the checks of admm_engine_create_sparse on D */
int admm_op_spmm_cg(const admm_sparse_desc* D, int32_t K, const double* Y, const double* X0, double shift, double tol,
                    int32_t maxit, int32_t batch, const int32_t* stop, double* X, double* R, int64_t* state,
                    int32_t* next_batch);
/* W = D'*D (+ shift on the diagonal), n x n  (lasso.m:168, lad.m:134, unwrappedadmm.m:115) */
int admm_op_gram(const double* D, int64_t m, int64_t n, int64_t ldD, double shift, double* W);
/* in place lower Cholesky of the n x n SPD matrix A (chol(.,'lower'), lasso.m:168) */
int admm_op_cholesky(double* A, int64_t n, int64_t ldA);
/* x = L' \ (L \ y)  (getProxOps.m:1200, 1514) */
int admm_op_trsv_pair(const double* L, int64_t n, int64_t ldL, const double* y, double* x);
/* soft threshold sign(v).*max(abs(v)-t,0)  (getProxOps.m:933-938) */
int admm_op_soft_threshold(const double* v, int64_t n, double t, double* out);
/* block soft threshold over ngroups contiguous groups of the given sizes (sum == n), t_g = lambda_over_rho * weights[g]
 * (weights NULL = 1):  out_g = v_g * (||v_g|| > t_g ? 1 - t_g/||v_g|| : 0) -- the z-prox of group lasso (Boyd et al.
 * 6.4.2; admm_engine_set_groups), the same device code over the same workgroup plan as the loop's element update */
int admm_op_group_soft_threshold(const double* v, int64_t n, const int64_t* sizes, int32_t ngroups,
                                 const double* weights, double lambda_over_rho, double* out);
/* the z-prox of the penalty family (admm_engine_set_penalty) on a host vector, by the same device functions over the
 * same workgroup plan as the loop's element update.  sizes == NULL / ngroups == 0: no groups, and lambda_over_rho is
 * the l1 threshold (tau_i = lambda_over_rho * l1weights[i]); with groups lambda_over_rho is theirs (t_g =
 * lambda_over_rho * groupweights[g]) and tau_i = (desc->l1 / rho) * l1weights[i].  out = rho/(rho + ridge) * e.
 * desc == NULL: the defaults */
int admm_op_penalty_prox(const double* v, int64_t n, const int64_t* sizes, int32_t ngroups, const double* groupweights,
                         double lambda_over_rho, const admm_penalty_desc* desc, double rho, double* out);
/* the z-prox of the loss family (admm_engine_set_loss) on a host vector, by the device function of the loop's element
 * update: problem = ADMM_PROB_LAD or ADMM_PROB_HUBERFIT selects phi, desc == NULL the defaults; desc->weights holds len
 * values.  The refusals are admm_engine_set_loss's. */
int admm_op_loss_prox(const double* v, int64_t len, int32_t problem, const admm_loss_desc* desc, double rho, double* out);
/* the z-prox of the linear SVM with costs (admm_engine_set_svm_cost) on a host vector, by the device function of the
 * loop's element update: out = prox of (C/rho)*c_i*phi(ell_i*.) at v, loss = ADMM_LOSS_* selects phi, desc == NULL the
 * defaults; ell and desc->weights hold len values.  The refusals are admm_engine_set_svm_cost's. */
int admm_op_svm_prox(const double* v, const double* ell, int64_t len, int32_t loss, double C, double rho,
                     const admm_svm_cost_desc* desc, double* out);
/* out = the pair shrink of isotropic 2-D total variation (admm_engine_set_tv2d_isotropic) over a 2N-vector whose halves
 * are paired: (out[k], out[N+k]) = (v[k], v[N+k]) * (||.|| > t ? 1 - t/||.|| : 0); the device function of the loop */
int admm_op_pair_soft_threshold(const double* v, int64_t N, double t, double* out);
/* y = M*x for a symmetric n x n M by the kernels of the explicit-inverse x-update (getProxOps.m:1200).  form selects
 * the launcher: 0 = the small form (one wave per column; reads FULL storage, ldM must be even), 1 = the 128 x 128 tile
 * kernel on padded column-major storage, 2 = the same on tile-packed storage, 3 = the tile-packed launch that carries
 * the deferred finalize step (here without one).  Forms 1 - 3 read the LOWER triangle only: what the caller stores
 * strictly above the diagonal reaches the device as given and must not matter.  ncached: -1 = the plan's cache split,
 * k >= 0 = the first k lower-triangle tiles (row-major triangle order) are read with default loads, the rest
 * non-temporally.  part_count = P >= 1: P launches, launch r taking every P-th tile as rank r of P does in a multi-GPU
 * run, each into zero-filled partial rows; y is the sum of the P partial results in rank order (form 0: P = 1 only). */
int admm_op_symv(const double* M, int64_t n, int64_t ldM, const double* x, int32_t form, int64_t ncached,
                 int32_t part_count, double* y);
/* y = Q*x by the compact storage of the streamed explicit-inverse x-update: the lower triangle of M is tile-packed,
 * quantised (admm_engine_xsolve_storage) and multiplied by the compact instantiation of the tile kernel.  fin != 0: the
 * launch that carries the deferred finalize step (here without one), else the plain tile-packed launch.  ncached and
 * part_count as in admm_op_symv (ncached counts tiles of the compact storage).  Q (optional, ldQ >= n): the symmetric
 * matrix the kernel actually multiplied -- every off-diagonal tile dequantised, the diagonal tiles as given, the lower
 * triangle mirrored. */
int admm_op_symv_compact(const double* M, int64_t n, int64_t ldM, const double* x, int32_t fin, int64_t ncached,
                         int32_t part_count, double* y, double* Q, int64_t ldQ);
/* the same with the tile width chosen: bits = 48 (admm_op_symv_compact itself), 40, 38 or 36; any other width is
 * ADMM_E_INVALID */
int admm_op_symv_compact_bits(const double* M, int64_t n, int64_t ldM, const double* x, int32_t fin, int64_t ncached,
                              int32_t part_count, double* y, double* Q, int64_t ldQ, int32_t bits);
/* Where the compact storage of an order-n matrix puts lower-triangle tile t (row-major triangle order) at that width,
 * in bytes from its start; t = the tile count gives the stored bytes.  Host arithmetic, no device. */
int admm_symv_compact_tile_offset(int64_t n, int32_t bits, int64_t t, int64_t* offset);
/* Y(:,k) = M_k * X(:,k), k < K: K symmetric n x n matrices stored back to back (matrix k at Ms + k*ldM*n), tile-packed
 * and multiplied in ONE batched launch (the slice inverses of consensus lasso); lower triangles only, ncached as above */
int admm_op_symv_batch(const double* Ms, int64_t n, int64_t ldM, int32_t K, const double* X, int64_t ldX,
                       int64_t ncached, double* Y, int64_t ldY);
/* C = alpha*op(A)*op(B) + beta*C (M x N, inner length K; transX: 0 = N, 1 = T) on the fp64 matrix cores, the GEMM of the
 * setup (`D'*D`, the Cholesky updates, the factor inverse).  A, B and C go to the device with the caller's leading
 * dimensions: an odd one selects the guarded tile loader.  A and B are read as (cols-1)*ld + rows doubles; C must hold
 * ldc*N doubles and comes back whole (rows M .. ldc-1 are never written).  beta == 0 never reads C.  lower_only (M == N):
 * only the lower triangle, diagonal included, is defined on return. */
int admm_op_gemm(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
                 int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int32_t lower_only);
/* X = inv(L) for the lower factor L (what it stores above the diagonal is ignored): the 64 x 64 diagonal blocks by
 * substitution, the rest by recursive doubling over batched GEMMs -- every explicit inverse and every pre-inverted
 * panel of the triangular solves is built this way.  X must hold ldX*n doubles and comes back whole: the inverse in its
 * n x n block (zero above the diagonal) and +0.0 in the padding rows n .. ldX-1, which the launcher clears and no kernel
 * writes afterwards. */
int admm_op_trtri(const double* L, int64_t n, int64_t ldL, double* X, int64_t ldX);
/* y = L*(L'*x) for the lower factor L (above the diagonal ignored): the right-hand side of the setup probe that picks
 * the x-solve form, whose exact solution is x */
int admm_op_llt_apply(const double* L, int64_t n, int64_t ldL, const double* x, double* y);
/* The kernels of the spectral x-update of 2-D total variation on host images (H x W, column-major, ld = H on both
 * sides), through the launchers and tables the loop uses.  H must be a length the column transform supports (8 .. 8192
 * a power of two, or any other 8 .. 4096), W >= 1, rho finite and > 0; everything else is ADMM_E_INVALID before any
 * launch.  The device image lies between guard columns: a kernel that writes outside it gives ADMM_E_NUMERIC.
 *   dct_cols : out = the unnormalised DCT-II of every column of img (inverse = 0), or the inverse with its 1/H
 *   tv2d_rows: out = inv((1 + rho*lamH[i]) I + rho*L_W) along every row i of src (a column-transformed image) by the
 *              form ADMM_TV2D_ROWS_* (AUTO: admm_tv2d_row_stage).  A forced form outside its own precondition --
 *              GREEN: truncation < W; COOP: truncation <= 64 and W >= 384; DCT: W a power of two in 8 .. 8192 and even
 *              H -- is ADMM_E_INVALID
 *   tv2d_xsolve: x = inv(I + rho*D'D) b: forward columns, that row stage, inverse columns, as one x-update does */
int admm_op_dct_cols(const double* img, int64_t H, int64_t W, int32_t inverse, double* out);
int admm_op_tv2d_rows(const double* src, int64_t H, int64_t W, double rho, int32_t form, double* out);
int admm_op_tv2d_xsolve(const double* b, int64_t H, int64_t W, double rho, int32_t form, double* x);
/* ONE consensus-lasso iteration tail (getProxOps.m:1281-1343: the slice sums, the means, z by the soft threshold
 * lambda/(rho*Ntot), u_k += x_k - z, the next right-hand sides y_k = rho*(z - u_k) + D_k's_k, the residual sums) on
 * host arrays, through the launchers and in the launch sequence of the loop.  form selects the sequence:
 *   0: cons_sum + cons_update                 x_k given in X
 *   1: cons_gather_sum + cons_update          x_k assembled from the partial rows, X is output only
 *   2: cons_gather_update (one launch)        the same; K <= 16, remote == NULL and with_q == 0, else ADMM_E_INVALID
 * rows (forms 1, 2; ignored by form 0): the logical partial rows [K][P][n], P = ceil(n / 128) + 1, x_k[i] = sum_p
 * rows[k][p][i].  They reach the device where the lower-triangle x-solve leaves them: row p of element i in row p of
 * the N-part when p <= i / 128 and in row p - 1 of the T-part otherwise, with the row and slice strides of the
 * engine's plan for order n; every other double of both buffers, padding columns included, is the all-ones NaN, so a
 * wrong source row reaches the output as NaN.
 * X, U, Dts, Y: [K][n] (slice k at + k*n); U, xave and ubar (n each) are read and updated in place; z and xaveprev
 * receive n values.  K local slices of Ntot >= K in all.  remote (optional, [2][n]): the other ranks' sum of x_k and
 * of u_k, added to the sums on the host between the two launches as the all-reduce of a row-sharded run would.
 * with_q = 1 (forms 0, 1): the first launch also forms q = sum_k ||x_k - xave||^2 about the xave that came IN, folded
 * as the sharded run folds it, and *q receives it.
 * sums: [2][n], sum_k x_k and sum_k u_k as the update kernel read them (remote included); form 2 never stores them and
 * leaves the buffer untouched.  slots[5]: the totals of S_R2 = sum_k ||x_k - xave||^2, S_AX2 = ||xave||^2, S_G2 =
 * ||xave - xaveprev||^2, S_U2 = ||ubar||^2 and S_DU2 = ||ubar - ubar_in||^2 over the workgroup partials the finalize
 * step reads.  The device X, U and Y carry the padding column of an odd n and one guard row behind the last slice, and
 * the partial-row buffers one guard row in front: a kernel that stores past the n elements of a slice gives
 * ADMM_E_NUMERIC.  Bad arguments are ADMM_E_INVALID before any device call. */
int admm_op_consensus_tail(int32_t form, int64_t n, int32_t K, int32_t Ntot, double rho, double lambda,
                           const double* rows, double* X, double* U, const double* Dts, double* xave, double* ubar,
                           const double* remote, int32_t with_q, double* Y, double* sums, double* z, double* xaveprev,
                           double* slots, double* q);

/* ---- multi-GPU (one process per GPU; rows of D sharded; RCCL over xGMI) --------
 * unique id is created on rank 0 and handed to the other ranks by the host
 * (torch.distributed / MPI / a file).  errorcheck.m:216-267 defines the row partition.
 */
#define ADMM_COMM_ID_BYTES 128
/* transports: RCCL over xGMI (collectives enqueued on the engine's stream), or a host-staged
 * all-reduce through POSIX shared memory (any number of ranks may then share one GPU; used for
 * single-GPU testing of the sharded engines and as a fallback) */
enum { ADMM_COMM_RCCL = 0, ADMM_COMM_SHM = 1,
       /* one-shot peer-to-peer all-reduce for the loop's small payloads (80-240 KB: latency, not bandwidth): every rank
        * stores its contribution straight into a slot of every peer's device buffer (xGMI is a full point-to-point
        * mesh: one hop, where a ring makes 2(N-1)), raises a flag there, waits for the N flags in its own buffer and
        * sums the N slots in rank order -- ONE kernel per rank, on the engine's stream, no host synchronisation, bitwise
        * the same result on every rank.  Ranks of one node (processes or threads): buffers are shared through HIP IPC
        * handles exchanged over the shared-memory rendezvous.  Never run on real links in this repository's records. */
       ADMM_COMM_P2P = 2 };
int admm_comm_unique_id(char id[ADMM_COMM_ID_BYTES]);
int admm_comm_init(const char id[ADMM_COMM_ID_BYTES], int rank, int nranks, int device, int transport,
                   admm_comm** out);
int admm_comm_info(admm_comm* comm, int* rank, int* nranks, int* transport);
int admm_comm_allreduce_sum(admm_comm* comm, double* host_buf, size_t count); /* host convenience/test */
/* average wall time (microseconds) of one in-place sum all-reduce of `count` doubles on this communicator: `reps` of
 * them enqueued back to back on a stream of their own after 3 warm-up rounds (collective: every rank calls it with the
 * same arguments).  What the engine's per-iteration exchange costs on the links this process group really has. */
int admm_comm_measure_latency(admm_comm* comm, size_t count, int reps, double* microseconds);
void admm_comm_destroy(admm_comm* comm);

/* One host process driving several GPUs (a MATLAB session with a MEX gateway; the reference opens its pool from one
 * session: admm.m:347-356, unwrappedadmm.m:47).  The engines are the per-rank engines above; these calls run every
 * rank's create / run on a host thread of its own (each blocks inside its collectives) and join them.
 *   comm_init_all : nranks communicators of one group inside this process, comms[r] on devices[r] (the same device
 *                   may appear more than once with ADMM_COMM_SHM)
 *   create_all    : descs[r].comm = comms[r], descs[r].device = devices[r], each with its rows (slicemaker order)
 *   run_all       : opts[0] for every rank (opts_per_rank = 0) or opts[r]; summaries may be NULL
 * On failure the message of the first failing rank is the caller's admm_last_error(). */
int admm_comm_init_all(int nranks, const int* devices, int transport, admm_comm** comms);
int admm_engine_create_all(int nranks, const admm_problem_desc* descs, admm_engine** engines);
int admm_engine_run_all(int nranks, admm_engine* const* engines, const admm_options* opts, int opts_per_rank,
                        admm_run_summary* summaries);

/* ---- linear SVM, all one-vs-rest classes in one pass over D (additive to ABI 5) ---------------------------------
 * examples/mnistsvm.m:88-102 trains one linearsvm per digit and loss on the SAME matrix D: calls that differ only in
 * the label vector and the loss.  xminLinearSVM is Dplus*(z-u) (getProxOps.m:1062-1068) and does not contain ell; the
 * labels enter the element-wise z-prox (getProxOps.m:1084-1103) and the objective (linearsvm.m:231-237) alone.  So K
 * classes are K independent plain-ADMM runs (unwrappedadmm.m:76-92: A = D, B = -1, c = 0, stopcond = 'both',
 * nodualerror = 1) that share D, its pseudo-inverse and every byte an iteration reads: this object runs them side by
 * side, one read of D per iteration for a chunk of classes (csrc/svm_ovr.hip).  A class that has met its stop
 * condition is frozen: its result is that of an independent run with that many steps.
 * Not available here, each refused with ADMM_E_UNSUPPORTED (use one ADMM_PROB_LINEARSVM engine per class instead):
 * n > 448, fast ADMM, relaxation, convtest, a communicator; there are no callback or hook entry points.
 * Vector histories (xvals, zvals, uvals) are not recorded. */
typedef struct admm_svm_ovr admm_svm_ovr; /* opaque */
#define ADMM_SVM_OVR_MAX_N 448

/* what mnistsvm.m:88-102 passes to its linearsvm calls, for all of them at once */
typedef struct admm_svm_ovr_desc {
  int32_t struct_size;   /* sizeof(admm_svm_ovr_desc) */
  int32_t K;             /* number of classes (columns of ELL), >= 1 */
  int64_t m, n;          /* D is m x n */
  const double* D;       /* m x n, column-major */
  int64_t ldD;           /* leading dimension of D (0 = m) */
  const double* ELL;     /* m x K, column-major, +-1: column c is the ell of class c (mnistsvm.m:136-142) */
  const int32_t* loss;   /* K values ADMM_LOSS_* (linearsvm.m:154-158, 231-237); NULL = hinge for every class */
  double C;              /* regularisation (linearsvm.m:270-274) */
  int32_t mem;           /* ADMM_MEM_* of D, ELL, Dplus */
  int32_t device;        /* HIP device ordinal */
  const double* Dplus;   /* optional pinv(D), n x m column-major, ld = n (linearsvm.m:185-186): the x-update's
                            n x n map is then Dplus*Dplus' = (D'D)^+; NULL: built from D'D as admm_engine_create does */
  admm_comm* comm;       /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_svm_ovr_desc;

/* the options the K runs share (admm.m:51-76); fields of admm_options that have no meaning here are absent, and the
 * ones that select a variant this object does not run are refused */
typedef struct admm_svm_ovr_options {
  int32_t struct_size;   /* sizeof(admm_svm_ovr_options) */
  int32_t maxiters;      /* default 1000 (unwrappedadmm.m:90 forces it) */
  double rho;            /* default 1.0 */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double Hnormtol;       /* default 1e-6 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations enqueued between host polls of "every class has stopped" (0 = auto) */
  int32_t reserved0;
  const double* x0;      /* n x K host matrix (NULL = zeros; admm.m:252-254) */
  const double* z0;      /* m x K */
  const double* u0;      /* m x K */
} admm_svm_ovr_options;

typedef struct admm_svm_ovr_summary {  /* one per class */
  int32_t steps;          /* results.steps of that class (admm.m:746) */
  int32_t stopped_early;  /* 1 if a stop condition fired before maxiters (admm.m:710-722) */
  double objopt;          /* results.objopt (admm.m:752-754), NaN if not evaluated */
} admm_svm_ovr_summary;

/* fields of admm_svm_ovr_fetch */
enum {
  ADMM_OVR_F_XOPT = 1,      /* n x K */
  ADMM_OVR_F_ZOPT = 2,      /* m x K */
  ADMM_OVR_F_UOPT = 3,      /* m x K */
  /* scalar histories (admm.m:621-658, 305-306, 603-605): S x K column-major with S = the largest steps of any
   * class, NaN past a class's own last step */
  ADMM_OVR_F_PNORM = 4, ADMM_OVR_F_PERR = 5, ADMM_OVR_F_HNORMSQ = 6, ADMM_OVR_F_OBJEVALS = 7
};

void admm_svm_ovr_desc_default(admm_svm_ovr_desc* desc);
void admm_svm_ovr_options_default(admm_svm_ovr_options* opts);
/* the one-time setup of linearsvm.m:183-217 for all classes: uploads D and ELL, builds (D'D)^-1 or (D'D)^+ */
int admm_svm_ovr_create(const admm_svm_ovr_desc* desc, admm_svm_ovr** out);
/* the K loops of admm.m:496-743; summaries: K entries (may be NULL); runtime_s: the loop alone (admm.m:315 .. 756;
 * may be NULL).  May be called again on the same object: every run starts from its own x0 / z0 / u0 */
int admm_svm_ovr_run(admm_svm_ovr* obj, const admm_svm_ovr_options* opts, admm_svm_ovr_summary* summaries,
                     double* runtime_s);
int admm_svm_ovr_fetch(admm_svm_ovr* obj, int field, double* dst, size_t cap, size_t* written);
/* The costs of the K classes (admm_engine_set_svm_cost states the arithmetic): weights = m HOST values
 * shared by all classes, or NULL (every weight 1); class_cost = K x 2 HOST values, row c = (cost_pos, cost_neg) of class
 * c, or NULL (every cost 1).  Both are copied at the call and hold for every later run; (NULL, NULL) restores the
 * defaults, with which the pass launches the kernels it always did.  A chunk of classes takes the cost form of the pass
 * when there are weights or one of its classes has a cost != 1 or ADMM_LOSS_SQHINGE; no m x K array is built.
 * ADMM_E_INVALID: a negative or non-finite weight or cost -- a refused call changes nothing. */
int admm_svm_ovr_set_cost(admm_svm_ovr* obj, const double* weights, const double* class_cost);
/* classes one pass over D serves (K beyond it: ceil(K / chunk) passes per iteration) */
int admm_svm_ovr_chunk(void);
void admm_svm_ovr_destroy(admm_svm_ovr* obj);

/* ---- quantile / LAD / Huber regression, K fits in one pass over D (additive to ABI 5) ---------------
 * A caller of lad.m / huberfit.m wants a set of quantiles of one design matrix, a Huber fit at several thresholds, or
 * one loss against several response columns.  The x-update of the A = D iteration, (D'D)^-1 D'(s + z - u)
 * (getProxOps.m:1511-1515), contains neither the loss nor its parameters; those enter the element-wise z-prox (the loss
 * family of admm_engine_set_loss) and the objective alone.  So K fits are K independent plain-ADMM runs
 * (admm.m:496-743: A = D, B = -1, c = s_k, stopcond = 'standard', nodualerror = 1) that share D, the map (D'D)^-1 and
 * every byte an iteration reads: this object runs them side by side, one read of D per iteration for a chunk of fits
 * (csrc/reg_multi.hip).  A fit that has met its stop condition is frozen: its result is that of an independent run with
 * that many steps.
 * The dual residual is NOT evaluated: it would need two more transposed products with D per fit and iteration -- the
 * same restriction as the engine's one-pass form.  A fit stops when pnorm < perr, and therefore equals
 * lad(D, s, {..., 'nodualerror': 1}) / huberfit(D, s, {..., 'nodualerror': 1}), not the default lad / huberfit.
 * Not available here, each refused with ADMM_E_UNSUPPORTED (use one ADMM_PROB_LAD / ADMM_PROB_HUBERFIT engine per fit
 * instead): n > 448, m < n, fast ADMM, relaxation, convtest, a communicator; there is no H-norm stop, and there are no
 * callback or hook entry points.  Vector histories (xvals, zvals, uvals) are not recorded. */
typedef struct admm_reg_multi admm_reg_multi; /* opaque */
#define ADMM_REG_MULTI_MAX_N 448

typedef struct admm_reg_multi_desc {
  int32_t struct_size;   /* sizeof(admm_reg_multi_desc) */
  int32_t K;             /* number of fits, >= 1 */
  int64_t m, n;          /* D is m x n, m >= n */
  const double* D;       /* m x n, column-major */
  int64_t ldD;           /* leading dimension of D (0 = m) */
  const double* S;       /* m x ns, column-major: the response of every fit (ns = 1) or one column per fit (ns = K) */
  int32_t ns;            /* 1 or K */
  int32_t mem;           /* ADMM_MEM_* of D and S */
  int32_t device;        /* HIP device ordinal */
  int32_t reserved0;
  const int32_t* kind;   /* K values: 0 = the LAD engine's phi, 1 = the Huber engine's (admm_engine_set_loss); NULL = all 0 */
  const double* a;       /* K slopes of the positive side (NULL = 1); the tau-quantile: a = tau, b = 1 - tau */
  const double* b;       /* K slopes of the negative side (NULL = 1) */
  const double* epsilon; /* K dead zones, LAD fits (NULL = 0) */
  const double* delta;   /* K thresholds, Huber fits (NULL = 1) */
  admm_comm* comm;       /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_reg_multi_desc;

/* the options the K runs share (admm.m:51-76); the ones that select a variant this object does not run are refused */
typedef struct admm_reg_multi_options {
  int32_t struct_size;   /* sizeof(admm_reg_multi_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0 */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations enqueued between host polls of "every fit has stopped" (0 = auto: 8; 64 with
                            domaxiters) */
  int32_t reserved0;
  const double* x0;      /* n x K host matrix (NULL = zeros; admm.m:252-254) */
  const double* z0;      /* m x K */
  const double* u0;      /* m x K */
} admm_reg_multi_options;

typedef struct admm_reg_multi_summary {  /* one per fit */
  int32_t steps;          /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;  /* 1 if pnorm < perr fired before maxiters (admm.m:710-713) */
  double objopt;          /* results.objopt = sum_i w_i*phi_k(z_i) (lad.m:148 / huberfit.m:180 with the family inside), NaN
                             if not evaluated */
} admm_reg_multi_summary;

/* fields of admm_reg_multi_fetch */
enum {
  ADMM_REGM_F_XOPT = 1,      /* n x K */
  ADMM_REGM_F_ZOPT = 2,      /* m x K */
  ADMM_REGM_F_UOPT = 3,      /* m x K */
  /* scalar histories (admm.m:621-658, 603-605): S x K column-major with S = the largest steps of any fit, NaN past a
   * fit's own last step */
  ADMM_REGM_F_PNORM = 4, ADMM_REGM_F_PERR = 5, ADMM_REGM_F_OBJEVALS = 6
};

void admm_reg_multi_desc_default(admm_reg_multi_desc* desc);
void admm_reg_multi_options_default(admm_reg_multi_options* opts);
/* the one-time setup of lad.m:134 for all fits: uploads D and S, builds (D'D)^-1 or keeps the Cholesky factor as
 * admm_engine_create's probe decides.  ADMM_E_INVALID, naming the fit: a kind other than 0 / 1; a slope <= 0;
 * epsilon < 0, or != 0 on a Huber fit; delta <= 0, or != 1 on a LAD fit; a non-finite value.  ADMM_E_NUMERIC: D'D is
 * numerically singular (lad.m:134 calls chol: there are no pinv semantics here). */
int admm_reg_multi_create(const admm_reg_multi_desc* desc, admm_reg_multi** out);
/* the K loops of admm.m:496-743; summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be
 * called again on the same object: every run starts from its own x0 / z0 / u0 */
int admm_reg_multi_run(admm_reg_multi* obj, const admm_reg_multi_options* opts, admm_reg_multi_summary* summaries,
                       double* runtime_s);
int admm_reg_multi_fetch(admm_reg_multi* obj, int field, double* dst, size_t cap, size_t* written);
/* weights = m HOST values w_i >= 0 shared by all fits, copied at the call and held for every later run; NULL restores 1.
 * ADMM_E_INVALID: a negative or non-finite weight -- a refused call changes nothing. */
int admm_reg_multi_set_weights(admm_reg_multi* obj, const double* weights);
/* kernel launches of the last run's iterations (the start's D'(s + z0 - u0) not counted): counts[0] iterations
 * enqueued, [1] x-solve launches, [2] passes over D, [3] sum / finalize launches, [4] 1 where the x-solve is the one
 * launch of the explicit map (0: two triangular solves per fit and one copy) */
int admm_reg_multi_launches(admm_reg_multi* obj, int64_t counts[5]);
/* fits one pass over D serves (K beyond it: ceil(K / chunk) passes per iteration) */
int admm_reg_multi_chunk(void);
void admm_reg_multi_destroy(admm_reg_multi* obj);

/* ---- linear SVM on a sparse design matrix, all one-vs-rest classes over one sparse product (additive to ABI 5;
 * DESIGN.md q37).  The K runs are those of admm_svm_ovr (plain ADMM, A = D, B = -1, c = 0, stopcond = 'both',
 * nodualerror = 1, the losses and costs of admm_svm_ovr_set_cost) with D an admm_sparse_desc and the x-update
 * x_c = D^+(z_c - u_c) computed as conjugate gradients on D'D x = D'(z_c - u_c): no shift, nothing factored, nothing
 * n x n stored, so there is no limit on n.  The first x-update of a run starts CG from 0 (x0 is never read, as in the
 * reference's x-update) and every later one from the previous x: every iterate stays in range(D'), the limit is the
 * pseudo-inverse solution, and a column of D without nonzeros keeps x = 0.0 exactly.  The K solves run in lock-step:
 * each inner iteration is D*P and D'*(D*P) for all classes of a chunk over ONE read of the matrix (csrc/spmm.hip); a
 * class whose solve has converged, or whose run has stopped, is masked.  Per class ||r|| <= cg_tol*||y|| ends a solve; an
 * x-update that ends on cg_maxit above cg_tol is counted per class.  A zero right-hand side gives x = 0, and p.q = 0 ends
 * the class's solve, both without a division.
 * ADMM_E_INVALID (before the device is touched): whatever admm_engine_create_sparse refuses in D, D not in host arrays,
 * a label that is not +-1, K < 1, an unknown loss, C < 0.  ADMM_E_UNSUPPORTED: a communicator; at run: fast ADMM,
 * relaxation, convtest.  Vector histories are not recorded and the dual residual is not evaluated. */
typedef struct admm_sparse_svm admm_sparse_svm; /* opaque */

typedef struct admm_sparse_svm_desc {
  int32_t struct_size;        /* sizeof(admm_sparse_svm_desc) */
  int32_t K;                  /* number of classes (columns of ELL), >= 1 */
  const admm_sparse_desc* D;  /* rows x cols, ADMM_MEM_HOST; copied at create */
  const double* ELL;          /* rows x K HOST values, column-major, +-1: column c is the ell of class c */
  const int32_t* loss;        /* K values ADMM_LOSS_*; NULL = hinge for every class */
  double C;                   /* regularisation (linearsvm.m:270-274) */
  int32_t device;             /* HIP device ordinal */
  int32_t reserved0;
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_sparse_svm_desc;

typedef struct admm_sparse_svm_options {
  int32_t struct_size;   /* sizeof(admm_sparse_svm_options) */
  int32_t maxiters;      /* default 1000 (unwrappedadmm.m:90 forces it) */
  double rho;            /* default 1.0 */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double Hnormtol;       /* default 1e-6 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every class has stopped" (0 = auto) */
  int32_t cg_maxit;      /* cap on the inner iterations of one x-update; default 200, <= 0 = default */
  double cg_tol;         /* relative residual of the x-update; default 1e-12, <= 0 = default */
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* rows x K host matrix (NULL = zeros) */
  const double* u0;      /* rows x K */
} admm_sparse_svm_options;

typedef struct admm_sparse_svm_summary {  /* one per class */
  int32_t steps;              /* results.steps of that class (admm.m:746) */
  int32_t stopped_early;      /* 1 if a stop condition fired before maxiters (admm.m:710-722) */
  double objopt;              /* results.objopt (admm.m:752-754), NaN if not evaluated */
  int64_t cg_iters_total;     /* inner iterations of the class over the run */
  int64_t cg_capped_updates;  /* x-updates of the class that ended with the residual still above cg_tol */
} admm_sparse_svm_summary;

void admm_sparse_svm_desc_default(admm_sparse_svm_desc* desc);
void admm_sparse_svm_options_default(admm_sparse_svm_options* opts);
int admm_sparse_svm_create(const admm_sparse_svm_desc* desc, admm_sparse_svm** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object:
 * every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_sparse_svm_run(admm_sparse_svm* obj, const admm_sparse_svm_options* opts, admm_sparse_svm_summary* summaries,
                        double* runtime_s);
/* field: ADMM_OVR_F_*, the shapes of admm_svm_ovr_fetch */
int admm_sparse_svm_fetch(admm_sparse_svm* obj, int field, double* dst, size_t cap, size_t* written);
/* the arguments, the arithmetic and the refusals of admm_svm_ovr_set_cost */
int admm_sparse_svm_set_cost(admm_sparse_svm* obj, const double* weights, const double* class_cost);
/* classes one sparse product serves (K beyond it: ceil(K / chunk) chunks per launch) */
int admm_sparse_svm_chunk(void);
void admm_sparse_svm_destroy(admm_sparse_svm* obj);

/* ---- quantile / LAD / Huber regression on a sparse design matrix, K fits over one sparse product (additive to ABI 5;
 * DESIGN.md q38).  The K runs are those of admm_reg_multi (plain ADMM, A = D, B = -1, c = s_k, stopcond = 'standard', the
 * loss family of admm_engine_set_loss per fit, m shared weights) with D an admm_sparse_desc and the x-update
 * x_k = (D'D)^-1 D'(s_k + z_k - u_k) computed as admm_sparse_svm computes its own: lock-step conjugate gradients on
 * D'D x = D'(s_k + z_k - u_k), no shift, nothing factored, nothing n x n stored, so there is no limit on n and m < n
 * runs.  The first x-update of a run starts CG from 0 (x0 is never read) and every later one from the previous x: with
 * full column rank that is the reference's solution; with an empty or duplicated column it is the minimum-norm one
 * (x = 0.0 exactly on an empty column), where lad.m:134 fails in chol.
 * nodualerror = 0 evaluates the dual residual as well -- dnorm = rho*||D'(z - zprev)||, derr = sqrt(m)*abstol +
 * reltol*||rho*D'u|| (admm.m:624, 652-654), two more transposed products per iteration -- and a fit then stops on
 * pnorm < perr and dnorm < derr, as the default lad / huberfit do.
 * ADMM_E_INVALID (before the device is touched): whatever admm_engine_create_sparse refuses in D, D not in host arrays,
 * K < 1, ns not 1 or K, and per fit (named in the message) whatever admm_engine_set_loss refuses.  ADMM_E_UNSUPPORTED: a
 * communicator; at run: fast ADMM, relaxation, convtest.  Vector histories are not recorded. */
typedef struct admm_sparse_reg admm_sparse_reg; /* opaque */

typedef struct admm_sparse_reg_desc {
  int32_t struct_size;        /* sizeof(admm_sparse_reg_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  const admm_sparse_desc* D;  /* rows x cols, ADMM_MEM_HOST; copied at create */
  const double* S;            /* rows x ns HOST values, column-major: one response for every fit, or one column per fit */
  int32_t ns;                 /* 1 or K */
  int32_t device;             /* HIP device ordinal */
  const int32_t* kind;        /* K values: 0 = the LAD engine's phi, 1 = the Huber engine's; NULL = all 0 */
  const double* a;            /* K slopes of the positive side (NULL = 1); the tau-quantile: a = tau, b = 1 - tau */
  const double* b;            /* K slopes of the negative side (NULL = 1) */
  const double* epsilon;      /* K dead zones, LAD fits (NULL = 0) */
  const double* delta;        /* K thresholds, Huber fits (NULL = 1) */
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_sparse_reg_desc;

typedef struct admm_sparse_reg_options {
  int32_t struct_size;   /* sizeof(admm_sparse_reg_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0 */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every fit has stopped" (0 = auto: 8; 64 with domaxiters) */
  int32_t cg_maxit;      /* cap on the inner iterations of one x-update; default 200, <= 0 = default */
  double cg_tol;         /* relative residual of the x-update; default 1e-12, <= 0 = default */
  int32_t nodualerror;   /* default 1: stop on pnorm < perr alone, as admm_reg_multi; 0: the reference's default rule */
  int32_t reserved0;
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* rows x K host matrix (NULL = zeros) */
  const double* u0;      /* rows x K */
} admm_sparse_reg_options;

typedef struct admm_sparse_reg_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* sum_i w_i*phi_k(z_i) (lad.m:148 / huberfit.m:180 with the family inside), NaN if not evaluated */
  int64_t cg_iters_total;     /* inner iterations of the fit over the run */
  int64_t cg_capped_updates;  /* x-updates of the fit that ended with the residual still above cg_tol */
} admm_sparse_reg_summary;

/* fields of admm_sparse_reg_fetch: 1 .. 6 are admm_reg_multi_fetch's */
enum {
  ADMM_SRG_F_XOPT = 1,      /* cols x K */
  ADMM_SRG_F_ZOPT = 2,      /* rows x K */
  ADMM_SRG_F_UOPT = 3,      /* rows x K */
  /* scalar histories: S x K column-major with S = the largest steps of any fit, NaN past a fit's own last step; DNORM
   * and DERR after a run with nodualerror = 0 only */
  ADMM_SRG_F_PNORM = 4, ADMM_SRG_F_PERR = 5, ADMM_SRG_F_OBJEVALS = 6, ADMM_SRG_F_DNORM = 7, ADMM_SRG_F_DERR = 8
};

void admm_sparse_reg_desc_default(admm_sparse_reg_desc* desc);
void admm_sparse_reg_options_default(admm_sparse_reg_options* opts);
int admm_sparse_reg_create(const admm_sparse_reg_desc* desc, admm_sparse_reg** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object:
 * every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_sparse_reg_run(admm_sparse_reg* obj, const admm_sparse_reg_options* opts, admm_sparse_reg_summary* summaries,
                        double* runtime_s);
int admm_sparse_reg_fetch(admm_sparse_reg* obj, int field, double* dst, size_t cap, size_t* written);
/* weights = rows HOST values w_i >= 0 shared by all fits, copied at the call and held for every later run; NULL restores
 * 1.  ADMM_E_INVALID: a negative or non-finite weight -- a refused call changes nothing. */
int admm_sparse_reg_set_weights(admm_sparse_reg* obj, const double* weights);
/* fits one sparse product serves (K beyond it: ceil(K / chunk) chunks per launch) */
int admm_sparse_reg_chunk(void);
void admm_sparse_reg_destroy(admm_sparse_reg* obj);

/* ---- the lasso on a sparse design matrix, K fits over one sparse product (additive to ABI 5): a
 * regularisation path, a cross-validation grid or several response columns in one run.  The K runs are plain ADMM as
 * lasso.m:227-239 poses it (A = 1, B = -1, c = 0, sizes cols, stopcond = 'standard'); they share D, rho and cols l1
 * weights w_i >= 0 and differ in (lambda_k, mu_k, nonneg_k) and, with ns = K, in their column of S:
 *   minimise 1/2*||D x - s_k||^2 + lambda_k*sum_i w_i*|z_i| + mu_k/2*||z||^2 + [z >= 0 when nonneg_k]  s.t. x = z
 * (the penalty family of admm_engine_set_penalty without groups).  The x-update (D'D + rho*I) x = D's_k + rho*(z - u)
 * (lasso.m:28-30) is the lock-step conjugate gradients of admm_sparse_svm / admm_sparse_reg with the shift rho: nothing
 * factored, nothing cols x cols stored.  The first x-update of a run starts CG from 0 (x0 is never read) and every later
 * one from the previous x.  A fit stops on pnorm = ||x - z|| < perr = sqrt(cols)*abstol + reltol*max(||x||, ||z||) and
 * dnorm = rho*||z - zprev|| < derr = sqrt(cols)*abstol + reltol*rho*||u|| (admm.m:621-654), the reference lasso's rule and
 * the default here (the dual residual costs no product); nodualerror = 1 stops on the primal residual alone.  The
 * objective (objevals = 1: one more sparse product per iteration) is 1/2*||D x - s_k||^2 + g_k(z).
 * ADMM_E_INVALID (before the device is touched): whatever admm_engine_create_sparse refuses in D, D not in host arrays,
 * K < 1, ns not 1 or K, per fit (named in the message) a negative or non-finite lambda or ridge, nonneg other than
 * 0 | 1, and a negative or non-finite weight (its index named).  ADMM_E_UNSUPPORTED: a communicator; at run: fast ADMM, relaxation, convtest.  Vector histories are not
 * recorded. */
typedef struct admm_sparse_lasso admm_sparse_lasso; /* opaque */

typedef struct admm_sparse_lasso_desc {
  int32_t struct_size;        /* sizeof(admm_sparse_lasso_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  const admm_sparse_desc* D;  /* rows x cols, ADMM_MEM_HOST; copied at create */
  const double* S;            /* rows x ns HOST values, column-major: one response for every fit, or one column per fit */
  int32_t ns;                 /* 1 or K */
  int32_t device;             /* HIP device ordinal */
  const double* lambda;       /* K values lambda_k >= 0 */
  const double* ridge;        /* K values mu_k >= 0 (NULL = 0) */
  const int32_t* nonneg;      /* K values 0 | 1 (NULL = 0) */
  const double* weights;      /* cols l1 weights w_i >= 0 shared by all fits (NULL = 1); admm_sparse_lasso_set_weights
                                 replaces them */
  admm_comm* comm;           /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_sparse_lasso_desc;

typedef struct admm_sparse_lasso_options {
  int32_t struct_size;   /* sizeof(admm_sparse_lasso_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0: the shift of every x-update */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every fit has stopped" (0 = auto: 8; 64 with domaxiters) */
  int32_t cg_maxit;      /* cap on the inner iterations of one x-update; default 200, <= 0 = default */
  double cg_tol;         /* relative residual of the x-update; default 1e-12, <= 0 = default */
  int32_t nodualerror;   /* default 0: the reference lasso's rule; 1: stop on pnorm < perr alone */
  int32_t reserved0;
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* cols x K host matrix (NULL = zeros) */
  const double* u0;      /* cols x K */
} admm_sparse_lasso_options;

typedef struct admm_sparse_lasso_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* the objective at the fit's last step, NaN if not evaluated */
  int64_t cg_iters_total;     /* inner iterations of the fit over the run */
  int64_t cg_capped_updates;  /* x-updates of the fit that ended with the residual still above cg_tol */
} admm_sparse_lasso_summary;

/* fields of admm_sparse_lasso_fetch: the numbers of admm_sparse_reg_fetch */
enum {
  ADMM_SLM_F_XOPT = 1,      /* cols x K */
  ADMM_SLM_F_ZOPT = 2,      /* cols x K */
  ADMM_SLM_F_UOPT = 3,      /* cols x K */
  /* scalar histories: S x K column-major with S = the largest steps of any fit, NaN past a fit's own last step; DNORM
   * and DERR after a run with nodualerror = 0 only, OBJEVALS after a run with objevals = 1 only */
  ADMM_SLM_F_PNORM = 4, ADMM_SLM_F_PERR = 5, ADMM_SLM_F_OBJEVALS = 6, ADMM_SLM_F_DNORM = 7, ADMM_SLM_F_DERR = 8
};

void admm_sparse_lasso_desc_default(admm_sparse_lasso_desc* desc);
void admm_sparse_lasso_options_default(admm_sparse_lasso_options* opts);
int admm_sparse_lasso_create(const admm_sparse_lasso_desc* desc, admm_sparse_lasso** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object:
 * every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_sparse_lasso_run(admm_sparse_lasso* obj, const admm_sparse_lasso_options* opts,
                          admm_sparse_lasso_summary* summaries, double* runtime_s);
int admm_sparse_lasso_fetch(admm_sparse_lasso* obj, int field, double* dst, size_t cap, size_t* written);
/* weights = cols HOST values w_i >= 0 shared by all fits (the l1 weights), copied at the call and held for every later
 * run; NULL restores 1.  ADMM_E_INVALID: a negative or non-finite weight -- a refused call changes nothing. */
int admm_sparse_lasso_set_weights(admm_sparse_lasso* obj, const double* weights);
/* Groups for every later run (additive to ABI 5): G contiguous groups of sizes[g] >= 1 coefficients that
 * sum to cols, group weights omega_g >= 0 (NULL = 1) shared by all fits, and per fit the strength l1[k] >= 0 of the l1
 * term (K values, NULL = 0); all HOST arrays, copied at the call.  With groups in force lambda_k weighs the group term,
 *   g_k(z) = lambda_k*sum_g omega_g*||z_g||_2 + l1[k]*sum_i w_i*|z_i| + mu_k/2*||z||^2 + [z >= 0 when nonneg_k],
 * and the z-update is soft threshold (or positive part), block soft threshold, scale by rho/(rho + mu_k).  G = 0 or
 * sizes = NULL restores the ungrouped prox, where lambda_k weighs the l1 term.  ADMM_E_INVALID: a size below 1, sizes
 * that do not sum to cols, a negative or non-finite group weight (its index named) or l1[k] (the fit named);
 * ADMM_E_UNSUPPORTED: more than 65536 groups that the plan cannot pack (256 workgroups of at most 256 groups each).  A
 * refused call changes nothing. */
int admm_sparse_lasso_set_groups(admm_sparse_lasso* obj, int32_t G, const int64_t* sizes, const double* groupweights,
                                 const double* l1);
/* Observation weights and held-out folds for every later run (additive to ABI 5): the fit term of fit k
 * becomes 1/2*sum_i omega_ik*(d_i'x - s_ik)^2 with omega_ik = obsweights[i] * [fold[i] != heldout[k]] -- weighted least
 * squares under the same penalties, and K fits that each leave one fold of rows out, over one D.  obsweights: rows HOST
 * values >= 0 shared by all fits (NULL = 1); fold: rows fold ids in [0, nfolds) (NULL: no row is held out); heldout: K
 * values in [-1, nfolds), -1 (and NULL) = the fit holds nothing out.  All copied at the call.  The x-update solves
 * (D'Omega_k D + rho*I) x = D'(Omega_k s_k) + rho*(z - u) by the same lock-step CG, whose forward product stores
 * omega_ik*(D p)_i per fit (a held-out row stores +0.0 by a select); the z-update, the residuals and the stop rule are
 * unchanged, the objective (objevals = 1) carries the weighted fit term, and groups (admm_sparse_lasso_set_groups)
 * combine with it.  All three NULL restore the unweighted object, bit for bit.  ADMM_E_INVALID, the culprit named: a
 * negative or non-finite weight (its index), nfolds < 1 with fold given, a fold id outside [0, nfolds) (its row), a
 * heldout outside [-1, nfolds) (its fit), heldout without fold.  A refused call changes nothing. */
int admm_sparse_lasso_set_observations(admm_sparse_lasso* obj, const double* obsweights, int32_t nfolds,
                                       const int32_t* fold, const int32_t* heldout);
/* The held-out sums of the last run under observations, K doubles each, evaluated behind the loop at z (the sparse
 * iterate) for every fit: sse[k] = sum_i obsweights[i]*[fold[i] = heldout[k]]*(d_i'z_k - s_ik)^2 and weight[k] =
 * sum_i obsweights[i]*[fold[i] = heldout[k]] (both 0.0 for a fit that holds nothing out).  ADMM_E_INVALID before a run
 * or when the last run had no observations set. */
int admm_sparse_lasso_heldout(admm_sparse_lasso* obj, double* sse, double* weight);
/* fits one sparse product serves (K beyond it: ceil(K / chunk) chunks per launch) */
int admm_sparse_lasso_chunk(void);
void admm_sparse_lasso_destroy(admm_sparse_lasso* obj);

/* ---- the lasso on a DENSE design matrix, K fits over one cached inverse (additive to ABI 5): the family,
 * the arithmetic, the stop rule and the histories of admm_sparse_lasso above, fit for fit --
 *   minimise 1/2*||D x - s_k||^2 + lambda_k*sum_i w_i*|z_i| + mu_k/2*||z||^2 + [z >= 0 when nonneg_k]  s.t. x = z
 * -- with the x-update x = inv(D'D + rho*I) (D's_k + rho*(z - u)) (lasso.m:28-30, getProxOps.m:1195-1200) applied from
 * the cached factor of an ordinary ADMM_PROB_LASSO engine that the object creates and never runs.  Where that engine
 * holds the explicit inverse, every iteration reads its fp64 tile-packed lower triangle ONCE per chunk of
 * admm_lasso_multi_chunk() fits (csrc/symm.hip), whatever K is; where create's accuracy probe kept the triangular
 * solves, the x-update is K pairs of them.  The inverse depends on D and rho alone, so rho belongs to the desc and
 * options.rho must repeat it.  The objective (objevals = 1: one dense product D X per chunk and iteration) is
 * 1/2*||D x - s_k||^2 + g_k(z).  x0 is accepted and never read: the first x-update defines x.
 * ADMM_E_INVALID (before the device is touched): K < 1, no D / S / lambda, ns not 1 or K, per fit (named in the message)
 * a negative or non-finite lambda or ridge, nonneg other than 0 | 1, a negative or non-finite weight (its index named), a
 * rho that is not finite and > 0; at run: options.rho other than desc.rho.  ADMM_E_UNSUPPORTED: a communicator, an xsolve
 * other than AUTO / INVERSE / TRSV, m < n (the fat lasso's Woodbury form needs two dense multi-products per iteration
 * and stays with one engine per fit); at run: fast ADMM, relaxation, convtest.  Vector histories are not recorded. */
typedef struct admm_lasso_multi admm_lasso_multi; /* opaque */

typedef struct admm_lasso_multi_desc {
  int32_t struct_size;        /* sizeof(admm_lasso_multi_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  int64_t m, n;               /* D is m x n, m >= n */
  const double* D;            /* HOST, column-major; copied at create */
  int64_t ldD;                /* >= m */
  const double* S;            /* m x ns HOST values, column-major: one response for every fit, or one column per fit */
  int32_t ns;                 /* 1 or K */
  int32_t device;             /* HIP device ordinal */
  double rho;                 /* default 1.0: the rho the factor is built for, and the rho of every run */
  int32_t xsolve;             /* ADMM_XSOLVE_AUTO (default: the engine's probe decides), _INVERSE or _TRSV */
  int32_t reserved0;
  const double* lambda;       /* K values lambda_k >= 0 */
  const double* ridge;        /* K values mu_k >= 0 (NULL = 0) */
  const int32_t* nonneg;      /* K values 0 | 1 (NULL = 0) */
  const double* weights;      /* n l1 weights w_i >= 0 shared by all fits (NULL = 1); admm_lasso_multi_set_weights
                                 replaces them */
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_lasso_multi_desc;

typedef struct admm_lasso_multi_options {
  int32_t struct_size;   /* sizeof(admm_lasso_multi_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0; must equal desc.rho */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every fit has stopped" (0 = auto: 8; 64 with domaxiters) */
  int32_t nodualerror;   /* default 0: the reference lasso's rule; 1: stop on pnorm < perr alone */
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* n x K host matrix (NULL = zeros) */
  const double* u0;      /* n x K */
} admm_lasso_multi_options;

typedef struct admm_lasso_multi_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* the objective at the fit's last step, NaN if not evaluated */
  int32_t xsolve;             /* ADMM_XSOLVE_INVERSE (the packed product) or ADMM_XSOLVE_TRSV, the same for every fit */
  int32_t reserved0;
} admm_lasso_multi_summary;

/* fields of admm_lasso_multi_fetch: the numbers of admm_sparse_lasso_fetch */
enum {
  ADMM_LM_F_XOPT = 1,      /* n x K */
  ADMM_LM_F_ZOPT = 2,      /* n x K */
  ADMM_LM_F_UOPT = 3,      /* n x K */
  /* scalar histories: S x K column-major with S = the largest steps of any fit, NaN past a fit's own last step; DNORM
   * and DERR after a run with nodualerror = 0 only, OBJEVALS after a run with objevals = 1 only */
  ADMM_LM_F_PNORM = 4, ADMM_LM_F_PERR = 5, ADMM_LM_F_OBJEVALS = 6, ADMM_LM_F_DNORM = 7, ADMM_LM_F_DERR = 8
};

void admm_lasso_multi_desc_default(admm_lasso_multi_desc* desc);
void admm_lasso_multi_options_default(admm_lasso_multi_options* opts);
int admm_lasso_multi_create(const admm_lasso_multi_desc* desc, admm_lasso_multi** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object:
 * every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_lasso_multi_run(admm_lasso_multi* obj, const admm_lasso_multi_options* opts, admm_lasso_multi_summary* summaries,
                         double* runtime_s);
int admm_lasso_multi_fetch(admm_lasso_multi* obj, int field, double* dst, size_t cap, size_t* written);
/* weights = n HOST values w_i >= 0 shared by all fits (the l1 weights), copied at the call and held for every later
 * run; NULL restores 1.  ADMM_E_INVALID: a negative or non-finite weight -- a refused call changes nothing. */
int admm_lasso_multi_set_weights(admm_lasso_multi* obj, const double* weights);
/* admm_sparse_lasso_set_groups on the dense object: the same arguments, checks and z-update */
int admm_lasso_multi_set_groups(admm_lasso_multi* obj, int32_t G, const int64_t* sizes, const double* groupweights,
                                const double* l1);
/* fits one read of the inverse serves (K beyond it: ceil(K / chunk) chunks per launch) */
int admm_lasso_multi_chunk(void);
/* measurement: the x-update's packed product alone (tile pass + partial-row sum over the object's own buffers, every fit
 * running), event-timed: the median of reps calls in microseconds, the bytes of the stored triangle that one call reads
 * per chunk, and the fused multiply-adds one call issues.  Overwrites x; ADMM_E_UNSUPPORTED where the object applies
 * triangular solves. */
int admm_lasso_multi_product_time(admm_lasso_multi* obj, int32_t reps, double* us_per_call, int64_t* stored_bytes,
                                  int64_t* fma_count);
void admm_lasso_multi_destroy(admm_lasso_multi* obj);

/* ---- sparse linear classifiers on a DENSE design matrix, K fits over one D (additive to ABI 5): the
 * l1 / elastic-net penalty of the lasso family on the losses of the linear SVM,
 *   minimise C*sum_i c_ik*phi_k(ell_ik*(D x)_i) + lambda_k*sum_j w_j*|x_j| + mu_k/2*||x||^2  [x >= 0 when nonneg_k]
 * with phi_k hinge, squared hinge or logistic, c_ik = weights_i * (ell_ik > 0 ? cost_pos_k : cost_neg_k) and l1 weights
 * w_j >= 0 shared by all fits (w_j = 0: an unpenalised coefficient, e.g. an intercept column of ones).  Every fit is a
 * plain-ADMM run of admm.m with A = [D; I_n], B = -1, c = 0, z = [z1 (m); z2 (n)], stopcond 'standard':
 *   x = inv(D'D + I) (D'(z1 - u1) + (z2 - u2))      one factor and one explicit inverse for every fit and every rho
 *   z1 = prox of (C*c/rho)*phi at (D x + u1),  z2 = kappa*penalty_elem(x + u2, (lambda/rho)*w, nonneg)
 * Per iteration D is read twice per chunk of admm_l1class_chunk() fits (csrc/l1class.hip: a forward pass D X with the
 * z1 / u1 update in the launch, a transposed pass D'(z1 - u1)), whatever n is; the n x n product is csrc/symm.hip's, or
 * K pairs of triangular solves where create's accuracy probe kept them.  rho is a run option.  The dual residual
 * rho*||D'(z1 - z1prev) + (z2 - z2prev)|| and its tolerance widen the transposed pass to three vectors per fit; with
 * nodualerror = 1 they are not computed.  x0 is accepted and never read: the first x-update defines x.
 * ADMM_E_INVALID (before the device is touched): K < 1, no D / ELL / lambda, nell not 1 or K, a label that is not +-1,
 * per fit (named in the message) a loss other than ADMM_LOSS_HINGE / _SQHINGE / _LOGISTIC (the 0-1 loss is not convex
 * and has no lambda_max), a negative or non-finite lambda or ridge, nonneg other than 0 | 1; a negative or non-finite l1
 * weight (its index named); C that is not finite and > 0.  ADMM_E_UNSUPPORTED: a communicator, an xsolve other than
 * AUTO / INVERSE / TRSV; at run: fast ADMM, relaxation, convtest.  Vector histories are not recorded. */
typedef struct admm_l1class admm_l1class; /* opaque */

typedef struct admm_l1class_desc {
  int32_t struct_size;        /* sizeof(admm_l1class_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  int64_t m, n;               /* D is m x n, any shape */
  const double* D;            /* HOST, column-major; copied at create */
  int64_t ldD;                /* >= m */
  const double* ELL;          /* m x nell HOST labels +-1, column-major: one column for every fit, or one per fit */
  int32_t nell;               /* 1 or K */
  int32_t device;             /* HIP device ordinal */
  double C;                   /* default 1.0: the cost of the loss term, > 0 */
  int32_t xsolve;             /* ADMM_XSOLVE_AUTO (default: the engine's probe decides), _INVERSE or _TRSV */
  int32_t reserved0;
  const int32_t* loss;        /* K values ADMM_LOSS_HINGE | _SQHINGE | _LOGISTIC (NULL = logistic for every fit) */
  const double* lambda;       /* K values lambda_k >= 0 */
  const double* ridge;        /* K values mu_k >= 0 (NULL = 0) */
  const int32_t* nonneg;      /* K values 0 | 1 (NULL = 0) */
  const double* l1weights;    /* n l1 weights w_j >= 0 shared by all fits (NULL = 1); admm_l1class_set_l1weights
                                 replaces them */
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_l1class_desc;

typedef struct admm_l1class_options {
  int32_t struct_size;   /* sizeof(admm_l1class_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0; any value > 0: the factor does not depend on it */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every fit has stopped" (0 = auto: 8; 64 with domaxiters) */
  int32_t nodualerror;   /* default 0: admm.m's rule on both residuals; 1: stop on pnorm < perr alone */
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* (m + n) x K host matrix, z1 above z2 (NULL = zeros) */
  const double* u0;      /* (m + n) x K */
} admm_l1class_options;

typedef struct admm_l1class_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* the objective at the fit's last step, NaN if not evaluated */
  int32_t xsolve;             /* ADMM_XSOLVE_INVERSE (the packed product) or ADMM_XSOLVE_TRSV, the same for every fit */
  int32_t reserved0;
} admm_l1class_summary;

/* fields of admm_l1class_fetch */
enum {
  ADMM_L1C_F_XOPT = 1,      /* n x K */
  ADMM_L1C_F_ZOPT = 2,      /* (m + n) x K */
  ADMM_L1C_F_UOPT = 3,      /* (m + n) x K */
  /* scalar histories: S x K column-major with S = the largest steps of any fit, NaN past a fit's own last step; DNORM
   * and DERR after a run with nodualerror = 0 only, OBJEVALS after a run with objevals = 1 only */
  ADMM_L1C_F_PNORM = 4, ADMM_L1C_F_PERR = 5, ADMM_L1C_F_OBJEVALS = 6, ADMM_L1C_F_DNORM = 7, ADMM_L1C_F_DERR = 8
};

void admm_l1class_desc_default(admm_l1class_desc* desc);
void admm_l1class_options_default(admm_l1class_options* opts);
int admm_l1class_create(const admm_l1class_desc* desc, admm_l1class** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object,
 * with another rho as well: every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_l1class_run(admm_l1class* obj, const admm_l1class_options* opts, admm_l1class_summary* summaries,
                     double* runtime_s);
int admm_l1class_fetch(admm_l1class* obj, int field, double* dst, size_t cap, size_t* written);
/* admm_svm_ovr_set_cost on this object: weights = m HOST values >= 0 shared by all fits (NULL = 1), class_cost = K x 2
 * HOST values, row k = (cost_pos, cost_neg) of fit k (NULL = 1).  ADMM_E_INVALID: a negative or non-finite weight or
 * cost -- a refused call changes nothing. */
int admm_l1class_set_cost(admm_l1class* obj, const double* weights, const double* class_cost);
/* l1weights = n HOST values w_j >= 0 shared by all fits, copied at the call and held for every later run; NULL
 * restores 1.  ADMM_E_INVALID: a negative or non-finite weight -- a refused call changes nothing. */
int admm_l1class_set_l1weights(admm_l1class* obj, const double* l1weights);
/* Groups for every later run of an admm_l1class object (additive to ABI 5; the admm_l1class_* family
 * itself stays the eleven functions of q42, so this entry point carries the prefix admm_group_l1class_): admm_sparse_lasso_set_groups' arguments, checks and
 * messages on the classifier.  The penalty of fit k becomes lambda_k*sum_g omega_g*||x_g||_2 + l1[k]*sum_j w_j*|x_j| +
 * mu_k/2*||x||^2 (x >= 0 where nonneg_k): desc.lambda is the group strength, l1 (K HOST values >= 0, NULL = 0) the l1
 * strength; sizes = G HOST group sizes >= 1 that sum to n, groupweights = G HOST values omega_g >= 0 (NULL = 1; 0 leaves
 * a group unpenalised).  G = 0 or sizes = NULL restores the ungrouped prox bit for bit.  ADMM_E_INVALID: a size below 1,
 * sizes that do not sum to n, a negative or non-finite group weight (its index named) or l1[k] (the fit named);
 * ADMM_E_UNSUPPORTED: more than 65536 groups that cannot be packed.  A refused call changes nothing. */
int admm_group_l1class_set_groups(admm_l1class* obj, int32_t G, const int64_t* sizes, const double* groupweights,
                                  const double* l1);
/* fits one pass over D serves (K beyond it: ceil(K / chunk) chunks, each with its own two passes) */
int admm_l1class_chunk(void);
/* the last run's kernel launches, and how many of them read D (two per chunk and iteration plus one per chunk before
 * the first; the same with and without the dual residual) */
int admm_l1class_launches(admm_l1class* obj, int64_t* launches, int64_t* d_passes);
/* measurement: the forward and the transposed pass alone over the object's own buffers (one chunk, every fit
 * running, the element update included), event-timed: the medians of reps launches in microseconds and the bytes of D
 * one pass reads.  nvec = 1 | 3: the transposed pass without / with the dual residual's vectors.  Overwrites the
 * iterates: call it between runs. */
int admm_l1class_pass_time(admm_l1class* obj, int32_t reps, int32_t nvec, double* forward_us, double* transposed_us,
                           int64_t* d_bytes);
void admm_l1class_destroy(admm_l1class* obj);

/* ---- sparse linear classifiers on a SPARSE design matrix, K fits over one sparse product (additive to ABI 5; DESIGN.md
 * q43): the family, the arithmetic, the stop rule and the histories of admm_l1class above, fit for fit --
 *   minimise C*sum_i c_ik*phi_k(ell_ik*(D x)_i) + lambda_k*sum_j w_j*|x_j| + mu_k/2*||x||^2  [x >= 0 when nonneg_k]
 * as plain ADMM with A = [D; I_cols], B = -1, c = 0, z = [z1 (rows); z2 (cols)], stopcond 'standard' -- with the x-update
 * (D'D + I) x = D'(z1 - u1) + (z2 - u2) solved by the lock-step conjugate gradients of admm_sparse_lasso with the shift
 * 1, whatever rho is: nothing factored, nothing cols x cols stored, no limit on cols, positive definite for every D.  The
 * first x-update of a run starts CG from 0 (x0 is never read) and every later one from the previous x.  Per iteration
 * beside the solve: one product D X, one product D'(z1 - u1); the dual residual rho*||D'(z1 - z1prev) + (z2 - z2prev)||
 * and its tolerance rho*||D'u1 + u2|| cost two more transposed products, which nodualerror = 1 leaves out.  rho is a run
 * option.
 * ADMM_E_INVALID (before the device is touched): whatever admm_engine_create_sparse refuses in D, D not in host arrays,
 * and everything admm_l1class_create refuses (K < 1, nell not 1 or K, a label that is not +-1, per fit -- named in the
 * message -- a loss other than ADMM_LOSS_HINGE / _SQHINGE / _LOGISTIC, a negative or non-finite lambda or ridge, nonneg
 * other than 0 | 1; a negative or non-finite l1 weight, its index named; C that is not finite and > 0).
 * ADMM_E_UNSUPPORTED: a communicator, an xsolve other than AUTO / CG; at run: fast ADMM, relaxation, convtest.  Vector
 * histories are not recorded. */
typedef struct admm_sparse_l1class admm_sparse_l1class; /* opaque */

typedef struct admm_sparse_l1class_desc {
  int32_t struct_size;        /* sizeof(admm_sparse_l1class_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  const admm_sparse_desc* D;  /* rows x cols, ADMM_MEM_HOST; copied at create */
  const double* ELL;          /* rows x nell HOST labels +-1, column-major: one column for every fit, or one per fit */
  int32_t nell;               /* 1 or K */
  int32_t device;             /* HIP device ordinal */
  double C;                   /* default 1.0: the cost of the loss term, > 0 */
  int32_t xsolve;             /* ADMM_XSOLVE_AUTO (default) or ADMM_XSOLVE_CG: the matrix-free x-update */
  int32_t reserved0;
  const int32_t* loss;        /* K values ADMM_LOSS_HINGE | _SQHINGE | _LOGISTIC (NULL = logistic for every fit) */
  const double* lambda;       /* K values lambda_k >= 0 */
  const double* ridge;        /* K values mu_k >= 0 (NULL = 0) */
  const int32_t* nonneg;      /* K values 0 | 1 (NULL = 0) */
  const double* l1weights;    /* cols l1 weights w_j >= 0 shared by all fits (NULL = 1); admm_sparse_l1class_set_l1weights
                                 replaces them */
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_sparse_l1class_desc;

typedef struct admm_sparse_l1class_options {
  int32_t struct_size;   /* sizeof(admm_sparse_l1class_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0; any value > 0: the x-update's matrix does not depend on it */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations between host polls of "every fit has stopped" (0 = auto: 8; 64 with domaxiters) */
  int32_t cg_maxit;      /* cap on the inner iterations of one x-update; default 200, <= 0 = default */
  double cg_tol;         /* relative residual of the x-update; default 1e-12, <= 0 = default */
  int32_t nodualerror;   /* default 0: admm.m's rule on both residuals; 1: stop on pnorm < perr alone */
  int32_t reserved0;
  const double* x0;      /* accepted and never read (see above) */
  const double* z0;      /* (rows + cols) x K host matrix, z1 above z2 (NULL = zeros) */
  const double* u0;      /* (rows + cols) x K */
} admm_sparse_l1class_options;

typedef struct admm_sparse_l1class_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* the objective at the fit's last step, NaN if not evaluated */
  int32_t xsolve;             /* ADMM_XSOLVE_CG */
  int32_t reserved0;
  int64_t cg_iters_total;     /* inner iterations of the fit over the run */
  int64_t cg_capped_updates;  /* x-updates of the fit that ended with the residual still above cg_tol */
} admm_sparse_l1class_summary;

/* admm_sparse_l1class_fetch takes the fields of admm_l1class_fetch (ADMM_L1C_F_*): XOPT cols x K, ZOPT and UOPT
 * (rows + cols) x K, the scalar histories as there */
void admm_sparse_l1class_desc_default(admm_sparse_l1class_desc* desc);
void admm_sparse_l1class_options_default(admm_sparse_l1class_options* opts);
int admm_sparse_l1class_create(const admm_sparse_l1class_desc* desc, admm_sparse_l1class** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object,
 * with another rho as well: every run starts from its own z0 / u0, and two runs from the same starts give the same bits */
int admm_sparse_l1class_run(admm_sparse_l1class* obj, const admm_sparse_l1class_options* opts,
                            admm_sparse_l1class_summary* summaries, double* runtime_s);
int admm_sparse_l1class_fetch(admm_sparse_l1class* obj, int field, double* dst, size_t cap, size_t* written);
/* admm_l1class_set_cost and admm_l1class_set_l1weights on this object: rows weights, K x 2 class costs; cols l1 weights */
int admm_sparse_l1class_set_cost(admm_sparse_l1class* obj, const double* weights, const double* class_cost);
int admm_sparse_l1class_set_l1weights(admm_sparse_l1class* obj, const double* l1weights);
/* admm_group_l1class_set_groups on the sparse object (sizes sum to cols); it combines with set_cost, set_l1weights and set_folds in
 * any order, and admm_sparse_l1class_kernel_time then times the grouped element kernel */
int admm_sparse_l1class_set_groups(admm_sparse_l1class* obj, int32_t G, const int64_t* sizes, const double* groupweights,
                                   const double* l1);
/* Held-out folds for every later run (additive to ABI 5): fit k gets the cost c_ik = weights[i] * (class
 * cost of fit k by the sign of ell_ik) * [fold[i] != heldout[k]] -- K classifiers that each leave one fold of rows out,
 * over one D.  fold: rows HOST fold ids in [0, nfolds); heldout: K values in [-1, nfolds), -1 (and NULL) = the fit holds
 * nothing out.  Both copied at the call.  The x-update's matrix D'D + I holds no cost, so every fit keeps the operator it
 * had: a held-out row is a row of cost 0, a select in the row kernel.  Fit k's minimiser is that of the classifier on the
 * rows it keeps; its iterates and its stop rule are those of the full-row problem with zero-cost rows: on a held-out row
 * z1 = D x + u1 and u1 = 0 after one iteration, and such rows still enter ||A x||, ||z|| and the dual products.  fold and
 * heldout both NULL restore the object without folds, bit for bit.  Combines with admm_sparse_l1class_set_cost in either
 * order.  ADMM_E_INVALID, the culprit named, in the words of admm_sparse_lasso_set_observations: nfolds < 1 with fold
 * given, a fold id outside [0, nfolds) (its row), a heldout outside [-1, nfolds) (its fit), heldout without fold.  A
 * refused call changes nothing. */
int admm_sparse_l1class_set_folds(admm_sparse_l1class* obj, int32_t nfolds, const int32_t* fold, const int32_t* heldout);
/* The held-out sums of the last run under folds, K doubles each, evaluated behind the loop at t = D z2 (z2: the sparse
 * coefficient block of z) for every fit over the rows with fold[i] = heldout[k], with c_i = weights[i] * class cost:
 * loss[k] = sum c_i*phi_k(ell_ik*t_i) (without the factor C), errors[k] = sum c_i*[ell_ik*t_i <= 0], weight[k] = sum c_i
 * (all 0.0 for a fit that holds nothing out).  ADMM_E_INVALID before a run or when the last run had no folds set. */
int admm_sparse_l1class_heldout(admm_sparse_l1class* obj, double* loss, double* errors, double* weight);
/* The multinomial (softmax) loss for every later run (additive to ABI 5).  classes = Cn in 2 .. 10 (the
 * chunk) turns the K fits into models of Cn classes each: P = floor(10 / Cn) models share a chunk of ten fits, model p of
 * a chunk owns its slots [p*Cn, (p + 1)*Cn), and the slots >= P*Cn of every chunk are idle -- never run, their summaries
 * and histories never written (steps 0).  One model is ONE ADMM problem over x (cols x Cn):
 *   C*sum_i c_i*(logsumexp((D x)_i,:) - (D x)_i,y_i) + sum_c [lambda*sum_j w_j*|x_jc| + mu/2*||x_c||^2]  (x >= 0 where nonneg)
 * with c_i = weights[i] * class_cost[2 k] of the true class's fit k (admm_sparse_l1class_set_cost; the second cost of a
 * pair is not read).  The labels stay the +-1 one-vs-rest coding: column k of ELL is +1 on the rows whose class is k's.
 * The classes meet in the prox of a row -- the root of z - v + a*(softmax(z) - e_y), a = C*c_i/rho, by a damped Newton
 * iteration with a Sherman-Morrison solve -- and in the stop rule: pnorm, perr, dnorm and derr run over all (m + n)*Cn
 * stacked elements, both tolerances use sqrt((m + n)*Cn), and a model has one objective and one stop decision, reported
 * in the summary and the histories of each of its Cn fits.  The x-update, the products and the penalties are the per-fit
 * object's.  classes = 0 restores the per-fit object, bit for bit.
 * ADMM_E_INVALID, the slot or the row named: classes outside {0, 2 .. 10}; K mod 10 no multiple of Cn or above P*Cn; a
 * shared label column (nell = 1); a live fit whose loss is not logistic; lambda, ridge or nonneg that differ within a
 * model; a row that has not exactly one +1 among a model's label columns.  ADMM_E_UNSUPPORTED: folds or groups are set --
 * and admm_sparse_l1class_set_folds / _set_groups return it while classes > 0.  A refused call changes nothing.
 * admm_sparse_l1class_kernel_time then times the multinomial row kernel. */
int admm_sparse_l1class_set_multinomial(admm_sparse_l1class* obj, int32_t classes);
/* The row prox of q49 alone, on HOST arrays: V is m x Cn row-major, y[i] in [0, Cn) the true class of row i, a[i] >= 0
 * finite; out (m x Cn row-major) = argmin_z a[i]*(lse(z) - z_y[i]) + 1/2*||z - V_i||^2 and iters_out[i] = the Newton steps
 * row i took (at most 100).  a[i] = 0 returns the row bit for bit.  Cn in 2 .. 10. */
int admm_op_softmax_prox(const double* V, const int32_t* y, const double* a, int64_t m, int32_t Cn, double* out,
                         int32_t* iters_out);
/* fits one sparse product serves (K beyond it: ceil(K / chunk) chunks per launch) */
int admm_sparse_l1class_chunk(void);
/* measurement: the row kernel and the element kernel alone over the object's own buffers (every fit running, the dual
 * residual's sums included with dual != 0), event-timed: the medians of reps launches in microseconds.  Overwrites the
 * iterates: call it between runs. */
int admm_sparse_l1class_kernel_time(admm_sparse_l1class* obj, int32_t reps, int32_t dual, double* row_us, double* elem_us);
void admm_sparse_l1class_destroy(admm_sparse_l1class* obj);

/* ---- covariance selection, K fits over one S in one run (additive to ABI 5): a regularisation path or a
 * cross-validation grid of
 *   minimise trace(S*X) - log det X + lambda_k*||Z||_1  s.t. X = Z,   S = cov(D) or given,
 * every fit the plain-ADMM run an ADMM_PROB_COVSEL engine makes (A = 1, B = -1, c = 0 on the n^2 entries, 'fro' norms,
 * stopcond 'standard').  One kernel carries a fit's whole iteration -- the eigen-step of the engine's one-workgroup path
 * (csrc/covsel_device.h), the soft threshold, the residual sums and the stop decision -- in ONE workgroup per fit, and
 * one launch runs up to check_every iterations of every fit.  The fits share nothing but S; the eigen-step caches no
 * factor, so rho may differ per fit (options.rhos).  Iterates are n x n column-major, fit after fit.
 * ADMM_E_INVALID (before the device is touched): K < 1, n < 1, neither or both of D and S, m < 2 with D, an S that is
 * not finite and symmetric, per fit (named in the message) a lambda that is not positive and finite; at run a rho_k that
 * is not positive and finite.  ADMM_E_UNSUPPORTED: n > 96 (a fit has to fit one workgroup's LDS: run one ADMM_PROB_COVSEL
 * engine per fit), a communicator; at run: fast ADMM, relaxation, convtest.  Vector histories are not recorded. */
typedef struct admm_covsel_multi admm_covsel_multi; /* opaque */

typedef struct admm_covsel_multi_desc {
  int32_t struct_size;        /* sizeof(admm_covsel_multi_desc) */
  int32_t K;                  /* number of fits, >= 1 */
  int64_t m, n;               /* D is m x n (m samples of n variables); S is n x n, n <= 96 */
  const double* D;            /* HOST, column-major; S = cov(D) is built on the device at create.  Or NULL with S */
  int64_t ldD;                /* >= m */
  const double* S;            /* HOST n x n symmetric, leading dimension n, in place of D.  Or NULL with D */
  const double* lambda;       /* K values lambda_k > 0 */
  int32_t device;             /* HIP device ordinal */
  int32_t reserved0;
  admm_comm* comm;            /* must be NULL (row sharding: ADMM_E_UNSUPPORTED) */
} admm_covsel_multi_desc;

typedef struct admm_covsel_multi_options {
  int32_t struct_size;   /* sizeof(admm_covsel_multi_options) */
  int32_t maxiters;      /* default 1000 */
  double rho;            /* default 1.0: the rho of every fit unless rhos is given */
  double abstol;         /* default 1e-5 */
  double reltol;         /* default 1e-3 */
  double relax;          /* default 1.0; anything else: ADMM_E_UNSUPPORTED */
  int32_t fast;          /* default ADMM_FAST_OFF; anything else: ADMM_E_UNSUPPORTED */
  int32_t convtest;      /* default 0; anything else: ADMM_E_UNSUPPORTED */
  int32_t domaxiters;    /* default 0 */
  int32_t objevals;      /* default 0 */
  int32_t check_every;   /* iterations of every fit in one launch, between two host polls (0 = auto: 8; 64 with domaxiters) */
  int32_t nodualerror;   /* default 0: admm.m's rule on both residuals; 1: stop on pnorm < perr alone */
  const double* rhos;    /* K values rho_k > 0, or NULL: rho for every fit */
  const double* z0;      /* n*n x K host matrix, one n x n column-major start per fit (NULL = zeros) */
  const double* u0;      /* n*n x K */
} admm_covsel_multi_options;

typedef struct admm_covsel_multi_summary {  /* one per fit */
  int32_t steps;              /* results.steps of that fit (admm.m:746) */
  int32_t stopped_early;      /* 1 if the stop rule fired before maxiters (admm.m:710-713) */
  double objopt;              /* the objective at the fit's last step, NaN if not evaluated */
  int32_t jacobi_sweeps;      /* sweeps of the fit's eigen-steps over the run */
  int32_t reserved0;
} admm_covsel_multi_summary;

/* fields of admm_covsel_multi_fetch */
enum {
  ADMM_CM_F_XOPT = 1,      /* n*n x K */
  ADMM_CM_F_ZOPT = 2,      /* n*n x K */
  ADMM_CM_F_UOPT = 3,      /* n*n x K */
  /* scalar histories: S x K column-major with S = the largest steps of any fit, NaN past a fit's own last step; DNORM
   * and DERR after a run with nodualerror = 0 only, OBJEVALS after a run with objevals = 1 only */
  ADMM_CM_F_PNORM = 4, ADMM_CM_F_PERR = 5, ADMM_CM_F_OBJEVALS = 6, ADMM_CM_F_DNORM = 7, ADMM_CM_F_DERR = 8,
  ADMM_CM_F_COV = 9        /* S as the object holds it, n x n (cap >= n*n): available from create on */
};

void admm_covsel_multi_desc_default(admm_covsel_multi_desc* desc);
void admm_covsel_multi_options_default(admm_covsel_multi_options* opts);
int admm_covsel_multi_create(const admm_covsel_multi_desc* desc, admm_covsel_multi** out);
/* summaries: K entries (may be NULL); runtime_s: the loop alone (may be NULL).  May be called again on the same object,
 * with other rhos as well: every run starts from its own z0 / u0 and from the eigenvector basis I, and two runs from the
 * same starts give the same bits.  A fit's results do not depend on K or on the other fits. */
int admm_covsel_multi_run(admm_covsel_multi* obj, const admm_covsel_multi_options* opts,
                          admm_covsel_multi_summary* summaries, double* runtime_s);
int admm_covsel_multi_fetch(admm_covsel_multi* obj, int field, double* dst, size_t cap, size_t* written);
void admm_covsel_multi_destroy(admm_covsel_multi* obj);

/* X(:, k) = M * Y(:, k) for the columns k < K whose stop_mask[k] is 0 (stop_mask == NULL: every column) through the
 * multi-lasso's product kernel (csrc/symm.hip): M symmetric n x n (ldM >= n), only its lower triangle is read (the
 * operator builds the tile-packed triangle from it); X and Y are n x K column-major HOST matrices.  X is in/out: a masked
 * column keeps the caller's values bit for bit.  The kernel streams every tile non-temporally: there is no cache split. */
int admm_op_symm_packed(const double* M, int64_t n, int64_t ldM, double* X, int32_t K, const int32_t* stop_mask,
                        const double* Y);

/* Z(:, k) = the block soft threshold of V(:, k) with the thresholds t[k]*omega_g, for the columns k < K whose
 * stop_mask[k] is 0 (stop_mask == NULL: every column), through the device functions of the multi-fit lasso's grouped
 * element kernel (csrc/group_multi.hip) over its fit-interleaved layout and its plan: stage 2 of the prox
 * alone.  V and Z are n x K column-major HOST matrices; sizes / ngroups / groupweights as admm_op_group_soft_threshold;
 * t holds K finite values >= 0.  Z is in/out: a masked column keeps the caller's values bit for bit. */
int admm_op_group_soft_threshold_multi(const double* V, int64_t n, int32_t K, const int64_t* sizes, int32_t ngroups,
                                       const double* groupweights, const double* t, const int32_t* stop_mask, double* Z);
/* The plan of that kernel, on the host alone (no device is touched): *nwg workgroups, workgroup b owning the rows
 * wg_first[b] .. wg_first[b + 1] (cap >= *nwg + 1 entries; wg_first may be NULL), and the row budget it was packed for. */
int admm_group_multi_plan(int64_t n, const int64_t* sizes, int32_t ngroups, int64_t* wg_first, int32_t cap, int32_t* nwg,
                          int64_t* budget);

#ifdef __cplusplus
}
#endif
#endif /* ADMM_ENGINE_H */
