// lasso_multi.hip -- the lasso on a DENSE design matrix, K fits at once over one cached inverse: a
// regularisation path, a cross-validation grid or several response columns.  The family, the arithmetic and the element
// kernels are sparse_lasso.hip's (q39): K independent plain-ADMM runs of lasso.m:227-239 (A = 1, B = -1, c = 0, sizes n,
// stopcond 'standard') that share D, rho and the l1 weights and differ in (lambda_k, mu_k, nonneg_k) and optionally in
// their column of S.  What differs is the x-update: an ordinary ADMM_PROB_LASSO engine, which never runs, owns D, the
// factor of D'D + rho*I and its explicit inverse, and
//   X = inv(D'D + rho*I) Y        symm.hip: the fp64 tile-packed inverse read ONCE per chunk of kSpmmChunk fits
// replaces the lock-step CG.  The inverse depends on D and rho alone, so rho is fixed at create.  Where create's accuracy
// probe keeps the triangular solves, the x-update is K launch_trsv_pair calls between a gather and a scatter of the
// fit-interleaved layout.  Per iteration, for all fits:
//   launch_symm_packed            X from Y, two launches
//   launch_slm_elem               z, u, the next right-hand side rho*(z - u) + D's_k, six partial sums per fit
//                                 (launch_slm_group_elem with groups set: admm_lasso_multi_set_groups, q41)
//   (objevals = 1)                T = D X per chunk through launch_gemm (T' = X' D'), then launch_slm_fit
//   launch_slm_fin                the fit's residuals, tolerances, objective and stop decision
// Freezing, determinism and the histories are q39's: a stopped fit is skipped by every kernel, no atomics, every sum in an
// order the sizes fix.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "group_multi.h"
#include "multi_host.h"
#include "sparse_lasso.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// the triangular solves take one contiguous vector per fit: col[k][ld] <- the fit's column of a multi-vector, and back
// for the running fits
__global__ __launch_bounds__(kBlock) void lm_gather_kernel(const double* __restrict__ V, int64_t n, int32_t K,
                                                           double* __restrict__ col, int64_t ld) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int32_t k = blockIdx.y;
  if (i < n) col[k * ld + i] = V[(static_cast<int64_t>(k / KC) * n + i) * KC + k % KC];
}

__global__ __launch_bounds__(kBlock) void lm_scatter_kernel(const double* __restrict__ col, int64_t ld, int64_t n,
                                                            int32_t K, const MultiRec* __restrict__ rec,
                                                            double* __restrict__ V) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int32_t k = blockIdx.y;
  if (i < n && rec[k].stop == 0) V[(static_cast<int64_t>(k / KC) * n + i) * KC + k % KC] = col[k * ld + i];
}

}  // namespace

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_lasso_multi : MultiHost {
  admm_engine* eng = nullptr;  // an ordinary ADMM_PROB_LASSO engine: D, the factor, the inverse; stream = eng->stream
  int64_t m = 0, n = 0, ldt = 0;
  int32_t ns = 1, chunks = 0, nwg_n = 0, nwg_m = 0;
  double rho = 1.0;
  SymvPlan plan{};             // the packed plan of the inverse (null P: the triangular solves)
  const double* P = nullptr;   // fp64 tile-packed inverse: the engine's own, or packed here below kSymvHalfMin
  double* spart = nullptr;     // partial rows of the product
  double *ycol = nullptr, *xcol = nullptr;  // [K][ldt]: the triangular solves' vectors
  double *X = nullptr, *Y = nullptr, *Z = nullptr, *U = nullptr;  // multi-vectors of len n
  double* T = nullptr;         // D X, a multi-vector of len m (objevals)
  double* S = nullptr;         // ns == 1: ONE chunk of len m, column 0; ns == K: a multi-vector of len m
  double* DTS = nullptr;       // D'S in the layout of S, len n
  double *part = nullptr, *fpart = nullptr;
  double *W = nullptr, *par = nullptr;
  int32_t* nonneg = nullptr;
  GroupMulti grp;  // admm_lasso_multi_set_groups (q41)
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  admm_lasso_multi_options last{};
};

namespace {

using namespace admm;

const char* kPerFit = ": run one ADMM_PROB_LASSO engine (admm_engine_create) per fit instead";

// host column-major (rows x cols, ld) <-> a chunked multi-vector on the device
int lm_upload(admm_lasso_multi* o, double* dst, const double* src, int64_t rows, int32_t cols, int32_t chunks) {
  const size_t elems = static_cast<size_t>(chunks) * KC * rows;
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * elems, o->stream));
    return ADMM_OK;
  }
  std::vector<double> hb(elems);
  spmm_pack(src, rows, rows, cols, hb.data());
  ADMM_HIP_TRY(hipMemcpyAsync(dst, hb.data(), sizeof(double) * elems, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hb goes out of scope)
  return ADMM_OK;
}

int lm_fetch(admm_lasso_multi* o, const double* src, int64_t rows, double* dst, size_t cap, size_t* written) {
  const size_t need = static_cast<size_t>(rows) * o->K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  std::vector<double> hb(static_cast<size_t>(o->chunks) * KC * rows);
  ADMM_HIP_TRY(hipMemcpy(hb.data(), src, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
  spmm_unpack(hb.data(), rows, o->K, dst, rows);
  if (written) *written = need;
  return ADMM_OK;
}

int lm_setup(admm_lasso_multi* o, const admm_lasso_multi_desc* desc, const std::vector<double>& ph,
             const std::vector<int32_t>& nh) {
  const int64_t m = desc->m, n = desc->n;
  const int32_t K = desc->K;
  admm_problem_desc d;
  admm_problem_desc_default(&d);
  d.problem = ADMM_PROB_LASSO;
  d.m = m;
  d.n = n;
  d.D = desc->D;
  d.ldD = desc->ldD;
  d.s = desc->S;  // (the engine wants one response; it never runs)
  d.lambda = 0.0;
  d.rho = desc->rho;
  d.xsolve = desc->xsolve;
  d.mem = ADMM_MEM_HOST;
  d.device = desc->device;
  ADMM_TRY(engine_create_keep_fp64(&d, &o->eng));
  admm_engine* e = o->eng;
  o->stream = e->stream;
  o->device = e->device;
  o->K = K;
  o->m = m;
  o->n = n;
  o->ns = desc->ns;
  o->rho = desc->rho;
  o->chunks = spmm_chunks(K);
  o->nwg_n = scg_vec_workgroups(n);
  o->nwg_m = scg_vec_workgroups(m);
  o->ldt = round_up(n, 2);
  const SliceFactor& f = e->xfac;
  const size_t kp = static_cast<size_t>(o->chunks) * KC;
  if (f.mode == ADMM_XSOLVE_INVERSE && f.Minv && !f.pinv && !f.planSy.cbits) {
    o->plan = f.planSy;
    if (f.planSy.packed) {
      o->P = f.Minv;
    } else {  // full symmetric storage below kSymvHalfMin: the product has one form, so the tiles are packed here
      double* P = nullptr;
      ADMM_TRY(o->mem.alloc(&P, symv_packed_elems(o->plan)));
      launch_symv_pack(o->plan, f.Minv, f.ldM, P, o->stream);
      o->plan.packed = true;
      o->P = P;
    }
    ADMM_TRY(o->mem.alloc(&o->spart, symm_part_elems(o->plan, K)));
  } else if (f.mode == ADMM_XSOLVE_TRSV && f.F) {
    for (double** p : {&o->ycol, &o->xcol}) {
      ADMM_TRY(o->mem.alloc(p, static_cast<size_t>(o->ldt) * K));
      ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * o->ldt * K, o->stream));
    }
  } else {
    return fail(ADMM_E_UNSUPPORTED, std::string("the engine built no n x n form of the x-update for this D") + kPerFit);
  }
  for (double** p : {&o->X, &o->Y, &o->Z, &o->U}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  ADMM_TRY(o->mem.alloc(&o->T, kp * m));
  ADMM_HIP_TRY(hipMemsetAsync(o->T, 0, sizeof(double) * kp * m, o->stream));
  {  // S in the layout of the element kernels, and D'S for its ns columns once, by the dense product
    const int32_t sch = o->ns == 1 ? 1 : o->chunks;
    const size_t sp = static_cast<size_t>(sch) * KC;
    ADMM_TRY(o->mem.alloc(&o->S, sp * m));
    ADMM_TRY(o->mem.alloc(&o->DTS, sp * n));
    ADMM_TRY(lm_upload(o, o->S, desc->S, m, o->ns, sch));
    double *sc = nullptr, *gc = nullptr;  // column-major S (ld m) and D'S (ld n)
    ADMM_TRY(o->mem.alloc(&sc, static_cast<size_t>(m) * o->ns));
    ADMM_TRY(o->mem.alloc(&gc, static_cast<size_t>(n) * o->ns));
    ADMM_HIP_TRY(hipMemcpyAsync(sc, desc->S, sizeof(double) * m * o->ns, hipMemcpyHostToDevice, o->stream));
    launch_gemm(1, 0, n, o->ns, m, 1.0, e->D, e->ldD, sc, m, 0.0, gc, n, false, o->stream);
    std::vector<double> gh(static_cast<size_t>(n) * o->ns);
    ADMM_HIP_TRY(hipMemcpyAsync(gh.data(), gc, sizeof(double) * gh.size(), hipMemcpyDeviceToHost, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
    ADMM_TRY(lm_upload(o, o->DTS, gh.data(), n, o->ns, sch));
    o->mem.free_one(sc);
    o->mem.free_one(gc);
  }
  ADMM_TRY(o->mem.alloc(&o->part, kp * SL_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * kp * SL_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->fpart, kp * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->fpart, 0, sizeof(double) * kp * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(2) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_words(*o, &o->nonneg, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->nonneg, nh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (ph, nh and the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  if (desc->weights) ADMM_TRY(set_shared_weights(*o, n, desc->weights, &o->W));
  return ADMM_OK;
}

// X <- inv(D'D + rho*I) Y for every running fit
void lm_xupdate(admm_lasso_multi* o) {
  if (o->P) {
    launch_symm_packed(o->plan, o->P, o->Y, o->X, o->spart, o->rec, o->K, o->stream);
    return;
  }
  const dim3 grid(static_cast<unsigned>(ceil_div(o->n, kBlock)), static_cast<unsigned>(o->K));
  hipLaunchKernelGGL(lm_gather_kernel, grid, dim3(kBlock), 0, o->stream, o->Y, o->n, o->K, o->ycol, o->ldt);
  for (int32_t k = 0; k < o->K; ++k)
    launch_trsv_pair(o->eng->xfac.trsv, o->ycol + static_cast<int64_t>(k) * o->ldt,
                     o->xcol + static_cast<int64_t>(k) * o->ldt, nullptr, o->stream);
  hipLaunchKernelGGL(lm_scatter_kernel, grid, dim3(kBlock), 0, o->stream, o->xcol, o->ldt, o->n, o->K, o->rec, o->X);
}

}  // namespace

extern "C" {

void admm_lasso_multi_desc_default(admm_lasso_multi_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_lasso_multi_desc);
  d->K = 1;
  d->ns = 1;
  d->rho = 1.0;  // admm.m:57
  d->xsolve = ADMM_XSOLVE_AUTO;
}

void admm_lasso_multi_options_default(admm_lasso_multi_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_lasso_multi_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->nodualerror = 0;  // admm.m:76: the reference lasso's stop rule (the dual residual costs no product here)
}

int admm_lasso_multi_chunk(void) { return kSpmmChunk; }

int admm_lasso_multi_create(const admm_lasso_multi_desc* desc, admm_lasso_multi** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_lasso_multi_desc)))
    return fail(ADMM_E_INVALID, "admm_lasso_multi_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the multi-lasso needs at least one fit (K >= 1)");
  if (!desc->D || desc->m <= 0 || desc->n <= 0 || desc->ldD < desc->m)
    return fail(ADMM_E_INVALID, "the multi-lasso needs D (m x n, ldD >= m)");
  if (!desc->S) return fail(ADMM_E_INVALID, "the multi-lasso needs the responses S (m x ns)");
  ADMM_TRY(check_response_columns(desc->ns, desc->K));
  if (!desc->lambda) return fail(ADMM_E_INVALID, "the multi-lasso needs lambda (K values)");
  std::vector<double> ph(static_cast<size_t>(2) * desc->K, 0.0);
  std::vector<int32_t> nh(static_cast<size_t>(desc->K), 0);
  for (int32_t k = 0; k < desc->K; ++k) {
    const std::string who = "fit " + std::to_string(k) + ": ";
    ph[2 * k] = desc->lambda[k];
    if (!finite_nonneg(ph[2 * k])) return fail(ADMM_E_INVALID, who + "lambda is negative or not finite");
    if (desc->ridge) ph[2 * k + 1] = desc->ridge[k];
    if (!finite_nonneg(ph[2 * k + 1])) return fail(ADMM_E_INVALID, who + "ridge is negative or not finite");
    if (desc->nonneg) nh[k] = desc->nonneg[k];
    if (nh[k] != 0 && nh[k] != 1) return fail(ADMM_E_INVALID, who + "nonneg must be 0 or 1");
  }
  if (desc->weights)
    for (int64_t i = 0; i < desc->n; ++i)
      if (!finite_nonneg(desc->weights[i]))
        return fail(ADMM_E_INVALID, "penalty: weight " + std::to_string(i) + " is negative or not finite");
  if (!finite_pos(desc->rho)) return fail(ADMM_E_INVALID, "desc.rho must be positive and finite");
  if (desc->xsolve != ADMM_XSOLVE_AUTO && desc->xsolve != ADMM_XSOLVE_INVERSE && desc->xsolve != ADMM_XSOLVE_TRSV)
    return fail(ADMM_E_UNSUPPORTED, std::string("the multi-lasso applies the cached factor (xsolve = auto, inverse or "
                                                "trsv)") + kPerFit);
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, std::string("the multi-lasso is not row-sharded") + kPerFit);
  if (desc->m < desc->n)
    return fail(ADMM_E_UNSUPPORTED, "the fat lasso (m < n) applies its m x m factor through two dense products per fit "
                                    "(getProxOps.m:1201-1205), which the multi-lasso does not form: run lasso per fit");
  return create_object(out, admm_lasso_multi_destroy, [&](admm_lasso_multi* o) { return lm_setup(o, desc, ph, nh); });
}

int admm_lasso_multi_run(admm_lasso_multi* o, const admm_lasso_multi_options* opts, admm_lasso_multi_summary* summaries,
                         double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_lasso_multi_options)))
    return fail(ADMM_E_INVALID, "admm_lasso_multi_options.struct_size mismatch (ABI version skew)");
  admm_lasso_multi_options op = *opts;
  ADMM_TRY(check_run_options("multi-lasso", kPerFit, &op));
  if (op.rho != o->rho)
    return fail(ADMM_E_INVALID, "options.rho = " + std::to_string(op.rho) + " differs from the rho the cached factor was "
                                "built for (" + std::to_string(o->rho) + "): create another object");
  const bool dual = op.nodualerror == 0;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  ADMM_TRY(begin_run(*o));
  ADMM_HIP_TRY(hipMemsetAsync(o->X, 0, sizeof(double) * o->chunks * KC * o->n, o->stream));
  ADMM_TRY(lm_upload(o, o->Z, op.z0, o->n, K, o->chunks));
  ADMM_TRY(lm_upload(o, o->U, op.u0, o->n, K, o->chunks));

  SlmElemArgs ea{};
  ea.n = o->n;
  ea.X = o->X;
  ea.Z = o->Z;
  ea.U = o->U;
  ea.Y = o->Y;
  ea.DTS = o->DTS;
  ea.W = o->W;
  ea.par = o->par;
  ea.nonneg = o->nonneg;
  ea.rec = o->rec;
  ea.part = o->part;
  ea.K = K;
  ea.ns = o->ns;
  ea.dts_ns = o->ns;
  ea.objevals = op.objevals;
  ea.rho = op.rho;
  SlmFitArgs ta{};
  ta.m = o->m;
  ta.T = o->T;
  ta.S = o->S;
  ta.rec = o->rec;
  ta.part = o->fpart;
  ta.K = K;
  ta.ns = o->ns;
  SlmFinArgs fa{};
  fa.part = o->part;
  fa.fpart = o->fpart;
  fa.n = o->n;
  fa.K = K;
  fa.nwg_n = o->grp.on() ? o->grp.plan.nwg : o->nwg_n;  // (the grouped kernel: one partial per workgroup of the plan)
  fa.nwg_m = o->nwg_m;
  fa.dual = dual ? 1 : 0;
  fa.rec = o->rec;
  fa.pnorm = o->pnorm;
  fa.perr = o->perr;
  fa.dnorm = o->dnorm;
  fa.derr = o->derr;
  fa.objv = o->objv;
  fa.hist_ld = N;
  fa.rho = op.rho;
  fa.abstol = op.abstol;
  fa.reltol = op.reltol;
  fa.domaxiters = op.domaxiters;
  fa.objevals = op.objevals;
  fa.fit_slots = 1;
  fa.maxiters = N;

  ADMM_TRY(begin_timing(*o));
  launch_slm_elem(ea, true, o->stream);  // y = rho*(z0 - u0) + D's
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    lm_xupdate(o);
    if (o->grp.on()) launch_slm_group_elem(ea, o->grp, o->stream);
    else launch_slm_elem(ea, false, o->stream);
    if (op.objevals) {
      for (int32_t ch = 0; ch < o->chunks; ++ch)  // T' = X' D' per chunk: (KC x n)(n x m), both of leading dimension KC
        launch_gemm(0, 1, KC, o->m, o->n, 1.0, o->X + static_cast<int64_t>(ch) * o->n * KC, KC, o->eng->D, o->eng->ldD,
                    0.0, o->T + static_cast<int64_t>(ch) * o->m * KC, KC, false, o->stream);
      launch_slm_fit(ta, o->stream);
    }
    launch_slm_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the multi-lasso loop ended with fits still running", N, op.objevals != 0, o->objv,
                      runtime_s, summaries));
  for (int32_t c = 0; summaries && c < K; ++c) summaries[c].xsolve = o->P ? ADMM_XSOLVE_INVERSE : ADMM_XSOLVE_TRSV;
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_lasso_multi_set_weights(admm_lasso_multi* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (weights)  // (the message of the create-time check; a refused call changes nothing)
    for (int64_t i = 0; i < o->n; ++i)
      if (!finite_nonneg(weights[i]))
        return fail(ADMM_E_INVALID, "penalty: weight " + std::to_string(i) + " is negative or not finite");
  return set_shared_weights(*o, o->n, weights, &o->W);
}

int admm_lasso_multi_set_groups(admm_lasso_multi* o, int32_t G, const int64_t* sizes, const double* groupweights,
                                const double* l1) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_multi_groups(*o, o->n, G, sizes, groupweights, l1, &o->grp);
}

int admm_lasso_multi_product_time(admm_lasso_multi* o, int32_t reps, double* us_per_call, int64_t* stored_bytes,
                                  int64_t* fma_count) {
  if (!o || reps < 1) return fail(ADMM_E_INVALID, "object is NULL or reps < 1");
  if (!o->P) return fail(ADMM_E_UNSUPPORTED, "the object applies triangular solves: there is no packed product to time");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  ADMM_TRY(begin_run(*o));  // every fit runs; X is overwritten, as the next run's first x-update does anyway
  lm_xupdate(o);            // warm-up
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  std::vector<float> ms(static_cast<size_t>(reps));
  for (int32_t i = 0; i < reps; ++i) {
    ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
    lm_xupdate(o);
    ADMM_HIP_TRY(hipEventRecord(o->ev1, o->stream));
    ADMM_HIP_TRY(hipEventSynchronize(o->ev1));
    ADMM_HIP_TRY(hipEventElapsedTime(&ms[i], o->ev0, o->ev1));
  }
  ADMM_HIP_TRY(hipGetLastError());
  std::sort(ms.begin(), ms.end());
  const int64_t elems = static_cast<int64_t>(symv_packed_elems(o->plan));
  if (us_per_call) *us_per_call = 1e3 * static_cast<double>(ms[reps / 2]);
  if (stored_bytes) *stored_bytes = 8 * elems;
  if (fma_count) *fma_count = 2 * elems * KC * o->chunks;  // both uses of every stored element, every column of a chunk
  return ADMM_OK;
}

int admm_lasso_multi_fetch(admm_lasso_multi* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_LM_F_XOPT: return lm_fetch(o, o->X, o->n, dst, cap, written);
    case ADMM_LM_F_ZOPT: return lm_fetch(o, o->Z, o->n, dst, cap, written);
    case ADMM_LM_F_UOPT: return lm_fetch(o, o->U, o->n, dst, cap, written);
    case ADMM_LM_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_LM_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_LM_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_LM_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_LM_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the multi-lasso");
  }
}

void admm_lasso_multi_destroy(admm_lasso_multi* o) {
  if (!o) return;
  destroy_common(*o);
  if (o->eng) admm_engine_destroy(o->eng);
  delete o;
}

}  // extern "C"
