// covsel_multi.hip -- covariance selection (sparse inverse covariance), K fits over one S at once: a
// regularisation path or a cross-validation grid.  Every fit is the plain-ADMM run of covarianceselection.m:145-172 that
// an ADMM_PROB_COVSEL engine makes (A = 1, B = -1, c = 0 on the n^2 entries, 'fro' norms, sqrt(numel) = n, stopcond
// 'standard'); the fits share S and differ in lambda_k and, because the eigen-step caches no factor, in rho_k.
//   covsel_multi_kernel           grid = K workgroups of 512 threads, workgroup k owns fit k.  Per iteration:
//                                 X = f(rho_k*Y - S) by covsel_device.h's eigen-step (the one of covsel.hip), then over
//                                 the n^2 entries z = soft(x + u, lambda_k/rho_k), u += x - z, y = z - u with the seven
//                                 sums by block_sum in a fixed order, then the residuals, tolerances, objective and stop
//                                 decision of admm.m:621-654, 710-722.  No workgroup waits for another, so one launch
//                                 runs up to check_every iterations; the host polls the records between launches.
// A fit whose stop flag is set is FROZEN: its workgroup returns at once.  No atomics on doubles; every sum runs in an
// order that n alone fixes, so a fit gets the same bits alone or among K, and two runs give the same bits.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "covsel_device.h"
#include "covsel_multi.h"
#include "multi_host.h"
#include "prox_device.h"

namespace admm {

namespace {

enum { CM_R2 = 0, CM_X2, CM_Z2, CM_DZ2, CM_U2, CM_OBJX, CM_OBJZ, CM_COUNT };

__global__ __launch_bounds__(kCovThreads) void covsel_multi_kernel(CovselMultiArgs a) {
  const int fit = blockIdx.x;
  MultiRec* rec = a.rec + fit;
  if (rec->stop) return;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int32_t stopped;
  const int tid = threadIdx.x;
  const int n = static_cast<int>(a.n);
  const int nn = n * n;
  const int64_t base = static_cast<int64_t>(fit) * nn;
  const double lam = a.lam[fit], rho = a.rho[fit];
  const double t = lam / rho;  // getProxOps.m:750
  double* __restrict__ X = a.X + base;
  double* __restrict__ Z = a.Z + base;
  double* __restrict__ U = a.U + base;
  double* __restrict__ Y = a.Y + base;
  double* V = a.V + base;
  const double* __restrict__ S = a.S;
  double* red = covsel_lds_red(lds, n);
  const CovselArgs ca{a.n, rho, Y, S, X, V, a.n, a.logpart + fit, a.sweeps + fit};
  int it = rec->iter;  // (thread 0 writes the record behind the sums' barriers)
  if (it == 0) {       // a run starts: the first right-hand side, and V = I
    for (int idx = tid; idx < nn; idx += kCovThreads) {
      const int j = idx / n, i = idx - j * n;
      Y[idx] = Z[idx] - U[idx];
      V[idx] = (i == j) ? 1.0 : 0.0;
    }
    __syncthreads();
  }
  for (int s = 0; s < a.iters; ++s, ++it) {
    covsel_eigen_step(ca, lds);
    __syncthreads();  // X (both halves by the thread of the lower one), V and logpart are written
    double acc[CM_COUNT];
#pragma unroll
    for (int q = 0; q < CM_COUNT; ++q) acc[q] = 0.0;
    for (int idx = tid; idx < nn; idx += kCovThreads) {
      const double x = X[idx], zp = Z[idx], uo = U[idx];
      const double zn = soft(x + uo, t);
      const double r = x - zn;   // admm.m:621
      const double un = uo + r;  // admm.m:542-550
      const double dz = zn - zp;
      Z[idx] = zn;
      U[idx] = un;
      Y[idx] = zn - un;
      acc[CM_R2] += r * r;
      acc[CM_X2] += x * x;
      acc[CM_Z2] += zn * zn;
      acc[CM_DZ2] += dz * dz;
      acc[CM_U2] += un * un;
      if (a.objevals) {
        acc[CM_OBJX] += S[idx] * x;  // trace(S*X) = sum S_ij X_ij: X is symmetric
        acc[CM_OBJZ] += fabs(zn);
      }
    }
    double tot[CM_COUNT];
#pragma unroll
    for (int q = 0; q < CM_COUNT; ++q) tot[q] = block_sum(acc[q], red);  // (valid in thread 0)
    if (tid == 0) {
      const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
      const int64_t h = static_cast<int64_t>(fit) * a.hist_ld + it;
      // covarianceselection.m:169: trace(S*x) - log(det(x)) + lambda*norm(z(:), 1)
      if (a.objevals) a.objv[h] = (a.logpart[fit] + lam * tot[CM_OBJZ]) + tot[CM_OBJX];
      const double sqn = static_cast<double>(n);  // sqrt(numel) of an n x n iterate
      const double pn = sqrt(tot[CM_R2]);                                                        // admm.m:621
      const double pe = sqn * a.abstol + a.reltol * fmax(sqrt(tot[CM_X2]), sqrt(tot[CM_Z2]));  // admm.m:644-650, c = 0
      a.pnorm[h] = pn;
      a.perr[h] = pe;
      bool dual_ok = true;
      if (a.dual) {
        const double dn = rho * sqrt(tot[CM_DZ2]);                                 // admm.m:624, A = 1
        const double de = sqn * a.abstol + a.reltol * (rho * sqrt(tot[CM_U2]));  // admm.m:652-654
        a.dnorm[h] = dn;
        a.derr[h] = de;
        dual_ok = dn < de;
      }
      const bool stop = !a.domaxiters && pn < pe && dual_ok;  // admm.m:710-713
      multi_stop_tail(rec, stop, i1, a.maxiters);
      stopped = rec->stop;
    }
    __syncthreads();  // the decision, and this iteration's Y and V before the next eigen-step reads them
    if (stopped) break;
  }
}

}  // namespace

int covsel_multi_prepare() {
  ADMM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(covsel_multi_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(covsel_small_lds(kCovselSmallMax))));
  return ADMM_OK;
}

void launch_covsel_multi(const CovselMultiArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(covsel_multi_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kCovThreads), covsel_small_lds(a.n),
                     stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_covsel_multi : MultiHost {
  int64_t n = 0;
  double* S = nullptr;                          // n x n, ld n, exactly symmetric
  double *lam = nullptr, *rho = nullptr;        // [K]
  double *X = nullptr, *Z = nullptr, *U = nullptr, *Y = nullptr, *V = nullptr;  // [K][n*n]
  double* logpart = nullptr;                    // [K]
  int32_t* sweeps = nullptr;                    // [K]
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  admm_covsel_multi_options last{};
};

namespace {

using namespace admm;

const char* kPerFit = ": run one ADMM_PROB_COVSEL engine (admm_engine_create) per fit instead";

int cm_setup(admm_covsel_multi* o, const admm_covsel_multi_desc* desc) {
  const int64_t m = desc->m, n = desc->n, nn = n * n;
  const int32_t K = desc->K;
  ADMM_HIP_TRY(hipSetDevice(desc->device));
  o->device = desc->device;
  ADMM_HIP_TRY(hipStreamCreate(&o->stream));
  o->K = K;
  o->n = n;
  ADMM_TRY(o->mem.alloc(&o->S, static_cast<size_t>(nn)));
  if (desc->S) {
    ADMM_HIP_TRY(hipMemcpyAsync(o->S, desc->S, sizeof(double) * nn, hipMemcpyHostToDevice, o->stream));
  } else {  // S = cov(D), covarianceselection.m:150: the columns centred in place on a copy, then the Gram / (m - 1)
    // (the engine's own upload and scratch shape: the same S, bit for bit)
    const int64_t ldw = round_up(n, 16);
    int64_t ldd = 0;
    double *D = nullptr, *W = nullptr;
    ADMM_TRY(upload_matrix(o->mem, &D, &ldd, desc->D, m, n, desc->ldD, ADMM_MEM_HOST, o->stream));
    ADMM_TRY(o->mem.alloc(&W, static_cast<size_t>(ldw) * n));
    covsel_cov(D, ldd, m, n, W, ldw, o->S, o->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
    o->mem.free_one(D);
    o->mem.free_one(W);
  }
  for (double** p : {&o->X, &o->Z, &o->U, &o->Y, &o->V}) {
    ADMM_TRY(o->mem.alloc(p, static_cast<size_t>(nn) * K));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * nn * K, o->stream));
  }
  ADMM_TRY(o->mem.alloc(&o->lam, static_cast<size_t>(K)));
  ADMM_TRY(o->mem.alloc(&o->rho, static_cast<size_t>(K)));
  ADMM_TRY(o->mem.alloc(&o->logpart, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->lam, desc->lambda, sizeof(double) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipMemsetAsync(o->logpart, 0, sizeof(double) * K, o->stream));
  ADMM_TRY(alloc_words(*o, &o->sweeps, static_cast<size_t>(K)));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  return covsel_multi_prepare();
}

}  // namespace

extern "C" {

void admm_covsel_multi_desc_default(admm_covsel_multi_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_covsel_multi_desc);
  d->K = 1;
}

void admm_covsel_multi_options_default(admm_covsel_multi_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_covsel_multi_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->nodualerror = 0;  // admm.m:76: both residuals (the dual one costs no product here)
}

int admm_covsel_multi_create(const admm_covsel_multi_desc* desc, admm_covsel_multi** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_covsel_multi_desc)))
    return fail(ADMM_E_INVALID, "admm_covsel_multi_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the multi covariance selection needs at least one fit (K >= 1)");
  if (desc->n < 1) return fail(ADMM_E_INVALID, "the multi covariance selection needs n >= 1 (S is n x n)");
  if ((desc->D != nullptr) == (desc->S != nullptr))
    return fail(ADMM_E_INVALID, "the multi covariance selection needs either the samples D (m x n) or S (n x n), "
                                "not both and not neither");
  if (desc->D && desc->m < 2)
    return fail(ADMM_E_INVALID, "the multi covariance selection: cov(D) needs at least two samples (m >= 2)");
  if (desc->D && desc->ldD < desc->m) return fail(ADMM_E_INVALID, "the multi covariance selection: ldD < m");
  if (!desc->lambda) return fail(ADMM_E_INVALID, "the multi covariance selection needs lambda (K values)");
  for (int32_t k = 0; k < desc->K; ++k)
    if (!finite_pos(desc->lambda[k]))
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": lambda is not positive and finite");
  if (desc->n > kCovselSmallMax)
    return fail(ADMM_E_UNSUPPORTED, "the multi covariance selection keeps a fit in one workgroup's LDS (n <= " +
                                        std::to_string(kCovselSmallMax) + ")" + kPerFit);
  if (desc->S) {  // the engine's rule (setup_covsel)
    double amax = 0.0, asym = 0.0;
    for (int64_t j = 0; j < desc->n; ++j)
      for (int64_t i = j; i < desc->n; ++i) {
        const double a = desc->S[i + j * desc->n], b = desc->S[j + i * desc->n];
        amax = std::max(amax, std::max(std::fabs(a), std::fabs(b)));
        asym = std::max(asym, std::fabs(a - b));
        if (!std::isfinite(a) || !std::isfinite(b)) asym = INFINITY;
      }
    if (!(asym <= 1e-12 * amax))
      return fail(ADMM_E_INVALID, "the multi covariance selection: S must be a finite symmetric matrix (|S - S'| <= "
                                  "1e-12 * max|S|)");
  }
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, std::string("the multi covariance selection is not row-sharded") + kPerFit);
  ADMM_TRY(check_placement("the multi covariance selection", nullptr, desc->device));
  return create_object(out, admm_covsel_multi_destroy, [&](admm_covsel_multi* o) { return cm_setup(o, desc); });
}

int admm_covsel_multi_run(admm_covsel_multi* o, const admm_covsel_multi_options* opts,
                          admm_covsel_multi_summary* summaries, double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_covsel_multi_options)))
    return fail(ADMM_E_INVALID, "admm_covsel_multi_options.struct_size mismatch (ABI version skew)");
  admm_covsel_multi_options op = *opts;
  ADMM_TRY(check_run_options("multi covariance selection", kPerFit, &op));
  const int32_t N = op.maxiters, K = o->K;
  std::vector<double> rh(static_cast<size_t>(K), op.rho);
  for (int32_t k = 0; k < K; ++k) {
    if (op.rhos) rh[k] = op.rhos[k];
    if (!finite_pos(rh[k])) return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": rho is not positive and finite");
  }
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const size_t nnK = static_cast<size_t>(o->n) * o->n * K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  ADMM_TRY(begin_run(*o));
  ADMM_HIP_TRY(hipMemcpyAsync(o->rho, rh.data(), sizeof(double) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipMemsetAsync(o->X, 0, sizeof(double) * nnK, o->stream));
  ADMM_HIP_TRY(hipMemsetAsync(o->sweeps, 0, sizeof(int32_t) * K, o->stream));
  for (auto [dst, src] : {std::pair<double*, const double*>{o->Z, op.z0}, {o->U, op.u0}}) {
    if (src) ADMM_HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * nnK, hipMemcpyHostToDevice, o->stream));
    else ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * nnK, o->stream));
  }
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (rh and the caller's starts were read)

  CovselMultiArgs ka{};
  ka.n = o->n;
  ka.K = K;
  ka.S = o->S;
  ka.lam = o->lam;
  ka.rho = o->rho;
  ka.X = o->X;
  ka.Z = o->Z;
  ka.U = o->U;
  ka.Y = o->Y;
  ka.V = o->V;
  ka.logpart = o->logpart;
  ka.sweeps = o->sweeps;
  ka.rec = o->rec;
  ka.pnorm = o->pnorm;
  ka.perr = o->perr;
  ka.dnorm = o->dnorm;
  ka.derr = o->derr;
  ka.objv = o->objv;
  ka.hist_ld = N;
  ka.maxiters = N;
  ka.abstol = op.abstol;
  ka.reltol = op.reltol;
  ka.domaxiters = op.domaxiters;
  ka.objevals = op.objevals;
  ka.dual = op.nodualerror == 0 ? 1 : 0;

  ADMM_TRY(begin_timing(*o));
  bool all = false;
  for (int32_t it = 0; it < N && !all; it += op.check_every) {  // a launch: up to check_every iterations of every fit
    ka.iters = std::min(op.check_every, N - it);
    launch_covsel_multi(ka, o->stream);
    ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the multi covariance selection loop ended with fits still running", N,
                      op.objevals != 0, o->objv, runtime_s, summaries));
  if (summaries) {
    std::vector<int32_t> sw(static_cast<size_t>(K));
    ADMM_HIP_TRY(hipMemcpy(sw.data(), o->sweeps, sizeof(int32_t) * K, hipMemcpyDeviceToHost));
    for (int32_t c = 0; c < K; ++c) summaries[c].jacobi_sweeps = sw[c];
  }
  o->last = op;
  o->last.rhos = o->last.z0 = o->last.u0 = nullptr;  // (the caller's arrays are not kept)
  o->has_run = true;
  return ADMM_OK;
}

int admm_covsel_multi_fetch(admm_covsel_multi* o, int field, double* dst, size_t cap, size_t* written) {
  if (o && dst && field == ADMM_CM_F_COV) {  // S as built: there from create on
    const size_t need = static_cast<size_t>(o->n) * o->n;
    if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    ADMM_HIP_TRY(hipSetDevice(o->device));
    ADMM_HIP_TRY(hipMemcpy(dst, o->S, sizeof(double) * need, hipMemcpyDeviceToHost));
    if (written) *written = need;
    return ADMM_OK;
  }
  ADMM_TRY(fetch_head(o, dst));
  const int64_t nn = o->n * o->n;
  switch (field) {
    case ADMM_CM_F_XOPT: return fetch_cols(*o, o->X, nn, nn, dst, cap, written);
    case ADMM_CM_F_ZOPT: return fetch_cols(*o, o->Z, nn, nn, dst, cap, written);
    case ADMM_CM_F_UOPT: return fetch_cols(*o, o->U, nn, nn, dst, cap, written);
    case ADMM_CM_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_CM_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_CM_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_CM_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_CM_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the multi covariance selection");
  }
}

void admm_covsel_multi_destroy(admm_covsel_multi* o) {
  if (!o) return;
  destroy_common(*o);
  if (o->stream) (void)hipStreamDestroy(o->stream);
  delete o;
}

}  // extern "C"
