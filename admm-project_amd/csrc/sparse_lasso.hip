// sparse_lasso.hip -- the lasso on a SPARSE design matrix, K fits at once: a regularisation path, a
// cross-validation grid or several response columns over one D.  K independent plain-ADMM runs as lasso.m:227-239 poses
// them (A = 1, B = -1, c = 0, sizes n, stopcond 'standard') that share D, rho and the l1 weights w and differ in
// (lambda_k, mu_k, nonneg_k) and optionally in their column of S:
//   g_k(z) = lambda_k*sum_i w_i*|z_i| + mu_k/2*||z||^2 + [z >= 0],  z = kappa_k*penalty_elem(x + u, tau_k*w_i, nonneg_k),
//   tau_k = lambda_k/rho, kappa_k = rho/(rho + mu_k)          (q32's family without groups: penalty_device.h)
// With groups set (admm_sparse_lasso_set_groups, q41) the element kernel is group_multi.hip's slm_group_elem_kernel.
// With observations set (admm_sparse_lasso_set_observations, q46) fit k weighs row i by omega_ik = obsw_i * [fold_i !=
// held_k]: the CG's forward product stores omega_k o (D p) (SpmmCg::weighted), D's becomes the K-column D'(Omega_k s_k),
// slm_fit_weighted_kernel sums the weighted fit term and, behind the loop at T = D z, the held-out error and weight.
// The x-update (D'D + rho*I) x = D's_k + rho*(z - u) (lasso.m:28-30) is spmm_cg.hip's lock-step CG with the shift rho:
// the first solve of a run starts from 0 and every later one from the previous x.
// Per iteration, every launch for all K fits at once (blockIdx.y = chunk of kSpmmChunk fits):
//   SpmmCg::solve                 two SpMM and four small launches per inner iteration
//   slm_elem_kernel               over n: z in a register, prox_apply (the code of the dense engine's element update) for
//                                 u, the residual sums and the next right-hand side rho*(z - u) + D's; g_k(z)
//   (objevals = 1)                T = D X, one SpMM, and slm_fit_kernel over m: sum (D x - s_k)^2
//   slm_fin_kernel                per fit pnorm, perr, dnorm, derr, the objective and the stop decision (admm.m:612-713)
// The dual residual rho*||z - zprev|| needs no product (A = 1), so the reference's stop rule is the default.
// A fit whose stop flag is set is FROZEN, and a fit whose solve is done is masked until the next solve: every kernel and
// every product skips it.  Every sum runs in a fixed order that depends on the sizes alone: two runs give the same bits,
// and a fit gets the same numbers wherever it lands.  No atomics.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "group_multi.h"
#include "multi_host.h"
#include "penalty_device.h"
#include "sparse_lasso.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// INIT: only Y = rho*(z0 - u0) + D's, before the first iteration
template <bool INIT>
__global__ __launch_bounds__(kScgBlock) void slm_elem_kernel(SlmElemArgs a) {
  __shared__ double lds[SL_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[S_COUNT];
#pragma unroll
  for (int q = 0; q < S_COUNT; ++q) acc[q] = 0.0;
  double obj = 0.0;
  const int fit = l.run ? l.fit : 0;
  const double lam = a.par[2 * fit], mu = a.par[2 * fit + 1];
  // engine_run_general.hip's own expressions for the family's numbers
  const PenaltyArgs pen{a.W, lam / a.rho, a.rho / (a.rho + mu), lam, 0.0, 0.5 * mu, a.nonneg[fit]};
  // plain ADMM, A = 1, B = -1, c = 0, z given in a register, no histories; z, u and the next right-hand side addressed
  // through the chunk base with the element's own index
  ProxArgs pa{};
  pa.len = a.n;
  pa.z = a.Z + base;
  pa.u = a.U + base;
  pa.c = nullptr;
  pa.rhs = a.Y + base;
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = PROX_GIVEN;
  pa.objx = OBJX_NONE;
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;  // (x is where the solve left it)
  pa.rhs_kind = RHS_RHO_DTS;
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (!l.run || i >= a.n) continue;
    const int64_t e = i * KC + l.c;
    const double zp = pa.z[e], uo = pa.u[e];
    const double dts = (a.dts_ns == 1) ? a.DTS[i * KC] : a.DTS[base + e];
    if constexpr (INIT) {
      pa.rhs[e] = rhs_value(RHS_RHO_DTS, a.rho, zp, uo, 0.0, dts);
    } else {
      const double xv = a.X[base + e];
      const double wi = penalty_weight(pen, i);
      ProxIn in{};
      in.zp = zp;
      in.u_old = uo;
      in.uhat_i = uo;
      in.add_i = dts;
      in.zg_i = pen.kappa * penalty_elem(group_prox_v(pa, xv, in), pen.tau * wi, pen.nonneg);
      if (a.objevals) obj += penalty_obj_elem(pen, wi, in.zg_i);
      prox_apply<false>(pa, e, xv, 0, 0.0, in, acc);
    }
  }
  if (INIT) return;
  const double sums[SL_COUNT] = {acc[S_R2], acc[S_AX2], acc[S_Z2], acc[S_DZ2], acc[S_U2], obj};
  scg_sums<SL_COUNT>(sums, lds, a.part, SL_COUNT, 0);
}

// per fit the partial sums over m of (D x - s_k)^2
__global__ __launch_bounds__(kScgBlock) void slm_fit_kernel(SlmFitArgs a) {
  __shared__ double lds[kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[1] = {0.0};
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (l.run && i < a.m) {
      const int64_t e = base + i * KC + l.c;
      const double sv = (a.ns == 1) ? a.S[i * KC] : a.S[e];
      const double d = a.T[e] - sv;
      acc[0] += d * d;
    }
  }
  scg_sums<1>(acc, lds, a.part, 1, 0);
}

// the weighted form (observations set, q46): three sums per fit over m (SlmFitSlot).  Every weight is a select on the
// fold, never a product with 0; a.all: every fit, stopped or not
__global__ __launch_bounds__(kScgBlock) void slm_fit_weighted_kernel(SlmFitArgs a) {
  __shared__ double lds[SLW_COUNT * kScgBlock];
  ScgLane l = scg_lane(a.rec, a.K);
  if (a.all) l.run = l.fit < a.K;
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  const int32_t hk = a.held[l.run ? l.fit : 0];
  double acc[SLW_COUNT] = {0.0, 0.0, 0.0};
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (l.run && i < a.m) {
      const int64_t e = base + i * KC + l.c;
      const double sv = (a.ns == 1) ? a.S[i * KC] : a.S[e];
      const double d = a.T[e] - sv;
      const double w = a.obsw ? a.obsw[i] : 1.0;
      const bool out = a.fold && a.fold[i] == hk;
      const double wd2 = w * (d * d);
      acc[SLW_FIT] += out ? 0.0 : wd2;
      acc[SLW_HELD_SSE] += out ? wd2 : 0.0;
      acc[SLW_HELD_W] += out ? w : 0.0;
    }
  }
  scg_sums<SLW_COUNT>(acc, lds, a.part, SLW_COUNT, 0);
}

// T(:, k) = omega_k o s_k for every fit (the columns past K stay as they are: +0.0)
__global__ __launch_bounds__(kScgBlock) void slm_obs_rhs_kernel(SlmObsRhsArgs a) {
  const int c = threadIdx.x % KC, r = threadIdx.x / KC;
  const int fit = static_cast<int>(blockIdx.y) * KC + c;
  if (fit >= a.K) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  const int32_t hk = a.held[fit];
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + r;
    if (i >= a.m) continue;
    const int64_t e = base + i * KC + c;
    const double sv = (a.ns == 1) ? a.S[i * KC] : a.S[e];
    const bool out = a.fold && a.fold[i] == hk;
    a.T[e] = out ? 0.0 : (a.obsw ? sv * a.obsw[i] : sv);
  }
}

// blockIdx.x = fit: the two held-out totals in multi_slot_totals' order
__global__ __launch_bounds__(kBlock) void slm_heldout_kernel(const double* part, int32_t nwg_m, double* heldout) {
  __shared__ double S[8];
  const int fit = blockIdx.x;
  multi_slot_totals(part, fit, SLW_COUNT, nwg_m, S);
  __syncthreads();
  if (threadIdx.x == 0) {
    heldout[2 * fit] = S[SLW_HELD_SSE];
    heldout[2 * fit + 1] = S[SLW_HELD_W];
  }
}

// blockIdx.x = fit: the finalize logic of the fit's iteration -- admm.m:612-658, 706-713 as oracle/admm_ref.py restates
// it for A = 1, B = -1, c = 0, plain ADMM with stopcond = 'standard'; the dual residual takes part when a.dual is set
__global__ __launch_bounds__(kBlock) void slm_fin_kernel(SlmFinArgs a) {
  const int fit = blockIdx.x;
  MultiRec* rec = a.rec + fit;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[8];
  const int tid = threadIdx.x;
  multi_slot_totals(a.part, fit, SL_COUNT, a.nwg_n, S);
  // (fit_slots = SLW_COUNT: the 32-lane groups 6 and 7 total the slots 0 and 1 into S[6] and S[7]; S[SL_COUNT] is read)
  if (a.objevals) multi_slot_totals(a.fpart, fit, a.fit_slots, a.nwg_m, S, SL_COUNT);
  __syncthreads();
  if (tid != 0) return;
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(fit) * a.hist_ld + it;
  if (a.objevals) a.objv[h] = 0.5 * S[SL_COUNT] + S[SL_OBJ];  // lasso.m:227 with the family's g_k(z)
  const double sqn = sqrt(static_cast<double>(a.n));
  const double pn = sqrt(S[SL_R2]);                                                        // admm.m:621
  const double pe = sqn * a.abstol + a.reltol * fmax(sqrt(S[SL_X2]), sqrt(S[SL_Z2]));     // admm.m:644-650, c = 0
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  bool dual_ok = true;
  if (a.dual) {
    const double dn = a.rho * sqrt(S[SL_DZ2]);                                   // admm.m:624, A = 1
    const double de = sqn * a.abstol + a.reltol * (a.rho * sqrt(S[SL_U2]));      // admm.m:652-654
    a.dnorm[h] = dn;
    a.derr[h] = de;
    dual_ok = dn < de;
  }
  const bool stop = !a.domaxiters && pn < pe && dual_ok;  // admm.m:710-713
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

}  // namespace

void launch_slm_elem(const SlmElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.n), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(slm_elem_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL(slm_elem_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_slm_fit(const SlmFitArgs& a, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(slm_fit_kernel, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_slm_fit_weighted(const SlmFitArgs& a, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(slm_fit_weighted_kernel, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_slm_obs_rhs(const SlmObsRhsArgs& a, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(slm_obs_rhs_kernel, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_slm_heldout(const double* part, int32_t K, int32_t nwg_m, double* heldout, hipStream_t stream) {
  hipLaunchKernelGGL(slm_heldout_kernel, dim3(static_cast<unsigned>(K)), dim3(kBlock), 0, stream, part, nwg_m, heldout);
}

void launch_slm_fin(const SlmFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(slm_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_lasso : MultiHost {
  SpmmCg cg;  // D, the x-update and its multi-vectors
  int64_t m = 0, n = 0;
  int32_t ns = 1, nwg_n = 0, nwg_m = 0;
  double *Z = nullptr, *U = nullptr;  // multi-vectors of len n
  double* S = nullptr;                // ns == 1: ONE chunk of len m, column 0; ns == K: a multi-vector of len m
  double* DTS = nullptr;              // D'S in the layout of S, len n
  double *part = nullptr, *fpart = nullptr;
  double *W = nullptr, *par = nullptr;
  int32_t* nonneg = nullptr;
  GroupMulti grp;  // admm_sparse_lasso_set_groups (q41)
  // admm_sparse_lasso_set_observations (q46); all null: the unweighted object
  bool obs = false;
  double* obsw = nullptr;     // m observation weights or null
  int32_t* fold = nullptr;    // m fold ids or null
  int32_t* held = nullptr;    // K values (-1: nothing held out)
  double* DTSK = nullptr;     // D'(Omega_k s_k), a multi-vector of len n
  double* wpart = nullptr;    // the weighted fit pass's partials, SLW_COUNT per fit
  double* held_dev = nullptr; // K x 2: the held-out error and weight of the last run
  std::vector<double> held_sse, held_w;  // the same on the host; empty: no run under observations behind the object
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  admm_sparse_lasso_options last{};
};

namespace {

using namespace admm;

const char* kWho = "the sparse multi-lasso";

int slm_setup(admm_sparse_lasso* o, const admm_sparse_lasso_desc* desc, const std::vector<double>& ph,
              const std::vector<int32_t>& nh) {
  const int32_t K = desc->K;
  o->K = K;
  ADMM_TRY(o->cg.build(o, desc->device, desc->D));
  const int64_t m = o->cg.m, n = o->cg.n;
  o->m = m;
  o->n = n;
  o->ns = desc->ns;
  o->nwg_n = scg_vec_workgroups(n);
  o->nwg_m = scg_vec_workgroups(m);
  const size_t kp = static_cast<size_t>(o->cg.chunks) * kSpmmChunk;
  for (double** p : {&o->Z, &o->U}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  {  // S in the layout of the products and D'S, once: the shared response is column 0 of one chunk
    const int32_t sch = o->ns == 1 ? 1 : o->cg.chunks;
    const size_t sp = static_cast<size_t>(sch) * kSpmmChunk;
    ADMM_TRY(o->mem.alloc(&o->S, sp * m));
    ADMM_TRY(o->mem.alloc(&o->DTS, sp * n));
    ADMM_HIP_TRY(hipMemsetAsync(o->DTS, 0, sizeof(double) * sp * n, o->stream));
    std::vector<double> hb(sp * m);
    spmm_pack(desc->S, m, m, o->ns, hb.data());
    ADMM_HIP_TRY(hipMemcpyAsync(o->S, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, o->stream));
    SpmmMask all;
    all.K = o->ns;
    launch_spmm(o->cg.sp.t, o->S, o->DTS, sch, all, o->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hb goes out of scope)
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

}  // namespace

extern "C" {

void admm_sparse_lasso_desc_default(admm_sparse_lasso_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_sparse_lasso_desc);
  d->K = 1;
  d->ns = 1;
}

void admm_sparse_lasso_options_default(admm_sparse_lasso_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_sparse_lasso_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->cg_tol = 1e-12;   // admm_problem_desc_default
  o->cg_maxit = 200;
  o->nodualerror = 0;  // admm.m:76: the reference lasso's stop rule (the dual residual costs no product here)
}

int admm_sparse_lasso_chunk(void) { return kSpmmChunk; }

int admm_sparse_lasso_create(const admm_sparse_lasso_desc* desc, admm_sparse_lasso** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_sparse_lasso_desc)))
    return fail(ADMM_E_INVALID, "admm_sparse_lasso_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the sparse multi-lasso needs at least one fit (K >= 1)");
  ADMM_TRY(check_sparse_D(kWho, desc->D));
  if (!desc->S) return fail(ADMM_E_INVALID, "the sparse multi-lasso needs the responses S (rows x ns)");
  ADMM_TRY(check_response_columns(desc->ns, desc->K));
  if (!desc->lambda) return fail(ADMM_E_INVALID, "the sparse multi-lasso needs lambda (K values)");
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
    for (int64_t i = 0; i < desc->D->cols; ++i)
      if (!finite_nonneg(desc->weights[i]))
        return fail(ADMM_E_INVALID, "penalty: weight " + std::to_string(i) + " is negative or not finite");
  ADMM_TRY(check_placement(kWho, desc->comm, desc->device));
  return create_object(out, admm_sparse_lasso_destroy, [&](admm_sparse_lasso* o) { return slm_setup(o, desc, ph, nh); });
}

int admm_sparse_lasso_run(admm_sparse_lasso* o, const admm_sparse_lasso_options* opts,
                          admm_sparse_lasso_summary* summaries, double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_lasso_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_lasso_options.struct_size mismatch (ABI version skew)");
  admm_sparse_lasso_options op = *opts;
  ADMM_TRY(check_sparse_run_options("sparse multi-lasso", &op));
  const bool dual = op.nodualerror == 0;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  SpmmCg& cg = o->cg;
  ADMM_TRY(begin_run(*o));
  ScgArgs ca{};
  ADMM_TRY(cg.begin_run(op.cg_tol, op.cg_maxit, &ca, op.rho));
  ADMM_TRY(cg.upload(o->Z, op.z0, o->n));
  ADMM_TRY(cg.upload(o->U, op.u0, o->n));

  SlmElemArgs ea{};
  ea.n = o->n;
  ea.X = cg.X;
  ea.Z = o->Z;
  ea.U = o->U;
  ea.Y = cg.Y;
  ea.DTS = o->obs ? o->DTSK : o->DTS;
  ea.W = o->W;
  ea.par = o->par;
  ea.nonneg = o->nonneg;
  ea.rec = o->rec;
  ea.part = o->part;
  ea.K = K;
  ea.ns = o->ns;
  ea.dts_ns = o->obs ? K : o->ns;
  ea.objevals = op.objevals;
  ea.rho = op.rho;
  SlmFitArgs ta{};
  ta.m = o->m;
  ta.T = cg.T;
  ta.S = o->S;
  ta.rec = o->rec;
  ta.part = o->fpart;
  ta.K = K;
  ta.ns = o->ns;
  if (o->obs) {  // the weighted fit pass and its own partials
    ta.part = o->wpart;
    ta.obsw = o->obsw;
    ta.fold = o->fold;
    ta.held = o->held;
  }
  SlmFinArgs fa{};
  fa.part = o->part;
  fa.fpart = o->obs ? o->wpart : o->fpart;
  fa.fit_slots = o->obs ? SLW_COUNT : 1;
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
  fa.maxiters = N;
  const SpmmMask run = cg.mask(false);

  ADMM_TRY(begin_timing(*o));
  launch_slm_elem(ea, true, o->stream);  // y = rho*(z0 - u0) + D's
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    ADMM_TRY(cg.solve(ca, it == 0));
    if (o->grp.on()) launch_slm_group_elem(ea, o->grp, o->stream);
    else launch_slm_elem(ea, false, o->stream);
    if (op.objevals) {
      launch_spmm(cg.sp.n, cg.X, cg.T, cg.chunks, run, o->stream);  // D x
      if (o->obs) launch_slm_fit_weighted(ta, o->stream);
      else launch_slm_fit(ta, o->stream);
    }
    launch_slm_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  o->held_sse.clear();
  o->held_w.clear();
  if (o->obs && all) {  // T = D z for every fit, stopped or not (z: the sparse iterate df counts), and the held-out sums
    SpmmMask every;
    every.K = K;
    launch_spmm(cg.sp.n, o->Z, cg.T, cg.chunks, every, o->stream);
    ta.all = 1;
    launch_slm_fit_weighted(ta, o->stream);
    launch_slm_heldout(o->wpart, K, o->nwg_m, o->held_dev, o->stream);
  }
  ADMM_TRY(finish_run(*o, all, "the sparse multi-lasso loop ended with fits still running", N, op.objevals != 0, o->objv,
                      runtime_s, summaries));
  if (o->obs) {
    std::vector<double> hb(static_cast<size_t>(2) * K);
    ADMM_HIP_TRY(hipMemcpy(hb.data(), o->held_dev, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
    o->held_sse.resize(static_cast<size_t>(K));
    o->held_w.resize(static_cast<size_t>(K));
    for (int32_t k = 0; k < K; ++k) {
      o->held_sse[k] = hb[2 * k];
      o->held_w[k] = hb[2 * k + 1];
    }
  }
  return end_sparse_run(o, op, summaries);
}

int admm_sparse_lasso_set_observations(admm_sparse_lasso* o, const double* obsweights, int32_t nfolds, const int32_t* fold,
                                       const int32_t* heldout) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  const int64_t m = o->m, n = o->n;
  const int32_t K = o->K;
  ADMM_TRY(check_observations(m, K, obsweights, nfolds, fold, heldout));  // (a refused call changes nothing)
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const bool on = obsweights || fold;
  double* w = nullptr;
  int32_t *f = nullptr, *hd = nullptr;
  if (on) {
    const size_t kp = static_cast<size_t>(o->cg.chunks) * kSpmmChunk;
    if (!o->DTSK) {  // what every weighted object needs, once
      ADMM_TRY(o->mem.alloc(&o->DTSK, kp * n));
      ADMM_HIP_TRY(hipMemsetAsync(o->DTSK, 0, sizeof(double) * kp * n, o->stream));
      ADMM_TRY(o->mem.alloc(&o->wpart, kp * SLW_COUNT * kScgMaxWg));
      ADMM_HIP_TRY(hipMemsetAsync(o->wpart, 0, sizeof(double) * kp * SLW_COUNT * kScgMaxWg, o->stream));
      ADMM_TRY(o->mem.alloc(&o->held_dev, static_cast<size_t>(2) * K));
    }
    std::vector<int32_t> hh(static_cast<size_t>(K), -1);
    for (int32_t k = 0; heldout && k < K; ++k) hh[k] = heldout[k];
    ADMM_TRY(alloc_words(*o, &hd, static_cast<size_t>(K)));
    ADMM_HIP_TRY(hipMemcpyAsync(hd, hh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
    if (fold) {
      ADMM_TRY(alloc_words(*o, &f, static_cast<size_t>(m)));
      ADMM_HIP_TRY(hipMemcpyAsync(f, fold, sizeof(int32_t) * m, hipMemcpyHostToDevice, o->stream));
    }
    if (obsweights) {
      ADMM_TRY(o->mem.alloc(&w, static_cast<size_t>(m)));
      ADMM_HIP_TRY(hipMemcpyAsync(w, obsweights, sizeof(double) * m, hipMemcpyHostToDevice, o->stream));
    }
    // D'(Omega_k s_k) per fit: T = omega_k o s_k, one transposed product over all K fits
    const SlmObsRhsArgs ra{m, o->S, o->cg.T, w, f, hd, K, o->ns};
    launch_slm_obs_rhs(ra, o->stream);
    SpmmMask every;
    every.K = K;
    launch_spmm(o->cg.sp.t, o->cg.T, o->DTSK, o->cg.chunks, every, o->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hh and the caller's buffers were read)
    ADMM_HIP_TRY(hipGetLastError());
  }
  for (void* p : {static_cast<void*>(o->obsw), static_cast<void*>(o->fold), static_cast<void*>(o->held)})
    o->mem.free_one(p);
  o->obsw = w;
  o->fold = f;
  o->held = hd;
  o->obs = on;
  o->cg.weighted = on;
  o->cg.roww = SpmmRowWeights{w, f, hd, K};
  o->held_sse.clear();
  o->held_w.clear();
  return ADMM_OK;
}

int admm_sparse_lasso_heldout(admm_sparse_lasso* o, double* sse, double* weight) {
  if (!o || !sse || !weight) return fail(ADMM_E_INVALID, "object, sse or weight is NULL");
  if (!o->has_run || o->held_sse.empty())
    return fail(ADMM_E_INVALID, "the held-out sums need a run with observations set (admm_sparse_lasso_set_observations)");
  std::memcpy(sse, o->held_sse.data(), sizeof(double) * o->K);
  std::memcpy(weight, o->held_w.data(), sizeof(double) * o->K);
  return ADMM_OK;
}

int admm_sparse_lasso_set_weights(admm_sparse_lasso* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_shared_weights(*o, o->n, weights, &o->W);
}

int admm_sparse_lasso_set_groups(admm_sparse_lasso* o, int32_t G, const int64_t* sizes, const double* groupweights,
                                 const double* l1) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_multi_groups(*o, o->n, G, sizes, groupweights, l1, &o->grp);
}

int admm_sparse_lasso_fetch(admm_sparse_lasso* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_SLM_F_XOPT: return o->cg.fetch_matrix(o->cg.X, o->n, dst, cap, written);
    case ADMM_SLM_F_ZOPT: return o->cg.fetch_matrix(o->Z, o->n, dst, cap, written);
    case ADMM_SLM_F_UOPT: return o->cg.fetch_matrix(o->U, o->n, dst, cap, written);
    case ADMM_SLM_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_SLM_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_SLM_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_SLM_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_SLM_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse multi-lasso");
  }
}

void admm_sparse_lasso_destroy(admm_sparse_lasso* o) { destroy_sparse(o); }

}  // extern "C"
