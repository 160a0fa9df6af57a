// sparse_svm.hip -- the linear SVM for all one-vs-rest classes on a SPARSE design matrix.  The loop is
// svm_ovr.hip's: K independent plain-ADMM runs (unwrappedadmm.m:76-92: A = D, B = -1, c = 0, stopcond 'both',
// nodualerror 1) that share D; the one difference is the x-update.  x_c = D^+(z_c - u_c) is CG on D'D x = D'(z_c - u_c),
// no shift, nothing n x n: the first solve of a run starts from 0 and every later one from the previous x, so every
// iterate stays in range(D') and the limit is the pseudo-inverse solution (a column of D without nonzeros keeps x = 0.0).
// Per iteration, every launch for all K classes at once (blockIdx.y = chunk of kSpmmChunk classes):
//   Y = D' V                      one SpMM (spmm.hip)
//   SpmmCg::solve                 the lock-step CG of spmm_cg.hip: two SpMM and four small launches per inner iteration
//   AX = D X                     one SpMM
//   ssv_elem_kernel               the element update of every class -- prox_apply / loss_form_z, the code of the dense pass
//                                 -- its residual sums, and V = z - u
//   ssv_fin_kernel                per class pnorm, perr, Hnormsq, the objective and the stop decision (admm.m:612-722)
// A class whose stop flag is set is FROZEN, and a class whose solve is done is masked until the next solve: every kernel
// and every product skips it.  Every sum runs in a fixed order that depends on the sizes alone: two runs give the same
// bits, and a class gets the same numbers wherever it lands.
#include <cmath>
#include <cstddef>
#include <vector>

#include "multi_host.h"
#include "prox_device.h"
#include "sparse_svm.h"
#include "svm_cost_device.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// the ProxArgs of one class: plain ADMM, B = -1, c = 0, no histories -- the fields svm_ovr.hip's pass sets
__device__ __forceinline__ ProxArgs ssv_prox_args(const SsvElemArgs& a, double* z, double* u, const double* ell,
                                                  int32_t loss) {
  ProxArgs pa{};
  pa.len = a.m;
  pa.z = z;
  pa.u = u;
  pa.ell = ell;
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = (loss == ADMM_LOSS_01) ? PROX_01 : PROX_HINGE;    // getProxOps.m:1094
  pa.t = (loss == ADMM_LOSS_01) ? a.rho / a.C : a.C / a.rho;  // getProxOps.m:1100 | 1096
  pa.objx = !a.objevals ? OBJX_NONE : (loss == ADMM_LOSS_HINGE ? OBJX_HINGE : OBJX_ZEROONE);  // linearsvm.m:231-237
  if (loss == ADMM_LOSS_LOGISTIC) {
    pa.prox = PROX_LOGISTIC;
    pa.objx = a.objevals ? OBJX_LOGISTIC : OBJX_NONE;
  }
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;
  pa.rhs_kind = RHS_NONE;
  return pa;
}

// INIT: only V = z0 - u0, before the first iteration
template <bool INIT>
__global__ __launch_bounds__(kScgBlock) void ssv_elem_kernel(SsvElemArgs a) {
  __shared__ double lds[OV_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[S_COUNT];
#pragma unroll
  for (int q = 0; q < S_COUNT; ++q) acc[q] = 0.0;
  const int cl = l.run ? l.fit : 0;
  const int32_t loss = a.loss[cl];
  const bool cost = a.chunk_cost[blockIdx.y] != 0;
  // (z, u, ell addressed through the chunk base with the element's own index)
  ProxArgs pa = ssv_prox_args(a, a.Z + base, a.U + base, a.ELL + base, loss);
  const SvmCostArgs ks{nullptr, a.CC[2 * cl], a.CC[2 * cl + 1], a.C, a.rho, loss, a.objevals};
  if (cost) {  // z reaches prox_apply in a register; the objective's terms are summed beside it
    pa.prox = PROX_GIVEN;
    pa.objx = OBJX_NONE;
  }
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (!l.run || i >= a.m) continue;
    const int64_t e = i * KC + l.c;
    const double zp = pa.z[e], uo = pa.u[e];
    double t;
    if constexpr (INIT) {
      t = (0.0 + zp) - uo;  // (c + z0) - u0 with c = 0, as prox_apply forms it
    } else {
      const double ax = a.AX[base + e];
      ProxIn in{};
      in.zp = zp;
      in.u_old = uo;
      in.uhat_i = uo;
      in.ell_i = pa.ell[e];
      if (cost) {
        const double wv = a.W ? a.W[i] : 1.0;
        loss_form_z<true>(pa, ks, wv, ax, in, acc);
      }
      prox_apply<true>(pa, e, ax, 0, 0.0, in, acc, &t);
    }
    a.V[base + e] = t;
  }
  if (INIT) return;
  const double sums[OV_COUNT] = {acc[S_R2], acc[S_AX2], acc[S_Z2], acc[S_DZ2], acc[S_DU2], acc[S_OBJX]};
  scg_sums<OV_COUNT>(sums, lds, a.part, OV_COUNT, 0);
}

// blockIdx.x = class: the finalize logic of the class's iteration -- ovr_gsum_fin_kernel's (admm.m:612-722 for plain ADMM
// with nodualerror = 1 and stopcond = 'both'), with x read from the chunked layout
__global__ __launch_bounds__(kBlock) void ssv_fin_kernel(SsvFinArgs a) {
  const int cls = blockIdx.x;
  MultiRec* rec = a.rec + cls;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[8];
  __shared__ double sq[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  multi_slot_totals(a.part, cls, OV_COUNT, a.nwg, S);
  double xx = 0.0;
  if (a.objevals) {
    const double* __restrict__ x = a.X + static_cast<int64_t>(cls / KC) * a.n * KC + cls % KC;
    for (int64_t j = tid; j < a.n; j += kBlock) xx += x[j * KC] * x[j * KC];
  }
  xx = wave_sum(xx);
  if (lane == 0) sq[wid] = xx;
  __syncthreads();
  if (tid != 0) return;
  const double nx2 = ((sq[0] + sq[1]) + sq[2]) + sq[3];
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(cls) * a.hist_ld + it;
  const double hn = a.rho * S[OV_DZ2] + a.rho * (a.rho * a.rho) * S[OV_DU2];  // admm.m:305-306, w = [x; z; rho*u]
  a.hnorm[h] = hn;
  if (a.objevals) a.objv[h] = a.C * S[OV_OBJX] + 0.5 * nx2;  // linearsvm.m:231-237
  const double pn = sqrt(S[OV_R2]);  // admm.m:621
  const double pe = sqrt(static_cast<double>(a.m)) * a.abstol +
                    a.reltol * fmax(fmax(sqrt(S[OV_AX2]), sqrt(S[OV_Z2])), 0.0);  // admm.m:644-650, c = 0
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  bool stop = false;
  if (!a.domaxiters && pn < pe) stop = true;                     // admm.m:710-713, nodualerror
  if (!a.domaxiters && i1 > 2 && hn <= a.Hnormtol) stop = true;  // admm.m:719-722
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

}  // namespace

void launch_ssv_elem(const SsvElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(ssv_elem_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL(ssv_elem_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_ssv_fin(const SsvFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(ssv_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_svm : MultiHost {
  SpmmCg cg;  // D, the x-update and its multi-vectors
  int64_t m = 0, n = 0;
  int32_t nwg = 0;
  double C = 0.0;
  double *Z = nullptr, *U = nullptr, *ELL = nullptr, *V = nullptr;  // multi-vectors of len m
  double* part = nullptr;
  double *W = nullptr, *CC = nullptr;
  int32_t *loss = nullptr, *chunk_cost = nullptr;
  std::vector<int32_t> loss_host;
  std::vector<double> cost_host;
  double *pnorm = nullptr, *perr = nullptr, *hnorm = nullptr, *objv = nullptr;  // histories
  admm_sparse_svm_options last{};
};

namespace {

// svm_ovr.hip's rule: a chunk takes the cost form with weights, a class cost != 1 or the squared hinge
int ssv_plan_cost(admm_sparse_svm* o) {
  const std::vector<int32_t> cc = svm_cost_chunks(o->K, kSpmmChunk, o->W != nullptr, o->loss_host, o->cost_host);
  ADMM_HIP_TRY(hipMemcpyAsync(o->chunk_cost, cc.data(), sizeof(int32_t) * cc.size(), hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  return ADMM_OK;
}

int ssv_setup(admm_sparse_svm* o, const admm_sparse_svm_desc* desc) {
  const int32_t K = desc->K;
  o->K = K;
  ADMM_TRY(o->cg.build(o, desc->device, desc->D));
  const int64_t m = o->cg.m;
  o->m = m;
  o->n = o->cg.n;
  o->nwg = scg_vec_workgroups(m);
  o->C = desc->C;
  const size_t kp = static_cast<size_t>(o->cg.chunks) * kSpmmChunk;
  for (double** p : {&o->Z, &o->U, &o->ELL, &o->V}) {
    ADMM_TRY(o->mem.alloc(p, kp * m));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * m, o->stream));
  }
  ADMM_TRY(o->cg.upload(o->ELL, desc->ELL, m));
  ADMM_TRY(o->mem.alloc(&o->part, kp * OV_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * kp * OV_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(alloc_words(*o, &o->loss, static_cast<size_t>(K)));
  ADMM_TRY(alloc_words(*o, &o->chunk_cost, static_cast<size_t>(o->cg.chunks)));
  o->loss_host.assign(static_cast<size_t>(K), ADMM_LOSS_HINGE);
  if (desc->loss) o->loss_host.assign(desc->loss, desc->loss + K);
  ADMM_HIP_TRY(hipMemcpyAsync(o->loss, o->loss_host.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->cost_host.assign(static_cast<size_t>(2 * K), 1.0);
  ADMM_TRY(o->mem.alloc(&o->CC, static_cast<size_t>(2 * K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, o->cost_host.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(ssv_plan_cost(o));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  return ADMM_OK;
}

}  // namespace

extern "C" {

void admm_sparse_svm_desc_default(admm_sparse_svm_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_sparse_svm_desc);
  d->K = 1;
}

void admm_sparse_svm_options_default(admm_sparse_svm_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_sparse_svm_options);
  o->maxiters = 1000;  // unwrappedadmm.m:90
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->Hnormtol = 1e-6;  // admm.m:73
  o->relax = 1.0;      // admm.m:60
  o->cg_tol = 1e-12;   // admm_problem_desc_default
  o->cg_maxit = 200;
}

int admm_sparse_svm_chunk(void) { return kSpmmChunk; }

int admm_sparse_svm_create(const admm_sparse_svm_desc* desc, admm_sparse_svm** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_sparse_svm_desc)))
    return fail(ADMM_E_INVALID, "admm_sparse_svm_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the one-vs-rest linear SVM needs at least one class (K >= 1)");
  ADMM_TRY(check_sparse_D("the sparse linear SVM", desc->D));
  if (!desc->ELL) return fail(ADMM_E_INVALID, "the linear SVM needs the label matrix ELL (m x K)");
  if (!(desc->C >= 0.0) || !finite_nonneg(desc->C))
    return fail(ADMM_E_INVALID, "Given regularization parameter C is not a nonnegative number!");
  ADMM_TRY(check_svm_losses(desc->K, desc->loss));
  const int64_t mk = desc->D->rows * static_cast<int64_t>(desc->K);
  for (int64_t i = 0; i < mk; ++i)
    if (desc->ELL[i] != 1.0 && desc->ELL[i] != -1.0)
      return fail(ADMM_E_INVALID, "a label of class " + std::to_string(i / desc->D->rows) + " is neither +1 nor -1");
  ADMM_TRY(check_placement("the sparse one-vs-rest linear SVM", desc->comm, desc->device));
  return create_object(out, admm_sparse_svm_destroy, [&](admm_sparse_svm* o) { return ssv_setup(o, desc); });
}

int admm_sparse_svm_run(admm_sparse_svm* o, const admm_sparse_svm_options* opts, admm_sparse_svm_summary* summaries,
                        double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_svm_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_svm_options.struct_size mismatch (ABI version skew)");
  admm_sparse_svm_options op = *opts;
  ADMM_TRY(check_sparse_run_options("sparse one-vs-rest", &op));
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->hnorm, &o->objv}, N));
  ADMM_TRY(begin_run(*o));
  SpmmCg& cg = o->cg;
  ScgArgs ca{};
  ADMM_TRY(cg.begin_run(op.cg_tol, op.cg_maxit, &ca));
  ADMM_TRY(cg.upload(o->Z, op.z0, o->m));
  ADMM_TRY(cg.upload(o->U, op.u0, o->m));

  SsvElemArgs ea{};
  ea.m = o->m;
  ea.AX = cg.T;
  ea.Z = o->Z;
  ea.U = o->U;
  ea.ELL = o->ELL;
  ea.V = o->V;
  ea.W = o->W;
  ea.CC = o->CC;
  ea.loss = o->loss;
  ea.chunk_cost = o->chunk_cost;
  ea.rec = o->rec;
  ea.part = o->part;
  ea.K = K;
  ea.objevals = op.objevals;
  ea.rho = op.rho;
  ea.C = o->C;
  SsvFinArgs fa{};
  fa.part = o->part;
  fa.X = cg.X;
  fa.n = o->n;
  fa.m = o->m;
  fa.K = K;
  fa.nwg = o->nwg;
  fa.rec = o->rec;
  fa.pnorm = o->pnorm;
  fa.perr = o->perr;
  fa.hnorm = o->hnorm;
  fa.objv = o->objv;
  fa.hist_ld = N;
  fa.rho = op.rho;
  fa.C = o->C;
  fa.abstol = op.abstol;
  fa.reltol = op.reltol;
  fa.Hnormtol = op.Hnormtol;
  fa.domaxiters = op.domaxiters;
  fa.objevals = op.objevals;
  fa.maxiters = N;
  const SpmmMask run = cg.mask(false);

  ADMM_TRY(begin_timing(*o));
  launch_ssv_elem(ea, true, o->stream);  // V = z0 - u0
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    launch_spmm(cg.sp.t, o->V, cg.Y, cg.chunks, run, o->stream);  // y = D'(z - u)
    ADMM_TRY(cg.solve(ca, it == 0));
    launch_spmm(cg.sp.n, cg.X, cg.T, cg.chunks, run, o->stream);  // D x
    launch_ssv_elem(ea, false, o->stream);
    launch_ssv_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the sparse one-vs-rest loop ended with classes still running", N, op.objevals != 0,
                      o->objv, runtime_s, summaries));
  return end_sparse_run(o, op, summaries);
}

int admm_sparse_svm_set_cost(admm_sparse_svm* o, const double* weights, const double* class_cost) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  ADMM_TRY(set_svm_cost(*o, o->m, weights, class_cost, &o->W, o->CC, &o->cost_host));
  return ssv_plan_cost(o);
}

int admm_sparse_svm_fetch(admm_sparse_svm* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_OVR_F_XOPT: return o->cg.fetch_matrix(o->cg.X, o->n, dst, cap, written);
    case ADMM_OVR_F_ZOPT: return o->cg.fetch_matrix(o->Z, o->m, dst, cap, written);
    case ADMM_OVR_F_UOPT: return o->cg.fetch_matrix(o->U, o->m, dst, cap, written);
    case ADMM_OVR_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_OVR_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_OVR_F_HNORMSQ: return fetch_history(*o, o->hnorm, dst, cap, written);
    case ADMM_OVR_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse one-vs-rest linear SVM");
  }
}

void admm_sparse_svm_destroy(admm_sparse_svm* o) { destroy_sparse(o); }

}  // extern "C"
