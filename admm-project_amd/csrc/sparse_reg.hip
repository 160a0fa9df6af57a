// sparse_reg.hip -- quantile / LAD / Huber regression, K fits at once on a SPARSE design matrix.  The loop
// is reg_multi.hip's: K independent plain-ADMM runs (admm.m:496-743: A = D, B = -1, c = s_k, stopcond 'standard') that
// share D; the loss and its parameters sit in the element-wise z-prox (loss_device.h: loss_prox_elem) and the objective
// alone.  The x-update is spmm_cg.hip's: x_k = (D'D)^-1 D'(s_k + z_k - u_k) (getProxOps.m:1511-1515) as CG on
// D'D x = D'(s_k + z_k - u_k), no shift, nothing n x n: the first solve of a run starts from 0 and every later one from
// the previous x, so every iterate stays in range(D') -- with full column rank the reference's solution, otherwise the
// minimum-norm one (a column of D without nonzeros keeps x = 0.0; lad.m:134 would fail in chol there).
// Per iteration, every launch for all K fits at once (blockIdx.y = chunk of kSpmmChunk fits):
//   Y = D' V                      one SpMM (spmm.hip); V = (s + z) - u, left behind by the element pass
//   SpmmCg::solve                 the lock-step CG of spmm_cg.hip: two SpMM and four small launches per inner iteration
//   AX = D X                      one SpMM
//   srg_elem_kernel               the element update of every fit -- loss_form_z / prox_apply, the code of the dense pass
//                                 -- its residual sums, V, and z - zprev when the dual residual is on
//   (nodualerror = 0)             D'(z - zprev) and D'u, two SpMM, and srg_dual_kernel: their squared norms per fit
//   srg_fin_kernel                per fit pnorm, perr, dnorm, derr, the objective and the stop decision (admm.m:612-713)
// A fit whose stop flag is set is FROZEN, and a fit whose solve is done is masked until the next solve: every kernel and
// every product skips it.  Every sum runs in a fixed order that depends on the sizes alone: two runs give the same bits,
// and a fit gets the same numbers wherever it lands.  No atomics.
#include <cmath>
#include <cstddef>
#include <vector>

#include "loss_device.h"
#include "multi_host.h"
#include "reg_multi.h"
#include "sparse_reg.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// INIT: only V = (s + z0) - u0, before the first iteration
template <bool INIT>
__global__ __launch_bounds__(kScgBlock) void srg_elem_kernel(SrgElemArgs a) {
  __shared__ double lds[SR_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[S_COUNT];
#pragma unroll
  for (int q = 0; q < S_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const double* __restrict__ pp = a.par + 4 * fit;
  const LossArgs ls{nullptr, pp[0], pp[1], pp[2], pp[3], a.rho, a.kind[fit], a.objevals};  // (the weight: wv below)
  // plain ADMM, B = -1, c = s_k, z given in a register, no histories; z, u, dz and the next right-hand side addressed
  // through the chunk base with the element's own index
  ProxArgs pa{};
  pa.len = a.m;
  pa.z = a.Z + base;
  pa.u = a.U + base;
  pa.c = a.S;  // (non-null: c_i arrives in ProxIn)
  pa.dz = a.DZ ? a.DZ + base : nullptr;
  pa.rhs = a.V + base;
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = PROX_GIVEN;
  pa.objx = OBJX_NONE;
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;
  pa.rhs_kind = RHS_T1;
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (!l.run || i >= a.m) continue;
    const int64_t e = i * KC + l.c;
    const double zp = pa.z[e], uo = pa.u[e];
    const double sv = (a.ns == 1) ? a.S[i] : a.S[base + e];
    if constexpr (INIT) {
      pa.rhs[e] = (sv + zp) - uo;  // (c + z0) - u0, as prox_apply forms it for RHS_T1
    } else {
      const double ax = a.AX[base + e];
      const double wv = a.W ? a.W[i] : 1.0;
      ProxIn in{};
      in.zp = zp;
      in.u_old = uo;
      in.uhat_i = uo;
      in.c_i = sv;
      loss_form_z(pa, ls, wv, ax, in, acc);  // z = prox of the fit's loss at (ax + u) - s
      prox_apply<false>(pa, e, ax, 0, 0.0, in, acc);
    }
  }
  if (INIT) return;
  const double sums[SR_COUNT] = {acc[S_R2], acc[S_AX2], acc[S_Z2], acc[S_OBJZ]};
  scg_sums<SR_COUNT>(sums, lds, a.part, SR_COUNT, 0);
}

// per fit the partial squared norms over n of D'(z - zprev) and D'u
__global__ __launch_bounds__(kScgBlock) void srg_dual_kernel(SrgDualArgs a) {
  __shared__ double lds[SD_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[SD_COUNT] = {0.0, 0.0};
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (l.run && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      const double g = a.GDZ[e], h = a.GU[e];
      acc[SD_DZ2] += g * g;
      acc[SD_U2] += h * h;
    }
  }
  scg_sums<SD_COUNT>(acc, lds, a.part, SD_COUNT, 0);
}

// blockIdx.x = fit: the finalize logic of the fit's iteration -- admm.m:612-658, 706-713 as oracle/admm_ref.py restates
// it, for plain ADMM with stopcond = 'standard'; the dual residual takes part when a.dual is set
__global__ __launch_bounds__(kBlock) void srg_fin_kernel(SrgFinArgs a) {
  const int fit = blockIdx.x;
  MultiRec* rec = a.rec + fit;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[8];
  const int tid = threadIdx.x;
  multi_slot_totals(a.part, fit, SR_COUNT, a.nwg, S);
  if (a.dual) multi_slot_totals(a.dpart, fit, SD_COUNT, a.nwg_n, S, SR_COUNT);
  __syncthreads();
  if (tid != 0) return;
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(fit) * a.hist_ld + it;
  if (a.objevals) a.objv[h] = S[SR_OBJ];  // lad.m:148 / huberfit.m:180 with the family inside: sum_i w_i*phi(z_i)
  const double sqm = sqrt(static_cast<double>(a.m));
  const double pn = sqrt(S[SR_R2]);  // admm.m:621
  const double pe = sqm * a.abstol + a.reltol * fmax(fmax(sqrt(S[SR_AX2]), sqrt(S[SR_Z2])), a.snorm[fit]);  // admm.m:644-650
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  bool dual_ok = true;
  if (a.dual) {
    const double dn = a.rho * sqrt(S[SR_COUNT + SD_DZ2]);                           // admm.m:624
    const double de = sqm * a.abstol + a.reltol * (a.rho * sqrt(S[SR_COUNT + SD_U2]));  // admm.m:652-654, M2 = m
    a.dnorm[h] = dn;
    a.derr[h] = de;
    dual_ok = dn < de;
  }
  const bool stop = !a.domaxiters && pn < pe && dual_ok;  // admm.m:710-713
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

}  // namespace

void launch_srg_elem(const SrgElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(srg_elem_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL(srg_elem_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_srg_dual(const SrgDualArgs& a, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.n), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(srg_dual_kernel, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_srg_fin(const SrgFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(srg_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_reg : MultiHost {
  SpmmCg cg;  // D, the x-update and its multi-vectors (between two solves R and P hold D'(z - zprev) and D'u)
  int64_t m = 0, n = 0;
  int32_t ns = 1, nwg = 0, nwg_n = 0;
  double *Z = nullptr, *U = nullptr, *V = nullptr, *DZ = nullptr;  // multi-vectors of len m (DZ: with the dual residual only)
  double* S = nullptr;  // ns == 1: m values; ns == K: a multi-vector of len m
  double *part = nullptr, *dpart = nullptr;
  double *W = nullptr, *par = nullptr, *snorm = nullptr;
  int32_t* kind = nullptr;
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  admm_sparse_reg_options last{};
};

namespace {

const char* kWho = "the sparse multi-fit regression";

int srg_setup(admm_sparse_reg* o, const admm_sparse_reg_desc* desc, const std::vector<int32_t>& kh,
              const std::vector<double>& ph) {
  const int32_t K = desc->K;
  o->K = K;
  ADMM_TRY(o->cg.build(o, desc->device, desc->D));
  const int64_t m = o->cg.m;
  o->m = m;
  o->n = o->cg.n;
  o->ns = desc->ns;
  o->nwg = scg_vec_workgroups(m);
  o->nwg_n = scg_vec_workgroups(o->n);
  const size_t kp = static_cast<size_t>(o->cg.chunks) * kSpmmChunk;
  for (double** p : {&o->Z, &o->U, &o->V}) {
    ADMM_TRY(o->mem.alloc(p, kp * m));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * m, o->stream));
  }
  ADMM_TRY(o->mem.alloc(&o->snorm, static_cast<size_t>(K)));
  {  // ||s_k||, once: perr needs max(||Dx||, ||z||, ||s_k||).  The column-major copy is the shared response itself
    double* scol = nullptr;
    ADMM_TRY(o->mem.alloc(&scol, static_cast<size_t>(m) * o->ns));
    ADMM_HIP_TRY(hipMemcpyAsync(scol, desc->S, sizeof(double) * m * o->ns, hipMemcpyHostToDevice, o->stream));
    launch_regm_snorm(scol, m, m, K, o->ns, o->snorm, o->stream);
    if (o->ns == 1) {
      o->S = scol;
    } else {
      ADMM_TRY(o->mem.alloc(&o->S, kp * m));
      ADMM_TRY(o->cg.upload(o->S, desc->S, m));
      ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
      o->mem.free_one(scol);
    }
  }
  ADMM_TRY(o->mem.alloc(&o->part, kp * SR_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * kp * SR_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->dpart, kp * SD_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->dpart, 0, sizeof(double) * kp * SD_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(4) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 4 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_words(*o, &o->kind, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->kind, kh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (kh, ph and the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // namespace

extern "C" {

void admm_sparse_reg_desc_default(admm_sparse_reg_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_sparse_reg_desc);
  d->K = 1;
  d->ns = 1;
}

void admm_sparse_reg_options_default(admm_sparse_reg_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_sparse_reg_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->cg_tol = 1e-12;   // admm_problem_desc_default
  o->cg_maxit = 200;
  o->nodualerror = 1;  // what admm_reg_multi runs; 0 is the reference's default (admm.m:76)
}

int admm_sparse_reg_chunk(void) { return kSpmmChunk; }

int admm_sparse_reg_create(const admm_sparse_reg_desc* desc, admm_sparse_reg** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_sparse_reg_desc)))
    return fail(ADMM_E_INVALID, "admm_sparse_reg_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the sparse multi-fit regression needs at least one fit (K >= 1)");
  ADMM_TRY(check_sparse_D(kWho, desc->D));
  if (!desc->S) return fail(ADMM_E_INVALID, "the sparse multi-fit regression needs the responses S (rows x ns)");
  ADMM_TRY(check_response_columns(desc->ns, desc->K));
  std::vector<int32_t> kh;
  std::vector<double> ph;
  ADMM_TRY(check_reg_fits(desc->K, desc->kind, desc->a, desc->b, desc->epsilon, desc->delta, &kh, &ph));
  ADMM_TRY(check_placement(kWho, desc->comm, desc->device));
  return create_object(out, admm_sparse_reg_destroy, [&](admm_sparse_reg* o) { return srg_setup(o, desc, kh, ph); });
}

int admm_sparse_reg_run(admm_sparse_reg* o, const admm_sparse_reg_options* opts, admm_sparse_reg_summary* summaries,
                        double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_reg_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_reg_options.struct_size mismatch (ABI version skew)");
  admm_sparse_reg_options op = *opts;
  ADMM_TRY(check_sparse_run_options("sparse multi-fit", &op));
  const bool dual = op.nodualerror == 0;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  SpmmCg& cg = o->cg;
  if (dual && !o->DZ) {
    const size_t elems = static_cast<size_t>(cg.chunks) * kSpmmChunk * o->m;
    ADMM_TRY(o->mem.alloc(&o->DZ, elems));
    ADMM_HIP_TRY(hipMemsetAsync(o->DZ, 0, sizeof(double) * elems, o->stream));
  }
  ADMM_TRY(begin_run(*o));
  ScgArgs ca{};
  ADMM_TRY(cg.begin_run(op.cg_tol, op.cg_maxit, &ca));
  ADMM_TRY(cg.upload(o->Z, op.z0, o->m));
  ADMM_TRY(cg.upload(o->U, op.u0, o->m));

  SrgElemArgs ea{};
  ea.m = o->m;
  ea.AX = cg.T;
  ea.Z = o->Z;
  ea.U = o->U;
  ea.V = o->V;
  ea.DZ = dual ? o->DZ : nullptr;
  ea.S = o->S;
  ea.W = o->W;
  ea.par = o->par;
  ea.kind = o->kind;
  ea.rec = o->rec;
  ea.part = o->part;
  ea.K = K;
  ea.ns = o->ns;
  ea.objevals = op.objevals;
  ea.rho = op.rho;
  SrgDualArgs da{};
  da.n = o->n;
  da.GDZ = cg.R;  // (free between two solves: launch_scg_start writes R and P before it reads them)
  da.GU = cg.P;
  da.rec = o->rec;
  da.part = o->dpart;
  da.K = K;
  SrgFinArgs fa{};
  fa.part = o->part;
  fa.dpart = o->dpart;
  fa.snorm = o->snorm;
  fa.m = o->m;
  fa.K = K;
  fa.nwg = o->nwg;
  fa.nwg_n = o->nwg_n;
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
  launch_srg_elem(ea, true, o->stream);  // V = (s + z0) - u0
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    launch_spmm(cg.sp.t, o->V, cg.Y, cg.chunks, run, o->stream);  // y = D'((s + z) - u)
    ADMM_TRY(cg.solve(ca, it == 0));
    launch_spmm(cg.sp.n, cg.X, cg.T, cg.chunks, run, o->stream);  // D x
    launch_srg_elem(ea, false, o->stream);
    if (dual) {
      launch_spmm(cg.sp.t, o->DZ, cg.R, cg.chunks, run, o->stream);  // D'(z - zprev)
      launch_spmm(cg.sp.t, o->U, cg.P, cg.chunks, run, o->stream);   // D'u
      launch_srg_dual(da, o->stream);
    }
    launch_srg_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the sparse multi-fit loop ended with fits still running", N, op.objevals != 0, o->objv,
                      runtime_s, summaries));
  return end_sparse_run(o, op, summaries);
}

int admm_sparse_reg_set_weights(admm_sparse_reg* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_shared_weights(*o, o->m, weights, &o->W);
}

int admm_sparse_reg_fetch(admm_sparse_reg* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_SRG_F_XOPT: return o->cg.fetch_matrix(o->cg.X, o->n, dst, cap, written);
    case ADMM_SRG_F_ZOPT: return o->cg.fetch_matrix(o->Z, o->m, dst, cap, written);
    case ADMM_SRG_F_UOPT: return o->cg.fetch_matrix(o->U, o->m, dst, cap, written);
    case ADMM_SRG_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_SRG_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_SRG_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_SRG_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_SRG_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse multi-fit regression");
  }
}

void admm_sparse_reg_destroy(admm_sparse_reg* o) { destroy_sparse(o); }

}  // extern "C"
