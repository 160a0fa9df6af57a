// sparse_reg.hip -- quantile / LAD / Huber regression, K fits at once on a SPARSE design matrix.  The loop
// is reg_multi.hip's: K independent plain-ADMM runs (admm.m:496-743: A = D, B = -1, c = s_k, stopcond 'standard') that
// share D; the loss and its parameters sit in the element-wise z-prox (loss_device.h: loss_prox_elem) and the objective
// alone.  The x-update is sparse_svm.hip's: x_k = (D'D)^-1 D'(s_k + z_k - u_k) (getProxOps.m:1511-1515) as CG on
// D'D x = D'(s_k + z_k - u_k), no shift, nothing n x n: the first solve of a run starts from 0 and every later one from
// the previous x, so every iterate stays in range(D') -- with full column rank the reference's solution, otherwise the
// minimum-norm one (a column of D without nonzeros keeps x = 0.0; lad.m:134 would fail in chol there).
// Per iteration, every launch for all K fits at once (blockIdx.y = chunk of kSpmmChunk fits):
//   Y = D' V                      one SpMM (spmm.hip); V = (s + z) - u, left behind by the element pass
//   launch_ssv_cg_start / _step   the lock-step CG of sparse_svm.hip as it is, driven by srg_solve
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

#include "engine_internal.h"
#include "loss_device.h"
#include "reg_multi.h"
#include "sparse_reg.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// per-fit sums over the workgroup of NS per-thread values, the rows of the block added in row order (the order of
// sparse_svm.hip's ssv_class_sums): part[(fit * NS + s) * kSsvMaxWg + blockIdx.x].  lds: NS * kSsvBlock doubles.
template <int NS>
__device__ __forceinline__ void srg_fit_sums(const double (&acc)[NS], double* lds, double* part) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < NS; ++s) lds[s * kSsvBlock + tid] = acc[s];
  __syncthreads();
  if (tid < NS * KC) {
    const int s = tid / KC, c = tid % KC;
    double v = 0.0;
    for (int r = 0; r < kSsvRows; ++r) v += lds[s * kSsvBlock + r * KC + c];
    const int64_t fit = static_cast<int64_t>(blockIdx.y) * KC + c;
    part[(fit * NS + s) * kSsvMaxWg + blockIdx.x] = v;
  }
}

struct SrgLane {
  int c, r, fit;
  bool run;  // the fit exists and its ADMM run has not stopped
};
__device__ __forceinline__ SrgLane srg_lane(const OvrRec* rec, int32_t K) {
  SrgLane l;
  l.c = threadIdx.x % KC;
  l.r = threadIdx.x / KC;
  l.fit = static_cast<int>(blockIdx.y) * KC + l.c;
  l.run = l.fit < K && rec[l.fit < K ? l.fit : K - 1].stop == 0;
  return l;
}

// INIT: only V = (s + z0) - u0, before the first iteration
template <bool INIT>
__global__ __launch_bounds__(kSsvBlock) void srg_elem_kernel(SrgElemArgs a) {
  __shared__ double lds[SR_COUNT * kSsvBlock];
  const SrgLane l = srg_lane(a.rec, a.K);
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
  const int64_t nrb = (a.m + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
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
  srg_fit_sums<SR_COUNT>(sums, lds, a.part);
}

// per fit the partial squared norms over n of D'(z - zprev) and D'u
__global__ __launch_bounds__(kSsvBlock) void srg_dual_kernel(SrgDualArgs a) {
  __shared__ double lds[SD_COUNT * kSsvBlock];
  const SrgLane l = srg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[SD_COUNT] = {0.0, 0.0};
  const int64_t nrb = (a.n + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
    if (l.run && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      const double g = a.GDZ[e], h = a.GU[e];
      acc[SD_DZ2] += g * g;
      acc[SD_U2] += h * h;
    }
  }
  srg_fit_sums<SD_COUNT>(acc, lds, a.part);
}

// blockIdx.x = fit: the finalize logic of the fit's iteration -- admm.m:612-658, 706-713 as oracle/admm_ref.py restates
// it, for plain ADMM with stopcond = 'standard'; the dual residual takes part when a.dual is set
__global__ __launch_bounds__(kBlock) void srg_fin_kernel(SrgFinArgs a) {
  const int fit = blockIdx.x;
  OvrRec* rec = a.rec + fit;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[8];
  const int tid = threadIdx.x;
  {  // 32 lanes per slot stride over the workgroup partials, then a fixed shuffle tree
    const int slot = tid >> 5, sub = tid & 31;
    double v = 0.0;
    if (slot < SR_COUNT) {
      const double* __restrict__ ps = a.part + (static_cast<int64_t>(fit) * SR_COUNT + slot) * kSsvMaxWg;
      for (int b = sub; b < a.nwg; b += 32) v += ps[b];
    } else if (a.dual && slot < SR_COUNT + SD_COUNT) {
      const double* __restrict__ ps = a.dpart + (static_cast<int64_t>(fit) * SD_COUNT + (slot - SR_COUNT)) * kSsvMaxWg;
      for (int b = sub; b < a.nwg_n; b += 32) v += ps[b];
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (sub == 0 && slot < 8) S[slot] = v;
  }
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
  rec->iter = i1;
  rec->steps = i1;
  if (stop) rec->early = 1;
  if (stop || i1 >= a.maxiters) rec->stop = 1;
}

}  // namespace

void launch_srg_elem(const SrgElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(ssv_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(srg_elem_kernel<true>, grid, dim3(kSsvBlock), 0, stream, a);
  else hipLaunchKernelGGL(srg_elem_kernel<false>, grid, dim3(kSsvBlock), 0, stream, a);
}

void launch_srg_dual(const SrgDualArgs& a, hipStream_t stream) {
  const dim3 grid(ssv_vec_workgroups(a.n), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(srg_dual_kernel, grid, dim3(kSsvBlock), 0, stream, a);
}

void launch_srg_fin(const SrgFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(srg_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_reg {
  hipStream_t stream = nullptr;
  DevMem mem;
  SparseDev sp;
  int device = 0;
  int64_t m = 0, n = 0, nnz = 0;
  int32_t K = 0, ns = 1, chunks = 0, nwg = 0, nwg_n = 0;
  // multi-vectors, [chunks][len][kSpmmChunk]
  double *X = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr, *Y = nullptr;  // len n (between two solves R and P hold
                                                                                // D'(z - zprev) and D'u)
  double *Z = nullptr, *U = nullptr, *V = nullptr, *T = nullptr, *DZ = nullptr;  // len m (T: D p and D x; DZ: with the
                                                                                 // dual residual only)
  double* S = nullptr;  // ns == 1: m values; ns == K: a multi-vector of len m
  double *cgpart = nullptr, *part = nullptr, *dpart = nullptr;
  double *W = nullptr, *par = nullptr, *snorm = nullptr;
  int32_t *kind = nullptr, *alldone = nullptr;
  SsvCg* cg = nullptr;
  OvrRec* rec = nullptr;
  struct Poll {  // pinned
    int32_t alldone, longest;
  }* poll = nullptr;
  OvrRec* rec_host = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // [K][hist_ld]
  int32_t hist_ld = 0;
  int cg_batch = 8;  // inner iterations enqueued between two polls of the all-done word
  bool has_run = false;
  admm_sparse_reg_options last{};
  std::vector<int32_t> steps;
};

namespace {

template <class T>
int srg_alloc_words(admm_sparse_reg* o, T** out, size_t count) {
  double* raw = nullptr;
  ADMM_TRY(o->mem.alloc(&raw, (count * sizeof(T) + 7) / 8));
  ADMM_HIP_TRY(hipMemsetAsync(raw, 0, (count * sizeof(T) + 7) / 8 * 8, o->stream));
  *out = reinterpret_cast<T*>(raw);
  return ADMM_OK;
}

// column-major host matrix (rows x K), or zeros, into a chunked multi-vector
int srg_upload(admm_sparse_reg* o, double* dst, const double* src, int64_t rows) {
  const size_t elems = static_cast<size_t>(o->chunks) * rows * kSpmmChunk;
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * elems, o->stream));
    return ADMM_OK;
  }
  std::vector<double> h(elems);
  spmm_pack(src, rows, rows, o->K, h.data());
  ADMM_HIP_TRY(hipMemcpyAsync(dst, h.data(), sizeof(double) * elems, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (h goes out of scope)
  return ADMM_OK;
}

int srg_setup(admm_sparse_reg* o, const admm_sparse_reg_desc* desc, const std::vector<int32_t>& kh,
              const std::vector<double>& ph) {
  ADMM_HIP_TRY(hipSetDevice(desc->device));
  o->device = desc->device;
  ADMM_HIP_TRY(hipStreamCreate(&o->stream));
  const admm_sparse_desc* D = desc->D;
  ADMM_TRY(sparse_device_build(D, &o->sp, o->stream));
  const int64_t m = D->rows, n = D->cols;
  const int32_t K = desc->K;
  o->m = m;
  o->n = n;
  o->nnz = D->nnz;
  o->K = K;
  o->ns = desc->ns;
  o->chunks = spmm_chunks(K);
  o->nwg = ssv_vec_workgroups(m);
  o->nwg_n = ssv_vec_workgroups(n);
  const size_t kp = static_cast<size_t>(o->chunks) * kSpmmChunk;
  for (double** p : {&o->X, &o->R, &o->P, &o->Q, &o->Y}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  for (double** p : {&o->Z, &o->U, &o->V, &o->T}) {
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
      ADMM_TRY(srg_upload(o, o->S, desc->S, m));
      ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
      o->mem.free_one(scol);
    }
  }
  ADMM_TRY(o->mem.alloc(&o->cgpart, kp * 2 * kSsvMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->cgpart, 0, sizeof(double) * kp * 2 * kSsvMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->part, kp * SR_COUNT * kSsvMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * kp * SR_COUNT * kSsvMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->dpart, kp * SD_COUNT * kSsvMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->dpart, 0, sizeof(double) * kp * SD_COUNT * kSsvMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(4) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 4 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(srg_alloc_words(o, &o->kind, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->kind, kh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(srg_alloc_words(o, &o->alldone, 2));
  ADMM_TRY(srg_alloc_words(o, &o->cg, static_cast<size_t>(K)));
  ADMM_TRY(srg_alloc_words(o, &o->rec, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&o->poll), sizeof(*o->poll)));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&o->rec_host), sizeof(OvrRec) * K));
  ADMM_HIP_TRY(hipEventCreate(&o->ev0));
  ADMM_HIP_TRY(hipEventCreate(&o->ev1));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (kh, ph and the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

SpmmMask srg_mask(const admm_sparse_reg* o, bool with_cg) {
  SpmmMask mk;
  mk.flag_a = &o->rec->stop;
  mk.stride_a = kOvrRecWords;
  if (with_cg) {
    mk.flag_b = reinterpret_cast<const int32_t*>(o->cg) + kSsvDoneWord;
    mk.stride_b = kSsvCgWords;
  }
  mk.K = o->K;
  return mk;
}

// X <- the CG solution of D'D x = Y for every running fit; the host polls the all-done word once per batch (the shape
// of sparse_svm.hip's driver)
int srg_solve(admm_sparse_reg* o, const SsvCgArgs& a, bool first) {
  const SpmmMask run = srg_mask(o, false), live = srg_mask(o, true);
  if (!first) {  // q = D'(D x) in front of a warm start
    launch_spmm(o->sp.n, o->X, o->T, o->chunks, run, o->stream);
    launch_spmm(o->sp.t, o->T, o->Q, o->chunks, run, o->stream);
  }
  launch_ssv_cg_start(a, first, o->stream);
  for (int32_t done_it = 0; done_it < a.maxit;) {
    const int32_t k = std::min(a.maxit - done_it, static_cast<int32_t>(o->cg_batch));
    for (int32_t c = 0; c < k; ++c) {
      launch_spmm(o->sp.n, o->P, o->T, o->chunks, live, o->stream);
      launch_spmm(o->sp.t, o->T, o->Q, o->chunks, live, o->stream);
      launch_ssv_cg_step(a, o->stream);
    }
    done_it += k;
    ADMM_HIP_TRY(hipMemcpyAsync(o->poll, o->alldone, sizeof(*o->poll), hipMemcpyDeviceToHost, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
    if (o->poll->alldone) break;
  }
  // (a batch as long as the last solve took: one or two polls per solve)
  o->cg_batch = std::min(64, std::max(4, static_cast<int>(o->poll->longest) + 2));
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
  if (!desc->D) return fail(ADMM_E_INVALID, "the sparse multi-fit regression needs D (admm_sparse_desc)");
  if (desc->D->mem != ADMM_MEM_HOST)
    return fail(ADMM_E_INVALID, "the sparse multi-fit regression takes D in host arrays");
  ADMM_TRY(sparse_csc_check(desc->D));
  if (!desc->S) return fail(ADMM_E_INVALID, "the sparse multi-fit regression needs the responses S (rows x ns)");
  if (desc->ns != 1 && desc->ns != desc->K)
    return fail(ADMM_E_INVALID, "S has " + std::to_string(desc->ns) + " columns: one shared response or one per fit (" +
                                    std::to_string(desc->K) + ")");
  const int32_t K = desc->K;
  std::vector<int32_t> kh(static_cast<size_t>(K), 0);
  std::vector<double> ph(static_cast<size_t>(4) * K);
  for (int32_t k = 0; k < K; ++k) {  // per fit, exactly as admm_engine_set_loss checks it
    if (desc->kind) kh[k] = desc->kind[k];
    if (kh[k] != 0 && kh[k] != 1)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": kind must be 0 (LAD family) or 1 (Huber family)");
    const admm_loss_desc ld{nullptr, desc->a ? desc->a[k] : 1.0, desc->b ? desc->b[k] : 1.0,
                            desc->epsilon ? desc->epsilon[k] : 0.0, desc->delta ? desc->delta[k] : 1.0};
    if (check_loss_desc(kh[k] ? ADMM_PROB_HUBERFIT : ADMM_PROB_LAD, ld, 0) != ADMM_OK)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": " + std::string(admm_last_error()));
    ph[4 * k + 0] = ld.slope_pos;
    ph[4 * k + 1] = ld.slope_neg;
    ph[4 * k + 2] = ld.epsilon;
    ph[4 * k + 3] = ld.delta;
  }
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, "the sparse multi-fit regression is not row-sharded");
  int ndev = 0;
  ADMM_TRY(admm_device_count(&ndev));
  if (ndev <= 0) return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  if (desc->device < 0 || desc->device >= ndev) return fail(ADMM_E_INVALID, "bad device ordinal");
  admm_sparse_reg* o = new admm_sparse_reg();
  const int rc = srg_setup(o, desc, kh, ph);
  if (rc != ADMM_OK) {
    const std::string msg = admm_last_error();
    admm_sparse_reg_destroy(o);
    return fail(rc, msg);
  }
  *out = o;
  return ADMM_OK;
}

int admm_sparse_reg_run(admm_sparse_reg* o, const admm_sparse_reg_options* opts, admm_sparse_reg_summary* summaries,
                        double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_reg_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_reg_options.struct_size mismatch (ABI version skew)");
  admm_sparse_reg_options op = *opts;
  if (op.fast != ADMM_FAST_OFF)
    return fail(ADMM_E_UNSUPPORTED, "fast / accelerated ADMM is not part of the sparse multi-fit loop");
  if (op.relax != 1.0) return fail(ADMM_E_UNSUPPORTED, "relaxation is not part of the sparse multi-fit loop");
  if (op.convtest) return fail(ADMM_E_UNSUPPORTED, "convtest is not part of the sparse multi-fit loop");
  if (!(op.rho > 0.0)) return fail(ADMM_E_INVALID, "options.rho must be positive");
  if (op.maxiters <= 0) op.maxiters = 1000;  // admm.m:334-339
  if (!(op.cg_tol > 0.0)) op.cg_tol = 1e-12;
  if (op.cg_maxit <= 0) op.cg_maxit = 200;
  const bool dual = op.nodualerror == 0;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  if (o->hist_ld != N) {
    for (double** p : {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}) {
      o->mem.free_one(*p);
      *p = nullptr;
      ADMM_TRY(o->mem.alloc(p, static_cast<size_t>(N) * K));
    }
    o->hist_ld = N;
  }
  if (dual && !o->DZ) {
    const size_t elems = static_cast<size_t>(o->chunks) * kSpmmChunk * o->m;
    ADMM_TRY(o->mem.alloc(&o->DZ, elems));
    ADMM_HIP_TRY(hipMemsetAsync(o->DZ, 0, sizeof(double) * elems, o->stream));
  }
  o->has_run = false;
  ADMM_HIP_TRY(hipMemsetAsync(o->rec, 0, sizeof(OvrRec) * K, o->stream));
  ADMM_HIP_TRY(hipMemsetAsync(o->cg, 0, sizeof(SsvCg) * K, o->stream));
  ADMM_TRY(srg_upload(o, o->X, nullptr, o->n));  // (x0 is never read: the first x-update starts CG from 0)
  ADMM_TRY(srg_upload(o, o->Z, op.z0, o->m));
  ADMM_TRY(srg_upload(o, o->U, op.u0, o->m));

  SsvCgArgs ca{};
  ca.n = o->n;
  ca.tol = op.cg_tol;
  ca.maxit = op.cg_maxit;
  ca.K = K;
  ca.Y = o->Y;
  ca.X = o->X;
  ca.R = o->R;
  ca.P = o->P;
  ca.Q = o->Q;
  ca.part = o->cgpart;
  ca.st = o->cg;
  ca.rec = o->rec;
  ca.alldone = o->alldone;
  SrgElemArgs ea{};
  ea.m = o->m;
  ea.AX = o->T;
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
  da.GDZ = o->R;  // (free between two solves: launch_ssv_cg_start writes R and P before it reads them)
  da.GU = o->P;
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
  const SpmmMask run = srg_mask(o, false);
  const int check_every = op.check_every > 0 ? op.check_every : (op.domaxiters ? 64 : 8);
  o->cg_batch = 8;  // (a run never depends on the one before it)

  ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
  launch_srg_elem(ea, true, o->stream);  // V = (s + z0) - u0
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    launch_spmm(o->sp.t, o->V, o->Y, o->chunks, run, o->stream);  // y = D'((s + z) - u)
    ADMM_TRY(srg_solve(o, ca, it == 0));
    launch_spmm(o->sp.n, o->X, o->T, o->chunks, run, o->stream);  // D x
    launch_srg_elem(ea, false, o->stream);
    if (dual) {
      launch_spmm(o->sp.t, o->DZ, o->R, o->chunks, run, o->stream);  // D'(z - zprev)
      launch_spmm(o->sp.t, o->U, o->P, o->chunks, run, o->stream);   // D'u
      launch_srg_dual(da, o->stream);
    }
    launch_srg_fin(fa, o->stream);
    if ((it + 1) % check_every == 0 || it + 1 == N) {
      ADMM_HIP_TRY(hipMemcpyAsync(o->rec_host, o->rec, sizeof(OvrRec) * K, hipMemcpyDeviceToHost, o->stream));
      ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
      all = true;
      for (int32_t c = 0; c < K; ++c) all = all && o->rec_host[c].stop != 0;
    }
  }
  ADMM_HIP_TRY(hipEventRecord(o->ev1, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  ADMM_HIP_TRY(hipGetLastError());
  if (!all) return fail(ADMM_E_DEVICE, "the sparse multi-fit loop ended with fits still running");
  float ms = 0.f;
  ADMM_HIP_TRY(hipEventElapsedTime(&ms, o->ev0, o->ev1));
  if (runtime_s) *runtime_s = 1e-3 * static_cast<double>(ms);
  o->steps.assign(static_cast<size_t>(K), 0);
  std::vector<double> objh;
  if (op.objevals) {
    objh.resize(static_cast<size_t>(N) * K);
    ADMM_HIP_TRY(hipMemcpy(objh.data(), o->objv, sizeof(double) * N * K, hipMemcpyDeviceToHost));
  }
  std::vector<SsvCg> cgh(static_cast<size_t>(K));
  ADMM_HIP_TRY(hipMemcpy(cgh.data(), o->cg, sizeof(SsvCg) * K, hipMemcpyDeviceToHost));
  for (int32_t c = 0; c < K; ++c) {
    const OvrRec& r = o->rec_host[c];
    o->steps[c] = r.steps;
    if (summaries) {
      summaries[c].steps = r.steps;
      summaries[c].stopped_early = r.early;
      summaries[c].objopt = (op.objevals && r.steps > 0) ? objh[static_cast<size_t>(c) * N + r.steps - 1]
                                                         : __builtin_nan("");
      summaries[c].cg_iters_total = cgh[c].total;
      summaries[c].cg_capped_updates = cgh[c].capped;
    }
  }
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_sparse_reg_set_weights(admm_sparse_reg* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (weights)  // (a refused call changes nothing)
    for (int64_t i = 0; i < o->m; ++i)
      if (!finite_nonneg(weights[i]))
        return fail(ADMM_E_INVALID, "loss: weight " + std::to_string(i) + " is negative or not finite");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  double* w = nullptr;
  if (weights) {
    ADMM_TRY(o->mem.alloc(&w, static_cast<size_t>(o->m)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, weights, sizeof(double) * o->m, hipMemcpyHostToDevice, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the caller's buffer is read until here)
  }
  if (o->W) o->mem.free_one(o->W);
  o->W = w;
  return ADMM_OK;
}

int admm_sparse_reg_fetch(admm_sparse_reg* o, int field, double* dst, size_t cap, size_t* written) {
  if (!o || !dst) return fail(ADMM_E_INVALID, "object/dst is NULL");
  if (!o->has_run) return fail(ADMM_E_INVALID, "fetch before the first run");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t K = o->K;
  auto matrix = [&](const double* src, int64_t rows) -> int {
    const size_t need = static_cast<size_t>(rows) * K;
    if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    std::vector<double> h(static_cast<size_t>(o->chunks) * rows * kSpmmChunk);
    ADMM_HIP_TRY(hipMemcpy(h.data(), src, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    spmm_unpack(h.data(), rows, K, dst, rows);
    if (written) *written = need;
    return ADMM_OK;
  };
  auto history = [&](const double* src) -> int {
    int32_t S = 0;
    for (int32_t s : o->steps) S = s > S ? s : S;
    const size_t need = static_cast<size_t>(S) * K;
    if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    if (S > 0)
      ADMM_HIP_TRY(hipMemcpy2D(dst, S * sizeof(double), src, o->hist_ld * sizeof(double), S * sizeof(double), K,
                               hipMemcpyDeviceToHost));
    for (int32_t c = 0; c < K; ++c)
      for (int32_t i = o->steps[c]; i < S; ++i) dst[static_cast<size_t>(c) * S + i] = __builtin_nan("");
    if (written) *written = need;
    return ADMM_OK;
  };
  switch (field) {
    case ADMM_SRG_F_XOPT: return matrix(o->X, o->n);
    case ADMM_SRG_F_ZOPT: return matrix(o->Z, o->m);
    case ADMM_SRG_F_UOPT: return matrix(o->U, o->m);
    case ADMM_SRG_F_PNORM: return history(o->pnorm);
    case ADMM_SRG_F_PERR: return history(o->perr);
    case ADMM_SRG_F_OBJEVALS:
      if (!o->last.objevals) return fail(ADMM_E_INVALID, "the last run did not evaluate the objective (objevals = 0)");
      return history(o->objv);
    case ADMM_SRG_F_DNORM:
    case ADMM_SRG_F_DERR:
      if (o->last.nodualerror)
        return fail(ADMM_E_INVALID, "the last run did not evaluate the dual residual (nodualerror = 1)");
      return history(field == ADMM_SRG_F_DNORM ? o->dnorm : o->derr);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse multi-fit regression");
  }
}

void admm_sparse_reg_destroy(admm_sparse_reg* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  if (o->stream) (void)hipStreamSynchronize(o->stream);
  if (o->ev0) (void)hipEventDestroy(o->ev0);
  if (o->ev1) (void)hipEventDestroy(o->ev1);
  o->mem.release();
  sparse_device_free(&o->sp);
  if (o->poll) (void)hipHostFree(o->poll);
  if (o->rec_host) (void)hipHostFree(o->rec_host);
  if (o->stream) (void)hipStreamDestroy(o->stream);
  delete o;
}

}  // extern "C"
