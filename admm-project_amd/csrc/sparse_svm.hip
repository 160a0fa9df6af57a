// sparse_svm.hip -- the linear SVM for all one-vs-rest classes on a SPARSE design matrix.  The loop is
// svm_ovr.hip's: K independent plain-ADMM runs (unwrappedadmm.m:76-92: A = D, B = -1, c = 0, stopcond 'both',
// nodualerror 1) that share D; the one difference is the x-update.  x_c = D^+(z_c - u_c) is CG on D'D x = D'(z_c - u_c),
// no shift, nothing n x n: the first solve of a run starts from 0 and every later one from the previous x, so every
// iterate stays in range(D') and the limit is the pseudo-inverse solution (a column of D without nonzeros keeps x = 0.0).
// Per iteration, every launch for all K classes at once (blockIdx.y = chunk of kSpmmChunk classes):
//   Y = D' V                      one SpMM (spmm.hip)
//   ssv_cg_init / _start          r = y - D'(D x), p = r, per-class rs and ||y||
//   per inner iteration           T = D P, Q = D' T (two SpMM), ssv_cg_dot / _update / _direction / _advance
//   AX = D X                      one SpMM
//   ssv_elem_kernel               the element update of every class -- prox_apply / loss_form_z, the code of the dense pass
//                                 -- its residual sums, and V = z - u
//   ssv_fin_kernel                per class pnorm, perr, Hnormsq, the objective and the stop decision (admm.m:612-722)
// A class whose stop flag is set is FROZEN, and a class whose solve is done is masked until the next solve: every kernel
// and every product skips it.  Every sum runs in a fixed order that depends on the sizes alone: two runs give the same
// bits, and a class gets the same numbers wherever it lands.
#include <cmath>
#include <cstddef>
#include <vector>

#include "engine_internal.h"
#include "prox_device.h"
#include "sparse_svm.h"
#include "svm_cost_device.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// per-class sums over the workgroup of NS per-thread values, the rows of the block added in row order:
// part[(class * nstot + slot0 + s) * kSsvMaxWg + blockIdx.x].  lds: NS * kSsvBlock doubles.
template <int NS>
__device__ __forceinline__ void ssv_class_sums(const double (&acc)[NS], double* lds, double* part, int nstot, int slot0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < NS; ++s) lds[s * kSsvBlock + tid] = acc[s];
  __syncthreads();
  if (tid < NS * KC) {
    const int s = tid / KC, c = tid % KC;
    double v = 0.0;
    for (int r = 0; r < kSsvRows; ++r) v += lds[s * kSsvBlock + r * KC + c];
    const int64_t cls = static_cast<int64_t>(blockIdx.y) * KC + c;
    part[(cls * nstot + slot0 + s) * kSsvMaxWg + blockIdx.x] = v;
  }
}

// the sum of a slot's nb workgroup partials for every class of `chunk`; each thread returns its own class's.  Wave w
// sums the classes w, w + kSsvWaves, ...: lane l adds the partials l, l + 64, ... in that order, then the shuffle tree.
__device__ __forceinline__ double ssv_class_total(const double* part, int nstot, int slot, int chunk, int nb, double* lds) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int c = wid; c < KC; c += kSsvWaves) {
    const double* __restrict__ p = part + ((static_cast<int64_t>(chunk) * KC + c) * nstot + slot) * kSsvMaxWg;
    double v = 0.0;
    for (int b = lane; b < nb; b += kWave) v += p[b];
    v = wave_sum(v);
    if (lane == 0) lds[c] = v;
  }
  __syncthreads();
  return lds[threadIdx.x % KC];
}

struct SsvLane {
  int c, r, cls;
  bool run;  // the class exists and its ADMM run has not stopped
};
__device__ __forceinline__ SsvLane ssv_lane(const OvrRec* rec, int32_t K) {
  SsvLane l;
  l.c = threadIdx.x % KC;
  l.r = threadIdx.x / KC;
  l.cls = static_cast<int>(blockIdx.y) * KC + l.c;
  l.run = l.cls < K && rec[l.cls < K ? l.cls : K - 1].stop == 0;
  return l;
}

// r = y - q, p = r, partials of r.r and y.y.  FIRST: the first x-update of a run starts from x = 0 (r = y)
template <bool FIRST>
__global__ __launch_bounds__(kSsvBlock) void ssv_cg_init_kernel(SsvCgArgs a) {
  __shared__ double lds[2 * kSsvBlock];
  const SsvLane l = ssv_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[2] = {0.0, 0.0};
  const int64_t nrb = (a.n + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
    if (l.run && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      const double yv = a.Y[e];
      double rv = yv;
      if (FIRST) a.X[e] = 0.0;
      else rv = yv - a.Q[e];
      a.R[e] = rv;
      a.P[e] = rv;
      acc[0] += rv * rv;
      acc[1] += yv * yv;
    }
  }
  ssv_class_sums<2>(acc, lds, a.part, 2, 0);
}

// one workgroup per chunk: rs, ||y||, and whether x is already good enough.  A zero right-hand side ends the solve with
// x = 0 (ssv_cg_update_kernel stores it)
__global__ __launch_bounds__(kSsvBlock) void ssv_cg_start_kernel(SsvCgArgs a, int nb) {
  __shared__ double l0[KC], l1[KC];
  const SsvLane l = ssv_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const double rs = ssv_class_total(a.part, 2, 0, blockIdx.y, nb, l0);
  const double yy = ssv_class_total(a.part, 2, 1, blockIdx.y, nb, l1);
  if (l.r == 0 && l.run) {
    SsvCg* st = a.st + l.cls;
    const bool zero = yy == 0.0;
    st->rs = rs;
    st->ynorm = sqrt(yy);
    st->iters = 0;
    st->brk = 0;
    st->zero = zero ? 1 : 0;
    st->done = (zero || sqrt(rs) <= a.tol * sqrt(yy)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(kSsvBlock) void ssv_cg_dot_kernel(SsvCgArgs a) {
  __shared__ double lds[kSsvBlock];
  const SsvLane l = ssv_lane(a.rec, a.K);
  const bool live = l.run && a.st[l.run ? l.cls : 0].done == 0;
  if (!__syncthreads_or(live)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[1] = {0.0};
  const int64_t nrb = (a.n + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
    if (live && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      acc[0] += a.P[e] * a.Q[e];
    }
  }
  ssv_class_sums<1>(acc, lds, a.part, 2, 0);
}

// alpha = rs / (p.q); x += alpha p; r -= alpha q; partial r.r.  p.q == 0: nothing is divided or updated, the class ends
__global__ __launch_bounds__(kSsvBlock) void ssv_cg_update_kernel(SsvCgArgs a, int nb) {
  __shared__ double lds[kSsvBlock];
  __shared__ double lt[KC];
  const SsvLane l = ssv_lane(a.rec, a.K);
  const SsvCg st = a.st[l.run ? l.cls : 0];
  const bool live = l.run && st.done == 0;
  const bool zero = l.run && st.zero != 0;
  if (!__syncthreads_or(live || zero)) return;
  const double pq = ssv_class_total(a.part, 2, 0, blockIdx.y, nb, lt);
  const bool brk = pq == 0.0;
  const double alpha = brk ? 0.0 : st.rs / pq;
  if (live && brk && blockIdx.x == 0 && l.r == 0) a.st[l.cls].brk = 1;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[1] = {0.0};
  const int64_t nrb = (a.n + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
    if (i >= a.n) continue;
    const int64_t e = base + i * KC + l.c;
    if (zero) a.X[e] = 0.0;
    if (live && !brk) {
      a.X[e] = a.X[e] + alpha * a.P[e];
      const double rv = a.R[e] - alpha * a.Q[e];
      a.R[e] = rv;
      acc[0] += rv * rv;
    }
  }
  ssv_class_sums<1>(acc, lds, a.part, 2, 1);
}

// beta = rs_new / rs; p = r + beta p.  Every workgroup reads st->rs here: the scalar state advances in its own launch
__global__ __launch_bounds__(kSsvBlock) void ssv_cg_direction_kernel(SsvCgArgs a, int nb) {
  __shared__ double lt[KC];
  const SsvLane l = ssv_lane(a.rec, a.K);
  const SsvCg st = a.st[l.run ? l.cls : 0];
  const bool live = l.run && st.done == 0 && st.brk == 0;
  if (!__syncthreads_or(live)) return;
  const double rsn = ssv_class_total(a.part, 2, 1, blockIdx.y, nb, lt);
  const double beta = live ? rsn / st.rs : 0.0;  // (rs > 0: a class with rs = 0 was done at its start)
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  const int64_t nrb = (a.n + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
    if (live && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      a.P[e] = a.R[e] + beta * a.P[e];
    }
  }
}

// ONE workgroup walks the chunks: rs <- r.r, the iteration counts, converged / capped, and the word the host polls
__global__ __launch_bounds__(kSsvBlock) void ssv_cg_advance_kernel(SsvCgArgs a, int nb, int chunks) {
  __shared__ double lt[KC];
  __shared__ int longest;  // inner iterations of the slowest class of this solve (sizes the host's next batch)
  const int c = threadIdx.x % KC, r = threadIdx.x / KC;
  if (threadIdx.x == 0) longest = 0;
  int all = 1;
  for (int ch = 0; ch < chunks; ++ch) {
    const int cls = ch * KC + c;
    const bool run = cls < a.K && a.rec[cls < a.K ? cls : a.K - 1].stop == 0;
    const double rsn = ssv_class_total(a.part, 2, 1, ch, nb, lt);
    int fin = 1;
    if (run && r == 0) {
      SsvCg* st = a.st + cls;
      if (st->done == 0) {
        const bool brk = st->brk != 0;
        if (!brk) st->rs = rsn;
        st->iters += 1;
        st->total += 1;
        const bool converged = sqrt(st->rs) <= a.tol * st->ynorm;
        if (converged || brk || st->iters >= a.maxit) {
          if (!converged) st->capped += 1;
          st->done = 1;
        }
      }
      fin = st->done;
      atomicMax(&longest, st->iters);
    }
    all &= __syncthreads_and(fin);  // (also the barrier in front of the next chunk's use of lt)
  }
  if (threadIdx.x == 0) {
    a.alldone[0] = all;
    a.alldone[1] = longest;
  }
}

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
__global__ __launch_bounds__(kSsvBlock) void ssv_elem_kernel(SsvElemArgs a) {
  __shared__ double lds[OV_COUNT * kSsvBlock];
  const SsvLane l = ssv_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[S_COUNT];
#pragma unroll
  for (int q = 0; q < S_COUNT; ++q) acc[q] = 0.0;
  const int cl = l.run ? l.cls : 0;
  const int32_t loss = a.loss[cl];
  const bool cost = a.chunk_cost[blockIdx.y] != 0;
  // (z, u, ell addressed through the chunk base with the element's own index)
  ProxArgs pa = ssv_prox_args(a, a.Z + base, a.U + base, a.ELL + base, loss);
  const SvmCostArgs ks{nullptr, a.CC[2 * cl], a.CC[2 * cl + 1], a.C, a.rho, loss, a.objevals};
  if (cost) {  // z reaches prox_apply in a register; the objective's terms are summed beside it
    pa.prox = PROX_GIVEN;
    pa.objx = OBJX_NONE;
  }
  const int64_t nrb = (a.m + kSsvRows - 1) / kSsvRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kSsvRows + l.r;
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
  ssv_class_sums<OV_COUNT>(sums, lds, a.part, OV_COUNT, 0);
}

// blockIdx.x = class: the finalize logic of the class's iteration -- ovr_gsum_fin_kernel's (admm.m:612-722 for plain ADMM
// with nodualerror = 1 and stopcond = 'both'), with x read from the chunked layout
__global__ __launch_bounds__(kBlock) void ssv_fin_kernel(SsvFinArgs a) {
  const int cls = blockIdx.x;
  OvrRec* rec = a.rec + cls;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[8];
  __shared__ double sq[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  {  // 32 lanes per slot stride over the workgroup partials, then a fixed shuffle tree
    const int slot = tid >> 5, sub = tid & 31;
    double v = 0.0;
    if (slot < OV_COUNT) {
      const double* __restrict__ ps = a.part + (static_cast<int64_t>(cls) * OV_COUNT + slot) * kSsvMaxWg;
      for (int b = sub; b < a.nwg; b += 32) v += ps[b];
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (sub == 0 && slot < 8) S[slot] = v;
  }
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
  rec->iter = i1;
  rec->steps = i1;
  if (stop) rec->early = 1;
  if (stop || i1 >= a.maxiters) rec->stop = 1;
}

}  // namespace

int ssv_vec_workgroups(int64_t len) {
  return static_cast<int>(std::min<int64_t>(std::max<int64_t>(ceil_div(len, int64_t{kSsvRows}), 1), kSsvMaxWg));
}

void launch_ssv_cg_start(const SsvCgArgs& a, bool first, hipStream_t stream) {
  const int nb = ssv_vec_workgroups(a.n);
  const unsigned chunks = static_cast<unsigned>(spmm_chunks(a.K));
  if (first) hipLaunchKernelGGL(ssv_cg_init_kernel<true>, dim3(nb, chunks), dim3(kSsvBlock), 0, stream, a);
  else hipLaunchKernelGGL(ssv_cg_init_kernel<false>, dim3(nb, chunks), dim3(kSsvBlock), 0, stream, a);
  hipLaunchKernelGGL(ssv_cg_start_kernel, dim3(1, chunks), dim3(kSsvBlock), 0, stream, a, nb);
}

void launch_ssv_cg_step(const SsvCgArgs& a, hipStream_t stream) {
  const int nb = ssv_vec_workgroups(a.n);
  const int chunks = spmm_chunks(a.K);
  const dim3 grid(nb, static_cast<unsigned>(chunks));
  hipLaunchKernelGGL(ssv_cg_dot_kernel, grid, dim3(kSsvBlock), 0, stream, a);
  hipLaunchKernelGGL(ssv_cg_update_kernel, grid, dim3(kSsvBlock), 0, stream, a, nb);
  hipLaunchKernelGGL(ssv_cg_direction_kernel, grid, dim3(kSsvBlock), 0, stream, a, nb);
  hipLaunchKernelGGL(ssv_cg_advance_kernel, dim3(1), dim3(kSsvBlock), 0, stream, a, nb, chunks);
}

void launch_ssv_elem(const SsvElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(ssv_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(ssv_elem_kernel<true>, grid, dim3(kSsvBlock), 0, stream, a);
  else hipLaunchKernelGGL(ssv_elem_kernel<false>, grid, dim3(kSsvBlock), 0, stream, a);
}

void launch_ssv_fin(const SsvFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(ssv_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_svm {
  hipStream_t stream = nullptr;
  DevMem mem;
  SparseDev sp;
  int device = 0;
  int64_t m = 0, n = 0, nnz = 0;
  int32_t K = 0, chunks = 0, nwg = 0;
  double C = 0.0;
  // multi-vectors, [chunks][len][kSpmmChunk]
  double *X = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr, *Y = nullptr;              // len n
  double *Z = nullptr, *U = nullptr, *ELL = nullptr, *V = nullptr, *T = nullptr;            // len m (T: D p and D x)
  double *cgpart = nullptr, *part = nullptr;
  double *W = nullptr, *CC = nullptr;
  int32_t *loss = nullptr, *chunk_cost = nullptr, *alldone = nullptr;
  SsvCg* cg = nullptr;
  OvrRec* rec = nullptr;
  std::vector<int32_t> loss_host;
  std::vector<double> cost_host;
  struct Poll {  // pinned
    int32_t alldone, longest;
  }* poll = nullptr;
  OvrRec* rec_host = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double *pnorm = nullptr, *perr = nullptr, *hnorm = nullptr, *objv = nullptr;  // [K][hist_ld]
  int32_t hist_ld = 0;
  int cg_batch = 8;  // inner iterations enqueued between two polls of the all-done word
  bool has_run = false;
  admm_sparse_svm_options last{};
  std::vector<int32_t> steps;
};

namespace {

template <class T>
int ssv_alloc_words(admm_sparse_svm* o, T** out, size_t count) {
  double* raw = nullptr;
  ADMM_TRY(o->mem.alloc(&raw, (count * sizeof(T) + 7) / 8));
  ADMM_HIP_TRY(hipMemsetAsync(raw, 0, (count * sizeof(T) + 7) / 8 * 8, o->stream));
  *out = reinterpret_cast<T*>(raw);
  return ADMM_OK;
}

// column-major host matrix (rows x K), or zeros, into a chunked multi-vector
int ssv_upload(admm_sparse_svm* o, double* dst, const double* src, int64_t rows) {
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

// svm_ovr.hip's rule: a chunk takes the cost form with weights, a class cost != 1 or the squared hinge
int ssv_plan_cost(admm_sparse_svm* o) {
  std::vector<int32_t> cc(static_cast<size_t>(o->chunks), 0);
  for (int32_t c = 0; c < o->K; ++c)
    if (o->W || o->loss_host[c] == ADMM_LOSS_SQHINGE || o->cost_host[2 * c] != 1.0 || o->cost_host[2 * c + 1] != 1.0)
      cc[c / kSpmmChunk] = 1;
  ADMM_HIP_TRY(hipMemcpyAsync(o->chunk_cost, cc.data(), sizeof(int32_t) * o->chunks, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  return ADMM_OK;
}

int ssv_setup(admm_sparse_svm* o, const admm_sparse_svm_desc* desc, const admm_sparse_desc* D) {
  ADMM_HIP_TRY(hipSetDevice(desc->device));
  o->device = desc->device;
  ADMM_HIP_TRY(hipStreamCreate(&o->stream));
  ADMM_TRY(sparse_device_build(D, &o->sp, o->stream));
  const int64_t m = D->rows, n = D->cols;
  const int32_t K = desc->K;
  o->m = m;
  o->n = n;
  o->nnz = D->nnz;
  o->K = K;
  o->chunks = spmm_chunks(K);
  o->nwg = ssv_vec_workgroups(m);
  o->C = desc->C;
  const size_t kp = static_cast<size_t>(o->chunks) * kSpmmChunk;
  for (double** p : {&o->X, &o->R, &o->P, &o->Q, &o->Y}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  for (double** p : {&o->Z, &o->U, &o->ELL, &o->V, &o->T}) {
    ADMM_TRY(o->mem.alloc(p, kp * m));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * m, o->stream));
  }
  ADMM_TRY(ssv_upload(o, o->ELL, desc->ELL, m));
  ADMM_TRY(o->mem.alloc(&o->cgpart, kp * 2 * kSsvMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->cgpart, 0, sizeof(double) * kp * 2 * kSsvMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->part, kp * OV_COUNT * kSsvMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * kp * OV_COUNT * kSsvMaxWg, o->stream));
  ADMM_TRY(ssv_alloc_words(o, &o->loss, static_cast<size_t>(K)));
  ADMM_TRY(ssv_alloc_words(o, &o->chunk_cost, static_cast<size_t>(o->chunks)));
  ADMM_TRY(ssv_alloc_words(o, &o->alldone, 2));
  ADMM_TRY(ssv_alloc_words(o, &o->cg, static_cast<size_t>(K)));
  ADMM_TRY(ssv_alloc_words(o, &o->rec, static_cast<size_t>(K)));
  o->loss_host.assign(static_cast<size_t>(K), ADMM_LOSS_HINGE);
  if (desc->loss)
    for (int32_t c = 0; c < K; ++c) o->loss_host[c] = desc->loss[c];
  ADMM_HIP_TRY(hipMemcpyAsync(o->loss, o->loss_host.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->cost_host.assign(static_cast<size_t>(2 * K), 1.0);
  ADMM_TRY(o->mem.alloc(&o->CC, static_cast<size_t>(2 * K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, o->cost_host.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(ssv_plan_cost(o));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&o->poll), sizeof(*o->poll)));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&o->rec_host), sizeof(OvrRec) * K));
  ADMM_HIP_TRY(hipEventCreate(&o->ev0));
  ADMM_HIP_TRY(hipEventCreate(&o->ev1));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  return ADMM_OK;
}

SpmmMask ssv_mask(const admm_sparse_svm* o, bool with_cg) {
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

// X <- the CG solution of D'D x = Y for every running class; the host polls the all-done word once per batch
int ssv_solve(admm_sparse_svm* o, const SsvCgArgs& a, bool first) {
  const SpmmMask run = ssv_mask(o, false), live = ssv_mask(o, true);
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
  // (a batch as long as the last solve took, as cg_solve sizes its own: one or two polls per solve)
  o->cg_batch = std::min(64, std::max(4, static_cast<int>(o->poll->longest) + 2));
  return ADMM_OK;
}

}  // namespace

static_assert(offsetof(SsvCg, done) == kSsvDoneWord * sizeof(int32_t), "SpmmMask reads the done word");
static_assert(offsetof(OvrRec, stop) == 0, "SpmmMask reads the stop word");

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
  if (!desc->D) return fail(ADMM_E_INVALID, "the sparse linear SVM needs D (admm_sparse_desc)");
  if (desc->D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, "the sparse linear SVM takes D in host arrays");
  ADMM_TRY(sparse_csc_check(desc->D));
  if (!desc->ELL) return fail(ADMM_E_INVALID, "the linear SVM needs the label matrix ELL (m x K)");
  if (!(desc->C >= 0.0) || !finite_nonneg(desc->C))
    return fail(ADMM_E_INVALID, "Given regularization parameter C is not a nonnegative number!");
  if (desc->loss)
    for (int32_t c = 0; c < desc->K; ++c)
      if (desc->loss[c] != ADMM_LOSS_HINGE && desc->loss[c] != ADMM_LOSS_01 && desc->loss[c] != ADMM_LOSS_HINGE_OBJ01 &&
          desc->loss[c] != ADMM_LOSS_LOGISTIC && desc->loss[c] != ADMM_LOSS_SQHINGE)
        return fail(ADMM_E_INVALID, "bad loss for class " + std::to_string(c));
  const int64_t mk = desc->D->rows * static_cast<int64_t>(desc->K);
  for (int64_t i = 0; i < mk; ++i)
    if (desc->ELL[i] != 1.0 && desc->ELL[i] != -1.0)
      return fail(ADMM_E_INVALID, "a label of class " + std::to_string(i / desc->D->rows) + " is neither +1 nor -1");
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, "the sparse one-vs-rest linear SVM is not row-sharded");
  int ndev = 0;
  ADMM_TRY(admm_device_count(&ndev));
  if (ndev <= 0) return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  if (desc->device < 0 || desc->device >= ndev) return fail(ADMM_E_INVALID, "bad device ordinal");
  admm_sparse_svm* o = new admm_sparse_svm();
  const int rc = ssv_setup(o, desc, desc->D);
  if (rc != ADMM_OK) {
    const std::string msg = admm_last_error();
    admm_sparse_svm_destroy(o);
    return fail(rc, msg);
  }
  *out = o;
  return ADMM_OK;
}

int admm_sparse_svm_run(admm_sparse_svm* o, const admm_sparse_svm_options* opts, admm_sparse_svm_summary* summaries,
                        double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_svm_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_svm_options.struct_size mismatch (ABI version skew)");
  admm_sparse_svm_options op = *opts;
  if (op.fast != ADMM_FAST_OFF)
    return fail(ADMM_E_UNSUPPORTED, "fast / accelerated ADMM is not part of the sparse one-vs-rest loop");
  if (op.relax != 1.0) return fail(ADMM_E_UNSUPPORTED, "relaxation is not part of the sparse one-vs-rest loop");
  if (op.convtest) return fail(ADMM_E_UNSUPPORTED, "convtest is not part of the sparse one-vs-rest loop");
  if (!(op.rho > 0.0)) return fail(ADMM_E_INVALID, "options.rho must be positive");
  if (op.maxiters <= 0) op.maxiters = 1000;  // admm.m:334-339
  if (!(op.cg_tol > 0.0)) op.cg_tol = 1e-12;
  if (op.cg_maxit <= 0) op.cg_maxit = 200;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  if (o->hist_ld != N) {
    for (double** p : {&o->pnorm, &o->perr, &o->hnorm, &o->objv}) {
      o->mem.free_one(*p);
      *p = nullptr;
      ADMM_TRY(o->mem.alloc(p, static_cast<size_t>(N) * K));
    }
    o->hist_ld = N;
  }
  o->has_run = false;
  ADMM_HIP_TRY(hipMemsetAsync(o->rec, 0, sizeof(OvrRec) * K, o->stream));
  ADMM_HIP_TRY(hipMemsetAsync(o->cg, 0, sizeof(SsvCg) * K, o->stream));
  ADMM_TRY(ssv_upload(o, o->X, nullptr, o->n));  // (x0 is never read: the first x-update starts CG from 0)
  ADMM_TRY(ssv_upload(o, o->Z, op.z0, o->m));
  ADMM_TRY(ssv_upload(o, o->U, op.u0, o->m));

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
  SsvElemArgs ea{};
  ea.m = o->m;
  ea.AX = o->T;
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
  fa.X = o->X;
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
  const SpmmMask run = ssv_mask(o, false);
  const int check_every = op.check_every > 0 ? op.check_every : (op.domaxiters ? 64 : 8);
  o->cg_batch = 8;  // (a run never depends on the one before it)

  ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
  launch_ssv_elem(ea, true, o->stream);  // V = z0 - u0
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    launch_spmm(o->sp.t, o->V, o->Y, o->chunks, run, o->stream);  // y = D'(z - u)
    ADMM_TRY(ssv_solve(o, ca, it == 0));
    launch_spmm(o->sp.n, o->X, o->T, o->chunks, run, o->stream);  // D x
    launch_ssv_elem(ea, false, o->stream);
    launch_ssv_fin(fa, o->stream);
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
  if (!all) return fail(ADMM_E_DEVICE, "the sparse one-vs-rest loop ended with classes still running");
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

int admm_sparse_svm_set_cost(admm_sparse_svm* o, const double* weights, const double* class_cost) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  ADMM_TRY(check_svm_cost(weights, o->m, class_cost, 2 * static_cast<int64_t>(o->K)));  // (a refused call changes nothing)
  ADMM_HIP_TRY(hipSetDevice(o->device));
  double* w = nullptr;
  if (weights) {
    ADMM_TRY(o->mem.alloc(&w, static_cast<size_t>(o->m)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, weights, sizeof(double) * o->m, hipMemcpyHostToDevice, o->stream));
  }
  std::vector<double> cc(static_cast<size_t>(2 * o->K), 1.0);
  if (class_cost) cc.assign(class_cost, class_cost + 2 * o->K);
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, cc.data(), sizeof(double) * 2 * o->K, hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the caller's buffers are read until here)
  if (o->W) o->mem.free_one(o->W);
  o->W = w;
  o->cost_host = cc;
  return ssv_plan_cost(o);
}

int admm_sparse_svm_fetch(admm_sparse_svm* o, int field, double* dst, size_t cap, size_t* written) {
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
    case ADMM_OVR_F_XOPT: return matrix(o->X, o->n);
    case ADMM_OVR_F_ZOPT: return matrix(o->Z, o->m);
    case ADMM_OVR_F_UOPT: return matrix(o->U, o->m);
    case ADMM_OVR_F_PNORM: return history(o->pnorm);
    case ADMM_OVR_F_PERR: return history(o->perr);
    case ADMM_OVR_F_HNORMSQ: return history(o->hnorm);
    case ADMM_OVR_F_OBJEVALS:
      if (!o->last.objevals) return fail(ADMM_E_INVALID, "the last run did not evaluate the objective (objevals = 0)");
      return history(o->objv);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse one-vs-rest linear SVM");
  }
}

void admm_sparse_svm_destroy(admm_sparse_svm* o) {
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
