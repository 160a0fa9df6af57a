// sparse_l1class.hip -- sparse linear classifiers on a SPARSE design matrix, K fits at once over one D:
// l1class.hip's iteration (q42: the lasso's penalty family on the linear SVM's losses, plain ADMM with A = [D; I_n],
// B = -1, c = 0, z = [z1 (m); z2 (n)], stopcond 'standard') with the one difference of the sparse objects, the x-update:
//   x  = (D'D + I)^-1 y,  y = D'(z1 - u1) + (z2 - u2)     spmm_cg.hip's lock-step CG with the shift 1, whatever rho is:
//                                                          nothing n x n, positive definite for every D
//   z1 = prox of (C*c/rho)*phi at (D x + u1)              svm_cost_device.h
//   z2 = kappa*penalty_elem(x + u2, (lambda/rho)*w)       l1class_device.h: the dense object's element update
//   u += A x - z
// The first solve of a run starts from 0 and every later one from the previous x.  Every multi-vector, of length m as of
// length n, has spmm.h's layout [chunks][len][kSpmmChunk].  Per iteration, every launch for all K fits at once
// (blockIdx.y = chunk of kSpmmChunk fits):
//   SpmmCg::solve                 two SpMM and four small launches per inner iteration
//   T = D X                       one SpMM
//   sl1c_row_kernel               over m: z1, u1, T1 = z1 - u1 (and z1 - z1prev with the dual residual), the m-block's sums
//   G = D'T1                      one SpMM; with the dual residual two more: D'(z1 - z1prev) and D'u1
//   sl1c_elem_kernel              over n: z2, u2, the next Y = G + (z2 - u2), the n-block's sums, the dual residual's two
//                                 norms, the penalty
//   l1c_fin_kernel                l1class.hip's, per fit: pnorm, perr, dnorm, derr, the objective, the stop decision
// With groups set (admm_sparse_l1class_set_groups, q48) the element kernel is sl1c_group_elem_kernel, the shared body of
// l1class_group_device.h over the plan's workgroups; nothing else of the iteration changes (D'D + I holds no penalty).
// With folds set (admm_sparse_l1class_set_folds, q47) fit k's cost on row i is 0 where fold_i = held_k -- a select in the
// row kernel's FOLD instantiation; D'D + I holds no cost, so nothing else of the iteration changes -- and behind the loop
// one product T = D Z2 over every fit and sl1c_heldout_kernel give the held-out loss, weighted errors and weight.
// A fit whose stop flag is set is FROZEN, and a fit whose solve is done is masked until the next solve: every kernel and
// every product skips it.  No atomics; every sum runs in an order the sizes fix: two runs give the same bits, and a fit
// gets the same numbers wherever it lands.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "l1class_device.h"
#include "l1class_group_device.h"
#include "multi_host.h"
#include "softmax_device.h"
#include "spmm_cg.h"
#include "svm_cost_device.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

struct Sl1cRowArgs {
  int64_t m;
  const double* AX;    // D X
  double *Z1, *U1;     // multi-vectors of len m
  double *T1, *DZ1;    // z1 - u1; z1 - z1prev (null without the dual residual)
  const double* ELL;   // a multi-vector of len m, or column 0 of ONE chunk (ell_shared)
  const double* W;     // m weights or null
  const double* CC;    // K x 2 class costs
  const int32_t* loss;
  const MultiRec* rec;
  double* part;        // [fit][LM_COUNT][kScgMaxWg]
  int32_t K, ell_shared, objevals;
  double rho, C;
  // held-out folds (admm_sparse_l1class_set_folds, q47), read by the FOLD instantiation alone; behind every other member,
  // so that the kernels without folds load their arguments from the offsets they always had
  const int32_t* fold;  // m fold ids, or null: no folds
  const int32_t* held;  // K values: the fold fit k holds out, or -1
  // the multinomial model (admm_sparse_l1class_set_multinomial, q49), read by the launcher alone: 0, or the classes Cn
  int32_t classes;
};

// the sums of the held-out pass over m (q47), per fit over the rows with fold_i = held_k, c = w_i * class cost: the loss
// sum c*phi(ell*t) without the factor C, the weighted errors sum c*[ell*t <= 0] and the weight sum c
enum Sl1cHeldSlot : int32_t { LH_LOSS = 0, LH_ERR = 1, LH_W = 2, LH_COUNT = 3 };

struct Sl1cHeldArgs {
  int64_t m;
  const double* T;     // D Z2
  const double* ELL;   // as Sl1cRowArgs
  const double* W;     // m weights or null
  const double* CC;    // K x 2 class costs
  const int32_t* loss;
  const int32_t* fold;  // m fold ids (never null)
  const int32_t* held;  // K values
  const MultiRec* rec;
  double* part;        // [fit][LH_COUNT][kScgMaxWg]
  int32_t K, ell_shared;
};

struct Sl1cElemArgs {
  int64_t n;
  const double* X;      // multi-vectors of len n
  double *Z2, *U2, *Y;
  const double *G, *GDZ, *GU;  // D'(z1 - u1), D'(z1 - z1prev), D'u1
  const double* W;      // n l1 weights or null
  const double* par;    // K x 2: (lambda, mu)
  const int32_t* nonneg;
  const MultiRec* rec;
  double* part;         // [fit][LN_COUNT][kScgMaxWg]
  int32_t K, dual, objevals;
  double rho;
};

// thread t: row t / KC of a row block, fit t % KC of the chunk (scg_lane).  INIT: only T1 = z1 - u1 of the start vectors.
// FOLD (q47): the row's weight is +0.0 where the fit holds the row's fold out -- a select in front of svm_cost_of, so the
// cost is 0 and the prox returns D x + u1 bit for bit; 4 B more per row, one word per thread in front of the loop
template <bool INIT, bool FOLD = false>
__global__ __launch_bounds__(kScgBlock) void sl1c_row_kernel(Sl1cRowArgs a) {
  __shared__ double lds[LM_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[LM_COUNT];
#pragma unroll
  for (int q = 0; q < LM_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const SvmCostArgs ks{nullptr, a.CC[2 * fit], a.CC[2 * fit + 1], a.C, a.rho, a.loss[fit], a.objevals};
  int32_t hk = -1;
  if constexpr (FOLD) hk = a.held[fit];
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (!l.run || i >= a.m) continue;
    const int64_t e = base + i * KC + l.c;
    const double zp = a.Z1[e], uo = a.U1[e];
    if constexpr (INIT) {
      a.T1[e] = (0.0 + zp) - uo;
    } else {
      const double ax = a.AX[e];
      const double el = a.ell_shared ? a.ELL[i * KC] : a.ELL[e];
      double wv = a.W ? a.W[i] : 1.0;
      if constexpr (FOLD) wv = (hk == a.fold[i]) ? 0.0 : wv;
      const double ci = svm_cost_of(ks, wv, el);
      const double zn = svm_cost_prox_elem<true>(ks, ci, el, ax + uo);
      const double rr = ax - zn;      // A x + B z - c
      const double un = uo + rr;      // admm.m:542-550
      acc[LM_R2] += rr * rr;
      acc[LM_AX2] += ax * ax;
      acc[LM_Z2] += zn * zn;
      if (a.objevals) acc[LM_LOSS] += svm_cost_obj_elem<true>(ks, ci, el * ax);
      a.Z1[e] = zn;
      a.U1[e] = un;
      a.T1[e] = zn - un;
      if (a.DZ1) a.DZ1[e] = zn - zp;
    }
  }
  if (INIT) return;
  scg_sums<LM_COUNT>(acc, lds, a.part, LM_COUNT, 0);
}

// The multinomial form (q49), CN classes per model and KC / CN models per chunk: model p of a chunk owns the slots
// [p*CN, (p + 1)*CN).  The same grid, thread layout and sums.  The row's values of D x + u1, of D x and of the labels go
// through LDS; the thread of a model's first slot solves the row prox of its CN values (softmax_device.h) -- its cost is
// w_i times the class weight CC[2 k] of the true class's fit k -- writes z1 back to LDS and keeps the model's loss;
// behind the barrier every thread finishes its own element as the per-fit kernel does.  The other classes add +0.0 to
// the loss slot.  The slots behind the chunk's last model are stopped from the start of a run and idle here.
template <int CN>
__global__ __launch_bounds__(kScgBlock) void sl1c_row_multinomial_kernel(Sl1cRowArgs a) {
  __shared__ double lds[LM_COUNT * kScgBlock];
  __shared__ double sv[kScgBlock], sx[kScgBlock], se[kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int tid = threadIdx.x;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[LM_COUNT];
#pragma unroll
  for (int q = 0; q < LM_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const bool lead = l.run && l.c % CN == 0 && l.c + CN <= KC;
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {  // (uniform over the workgroup: the barriers are too)
    const int64_t i = rb * kScgRows + l.r;
    const bool on = l.run && i < a.m;
    const int64_t e = base + i * KC + l.c;
    double zp = 0.0, uo = 0.0, ax = 0.0;
    if (on) {
      zp = a.Z1[e];
      uo = a.U1[e];
      ax = a.AX[e];
      sv[tid] = ax + uo;
      sx[tid] = ax;
      se[tid] = a.ELL[e];
    }
    __syncthreads();
    if (lead && on) {
      double v[CN], z[CN];
      int y = 0;
#pragma unroll
      for (int k = 0; k < CN; ++k) {
        v[k] = sv[tid + k];
        y = se[tid + k] > 0.0 ? k : y;
      }
      const double ci = (a.W ? a.W[i] : 1.0) * a.CC[2 * (fit + y)];
      softmax_prox<CN>(v, y, (a.C * ci) / a.rho, z);
#pragma unroll
      for (int k = 0; k < CN; ++k) sv[tid + k] = z[k];
      if (a.objevals) {
#pragma unroll
        for (int k = 0; k < CN; ++k) v[k] = sx[tid + k];
        acc[LM_LOSS] += ci * softmax_loss<CN>(v, y);
      }
    }
    __syncthreads();
    if (on) {
      const double zn = sv[tid];
      const double rr = ax - zn;  // A x + B z - c
      const double un = uo + rr;  // admm.m:542-550
      acc[LM_R2] += rr * rr;
      acc[LM_AX2] += ax * ax;
      acc[LM_Z2] += zn * zn;
      a.Z1[e] = zn;
      a.U1[e] = un;
      a.T1[e] = zn - un;
      if (a.DZ1) a.DZ1[e] = zn - zp;
    }
  }
  scg_sums<LM_COUNT>(acc, lds, a.part, LM_COUNT, 0);
}

// one workgroup per model (blockIdx.x = chunk * (KC / CN) + model of the chunk): l1c_model_fin_body
__global__ __launch_bounds__(kL1cModelFinThreads) void sl1c_model_fin_kernel(L1cFinArgs a, int32_t classes) {
  const int per = KC / classes;
  const int fit0 = (static_cast<int>(blockIdx.x) / per) * KC + (static_cast<int>(blockIdx.x) % per) * classes;
  if (fit0 + classes > a.K) return;
  l1c_model_fin_body(a, fit0, classes);
}

// blockIdx.x * blockDim.x + threadIdx.x = row: the row prox alone (admm_op_softmax_prox)
template <int CN>
__global__ __launch_bounds__(kBlock) void softmax_prox_op_kernel(const double* __restrict__ V, const int32_t* __restrict__ y,
                                                                 const double* __restrict__ av, int64_t m,
                                                                 double* __restrict__ out, int32_t* __restrict__ iters) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= m) return;
  double v[CN], z[CN];
#pragma unroll
  for (int k = 0; k < CN; ++k) v[k] = V[i * CN + k];
  iters[i] = softmax_prox<CN>(v, y[i], av[i], z);
#pragma unroll
  for (int k = 0; k < CN; ++k) out[i * CN + k] = z[k];
}

// f.template operator()<CN>() for the run-time classes in 2 .. KC
template <class F>
void with_classes(int32_t classes, F f) {
  switch (classes) {
    case 2: return f.template operator()<2>();
    case 3: return f.template operator()<3>();
    case 4: return f.template operator()<4>();
    case 5: return f.template operator()<5>();
    case 6: return f.template operator()<6>();
    case 7: return f.template operator()<7>();
    case 8: return f.template operator()<8>();
    case 9: return f.template operator()<9>();
    default: return f.template operator()<10>();
  }
}
static_assert(KC == 10, "with_classes lists the class counts of one chunk");

struct RowMultinomialLaunch {
  const Sl1cRowArgs& a;
  dim3 grid;
  hipStream_t stream;
  template <int CN>
  void operator()() const {
    hipLaunchKernelGGL(sl1c_row_multinomial_kernel<CN>, grid, dim3(kScgBlock), 0, stream, a);
  }
};

struct ProxOpLaunch {
  const double* V;
  const int32_t* y;
  const double* av;
  int64_t m;
  double* out;
  int32_t* iters;
  template <int CN>
  void operator()() const {
    hipLaunchKernelGGL(softmax_prox_op_kernel<CN>, dim3(static_cast<unsigned>((m + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       nullptr, V, y, av, m, out, iters);
  }
};

// behind the loop, at T = D Z2 (q47): the three held-out sums of EVERY fit, stopped or not, in the row kernel's thread
// layout and scg_sums' order.  A row the fit does not hold out adds +0.0 by a select; held = -1 matches no fold id
__global__ __launch_bounds__(kScgBlock) void sl1c_heldout_kernel(Sl1cHeldArgs a) {
  __shared__ double lds[LH_COUNT * kScgBlock];
  ScgLane l = scg_lane(a.rec, a.K);
  l.run = l.fit < a.K;
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.m * KC;
  double acc[LH_COUNT] = {0.0, 0.0, 0.0};
  const int fit = l.run ? l.fit : 0;
  const SvmCostArgs ks{nullptr, a.CC[2 * fit], a.CC[2 * fit + 1], 1.0, 1.0, a.loss[fit], 1};
  const int32_t hk = a.held[fit];
  const int64_t nrb = (a.m + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (!l.run || i >= a.m) continue;
    const int64_t e = base + i * KC + l.c;
    const double el = a.ell_shared ? a.ELL[i * KC] : a.ELL[e];
    const double wv = a.W ? a.W[i] : 1.0;
    const double ci = svm_cost_of(ks, wv, el);
    const double q = el * a.T[e];
    const bool out = a.fold[i] == hk;
    const double lv = svm_cost_obj_elem<true>(ks, ci, q);
    acc[LH_LOSS] += out ? lv : 0.0;
    acc[LH_ERR] += (out && q <= 0.0) ? ci : 0.0;
    acc[LH_W] += out ? ci : 0.0;
  }
  scg_sums<LH_COUNT>(acc, lds, a.part, LH_COUNT, 0);
}

// blockIdx.x = fit: the three held-out totals in multi_slot_totals' order
__global__ __launch_bounds__(kBlock) void sl1c_heldout_total_kernel(const double* part, int32_t nwg_m, double* heldout) {
  __shared__ double S[8];
  const int fit = blockIdx.x;
  multi_slot_totals(part, fit, LH_COUNT, nwg_m, S);
  __syncthreads();
  if (threadIdx.x < LH_COUNT) heldout[LH_COUNT * fit + threadIdx.x] = S[threadIdx.x];
}

// the same thread layout over n.  INIT: only Y = D'(z1 - u1) + (z2 - u2) of the start vectors
template <bool INIT>
__global__ __launch_bounds__(kScgBlock) void sl1c_elem_kernel(Sl1cElemArgs a) {
  __shared__ double lds[LN_COUNT * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[LN_COUNT];
#pragma unroll
  for (int q = 0; q < LN_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const double lam = a.par[2 * fit], mu = a.par[2 * fit + 1];
  // engine_run_general.hip's own expressions for the family's numbers
  const PenaltyArgs pen{a.W, lam / a.rho, a.rho / (a.rho + mu), lam, 0.0, 0.5 * mu, a.nonneg[fit]};
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t j = rb * kScgRows + l.r;
    if (!l.run || j >= a.n) continue;
    const int64_t e = base + j * KC + l.c;
    l1c_elem_update<INIT>(pen, a.X, a.Z2, a.U2, a.Y, e, j, a.G, a.GDZ, a.GU, e, a.dual, a.objevals, acc);
  }
  if (INIT) return;
  scg_sums<LN_COUNT>(acc, lds, a.part, LN_COUNT, 0);
}

// the grouped form (q48): l1class_group_device.h's body; g1, g2, g3 are multi-vectors of len n
__global__ __launch_bounds__(kScgBlock) void sl1c_group_elem_kernel(L1cGroupElemArgs a, GroupPlan gp,
                                                                    const double* __restrict__ G,
                                                                    const double* __restrict__ GDZ,
                                                                    const double* __restrict__ GU) {
  __shared__ double lds[kL1cGroupLds];
  __shared__ double sq[kScgBlock];
  __shared__ double gacc[kGmMaxGroups * KC];
  l1c_group_elem_body(
      a, gp,
      [&](int q, const ScgLane& l, int64_t base, int64_t j) {
        const double* __restrict__ g = q == 0 ? G : (q == 1 ? GDZ : GU);
        return g[base + j * KC + l.c];
      },
      lds, sq, gacc);
}

void launch_sl1c_row(const Sl1cRowArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(sl1c_row_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
  else if (a.classes) with_classes(a.classes, RowMultinomialLaunch{a, grid, stream});
  else if (a.fold) hipLaunchKernelGGL((sl1c_row_kernel<false, true>), grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL(sl1c_row_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
}

void launch_sl1c_model_fin(const L1cFinArgs& a, int32_t classes, hipStream_t stream) {
  const unsigned models = static_cast<unsigned>(spmm_chunks(a.K) * (KC / classes));
  hipLaunchKernelGGL(sl1c_model_fin_kernel, dim3(models), dim3(kL1cModelFinThreads), 0, stream, a, classes);
}

void launch_sl1c_heldout(const Sl1cHeldArgs& a, int32_t nwg_m, double* heldout, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.m), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(sl1c_heldout_kernel, grid, dim3(kScgBlock), 0, stream, a);
  hipLaunchKernelGGL(sl1c_heldout_total_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kBlock), 0, stream, a.part, nwg_m,
                     heldout);
}

void launch_sl1c_elem(const Sl1cElemArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(scg_vec_workgroups(a.n), static_cast<unsigned>(spmm_chunks(a.K)));
  if (init) hipLaunchKernelGGL(sl1c_elem_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL(sl1c_elem_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
}

// the iteration form of the element update the object would run: grouped with groups set (the INIT form needs none)
void launch_sl1c_elem_iter(const Sl1cElemArgs& a, const GroupMulti& gm, hipStream_t stream) {
  if (!gm.on()) return launch_sl1c_elem(a, false, stream);
  const L1cGroupElemArgs ga{a.n, a.X, a.Z2, a.U2, a.Y, a.W, a.par, gm.l1, a.nonneg, a.rec, a.part, a.K, a.dual, a.objevals,
                            a.rho};
  const dim3 grid(static_cast<unsigned>(gm.plan.nwg), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(sl1c_group_elem_kernel, grid, dim3(kScgBlock), 0, stream, ga, gm.plan, a.G, a.GDZ, a.GU);
}

}  // namespace

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_sparse_l1class : admm::MultiHost {
  admm::SpmmCg cg;  // D, the x-update and its multi-vectors
  int64_t m = 0, n = 0;
  int32_t nwg_m = 0, nwg_n = 0, ell_shared = 0;
  double C = 1.0;
  double *Z1 = nullptr, *U1 = nullptr, *T1 = nullptr, *DZ1 = nullptr, *ELL = nullptr;  // len m (ELL: or one chunk)
  double *Z2 = nullptr, *U2 = nullptr, *G = nullptr, *GDZ = nullptr, *GU = nullptr;    // len n
  double *mpart = nullptr, *npart = nullptr;
  double *W = nullptr, *CC = nullptr, *LW = nullptr, *par = nullptr;
  int32_t *loss = nullptr, *nonneg = nullptr;
  std::vector<double> cost_host;
  // admm_sparse_l1class_set_folds (q47); fold null: the object without folds
  int32_t *fold = nullptr, *held = nullptr;  // m fold ids; K values (-1: nothing held out)
  double *hpart = nullptr, *held_dev = nullptr;  // the held-out pass's own partials; K x LH_COUNT totals
  std::vector<double> held_host;  // the same on the host; empty: no run under folds behind the object
  admm::GroupMulti grp;  // admm_sparse_l1class_set_groups (q48)
  // admm_sparse_l1class_set_multinomial (q49); classes 0: the per-fit object.  start: the records a run starts from, the
  // idle slots behind a chunk's last model stopped
  int32_t classes = 0;
  std::vector<admm::MultiRec> start;
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  admm_sparse_l1class_options last{};
};

namespace {

using namespace admm;

const char* kWho = "the sparse l1 classifier";

int sl1c_setup(admm_sparse_l1class* o, const admm_sparse_l1class_desc* desc, const std::vector<double>& ph,
               const std::vector<int32_t>& nh, const std::vector<int32_t>& lh) {
  const int32_t K = desc->K;
  o->K = K;
  ADMM_TRY(o->cg.build(o, desc->device, desc->D));
  const int64_t m = o->cg.m, n = o->cg.n;
  o->m = m;
  o->n = n;
  o->C = desc->C;
  o->nwg_m = scg_vec_workgroups(m);
  o->nwg_n = scg_vec_workgroups(n);
  const size_t kp = static_cast<size_t>(o->cg.chunks) * KC;
  for (double** p : {&o->Z1, &o->U1, &o->T1, &o->DZ1}) {
    ADMM_TRY(o->mem.alloc(p, kp * m));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * m, o->stream));
  }
  for (double** p : {&o->Z2, &o->U2, &o->G, &o->GDZ, &o->GU}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  {  // the labels in the layout of the products: the shared column is column 0 of one chunk
    o->ell_shared = desc->nell == 1 && K > 1 ? 1 : 0;
    const int32_t ecols = o->ell_shared ? 1 : K;
    const size_t ep = static_cast<size_t>(spmm_chunks(ecols)) * KC;
    ADMM_TRY(o->mem.alloc(&o->ELL, ep * m));
    std::vector<double> hb(ep * m);
    spmm_pack(desc->ELL, m, m, ecols, hb.data());
    ADMM_HIP_TRY(hipMemcpyAsync(o->ELL, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hb goes out of scope)
  }
  ADMM_TRY(o->mem.alloc(&o->mpart, kp * LM_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->mpart, 0, sizeof(double) * kp * LM_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->npart, kp * LN_COUNT * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->npart, 0, sizeof(double) * kp * LN_COUNT * kScgMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(2) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_words(*o, &o->nonneg, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->nonneg, nh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_words(*o, &o->loss, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->loss, lh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->cost_host.assign(static_cast<size_t>(2 * K), 1.0);
  ADMM_TRY(o->mem.alloc(&o->CC, static_cast<size_t>(2 * K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, o->cost_host.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the host vectors and the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  if (desc->l1weights) ADMM_TRY(set_shared_weights(*o, n, desc->l1weights, &o->LW));
  return ADMM_OK;
}

// host (m + n) x K column-major <-> V1 (len m) above V2 (len n), both chunked multi-vectors
int sl1c_upload_stacked(admm_sparse_l1class* o, const double* src, double* V1, double* V2) {
  if (!src) {
    ADMM_TRY(o->cg.upload(V1, nullptr, o->m));
    return o->cg.upload(V2, nullptr, o->n);
  }
  const int64_t mn = o->m + o->n;
  const size_t kp = static_cast<size_t>(o->cg.chunks) * KC;
  std::vector<double> h1(kp * o->m), h2(kp * o->n);
  spmm_pack(src, mn, o->m, o->K, h1.data());
  spmm_pack(src + o->m, mn, o->n, o->K, h2.data());
  ADMM_HIP_TRY(hipMemcpyAsync(V1, h1.data(), sizeof(double) * h1.size(), hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipMemcpyAsync(V2, h2.data(), sizeof(double) * h2.size(), hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (h1 and h2 go out of scope)
  return ADMM_OK;
}

int sl1c_fetch_stacked(admm_sparse_l1class* o, const double* V1, const double* V2, double* dst, size_t cap,
                       size_t* written) {
  const int64_t mn = o->m + o->n;
  const size_t need = static_cast<size_t>(mn) * o->K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  const size_t kp = static_cast<size_t>(o->cg.chunks) * KC;
  std::vector<double> h1(kp * o->m), h2(kp * o->n);
  ADMM_HIP_TRY(hipMemcpy(h1.data(), V1, sizeof(double) * h1.size(), hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(h2.data(), V2, sizeof(double) * h2.size(), hipMemcpyDeviceToHost));
  spmm_unpack(h1.data(), o->m, o->K, dst, mn);
  spmm_unpack(h2.data(), o->n, o->K, dst + o->m, mn);
  if (written) *written = need;
  return ADMM_OK;
}

// begin_run, and under the multinomial model the idle slots stopped before any kernel reads a record
int sl1c_begin_run(admm_sparse_l1class* o) {
  ADMM_TRY(begin_run(*o));
  if (o->classes) {
    ADMM_HIP_TRY(hipMemcpyAsync(o->rec, o->start.data(), sizeof(MultiRec) * o->K, hipMemcpyHostToDevice, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  }
  return ADMM_OK;
}

Sl1cRowArgs sl1c_row_args(const admm_sparse_l1class* o, bool dual, int32_t objevals, double rho) {
  Sl1cRowArgs a{};
  a.m = o->m;
  a.AX = o->cg.T;
  a.Z1 = o->Z1;
  a.U1 = o->U1;
  a.T1 = o->T1;
  a.DZ1 = dual ? o->DZ1 : nullptr;
  a.ELL = o->ELL;
  a.W = o->W;
  a.CC = o->CC;
  a.loss = o->loss;
  a.rec = o->rec;
  a.part = o->mpart;
  a.K = o->K;
  a.ell_shared = o->ell_shared;
  a.objevals = objevals;
  a.rho = rho;
  a.C = o->C;
  a.fold = o->fold;
  a.held = o->held;
  a.classes = o->classes;
  return a;
}

Sl1cElemArgs sl1c_elem_args(const admm_sparse_l1class* o, bool dual, int32_t objevals, double rho) {
  Sl1cElemArgs a{};
  a.n = o->n;
  a.X = o->cg.X;
  a.Z2 = o->Z2;
  a.U2 = o->U2;
  a.Y = o->cg.Y;
  a.G = o->G;
  a.GDZ = o->GDZ;
  a.GU = o->GU;
  a.W = o->LW;
  a.par = o->par;
  a.nonneg = o->nonneg;
  a.rec = o->rec;
  a.part = o->npart;
  a.K = o->K;
  a.dual = dual ? 1 : 0;
  a.objevals = objevals;
  a.rho = rho;
  return a;
}

}  // namespace

extern "C" {

void admm_sparse_l1class_desc_default(admm_sparse_l1class_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_sparse_l1class_desc);
  d->K = 1;
  d->nell = 1;
  d->C = 1.0;
  d->xsolve = ADMM_XSOLVE_AUTO;
}

void admm_sparse_l1class_options_default(admm_sparse_l1class_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_sparse_l1class_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->cg_tol = 1e-12;   // admm_problem_desc_default
  o->cg_maxit = 200;
  o->nodualerror = 0;  // admm.m:76
}

int admm_sparse_l1class_chunk(void) { return KC; }

int admm_sparse_l1class_create(const admm_sparse_l1class_desc* desc, admm_sparse_l1class** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_sparse_l1class_desc)))
    return fail(ADMM_E_INVALID, "admm_sparse_l1class_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the sparse l1 classifier needs at least one fit (K >= 1)");
  ADMM_TRY(check_sparse_D(kWho, desc->D));
  const int64_t m = desc->D->rows, n = desc->D->cols;
  if (!desc->ELL) return fail(ADMM_E_INVALID, "the sparse l1 classifier needs the labels ELL (rows x nell)");
  if (desc->nell != 1 && desc->nell != desc->K)
    return fail(ADMM_E_INVALID, "ELL has " + std::to_string(desc->nell) + " columns: one shared label column or one per "
                                "fit (" + std::to_string(desc->K) + ")");
  if (!desc->lambda) return fail(ADMM_E_INVALID, "the sparse l1 classifier needs lambda (K values)");
  if (!finite_pos(desc->C)) return fail(ADMM_E_INVALID, "desc.C must be positive and finite");
  std::vector<double> ph;
  std::vector<int32_t> nh, lh;
  ADMM_TRY(check_l1class_fits(desc->K, desc->loss, desc->lambda, desc->ridge, desc->nonneg, &lh, &ph, &nh));
  ADMM_TRY(check_labels(desc->ELL, m, desc->nell));
  ADMM_TRY(check_l1_weights(desc->l1weights, n));
  if (desc->xsolve != ADMM_XSOLVE_AUTO && desc->xsolve != ADMM_XSOLVE_CG)
    return fail(ADMM_E_UNSUPPORTED, "the sparse l1 classifier runs the matrix-free x-update (xsolve = auto or cg)");
  ADMM_TRY(check_placement(kWho, desc->comm, desc->device));
  return create_object(out, admm_sparse_l1class_destroy,
                       [&](admm_sparse_l1class* o) { return sl1c_setup(o, desc, ph, nh, lh); });
}

int admm_sparse_l1class_run(admm_sparse_l1class* o, const admm_sparse_l1class_options* opts,
                            admm_sparse_l1class_summary* summaries, double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_sparse_l1class_options)))
    return fail(ADMM_E_INVALID, "admm_sparse_l1class_options.struct_size mismatch (ABI version skew)");
  admm_sparse_l1class_options op = *opts;
  ADMM_TRY(check_sparse_run_options("sparse l1 classifier", &op));
  if (!finite_pos(op.rho)) return fail(ADMM_E_INVALID, "options.rho must be positive and finite");
  const bool dual = op.nodualerror == 0;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  SpmmCg& cg = o->cg;
  ADMM_TRY(sl1c_begin_run(o));
  ScgArgs ca{};
  ADMM_TRY(cg.begin_run(op.cg_tol, op.cg_maxit, &ca, 1.0));  // D'D + I: the shift is 1 for every rho
  ADMM_TRY(sl1c_upload_stacked(o, op.z0, o->Z1, o->Z2));
  ADMM_TRY(sl1c_upload_stacked(o, op.u0, o->U1, o->U2));

  const Sl1cRowArgs ra = sl1c_row_args(o, dual, op.objevals, op.rho);
  const Sl1cElemArgs ea = sl1c_elem_args(o, dual, op.objevals, op.rho);
  L1cFinArgs fa{};
  fa.mpart = o->mpart;
  fa.npart = o->npart;
  fa.m = o->m;
  fa.n = o->n;
  fa.K = K;
  fa.nwg_m = o->nwg_m;
  fa.nwg_n = o->grp.on() ? o->grp.plan.nwg : o->nwg_n;  // the plan's workgroups wrote the n-block's partials
  fa.dual = dual ? 1 : 0;
  fa.rec = o->rec;
  fa.pnorm = o->pnorm;
  fa.perr = o->perr;
  fa.dnorm = o->dnorm;
  fa.derr = o->derr;
  fa.objv = o->objv;
  fa.hist_ld = N;
  fa.rho = op.rho;
  fa.C = o->C;
  fa.abstol = op.abstol;
  fa.reltol = op.reltol;
  fa.domaxiters = op.domaxiters;
  fa.objevals = op.objevals;
  fa.maxiters = N;
  const SpmmMask run = cg.mask(false);

  ADMM_TRY(begin_timing(*o));
  launch_sl1c_row(ra, true, o->stream);                          // T1 = z1 - u1 of the start vectors
  launch_spmm(cg.sp.t, o->T1, o->G, cg.chunks, run, o->stream);  // G = D'T1
  launch_sl1c_elem(ea, true, o->stream);                         // y = G + (z2 - u2)
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    ADMM_TRY(cg.solve(ca, it == 0));
    launch_spmm(cg.sp.n, cg.X, cg.T, cg.chunks, run, o->stream);  // D x
    launch_sl1c_row(ra, false, o->stream);
    launch_spmm(cg.sp.t, o->T1, o->G, cg.chunks, run, o->stream);  // D'(z1 - u1)
    if (dual) {
      launch_spmm(cg.sp.t, o->DZ1, o->GDZ, cg.chunks, run, o->stream);  // D'(z1 - z1prev)
      launch_spmm(cg.sp.t, o->U1, o->GU, cg.chunks, run, o->stream);    // D'u1
    }
    launch_sl1c_elem_iter(ea, o->grp, o->stream);
    if (o->classes) launch_sl1c_model_fin(fa, o->classes, o->stream);
    else launch_l1c_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  o->held_host.clear();
  if (o->fold && all) {  // T = D z2 for every fit, stopped or not (z2: the sparse block df counts), and the held-out sums
    SpmmMask every;
    every.K = K;
    launch_spmm(cg.sp.n, o->Z2, cg.T, cg.chunks, every, o->stream);
    const Sl1cHeldArgs ha{o->m, cg.T, o->ELL, o->W, o->CC, o->loss, o->fold, o->held, o->rec, o->hpart, K, o->ell_shared};
    launch_sl1c_heldout(ha, o->nwg_m, o->held_dev, o->stream);
  }
  ADMM_TRY(finish_run(*o, all, "the sparse l1 classifier loop ended with fits still running", N, op.objevals != 0,
                      o->objv, runtime_s, summaries));
  if (o->fold) {
    o->held_host.resize(static_cast<size_t>(LH_COUNT) * K);
    ADMM_HIP_TRY(hipMemcpy(o->held_host.data(), o->held_dev, sizeof(double) * o->held_host.size(), hipMemcpyDeviceToHost));
  }
  for (int32_t c = 0; summaries && c < K; ++c) summaries[c].xsolve = ADMM_XSOLVE_CG;
  return end_sparse_run(o, op, summaries);
}

int admm_sparse_l1class_set_cost(admm_sparse_l1class* o, const double* weights, const double* class_cost) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_svm_cost(*o, o->m, weights, class_cost, &o->W, o->CC, &o->cost_host);
}

int admm_sparse_l1class_set_folds(admm_sparse_l1class* o, int32_t nfolds, const int32_t* fold, const int32_t* heldout) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  const int64_t m = o->m;
  const int32_t K = o->K;
  if (o->classes && fold)
    return fail(ADMM_E_UNSUPPORTED, "held-out folds are not part of the multinomial model (admm_sparse_l1class_set_multinomial)");
  ADMM_TRY(check_observations(m, K, nullptr, nfolds, fold, heldout));  // (the lasso's own checks; a refused call changes nothing)
  ADMM_HIP_TRY(hipSetDevice(o->device));
  int32_t *f = nullptr, *hd = nullptr;
  if (fold) {
    if (!o->hpart) {  // what every object with folds needs, once
      const size_t kp = static_cast<size_t>(o->cg.chunks) * KC;
      ADMM_TRY(o->mem.alloc(&o->hpart, kp * LH_COUNT * kScgMaxWg));
      ADMM_HIP_TRY(hipMemsetAsync(o->hpart, 0, sizeof(double) * kp * LH_COUNT * kScgMaxWg, o->stream));
      ADMM_TRY(o->mem.alloc(&o->held_dev, static_cast<size_t>(LH_COUNT) * K));
    }
    std::vector<int32_t> hh(static_cast<size_t>(K), -1);
    for (int32_t k = 0; heldout && k < K; ++k) hh[k] = heldout[k];
    ADMM_TRY(alloc_words(*o, &hd, static_cast<size_t>(K)));
    ADMM_HIP_TRY(hipMemcpyAsync(hd, hh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
    ADMM_TRY(alloc_words(*o, &f, static_cast<size_t>(m)));
    ADMM_HIP_TRY(hipMemcpyAsync(f, fold, sizeof(int32_t) * m, hipMemcpyHostToDevice, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hh and the caller's buffer were read)
  }
  for (void* p : {static_cast<void*>(o->fold), static_cast<void*>(o->held)}) o->mem.free_one(p);
  o->fold = f;
  o->held = hd;
  o->held_host.clear();
  return ADMM_OK;
}

int admm_sparse_l1class_heldout(admm_sparse_l1class* o, double* loss, double* errors, double* weight) {
  if (!o || !loss || !errors || !weight) return fail(ADMM_E_INVALID, "object, loss, errors or weight is NULL");
  if (!o->has_run || o->held_host.empty())
    return fail(ADMM_E_INVALID, "the held-out sums need a run with folds set (admm_sparse_l1class_set_folds)");
  for (int32_t k = 0; k < o->K; ++k) {
    loss[k] = o->held_host[LH_COUNT * k + LH_LOSS];
    errors[k] = o->held_host[LH_COUNT * k + LH_ERR];
    weight[k] = o->held_host[LH_COUNT * k + LH_W];
  }
  return ADMM_OK;
}

int admm_sparse_l1class_set_l1weights(admm_sparse_l1class* o, const double* l1weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  ADMM_TRY(check_l1_weights(l1weights, o->n));  // (the message of the create-time check; a refused call changes nothing)
  return set_shared_weights(*o, o->n, l1weights, &o->LW);
}

int admm_sparse_l1class_set_groups(admm_sparse_l1class* o, int32_t G, const int64_t* sizes, const double* groupweights,
                                   const double* l1) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (o->classes && G > 0)
    return fail(ADMM_E_UNSUPPORTED, "groups are not part of the multinomial model (admm_sparse_l1class_set_multinomial)");
  return set_multi_groups(*o, o->n, G, sizes, groupweights, l1, &o->grp);
}

int admm_sparse_l1class_set_multinomial(admm_sparse_l1class* o, int32_t classes) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (classes == 0) {
    o->classes = 0;
    o->start.clear();
    return ADMM_OK;
  }
  if (classes < 2 || classes > KC)
    return fail(ADMM_E_INVALID, "multinomial: classes = " + std::to_string(classes) + " is neither 0 nor in 2 .. " +
                                    std::to_string(KC));
  if (o->fold) return fail(ADMM_E_UNSUPPORTED, "the multinomial model does not combine with held-out folds (admm_sparse_l1class_set_folds)");
  if (o->grp.on()) return fail(ADMM_E_UNSUPPORTED, "the multinomial model does not combine with groups (admm_sparse_l1class_set_groups)");
  const int32_t K = o->K, per = KC / classes, rem = K % KC;
  if (rem % classes != 0 || rem > per * classes)
    return fail(ADMM_E_INVALID, "multinomial: the last chunk holds " + std::to_string(rem) + " fits, not a multiple of " +
                                    std::to_string(classes) + " classes up to " + std::to_string(per * classes));
  if (o->ell_shared) return fail(ADMM_E_INVALID, "multinomial: the model needs one label column per fit (nell = K)");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  std::vector<int32_t> lh(static_cast<size_t>(K)), nh(static_cast<size_t>(K));
  std::vector<double> ph(static_cast<size_t>(2) * K);
  ADMM_HIP_TRY(hipMemcpy(lh.data(), o->loss, sizeof(int32_t) * K, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(nh.data(), o->nonneg, sizeof(int32_t) * K, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(ph.data(), o->par, sizeof(double) * 2 * K, hipMemcpyDeviceToHost));
  std::vector<MultiRec> start(static_cast<size_t>(K), MultiRec{0, 0, 0, 0});
  for (int32_t k = 0; k < K; ++k) {
    const int32_t c = k % KC;
    if (c >= per * classes) {  // an idle slot: never run, never reported
      start[k].stop = 1;
      continue;
    }
    if (lh[k] != ADMM_LOSS_LOGISTIC)
      return fail(ADMM_E_INVALID, "multinomial: slot " + std::to_string(k) + " does not carry the logistic loss");
    const int32_t k0 = k - c % classes;  // the model's first slot
    if (ph[2 * k] != ph[2 * k0] || ph[2 * k + 1] != ph[2 * k0 + 1] || nh[k] != nh[k0])
      return fail(ADMM_E_INVALID, "multinomial: slot " + std::to_string(k) + " differs from slot " + std::to_string(k0) +
                                      " of its model in lambda, ridge or nonneg");
  }
  {  // every row carries exactly one +1 among a model's label columns: ELL read back once
    const size_t ep = static_cast<size_t>(o->cg.chunks) * KC;
    std::vector<double> eh(ep * o->m);
    ADMM_HIP_TRY(hipMemcpy(eh.data(), o->ELL, sizeof(double) * eh.size(), hipMemcpyDeviceToHost));
    for (int32_t mo = 0; mo < o->cg.chunks * per; ++mo) {
      const int32_t k0 = (mo / per) * KC + (mo % per) * classes;  // the model's first slot
      if (k0 + classes > K) continue;
      const double* E = eh.data() + static_cast<size_t>(k0 / KC) * o->m * KC + k0 % KC;
      for (int64_t i = 0; i < o->m; ++i) {
        int pos = 0;
        for (int32_t c = 0; c < classes; ++c) pos += E[i * KC + c] > 0.0 ? 1 : 0;
        if (pos != 1)
          return fail(ADMM_E_INVALID, "multinomial: row " + std::to_string(i) + " carries " + std::to_string(pos) +
                                          " labels +1 among the slots " + std::to_string(k0) + " .. " +
                                          std::to_string(k0 + classes - 1) + " (exactly one class is the true one)");
      }
    }
  }
  o->classes = classes;
  o->start.swap(start);
  return ADMM_OK;
}

int admm_op_softmax_prox(const double* V, const int32_t* y, const double* a, int64_t m, int32_t Cn, double* out,
                         int32_t* iters_out) {
  if (!V || !y || !a || !out || !iters_out || m <= 0 || Cn < 2 || Cn > KC)
    return fail(ADMM_E_INVALID, "softmax_prox: bad argument (m >= 1, Cn in 2 .. 10)");
  for (int64_t i = 0; i < m; ++i) {
    if (y[i] < 0 || y[i] >= Cn) return fail(ADMM_E_INVALID, "softmax_prox: y[" + std::to_string(i) + "] is no class");
    if (!finite_nonneg(a[i])) return fail(ADMM_E_INVALID, "softmax_prox: a[" + std::to_string(i) + "] is negative or not finite");
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  DevMem mem;
  double *dV = nullptr, *da = nullptr, *dout = nullptr, *raw = nullptr;
  const size_t words = (static_cast<size_t>(m) * sizeof(int32_t) + 7) / 8;
  int rc = mem.alloc(&dV, static_cast<size_t>(m) * Cn);
  if (rc == ADMM_OK) rc = mem.alloc(&da, static_cast<size_t>(m));
  if (rc == ADMM_OK) rc = mem.alloc(&dout, static_cast<size_t>(m) * Cn);
  if (rc == ADMM_OK) rc = mem.alloc(&raw, 2 * words);
  hipError_t e = hipSuccess;
  if (rc == ADMM_OK) {
    int32_t* dy = reinterpret_cast<int32_t*>(raw);
    int32_t* dit = reinterpret_cast<int32_t*>(raw + words);
    e = hipMemcpy(dV, V, sizeof(double) * m * Cn, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(da, a, sizeof(double) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy, y, sizeof(int32_t) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      with_classes(Cn, ProxOpLaunch{dV, dy, da, m, dout, dit});
      e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * m * Cn, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(iters_out, dit, sizeof(int32_t) * m, hipMemcpyDeviceToHost);
  }
  mem.release();
  if (rc != ADMM_OK) return rc;
  if (e != hipSuccess) return fail(ADMM_E_DEVICE, std::string("softmax_prox: ") + hipGetErrorString(e));
  return ADMM_OK;
}

int admm_sparse_l1class_kernel_time(admm_sparse_l1class* o, int32_t reps, int32_t dual, double* row_us, double* elem_us) {
  if (!o || reps < 1) return fail(ADMM_E_INVALID, "object is NULL or reps < 1");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  ADMM_TRY(sl1c_begin_run(o));  // every fit runs; the iterates are overwritten, as the next run's start does anyway
  const Sl1cRowArgs ra = sl1c_row_args(o, dual != 0, 1, 1.0);
  const Sl1cElemArgs ea = sl1c_elem_args(o, dual != 0, 1, 1.0);
  double* outs[2] = {row_us, elem_us};
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<float> ms(static_cast<size_t>(reps));
    for (int32_t i = -1; i < reps; ++i) {  // (i = -1: warm-up)
      ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
      if (pass == 0) launch_sl1c_row(ra, false, o->stream);
      else launch_sl1c_elem_iter(ea, o->grp, o->stream);
      ADMM_HIP_TRY(hipEventRecord(o->ev1, o->stream));
      ADMM_HIP_TRY(hipEventSynchronize(o->ev1));
      if (i >= 0) ADMM_HIP_TRY(hipEventElapsedTime(&ms[i], o->ev0, o->ev1));
    }
    std::sort(ms.begin(), ms.end());
    if (outs[pass]) *outs[pass] = 1e3 * static_cast<double>(ms[reps / 2]);
  }
  ADMM_HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_sparse_l1class_fetch(admm_sparse_l1class* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_L1C_F_XOPT: return o->cg.fetch_matrix(o->cg.X, o->n, dst, cap, written);
    case ADMM_L1C_F_ZOPT: return sl1c_fetch_stacked(o, o->Z1, o->Z2, dst, cap, written);
    case ADMM_L1C_F_UOPT: return sl1c_fetch_stacked(o, o->U1, o->U2, dst, cap, written);
    case ADMM_L1C_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_L1C_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_L1C_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_L1C_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_L1C_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the sparse l1 classifier");
  }
}

void admm_sparse_l1class_destroy(admm_sparse_l1class* o) { destroy_sparse(o); }

}  // extern "C"
