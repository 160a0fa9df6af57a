// loop_kernels.hip -- the per-iteration vector work of the ADMM loop as fused kernels.
//
//   prox kernel     : admm.m:515-560 (relaxation, z-prox, u-update), 563-569 (fast ADMM
//                     extrapolation), 608-610 (history), and every partial sum needed by
//                     621-624 / 648-654 / 305-306 / 572-573, plus the NEXT x-update's rhs
//                     (getProxOps.m:1195, 1455, 1031, 1514, 1067) -- one pass over the vectors.
//   finalize kernel : one workgroup; sums the block partials in fixed order (bitwise
//                     reproducible), forms pnorm/dnorm/perr/derr/Hnormsq/objective, runs the
//                     convergence test (686-702) and the stop logic (706-722) on the device.
// All kernels no-op once ctrl->stop is set, so the host can enqueue ahead of the stop test.
#include "loop_kernels.h"
#include "finalize_device.h"
#include "prox_device.h"
#include "group_device.h"
#include "penalty_device.h"
#include "loss_device.h"
#include "svm_cost_device.h"
#include "tv2d_pixel.h"
#include "slot_reduce.h"

namespace admm {

// Loss: the element-update family the instantiation carries (loop_kernels.h: ProxFamily; with_prox_family picks it).
// LossArgs: the loss family (loss_device.h): the weight travels with prox_load's round trip and z reaches
// prox_apply in a register (PROX_GIVEN).  SvmCostArgs: the cost form of the linear SVM (svm_cost_device.h; DESIGN.md
// q34) through the same statements, LOGI saying whether it knows the logistic loss.  The pack is empty for every other
// instantiation: those keep their parameter list and their code, instruction for instruction.
template <bool LOGI, class... Loss>
__global__ __launch_bounds__(kBlock) void prox_kernel(ProxArgs a, const Ctrl* __restrict__ ctrl, Loss... la) {
  constexpr bool LOSS = sizeof...(Loss) != 0;
  // the three control words in one scalar round trip, before the branch
  const int32_t stop = ctrl->stop;
  const int64_t it = ctrl->iter;
  const double aprev = ctrl->acurr;
  if (stop) return;
  double acc[S_COUNT];
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) acc[s] = 0.0;
  double kcoef = 0.0;
  if (a.alg == 1) {  // admm.m:504, 567: aprev = acurr; acurr = (1+sqrt(1+4 aprev^2))/2
    const double acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
    kcoef = (aprev - 1.0) / acn;
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    if constexpr (LOSS) {
      ProxIn in = prox_load(a, i);
      const double wi = loss_weight(loss_of(la...), a.z, i);
      const double ax = gather_chunks(a.axsrc, a.naxpart, a.axld, i);
      loss_form_z<LOGI>(a, loss_of(la...), wi, ax, in, acc);
      prox_apply<false>(a, i, ax, it, kcoef, in, acc);
    } else {
      const ProxIn in = prox_load(a, i);
      const double ax = gather_chunks(a.axsrc, a.naxpart, a.axld, i);
      prox_apply<LOGI>(a, i, ax, it, kcoef, in, acc);
    }
  }
  __shared__ double sred[4][S_COUNT];
  block_reduce_slots<4>(acc, sred, a.part, kMaxPartBlocks, blockIdx.x);
}

// PROX_PAIR: prox_kernel with the pair shrink of isotropic 2-D TV as the z-prox.  One thread per PAIR: it loads the
// inputs of element k and of its partner k + len/2, shrinks once and runs prox_apply for both with z in ProxIn::zg_i
// (PROX_GIVEN from a register).  No thread reads what another one writes in this launch -- fast ADMM (alg 1) stores the
// extrapolated v, uhat in place from prox_apply -- and both elements of a pair get one scale.
__global__ __launch_bounds__(kBlock) void pair_prox_kernel(ProxArgs a, const Ctrl* __restrict__ ctrl) {
  const int32_t stop = ctrl->stop;
  const int64_t it = ctrl->iter;
  const double aprev = ctrl->acurr;
  if (stop) return;
  double acc[S_COUNT];
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) acc[s] = 0.0;
  double kcoef = 0.0;
  if (a.alg == 1) {
    const double acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
    kcoef = (aprev - 1.0) / acn;
  }
  const int64_t half = a.len >> 1;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; k < half;
       k += static_cast<int64_t>(gridDim.x) * kBlock) {
    ProxIn in0 = prox_load(a, k), in1 = prox_load(a, k + half);
    const double ax0 = gather_chunks(a.axsrc, a.naxpart, a.axld, k);
    const double ax1 = gather_chunks(a.axsrc, a.naxpart, a.axld, k + half);
    double u0, u1;  // (prox_apply forms u its own way, as for every other prox)
    tv2px_pair_shrink(group_prox_v(a, ax0, in0), group_prox_v(a, ax1, in1), a.t, in0.zg_i, in1.zg_i, u0, u1);
    prox_apply<false>(a, k, ax0, it, kcoef, in0, acc);
    prox_apply<false>(a, k + half, ax1, it, kcoef, in1, acc);
  }
  __shared__ double sred[4][S_COUNT];
  block_reduce_slots<4>(acc, sred, a.part, kMaxPartBlocks, blockIdx.x);
}

// (A variant of this kernel that gathered x_i straight from symv_lower_kernel's partial sums -- 16 elements x 16
// slots per workgroup, saving the symv_reduce launch -- was measured SLOWER on the headline loop: 10.29k vs
// 11.55k it/s.  625 workgroups instead of 40 make the 12-slot block reductions and the finalize kernel's
// partial sums cost more than the launch they save.  Re-measured after the finalize kernel's partial loads were
// unrolled and the prox loads batched: still 10.24k against 10.32k it/s on the same box -- the two-kernel form stays.)

__global__ __launch_bounds__(kBlock) void prez_kernel(PreZArgs a, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double ax = gather_chunks(a.axsrc, a.naxpart, a.axld, i);
    const double zp = a.z[i];
    const double ci = a.c ? a.c[i] : 0.0;
    // same expression as prox_kernel, so the split update is bit-identical to the fused one
    const double axh = (a.relax != 1.0) ? a.relax * ax - (1.0 - a.relax) * ((-zp) - ci) : ax;
    a.xh[i] = axh;
    if (a.rz) a.rz[i] = (a.add ? a.add[i] : 0.0) + a.rho * ((axh + a.uo[i]) - ci);
  }
}

void launch_prez(const PreZArgs& a, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(a.len, kBlock, 2048);
  hipLaunchKernelGGL(prez_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, ctrl);
}

__global__ __launch_bounds__(kBlock) void negate_kernel(const double* __restrict__ z, double* __restrict__ bz,
                                                        int64_t len, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < len;
       i += static_cast<int64_t>(gridDim.x) * kBlock)
    bz[i] = -z[i];  // B = -1 (a general B: the loop's z buffer holds w = -B*z, so this is B*z as well)
}

void launch_negate(const double* z, double* bz, int64_t len, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(len, kBlock, 2048);
  hipLaunchKernelGGL(negate_kernel, dim3(blocks), dim3(kBlock), 0, stream, z, bz, len, ctrl);
}

// grid = the prox kernel's block count: slots S_U2 / S_DU2 of every block it wrote are rewritten
__global__ __launch_bounds__(kBlock) void ufix_kernel(UFixArgs a, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  __shared__ double scratch[4];
  const int64_t it = ctrl->iter;
  double su = 0.0, sdu = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double un = a.unew[i], uo = a.uold[i], zn = a.z[i];
    const double ci = a.c ? a.c[i] : 0.0;
    const double add = a.rhs_add ? a.rhs_add[i] : 0.0;
    a.u[i] = un;
    if (a.uhist) a.uhist[it * a.len + i] = un;
    su += un * un;
    const double du = un - uo;
    sdu += du * du;
    // as prox_apply's epilogue (plain ADMM: zx = z, ux = u)
    if (a.rhs && a.rhs_kind != RHS_NONE) a.rhs[i] = rhs_value(a.rhs_kind, a.rho, zn, un, ci, add);
  }
  const double tu = block_sum(su, scratch);
  const double tdu = block_sum(sdu, scratch);
  if (threadIdx.x == 0) {
    a.part[S_U2 * kMaxPartBlocks + blockIdx.x] = tu;
    a.part[S_DU2 * kMaxPartBlocks + blockIdx.x] = tdu;
  }
}

void launch_ufix(const UFixArgs& a, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(ufix_kernel, dim3(static_cast<unsigned>(a.nblk < 1 ? 1 : a.nblk)), dim3(kBlock), 0, stream, a, ctrl);
}

// operands this variant does not read -> null (prox_load loads every non-null one up front, and some of them are shorter
// than len when the variant does not use them)
ProxArgs pruned_prox_operands(const ProxArgs& args) {
  ProxArgs a = args;
  const bool need_ell = a.prox == PROX_HINGE || a.prox == PROX_01 || a.prox == PROX_LOGISTIC || a.objx == OBJX_HINGE ||
                        a.objx == OBJX_ZEROONE || a.objx == OBJX_LOGISTIC || a.objx == OBJX_DOT;
  if (!need_ell) a.ell = nullptr;
  if (a.prox != PROX_GIVEN) a.zgiven = nullptr;
  if (a.prox != PROX_BOX) a.lb = a.ub = nullptr;
  const bool need_add = (a.alg != 2 && a.rhs && (a.rhs_kind == RHS_RHO_DTS || a.rhs_kind == RHS_RHO_MINUS_Q)) ||
                        a.objx == OBJX_SOLVE || a.objx == OBJX_SOLVE_QP;
  if (!need_add) a.rhs_add = nullptr;
  return a;
}

// The operands of every kernel that forms z in a register ahead of prox_apply -- a family's instantiation, the grouped
// tail -- and sums the objective term that goes with it itself.  (The cost form belongs to a linear-SVM engine: its prox
// is one of the SVM's, so ell stays.)
ProxArgs register_z_operands(const ProxArgs& args, bool cost, int32_t* want_obj) {
  ProxArgs a = pruned_prox_operands(args);
  a.prox = PROX_GIVEN;
  a.zgiven = nullptr;
  if (cost) {
    *want_obj = a.objx != OBJX_NONE ? 1 : 0;
    a.objx = OBJX_NONE;
  } else {
    *want_obj = a.objz != OBJZ_NONE ? 1 : 0;
    a.objz = OBJZ_NONE;
  }
  return a;
}

void launch_prox(const ProxArgs& args, const Ctrl* ctrl, int* nblk_out, hipStream_t stream, const ProxFamily* fam) {
  if (args.prox == PROX_PAIR) {  // one thread per pair; len is even (prox_pair_ok: the caller has checked); no family
    ProxArgs ap = pruned_prox_operands(args);
    ap.prox = PROX_GIVEN;  // z reaches prox_apply in a register
    const int pblocks = grid_blocks(ap.len / 2, kBlock, kMaxPartBlocks);
    *nblk_out = pblocks;
    hipLaunchKernelGGL(pair_prox_kernel, dim3(pblocks), dim3(kBlock), 0, stream, ap, ctrl);
    return;
  }
  const int blocks = grid_blocks(args.len, kBlock, kMaxPartBlocks);
  *nblk_out = blocks;
  with_prox_family<FAM_LOSS, FAM_COST>(args, fam, [&](auto logi, const ProxArgs& a, const auto&... fa) {
    hipLaunchKernelGGL((prox_kernel<decltype(logi)::value, std::decay_t<decltype(fa)>...>), dim3(blocks), dim3(kBlock), 0,
                       stream, a, ctrl, fa...);
  });
}

// ---------------------------------------------------------------- alg 2: decide + extrapolate
__device__ __forceinline__ double sum_slot(const double* part, int slot, int nblk, double* scratch) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) s += part[slot * kMaxPartBlocks + b];
  return block_sum(s, scratch);
}

__global__ __launch_bounds__(kBlock) void fast_decide_kernel(FinArgs a) {
  Ctrl* ctrl = a.ctrl;
  if (ctrl->stop) return;
  __shared__ double scratch[4];
  const double s_duh = a.slots_reduced ? a.slots_reduced[S_DUH2] : sum_slot(a.part, S_DUH2, a.nblk, scratch);
  const double s_dzv = a.slots_reduced ? a.slots_reduced[S_DZV2] : sum_slot(a.part, S_DZV2, a.nblk, scratch);
  if (threadIdx.x == 0) {
    const double aprev = ctrl->acurr;  // admm.m:504
    const double dprev = ctrl->d;      // admm.m:509
    double d = 1.0 / a.rho * s_duh + a.rho * s_dzv;  // admm.m:572-573 (B = -I)
    double acn, coef, rst;
    if (d < a.restart * dprev) {  // admm.m:576-582
      acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
      coef = (aprev - 1.0) / acn;
      rst = 0.0;
    } else {  // admm.m:583-591
      acn = 1.0;
      coef = 0.0;
      rst = 1.0;
      d = dprev / a.restart;
    }
    ctrl->aprev = aprev;
    ctrl->acurr = acn;
    ctrl->dprev = dprev;
    ctrl->d = d;
    ctrl->coef = coef;
    ctrl->restart_flag = rst;
  }
}

void launch_fast_decide(const FinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(fast_decide_kernel, dim3(1), dim3(kBlock), 0, stream, a);
}

__global__ __launch_bounds__(kBlock) void extrapolate_kernel(ExtrapArgs a, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  const int64_t it = ctrl->iter;
  const double coef = ctrl->coef;
  const bool rst = ctrl->restart_flag != 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double z = a.z[i], u = a.u[i], zp = a.zprev[i], up = a.uprev[i];
    const double vn = rst ? zp : z + coef * (z - zp);
    const double uh = rst ? up : u + coef * (u - up);
    a.v[i] = vn;
    a.uhat[i] = uh;
    if (a.vhist) a.vhist[it * a.len + i] = vn;
    if (a.uhathist) a.uhathist[it * a.len + i] = uh;
    if (a.rhs)
      a.rhs[i] = rhs_value(a.rhs_kind, a.rho, vn, uh, a.c ? a.c[i] : 0.0, a.rhs_add ? a.rhs_add[i] : 0.0);
  }
}

void launch_extrapolate(const ExtrapArgs& a, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(a.len, kBlock, 2048);
  hipLaunchKernelGGL(extrapolate_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, ctrl);
}

__global__ __launch_bounds__(kBlock) void zstate_kernel(ZStateArgs a, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  const int64_t it = ctrl->iter;
  double coef = 0.0;
  bool rst = false;
  if (a.phase == 1) {
    coef = ctrl->coef;
    rst = ctrl->restart_flag != 0.0;
  } else if (a.alg == 1) {  // admm.m:504, 567-568, as prox_kernel takes it: finalize has not advanced acurr yet
    const double aprev = ctrl->acurr;
    coef = (aprev - 1.0) / (0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev)));
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < a.len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    double zn, zp;
    if (a.phase == 0) {
      zn = a.znew[i];
      zp = a.z[i];
      a.zprev[i] = zp;
      a.z[i] = zn;
      if (a.zhist) a.zhist[it * a.len + i] = zn;
      if (a.alg != 1) continue;
    } else {
      zn = a.z[i];
      zp = a.zprev[i];
    }
    const double vn = rst ? zp : zn + coef * (zn - zp);
    a.v[i] = vn;
    if (a.vhist) a.vhist[it * a.len + i] = vn;
  }
}

void launch_zstate(const ZStateArgs& a, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(a.len, kBlock, 2048);
  hipLaunchKernelGGL(zstate_kernel, dim3(blocks), dim3(kBlock), 0, stream, a, ctrl);
}

__global__ __launch_bounds__(kBlock) void initial_rhs_kernel(int64_t len, int kind, double rho,
                                                             const double* __restrict__ zx,
                                                             const double* __restrict__ ux,
                                                             const double* __restrict__ c,
                                                             const double* __restrict__ add,
                                                             double* __restrict__ rhs) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < len;
       i += static_cast<int64_t>(gridDim.x) * kBlock)
    rhs[i] = rhs_value(kind, rho, zx[i], ux[i], c ? c[i] : 0.0, add ? add[i] : 0.0);
}

void launch_initial_rhs(int64_t len, int rhs_kind, double rho, const double* zx, const double* ux, const double* c,
                        const double* rhs_add, double* rhs, hipStream_t stream) {
  const int blocks = grid_blocks(len, kBlock, 2048);
  hipLaunchKernelGGL(initial_rhs_kernel, dim3(blocks), dim3(kBlock), 0, stream, len, rhs_kind,
                     rho, zx, ux, c, rhs_add, rhs);
}

// ---------------------------------------------------------------- finalize
// COHERENT: called by the last workgroup of the prox kernel to arrive (prox_fin_kernel): the block partials were
// published write-through by other compute units during this launch and are read past the L1 (sc1 loads).
__global__ __launch_bounds__(kBlock) void finalize_kernel(FinArgs a) {
  if (a.ctrl->stop) return;
  finalize_body<false>(a);
}

// ---------------------------------------------------------------- one-launch tail of an A = I iteration
// prox + finalize (and, after the lower-triangle x-solve, the sum of its partial rows) in ONE launch.  Workgroup =
// one tile of W elements x S slots (W * S = 512 threads): every thread sums its slot's share of the x-solve's partial
// rows of its element (all loads of a thread in one round), the shares meet in LDS, the first W threads run the fused
// element update, the block partials are stored (deferred) or published write-through (sc1) with an arrival on
// ctrl->arrive, where the LAST workgroup to arrive runs the finalize logic (norms, tolerances, H-norm, stop) on the
// device in the same launch.  Sums are taken in a fixed order whatever the arrival order: bitwise reproducible.
// (W, S): kTailTile x kTailSlots = 128 x 4, one diagonal tile of the x-solve per workgroup, everywhere but behind the
// packed lower-triangle x-solve.  There a workgroup's gather is W columns of every partial row, fetched from beyond
// the L2 (other XCDs wrote them one launch earlier); at n = 10000 that is 79 workgroups of 80 KB each, on 79 of 256
// compute units.  kTailTileWide x kTailSlotsWide = 64 x 8 halves what a compute unit takes in: dev/tail_bench.hip
// measures the gather's cost over the same kernel on one row at 1.2 us for 128 x 4, 0.9 for 64 x 8, 0.7 for 32 x 16 and
// 0.5 for 16 x 32, and the whole kernel 1.1 us shorter at 64 x 8 and 32 x 16 alike (16 x 32 gives 0.1 back); the
// smaller of the two grids is built (EXPERIMENTS.md, "Lasso tail: the grid of the partial-row gather").
constexpr int kTailBlock = 512;
constexpr int kTailTile = 128;
constexpr int kTailSlots = kTailBlock / kTailTile;          // threads per element: each sums a quarter of the partial rows
constexpr int kTailTileWide = 64;                           // behind the packed x-solve (tail_wide)
constexpr int kTailSlotsWide = kTailBlock / kTailTileWide;
constexpr int kTailXTile = 128;                             // the x-solve's tile: partial row p belongs to tile p
// partial rows a thread loads in one round: 24 at four slots, and as many loads per element with more of them
template <int S>
constexpr int kTailRows = 96 / S;

// the wide grid serves the gather behind the packed lower-triangle x-solve alone (the form dev/tail_bench.hip measured),
// while its workgroups' block partials fit the part array
static bool tail_wide(const ProxArgs& a) {
  return a.ax_t && !a.ax_tri && ceil_div(a.len, kTailTileWide) <= kMaxPartBlocks;
}

template <int S>
__device__ __forceinline__ double tail_gather(const ProxArgs& a, int64_t i, int32_t p0, int32_t p1) {
  // unified partial row p of element i (diagonal tile d = i / 128): p <= d -> axsrc[p] (N-part), else ax_t[p - 1]
  // (one-block triangular solves, ax_tri: the caller's p counts from the diagonal tile, rows d + p of ax_t)
  const int32_t d = static_cast<int32_t>(i / kTailXTile);
  double s = 0.0;
  for (int32_t p = p0; p < p1; p += kTailRows<S>) {
    double v[kTailRows<S>];
#pragma unroll
    for (int k = 0; k < kTailRows<S>; ++k) {
      const int32_t q = (p + k < p1) ? p + k : p1 - 1;
      const double* src = a.ax_tri ? a.ax_t + static_cast<int64_t>(d + q) * a.axld
                          : (!a.ax_t || q <= d) ? a.axsrc + static_cast<int64_t>(q) * a.axld
                                                : a.ax_t + static_cast<int64_t>(q - 1) * a.axld;
      v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < kTailRows<S>; ++k)
      if (p + k < p1) s += v[k];
  }
  return s;
}

// share `slot` of S of the partial rows of element ic, whose diagonal tile (of the x-solve: 128 elements) is d:
// naxpart + 1 rows after the lower-triangle x-solve (N-part rows up to the diagonal tile, T-part rows beyond),
// naxpart - d rows after the one-block triangular solves, naxpart chunk rows of a column-chunked GEMV otherwise -- split
// into S runs of ceil(P / S) consecutive rows, each summed in row order
template <int S>
__device__ __forceinline__ double tail_ax_share(const ProxArgs& a, int64_t ic, int32_t d, int slot) {
  const int32_t P = a.ax_tri ? a.naxpart - d : (a.ax_t ? a.naxpart + 1 : a.naxpart);
  const int32_t q = (P + S - 1) / S;
  const int32_t p0 = slot * q, p1 = (p0 + q < P) ? p0 + q : P;
  return p0 < P ? tail_gather<S>(a, ic, p0, p1) : 0.0;
}

// The shares of a workgroup of W elements x S slots meet in LDS; the slot-0 thread of element e gets their sum in slot
// order, ((s0 + s1) + s2) + ... (the other threads' return value means nothing).  One barrier inside.
template <int W, int S>
__device__ __forceinline__ double tail_fold(double share, int e, int slot, double (*shares)[W]) {
  if (slot > 0) shares[slot - 1][e] = share;
  __syncthreads();
  double ax = share;
  if (slot == 0) {
#pragma unroll
    for (int k = 1; k < S; ++k) ax += shares[k - 1][e];
  }
  return ax;
}

// The end of a one-launch tail kernel (the caller returns behind it).  Block partials of the EW waves that hold
// elements; deferred, they are stored plainly and the next launch on the stream takes them after the kernel boundary.
// Otherwise they are published write-through, the workgroup arrives on ctrl->arrive, and the LAST workgroup to arrive
// resets the counter and runs the finalize logic on what every workgroup published.  The only cross-workgroup memory
// ordering of the library.
template <int EW>
__device__ __forceinline__ void tail_publish_finalize(const double (&acc)[S_COUNT], double* part, const FinArgs& f,
                                                      Ctrl* __restrict__ ctrl, int32_t defer) {
  __shared__ double sred[EW][S_COUNT];
  __shared__ int32_t last;
  if ((threadIdx.x >> 6) < EW) slot_wave_sums(acc, sred);
  __syncthreads();
  if (defer) {
    if (threadIdx.x < S_COUNT) part[threadIdx.x * kMaxPartBlocks + blockIdx.x] = slot_total<EW>(sred, threadIdx.x);
    return;
  }
  if (threadIdx.x < S_COUNT) {
    const int s = threadIdx.x;
    __hip_atomic_store(part + s * kMaxPartBlocks + blockIdx.x, slot_total<EW>(sred, s), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains: the element stores as well
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t old = __hip_atomic_fetch_add(&ctrl->arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (old == static_cast<int32_t>(gridDim.x) - 1) ? 1 : 0;
    if (last) __hip_atomic_store(&ctrl->arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last || threadIdx.x >= kBlock) return;  // the finalize logic is written for one 256-thread workgroup
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  finalize_body<true>(f);
}

// defer = 1: the finalize logic is NOT run here; the block partials are stored plainly and the next launch on the
// stream (the x-solve of the next iteration, or a stand-alone finalize) takes them after the kernel boundary.
// Loss: as prox_kernel's.
template <int W, int S, bool LOGI, class... Loss>
__global__ __launch_bounds__(kTailBlock) void prox_fin_kernel(ProxArgs a, FinArgs f, Ctrl* __restrict__ ctrl,
                                                              int32_t defer, Loss... la) {
  static_assert(W * S == kTailBlock && kTailXTile % W == 0, "a tile of the tail lies inside one tile of the x-solve");
  constexpr bool LOSS = sizeof...(Loss) != 0;
  const int32_t stop = ctrl->stop;
  const int64_t it = ctrl->iter;
  const double aprev = ctrl->acurr;
  // (the stop test sits below the loads: they do not depend on it, and in front of them it costs this kernel one more
  // memory round trip)
  __shared__ double shares[S - 1][W];
  const int e = threadIdx.x & (W - 1), slot = threadIdx.x / W;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * W + e;
  const int64_t ic = i < a.len ? i : a.len - 1;
  ProxIn in{};
  double wi = 1.0;
  if (slot == 0) {
    in = prox_load(a, ic);  // in flight together with the partial rows
    if constexpr (LOSS) wi = loss_weight(loss_of(la...), a.z, ic);
  }
  // (the workgroup's elements lie in one diagonal tile of the x-solve: d is uniform)
  const double share = tail_ax_share<S>(a, ic, static_cast<int32_t>(i / kTailXTile), slot);
  if (stop) return;  // (uniform; nothing has been stored yet)
  const double ax = tail_fold<W, S>(share, e, slot, shares);
  double acc[S_COUNT];
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) acc[s] = 0.0;
  if (slot == 0 && i < a.len) {
    double kcoef = 0.0;
    if (a.alg == 1) {
      const double acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
      kcoef = (aprev - 1.0) / acn;
    }
    if constexpr (LOSS) {
      loss_form_z<LOGI>(a, loss_of(la...), wi, ax, in, acc);
      prox_apply<false>(a, i, ax, it, kcoef, in, acc);
    } else {
      prox_apply<LOGI>(a, i, ax, it, kcoef, in, acc);
    }
  }
  tail_publish_finalize<(W + kWave - 1) / kWave>(acc, a.part, f, ctrl, defer);
}

FinArgs prox_fin_args(const ProxArgs& a, const FinArgs& f) {
  FinArgs ff = f;
  ff.nblk = static_cast<int32_t>(ceil_div(a.len, tail_wide(a) ? kTailTileWide : kTailTile));
  // nothing but the block partials (and, for A = D, the x of this iteration) feeds the finalize logic -- and objective
  // partials an earlier launch of the iteration wrote when the caller passes them (covariance selection: -log det X)
  ff.g = nullptr;
  ff.slots_reduced = nullptr;
  ff.objp_reduced = nullptr;
  return ff;
}

template <int W, int S>
__global__ void penalty_prox_fin_kernel(ProxArgs a, FinArgs f, PenaltyArgs pen, Ctrl* __restrict__ ctrl, int32_t defer,
                                        int32_t want_objz);  // (below, behind the grouped tail)

void launch_prox_fin(const ProxArgs& args, const FinArgs& f, Ctrl* ctrl, int* nblk_out, hipStream_t stream,
                     bool defer, const ProxFamily* fam) {
  // (the operand preparation below leaves ax_t, ax_tri and len alone: prox_fin_args sees the same grid)
  const bool wide = tail_wide(args);
  const dim3 grid(static_cast<unsigned>(ceil_div(args.len, wide ? kTailTileWide : kTailTile)));
  *nblk_out = static_cast<int>(grid.x);
  if (fam && fam->kind == FAM_PENALTY) {  // the ungrouped penalty: a kernel of its own, older than the pack
    int32_t want_objz = 0;
    const ProxArgs a = register_z_operands(args, false, &want_objz);
    const FinArgs ff = prox_fin_args(a, f);
    if (wide)
      hipLaunchKernelGGL((penalty_prox_fin_kernel<kTailTileWide, kTailSlotsWide>), grid, dim3(kTailBlock), 0, stream, a,
                         ff, fam->pen, ctrl, defer ? 1 : 0, want_objz);
    else
      hipLaunchKernelGGL((penalty_prox_fin_kernel<kTailTile, kTailSlots>), grid, dim3(kTailBlock), 0, stream, a, ff,
                         fam->pen, ctrl, defer ? 1 : 0, want_objz);
    return;
  }
  with_prox_family<FAM_LOSS, FAM_COST>(args, fam, [&](auto logi, const ProxArgs& a, const auto&... fa) {
    constexpr bool LOGI = decltype(logi)::value;
    const FinArgs ff = prox_fin_args(a, f);
    if (wide)
      hipLaunchKernelGGL((prox_fin_kernel<kTailTileWide, kTailSlotsWide, LOGI, std::decay_t<decltype(fa)>...>), grid,
                         dim3(kTailBlock), 0, stream, a, ff, ctrl, defer ? 1 : 0, fa...);
    else
      hipLaunchKernelGGL((prox_fin_kernel<kTailTile, kTailSlots, LOGI, std::decay_t<decltype(fa)>...>), grid,
                         dim3(kTailBlock), 0, stream, a, ff, ctrl, defer ? 1 : 0, fa...);
  });
}

// out = prox_{g/rho}(v) of the loss family: the stand-alone operator (ops.hip)
__global__ __launch_bounds__(kBlock) void loss_prox_kernel(const double* __restrict__ v, int64_t n, LossArgs la,
                                                           double* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kBlock)
    out[i] = loss_prox_elem(la, la.w ? la.w[i] : 1.0, v[i]);
}

void launch_loss_prox(const double* v, int64_t n, const LossArgs& loss, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(loss_prox_kernel, dim3(grid_blocks(n, kBlock, 2048)), dim3(kBlock), 0, stream, v, n, loss, out);
}

// out = the z-prox of the linear SVM's cost form: the stand-alone operator (ops.hip)
template <bool LOGI>
__global__ __launch_bounds__(kBlock) void svm_cost_prox_kernel(const double* __restrict__ v, const double* __restrict__ ell,
                                                               int64_t n, SvmCostArgs ka, double* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double li = ell[i];
    out[i] = svm_cost_prox_elem<LOGI>(ka, svm_cost_of(ka, loss_weight(ka, v, i), li), li, v[i]);
  }
}

void launch_svm_cost_prox(const double* v, const double* ell, int64_t n, const SvmCostArgs& cost, double* out,
                          hipStream_t stream) {
  const dim3 grid(grid_blocks(n, kBlock, 2048));
  if (cost.loss == ADMM_LOSS_LOGISTIC)
    hipLaunchKernelGGL(svm_cost_prox_kernel<true>, grid, dim3(kBlock), 0, stream, v, ell, n, cost, out);
  else hipLaunchKernelGGL(svm_cost_prox_kernel<false>, grid, dim3(kBlock), 0, stream, v, ell, n, cost, out);
}

// ---------------------------------------------------------------- group lasso: the grouped one-launch tail
// prox_fin_kernel with the block soft threshold (group_device.h) as the z-prox.  Workgroup w owns the whole groups
// wg_g[w] .. wg_g[w + 1] = the elements wg_e[w] .. wg_e[w + 1] (loop_kernels.h: GroupPlan) and walks them in chunks of
// 128 elements x 4 slots, twice: the first pass sums the x-solve's partial rows, forms v and the groups' norms; the second
// applies the scale and runs the fused element update with the finished z in ProxIn::zg_i (PROX_GIVEN from a register).
// With one chunk -- every workgroup of a plan at the starting budget whose groups fit one tile -- the second pass
// reuses the registers of the first; longer ranges gather again (the same loads in the same order: the same bits).
// Element i sums its partial rows exactly as prox_fin_kernel does with S slots: the same S shares (tail_ax_share), added
// in the same order (tail_fold's).  The chunk stays 128 elements x 4 threads whatever S is: thread `slot` of an element
// takes the S / 4 consecutive shares from slot * S / 4 on, one after the other.
template <int S>
__device__ __forceinline__ double group_ax(const ProxArgs& a, int64_t ic, int slot, int e,
                                           double (*shares)[kGroupTile]) {
  constexpr int PER = S / kTailSlots;
  static_assert(PER * kTailSlots == S, "every thread of an element takes the same number of shares");
  const int32_t d = static_cast<int32_t>(ic / kTailXTile);
  double sh[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) sh[k] = tail_ax_share<S>(a, ic, d, slot * PER + k);
  __syncthreads();  // (the previous chunk's shares have been read)
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (slot * PER + k > 0) shares[slot * PER + k - 1][e] = sh[k];
  __syncthreads();
  double ax = sh[0];
  if (slot == 0) {
#pragma unroll
    for (int k = 1; k < S; ++k) ax += shares[k - 1][e];
  }
  return ax;  // (meaningful in slot 0)
}

// PEN: the instantiation with the elementwise stage of the penalty family in front of the squares (penalty_device.h:
// e_i = soft(v_i, tau*w_i) or its positive part), kappa behind the scale and the whole of g(z) in S_OBJZ; the plain
// group lasso compiles without any of it and never reads pen.
template <bool PEN, int S>
__global__ __launch_bounds__(kTailBlock) void group_prox_fin_kernel(ProxArgs a, FinArgs f, GroupPlan gp,
                                                                    Ctrl* __restrict__ ctrl, int32_t defer,
                                                                    int32_t want_objz, PenaltyArgs pen) {
  const int32_t stop = ctrl->stop;
  const int64_t it = ctrl->iter;
  const double aprev = ctrl->acurr;
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x], ng = gp.wg_g[blockIdx.x + 1] - g0;
  if (stop) return;  // (uniform; the plan words above arrive in the same round trip as the control words)
  __shared__ double shares[S - 1][kGroupTile];
  __shared__ double sq[kGroupTile];
  __shared__ double gacc[kGroupMaxPerWg];
  static_assert(kGroupTile * kTailSlots == kTailBlock, "a chunk of a group plan is 128 elements x 4 threads");
  const int e = threadIdx.x & (kGroupTile - 1), slot = threadIdx.x >> 7;
  const int32_t nch = static_cast<int32_t>((E1 - E0 + kGroupTile - 1) / kGroupTile);
  double acc[S_COUNT];
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) acc[s] = 0.0;
  ProxIn in{};
  double ax = 0.0, wi = 1.0;
  int32_t gi = 0;
  int64_t i = E0 + e;
  for (int32_t c = 0; c < nch; ++c) {  // ---- pass 1: v (PEN: e) and the norms of the groups
    const int64_t cs = E0 + static_cast<int64_t>(c) * kGroupTile, ce = (cs + kGroupTile < E1) ? cs + kGroupTile : E1;
    i = cs + e;
    const int64_t ic = i < E1 ? i : E1 - 1;
    if (slot == 0) {
      in = prox_load(a, ic);  // in flight together with the partial rows
      gi = gp.gid[ic] - g0;
      if constexpr (PEN) wi = penalty_weight(pen, ic);
    }
    ax = group_ax<S>(a, ic, slot, e, shares);
    if (slot == 0) {
      double v = group_prox_v(a, ax, in);
      if constexpr (PEN) v = penalty_elem(v, pen.tau * wi, pen.nonneg);
      sq[e] = i < E1 ? v * v : 0.0;
    }
    __syncthreads();
    const double oz = group_chunk(gp, g0, ng, cs, ce, a.t, sq, gacc);
    if constexpr (PEN) {
      if (want_objz) acc[S_OBJZ] += pen.lam_group * (pen.kappa * oz);  // ||z_g|| = kappa*scale_g*||e_g||
    } else {
      if (want_objz) acc[S_OBJZ] += oz;
    }
    __syncthreads();
  }
  double kcoef = 0.0;
  if (a.alg == 1) {
    const double acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
    kcoef = (aprev - 1.0) / acn;
  }
  for (int32_t c = 0; c < nch; ++c) {  // ---- pass 2: z = scale_g * v and the rest of the element update
    if (nch > 1) {
      i = E0 + static_cast<int64_t>(c) * kGroupTile + e;
      const int64_t ic = i < E1 ? i : E1 - 1;
      if (slot == 0) {
        in = prox_load(a, ic);
        gi = gp.gid[ic] - g0;
        if constexpr (PEN) wi = penalty_weight(pen, ic);
      }
      ax = group_ax<S>(a, ic, slot, e, shares);
    }
    if (slot == 0 && i < E1) {
      if constexpr (PEN) {
        const double ei = penalty_elem(group_prox_v(a, ax, in), pen.tau * wi, pen.nonneg);
        in.zg_i = pen.kappa * (ei * gacc[gi]);
        if (want_objz) acc[S_OBJZ] += penalty_obj_elem(pen, wi, in.zg_i);
      } else {
        in.zg_i = group_prox_v(a, ax, in) * gacc[gi];
      }
      prox_apply<false>(a, i, ax, it, kcoef, in, acc);
    }
  }
  tail_publish_finalize<2>(acc, a.part, f, ctrl, defer);  // (the two waves that hold elements also hold the group sums)
}

void launch_group_prox_fin(const ProxArgs& args, const FinArgs& f, const GroupPlan& gp, Ctrl* ctrl, int* nblk_out,
                           hipStream_t stream, bool defer, const ProxFamily* fam) {
  // groups exist on ADMM_PROB_LASSO engines only (admm_engine_set_groups) and the grouped update is not used behind a
  // split z-update: args.prox is PROX_SOFT and objx is none or OBJX_SOLVE, so ell, the bounds and zgiven are nulled
  int32_t want_objz = 0;  // the kernel adds the penalty once per group instead
  const ProxArgs a = register_z_operands(args, false, &want_objz);
  *nblk_out = gp.nwg;
  FinArgs ff = prox_fin_args(a, f);
  ff.nblk = gp.nwg;
  const dim3 grid(static_cast<unsigned>(gp.nwg));
  const bool pen = fam && fam->kind == FAM_PENALTY;
  const PenaltyArgs pa = pen ? fam->pen : PenaltyArgs{};
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kTailBlock), 0, stream, a, ff, gp, ctrl, defer ? 1 : 0, want_objz, pa);
  };
  // the slots of the plain tail on the same operands: the same shares of the partial rows in the same order
  if (tail_wide(a)) pen ? launch(group_prox_fin_kernel<true, kTailSlotsWide>) : launch(group_prox_fin_kernel<false, kTailSlotsWide>);
  else pen ? launch(group_prox_fin_kernel<true, kTailSlots>) : launch(group_prox_fin_kernel<false, kTailSlots>);
}

// ---------------------------------------------------------------- the penalty family without groups
// prox_fin_kernel<false> with z = kappa * e_i (penalty_device.h) formed in a register and handed to prox_apply as
// PROX_GIVEN; the weight is one more coalesced load of slot 0, in flight with the rest.  S_OBJZ takes the whole of g(z).
// (As prox_fin_kernel's PenaltyArgs instantiation it has the same registers, LDS and occupancy but measured 0.05 us per
// launch slower than this kernel, whose two runs differ by 0.02: EXPERIMENTS.md, "One dispatch of the families".)
template <int W, int S>
__global__ __launch_bounds__(kTailBlock) void penalty_prox_fin_kernel(ProxArgs a, FinArgs f, PenaltyArgs pen,
                                                                      Ctrl* __restrict__ ctrl, int32_t defer,
                                                                      int32_t want_objz) {
  static_assert(W * S == kTailBlock && kTailXTile % W == 0, "a tile of the tail lies inside one tile of the x-solve");
  const int32_t stop = ctrl->stop;
  const int64_t it = ctrl->iter;
  const double aprev = ctrl->acurr;
  __shared__ double shares[S - 1][W];
  const int e = threadIdx.x & (W - 1), slot = threadIdx.x / W;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * W + e;
  const int64_t ic = i < a.len ? i : a.len - 1;
  ProxIn in{};
  double wi = 1.0;
  if (slot == 0) {
    in = prox_load(a, ic);  // in flight together with the partial rows
    wi = penalty_weight(pen, ic);
  }
  const double share = tail_ax_share<S>(a, ic, static_cast<int32_t>(i / kTailXTile), slot);
  if (stop) return;  // (uniform; nothing has been stored yet)
  const double ax = tail_fold<W, S>(share, e, slot, shares);
  double acc[S_COUNT];
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) acc[s] = 0.0;
  if (slot == 0 && i < a.len) {
    double kcoef = 0.0;
    if (a.alg == 1) {
      const double acn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * aprev * aprev));
      kcoef = (aprev - 1.0) / acn;
    }
    in.zg_i = pen.kappa * penalty_elem(group_prox_v(a, ax, in), pen.tau * wi, pen.nonneg);
    if (want_objz) acc[S_OBJZ] += penalty_obj_elem(pen, wi, in.zg_i);
    prox_apply<false>(a, i, ax, it, kcoef, in, acc);
  }
  tail_publish_finalize<(W + kWave - 1) / kWave>(acc, a.part, f, ctrl, defer);
}

// out = prox_{g/rho}(v) without groups: the stand-alone operator (ops.hip)
__global__ __launch_bounds__(kBlock) void penalty_prox_kernel(const double* __restrict__ v, int64_t n, PenaltyArgs pen,
                                                              double* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kBlock)
    out[i] = pen.kappa * penalty_elem(v[i], pen.tau * penalty_weight(pen, i), pen.nonneg);
}

// out = v .* scale of its group: the stand-alone operator (ops.hip), one thread per element of a chunk
template <bool PEN>
__global__ __launch_bounds__(kGroupTile) void group_soft_threshold_kernel(const double* __restrict__ v, GroupPlan gp,
                                                                          double t, double* __restrict__ out,
                                                                          PenaltyArgs pen) {
  __shared__ double sq[kGroupTile];
  __shared__ double gacc[kGroupMaxPerWg];
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x], ng = gp.wg_g[blockIdx.x + 1] - g0;
  const int32_t nch = static_cast<int32_t>((E1 - E0 + kGroupTile - 1) / kGroupTile);
  for (int32_t c = 0; c < nch; ++c) {
    const int64_t cs = E0 + static_cast<int64_t>(c) * kGroupTile, ce = (cs + kGroupTile < E1) ? cs + kGroupTile : E1;
    const int64_t i = cs + threadIdx.x;
    double vi = i < E1 ? v[i] : 0.0;
    if constexpr (PEN) vi = i < E1 ? penalty_elem(vi, pen.tau * penalty_weight(pen, i), pen.nonneg) : 0.0;
    sq[threadIdx.x] = vi * vi;
    __syncthreads();
    (void)group_chunk(gp, g0, ng, cs, ce, t, sq, gacc);
    __syncthreads();
  }
  for (int64_t i = E0 + threadIdx.x; i < E1; i += kGroupTile) {
    if constexpr (PEN)
      out[i] = pen.kappa * (penalty_elem(v[i], pen.tau * penalty_weight(pen, i), pen.nonneg) * gacc[gp.gid[i] - g0]);
    else out[i] = v[i] * gacc[gp.gid[i] - g0];
  }
}

void launch_group_soft_threshold(const double* v, const GroupPlan& gp, double t, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(group_soft_threshold_kernel<false>, dim3(static_cast<unsigned>(gp.nwg)), dim3(kGroupTile), 0, stream,
                     v, gp, t, out, PenaltyArgs{});
}

void launch_penalty_prox(const double* v, int64_t n, const GroupPlan* gp, double t, const PenaltyArgs& pen, double* out,
                         hipStream_t stream) {
  if (gp)
    hipLaunchKernelGGL(group_soft_threshold_kernel<true>, dim3(static_cast<unsigned>(gp->nwg)), dim3(kGroupTile), 0, stream,
                       v, *gp, t, out, pen);
  else
    hipLaunchKernelGGL(penalty_prox_kernel, dim3(grid_blocks(n, kBlock, 2048)), dim3(kBlock), 0, stream, v, n, pen, out);
}

GroupPlan GroupPlanHost::bind(const double* dev) const {
  GroupPlan p{};
  p.off = reinterpret_cast<const int64_t*>(dev + o_off);
  p.w = has_w ? dev + o_w : nullptr;
  p.gid = reinterpret_cast<const int32_t*>(dev + o_gid);
  p.wg_e = reinterpret_cast<const int64_t*>(dev + o_wge);
  p.wg_g = reinterpret_cast<const int32_t*>(dev + o_wgg);
  p.nwg = nwg;
  p.G = G;
  p.n = n;
  p.budget = budget;
  return p;
}

int group_plan_build(const int64_t* sizes, int32_t G, const double* weights, int64_t n, GroupPlanHost* out) {
  return group_plan_build(sizes, G, weights, n, GroupPlanLimits{kGroupTile, kGroupMaxPerWg, kMaxPartBlocks}, out);
}

int group_plan_build(const int64_t* sizes, int32_t G, const double* weights, int64_t n, const GroupPlanLimits& lim,
                     GroupPlanHost* out) {
  if (!sizes || G < 1 || n < 1 || !out) return fail(ADMM_E_INVALID, "groups: sizes, their count and n must be given");
  int64_t sum = 0;
  for (int32_t g = 0; g < G; ++g) {
    if (sizes[g] < 1) return fail(ADMM_E_INVALID, "groups: group " + std::to_string(g) + " has a size below 1");
    if (sizes[g] > n - sum) return fail(ADMM_E_INVALID, "groups: the sizes sum to more than n = " + std::to_string(n));
    sum += sizes[g];
  }
  if (sum != n)
    return fail(ADMM_E_INVALID, "groups: the sizes sum to " + std::to_string(sum) + ", not to n = " + std::to_string(n));
  if (weights)
    for (int32_t g = 0; g < G; ++g)
      if (!finite_nonneg(weights[g]))
        return fail(ADMM_E_INVALID, "groups: weight " + std::to_string(g) + " is negative or not finite");
  // whole groups per workgroup, up to `budget` elements and lim.max_per_wg groups; a group past the budget stands alone
  std::vector<int64_t> wge;
  std::vector<int32_t> wgg;
  int64_t budget = lim.budget0;
  for (;;) {
    wge.assign(1, 0);
    wgg.assign(1, 0);
    int64_t cur_e = 0, at = 0;
    int32_t cur_g = 0;
    for (int32_t g = 0; g < G; ++g) {
      if (cur_g > 0 && (cur_e + sizes[g] > budget || cur_g == lim.max_per_wg)) {
        wge.push_back(at);
        wgg.push_back(g);
        cur_e = 0;
        cur_g = 0;
      }
      cur_e += sizes[g];
      cur_g += 1;
      at += sizes[g];
    }
    wge.push_back(n);
    wgg.push_back(G);
    if (static_cast<int64_t>(wge.size()) - 1 <= lim.max_wg) break;
    if (budget >= n)
      return fail(ADMM_E_UNSUPPORTED, "groups: more than " + std::to_string(int64_t{lim.max_wg} * lim.max_per_wg) +
                                          " groups are not supported");
    budget *= 2;
  }
  GroupPlanHost& h = *out;
  h = GroupPlanHost{};
  h.nwg = static_cast<int32_t>(wge.size()) - 1;
  h.G = G;
  h.n = n;
  h.budget = budget;
  h.has_w = weights != nullptr;
  const size_t nG = static_cast<size_t>(G), nW = static_cast<size_t>(h.nwg) + 1;
  h.o_off = 0;
  h.o_w = h.o_off + nG + 1;
  h.o_wge = h.o_w + nG;
  h.o_gid = h.o_wge + nW;
  h.o_wgg = h.o_gid + (static_cast<size_t>(n) + 1) / 2;
  h.blob.assign(h.o_wgg + (nW + 1) / 2, 0.0);
  int64_t* off = reinterpret_cast<int64_t*>(h.blob.data() + h.o_off);
  int32_t* gid = reinterpret_cast<int32_t*>(h.blob.data() + h.o_gid);
  off[0] = 0;
  for (int32_t g = 0; g < G; ++g) {
    off[g + 1] = off[g] + sizes[g];
    for (int64_t i = off[g]; i < off[g + 1]; ++i) gid[i] = g;
    if (weights) h.blob[h.o_w + g] = weights[g];
  }
  std::memcpy(h.blob.data() + h.o_wge, wge.data(), nW * sizeof(int64_t));
  std::memcpy(h.blob.data() + h.o_wgg, wgg.data(), nW * sizeof(int32_t));
  return ADMM_OK;
}

void launch_finalize(const FinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kBlock), 0, stream, a);
}

// ---------------------------------------------------------------- all-reduce payload packing
__global__ __launch_bounds__(kBlock) void pack_slots_kernel(const double* __restrict__ part, int32_t nblk,
                                                            double* __restrict__ out16,
                                                            const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int slot = threadIdx.x >> 4, sub = threadIdx.x & 15;
  double v = 0.0;
  if (slot < S_COUNT)
    for (int b = sub; b < nblk; b += 16) v += part[slot * kMaxPartBlocks + b];
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (sub == 0) out16[slot] = v;
}

void launch_pack_slots(const double* part, int32_t nblk, double* out16, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(pack_slots_kernel, dim3(1), dim3(kBlock), 0, stream, part, nblk, out16, ctrl);
}

__global__ __launch_bounds__(kBlock) void pack_sum_kernel(const double* __restrict__ v, int32_t n,
                                                          double* __restrict__ out1, const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  __shared__ double scratch[4];
  double s = 0.0;
  for (int b = threadIdx.x; b < n; b += blockDim.x) s += v[b];
  const double t = block_sum(s, scratch);
  if (threadIdx.x == 0) out1[0] = t;
}

void launch_pack_sum(const double* v, int32_t n, double* out1, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(pack_sum_kernel, dim3(1), dim3(kBlock), 0, stream, v, n, out1, ctrl);
}

// ---------------------------------------------------------------- small helpers
__global__ __launch_bounds__(kBlock) void residual_sq_kernel(const double* __restrict__ part, int32_t nchunk,
                                                             int64_t ld, const double* __restrict__ s, int64_t len,
                                                             double* __restrict__ objpart,
                                                             const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  __shared__ double scratch[4];
  double acc = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double y = gather_chunks(part, nchunk, ld, i);
    const double r = y - s[i];
    acc += r * r;
  }
  const double t = block_sum(acc, scratch);
  if (threadIdx.x == 0) objpart[blockIdx.x] = t;
}

void launch_residual_sq(const double* part, int32_t nchunk, int64_t ld, const double* s, int64_t len, double* objpart,
                        int* nblk_out, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(len, kBlock, kMaxPartBlocks);
  *nblk_out = blocks;
  hipLaunchKernelGGL(residual_sq_kernel, dim3(blocks), dim3(kBlock), 0, stream, part, nchunk,
                     ld, s, len, objpart, ctrl);
}

__global__ __launch_bounds__(kBlock) void qp_objective_kernel(const double* __restrict__ part, int32_t nchunk,
                                                              int64_t ld, const double* __restrict__ x,
                                                              const double* __restrict__ q, int64_t len,
                                                              double* __restrict__ objpart,
                                                              const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  __shared__ double scratch[4];
  double acc = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double y = gather_chunks(part, nchunk, ld, i);
    acc += x[i] * (0.5 * y + q[i]);
  }
  const double t = block_sum(acc, scratch);
  if (threadIdx.x == 0) objpart[blockIdx.x] = t;
}

void launch_qp_objective(const double* part, int32_t nchunk, int64_t ld, const double* x, const double* q,
                         int64_t len, double* objpart, int* nblk_out, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(len, kBlock, kMaxPartBlocks);
  *nblk_out = blocks;
  hipLaunchKernelGGL(qp_objective_kernel, dim3(blocks), dim3(kBlock), 0, stream, part, nchunk,
                     ld, x, q, len, objpart, ctrl);
}

__global__ __launch_bounds__(kBlock) void run_init_kernel(RunInitArgs a) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x, T = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = t; i < a.nA; i += T) a.x[i] = 0.0;
  for (int64_t i = t; i < a.len; i += T) {
    a.z[i] = 0.0;
    a.u[i] = 0.0;
    a.v[i] = 0.0;
    a.uhat[i] = 0.0;
  }
  for (int64_t i = t; i < a.N; i += T) {
#pragma unroll
    for (int k = 0; k < 9; ++k) a.scal[k][i] = 0.0;
  }
  if (t == 0) *a.ctrl = a.c0;
}

void launch_run_init(const RunInitArgs& a, hipStream_t stream) {
  int64_t most = a.len > a.nA ? a.len : a.nA;
  if (a.N > most) most = a.N;
  const int blocks = grid_blocks(most, kBlock, 2048);
  hipLaunchKernelGGL(run_init_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
}

__global__ __launch_bounds__(kBlock) void obj_compare_kernel(const double* __restrict__ pa, int na, double sa, double ca,
                                                             const double* __restrict__ pb, int nb, double sb, double cb,
                                                             double* __restrict__ disc, const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  __shared__ double scratch[4];
  double va = 0.0, vb = 0.0;
  for (int i = threadIdx.x; i < na; i += kBlock) va += pa[i];
  for (int i = threadIdx.x; i < nb; i += kBlock) vb += pb[i];
  const double ta = block_sum(va, scratch);
  __syncthreads();
  const double tb = block_sum(vb, scratch);
  if (threadIdx.x == 0) {
    const double a = sa * ta + ca, b = sb * tb + cb;
    const double rel = fabs(a - b) / fmax(fabs(a), 1e-300);
    if (!(rel <= disc[0])) disc[0] = rel;  // NaN-safe maximum
  }
}

void launch_obj_compare(const double* pa, int na, double sa, double ca, const double* pb, int nb, double sb, double cb,
                        double* disc, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(obj_compare_kernel, dim3(1), dim3(kBlock), 0, stream, pa, na, sa, ca, pb, nb, sb, cb, disc, ctrl);
}

__global__ __launch_bounds__(kBlock) void combine_kernel(const double* __restrict__ part, int32_t nchunk, int64_t ld,
                                                         double alpha, const double* __restrict__ y, double beta,
                                                         const double* __restrict__ add, double* __restrict__ x,
                                                         int64_t len, const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < len;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    double s = gather_chunks(part, nchunk, ld, i);
    double v = alpha * s;
    if (y) v += beta * y[i];
    if (add) v += add[i];
    x[i] = v;
  }
}

void launch_combine(const double* part, int32_t nchunk, int64_t ld, double alpha, const double* y, double beta,
                    const double* add, double* x, int64_t len, const Ctrl* ctrl, hipStream_t stream) {
  const int blocks = grid_blocks(len, kBlock, 2048);
  hipLaunchKernelGGL(combine_kernel, dim3(blocks), dim3(kBlock), 0, stream, part, nchunk, ld,
                     alpha, y, beta, add, x, len, ctrl);
}

}  // namespace admm
