// l1class.hip -- sparse linear classifiers on a DENSE design matrix, K fits at once over one D: the
// lasso's penalty family (q32: l1, l1 weights, ridge, sign constraint) on the linear SVM's losses (q29, q34: hinge,
// squared hinge, logistic, with weights and class costs).  Every fit is a plain-ADMM run of admm.m with A = [D; I_n],
// B = -1, c = 0, z = [z1 (m); z2 (n)], stopcond 'standard':
//   x  = inv(D'D + I) y,  y = D'(z1 - u1) + (z2 - u2)     the matrix knows neither rho nor the fit: one cached inverse
//   z1 = prox of (C*c/rho)*phi at (D x + u1)              svm_cost_device.h
//   z2 = kappa*penalty_elem(x + u2, (lambda/rho)*w)       penalty_device.h
//   u += A x - z
// An ordinary ADMM_PROB_LASSO engine with rho = 1, which never runs, owns D, the factor and the fp64 packed inverse (a
// fat D is handed to it with zero rows below, which leave D'D as it is: the engine then builds the n x n form).  Per
// iteration, a multi-vector of len n in spmm.h's layout [chunks][n][kSpmmChunk], one of len m as [fit][ldz]:
//   launch_symm_packed            X from Y (launch_trsv_pair per fit where create's probe kept the solves)
//   l1c_forward_kernel            per chunk: D read ONCE for ten fits, any n: lane = row of a 64-row block, wave w the
//                                 columns w (mod 8), X staged through LDS as [column][fit] in panels of kFwPanel columns;
//                                 then z1, u1, T1 = z1 - u1 (and z1 - z1prev with the dual residual) and the m-block's
//                                 partial sums
//   l1c_transposed_kernel         per chunk: D read a second time: workgroup = 64 columns x a range of row blocks, the
//                                 64 x 64 block of D turned through LDS so that a lane owns a COLUMN and sums over rows
//                                 without cross-lane traffic; NV = 1 (T1) or 3 (T1, z1 - z1prev, u1) vectors per fit
//   l1c_gsum_kernel               multi_device.h's fixed-order sum of the partial rows
//   l1c_elem_kernel               over n: z2, u2, the next Y = D'T1 + (z2 - u2), the n-block's partial sums, the dual
//                                 residual's two norms, the penalty
//   l1c_fin_kernel                per fit pnorm, perr, dnorm, derr, the objective and the stop decision (admm.m:612-713)
// With groups set (admm_group_l1class_set_groups, q48) the element kernel is l1c_group_elem_kernel, the shared body of
// l1class_group_device.h over the plan's workgroups, reading GS; nothing else of the iteration changes.
// A fit whose stop flag is set is FROZEN: every kernel skips it.  No atomics; every sum runs in an order the sizes fix,
// independent of the chunk and slot a fit occupies: a fit duplicated into another chunk comes out bitwise equal.
// All loads of D are unconditional on clamped addresses (X and T are zero beyond n and m).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "l1class_device.h"
#include "l1class_group_device.h"
#include "multi_host.h"
#include "spmm.h"
#include "svm_cost_device.h"
#include "svm_ovr.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;
static_assert(kSpmmChunk == kOvrChunk, "one chunk for the n x n product and for the passes over D");

constexpr int kFwRows = 64, kFwWaves = 8, kFwThreads = kFwWaves * kWave;
constexpr int kFwPanel = 512;  // columns of X in LDS at a time: kFwPanel * KC * 8 B = 40 KB
constexpr int kFwStep = 8;     // loads of D a lane keeps in flight: one per column of a step of kFwWaves * kFwStep
constexpr int kFwSlots = (KC + kFwWaves - 1) / kFwWaves;  // fits whose element update one wave runs
static_assert(kFwPanel % (kFwWaves * kFwStep) == 0, "whole steps per panel");
static_assert(kFwWaves * KC * kFwRows <= kFwPanel * KC, "the wave sums reuse the panel's LDS");

constexpr int kTrTile = 64, kTrLd = kTrTile + 1, kTrWaves = 4, kTrThreads = kTrWaves * kWave;
constexpr int kTrPer = kTrTile / kTrWaves;  // columns a wave loads = rows a wave sums, per block of D
constexpr int kTrTarget = 1024;             // workgroups the row split aims at

constexpr int kFinThreads = 512;  // multi_slot_totals: 32 lanes per slot, LM_COUNT + LN_COUNT slots
static_assert((LM_COUNT + LN_COUNT) * 32 <= kFinThreads, "one 32-lane group per slot");

struct L1cFwdArgs {
  const double* D;
  int64_t ldD, m, n;
  const double* X;     // the chunk's [n][KC]
  double *Z1, *U1;     // [fit][ldz]
  double *T1, *DZ1;    // z1 - u1; z1 - z1prev (null without the dual residual)
  const double* ELL;   // [fit][ldz], or one column (ell_shared)
  const double* W;     // m weights or null
  const double* CC;    // K x 2 class costs
  const int32_t* loss;
  const MultiRec* rec;
  double* part;        // [fit][LM_COUNT][kMultiMaxWg]
  int64_t ldz;
  int32_t K, c0, ell_shared, objevals;
  double rho, C;
};

struct L1cTrArgs {
  const double* D;
  int64_t ldD, m, n;
  const double* V[3];  // [fit][ldz]: T1, z1 - z1prev, u1
  const MultiRec* rec;
  double* gpart;       // [row range][nv * Kp][ldx]
  int64_t ldz, ldx;
  int32_t K, Kp, c0, tiles_per;  // row blocks per row range
};

struct L1cElemArgs {
  int64_t n, ldx;
  const double* X;      // multi-vectors of len n
  double *Z2, *U2, *Y;
  const double* GS;     // [nv * Kp][ldx]: the summed partial rows
  const double* W;      // n l1 weights or null
  const double* par;    // K x 2: (lambda, mu)
  const int32_t* nonneg;
  const MultiRec* rec;
  double* part;         // [fit][LN_COUNT][kMultiMaxWg]
  int32_t K, Kp, dual, objevals;
  double rho;
};

// bit c: fit c0 + c exists and is still running
__device__ __forceinline__ uint32_t l1c_active(const MultiRec* rec, int32_t K, int32_t c0) {
  uint32_t actv = 0;
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int fit = c0 + c;
    const int32_t st = rec[fit < K ? fit : K - 1].stop;
    if (fit < K && st == 0) actv |= 1u << c;
  }
  return __builtin_amdgcn_readfirstlane(actv);
}

// LOGI: the chunk holds a logistic fit: the instantiation whose element update carries logistic_root (prox_device.h)
template <bool LOGI>
__global__ __launch_bounds__(kFwThreads) void l1c_forward_kernel(L1cFwdArgs a) {
  __shared__ __attribute__((aligned(16))) double sh[kFwPanel * KC];  // the panel [column][fit]; then the wave sums
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n = a.n, m = a.m;
  const uint32_t act = l1c_active(a.rec, a.K, a.c0);
  if (act == 0) return;  // every fit of the chunk has stopped: a no-op
  double acc[kFwSlots][LM_COUNT];
  SvmCostArgs ks[kFwSlots];
  int fits[kFwSlots];
#pragma unroll
  for (int s = 0; s < kFwSlots; ++s) {
#pragma unroll
    for (int q = 0; q < LM_COUNT; ++q) acc[s][q] = 0.0;
    const int c = w + kFwWaves * s;
    const int fit = (c < KC && a.c0 + c < a.K) ? a.c0 + c : a.K - 1;
    fits[s] = fit;
    ks[s] = SvmCostArgs{nullptr, a.CC[2 * fit], a.CC[2 * fit + 1], a.C, a.rho, a.loss[fit], a.objevals};
  }
  const int64_t nblocks = (m + kFwRows - 1) / kFwRows;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r = blk * kFwRows + lane;
    const int64_t rc = r < m ? r : m - 1;
    const double* __restrict__ drow = a.D + rc;
    double p[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) p[c] = 0.0;
    for (int64_t j0 = 0; j0 < n; j0 += kFwPanel) {
      const int np = static_cast<int>(n - j0 < kFwPanel ? n - j0 : kFwPanel);
      __syncthreads();  // the previous panel, or the previous block's wave sums, have been read
      for (int idx = tid; idx < kFwPanel * KC; idx += kFwThreads)
        sh[idx] = idx < np * KC ? a.X[j0 * KC + idx] : 0.0;  // (zero beyond n: the clamped columns add nothing)
      __syncthreads();
      for (int jb = 0; jb < np; jb += kFwWaves * kFwStep) {
        double d[kFwStep];
#pragma unroll
        for (int k = 0; k < kFwStep; ++k) {
          const int64_t j = j0 + jb + w + kFwWaves * k;
          d[k] = drow[(j < n ? j : n - 1) * a.ldD];
        }
#pragma unroll
        for (int k = 0; k < kFwStep; ++k) {
          const double* __restrict__ xk = sh + (jb + w + kFwWaves * k) * KC;  // same address in every lane: broadcast
#pragma unroll
          for (int c = 0; c < KC; ++c) p[c] = __builtin_fma(d[k], xk[c], p[c]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < KC; ++c) sh[(w * KC + c) * kFwRows + lane] = p[c];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kFwSlots; ++s) {
      const int c = w + kFwWaves * s;
      if (c < KC && ((act >> c) & 1u) && r < m) {  // (c and act are wave-uniform)
        double ax = sh[c * kFwRows + lane];
#pragma unroll
        for (int q = 1; q < kFwWaves; ++q) ax += sh[(q * KC + c) * kFwRows + lane];
        const int64_t e = static_cast<int64_t>(fits[s]) * a.ldz + r;
        const double zp = a.Z1[e], uo = a.U1[e];
        const double el = a.ELL[(a.ell_shared ? 0 : static_cast<int64_t>(fits[s]) * a.ldz) + r];
        const double wv = a.W ? a.W[r] : 1.0;
        const double ci = svm_cost_of(ks[s], wv, el);
        const double zn = svm_cost_prox_elem<LOGI>(ks[s], ci, el, ax + uo);
        const double rr = ax - zn;      // A x + B z - c
        const double un = uo + rr;      // admm.m:542-550
        acc[s][LM_R2] += rr * rr;
        acc[s][LM_AX2] += ax * ax;
        acc[s][LM_Z2] += zn * zn;
        if (a.objevals) acc[s][LM_LOSS] += svm_cost_obj_elem<LOGI>(ks[s], ci, el * ax);
        a.Z1[e] = zn;
        a.U1[e] = un;
        a.T1[e] = zn - un;
        if (a.DZ1) a.DZ1[e] = zn - zp;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kFwSlots; ++s) {
    const int c = w + kFwWaves * s;
    if (c < KC && ((act >> c) & 1u)) {
#pragma unroll
      for (int q = 0; q < LM_COUNT; ++q) {
        const double v = wave_sum(acc[s][q]);
        if (lane == 0) a.part[(static_cast<int64_t>(fits[s]) * LM_COUNT + q) * kMultiMaxWg + blockIdx.x] = v;
      }
    }
  }
}

// before the first iteration: T1 = z1 - u1 of the start vectors
__global__ __launch_bounds__(kBlock) void l1c_t1_kernel(const double* __restrict__ Z1, const double* __restrict__ U1,
                                                        double* __restrict__ T1, int64_t m, int64_t ldz) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t e = static_cast<int64_t>(blockIdx.y) * ldz + i;
  if (i < m) T1[e] = (0.0 + Z1[e]) - U1[e];
}

// workgroup (x, y): the columns 64 x .. 64 x + 63 and the row blocks y * tiles_per .. of the chunk's NV * KC vectors.
// Wave w loads the columns 16 w .. 16 w + 15 of a block (lane = row: coalesced) into LDS, then lane = column sums the
// rows 16 w .. 16 w + 15 with the vectors' values broadcast from LDS; the next block's loads are in flight meanwhile.
// The four wave sums are added in wave order.
template <int NV>
__global__ __launch_bounds__(kTrThreads) void l1c_transposed_kernel(L1cTrArgs a) {
  constexpr int NQ = NV * KC;
  __shared__ double tile[kTrTile * kTrLd];  // [column][row]; at the end the four wave sums of one vector
  __shared__ __attribute__((aligned(16))) double ts[kTrTile * NQ];  // [row][vector][fit]
  static_assert(kTrWaves * KC * kTrTile <= kTrTile * kTrLd, "the wave sums reuse the tile's LDS");
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n = a.n, m = a.m;
  const uint32_t act = l1c_active(a.rec, a.K, a.c0);
  if (act == 0) return;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kTrTile;
  const int64_t ntiles = (m + kTrTile - 1) / kTrTile;
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * a.tiles_per;
  const int64_t t1 = t0 + a.tiles_per < ntiles ? t0 + a.tiles_per : ntiles;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  double d[kTrPer];
  auto load = [&](int64_t t) {
    const int64_t r = t * kTrTile + lane;
    const double* __restrict__ drow = a.D + (r < m ? r : m - 1);
#pragma unroll
    for (int k = 0; k < kTrPer; ++k) {
      const int64_t j = j0 + w * kTrPer + k;
      d[k] = drow[(j < n ? j : n - 1) * a.ldD];
    }
  };
  if (t0 < t1) load(t0);
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t i0 = t * kTrTile;
    for (int idx = tid; idx < kTrTile * NQ; idx += kTrThreads) {
      const int row = idx & (kTrTile - 1), q = idx / kTrTile;
      const int v = q / KC, c = q - v * KC;
      double tv = 0.0;  // rows beyond m and fits that do not run add nothing
      const double* __restrict__ vp = v == 0 ? a.V[0] : (v == 1 ? a.V[1] : a.V[2]);
      if (i0 + row < m && ((act >> c) & 1u)) tv = vp[static_cast<int64_t>(a.c0 + c) * a.ldz + i0 + row];
      ts[row * NQ + q] = tv;
    }
#pragma unroll
    for (int k = 0; k < kTrPer; ++k) tile[(w * kTrPer + k) * kTrLd + lane] = d[k];
    __syncthreads();
    if (t + 1 < t1) load(t + 1);
#pragma unroll 4
    for (int i = 0; i < kTrPer; ++i) {
      const int row = w * kTrPer + i;
      const double dv = tile[lane * kTrLd + row];
      const double* __restrict__ tp = ts + row * NQ;  // same address in every lane: broadcast
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = __builtin_fma(dv, tp[q], acc[q]);
    }
    __syncthreads();  // the block has been read: the next one may overwrite it
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int c = 0; c < KC; ++c) tile[(w * KC + c) * kTrTile + lane] = acc[v * KC + c];
    __syncthreads();
    for (int idx = tid; idx < KC * kTrTile; idx += kTrThreads) {
      const int c = idx / kTrTile, l = idx & (kTrTile - 1);
      if (j0 + l < n && ((act >> c) & 1u)) {
        const double s = ((tile[c * kTrTile + l] + tile[(KC + c) * kTrTile + l]) + tile[(2 * KC + c) * kTrTile + l]) +
                         tile[(3 * KC + c) * kTrTile + l];
        a.gpart[((static_cast<int64_t>(blockIdx.y) * NV + v) * a.Kp + a.c0 + c) * a.ldx + j0 + l] = s;
      }
    }
    __syncthreads();
  }
}
static_assert(kTrWaves == 4, "the transposed pass adds four wave sums");

// blockIdx.y = vector * Kp + fit, blockIdx.x = 64 columns: GS = the sum over the row ranges' partial rows
__global__ __launch_bounds__(kBlock) void l1c_gsum_kernel(const double* gpart, double* gsum, int64_t ldx, int64_t n,
                                                          int32_t K, int32_t Kp, int32_t nvk, int32_t nranges,
                                                          const MultiRec* rec) {
  __shared__ double sq[4][kMultiTile];
  const int fit = static_cast<int>(blockIdx.y) % Kp;
  if (fit >= K || rec[fit].stop) return;
  multi_gsum_tile(gpart, gsum, static_cast<int>(blockIdx.y), ldx, n, nvk, nranges, sq);
}

// blockIdx.y = fit, a thread per coefficient (grid-stride over at most kMultiMaxWg workgroups).  INIT: only
// Y = D'(z1 - u1) + (z2 - u2) of the start vectors
template <bool INIT>
__global__ __launch_bounds__(kBlock) void l1c_elem_kernel(L1cElemArgs a) {
  __shared__ double red[LN_COUNT][4];
  const int fit = blockIdx.y;
  if (a.rec[fit].stop) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t base = static_cast<int64_t>(fit / KC) * a.n * KC + fit % KC;
  const double lam = a.par[2 * fit], mu = a.par[2 * fit + 1];
  // engine_run_general.hip's own expressions for the family's numbers
  const PenaltyArgs pen{a.W, lam / a.rho, a.rho / (a.rho + mu), lam, 0.0, 0.5 * mu, a.nonneg[fit]};
  const double* __restrict__ g1 = a.GS + static_cast<int64_t>(fit) * a.ldx;
  const double* __restrict__ g2 = a.GS + static_cast<int64_t>(a.Kp + fit) * a.ldx;
  const double* __restrict__ g3 = a.GS + static_cast<int64_t>(2 * a.Kp + fit) * a.ldx;
  double acc[LN_COUNT];
#pragma unroll
  for (int q = 0; q < LN_COUNT; ++q) acc[q] = 0.0;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + tid; j < a.n; j += static_cast<int64_t>(gridDim.x) * kBlock) {
    l1c_elem_update<INIT>(pen, a.X, a.Z2, a.U2, a.Y, base + j * KC, j, g1, g2, g3, j, a.dual, a.objevals, acc);
  }
  if (INIT) return;
#pragma unroll
  for (int q = 0; q < LN_COUNT; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) red[q][wid] = v;
  }
  __syncthreads();
  if (tid < LN_COUNT)
    a.part[(static_cast<int64_t>(fit) * LN_COUNT + tid) * kMultiMaxWg + blockIdx.x] =
        ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// the grouped form (q48): l1class_group_device.h's body; g1, g2, g3 are the rows fit, Kp + fit and 2 Kp + fit of GS
__global__ __launch_bounds__(kScgBlock) void l1c_group_elem_kernel(L1cGroupElemArgs a, GroupPlan gp,
                                                                   const double* __restrict__ GS, int64_t ldx, int32_t Kp) {
  __shared__ double lds[kL1cGroupLds];
  __shared__ double sq[kScgBlock];
  __shared__ double gacc[kGmMaxGroups * KC];
  l1c_group_elem_body(
      a, gp,
      [&](int q, const ScgLane& l, int64_t, int64_t j) { return GS[(static_cast<int64_t>(q) * Kp + l.fit) * ldx + j]; },
      lds, sq, gacc);
}

// blockIdx.x = fit: admm.m:612-658, 706-713 as oracle/admm_ref.py restates it for A = [D; I], B = -1, c = 0, plain ADMM
// with stopcond = 'standard': every norm over the m + n stacked elements
__global__ __launch_bounds__(kFinThreads) void l1c_fin_kernel(L1cFinArgs a) {
  const int fit = blockIdx.x;
  MultiRec* rec = a.rec + fit;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[LM_COUNT + LN_COUNT];
  multi_slot_totals(a.mpart, fit, LM_COUNT, a.nwg_m, S);
  multi_slot_totals(a.npart, fit, LN_COUNT, a.nwg_n, S, LM_COUNT);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double* Sn = S + LM_COUNT;
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(fit) * a.hist_ld + it;
  if (a.objevals) a.objv[h] = a.C * S[LM_LOSS] + Sn[LN_PEN];
  const double sq = sqrt(static_cast<double>(a.m + a.n));
  const double pn = sqrt(S[LM_R2] + Sn[LN_R2]);                                                        // admm.m:621
  const double pe = sq * a.abstol + a.reltol * fmax(sqrt(S[LM_AX2] + Sn[LN_X2]), sqrt(S[LM_Z2] + Sn[LN_Z2]));  // :644-650
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  bool dual_ok = true;
  if (a.dual) {
    const double dn = a.rho * sqrt(Sn[LN_DZ2]);                               // admm.m:624
    const double de = sq * a.abstol + a.reltol * (a.rho * sqrt(Sn[LN_DU2]));  // admm.m:652-654
    a.dnorm[h] = dn;
    a.derr[h] = de;
    dual_ok = dn < de;
  }
  const bool stop = !a.domaxiters && pn < pe && dual_ok;  // admm.m:710-713
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

// the triangular solves take one contiguous vector per fit: col[k][ld] <- the fit's column of a multi-vector, and back
// for the running fits
__global__ __launch_bounds__(kBlock) void l1c_gather_kernel(const double* __restrict__ V, int64_t n, double* __restrict__ col,
                                                            int64_t ld) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int32_t k = blockIdx.y;
  if (i < n) col[k * ld + i] = V[(static_cast<int64_t>(k / KC) * n + i) * KC + k % KC];
}

__global__ __launch_bounds__(kBlock) void l1c_scatter_kernel(const double* __restrict__ col, int64_t ld, int64_t n,
                                                             const MultiRec* __restrict__ rec, double* __restrict__ V) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int32_t k = blockIdx.y;
  if (i < n && rec[k].stop == 0) V[(static_cast<int64_t>(k / KC) * n + i) * KC + k % KC] = col[k * ld + i];
}

}  // namespace

void launch_l1c_fin(const L1cFinArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(l1c_fin_kernel, dim3(static_cast<unsigned>(a.K)), dim3(kFinThreads), 0, stream, a);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_l1class : admm::MultiHost {
  admm_engine* eng = nullptr;  // an ordinary ADMM_PROB_LASSO engine with rho = 1: D, the factor, the inverse
  int64_t m = 0, n = 0, ldz = 0, ldx = 0, ldt = 0;
  int32_t chunks = 0, Kp = 0, nwg_m = 0, nwg_n = 0, tiles_per = 0, nranges = 0, ell_shared = 0;
  double C = 1.0;
  admm::SymvPlan plan{};
  const double* P = nullptr;   // fp64 tile-packed inverse of D'D + I (null: the triangular solves)
  double* spart = nullptr;     // partial rows of the n x n product
  double *ycol = nullptr, *xcol = nullptr;  // [K][ldt]: the triangular solves' vectors
  double *X = nullptr, *Y = nullptr, *Z2 = nullptr, *U2 = nullptr;  // multi-vectors of len n
  double *Z1 = nullptr, *U1 = nullptr, *T1 = nullptr, *DZ1 = nullptr, *ELL = nullptr;  // [Kp][ldz] (ELL: or one column)
  double *gpart = nullptr, *GS = nullptr;  // [nranges][3 Kp][ldx], [3 Kp][ldx]
  double *mpart = nullptr, *npart = nullptr;
  double *W = nullptr, *CC = nullptr, *LW = nullptr, *par = nullptr;
  int32_t *loss = nullptr, *nonneg = nullptr;
  std::vector<int32_t> loss_host;
  std::vector<double> cost_host;
  std::vector<char> chunk_logistic;
  double *pnorm = nullptr, *perr = nullptr, *dnorm = nullptr, *derr = nullptr, *objv = nullptr;  // histories
  int64_t launches = 0, d_passes = 0;
  admm::GroupMulti grp;  // admm_group_l1class_set_groups (q48)
  admm_l1class_options last{};
};

namespace {

using namespace admm;

const char* kPerFit = ": run admm() with A = [D; I] per fit instead";

int l1c_setup(admm_l1class* o, const admm_l1class_desc* desc, const std::vector<double>& ph,
              const std::vector<int32_t>& nh) {
  const int64_t m = desc->m, n = desc->n;
  const int32_t K = desc->K;
  // the engine builds the n x n factor for m >= n alone: a fat D gets n - m zero rows, which D'D does not see
  const int64_t me = std::max(m, n);
  std::vector<double> pad, zeros(static_cast<size_t>(me), 0.0);
  admm_problem_desc d;
  admm_problem_desc_default(&d);
  d.problem = ADMM_PROB_LASSO;
  d.m = me;
  d.n = n;
  d.D = desc->D;
  d.ldD = desc->ldD;
  if (me != m) {
    pad.assign(static_cast<size_t>(me) * n, 0.0);
    for (int64_t j = 0; j < n; ++j)
      std::memcpy(pad.data() + j * me, desc->D + j * desc->ldD, sizeof(double) * m);
    d.D = pad.data();
    d.ldD = me;
  }
  d.s = zeros.data();  // (the engine wants one response; it never runs)
  d.lambda = 0.0;
  d.rho = 1.0;  // D'D + I
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
  o->C = desc->C;
  o->chunks = spmm_chunks(K);
  o->Kp = o->chunks * KC;
  o->ldz = round_up(m, 2);
  o->ldx = round_up(n, 2);
  o->ldt = round_up(n, 2);
  o->nwg_m = ovr_pass_workgroups(m);
  o->nwg_n = grid_blocks(n, kBlock, kMultiMaxWg);
  {  // the transposed pass: about kTrTarget workgroups, whole row blocks per row range
    const int64_t tiles = ceil_div(m, int64_t{kTrTile}), strips = ceil_div(n, int64_t{kTrTile});
    const int64_t want = std::min<int64_t>(std::max<int64_t>(ceil_div(int64_t{kTrTarget}, strips), 1), tiles);
    o->tiles_per = static_cast<int32_t>(ceil_div(tiles, want));
    o->nranges = static_cast<int32_t>(ceil_div(tiles, int64_t{o->tiles_per}));
  }
  const SliceFactor& f = e->xfac;
  const size_t kp = static_cast<size_t>(o->Kp);
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
  for (double** p : {&o->X, &o->Y, &o->Z2, &o->U2}) {
    ADMM_TRY(o->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, o->stream));
  }
  for (double** p : {&o->Z1, &o->U1, &o->T1, &o->DZ1}) {
    ADMM_TRY(o->mem.alloc(p, kp * o->ldz));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * o->ldz, o->stream));
  }
  o->ell_shared = desc->nell == 1 && K > 1 ? 1 : 0;
  const int32_t ecols = o->ell_shared ? 1 : K;
  ADMM_TRY(o->mem.alloc(&o->ELL, static_cast<size_t>(ecols) * o->ldz));
  ADMM_HIP_TRY(hipMemsetAsync(o->ELL, 0, sizeof(double) * ecols * o->ldz, o->stream));
  ADMM_TRY(upload_cols(*o, o->ELL, o->ldz, desc->ELL, m, ecols, ADMM_MEM_HOST));
  ADMM_TRY(o->mem.alloc(&o->gpart, static_cast<size_t>(o->nranges) * 3 * kp * o->ldx));
  ADMM_TRY(o->mem.alloc(&o->GS, 3 * kp * o->ldx));
  ADMM_HIP_TRY(hipMemsetAsync(o->GS, 0, sizeof(double) * 3 * kp * o->ldx, o->stream));
  ADMM_TRY(o->mem.alloc(&o->mpart, kp * LM_COUNT * kMultiMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->mpart, 0, sizeof(double) * kp * LM_COUNT * kMultiMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->npart, kp * LN_COUNT * kMultiMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->npart, 0, sizeof(double) * kp * LN_COUNT * kMultiMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(2) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_words(*o, &o->nonneg, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->nonneg, nh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->loss_host.assign(static_cast<size_t>(K), ADMM_LOSS_LOGISTIC);
  if (desc->loss) o->loss_host.assign(desc->loss, desc->loss + K);
  o->chunk_logistic.assign(static_cast<size_t>(o->chunks), 0);
  for (int32_t k = 0; k < K; ++k)
    if (o->loss_host[k] == ADMM_LOSS_LOGISTIC) o->chunk_logistic[k / KC] = 1;
  ADMM_TRY(alloc_words(*o, &o->loss, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->loss, o->loss_host.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->cost_host.assign(static_cast<size_t>(2 * K), 1.0);
  ADMM_TRY(o->mem.alloc(&o->CC, static_cast<size_t>(2 * K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, o->cost_host.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(alloc_common(*o));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the host vectors and the caller's buffers were read)
  ADMM_HIP_TRY(hipGetLastError());
  if (desc->l1weights) ADMM_TRY(set_shared_weights(*o, n, desc->l1weights, &o->LW));
  return ADMM_OK;
}

// host (m + n) x K column-major <-> Z1 / U1 ([fit][ldz]) above Z2 / U2 (a chunked multi-vector)
int l1c_upload_stacked(admm_l1class* o, const double* src, double* V1, double* V2) {
  const size_t kp = static_cast<size_t>(o->Kp);
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(V1, 0, sizeof(double) * kp * o->ldz, o->stream));
    ADMM_HIP_TRY(hipMemsetAsync(V2, 0, sizeof(double) * kp * o->n, o->stream));
    return ADMM_OK;
  }
  const int64_t mn = o->m + o->n;
  ADMM_HIP_TRY(hipMemcpy2DAsync(V1, o->ldz * sizeof(double), src, mn * sizeof(double), o->m * sizeof(double), o->K,
                                hipMemcpyHostToDevice, o->stream));
  std::vector<double> hb(kp * o->n);
  spmm_pack(src + o->m, mn, o->n, o->K, hb.data());
  ADMM_HIP_TRY(hipMemcpyAsync(V2, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (hb goes out of scope)
  return ADMM_OK;
}

int l1c_fetch_n(admm_l1class* o, const double* src, double* dst, int64_t ld) {
  std::vector<double> hb(static_cast<size_t>(o->Kp) * o->n);
  ADMM_HIP_TRY(hipMemcpy(hb.data(), src, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
  spmm_unpack(hb.data(), o->n, o->K, dst, ld);
  return ADMM_OK;
}

int l1c_fetch_stacked(admm_l1class* o, const double* V1, const double* V2, double* dst, size_t cap, size_t* written) {
  const int64_t mn = o->m + o->n;
  const size_t need = static_cast<size_t>(mn) * o->K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  ADMM_HIP_TRY(hipMemcpy2D(dst, mn * sizeof(double), V1, o->ldz * sizeof(double), o->m * sizeof(double), o->K,
                           hipMemcpyDeviceToHost));
  ADMM_TRY(l1c_fetch_n(o, V2, dst + o->m, mn));
  if (written) *written = need;
  return ADMM_OK;
}

// X <- inv(D'D + I) Y for every running fit; returns the number of launches
int l1c_xupdate(admm_l1class* o) {
  if (o->P) {
    launch_symm_packed(o->plan, o->P, o->Y, o->X, o->spart, o->rec, o->K, o->stream);
    return 2;
  }
  const dim3 grid(static_cast<unsigned>(ceil_div(o->n, int64_t{kBlock})), static_cast<unsigned>(o->K));
  hipLaunchKernelGGL(l1c_gather_kernel, grid, dim3(kBlock), 0, o->stream, o->Y, o->n, o->ycol, o->ldt);
  for (int32_t k = 0; k < o->K; ++k)
    launch_trsv_pair(o->eng->xfac.trsv, o->ycol + static_cast<int64_t>(k) * o->ldt,
                     o->xcol + static_cast<int64_t>(k) * o->ldt, nullptr, o->stream);
  hipLaunchKernelGGL(l1c_scatter_kernel, grid, dim3(kBlock), 0, o->stream, o->xcol, o->ldt, o->n, o->rec, o->X);
  return o->K + 2;
}

L1cFwdArgs l1c_fwd_args(const admm_l1class* o, bool dual, int32_t objevals, double rho) {
  L1cFwdArgs a{};
  a.D = o->eng->D;
  a.ldD = o->eng->ldD;
  a.m = o->m;
  a.n = o->n;
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
  a.ldz = o->ldz;
  a.K = o->K;
  a.ell_shared = o->ell_shared;
  a.objevals = objevals;
  a.rho = rho;
  a.C = o->C;
  return a;
}

L1cTrArgs l1c_tr_args(const admm_l1class* o) {
  L1cTrArgs a{};
  a.D = o->eng->D;
  a.ldD = o->eng->ldD;
  a.m = o->m;
  a.n = o->n;
  a.V[0] = o->T1;
  a.V[1] = o->DZ1;
  a.V[2] = o->U1;
  a.rec = o->rec;
  a.gpart = o->gpart;
  a.ldz = o->ldz;
  a.ldx = o->ldx;
  a.K = o->K;
  a.Kp = o->Kp;
  a.tiles_per = o->tiles_per;
  return a;
}

void l1c_launch_forward(const admm_l1class* o, L1cFwdArgs a, int32_t ch) {
  a.c0 = ch * KC;
  a.X = o->X + static_cast<int64_t>(ch) * o->n * KC;
  const dim3 grid(static_cast<unsigned>(o->nwg_m)), block(kFwThreads);
  if (o->chunk_logistic[ch]) hipLaunchKernelGGL(l1c_forward_kernel<true>, grid, block, 0, o->stream, a);
  else hipLaunchKernelGGL(l1c_forward_kernel<false>, grid, block, 0, o->stream, a);
}

void l1c_launch_transposed(const admm_l1class* o, L1cTrArgs a, int32_t ch, int nv) {
  a.c0 = ch * KC;
  const dim3 grid(static_cast<unsigned>(ceil_div(o->n, int64_t{kTrTile})), static_cast<unsigned>(o->nranges));
  if (nv == 3) hipLaunchKernelGGL(l1c_transposed_kernel<3>, grid, dim3(kTrThreads), 0, o->stream, a);
  else hipLaunchKernelGGL(l1c_transposed_kernel<1>, grid, dim3(kTrThreads), 0, o->stream, a);
}

void l1c_launch_gsum(const admm_l1class* o, int nv) {
  const dim3 grid(static_cast<unsigned>(ceil_div(o->n, int64_t{kMultiTile})), static_cast<unsigned>(nv * o->Kp));
  hipLaunchKernelGGL(l1c_gsum_kernel, grid, dim3(kBlock), 0, o->stream, o->gpart, o->GS, o->ldx, o->n, o->K, o->Kp,
                     nv * o->Kp, o->nranges, o->rec);
}

}  // namespace

extern "C" {

void admm_l1class_desc_default(admm_l1class_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_l1class_desc);
  d->K = 1;
  d->nell = 1;
  d->C = 1.0;
  d->xsolve = ADMM_XSOLVE_AUTO;
}

void admm_l1class_options_default(admm_l1class_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_l1class_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
  o->nodualerror = 0;  // admm.m:76
}

int admm_l1class_chunk(void) { return KC; }

int admm_l1class_create(const admm_l1class_desc* desc, admm_l1class** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_l1class_desc)))
    return fail(ADMM_E_INVALID, "admm_l1class_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the l1 classifier needs at least one fit (K >= 1)");
  if (!desc->D || desc->m <= 0 || desc->n <= 0 || desc->ldD < desc->m)
    return fail(ADMM_E_INVALID, "the l1 classifier needs D (m x n, ldD >= m)");
  if (!desc->ELL) return fail(ADMM_E_INVALID, "the l1 classifier needs the labels ELL (m x nell)");
  if (desc->nell != 1 && desc->nell != desc->K)
    return fail(ADMM_E_INVALID, "ELL has " + std::to_string(desc->nell) + " columns: one shared label column or one per "
                                "fit (" + std::to_string(desc->K) + ")");
  if (!desc->lambda) return fail(ADMM_E_INVALID, "the l1 classifier needs lambda (K values)");
  if (!finite_pos(desc->C)) return fail(ADMM_E_INVALID, "desc.C must be positive and finite");
  std::vector<double> ph;
  std::vector<int32_t> nh, lh;
  ADMM_TRY(check_l1class_fits(desc->K, desc->loss, desc->lambda, desc->ridge, desc->nonneg, &lh, &ph, &nh));
  ADMM_TRY(check_labels(desc->ELL, desc->m, desc->nell));
  ADMM_TRY(check_l1_weights(desc->l1weights, desc->n));
  if (desc->xsolve != ADMM_XSOLVE_AUTO && desc->xsolve != ADMM_XSOLVE_INVERSE && desc->xsolve != ADMM_XSOLVE_TRSV)
    return fail(ADMM_E_UNSUPPORTED, std::string("the l1 classifier applies the cached factor (xsolve = auto, inverse or "
                                                "trsv)") + kPerFit);
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, std::string("the l1 classifier is not row-sharded") + kPerFit);
  return create_object(out, admm_l1class_destroy, [&](admm_l1class* o) { return l1c_setup(o, desc, ph, nh); });
}

int admm_l1class_run(admm_l1class* o, const admm_l1class_options* opts, admm_l1class_summary* summaries,
                     double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_l1class_options)))
    return fail(ADMM_E_INVALID, "admm_l1class_options.struct_size mismatch (ABI version skew)");
  admm_l1class_options op = *opts;
  ADMM_TRY(check_run_options("l1 classifier", kPerFit, &op));
  if (!finite_pos(op.rho)) return fail(ADMM_E_INVALID, "options.rho must be positive and finite");
  const bool dual = op.nodualerror == 0;
  const int nv = dual ? 3 : 1;
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->dnorm, &o->derr, &o->objv}, N));
  ADMM_TRY(begin_run(*o));
  ADMM_HIP_TRY(hipMemsetAsync(o->X, 0, sizeof(double) * o->Kp * o->n, o->stream));
  ADMM_TRY(l1c_upload_stacked(o, op.z0, o->Z1, o->Z2));
  ADMM_TRY(l1c_upload_stacked(o, op.u0, o->U1, o->U2));

  const L1cFwdArgs fw = l1c_fwd_args(o, dual, op.objevals, op.rho);
  const L1cTrArgs tr = l1c_tr_args(o);
  L1cElemArgs ea{};
  ea.n = o->n;
  ea.ldx = o->ldx;
  ea.X = o->X;
  ea.Z2 = o->Z2;
  ea.U2 = o->U2;
  ea.Y = o->Y;
  ea.GS = o->GS;
  ea.W = o->LW;
  ea.par = o->par;
  ea.nonneg = o->nonneg;
  ea.rec = o->rec;
  ea.part = o->npart;
  ea.K = K;
  ea.Kp = o->Kp;
  ea.dual = dual ? 1 : 0;
  ea.objevals = op.objevals;
  ea.rho = op.rho;
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
  const dim3 egrid(static_cast<unsigned>(o->nwg_n), static_cast<unsigned>(K));
  const L1cGroupElemArgs ga{ea.n, ea.X, ea.Z2, ea.U2, ea.Y, ea.W, ea.par, o->grp.l1, ea.nonneg, ea.rec, ea.part, K, ea.dual,
                            ea.objevals, ea.rho};
  const dim3 ggrid(static_cast<unsigned>(o->grp.plan.nwg), static_cast<unsigned>(o->chunks));
  int64_t launches = 0, d_passes = 0;

  ADMM_TRY(begin_timing(*o));
  {  // Y = D'(z1 - u1) + (z2 - u2) of the start vectors
    const dim3 grid(static_cast<unsigned>(ceil_div(o->m, int64_t{kBlock})), static_cast<unsigned>(K));
    hipLaunchKernelGGL(l1c_t1_kernel, grid, dim3(kBlock), 0, o->stream, o->Z1, o->U1, o->T1, o->m, o->ldz);
    for (int32_t ch = 0; ch < o->chunks; ++ch) l1c_launch_transposed(o, tr, ch, 1);
    l1c_launch_gsum(o, 1);
    hipLaunchKernelGGL(l1c_elem_kernel<true>, egrid, dim3(kBlock), 0, o->stream, ea);
    launches += 3 + o->chunks;
    d_passes += o->chunks;
  }
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    launches += l1c_xupdate(o);
    for (int32_t ch = 0; ch < o->chunks; ++ch) l1c_launch_forward(o, fw, ch);
    for (int32_t ch = 0; ch < o->chunks; ++ch) l1c_launch_transposed(o, tr, ch, nv);
    l1c_launch_gsum(o, nv);
    if (o->grp.on())
      hipLaunchKernelGGL(l1c_group_elem_kernel, ggrid, dim3(kScgBlock), 0, o->stream, ga, o->grp.plan, o->GS, o->ldx, o->Kp);
    else
      hipLaunchKernelGGL(l1c_elem_kernel<false>, egrid, dim3(kBlock), 0, o->stream, ea);
    launch_l1c_fin(fa, o->stream);
    launches += 2 * o->chunks + 3;
    d_passes += 2 * o->chunks;
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the l1 classifier loop ended with fits still running", N, op.objevals != 0, o->objv,
                      runtime_s, summaries));
  for (int32_t c = 0; summaries && c < K; ++c) summaries[c].xsolve = o->P ? ADMM_XSOLVE_INVERSE : ADMM_XSOLVE_TRSV;
  o->launches = launches;
  o->d_passes = d_passes;
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_l1class_set_cost(admm_l1class* o, const double* weights, const double* class_cost) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_svm_cost(*o, o->m, weights, class_cost, &o->W, o->CC, &o->cost_host);
}

int admm_l1class_set_l1weights(admm_l1class* o, const double* l1weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  ADMM_TRY(check_l1_weights(l1weights, o->n));  // (the message of the create-time check; a refused call changes nothing)
  return set_shared_weights(*o, o->n, l1weights, &o->LW);
}

int admm_group_l1class_set_groups(admm_l1class* o, int32_t G, const int64_t* sizes, const double* groupweights,
                            const double* l1) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_multi_groups(*o, o->n, G, sizes, groupweights, l1, &o->grp);
}

int admm_l1class_launches(admm_l1class* o, int64_t* launches, int64_t* d_passes) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (!o->has_run) return fail(ADMM_E_INVALID, "launches before the first run");
  if (launches) *launches = o->launches;
  if (d_passes) *d_passes = o->d_passes;
  return ADMM_OK;
}

int admm_l1class_pass_time(admm_l1class* o, int32_t reps, int32_t nvec, double* forward_us, double* transposed_us,
                           int64_t* d_bytes) {
  if (!o || reps < 1 || (nvec != 1 && nvec != 3)) return fail(ADMM_E_INVALID, "object is NULL, reps < 1 or nvec not 1 | 3");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  ADMM_TRY(begin_run(*o));  // every fit runs; the iterates are overwritten, as the next run's start does anyway
  const L1cFwdArgs fw = l1c_fwd_args(o, nvec == 3, 1, 1.0);
  const L1cTrArgs tr = l1c_tr_args(o);
  double* outs[2] = {forward_us, transposed_us};
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<float> ms(static_cast<size_t>(reps));
    for (int32_t i = -1; i < reps; ++i) {  // (i = -1: warm-up)
      ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
      if (pass == 0) l1c_launch_forward(o, fw, 0);
      else l1c_launch_transposed(o, tr, 0, nvec);
      ADMM_HIP_TRY(hipEventRecord(o->ev1, o->stream));
      ADMM_HIP_TRY(hipEventSynchronize(o->ev1));
      if (i >= 0) ADMM_HIP_TRY(hipEventElapsedTime(&ms[i], o->ev0, o->ev1));
    }
    std::sort(ms.begin(), ms.end());
    if (outs[pass]) *outs[pass] = 1e3 * static_cast<double>(ms[reps / 2]);
  }
  ADMM_HIP_TRY(hipGetLastError());
  if (d_bytes) *d_bytes = 8 * o->m * o->n;
  return ADMM_OK;
}

int admm_l1class_fetch(admm_l1class* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_L1C_F_XOPT: {
      const size_t need = static_cast<size_t>(o->n) * o->K;
      if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
      ADMM_TRY(l1c_fetch_n(o, o->X, dst, o->n));
      if (written) *written = need;
      return ADMM_OK;
    }
    case ADMM_L1C_F_ZOPT: return l1c_fetch_stacked(o, o->Z1, o->Z2, dst, cap, written);
    case ADMM_L1C_F_UOPT: return l1c_fetch_stacked(o, o->U1, o->U2, dst, cap, written);
    case ADMM_L1C_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_L1C_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_L1C_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    case ADMM_L1C_F_DNORM: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->dnorm, dst, cap, written);
    case ADMM_L1C_F_DERR: return fetch_kept_history(*o, !o->last.nodualerror, kNoDual, o->derr, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the l1 classifier");
  }
}

void admm_l1class_destroy(admm_l1class* o) {
  if (!o) return;
  destroy_common(*o);
  if (o->eng) admm_engine_destroy(o->eng);
  delete o;
}

}  // extern "C"
