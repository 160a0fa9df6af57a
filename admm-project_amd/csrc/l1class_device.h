// l1class_device.h -- what the two sparse-linear-classifier objects share (l1class.hip, a dense D; q43:
// sparse_l1class.hip, a sparse D): the slots of the block partials over the m rows and over the n coefficients, the
// element update of one coefficient -- z2, u2, the next right-hand side and the n-block's sums -- and the per-fit
// finalize, which is ONE kernel (l1class.hip's l1c_fin_kernel) behind launch_l1c_fin.  Both objects write their block
// partials as part[(fit * count + slot) * kMultiMaxWg + workgroup], so the finalize reads either.
#pragma once
#include "multi_device.h"
#include "penalty_device.h"

namespace admm {

// sums of the pass over m, and of the element kernel over n (admm.m:621-654 over the stacked vector)
enum L1cMSlot : int32_t { LM_R2 = 0, LM_AX2 = 1, LM_Z2 = 2, LM_LOSS = 3, LM_COUNT = 4 };
enum L1cNSlot : int32_t { LN_R2 = 0, LN_X2 = 1, LN_Z2 = 2, LN_DZ2 = 3, LN_DU2 = 4, LN_PEN = 5, LN_COUNT = 6 };

struct L1cFinArgs {
  const double *mpart, *npart;
  int64_t m, n;
  int32_t K, nwg_m, nwg_n, dual;
  MultiRec* rec;
  double *pnorm, *perr, *dnorm, *derr, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, C, abstol, reltol;
  int32_t domaxiters, objevals, maxiters;
};

// one workgroup per fit: pnorm, perr, dnorm, derr, the objective and the stop decision (admm.m:612-713)
void launch_l1c_fin(const L1cFinArgs& a, hipStream_t stream);

constexpr int kL1cModelFinThreads = 512;  // multi_slot_totals: 32 lanes per slot, LM_COUNT + LN_COUNT slots

#ifdef __HIPCC__
// The finalize of one multinomial model (q49) whose `classes` fits start at fit0, by one workgroup of
// kL1cModelFinThreads threads: multi_slot_totals per class over the m-partials and the n-partials, the classes added in
// class order, then admm.m's stop rule ONCE over the (m + n)*classes stacked elements; the histories go to the row of
// every class and the same record to all of them: a model stops and freezes as a whole.  The model's loss sits in the
// first class's LM_LOSS slot (the others hold +0.0); every class carries its own penalty.
__device__ __forceinline__ void l1c_model_fin_body(const L1cFinArgs& a, int fit0, int classes) {
  MultiRec* rec = a.rec + fit0;
  const int32_t it = rec->iter;
  if (rec->stop) return;
  __shared__ double S[LM_COUNT + LN_COUNT];
  double tot[LM_COUNT + LN_COUNT];
#pragma unroll
  for (int q = 0; q < LM_COUNT + LN_COUNT; ++q) tot[q] = 0.0;
  for (int c = 0; c < classes; ++c) {
    multi_slot_totals(a.mpart, fit0 + c, LM_COUNT, a.nwg_m, S);
    multi_slot_totals(a.npart, fit0 + c, LN_COUNT, a.nwg_n, S, LM_COUNT);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LM_COUNT + LN_COUNT; ++q) tot[q] += S[q];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double* Sn = tot + LM_COUNT;
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const double sq = sqrt(static_cast<double>(a.m + a.n) * static_cast<double>(classes));
  const double pn = sqrt(tot[LM_R2] + Sn[LN_R2]);                                                                // admm.m:621
  const double pe = sq * a.abstol + a.reltol * fmax(sqrt(tot[LM_AX2] + Sn[LN_X2]), sqrt(tot[LM_Z2] + Sn[LN_Z2]));  // :644-650
  double dn = 0.0, de = 0.0;
  bool dual_ok = true;
  if (a.dual) {
    dn = a.rho * sqrt(Sn[LN_DZ2]);                               // admm.m:624
    de = sq * a.abstol + a.reltol * (a.rho * sqrt(Sn[LN_DU2]));  // admm.m:652-654
    dual_ok = dn < de;
  }
  const bool stop = !a.domaxiters && pn < pe && dual_ok;  // admm.m:710-713
  for (int c = 0; c < classes; ++c) {
    const int64_t h = static_cast<int64_t>(fit0 + c) * a.hist_ld + it;
    if (a.objevals) a.objv[h] = a.C * tot[LM_LOSS] + Sn[LN_PEN];
    a.pnorm[h] = pn;
    a.perr[h] = pe;
    if (a.dual) {
      a.dnorm[h] = dn;
      a.derr[h] = de;
    }
    multi_stop_tail(rec + c, stop, i1, a.maxiters);
  }
}

// Coefficient j of one fit, stored at e in the multi-vectors X, Z2, U2 and Y: z2 = kappa*penalty_elem(x + u2, tau*w_j),
// u2 += x - z2, the next right-hand side Y = D'(z1 - u1) + (z2 - u2) and the element's shares of the n-block's sums.
// g1, g2, g3 hold D'(z1 - u1), D'(z1 - z1prev) and D'u1 (the last two are read with the dual residual alone) and ge is the
// element's index in them: that addressing is all the two objects differ in.  INIT: only Y of the start vectors.
template <bool INIT>
__device__ __forceinline__ void l1c_elem_update(const PenaltyArgs& pen, const double* X, double* Z2, double* U2, double* Y,
                                                int64_t e, int64_t j, const double* __restrict__ g1,
                                                const double* __restrict__ g2, const double* __restrict__ g3, int64_t ge,
                                                int32_t dual, int32_t objevals, double (&acc)[LN_COUNT]) {
  const double zp = Z2[e], uo = U2[e];
  if constexpr (INIT) {
    Y[e] = g1[ge] + ((0.0 + zp) - uo);
  } else {
    const double xv = X[e];
    const double wi = penalty_weight(pen, j);
    const double zn = pen.kappa * penalty_elem(xv + uo, pen.tau * wi, pen.nonneg);
    const double rr = xv - zn;
    const double un = uo + rr;
    acc[LN_R2] += rr * rr;
    acc[LN_X2] += xv * xv;
    acc[LN_Z2] += zn * zn;
    if (dual) {
      const double dz = g2[ge] + (zn - zp);  // At(z - zprev) = D'(z1 - z1prev) + (z2 - z2prev)
      const double du = g3[ge] + un;         // At(u)
      acc[LN_DZ2] += dz * dz;
      acc[LN_DU2] += du * du;
    }
    if (objevals) acc[LN_PEN] += penalty_obj_elem(pen, wi, zn);
    Z2[e] = zn;
    U2[e] = un;
    Y[e] = g1[ge] + (zn - un);
  }
}
#endif

}  // namespace admm
