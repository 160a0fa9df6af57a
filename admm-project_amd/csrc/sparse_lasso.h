// sparse_lasso.h -- argument blocks of the multi-fit lasso on a sparse design matrix (sparse_lasso.hip): K
// independent plain-ADMM runs of the A = 1 iteration (lasso.m:227-239: B = -1, c = 0, sizes n, stopcond 'standard') that
// share D and rho and differ in (lambda_k, mu_k, nonneg_k) and optionally in their column of S.  The x-update
// (D'D + rho*I) x = D's_k + rho*(z - u) (lasso.m:28-30) is the lock-step CG of spmm_cg.h with the shift rho.  Every
// multi-vector has spmm.h's layout [chunks][len][kSpmmChunk] and every elementwise kernel spmm_cg.h's thread layout.
#pragma once
#include "spmm_cg.h"

namespace admm {

// the sums of the element pass over n (admm.m:621-654 with A = 1, B = -1, c = 0) and g_k(z) without the indicator
enum SlmSlot : int32_t { SL_R2 = 0, SL_X2 = 1, SL_Z2 = 2, SL_DZ2 = 3, SL_U2 = 4, SL_OBJ = 5, SL_COUNT = 6 };

struct SlmElemArgs {
  int64_t n;
  const double* X;        // the x-update's solution
  double* Z;
  double* U;
  double* Y;              // the next right-hand side rho*(z - u) + D's
  const double* DTS;      // D's: dts_ns == 1 column 0 of ONE chunk, shared by all fits; otherwise a multi-vector
  const double* W;        // n shared l1 weights or null
  const double* par;      // K x 2: (lambda, mu) of every fit
  const int32_t* nonneg;  // K values 0 | 1
  const MultiRec* rec;
  double* part;           // [chunks * kSpmmChunk][SL_COUNT][kScgMaxWg]
  int32_t K, ns, objevals;
  double rho;
  int32_t dts_ns;         // how DTS is indexed: ns, or K under observations (D'(Omega_k s_k) differs per fit even when S
                          // is shared: DESIGN.md q46)
};

struct SlmFitArgs {
  int64_t m;
  const double* T;        // D x
  const double* S;        // ns == 1 column 0 of ONE chunk; ns == K a multi-vector of len m
  const MultiRec* rec;
  double* part;           // [chunks * kSpmmChunk][1][kScgMaxWg]: sum (D x - s_k)^2
  int32_t K, ns;
  // the weighted form (observations set, q46): part is [chunks * kSpmmChunk][SLW_COUNT][kScgMaxWg]
  const double* obsw;     // m observation weights or null (1)
  const int32_t* fold;    // m fold ids or null (no row is held out)
  const int32_t* held;    // K values: the fold fit k holds out, or -1
  int32_t all;            // every fit, stopped or not (the pass behind the loop); 0: the running fits
};

// the sums of the weighted fit pass over m: the fit term sum omega_ik (t - s)^2, the held-out error
// sum obsw_i [fold_i = held_k] (t - s)^2 and the held-out weight sum obsw_i [fold_i = held_k]
enum SlmFitSlot : int32_t { SLW_FIT = 0, SLW_HELD_SSE = 1, SLW_HELD_W = 2, SLW_COUNT = 3 };

// T(:, k) = omega_k o s_k over m, for the right-hand side D'(Omega_k s_k) (S and ns as SlmFitArgs)
struct SlmObsRhsArgs {
  int64_t m;
  const double* S;
  double* T;
  const double* obsw;
  const int32_t* fold;
  const int32_t* held;
  int32_t K, ns;
};

struct SlmFinArgs {
  const double* part;     // the element pass's partials, nwg_n per slot
  const double* fpart;    // the fit pass's partials, nwg_m (objevals != 0): fit_slots per fit, the fit term in slot 0
  int64_t n;
  int32_t K, nwg_n, nwg_m;
  int32_t dual;           // the dual residual takes part in the stop rule (nodualerror = 0)
  MultiRec* rec;
  double *pnorm, *perr, *dnorm, *derr, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, abstol, reltol;
  int32_t domaxiters, objevals, maxiters;
  int32_t fit_slots;      // 1, or SLW_COUNT when the weighted fit pass wrote fpart
};

// init: Y = rho*(z0 - u0) + D's only
void launch_slm_elem(const SlmElemArgs& a, bool init, hipStream_t stream);
void launch_slm_fit(const SlmFitArgs& a, hipStream_t stream);
void launch_slm_fit_weighted(const SlmFitArgs& a, hipStream_t stream);
void launch_slm_obs_rhs(const SlmObsRhsArgs& a, hipStream_t stream);
// heldout[2k], heldout[2k + 1] = the totals of slots SLW_HELD_SSE and SLW_HELD_W of fit k (multi_slot_totals' order)
void launch_slm_heldout(const double* part, int32_t K, int32_t nwg_m, double* heldout, hipStream_t stream);
void launch_slm_fin(const SlmFinArgs& a, hipStream_t stream);

}  // namespace admm
