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
  const double* DTS;      // D's: ns == 1 column 0 of ONE chunk, shared by all fits; ns == K a multi-vector
  const double* W;        // n shared l1 weights or null
  const double* par;      // K x 2: (lambda, mu) of every fit
  const int32_t* nonneg;  // K values 0 | 1
  const MultiRec* rec;
  double* part;           // [chunks * kSpmmChunk][SL_COUNT][kScgMaxWg]
  int32_t K, ns, objevals;
  double rho;
};

struct SlmFitArgs {
  int64_t m;
  const double* T;        // D x
  const double* S;        // ns == 1 column 0 of ONE chunk; ns == K a multi-vector of len m
  const MultiRec* rec;
  double* part;           // [chunks * kSpmmChunk][1][kScgMaxWg]: sum (D x - s_k)^2
  int32_t K, ns;
};

struct SlmFinArgs {
  const double* part;     // the element pass's partials, nwg_n per slot
  const double* fpart;    // the fit pass's partials, nwg_m (objevals != 0)
  int64_t n;
  int32_t K, nwg_n, nwg_m;
  int32_t dual;           // the dual residual takes part in the stop rule (nodualerror = 0)
  MultiRec* rec;
  double *pnorm, *perr, *dnorm, *derr, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, abstol, reltol;
  int32_t domaxiters, objevals, maxiters;
};

// init: Y = rho*(z0 - u0) + D's only
void launch_slm_elem(const SlmElemArgs& a, bool init, hipStream_t stream);
void launch_slm_fit(const SlmFitArgs& a, hipStream_t stream);
void launch_slm_fin(const SlmFinArgs& a, hipStream_t stream);

}  // namespace admm
