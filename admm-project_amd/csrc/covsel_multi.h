// covsel_multi.h -- covariance selection, K fits over one S (covsel_multi.hip): the argument block of
// the one kernel that carries a fit's whole ADMM iteration, one workgroup per fit.
#pragma once
#include "covsel.h"
#include "multi_device.h"

namespace admm {

struct CovselMultiArgs {
  int64_t n;          // <= kCovselSmallMax
  int32_t K;          // the grid: workgroup k owns fit k
  int32_t iters;      // iterations of every running fit in this launch, at most
  const double* S;    // n x n, ld n, shared by all fits
  const double* lam;  // [K]
  const double* rho;  // [K]
  // per fit contiguous, n x n column-major with leading dimension n: fit k at k * n * n
  double *X, *Z, *U, *Y, *V;  // Y = Z - U, the right-hand side of the next eigen-step; V its warm start (I at iteration 0)
  double* logpart;    // [K]: -log det X of the fit's last eigen-step
  int32_t* sweeps;    // [K]: += the Jacobi sweeps of the fit
  MultiRec* rec;
  double *pnorm, *perr, *dnorm, *derr, *objv;  // histories [K][hist_ld]
  int32_t hist_ld;
  int32_t maxiters;
  double abstol, reltol;
  int32_t domaxiters, objevals, dual;
};
// once per device before the first launch: allow the dynamic LDS the largest n needs
int covsel_multi_prepare();
// K workgroups of 512 threads; no host synchronisation.  A fit whose record says stop is not touched.
void launch_covsel_multi(const CovselMultiArgs& a, hipStream_t stream);

}  // namespace admm
