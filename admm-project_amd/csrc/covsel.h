// covsel.h -- the x-update of covariance selection (covsel.hip): X = f(M), M = rho*(Z - U) - S, with
// f(l) = (l + sqrt(l^2 + 4*rho)) / (2*rho) applied to the eigenvalues of M (getProxOps.m:1487-1495).
#pragma once
#include "common.h"

namespace admm {

// the one-workgroup path keeps M and its eigenvector basis in LDS (2 * n * (n | 1) doubles: 149 KiB at n = 96 of the
// 160 KiB a workgroup may use); larger n take the one-sided Jacobi rounds of jacobi.hip, one launch per round
constexpr int64_t kCovselSmallMax = 96;

struct CovselArgs {
  int64_t n;
  double rho;
  const double* y;   // Z - U (or v - uhat), n x n column-major, ld n: the right-hand side the prox kernel wrote
  const double* S;   // n x n, ld n; only the lower triangle enters M (symmetric-eig semantics, q26)
  double* X;         // out: n x n, ld n, exactly symmetric
  double* V;         // eigenvector basis of the previous x-update (in: M is rotated into it first) and of this one (out)
  int64_t ldv;
  double* logpart;   // out: [0] = -sum_i log f(lambda_i) = -log det X (objective term)
  int32_t* sweeps;   // += sweeps this x-update took
};
// one launch, no host synchronisation; a no-op once ctrl->stop is set
void launch_covsel_small(const CovselArgs& a, const Ctrl* ctrl, hipStream_t stream);
// once per device before the first launch: allow the dynamic LDS the largest small-path n needs
int covsel_small_prepare();

// large path buffers: all n x n with leading dimension ld (padding rows zero)
struct CovselLarge {
  int64_t n = 0, ld = 0;
  double *W = nullptr, *B = nullptr, *V = nullptr, *T = nullptr;
  double *lam = nullptr, *sig = nullptr;  // [2n]: column norms, sqrt(f); [1 + 2n]: the shift, Gershgorin bounds
  int32_t* rot = nullptr;
};
// X = f(M) through W = M + sigma*I (sigma from Gershgorin discs: W positive definite), B0 = W*V_prev, one-sided
// Jacobi rounds on (B, V) until a sweep rotates nothing (one host check per sweep); lambda_i = ||b_i|| / ||v_i|| - sigma,
// then one Newton-Schulz step re-orthonormalises V before X is formed and V is kept for the next warm start.
// ctrl_host receives the device control block at every check: a run that has stopped skips the rest.
int covsel_large_x_update(const CovselLarge& c, double rho, const double* y, const double* S, double* X,
                          double* logpart, const Ctrl* ctrl, Ctrl* ctrl_host, int* sweeps, hipStream_t stream);

// S = cov(D) (covarianceselection.m:150, MATLAB cov): centre each column of the m x n samples (in place, ld ldD),
// then the MFMA Gram D'D / (m - 1) into S (n x n, ld n, exactly symmetric).  W: ld_w x n scratch.
void covsel_cov(double* D, int64_t ldD, int64_t m, int64_t n, double* W, int64_t ldw, double* S, hipStream_t stream);

}  // namespace admm
