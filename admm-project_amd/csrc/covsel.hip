// covsel.hip -- covariance selection (sparse inverse covariance): the x-update of getProxOps.m:1487-1495
//   [Q, E] = eig(rho*(z - u) - S);  x = Q*diag((e + sqrt(e.^2 + 4*rho))./(2*rho))*Q'
// evaluated as the matrix function X = f(M) of the symmetric, indefinite M = rho*(Z - U) - S.  f is increasing and
// 1/rho-Lipschitz, so X is well defined (and stable) where eigenvalues repeat and Q is ambiguous: nothing here depends
// on which eigenvectors come out, only on the subspaces.  X is stored exactly symmetric (q26).
//
// Two paths, chosen from n alone (kCovselSmallMax):
//  - small: ONE workgroup runs two-sided cyclic Jacobi (round-robin parallel order: n/2 disjoint rotations per round)
//    on A = M and the basis V, both in LDS, warm-started from the previous x-update's basis (A = V'MV is nearly
//    diagonal when Z and U move slowly), then writes X = V f(Lambda) V' and -log det X.  One launch per x-update.
//  - large: one-sided (Hestenes) Jacobi of jacobi.hip on W = M + sigma*I, positive definite by a Gershgorin bound,
//    warm-started by B0 = W*V_prev (MFMA GEMM); lambda_i = ||b_i|| - sigma, X = (V F^1/2)(V F^1/2)' by the GEMM.
#include <algorithm>
#include <cmath>

#include "covsel_device.h"
#include "kernels.h"

namespace admm {

// M(i, j) from the lower triangle of rho*y - S
__device__ __forceinline__ double covsel_m(const double* __restrict__ y, const double* __restrict__ S, int64_t n,
                                           double rho, int64_t i, int64_t j) {
  const int64_t k = (i >= j) ? i + j * n : j + i * n;
  return rho * y[k] - S[k];
}

// one fit: the eigen-step of covsel_device.h in a launch of its own
__global__ __launch_bounds__(kCovThreads) void covsel_small_kernel(CovselArgs a, const Ctrl* __restrict__ ctrl) {
  if (ctrl->stop) return;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  covsel_eigen_step(a, lds);
}

int covsel_small_prepare() {
  ADMM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(covsel_small_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(covsel_small_lds(kCovselSmallMax))));
  return ADMM_OK;
}

void launch_covsel_small(const CovselArgs& a, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(covsel_small_kernel, dim3(1), dim3(kCovThreads), covsel_small_lds(a.n), stream, a, ctrl);
}

// ------------------------------------------------------------------------------------------------ large path
// column j of W = M (lower triangle mirrored) and its Gershgorin disc: bounds[j] = M_jj - r_j, bounds[n + j] = |M_jj| + r_j
__global__ __launch_bounds__(kBlock) void covsel_gershgorin_kernel(const double* __restrict__ y,
                                                                   const double* __restrict__ S, int64_t n, double rho,
                                                                   double* __restrict__ W, int64_t ldw,
                                                                   double* __restrict__ bounds) {
  __shared__ double scratch[kBlock / kWave];
  const int64_t j = blockIdx.x;
  double diag = 0.0, rad = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {
    const double m = covsel_m(y, S, n, rho, i, j);
    W[i + j * ldw] = m;
    if (i == j) diag = m;
    else rad += fabs(m);
  }
  diag = block_sum(diag, scratch);
  rad = block_sum(rad, scratch);
  if (threadIdx.x == 0) {
    bounds[j] = diag - rad;
    bounds[n + j] = fabs(diag) + rad;
  }
}

// sigma = max(0, -min_j lo_j) + 1e-3 * max_j hi_j (so lambda_min(W) >= 1e-3*||M||-ish > 0); W += sigma*I
__global__ __launch_bounds__(kBlock) void covsel_shift_kernel(double* __restrict__ W, int64_t ldw, int64_t n,
                                                              double* __restrict__ sig) {
  __shared__ double slo[kBlock], shi[kBlock];
  double lo = INFINITY, hi = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kBlock) {
    lo = fmin(lo, sig[1 + j]);
    hi = fmax(hi, sig[1 + n + j]);
  }
  slo[threadIdx.x] = lo;
  shi[threadIdx.x] = hi;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      slo[threadIdx.x] = fmin(slo[threadIdx.x], slo[threadIdx.x + w]);
      shi[threadIdx.x] = fmax(shi[threadIdx.x], shi[threadIdx.x + w]);
    }
    __syncthreads();
  }
  double s = fmax(0.0, -slo[0]) + 1e-3 * shi[0];
  if (!(s > 0.0)) s = 1.0;  // M = 0
  for (int64_t j = threadIdx.x; j < n; j += kBlock) W[j + j * ldw] += s;
  if (threadIdx.x == 0) sig[0] = s;
}

// lambda_i = ||b_i|| / ||v_i|| - sigma (b_i = W v_i; G = V'V before the Newton-Schulz step, so G_ii = ||v_i||^2)
// -> scale[i] = sqrt(f(lambda_i)); logpart[0] = -sum log f(lambda_i)
__global__ __launch_bounds__(kBlock) void covsel_spectrum_kernel(const double* __restrict__ norms,
                                                                 const double* __restrict__ G, int64_t ldg,
                                                                 const double* __restrict__ sig, int64_t n, double rho,
                                                                 double* __restrict__ scale,
                                                                 double* __restrict__ logpart) {
  __shared__ double scratch[kBlock / kWave];
  const double s = sig[0];
  double lsum = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {
    const double f = covsel_f(norms[i] / sqrt(G[i + i * ldg]) - s, rho);
    scale[i] = sqrt(f);
    lsum += log(f);
  }
  lsum = block_sum(lsum, scratch);
  if (threadIdx.x == 0) logpart[0] = -lsum;
}

// T(:, j) = V(:, j) * scale[j]
__global__ __launch_bounds__(kBlock) void covsel_scale_copy_kernel(const double* __restrict__ V,
                                                                   double* __restrict__ T, int64_t ld, int64_t n,
                                                                   const double* __restrict__ scale) {
  const int64_t j = blockIdx.x;
  const double s = scale[j];
  for (int64_t i = threadIdx.x; i < n; i += kBlock) T[i + j * ld] = V[i + j * ld] * s;
}

// V <- 1.5 V - 0.5 T, T = V*(V'V): one Newton-Schulz step towards the nearest orthonormal basis
__global__ __launch_bounds__(kBlock) void covsel_ns_kernel(double* __restrict__ V, const double* __restrict__ T,
                                                           int64_t ld, int64_t n) {
  const int64_t j = blockIdx.x;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) V[i + j * ld] = 1.5 * V[i + j * ld] - 0.5 * T[i + j * ld];
}

// dst (n x n, ld n) = the lower triangle of src (ld) mirrored: exactly symmetric.  ctrl (nullable): no-op once stopped
__global__ __launch_bounds__(kBlock) void covsel_mirror_kernel(const double* __restrict__ src, int64_t ld, int64_t n,
                                                               double scale, double* __restrict__ dst,
                                                               const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int64_t j = blockIdx.x;
  for (int64_t i = threadIdx.x; i < n; i += kBlock)
    dst[i + j * n] = scale * ((i >= j) ? src[i + j * ld] : src[j + i * ld]);
}

int covsel_large_x_update(const CovselLarge& c, double rho, const double* y, const double* S, double* X,
                          double* logpart, const Ctrl* ctrl, Ctrl* ctrl_host, int* sweeps, hipStream_t stream) {
  const int64_t n = c.n, ld = c.ld;
  const unsigned gn = static_cast<unsigned>(n);
  hipLaunchKernelGGL(covsel_gershgorin_kernel, dim3(gn), dim3(kBlock), 0, stream, y, S, n, rho, c.W, ld, c.sig + 1);
  hipLaunchKernelGGL(covsel_shift_kernel, dim3(1), dim3(kBlock), 0, stream, c.W, ld, n, c.sig);
  launch_gemm(0, 0, n, n, n, 1.0, c.W, ld, c.V, ld, 0.0, c.B, ld, false, stream);  // B0 = W*V_prev, V0 = V_prev
  // orthogonality threshold of jacobi_eig_psd; no null-space cut-off (W is positive definite)
  const double tol = std::max(1e-15, std::sqrt(static_cast<double>(n)) * 2.220446049250313e-16);
  const int32_t ne = static_cast<int32_t>((n + 1) & ~int64_t{1});
  int done = 0;
  for (int sweep = 0; sweep < kCovMaxSweeps; ++sweep) {
    ADMM_HIP_TRY(hipMemsetAsync(c.rot, 0, sizeof(int32_t), stream));
    for (int32_t r = 0; r < ne - 1; ++r) launch_jacobi_round(c.B, ld, c.V, ld, n, r, tol, 0.0, c.rot, stream);
    int32_t nrot = 0;
    ADMM_HIP_TRY(hipMemcpyAsync(&nrot, c.rot, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    ADMM_HIP_TRY(hipMemcpyAsync(ctrl_host, ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, stream));
    ADMM_HIP_TRY(hipStreamSynchronize(stream));
    ++done;
    if (ctrl_host->stop) break;  // the run has stopped: this x-update is discarded anyway
    if (nrot == 0) break;
  }
  *sweeps += done;
  if (ctrl_host->stop) return ADMM_OK;
  launch_jacobi_norms(c.B, ld, n, c.lam, stream);
  // one Newton-Schulz step on V (W is free until X): G = V'V, T = V*G, V <- 1.5 V - 0.5 T.  The rotations leave V
  // orthonormal only to their accumulated rounding, and the next x-update warm-starts from it
  launch_gemm(1, 0, n, n, n, 1.0, c.V, ld, c.V, ld, 0.0, c.W, ld, false, stream);
  launch_gemm(0, 0, n, n, n, 1.0, c.V, ld, c.W, ld, 0.0, c.T, ld, false, stream);
  hipLaunchKernelGGL(covsel_ns_kernel, dim3(gn), dim3(kBlock), 0, stream, c.V, c.T, ld, n);
  hipLaunchKernelGGL(covsel_spectrum_kernel, dim3(1), dim3(kBlock), 0, stream, c.lam, c.W, ld, c.sig, n, rho,
                     c.lam + n, logpart);
  hipLaunchKernelGGL(covsel_scale_copy_kernel, dim3(gn), dim3(kBlock), 0, stream, c.V, c.T, ld, n, c.lam + n);
  launch_gemm(0, 1, n, n, n, 1.0, c.T, ld, c.T, ld, 0.0, c.W, ld, true, stream);  // X = T*T' (lower tiles)
  hipLaunchKernelGGL(covsel_mirror_kernel, dim3(gn), dim3(kBlock), 0, stream, c.W, ld, n, 1.0, X, ctrl);
  return ADMM_OK;
}

// ------------------------------------------------------------------------------------------------ cov(D)
// column j of D minus its mean (MATLAB cov centres first: covarianceselection.m:150)
__global__ __launch_bounds__(kBlock) void covsel_center_kernel(double* __restrict__ D, int64_t ldD, int64_t m) {
  __shared__ double scratch[kBlock / kWave];
  __shared__ double smean;
  double* __restrict__ col = D + static_cast<int64_t>(blockIdx.x) * ldD;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kBlock) s += col[i];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) smean = s / static_cast<double>(m);
  __syncthreads();
  const double mu = smean;
  for (int64_t i = threadIdx.x; i < m; i += kBlock) col[i] -= mu;
}

void covsel_cov(double* D, int64_t ldD, int64_t m, int64_t n, double* W, int64_t ldw, double* S, hipStream_t stream) {
  hipLaunchKernelGGL(covsel_center_kernel, dim3(static_cast<unsigned>(n)), dim3(kBlock), 0, stream, D, ldD, m);
  launch_gemm(1, 0, n, n, m, 1.0, D, ldD, D, ldD, 0.0, W, ldw, true, stream);
  hipLaunchKernelGGL(covsel_mirror_kernel, dim3(static_cast<unsigned>(n)), dim3(kBlock), 0, stream, W, ldw, n,
                     1.0 / static_cast<double>(m - 1), S, nullptr);
}

}  // namespace admm
