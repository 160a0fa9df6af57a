// covsel_device.h -- the one-workgroup eigen-step of covariance selection as an inline device function: X = f(M),
// M = rho*Y - S, by two-sided cyclic Jacobi on A = M and the basis V, both in LDS (the small path of covsel.hip).
// Called by covsel_small_kernel (covsel.hip: one fit, one launch per x-update) and by covsel_multi_kernel
// (covsel_multi.hip: one workgroup per fit, the whole iteration in the launch).  One eigen-step, defined once: the
// arithmetic and its order are the same for both callers.
#pragma once
#include "covsel.h"
#include "kernels.h"

namespace admm {

constexpr int kCovThreads = 512;  // 8 waves: two per SIMD
constexpr int kCovMaxSweeps = 40;
// (pair, row) items of one rotation phase per thread: ceil(48 * 96 / 512)
constexpr int kCovItems = static_cast<int>((kCovselSmallMax / 2 * kCovselSmallMax + kCovThreads - 1) / kCovThreads);
// entries of an n x n matrix per thread: ceil(96 * 96 / 512)
constexpr int kCovCells = static_cast<int>((kCovselSmallMax * kCovselSmallMax + kCovThreads - 1) / kCovThreads);

// f(l) = (l + sqrt(l^2 + 4 rho)) / (2 rho), in the form without cancellation for l < 0 (= 2 / (sqrt(l^2 + 4 rho) - l))
__device__ __forceinline__ double covsel_f(double l, double rho) {
  const double r = sqrt(l * l + 4.0 * rho);
  return l >= 0.0 ? (l + r) / (2.0 * rho) : 2.0 / (r - l);
}

// LDS carve (in doubles, every offset a multiple of 2: 16-byte aligned, guide G17): A, V [n x ld], rotations [np][2],
// f [n], reduction scratch [8], then int32 words: 2 rotation counters + 2 spare, pairs [np][2]
__host__ __device__ inline int64_t covsel_ld(int64_t n) { return n | 1; }
__host__ __device__ inline int64_t covsel_r2(int64_t v) { return (v + 1) & ~int64_t{1}; }
__host__ __device__ inline size_t covsel_small_lds(int64_t n) {
  const int64_t np = (n + 1) / 2;
  const int64_t dbl = 2 * covsel_r2(n * covsel_ld(n)) + 2 * np + covsel_r2(n) + 8;
  return static_cast<size_t>(dbl) * sizeof(double) + static_cast<size_t>(4 + 2 * np) * sizeof(int32_t);
}
// the reduction scratch of the carve (8 doubles: one per wave), for what a caller sums behind the eigen-step
__device__ __forceinline__ double* covsel_lds_red(double* lds, int n) {
  const int np = ((n + 1) & ~1) / 2;
  return lds + 2 * covsel_r2(int64_t{n} * covsel_ld(n)) + 2 * np + covsel_r2(n);
}

// Every thread of a workgroup of kCovThreads calls it with the same arguments; lds: covsel_small_lds(a.n) bytes, 16-byte
// aligned.  Reads a.y, a.S (lower triangles) and a.V; writes a.X (both halves), a.V, a.logpart[0] and adds the sweeps to
// a.sweeps[0].  Ends without a barrier: what another thread wrote to global memory is ordered by the caller's.
__device__ __forceinline__ void covsel_eigen_step(const CovselArgs& a, double* lds) {
  const int n = static_cast<int>(a.n);
  const int ld = static_cast<int>(covsel_ld(n));
  const int ne = (n + 1) & ~1, np = ne / 2;
  double* A = lds;                          // A(i, j) = A[i + j*ld]
  double* V = A + covsel_r2(int64_t{n} * ld);
  double* cs = V + covsel_r2(int64_t{n} * ld);
  double* fv = cs + 2 * np;
  double* red = fv + covsel_r2(n);
  int* cnt = reinterpret_cast<int*>(red + 8);
  int* pq = cnt + 4;
  const int tid = threadIdx.x;
  const double rho = a.rho;
  const double* __restrict__ Vg = a.V;
  const int64_t ldg = a.ldv;

  double fro = 0.0;
  for (int idx = tid; idx < n * n; idx += kCovThreads) {
    const int j = idx / n, i = idx - j * n;
    if (i < j) continue;
    const double m = rho * a.y[idx] - a.S[idx];
    A[i + j * ld] = m;
    A[j + i * ld] = m;
    fro += (i == j ? 1.0 : 2.0) * m * m;
  }
  fro = block_sum(fro, red);
  if (tid == 0) {
    red[0] = fro;  // (block_sum's last use of red was behind its own barrier)
    cnt[0] = 0;
    cnt[1] = 0;
  }
  __syncthreads();
  // rotations below this size change no eigenvalue by more than a thousandth of eps*||M||_F
  const double absfloor = 1e-3 * 2.220446049250313e-16 * sqrt(red[0]);
  const double tol = 2.220446049250313e-16;
  {  // warm start (V_prev = I at a run's first x-update)
    // T = M*V_prev into the V slot, then A = T'*V_prev (= V'MV, symmetric: the lower triangle, mirrored)
    for (int idx = tid; idx < n * n; idx += kCovThreads) {
      const int j = idx / n, i = idx - j * n;
      const double* __restrict__ vj = Vg + j * ldg;
      double t = 0.0;
      for (int k = 0; k < n; ++k) t = __builtin_fma(A[i + k * ld], vj[k], t);
      V[i + j * ld] = t;
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += kCovThreads) {
      const int j = idx / n, i = idx - j * n;
      if (i < j) continue;
      const double* __restrict__ vj = Vg + j * ldg;
      double t = 0.0;
      for (int k = 0; k < n; ++k) t = __builtin_fma(V[k + i * ld], vj[k], t);
      A[i + j * ld] = t;
      A[j + i * ld] = t;
    }
    __syncthreads();
    for (int idx = tid; idx < n * n; idx += kCovThreads) {
      const int j = idx / n, i = idx - j * n;
      V[i + j * ld] = Vg[i + j * ldg];
    }
  }
  __syncthreads();

  // this thread's (pair, row) items of the rotation phases: the same in every round
  int itk[kCovItems], iti[kCovItems];
  int nit = 0;
#pragma unroll
  for (int e = 0; e < kCovItems; ++e) {
    const int it = tid + e * kCovThreads;
    itk[e] = it / n;
    iti[e] = it - itk[e] * n;
    if (it < np * n) nit = e + 1;
  }
  int sweeps = kCovMaxSweeps;
  for (int sweep = 0; sweep < kCovMaxSweeps; ++sweep) {
    for (int r = 0; r < ne - 1; ++r) {
      if (tid < np) {
        int p, q;
        jacobi_pair(ne, r, tid, p, q);
        double c = 1.0, s = 0.0;
        if (q < n) {
          const double app = A[p + p * ld], aqq = A[q + q * ld], apq = A[p + q * ld];
          if (fabs(apq) > absfloor && fabs(apq) > tol * sqrt(fabs(app) * fabs(aqq))) {
            // symmetric Schur rotation (Golub & Van Loan 8.5.2): J'AJ has a zero at (p, q)
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = fabs(theta) > 1e150 ? 0.5 / theta
                                                 : copysign(1.0, theta) / (fabs(theta) + sqrt(1.0 + theta * theta));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
            atomicAdd(&cnt[sweep & 1], 1);
          }
        }
        cs[2 * tid] = c;
        cs[2 * tid + 1] = s;
        pq[2 * tid] = p;
        pq[2 * tid + 1] = q;
      }
      __syncthreads();
      // every thread has read the previous sweep's counter: clear the one the next sweep counts in
      if (r == 0 && tid == 0) cnt[(sweep + 1) & 1] = 0;
#pragma unroll
      for (int e = 0; e < kCovItems; ++e) {  // columns: A <- A*J, V <- V*J
        if (e >= nit) break;
        const int k = itk[e], i = iti[e];
        const double s = cs[2 * k + 1];
        if (s == 0.0) continue;
        const double c = cs[2 * k];
        const int p = pq[2 * k], q = pq[2 * k + 1];
        const double x = A[i + p * ld], w = A[i + q * ld];
        A[i + p * ld] = c * x - s * w;
        A[i + q * ld] = s * x + c * w;
        const double vx = V[i + p * ld], vw = V[i + q * ld];
        V[i + p * ld] = c * vx - s * vw;
        V[i + q * ld] = s * vx + c * vw;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < kCovItems; ++e) {  // rows: A <- J'*A, the pivot pair set to zero
        if (e >= nit) break;
        const int k = itk[e], j = iti[e];
        const double s = cs[2 * k + 1];
        if (s == 0.0) continue;
        const double c = cs[2 * k];
        const int p = pq[2 * k], q = pq[2 * k + 1];
        const double x = A[p + j * ld], w = A[q + j * ld];
        A[p + j * ld] = (j == q) ? 0.0 : c * x - s * w;
        A[q + j * ld] = (j == p) ? 0.0 : s * x + c * w;
      }
      __syncthreads();
    }
    if (cnt[sweep & 1] == 0) {
      sweeps = sweep + 1;
      break;
    }
  }

  double lsum = 0.0;
  for (int i = tid; i < n; i += kCovThreads) {
    const double f = covsel_f(A[i + i * ld], rho);
    fv[i] = f;
    lsum += log(f);
  }
  lsum = block_sum(lsum, red);
  if (tid == 0) {
    a.logpart[0] = -lsum;
    atomicAdd(a.sweeps, sweeps);
  }
  __syncthreads();
  // one Newton-Schulz step, V <- V (3I - V'V) / 2: the rotations leave V orthonormal only to their accumulated
  // rounding, and the next x-update warm-starts from this V, so without it the loss of orthogonality grows over a run
  // (DESIGN.md section 10).  G = V'V goes to the A slot (the eigenvalues are in fv).
  for (int idx = tid; idx < n * n; idx += kCovThreads) {
    const int j = idx / n, i = idx - j * n;
    if (i < j) continue;
    double g = 0.0;
    for (int k = 0; k < n; ++k) g = __builtin_fma(V[k + i * ld], V[k + j * ld], g);
    A[i + j * ld] = g;
    A[j + i * ld] = g;
  }
  __syncthreads();
  {
    double vn[kCovCells];
#pragma unroll
    for (int e = 0; e < kCovCells; ++e) {
      const int idx = tid + e * kCovThreads;
      if (idx >= n * n) break;
      const int j = idx / n, i = idx - j * n;
      double t = 0.0;
      for (int k = 0; k < n; ++k) t = __builtin_fma(V[i + k * ld], A[k + j * ld], t);
      vn[e] = 1.5 * V[i + j * ld] - 0.5 * t;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kCovCells; ++e) {
      const int idx = tid + e * kCovThreads;
      if (idx >= n * n) break;
      const int j = idx / n, i = idx - j * n;
      V[i + j * ld] = vn[e];
    }
  }
  __syncthreads();
  // X = V f(Lambda) V': the lower triangle, stored to both halves (exactly symmetric)
  for (int idx = tid; idx < n * n; idx += kCovThreads) {
    const int j = idx / n, i = idx - j * n;
    if (i < j) continue;
    double t = 0.0;
    for (int k = 0; k < n; ++k) t = __builtin_fma(V[i + k * ld] * fv[k], V[j + k * ld], t);
    a.X[i + static_cast<int64_t>(j) * n] = t;
    a.X[j + static_cast<int64_t>(i) * n] = t;
  }
  for (int idx = tid; idx < n * n; idx += kCovThreads) {
    const int j = idx / n, i = idx - j * n;
    a.V[i + j * ldg] = V[i + j * ld];
  }
}

}  // namespace admm
