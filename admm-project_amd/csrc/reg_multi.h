// reg_multi.h -- argument blocks of the multi-fit robust-regression kernels (reg_multi.hip): K independent plain-ADMM
// runs of the A = D iteration (admm.m:496-743 with B = -1, c = s_k) over ONE matrix D.  The x-solve and the per-fit
// control record are svm_ovr.h's (ovr_xsolve_kernel, MultiRec).
#pragma once
#include "svm_ovr.h"

namespace admm {

constexpr int kRegmChunk = 10;  // fits one pass over D serves (registers and LDS of the pass)

// the sums a fit's stop test and objective need (admm.m:621, 644-650; lad.m:148 / huberfit.m:180)
enum RegmSlot : int32_t { RM_R2 = 0, RM_AX2 = 1, RM_Z2 = 2, RM_OBJ = 3, RM_COUNT = 4 };

struct RegmPassArgs {
  const double* D;      // m x n, column-major
  int64_t ldD, m, n;
  const double* X;      // n x K (ldx): the iteration's x of every fit
  int64_t ldx;
  double* Z;            // m x K (ldz)
  double* U;
  const double* S;      // m x ns (ldz): the responses
  int64_t ldz;
  const double* W;      // m weights shared by all fits, or null: every weight is 1
  const double* par;    // K x 4: (a, b, epsilon, delta) of every fit
  const int32_t* kind;  // K values: 0 LAD family, 1 Huber family
  double* gpart;        // [workgroups][K][ldx] partial rows of D'((s + z) - u): the next x-update's right-hand side
  double* part;         // [K][RM_COUNT][kMultiMaxWg] block partials of the residual sums
  const MultiRec* rec;    // K
  int32_t K, c0;        // fits c0 .. c0 + kRegmChunk - 1 belong to this launch
  int32_t ns;           // 1: every fit reads column 0 of S; K: fit k reads column k
  int32_t objevals;
  double rho;
};

struct RegmFinArgs {
  const double* gpart;  // as above
  double* gsum;         // K x ldx: the summed right-hand sides
  const double* part;
  const double* snorm;  // K: ||s_k||
  int64_t ldx, n, m;
  int32_t K, nwg;
  int32_t fin;          // 0: partial-row sums only (before the first iteration)
  MultiRec* rec;
  double *pnorm, *perr, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double abstol, reltol;
  int32_t domaxiters, objevals, maxiters;
};

void launch_regm_pass(const RegmPassArgs& a, bool init, hipStream_t stream);
void launch_regm_gsum_fin(const RegmFinArgs& a, hipStream_t stream);
// snorm[k] = ||s_k|| for every fit k < K (column 0 of S when ns == 1, column k otherwise), in a fixed order
void launch_regm_snorm(const double* S, int64_t ldz, int64_t m, int32_t K, int32_t ns, double* snorm, hipStream_t stream);

}  // namespace admm
