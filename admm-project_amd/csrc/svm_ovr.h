// svm_ovr.h -- argument blocks of the one-vs-rest linear-SVM kernels (svm_ovr.hip): K independent unwrapped-ADMM runs
// (unwrappedadmm.m:76-92) over ONE matrix D.
#pragma once
#include "multi_device.h"

namespace admm {

constexpr int kOvrChunk = 10;      // classes one pass over D serves (registers and LDS of the pass)

// the sums a class's stop test and objective need (admm.m:621-658, 305-306; linearsvm.m:231-237)
enum OvrSlot : int32_t { OV_R2 = 0, OV_AX2 = 1, OV_Z2 = 2, OV_DZ2 = 3, OV_DU2 = 4, OV_OBJX = 5, OV_COUNT = 6 };

struct OvrPassArgs {
  const double* D;     // m x n, column-major
  int64_t ldD, m, n;
  const double* X;     // n x K (ldx): the iteration's x of every class
  int64_t ldx;
  double* Z;           // m x K (ldz)
  double* U;
  const double* ELL;   // m x K, +-1
  int64_t ldz;
  const int32_t* loss; // K values ADMM_LOSS_*
  double* gpart;       // [workgroups][K][ldx] partial rows of D'(z - u): the next x-update's right-hand side
  double* part;        // [K][OV_COUNT][kMultiMaxWg] block partials of the residual sums
  const MultiRec* rec;   // K
  int32_t K, c0;       // classes c0 .. c0 + kOvrChunk - 1 belong to this launch
  int32_t objevals;
  double rho, C;
};

struct OvrFinArgs {
  const double* gpart;  // as above
  double* gsum;         // K x ldx: the summed right-hand sides
  const double* part;
  const double* X;
  int64_t ldx, n, m;
  int32_t K, nwg;
  int32_t fin;          // 0: partial-row sums only (before the first iteration)
  MultiRec* rec;
  double *pnorm, *perr, *hnorm, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, C, abstol, reltol, Hnormtol;
  int32_t domaxiters, objevals, maxiters;
};

struct OvrSolveArgs {
  const double* M;      // symmetric n x n map (D'D)^-1 or (D'D)^+, full storage
  int64_t ldM, n;
  const double* gsum;
  double* X;
  int64_t ldx;
  const MultiRec* rec;
};

// the costs of a pass whose chunk takes the cost form of the element update
struct OvrCostArgs {
  const double* w;           // m weights shared by all classes, or null: every weight is 1
  const double* class_cost;  // K x 2: (cost_pos, cost_neg) of every class
};

int ovr_pass_workgroups(int64_t m);
// cost: null, or the chunk's costs (the COST instantiation of the pass)
void launch_ovr_pass(const OvrPassArgs& a, bool init, bool logistic, const OvrCostArgs* cost, hipStream_t stream);
void launch_ovr_gsum_fin(const OvrFinArgs& a, hipStream_t stream);
void launch_ovr_xsolve(const OvrSolveArgs& a, int32_t K, hipStream_t stream);
// X(:, c) = Xnew(:, c) for every class that has not stopped (the triangular-solve form of the x-update)
void launch_ovr_xcopy(const double* Xnew, double* X, int64_t ldx, int64_t n, int32_t K, const MultiRec* rec,
                      hipStream_t stream);

}  // namespace admm
