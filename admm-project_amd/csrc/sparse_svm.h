// sparse_svm.h -- argument blocks of the one-vs-rest linear SVM on a sparse design matrix (sparse_svm.hip, DESIGN.md
// q37): K independent unwrapped-ADMM runs (unwrappedadmm.m:76-92) whose x-update D^+(z - u) is the lock-step CG of
// spmm_cg.h on D'D x = D'(z - u).  Every multi-vector has spmm.h's layout [chunks][len][kSpmmChunk] and every
// elementwise kernel spmm_cg.h's thread layout; the residual slots are svm_ovr.h's.
#pragma once
#include "spmm_cg.h"
#include "svm_ovr.h"

namespace admm {

struct SsvElemArgs {
  int64_t m;
  const double* AX;   // D x
  double* Z;
  double* U;
  const double* ELL;
  double* V;          // z - u: the next right-hand side in front of D'
  const double* W;    // m shared weights or null
  const double* CC;   // K x 2 class costs
  const int32_t* loss;        // K
  const int32_t* chunk_cost;  // per chunk: the cost form of the element update (svm_ovr.hip's rule)
  const MultiRec* rec;
  double* part;       // [chunks * kSpmmChunk][OV_COUNT][kScgMaxWg]
  int32_t K, objevals;
  double rho, C;
};

struct SsvFinArgs {
  const double* part;
  const double* X;
  int64_t n, m;
  int32_t K, nwg;
  MultiRec* rec;
  double *pnorm, *perr, *hnorm, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, C, abstol, reltol, Hnormtol;
  int32_t domaxiters, objevals, maxiters;
};

// init: V = z0 - u0 only
void launch_ssv_elem(const SsvElemArgs& a, bool init, hipStream_t stream);
void launch_ssv_fin(const SsvFinArgs& a, hipStream_t stream);

}  // namespace admm
