// sparse_svm.h -- argument blocks of the one-vs-rest linear SVM on a sparse design matrix (sparse_svm.hip, DESIGN.md
// q37): K independent unwrapped-ADMM runs (unwrappedadmm.m:76-92) whose x-update D^+(z - u) is CG on D'D x = D'(z - u),
// all classes in lock-step over one sparse product with kSpmmChunk right-hand sides (spmm.h).
// Every multi-vector has spmm.h's layout [chunks][len][kSpmmChunk]; an elementwise kernel runs one thread per stored
// value: workgroup (b, chunk) of kSsvRows * kSpmmChunk threads takes the row blocks b, b + gridDim.x, ... of its chunk,
// thread t the row t / kSpmmChunk of the block and the class t % kSpmmChunk -- consecutive threads read consecutive
// addresses, and a thread's class never changes.
#pragma once
#include "spmm.h"
#include "svm_ovr.h"

namespace admm {

constexpr int kSsvRows = 32;                        // rows of a row block
constexpr int kSsvBlock = kSsvRows * kSpmmChunk;    // threads of an elementwise workgroup
constexpr int kSsvWaves = kSsvBlock / kWave;
constexpr int kSsvMaxWg = kOvrMaxWg;                // workgroups per chunk of an elementwise launch (= partial sums per class)
static_assert(kSsvBlock % kWave == 0 && kSsvBlock <= 1024, "whole waves, one workgroup");

// CG state of ONE class (an array of K of them); it stays on the device
struct SsvCg {
  double rs;        // r.r
  double ynorm;     // ||y||
  int32_t iters;    // inner iterations of the current solve
  int32_t done;     // converged, capped, or ended early: every CG kernel and product skips the class
  int32_t brk;      // p.q == 0 met in this solve: the class ends without the division
  int32_t zero;     // the right-hand side is zero: x = 0 exactly
  int64_t total;    // inner iterations since the run started
  int64_t capped;   // x-updates of this run that ended with the residual still above tol
};
constexpr int32_t kSsvCgWords = sizeof(SsvCg) / sizeof(int32_t);  // SpmmMask stride
constexpr int32_t kSsvDoneWord = 5;                              // index of `done` in 32-bit words
constexpr int32_t kOvrRecWords = sizeof(OvrRec) / sizeof(int32_t);

struct SsvCgArgs {
  int64_t n;
  double tol;
  int32_t maxit, K;
  const double* Y;   // right-hand sides D'(z - u)
  double* X;
  double* R;
  double* P;
  const double* Q;   // D'(D p), or D'(D x) in front of a warm start
  double* part;      // [chunks * kSpmmChunk][2][kSsvMaxWg]: slot 0 p.q (and r.r of the start), slot 1 r.r (y.y of the start)
  SsvCg* st;         // K
  const OvrRec* rec; // K: a stopped class is skipped
  int32_t* alldone;  // [0] the word the host polls: every class is done or stopped; [1] the most inner iterations of a class
};

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
  const OvrRec* rec;
  double* part;       // [chunks * kSpmmChunk][OV_COUNT][kSsvMaxWg]
  int32_t K, objevals;
  double rho, C;
};

struct SsvFinArgs {
  const double* part;
  const double* X;
  int64_t n, m;
  int32_t K, nwg;
  OvrRec* rec;
  double *pnorm, *perr, *hnorm, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, C, abstol, reltol, Hnormtol;
  int32_t domaxiters, objevals, maxiters;
};

int ssv_vec_workgroups(int64_t len);
// r = y - q (first: x = 0, r = y), p = r, then per class rs, ||y||, iters = 0, done if already converged
void launch_ssv_cg_start(const SsvCgArgs& a, bool first, hipStream_t stream);
// one inner iteration behind Q = D'(D P): p.q, alpha, x and r, beta, p, the scalar state and the all-done word
void launch_ssv_cg_step(const SsvCgArgs& a, hipStream_t stream);
// init: V = z0 - u0 only
void launch_ssv_elem(const SsvElemArgs& a, bool init, hipStream_t stream);
void launch_ssv_fin(const SsvFinArgs& a, hipStream_t stream);

}  // namespace admm
