// spmm_cg.h -- the x-update of a multi-fit solver on a sparse design matrix: CG on
// (D'D + shift*I) x = y for K right-hand sides in lock-step over one sparse product with kSpmmChunk columns (spmm.h).  The
// kernels know nothing about the loss: sparse_svm.hip and sparse_reg.hip (shift = 0) and sparse_lasso.hip (shift = rho)
// drive them through SpmmCg.
// The shift never gets a pass of its own over Q: the three elementwise kernels that read Q form qv = Q + shift*V (V = P in
// an inner iteration, X in front of a warm start) through scg_qv, ONE explicit fma -- a single rounding whatever the
// compiler contracts around it, so the dot product and the update see the same bits of qv.  It is a template parameter:
// shift == 0 launches the SHIFT = false instantiations, which never read V for it and are the kernels as they were.
// Every multi-vector has spmm.h's layout [chunks][len][kSpmmChunk]; an elementwise kernel runs one thread per stored
// value: workgroup (b, chunk) of kScgRows * kSpmmChunk threads takes the row blocks b, b + gridDim.x, ... of its chunk,
// thread t the row t / kSpmmChunk of the block and the fit t % kSpmmChunk -- consecutive threads read consecutive
// addresses, and a thread's fit never changes.
#pragma once
#include <vector>

#include "multi_device.h"
#include "spmm.h"

namespace admm {

struct MultiHost;  // multi_host.h

constexpr int kScgRows = 32;                        // rows of a row block
constexpr int kScgBlock = kScgRows * kSpmmChunk;    // threads of an elementwise workgroup
constexpr int kScgWaves = kScgBlock / kWave;
constexpr int kScgMaxWg = kMultiMaxWg;              // workgroups per chunk of an elementwise launch (= partial sums per fit)
static_assert(kScgBlock % kWave == 0 && kScgBlock <= 1024, "whole waves, one workgroup");

// CG state of ONE fit (an array of K of them); it stays on the device
struct ScgState {
  double rs;        // r.r
  double ynorm;     // ||y||
  int32_t iters;    // inner iterations of the current solve
  int32_t done;     // converged, capped, or ended early: every CG kernel and product skips the fit
  int32_t brk;      // p.q == 0 met in this solve: the fit ends without the division
  int32_t zero;     // the right-hand side is zero: x = 0 exactly
  int64_t total;    // inner iterations since the run started
  int64_t capped;   // x-updates of this run that ended with the residual still above tol
};
constexpr int32_t kScgStateWords = sizeof(ScgState) / sizeof(int32_t);  // SpmmMask stride
constexpr int32_t kScgDoneWord = 5;                                     // index of `done` in 32-bit words
static_assert(offsetof(ScgState, done) == kScgDoneWord * sizeof(int32_t), "SpmmMask reads the done word");

struct ScgArgs {
  int64_t n;
  double tol;
  int32_t maxit, K;
  const double* Y;   // right-hand sides
  double* X;
  double* R;
  double* P;
  const double* Q;   // D'(D p), or D'(D x) in front of a warm start
  double* part;      // [chunks * kSpmmChunk][2][kScgMaxWg]: slot 0 p.q (and r.r of the start), slot 1 r.r (y.y of the start)
  ScgState* st;      // K
  const MultiRec* rec;  // K: a stopped fit is skipped
  int32_t* alldone;  // [0] the word the host polls: every fit is done or stopped; [1] the most inner iterations of a fit
  double shift;      // q = D'(D p) + shift*p; 0: no shift (the SHIFT = false kernels)
};

int scg_vec_workgroups(int64_t len);
// r = y - (q + shift*x) (first: x = 0, r = y), p = r, then per fit rs, ||y||, iters = 0, done if already converged
void launch_scg_start(const ScgArgs& a, bool first, hipStream_t stream);
// one inner iteration behind Q = D'(D P): p.qv with qv = q + shift*p, alpha, x and r, beta, p, the scalar state and the
// all-done word
void launch_scg_step(const ScgArgs& a, hipStream_t stream);

// what a sparse multi-fit solver owns for its x-update: D both ways, the n-length multi-vectors of CG, the m-length
// product buffer and the words the host polls.  The solver's own MultiHost lends stream, allocator, K and rec.
struct SpmmCg {
  MultiHost* h = nullptr;
  SparseDev sp;
  int64_t m = 0, n = 0;
  int32_t chunks = 0;
  double *X = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr, *Y = nullptr;  // len n
  double* T = nullptr;                                                         // len m: D p and D x
  double* cgpart = nullptr;
  ScgState* cg = nullptr;
  int32_t* alldone = nullptr;
  struct Poll {  // pinned
    int32_t alldone, longest;
  }* poll = nullptr;
  int cg_batch = 8;  // inner iterations enqueued between two polls of the all-done word
  // row weights of the forward product, one operator per fit (spmm.h): with `weighted` set, solve() stores
  // omega_k o (D V) into T for V = X in front of a warm start and V = P in an inner iteration, so that fit k solves
  // (D' Omega_k D + shift*I) x = y_k; the transposed product and the elementwise kernels are the same.  Unset: the
  // launches as they were.  The arrays belong to the solver.
  bool weighted = false;
  SpmmRowWeights roww;

  // the host's device and a stream of its own, D on the device, every buffer above zeroed (host->K is set)
  int build(MultiHost* host, int device, const admm_sparse_desc* D);
  void destroy();  // the whole teardown of the host: destroy_common, then D, the pinned word and the stream
  SpmmMask mask(bool with_cg) const;
  // column-major host matrix (rows x K), or zeros, into a chunked multi-vector, and back
  int upload(double* dst, const double* src, int64_t rows);
  int fetch_matrix(const double* src, int64_t rows, double* dst, size_t cap, size_t* written);
  // the CG state and x zeroed, the batch reset (a run never depends on the one before it), *a filled in
  int begin_run(double tol, int32_t maxit, ScgArgs* a, double shift = 0.0);
  // X <- the CG solution of (D'D + shift*I) x = Y for every running fit; the host polls the all-done word once per batch
  int solve(const ScgArgs& a, bool first);
  int fetch_counters(std::vector<ScgState>* out) const;
  template <class Summary>
  int fill_counters(Summary* summaries, int32_t K) const {  // the CG counters of the run that has just ended
    std::vector<ScgState> st;
    ADMM_TRY(fetch_counters(&st));
    for (int32_t c = 0; summaries && c < K; ++c) {
      summaries[c].cg_iters_total = st[c].total;
      summaries[c].cg_capped_updates = st[c].capped;
    }
    return ADMM_OK;
  }
};

#ifdef __HIPCC__
// what a thread of an elementwise kernel works on
struct ScgLane {
  int c, r, fit;
  bool run;  // the fit exists and its ADMM run has not stopped
};
__device__ __forceinline__ ScgLane scg_lane(const MultiRec* rec, int32_t K) {
  ScgLane l;
  l.c = threadIdx.x % kSpmmChunk;
  l.r = threadIdx.x / kSpmmChunk;
  l.fit = static_cast<int>(blockIdx.y) * kSpmmChunk + l.c;
  l.run = l.fit < K && rec[l.fit < K ? l.fit : K - 1].stop == 0;
  return l;
}

// per-fit sums over the workgroup of NS per-thread values, the rows of the block added in row order:
// part[(fit * nstot + slot0 + s) * kScgMaxWg + blockIdx.x].  lds: NS * kScgBlock doubles.
template <int NS>
__device__ __forceinline__ void scg_sums(const double (&acc)[NS], double* lds, double* part, int nstot, int slot0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int s = 0; s < NS; ++s) lds[s * kScgBlock + tid] = acc[s];
  __syncthreads();
  if (tid < NS * kSpmmChunk) {
    const int s = tid / kSpmmChunk, c = tid % kSpmmChunk;
    double v = 0.0;
    for (int r = 0; r < kScgRows; ++r) v += lds[s * kScgBlock + r * kSpmmChunk + c];
    const int64_t fit = static_cast<int64_t>(blockIdx.y) * kSpmmChunk + c;
    part[(fit * nstot + slot0 + s) * kScgMaxWg + blockIdx.x] = v;
  }
}
#endif

}  // namespace admm
