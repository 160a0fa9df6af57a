// multi_device.h -- what the "K runs over one D" solvers (svm_ovr.hip, reg_multi.hip, sparse_svm.hip, sparse_reg.hip)
// share on the device: the per-fit control record, the fixed-order sum of the pass's partial rows, the sum of a fit's
// block partials in front of its finalize arithmetic, and the tail that records the stop decision.  Every helper is
// forced inline and has the body the four files used to carry each on its own: one summation order, defined once.
#pragma once
#include <cstddef>

#include "common.h"

namespace admm {

constexpr int kMultiMaxWg = 256;  // workgroups of a pass or an elementwise launch (= block partials per fit): one per CU
constexpr int kMultiTile = 64;    // columns per workgroup of the partial-row sum / rows of the dense x-solve

// control record of ONE fit (an array of K of them; the single-run Ctrl block is not involved)
struct MultiRec {
  int32_t stop;   // this fit has met a stop condition or maxiters: frozen, every kernel skips it
  int32_t iter;   // completed iterations
  int32_t steps;  // results.steps (admm.m:746)
  int32_t early;  // a stop condition fired (admm.m:710-722), as opposed to maxiters running out
};
constexpr int32_t kMultiRecWords = sizeof(MultiRec) / sizeof(int32_t);  // SpmmMask stride
static_assert(offsetof(MultiRec, stop) == 0, "SpmmMask reads the stop word");

// Workgroup blockIdx.x of kBlock threads: gsum[fit][64 columns] = the sum over the nwg workgroups' partial rows
// gpart[workgroup][K][ldx].  Wave q takes rows q, q + 4, ... sixteen clamped loads at a time, and the four wave sums are
// added in wave order.
__device__ __forceinline__ void multi_gsum_tile(const double* gpart, double* gsum, int fit, int64_t ldx, int64_t n,
                                                int32_t K, int32_t nwg, double (*sq)[kMultiTile]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kMultiTile;
  const int64_t j = (j0 + lane < n) ? j0 + lane : n - 1;
  const double* __restrict__ G = gpart + static_cast<int64_t>(fit) * ldx + j;
  const int64_t rowstride = static_cast<int64_t>(K) * ldx;
  double s = 0.0;
  for (int32_t b0 = wid; b0 < nwg; b0 += 64) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int32_t b = (b0 + 4 * k < nwg) ? b0 + 4 * k : nwg - 1;
      v[k] = G[static_cast<int64_t>(b) * rowstride];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) s += (b0 + 4 * k < nwg) ? v[k] : 0.0;
  }
  sq[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && j0 + lane < n)
    gsum[static_cast<int64_t>(fit) * ldx + j0 + lane] = ((sq[0][lane] + sq[1][lane]) + sq[2][lane]) + sq[3][lane];
}

// S[slot0 + s] = the sum of the nb block partials part[(fit * count + s) * kMultiMaxWg + b] for s < count, in a
// workgroup of kBlock threads: the 32 lanes of slot (threadIdx.x >> 5) - slot0 add the partials sub, sub + 32, ... in that
// order, then a fixed shuffle tree.  The caller places the barrier before anything reads S.
// Two forms that add the same values in the same order.  The dense finalize keeps all eight loads of a lane in flight
// (clamped addresses); the sparse one strides, and takes a second source as a second call with its own slot0.
__device__ __forceinline__ void multi_slot_totals_unrolled(const double* part, int fit, int count, int nb, double* S) {
  const int slot = threadIdx.x >> 5, sub = threadIdx.x & 31;
  double v = 0.0;
  if (slot < count) {
    const double* __restrict__ ps = part + (static_cast<int64_t>(fit) * count + slot) * kMultiMaxWg;
    double wv[kMultiMaxWg / 32];
#pragma unroll
    for (int k = 0; k < kMultiMaxWg / 32; ++k) {
      const int b = sub + 32 * k;
      wv[k] = ps[b < nb ? b : nb - 1];
    }
#pragma unroll
    for (int k = 0; k < kMultiMaxWg / 32; ++k)
      if (sub + 32 * k < nb) v += wv[k];
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (sub == 0 && slot < 8) S[slot] = v;
}

__device__ __forceinline__ void multi_slot_totals(const double* part, int fit, int count, int nb, double* S,
                                                  int slot0 = 0) {
  const int slot = (threadIdx.x >> 5) - slot0, sub = threadIdx.x & 31;
  const bool mine = slot >= 0 && slot < count;
  double v = 0.0;
  if (mine) {
    const double* __restrict__ ps = part + (static_cast<int64_t>(fit) * count + slot) * kMultiMaxWg;
    for (int b = sub; b < nb; b += 32) v += ps[b];
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (sub == 0 && mine) S[slot0 + slot] = v;
}

// the end of every finalize: iteration i1 (1-based) of the fit is complete
__device__ __forceinline__ void multi_stop_tail(MultiRec* rec, bool stop, int i1, int32_t maxiters) {
  rec->iter = i1;
  rec->steps = i1;
  if (stop) rec->early = 1;
  if (stop || i1 >= maxiters) rec->stop = 1;
}

}  // namespace admm
