// slot_reduce.h -- the block reduction of the S_COUNT residual slots every element-update kernel ends with, and the
// fixed-order fold of partial rows behind the x-solves and the transposed GEMV.
#pragma once
#include "loop_kernels.h"

namespace admm {

// wave sums of the thread accumulators into sred[wave][slot] (lane 0 of each wave stores).  The caller owns the LDS
// array, decides which waves take part, and places the barrier before anything reads the sums.
__device__ __forceinline__ void slot_wave_sums(const double (&acc)[S_COUNT], double (*sred)[S_COUNT]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < S_COUNT; ++s) {
    const double w = wave_sum(acc[s]);
    if (lane == 0) sred[wid][s] = w;
  }
}

// total of slot s over WAVES waves, added in wave order (the order every partial sum of the loop is defined by)
template <int WAVES>
__device__ __forceinline__ double slot_total(const double (*sred)[S_COUNT], int s) {
  double tot = sred[0][s];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) tot += sred[w][s];
  return tot;
}

// the whole reduction of a workgroup of WAVES waves: thread s < S_COUNT stores part[s * stride + block]
template <int WAVES>
__device__ __forceinline__ void block_reduce_slots(const double (&acc)[S_COUNT], double (*sred)[S_COUNT], double* part,
                                                   int64_t stride, unsigned block) {
  slot_wave_sums(acc, sred);
  __syncthreads();
  const int s = threadIdx.x;
  if (s < S_COUNT) part[s * stride + block] = slot_total<WAVES>(sred, s);
}

// The fold of partial ROWS (symv.hip, trsv.hip, gemv.hip): a workgroup of kBlock threads = 16 consecutive elements
// (threadIdx & 15) x 16 slots (threadIdx >> 4) that split the partial rows of an element.  Every thread hands in the sum
// s of its slot's rows (each kernel has its own loop over them); the slots are added through LDS in slot order and the
// slot-0 thread of a live element stores out[i].  Bitwise reproducible.
__device__ __forceinline__ void fold_slots_store(double s, double* __restrict__ out, int64_t i, bool live) {
  __shared__ double sacc[16][17];
  const int ii = threadIdx.x & 15, slot = threadIdx.x >> 4;
  sacc[slot][ii] = s;
  __syncthreads();
  if (slot == 0 && live) {
    double t = sacc[0][ii];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += sacc[k][ii];
    out[i] = t;
  }
}

}  // namespace admm
