// slot_reduce.h -- the block reduction of the S_COUNT residual slots every element-update kernel ends with.
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

}  // namespace admm
