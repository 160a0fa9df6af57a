// group_multi_device.h -- the two-pass sum-of-squares walk of the grouped element kernels over the fit-interleaved layout
// [chunks][n][kSpmmChunk], as inline device functions: shared by group_multi.hip (the multi-fit
// lasso objects and the stand-alone shrink) and the grouped element kernels of the two classifier objects
// (l1class_group_device.h).  One copy of the summation order: group_device.h's four accumulators per (group, fit), the
// rows of a block in row order, the blocks of a workgroup in walking order.
#pragma once
#include "group_device.h"
#include "group_multi.h"

namespace admm {

// The row block [cs, ce) (at most kScgRows rows) of a workgroup that starts at group g0: sq[row - cs][fit] holds the
// squares, a barrier behind them.  Thread (r, c) takes the groups gid[cs] + r, + kScgRows, ... of the block for fit c.
// Returns the thread's share of sum_g omega_g*scale_g*||e_g|| of fit c.  The caller puts a barrier behind the call.
__device__ __forceinline__ double gm_chunk(const GroupPlan& gp, int32_t g0, int64_t cs, int64_t ce, const ScgLane& l,
                                           double t, const double* sq, double* gacc) {
  constexpr int KC = kSpmmChunk;
  double objz = 0.0;
  if (!l.run) return objz;
  const int32_t jhi = gp.gid[ce - 1] - g0;
  for (int32_t j = gp.gid[cs] - g0 + l.r; j <= jhi; j += kScgRows) {
    const int64_t o0 = gp.off[g0 + j], o1 = gp.off[g0 + j + 1];
    const int64_t lo = o0 > cs ? o0 : cs, hi = o1 < ce ? o1 : ce;
    const double* q = sq + (lo - cs) * KC + l.c;
    const int32_t cnt = static_cast<int32_t>(hi - lo);
    const double s = group_sq_sum<KC>(q, cnt);  // column c of the tile, in row order
    double* ga = gacc + j * KC + l.c;
    const double tot = (o0 >= cs) ? s : *ga + s;
    if (o1 <= ce) {  // the group ends here: group_chunk's rule
      double nrm;
      const double wg = gp.w ? gp.w[g0 + j] : 1.0;
      const double sc = group_scale(tot, t * wg, &nrm);
      *ga = sc;
      objz += wg * (sc * nrm);
    } else {
      *ga = tot;
    }
  }
  return objz;
}

// pass 1 over the workgroup's rows with elem(i) = the stage-1 value of (row i, the thread's fit); leaves the scales in
// gacc, a barrier behind them
template <class Elem>
__device__ __forceinline__ double gm_scales(const GroupPlan& gp, const ScgLane& l, double t, Elem elem, double* sq,
                                            double* gacc) {
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x];
  double objz = 0.0;
  for (int64_t cs = E0; cs < E1; cs += kScgRows) {
    const int64_t ce = (cs + kScgRows < E1) ? cs + kScgRows : E1, i = cs + l.r;
    const double ev = (l.run && i < ce) ? elem(i) : 0.0;
    sq[threadIdx.x] = ev * ev;
    __syncthreads();
    objz += gm_chunk(gp, g0, cs, ce, l, t, sq, gacc);
    __syncthreads();
  }
  return objz;
}

}  // namespace admm
