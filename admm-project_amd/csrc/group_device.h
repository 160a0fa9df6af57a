// group_device.h -- the block soft threshold of group lasso as inline device functions: shared by the
// grouped element update (loop_kernels.hip: group_prox_fin_kernel) and the stand-alone operator (ops.hip).
#pragma once
#include "prox_device.h"

namespace admm {

// the argument of the z-prox, v = (Axhat + u) - c: the expression of prox_apply and prez_kernel
__device__ __forceinline__ double group_prox_v(const ProxArgs& a, double ax, const ProxIn& in) {
  const double uo = (a.alg == 0) ? in.u_old : in.uhat_i;
  const double ci = a.c ? in.c_i : 0.0;
  const double axh = (a.relax != 1.0) ? a.relax * ax - (1.0 - a.relax) * ((-in.zp) - ci) : ax;
  return (axh + uo) - ci;
}

// The two steps every grouped z-update shares (group_chunk below; group_multi.hip's chunk over the fit-interleaved
// layout), defined once: the guarantees of the block soft threshold live here.
// The sum of cnt squares q[0], q[STRIDE], ... in index order: four interleaved accumulators, always the same ones (no
// atomics, bitwise reproducible).
template <int STRIDE>
__device__ __forceinline__ double group_sq_sum(const double* q, int32_t cnt) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int32_t k = 0;
  for (; k + 4 <= cnt; k += 4) {
    s0 += q[k * STRIDE];
    s1 += q[(k + 1) * STRIDE];
    s2 += q[(k + 2) * STRIDE];
    s3 += q[(k + 3) * STRIDE];
  }
  double s = (s0 + s1) + (s2 + s3);
  for (; k < cnt; ++k) s += q[k * STRIDE];
  return s;
}
// The scale 1 - t_g/||v_g|| of a group whose squares sum to tot, with tg = t * w_g (0 at or below the threshold; t = 0
// gives exactly 1 and ||v_g|| = 0 never divides); *nrm = ||v_g||, for the objective's w_g*scale_g*||v_g||.
__device__ __forceinline__ double group_scale(double tot, double tg, double* nrm) {
  *nrm = sqrt(tot);
  return (*nrm > tg) ? 1.0 - tg / *nrm : 0.0;
}

// One chunk [cs, ce) (at most kGroupTile elements) of a workgroup's element range: sq[k] = v_{cs+k}^2 is in LDS, a
// barrier behind it.  Thread j (of the first kGroupTile) takes the workgroup's groups g0 + j, g0 + j + kGroupTile, ...:
// it sums the squares of its group's elements inside the chunk in index order (four interleaved accumulators, always
// the same ones: no atomics, bitwise reproducible), adds them to what earlier chunks left in gacc[j] and, in the chunk
// where the group ends, replaces gacc[j] by the group's scale 1 - t_g/||v_g|| (0 at or below the threshold; t = 0
// gives exactly 1 and ||v_g|| = 0 never divides).  Returns this thread's share of sum_g w_g*||z_g|| = w_g*scale_g*||v_g||.
// The caller puts a barrier behind the call before sq or gacc are touched again.
__device__ __forceinline__ double group_chunk(const GroupPlan& gp, int32_t g0, int32_t ng, int64_t cs, int64_t ce,
                                              double t, const double* sq, double* gacc) {
  double objz = 0.0;
  if (threadIdx.x >= kGroupTile) return objz;
  for (int32_t j = threadIdx.x; j < ng; j += kGroupTile) {
    const int64_t o0 = gp.off[g0 + j], o1 = gp.off[g0 + j + 1];
    const int64_t lo = o0 > cs ? o0 : cs, hi = o1 < ce ? o1 : ce;
    if (lo >= hi) continue;
    const double* q = sq + (lo - cs);
    const int32_t cnt = static_cast<int32_t>(hi - lo);
    const double s = group_sq_sum<1>(q, cnt);
    const double tot = (o0 >= cs) ? s : gacc[j] + s;
    if (o1 <= ce) {  // the group ends here
      double nrm;
      const double wg = gp.w ? gp.w[g0 + j] : 1.0;
      const double sc = group_scale(tot, t * wg, &nrm);
      gacc[j] = sc;
      objz += wg * (sc * nrm);
    } else {
      gacc[j] = tot;
    }
  }
  return objz;
}

}  // namespace admm
