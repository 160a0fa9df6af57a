// l1class_group_device.h -- the grouped element update of the two sparse-linear-classifier objects: the
// group and sparse-group penalty of q41 on the losses of q42 / q43,
//   g_k(z2) = lambda_k*sum_g omega_g*||z2_g|| + l1_k*sum_j w_j*|z2_j| + mu_k/2*||z2||^2 + [z2 >= 0 where nonneg_k]
// as the counterpart of group_multi.hip's slm_group_elem_kernel for l1c_elem_update's contract.  Both objects keep X, Z2,
// U2 and Y as [chunks][n][kSpmmChunk], so the body is written once; an object instantiates it with its own addressing of
// g1 = D'(z1 - u1), g2 = D'(z1 - z1prev) and g3 = D'u1.
// Workgroup (b, chunk) of kScgBlock threads owns the whole groups wg_g[b] .. wg_g[b + 1] of the plan and walks their rows
// in blocks of kScgRows, twice; thread t is row t / kSpmmChunk of the block and fit t % kSpmmChunk.
//   pass 1   e = penalty_elem(x + u2, (l1_k/rho)*w_j), e^2 to LDS, the sums per (group, fit) in row order (gm_chunk), the
//            group's scale where it ends
//   pass 2   the same loads and expressions again (the same bits), z2 = kappa*(e*scale_g), u2 += x - z2,
//            Y = g1 + (z2 - u2), the six LN_* sums
// A sum of squares reads column c of the LDS tile alone: a fit's bits depend neither on its chunk, nor on its column,
// nor on whether its neighbours run.  No atomics and no cross-lane operation between fits.
#pragma once
#include "group_multi_device.h"
#include "l1class_device.h"

namespace admm {

struct L1cGroupElemArgs {
  int64_t n;
  const double* X;      // multi-vectors of len n
  double *Z2, *U2, *Y;
  const double* W;      // n l1 weights or null
  const double* par;    // K x 2: (lambda, mu); lambda is the group strength
  const double* l1;     // K values l1_k
  const int32_t* nonneg;
  const MultiRec* rec;
  double* part;         // [fit][LN_COUNT][kMultiMaxWg]: workgroup b of the plan writes slot b
  int32_t K, dual, objevals;
  double rho;
};

#ifdef __HIPCC__
constexpr int kL1cGroupLds = LN_COUNT * kScgBlock;  // doubles of the slot reduction

// gat(q, lane, base, j): element j of g_{q + 1} of the lane's fit; base = the chunk's offset in a multi-vector of len n.
// lds: kL1cGroupLds doubles, sq: kScgBlock, gacc: kGmMaxGroups * kSpmmChunk.
template <class GAt>
__device__ __forceinline__ void l1c_group_elem_body(const L1cGroupElemArgs& a, const GroupPlan& gp, GAt gat, double* lds,
                                                    double* sq, double* gacc) {
  constexpr int KC = kSpmmChunk;
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;  // no fit of the chunk runs: nothing is loaded
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[LN_COUNT];
#pragma unroll
  for (int q = 0; q < LN_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const double lam = a.par[2 * fit], mu = a.par[2 * fit + 1], l1k = a.l1[fit];
  // engine_run_general.hip's own expressions for the family's numbers with groups in force
  const PenaltyArgs pen{a.W, l1k / a.rho, a.rho / (a.rho + mu), l1k, lam, 0.5 * mu, a.nonneg[fit]};
  const double* __restrict__ X = a.X + base;
  double* __restrict__ Z2 = a.Z2 + base;
  double* __restrict__ U2 = a.U2 + base;
  double* __restrict__ Y = a.Y + base;
  auto stage1 = [&](int64_t j) {
    const int64_t e = j * KC + l.c;
    return penalty_elem(X[e] + U2[e], pen.tau * penalty_weight(pen, j), pen.nonneg);
  };
  const double oz = gm_scales(gp, l, lam / a.rho, stage1, sq, gacc);
  if (a.objevals) acc[LN_PEN] = pen.lam_group * (pen.kappa * oz);  // ||z2_g|| = kappa*scale_g*||e_g||
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x];
  for (int64_t cs = E0; cs < E1; cs += kScgRows) {
    const int64_t j = cs + l.r;
    if (!l.run || j >= E1) continue;
    const int64_t e = j * KC + l.c;
    const double xv = X[e], zp = Z2[e], uo = U2[e], wi = penalty_weight(pen, j);
    const double ei = penalty_elem(xv + uo, pen.tau * wi, pen.nonneg);
    const double zn = pen.kappa * (ei * gacc[(gp.gid[j] - g0) * KC + l.c]);
    const double rr = xv - zn;
    const double un = uo + rr;
    acc[LN_R2] += rr * rr;
    acc[LN_X2] += xv * xv;
    acc[LN_Z2] += zn * zn;
    if (a.dual) {
      const double dz = gat(1, l, base, j) + (zn - zp);  // At(z - zprev) = D'(z1 - z1prev) + (z2 - z2prev)
      const double du = gat(2, l, base, j) + un;         // At(u)
      acc[LN_DZ2] += dz * dz;
      acc[LN_DU2] += du * du;
    }
    if (a.objevals) acc[LN_PEN] += penalty_obj_elem(pen, wi, zn);
    Z2[e] = zn;
    U2[e] = un;
    Y[e] = gat(0, l, base, j) + (zn - un);
  }
  scg_sums<LN_COUNT>(acc, lds, a.part, LN_COUNT, 0);
}
#endif

}  // namespace admm
