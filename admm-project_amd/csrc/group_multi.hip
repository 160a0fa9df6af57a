// group_multi.hip -- the grouped element kernel of the multi-fit lasso objects (group_multi.h).
// Workgroup (b, chunk) of kScgRows * kSpmmChunk threads owns the whole groups wg_g[b] .. wg_g[b + 1] = the rows
// wg_e[b] .. wg_e[b + 1] of its chunk and walks them in row blocks of kScgRows, twice.  Thread t is row t / kSpmmChunk of
// the block and fit t % kSpmmChunk, as in every elementwise kernel of spmm_cg.h.
//   pass 1   e = penalty_elem(x + u) of the thread's (row, fit), e^2 to LDS; then the SAME thread, as (group j, fit c),
//            adds the squares of group j of fit c inside the block in row order (group_chunk's four accumulators) to
//            what earlier blocks left and, where the group ends, replaces the sum by the group's scale
//   pass 2   the same loads and expressions again (the same bits), z = kappa * (e * scale), prox_apply
// A sum of squares therefore reads column c of the LDS tile alone: it depends neither on the other fits of the chunk nor
// on whether they run, and the plan depends on the sizes alone.  No atomics and no cross-lane operation.
#include <string>
#include <vector>

#include "group_multi.h"
#include "group_multi_device.h"
#include "penalty_device.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

__global__ __launch_bounds__(kScgBlock) void slm_group_elem_kernel(SlmElemArgs a, GroupPlan gp,
                                                                   const double* __restrict__ l1) {
  __shared__ double lds[SL_COUNT * kScgBlock];
  __shared__ double sq[kScgBlock];
  __shared__ double gacc[kGmMaxGroups * KC];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[S_COUNT];
#pragma unroll
  for (int q = 0; q < S_COUNT; ++q) acc[q] = 0.0;
  const int fit = l.run ? l.fit : 0;
  const double lam = a.par[2 * fit], mu = a.par[2 * fit + 1], l1k = l1[fit];
  // engine_run_general.hip's own expressions for the family's numbers with groups in force
  const PenaltyArgs pen{a.W, l1k / a.rho, a.rho / (a.rho + mu), l1k, lam, 0.5 * mu, a.nonneg[fit]};
  ProxArgs pa{};  // slm_elem_kernel's: plain ADMM, A = 1, B = -1, c = 0, z given in a register, no histories
  pa.len = a.n;
  pa.z = a.Z + base;
  pa.u = a.U + base;
  pa.c = nullptr;
  pa.rhs = a.Y + base;
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = PROX_GIVEN;
  pa.objx = OBJX_NONE;
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;
  pa.rhs_kind = RHS_RHO_DTS;
  const double* __restrict__ X = a.X + base;
  auto stage1 = [&](int64_t i) {
    const int64_t e = i * KC + l.c;
    ProxIn in{};  // (zp stays unread: group_prox_v takes it under relaxation alone)
    in.u_old = pa.u[e];
    in.uhat_i = in.u_old;
    return penalty_elem(group_prox_v(pa, X[e], in), pen.tau * penalty_weight(pen, i), pen.nonneg);
  };
  const double oz = gm_scales(gp, l, lam / a.rho, stage1, sq, gacc);
  double obj = a.objevals ? pen.lam_group * (pen.kappa * oz) : 0.0;  // ||z_g|| = kappa*scale_g*||e_g||
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x];
  for (int64_t cs = E0; cs < E1; cs += kScgRows) {
    const int64_t i = cs + l.r;
    if (!l.run || i >= E1) continue;
    const int64_t e = i * KC + l.c;
    const double xv = X[e], wi = penalty_weight(pen, i);
    ProxIn in{};
    in.zp = pa.z[e];
    in.u_old = pa.u[e];
    in.uhat_i = in.u_old;
    in.add_i = (a.dts_ns == 1) ? a.DTS[i * KC] : a.DTS[base + e];
    const double ei = penalty_elem(group_prox_v(pa, xv, in), pen.tau * wi, pen.nonneg);
    in.zg_i = pen.kappa * (ei * gacc[(gp.gid[i] - g0) * KC + l.c]);
    if (a.objevals) obj += penalty_obj_elem(pen, wi, in.zg_i);
    prox_apply<false>(pa, e, xv, 0, 0.0, in, acc);
  }
  const double sums[SL_COUNT] = {acc[S_R2], acc[S_AX2], acc[S_Z2], acc[S_DZ2], acc[S_U2], obj};
  scg_sums<SL_COUNT>(sums, lds, a.part, SL_COUNT, 0);
}

__global__ __launch_bounds__(kScgBlock) void group_multi_shrink_kernel(const double* __restrict__ V,
                                                                       double* __restrict__ Z, int32_t K, GroupPlan gp,
                                                                       const double* __restrict__ t,
                                                                       const MultiRec* __restrict__ rec) {
  __shared__ double sq[kScgBlock];
  __shared__ double gacc[kGmMaxGroups * KC];
  const ScgLane l = scg_lane(rec, K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * gp.n * KC;
  const double tk = t[l.run ? l.fit : 0];
  gm_scales(gp, l, tk, [&](int64_t i) { return V[base + i * KC + l.c]; }, sq, gacc);
  const int64_t E0 = gp.wg_e[blockIdx.x], E1 = gp.wg_e[blockIdx.x + 1];
  const int32_t g0 = gp.wg_g[blockIdx.x];
  for (int64_t i = E0 + l.r; i < E1; i += kScgRows)
    if (l.run) Z[base + i * KC + l.c] = V[base + i * KC + l.c] * gacc[(gp.gid[i] - g0) * KC + l.c];
}

}  // namespace

void launch_slm_group_elem(const SlmElemArgs& a, const GroupMulti& gm, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(gm.plan.nwg), static_cast<unsigned>(spmm_chunks(a.K)));
  hipLaunchKernelGGL(slm_group_elem_kernel, grid, dim3(kScgBlock), 0, stream, a, gm.plan, gm.l1);
}

void launch_group_multi_shrink(const double* V, double* Z, int32_t K, const GroupPlan& gp, const double* t,
                               const MultiRec* rec, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(gp.nwg), static_cast<unsigned>(spmm_chunks(K)));
  hipLaunchKernelGGL(group_multi_shrink_kernel, grid, dim3(kScgBlock), 0, stream, V, Z, K, gp, t, rec);
}

int set_multi_groups(MultiHost& h, int64_t n, int32_t G, const int64_t* sizes, const double* gw, const double* l1,
                     GroupMulti* gm) {
  if (G < 0) return fail(ADMM_E_INVALID, "groups: their count is negative");
  const bool grouped = G > 0 && sizes;
  GroupPlanHost ph;
  if (grouped) {  // (a refused call changes nothing)
    ADMM_TRY(group_plan_build(sizes, G, gw, n, kGmLimits, &ph));
    for (int32_t k = 0; l1 && k < h.K; ++k)
      if (!finite_nonneg(l1[k]))
        return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": l1 is negative or not finite");
  }
  ADMM_HIP_TRY(hipSetDevice(h.device));
  double *blob = nullptr, *dl1 = nullptr;
  if (grouped) {
    int rc = h.mem.alloc(&blob, ph.blob.size());
    if (rc == ADMM_OK) rc = h.mem.alloc(&dl1, static_cast<size_t>(h.K));
    hipError_t he = hipSuccess;
    if (rc == ADMM_OK) he = hipMemcpyAsync(blob, ph.blob.data(), sizeof(double) * ph.blob.size(), hipMemcpyHostToDevice, h.stream);
    if (rc == ADMM_OK && he == hipSuccess)
      he = l1 ? hipMemcpyAsync(dl1, l1, sizeof(double) * h.K, hipMemcpyHostToDevice, h.stream)
              : hipMemsetAsync(dl1, 0, sizeof(double) * h.K, h.stream);
    if (rc == ADMM_OK && he == hipSuccess) he = hipStreamSynchronize(h.stream);  // (the host arrays are read until here)
    if (rc != ADMM_OK || he != hipSuccess) {
      if (blob) h.mem.free_one(blob);
      if (dl1) h.mem.free_one(dl1);
      if (rc != ADMM_OK) return rc;
      ADMM_HIP_TRY(he);
    }
  }
  if (gm->blob) h.mem.free_one(gm->blob);
  if (gm->l1) h.mem.free_one(gm->l1);
  gm->blob = blob;
  gm->l1 = dl1;
  gm->plan = grouped ? ph.bind(blob) : GroupPlan{};
  return ADMM_OK;
}

}  // namespace admm
