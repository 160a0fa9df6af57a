// group_multi.h -- the grouped z-update of the multi-fit lasso objects (sparse_lasso.hip, lasso_multi.hip):
// q32's family with groups in force, K fits at once over the fit-interleaved layout [chunks][n][kSpmmChunk],
//   g_k(z) = lambda_k*sum_g omega_g*||z_g|| + l1_k*sum_i w_i*|z_i| + mu_k/2*||z||^2 + [z >= 0 where nonneg_k]
// with contiguous groups and group weights shared by all fits.  The plan is loop_kernels.h's GroupPlan under the limits
// of this layout: whole groups per workgroup, the budget counted in rows (every row carries the kSpmmChunk fits of its
// chunk), at most kGmMaxGroups groups and kScgMaxWg workgroups.  What the two objects share on the host -- the checks,
// the plan, the upload -- lives here once.
#pragma once
#include "multi_host.h"
#include "sparse_lasso.h"

namespace admm {

constexpr int kGmMaxGroups = 256;  // groups of one workgroup: their sums of squares / scales per (group, fit) live in LDS
// the budget starts at one row block and doubles until the plan fits kScgMaxWg workgroups (= the partial sums of a fit)
constexpr GroupPlanLimits kGmLimits{kScgRows, kGmMaxGroups, kScgMaxWg};

struct GroupMulti {
  GroupPlan plan{};
  double* blob = nullptr;  // the plan on the device; null: no groups, the ungrouped element kernel runs
  double* l1 = nullptr;    // K values l1_k on the device
  bool on() const { return blob != nullptr; }
};

// G groups of `sizes` (and weights gw, or null: 1) with the per-fit l1 strengths (K values, or null: 0) on h's device;
// G == 0 or sizes == null: no groups.  ADMM_E_INVALID: a size below 1, sizes that do not sum to n, a negative or
// non-finite group weight (its index named) or l1[k] (the fit named); ADMM_E_UNSUPPORTED: more than
// kScgMaxWg * kGmMaxGroups groups of one element.  A refused call changes nothing.
int set_multi_groups(MultiHost& h, int64_t n, int32_t G, const int64_t* sizes, const double* gw, const double* l1,
                     GroupMulti* gm);

// slm_elem_kernel's iteration form with the three-stage prox; the partial sums of workgroup b go to slot b of a.part, so
// the finalize sums gm.plan.nwg of them
void launch_slm_group_elem(const SlmElemArgs& a, const GroupMulti& gm, hipStream_t stream);

// stage 2 alone: Z(:, k) = block soft threshold of V(:, k) with the thresholds t[k]*omega_g, for the fits rec leaves
// running (rec == null: all); V, Z multi-vectors of len gp.n, t and rec on the device
void launch_group_multi_shrink(const double* V, double* Z, int32_t K, const GroupPlan& gp, const double* t,
                               const MultiRec* rec, hipStream_t stream);

}  // namespace admm
