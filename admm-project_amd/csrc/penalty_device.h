// penalty_device.h -- the elementwise stages of the lasso's penalty family as inline device functions:
// shared by the penalised element updates (loop_kernels.hip: penalty_prox_fin_kernel, group_prox_fin_kernel<true>) and
// the stand-alone operator (ops.hip).
//   g(z) = l1 * sum_i w_i*|z_i| + lamG * sum_g omega_g*||z_g|| + mu/2*||z||^2 + [z >= 0 when nonneg]
//   prox_{g/rho}(v) = kappa * shrink_groups(e),  e_i = soft(v_i, tau*w_i)  or  max(v_i - tau*w_i, 0),
//   tau = l1/rho,  kappa = rho/(rho + mu)
#pragma once
#include "group_device.h"

namespace admm {

// stage 1: the weighted soft threshold, or its positive part under the sign constraint.  tau_i = 0 returns v bit for
// bit (max(v, 0) with nonneg)
__device__ __forceinline__ double penalty_elem(double v, double tau_i, int32_t nonneg) {
  if (nonneg) {
    const double a = v - tau_i;
    return a > 0.0 ? a : 0.0;
  }
  return soft(v, tau_i);
}

// tau_i = tau * w_i: one coalesced load, skipped without weights
__device__ __forceinline__ double penalty_weight(const PenaltyArgs& p, int64_t i) { return p.w ? p.w[i] : 1.0; }

// the elementwise shares of g(z) of one element: l1*w_i*|z_i| + mu/2*z_i^2
__device__ __forceinline__ double penalty_obj_elem(const PenaltyArgs& p, double wi, double z) {
  return p.l1 * (wi * fabs(z)) + p.half_mu * (z * z);
}

}  // namespace admm
