// svm_cost_device.h -- the cost form of the linear SVM's element update as inline device functions: shared
// by the SvmCostArgs instantiations of the element updates (loop_kernels.hip: prox_kernel, prox_fin_kernel; unwrapped.hip:
// uw_prox_kernel, ad_onepass_kernel), which with_prox_family (prox_device.h) picks for a ProxFamily of kind FAM_COST, by
// svm_ovr.hip's ovr_pass_kernel and by the stand-alone operator (ops.hip).
//   g(z) = C * sum_i c_i*phi(ell_i*z_i),   c_i = w_i*(ell_i > 0 ? cost_pos : cost_neg),   t_i = C*c_i/rho
//   hinge     phi(s) = max(1 - s, 0)       z = v + ell*max(min(1 - s, t_i), 0)
//   sqhinge   phi(s) = max(1 - s, 0)^2     z = s >= 1 ? v : ell*(s + 2 t_i)/(1 + 2 t_i)
//   logistic  phi(s) = log(1 + e^-s)       z = ell*logistic_root(s, t_i)
//   01        phi(s) = [s < 1]             z = ell*y,  y = s if s >= 1 or s < 1 - sqrt(2 t_i), else 1
// with s = ell*v.  c_i = 0 returns v bit for bit (ell = +-1).  The squared hinge exists in this form only.
#pragma once
#include "prox_device.h"

namespace admm {

// the one element of a kernel's Loss... parameter pack
__device__ __forceinline__ const SvmCostArgs& loss_of(const SvmCostArgs& k) { return k; }

// the weight of element i in prox_load's round trip: without weights the load is redirected to z (a cache hit), so it
// stays unconditional and no dependent round trip appears
__device__ __forceinline__ double loss_weight(const SvmCostArgs& k, const double* z, int64_t i) {
  const double* pw = k.w ? k.w : z;
  const double wi = pw[i];
  return k.w ? wi : 1.0;
}

__device__ __forceinline__ double svm_cost_of(const SvmCostArgs& k, double wi, double ell) {
  return wi * (ell > 0.0 ? k.cost_pos : k.cost_neg);
}

// prox_{g/rho}(v) of one element with cost ci.  LOGI: the instantiation that knows ADMM_LOSS_LOGISTIC (prox_apply's note)
template <bool LOGI>
__device__ __forceinline__ double svm_cost_prox_elem(const SvmCostArgs& k, double ci, double ell, double v) {
  const double t = (k.C * ci) / k.rho;
  const double s = ell * v;
  if (LOGI && k.loss == ADMM_LOSS_LOGISTIC) return ell * logistic_root(s, t);
  if (k.loss == ADMM_LOSS_SQHINGE) return s >= 1.0 ? v : ell * ((s + 2.0 * t) / (1.0 + 2.0 * t));
  if (k.loss == ADMM_LOSS_01) {
    const double y = ((s >= 1.0) || (s < (1.0 - sqrt(2.0 * t)))) ? s : 1.0;
    return ell * y;
  }
  return v + ell * fmax(fmin(1.0 - s, t), 0.0);  // ADMM_LOSS_HINGE, ADMM_LOSS_HINGE_OBJ01
}

// c_i*phi(ell_i*(Dx)_i): the element's share of the objective (linearsvm.m:231-237 with the cost inside the sum; every
// string but 'hinge', 'sqhinge' and 'logistic' reports the 0-1 objective)
template <bool LOGI>
__device__ __forceinline__ double svm_cost_obj_elem(const SvmCostArgs& k, double ci, double q) {
  if (LOGI && k.loss == ADMM_LOSS_LOGISTIC) return ci * (fmax(-q, 0.0) + log1p(exp(-fabs(q))));
  const double h = fmax(1.0 - q, 0.0);
  if (k.loss == ADMM_LOSS_HINGE) return ci * h;
  if (k.loss == ADMM_LOSS_SQHINGE) return ci * (h * h);
  return (1.0 - q > 0.0) ? ci : 0.0;
}

// the element update of the cost form in front of prox_apply: z in a register (the launcher has set a.prox = PROX_GIVEN
// and a.objx = OBJX_NONE), the element's share of the objective in S_OBJX (the finalize scales it by C as before)
template <bool LOGI>
__device__ __forceinline__ void loss_form_z(const ProxArgs& a, const SvmCostArgs& k, double wi, double ax, ProxIn& in,
                                            double (&acc)[S_COUNT]) {
  const double uo = (a.alg == 0) ? in.u_old : in.uhat_i;  // v as prox_apply forms it
  const double ci_c = a.c ? in.c_i : 0.0;
  const double axh = (a.relax != 1.0) ? a.relax * ax - (1.0 - a.relax) * ((-in.zp) - ci_c) : ax;
  const double ci = svm_cost_of(k, wi, in.ell_i);
  in.zg_i = svm_cost_prox_elem<LOGI>(k, ci, in.ell_i, (axh + uo) - ci_c);
  if (k.want_obj) acc[S_OBJX] += svm_cost_obj_elem<LOGI>(k, ci, in.ell_i * ax);
}

}  // namespace admm
