// loss_device.h -- the loss family of the robust-regression engines as inline device functions: shared by
// the LossArgs instantiations of the element updates (loop_kernels.hip: prox_kernel, prox_fin_kernel; unwrapped.hip:
// ad_onepass_kernel), which with_prox_family (prox_device.h) picks for a ProxFamily of kind FAM_LOSS, and the stand-alone
// operator (ops.hip).
//   g(z) = sum_i w_i*phi(z_i)
//   LAD engine:   phi(z) = a*max(z - eps, 0) + b*max(-z - eps, 0)
//   Huber engine: phi(z) = (z >= 0 ? a : b)*H_delta(z),  H_delta(z) = z^2/2 (|z| <= delta), delta*|z| - delta^2/2 beyond
#pragma once
#include "prox_device.h"

namespace admm {

// the one element of a kernel's Loss... parameter pack
__device__ __forceinline__ const LossArgs& loss_of(const LossArgs& l) { return l; }

// the weight of element i in prox_load's round trip: without weights the load is redirected to z (a cache hit), so it
// stays unconditional and no dependent round trip appears
__device__ __forceinline__ double loss_weight(const LossArgs& l, const double* z, int64_t i) {
  const double* pw = l.w ? l.w : z;
  const double wi = pw[i];
  return l.w ? wi : 1.0;
}

// prox_{g/rho}(v) of one element.  LAD engine, select form: the flats land on +-eps exactly, the dead zone and w_i = 0
// return v bit for bit.  Huber engine: z = v - clamp(alpha*v/(alpha + rho), .), alpha = w_i*a (v >= 0) or w_i*b.
__device__ __forceinline__ double loss_prox_elem(const LossArgs& l, double wi, double v) {
  if (l.huber) {
    const bool pos = v >= 0.0;
    const double alpha = wi * (pos ? l.a : l.b);
    const double q = (alpha * v) / (alpha + l.rho);
    const double lim = (alpha * l.delta) / l.rho;
    const double s = pos ? fmin(fmax(q, 0.0), lim) : fmax(fmin(q, 0.0), -lim);
    return v - s;
  }
  const double ta = (wi * l.a) / l.rho, tb = (wi * l.b) / l.rho;
  if (v > l.eps + ta) return v - ta;
  if (v >= l.eps) return l.eps;
  if (v > -l.eps) return v;
  if (v >= -l.eps - tb) return -l.eps;
  return v + tb;
}

// w_i*phi(z_i): the element's share of the objective
__device__ __forceinline__ double loss_obj_elem(const LossArgs& l, double wi, double z) {
  if (l.huber) {
    const double az = fabs(z);
    const double h = az <= l.delta ? 0.5 * (z * z) : l.delta * az - 0.5 * (l.delta * l.delta);
    return wi * ((z >= 0.0 ? l.a : l.b) * h);
  }
  return wi * (l.a * fmax(z - l.eps, 0.0) + l.b * fmax(-z - l.eps, 0.0));
}

// the element update of the family in front of prox_apply: z in a register (the launcher has set a.prox = PROX_GIVEN
// and a.objz = OBJZ_NONE), the whole of g(z) in S_OBJZ.  (The flag is the kernels' LOGI, which the linear SVM's overload
// in svm_cost_device.h reads; this family has no use for it.)
template <bool LOGI = false>
__device__ __forceinline__ void loss_form_z(const ProxArgs& a, const LossArgs& l, double wi, double ax, ProxIn& in,
                                            double (&acc)[S_COUNT]) {
  const double uo = (a.alg == 0) ? in.u_old : in.uhat_i;  // v as prox_apply forms it
  const double ci = a.c ? in.c_i : 0.0;
  const double axh = (a.relax != 1.0) ? a.relax * ax - (1.0 - a.relax) * ((-in.zp) - ci) : ax;
  in.zg_i = loss_prox_elem(l, wi, (axh + uo) - ci);
  if (l.want_obj) acc[S_OBJZ] += loss_obj_elem(l, wi, in.zg_i);
}

}  // namespace admm
