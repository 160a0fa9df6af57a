// softmax_device.h -- the row prox of the multinomial (softmax) loss as an inline device function: shared
// by the multinomial row kernel of sparse_l1class.hip and by the stand-alone operator admm_op_softmax_prox.
//   z = argmin_z a*(lse(z) - z_y) + 1/2*||z - v||^2        over the CN classes of one row, a = C*c_i/rho >= 0
// is the root of F(z) = z - v + a*(softmax(z) - e_y), whose Jacobian I + a*(diag p - p p') is a diagonal g_c = 1 + a*p_c
// minus the rank-one a*p p': Newton's step d = -J^-1 F by Sherman-Morrison,
//   w_c = F_c/g_c,  s = sum_c p_c*w_c,  den = 1 - a*sum_c p_c^2/g_c,  d_c = -(w_c + (p_c/g_c)*(a*s/den)).
// den > 0 always; it is formed as sum_c p_c/g_c, the same number with sum p = 1 and no cancellation where one class
// holds nearly all the mass.  The exponentials are taken behind the subtraction of max z, and the true class's
// p_y - 1 as -sum_{c != y} p_c.  A full step can increase ||F|| (z = v with a large and the true class far behind: the
// step lands a away, where the quadratic alone sends it straight back), so a step is halved until
// ||F(z + t d)||^2 <= (1 - 1e-4*t)*||F(z)||^2: d is a descent direction of ||F||^2 and J >= I, so the damped iteration
// converges from every start.  The iteration starts at z = v and ends when ||F||_inf <= kSoftmaxFloor*eps*max(1,
// ||v||_inf, a) -- the rounding of F's own terms -- when no halved step lowers ||F|| (rounding level reached above the
// floor), or at kSoftmaxCap steps.  a = 0: F(v) = 0, no step, z = v bit for bit.
// Every loop runs over the compile-time CN and every index into the per-class arrays is a loop counter: the arrays stay
// in registers (the true class is a predicate c == y, never a subscript).
#pragma once
#include "common.h"

namespace admm {

constexpr int kSoftmaxCap = 100;       // Newton steps of one row at the most
constexpr int kSoftmaxHalvings = 12;   // halvings of one step at the most
constexpr double kSoftmaxFloor = 4.0;  // the residual floor in units of eps*max(1, ||v||_inf, a)

#ifdef __HIPCC__
// F, p, ||F||^2 and ||F||_inf at z
template <int CN>
__device__ __forceinline__ void softmax_residual(const double (&z)[CN], const double (&v)[CN], int y, double a,
                                                 double (&F)[CN], double (&p)[CN], double* n2, double* ninf) {
  double zmax = z[0];
#pragma unroll
  for (int c = 1; c < CN; ++c) zmax = fmax(zmax, z[c]);
  double S = 0.0, So = 0.0;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    p[c] = exp(z[c] - zmax);
    S += p[c];
    So += (c == y) ? 0.0 : p[c];
  }
  const double py1 = -(So / S);  // p_y - 1
  double s2 = 0.0, si = 0.0;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    p[c] = p[c] / S;
    F[c] = (z[c] - v[c]) + a * ((c == y) ? py1 : p[c]);
    s2 += F[c] * F[c];
    si = fmax(si, fabs(F[c]));
  }
  *n2 = s2;
  *ninf = si;
}

// z <- the prox at v for the true class y and a >= 0; returns the Newton steps taken
template <int CN>
__device__ __forceinline__ int softmax_prox(const double (&v)[CN], int y, double a, double (&z)[CN]) {
  double F[CN], p[CN], n2, ninf;
  double scale = fmax(1.0, a);
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    z[c] = v[c];
    scale = fmax(scale, fabs(v[c]));
  }
  const double floor_ = kSoftmaxFloor * 2.220446049250313e-16 * scale;
  softmax_residual<CN>(z, v, y, a, F, p, &n2, &ninf);
  int it = 0;
  while (ninf > floor_ && it < kSoftmaxCap) {
    double d[CN], q[CN], s = 0.0, den = 0.0;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      const double g = 1.0 + a * p[c];
      d[c] = F[c] / g;  // w_c
      q[c] = p[c] / g;
      s += p[c] * d[c];
      den += q[c];
    }
    const double r = (a * s) / den;
#pragma unroll
    for (int c = 0; c < CN; ++c) d[c] = -(d[c] + q[c] * r);
    double t = 1.0, zt[CN], Ft[CN], n2t, ninft;
    bool ok = false;
    for (int h = 0; h <= kSoftmaxHalvings && !ok; ++h) {
#pragma unroll
      for (int c = 0; c < CN; ++c) zt[c] = z[c] + t * d[c];
      softmax_residual<CN>(zt, v, y, a, Ft, p, &n2t, &ninft);
      ok = n2t <= (1.0 - 1e-4 * t) * n2;
      t *= 0.5;
    }
    if (!ok) {  // rounding level: z stays
      break;
    }
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      z[c] = zt[c];
      F[c] = Ft[c];
    }
    n2 = n2t;
    ninf = ninft;
    ++it;
  }
  return it;
}

// lse(t) - t_y of one row: the multinomial loss at the scores t
template <int CN>
__device__ __forceinline__ double softmax_loss(const double (&t)[CN], int y) {
  double tmax = t[0];
#pragma unroll
  for (int c = 1; c < CN; ++c) tmax = fmax(tmax, t[c]);
  double S = 0.0, ty = 0.0;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    S += exp(t[c] - tmax);
    ty = (c == y) ? t[c] : ty;
  }
  return (tmax - ty) + log(S);
}
#endif

}  // namespace admm
