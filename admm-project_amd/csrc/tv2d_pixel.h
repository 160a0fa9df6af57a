// tv2d_pixel.h -- one pixel of the fused 2-D TV pass (tv2d.hip: tv2d_fused_kernel has the derivation and the same
// arithmetic, statement for statement): z/u update on the compact state v = z + u, the D' stencils of the dual
// residual / tolerance and the next right-hand side b = s + rho*D'(z+ - u+).  Shared with the kernel that sends b
// straight into the forward column transform (dct.hip: tv2d_fused_dct_kernel).
#pragma once
#include "kernels.h"
#include "loop_kernels.h"
#include "tv2d.h"

namespace admm {

__device__ __forceinline__ double tv2px_clamp(double v, double t) { return __builtin_fmin(__builtin_fmax(v, -t), t); }

// The isotropic prox: the block soft threshold of the pair (v0, v1) = the two differences of one pixel,
//   z = c*v,  c = ||v|| > t ? 1 - t/||v|| : 0,   u = v - z.
// A pixel's pair is shrunk by its owner and again by the pixels below it and to its right, which must get the owner's
// bits: the sum of squares is one product and one explicit fma, and nothing here may be contracted with anything else
// (contraction is decided per call site).  ||v|| = 0 is never above t >= 0: no division; t = 0 gives c = 1 exactly.
__device__ __forceinline__ double tv2px_pair_norm(double v0, double v1) {
#pragma clang fp contract(off)
  return __builtin_sqrt(__builtin_fma(v0, v0, v1 * v1));
}
__device__ __forceinline__ void tv2px_pair_shrink(double v0, double v1, double t, double& z0, double& z1, double& u0,
                                                  double& u1) {
#pragma clang fp contract(off)
  const double n = tv2px_pair_norm(v0, v1);
  const double c = n > t ? 1.0 - t / n : 0.0;
  z0 = c * v0;
  z1 = c * v1;
  u0 = v0 - z0;
  u1 = v1 - z1;
}

// what pixel (i, j) reads: x at the 5-point stencil, the dual state of its own two differences, of the vertical
// difference above it and of the horizontal difference to its left (z as given, or v = z + u when VIN), the image
struct Tv2Px {
  double xi, x_dn, x_up, x_lf, x_rt;
  double in0, in1, in_up, in_lf;      // VIN: v; else z
  double u0, u1, u_up, u_lf;          // !VIN only
  double si;
  // ISO only: the other half of the two neighbours' pairs -- the horizontal state of (i-1, j), the vertical state of
  // (i, j-1): v when VIN, else u -- and the x they difference against, x[i-1, j+1] and x[i+1, j-1]
  double in_up1, in_lf0, u_up1, u_lf0, x_ur, x_ld;
};

// base = j*H + row0 (first row of the thread block's row chunk), r = the thread's row inside it; o_up / o_dn: row offsets
// of the neighbours relative to (base - 1) / base, clamped at the image border; lbase / rbase: the same chunk in the
// columns j -+ 1, clamped.  Every load unconditional.
template <bool VIN, bool ISO = false>
__device__ __forceinline__ void tv2px_load(const Tv2Args& a, int64_t N, int64_t base, int64_t lbase, int64_t rbase,
                                           uint32_t r, uint32_t o_up, uint32_t o_dn, Tv2Px& p) {
  const double* __restrict__ xc = a.x + base;
  const double* __restrict__ zc = a.z + base;
  p.xi = xc[r];
  p.x_dn = xc[o_dn];
  p.x_up = (xc - 1)[o_up];
  p.x_lf = (a.x + lbase)[r];
  p.x_rt = (a.x + rbase)[r];
  p.in0 = zc[r];
  p.in1 = (zc + N)[r];
  p.in_up = (zc - 1)[o_up];
  p.in_lf = (a.z + N + lbase)[r];
  if (!VIN) {
    const double* __restrict__ uc = a.u + base;
    p.u0 = uc[r];
    p.u1 = (uc + N)[r];
    p.u_up = (uc - 1)[o_up];
    p.u_lf = (a.u + N + lbase)[r];
  }
  p.si = (a.s + base)[r];
  if (ISO) {  // four more, at the same clamped offsets: two of x, and the other halves of v (VIN) or of u (the other
              // halves of the neighbours' old z are not needed)
    p.x_ur = (a.x + rbase - 1)[o_up];
    p.x_ld = (a.x + lbase)[o_dn];
    if (VIN) {
      p.in_up1 = (zc + N - 1)[o_up];
      p.in_lf0 = (a.z + lbase)[r];
    } else {
      p.u_up1 = (a.u + N + base - 1)[o_up];
      p.u_lf0 = (a.u + lbase)[r];
    }
  }
}

// The isotropic pixel: tv2px_apply below with the pair shrink in place of the two clamps.  The neighbours' new pairs
// are recomputed whole, each with the differences its owner forms (a missing one is 0.0: (i-1, j) has its vertical
// difference and this column's `hash`, (i, j-1) its horizontal one and this row's `hasv`), and come first: what stays
// live across the own-pixel accumulation is their two used components, not their inputs.
template <bool VIN>
__device__ __forceinline__ double tv2px_apply_iso(const Tv2Args& a, int64_t N, int64_t it, int64_t base, uint32_t r,
                                                  bool hasv, bool up, bool hash, bool left, const Tv2Px& p,
                                                  double (&acc)[S_COUNT]) {
  const double t = a.thresh;
  const double xi = p.xi, si = p.si;
  double z_up, z_lf, znu, unu, znl, unl;  // the used halves: vertical of (i-1, j), horizontal of (i, j-1)
  {
    double zo0, zo1, uo0, uo1, zn1, un1;
    if (VIN) {
      tv2px_pair_shrink(p.in_up, p.in_up1, t, zo0, zo1, uo0, uo1);
    } else {
      zo0 = p.in_up;
      uo0 = p.u_up;
      uo1 = p.u_up1;
    }
    z_up = zo0;
    tv2px_pair_shrink(uo0 + (p.x_up - xi), uo1 + (hash ? p.x_up - p.x_ur : 0.0), t, znu, zn1, unu, un1);
  }
  {
    double zo0, zo1, uo0, uo1, zn0, un0;
    if (VIN) {
      tv2px_pair_shrink(p.in_lf0, p.in_lf, t, zo0, zo1, uo0, uo1);
    } else {
      zo1 = p.in_lf;
      uo0 = p.u_lf0;
      uo1 = p.u_lf;
    }
    z_lf = zo1;
    tv2px_pair_shrink(uo0 + (hasv ? p.x_lf - p.x_ld : 0.0), uo1 + (p.x_lf - xi), t, zn0, znl, un0, unl);
  }
  double z_own[2], u_own[2];
  if (VIN) {
    tv2px_pair_shrink(p.in0, p.in1, t, z_own[0], z_own[1], u_own[0], u_own[1]);
  } else {
    z_own[0] = p.in0;
    z_own[1] = p.in1;
    u_own[0] = p.u0;
    u_own[1] = p.u1;
  }
  const double d[2] = {hasv ? xi - p.x_dn : 0.0, hash ? xi - p.x_rt : 0.0};
  const double vn[2] = {u_own[0] + d[0], u_own[1] + d[1]};
  double zn[2], un[2];
  tv2px_pair_shrink(vn[0], vn[1], t, zn[0], zn[1], un[0], un[1]);
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const double ax = d[part];
    const double rr = ax - zn[part], dz = zn[part] - z_own[part], du = un[part] - u_own[part];
    acc[S_R2] += rr * rr;
    acc[S_AX2] += ax * ax;
    acc[S_Z2] += zn[part] * zn[part];
    acc[S_DZ2] += dz * dz;
    acc[S_U2] += un[part] * un[part];
    acc[S_DU2] += du * du;
    (a.zo + part * N + base)[r] = vn[part];
    if (a.zhist) {
      a.zhist[it * 2 * N + part * N + base + r] = zn[part];
      a.uhist[it * 2 * N + part * N + base + r] = un[part];
    }
  }
  if (a.objevals) {
    const double e = xi - si;
    acc[S_OBJX] += e * e;
    acc[S_OBJZ] += tv2px_pair_norm(d[0], d[1]);  // once per pixel
  }
  if (a.xhist) a.xhist[it * N + base + r] = xi;
  // D'w at (i, j), in tv2_dt's order of operations
  double g2 = 0.0, g3 = 0.0, gb = 0.0;
  if (hasv) {
    g2 += zn[0] - z_own[0];
    g3 += un[0];
    gb += zn[0] - un[0];
  }
  if (up) {
    g2 -= znu - z_up;
    g3 -= unu;
    gb -= znu - unu;
  }
  if (hash) {
    g2 += zn[1] - z_own[1];
    g3 += un[1];
    gb += zn[1] - un[1];
  }
  if (left) {
    g2 -= znl - z_lf;
    g3 -= unl;
    gb -= znl - unl;
  }
  acc[S_G2] += g2 * g2;
  acc[S_G3] += g3 * g3;
  return si + a.rho * gb;
}

// returns b(i, j); stores the new compact state and the history columns, adds the pixel's terms to acc
template <bool VIN, bool ISO = false>
__device__ __forceinline__ double tv2px_apply(const Tv2Args& a, int64_t N, int64_t it, int64_t base, uint32_t r, bool hasv,
                                              bool up, bool hash, bool left, const Tv2Px& p, double (&acc)[S_COUNT]) {
  if (ISO) return tv2px_apply_iso<VIN>(a, N, it, base, r, hasv, up, hash, left, p, acc);
  const double t = a.thresh;
  double z_own[2], u_own[2], z_up, u_up, z_lf, u_lf;
  if (VIN) {
    u_own[0] = tv2px_clamp(p.in0, t);
    u_own[1] = tv2px_clamp(p.in1, t);
    u_up = tv2px_clamp(p.in_up, t);
    u_lf = tv2px_clamp(p.in_lf, t);
    z_own[0] = p.in0 - u_own[0];
    z_own[1] = p.in1 - u_own[1];
    z_up = p.in_up - u_up;
    z_lf = p.in_lf - u_lf;
  } else {
    z_own[0] = p.in0;
    z_own[1] = p.in1;
    z_up = p.in_up;
    z_lf = p.in_lf;
    u_own[0] = p.u0;
    u_own[1] = p.u1;
    u_up = p.u_up;
    u_lf = p.u_lf;
  }
  const double xi = p.xi, si = p.si;
  const double d[2] = {hasv ? xi - p.x_dn : 0.0, hash ? xi - p.x_rt : 0.0};
  double zn[2], un[2];
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const double ax = d[part];
    const double uo = u_own[part];
    const double vn = uo + ax;
    un[part] = tv2px_clamp(vn, t);
    zn[part] = vn - un[part];
    const double rr = ax - zn[part], dz = zn[part] - z_own[part], du = un[part] - uo;
    acc[S_R2] += rr * rr;
    acc[S_AX2] += ax * ax;
    acc[S_Z2] += zn[part] * zn[part];
    acc[S_DZ2] += dz * dz;
    acc[S_U2] += un[part] * un[part];
    acc[S_DU2] += du * du;
    if (a.objevals) acc[S_OBJZ] += fabs(ax);
    (a.zo + part * N + base)[r] = vn;
    if (a.zhist) {
      a.zhist[it * 2 * N + part * N + base + r] = zn[part];
      a.uhist[it * 2 * N + part * N + base + r] = un[part];
    }
  }
  if (a.objevals) {
    const double e = xi - si;
    acc[S_OBJX] += e * e;
  }
  if (a.xhist) a.xhist[it * N + base + r] = xi;
  // the rows above / to the left: new z, u of (i-1, j) in the vertical part and of (i, j-1) in the horizontal one
  const double vnu = u_up + (p.x_up - xi), vnl = u_lf + (p.x_lf - xi);
  const double unu = tv2px_clamp(vnu, t), unl = tv2px_clamp(vnl, t);
  const double znu = vnu - unu, znl = vnl - unl;
  // D'w at (i, j), in tv2_dt's order of operations
  double g2 = 0.0, g3 = 0.0, gb = 0.0;
  if (hasv) {
    g2 += zn[0] - z_own[0];
    g3 += un[0];
    gb += zn[0] - un[0];
  }
  if (up) {
    g2 -= znu - z_up;
    g3 -= unu;
    gb -= znu - unu;
  }
  if (hash) {
    g2 += zn[1] - z_own[1];
    g3 += un[1];
    gb += zn[1] - un[1];
  }
  if (left) {
    g2 -= znl - z_lf;
    g3 -= unl;
    gb -= znl - unl;
  }
  acc[S_G2] += g2 * g2;
  acc[S_G3] += g3 * g3;
  return si + a.rho * gb;
}

}  // namespace admm
