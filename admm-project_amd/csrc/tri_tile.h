// tri_tile.h -- device helpers of the kernels that walk 128 x 128 tiles of a tile-packed triangle (symv.hip, trsv.hip):
// the tile numbering, the N-part column panel (lane owns a row pair, the input broadcast by v_readlane) and the T-part
// tile pass (column sums by the reduce-scatter of wave_reduce.h).  Also the one double2_t of the library.
#pragma once
#include "wave_reduce.h"

namespace admm {

typedef double double2_t __attribute__((ext_vector_type(2)));

constexpr int kTile = 128;  // rows per wave (64 lanes x 2) = columns per tile

// tile t of the lower triangle in row-major order (0,0), (1,0), (1,1), (2,0), ... -> (bi, bj)
__device__ __forceinline__ void tri_decode(unsigned t, unsigned& bi, unsigned& bj) {
  unsigned r = static_cast<unsigned>((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1u) / 2u > t) --r;
  while ((r + 1u) * (r + 2u) / 2u <= t) ++r;
  bi = r;
  bj = t - r * (r + 1u) / 2u;
}

// ---------------------------------------------------------------- N-part: a panel of P columns, rows in registers
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Mr: the lane's row pair in column 0; columns c .. c + P - 1
template <int P, bool NT>
__device__ __forceinline__ void panel_load(const double* __restrict__ Mr, int64_t ld, int64_t c, double2_t (&d)[P]) {
#pragma unroll
  for (int k = 0; k < P; ++k) d[k] = load2<NT>(Mr + (c + k) * ld);
}

// pair: lane l holds the input pair of the wave's columns (2l, 2l + 1); co = first column of the panel within the wave
template <int P>
__device__ __forceinline__ void panel_fma(double2_t pair, int co, const double2_t (&d)[P], double& a0, double& a1) {
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const double xj = readlane_f64((k & 1) ? pair.y : pair.x, (co + k) >> 1);
    a0 = __builtin_fma(d[k].x, xj, a0);
    a1 = __builtin_fma(d[k].y, xj, a1);
  }
}

// ---------------------------------------------------------------- T-part (and both parts at once): one tile pass
// (kSyPanel = 4 columns per panel = loads per buffer = T-part accumulators: wave_reduce.h)
struct SyLane {  // per-lane constants of a tile
  const double* M;
  const double* x;
  int64_t ld, n;
  int r;  // this lane's row pair (r, r+1), also its element offset from a column base
  double xr0, xr1;
};

template <bool NT>
__device__ __forceinline__ void sy_load(const SyLane& s, int64_t cp, double2_t (&d)[kSyPanel]) {
#pragma unroll
  for (int k = 0; k < kSyPanel; ++k) d[k] = load2<NT>(s.M + (cp + k) * s.ld + s.r);  // wave-uniform column base
}

// DIAG: the tile intersects the diagonal -> mask element-wise (N-part j <= row, T-part row > j)
// NP / TP: which of the two uses of an element are taken (both for the symmetric product; the T-part alone for the
// backward pass over a triangular inverse, whose diagonal tiles store their zeros: DIAG = false there)
template <bool DIAG, bool NP = true, bool TP = true>
__device__ __forceinline__ void sy_compute(const SyLane& s, int64_t cp, const double2_t (&d)[kSyPanel], double& n0,
                                           double& n1, double* __restrict__ tout, int lane) {
  double tacc[kSyPanel];
#pragma unroll
  for (int k = 0; k < kSyPanel; ++k) {
    const int64_t j = cp + k;
    const double xj = NP ? s.x[j < s.n ? j : s.n - 1] : 0.0;  // wave-uniform -> scalar load; padding columns are 0
    double a0 = d[k].x, a1 = d[k].y;
    double t0 = a0, t1 = a1;
    if (DIAG) {
      t0 = (s.r > j) ? a0 : 0.0;
      t1 = (s.r + 1 > j) ? a1 : 0.0;
      a0 = (j <= s.r) ? a0 : 0.0;
      a1 = (j <= s.r + 1) ? a1 : 0.0;
    }
    if (TP) tacc[k] = __builtin_fma(t0, s.xr0, t1 * s.xr1);
    if (NP) {
      n0 = __builtin_fma(a0, xj, n0);
      n1 = __builtin_fma(a1, xj, n1);
    }
  }
  if (TP) {
    const double sum = reduce_scatter4(tacc);
    if ((lane & 15) == 0) tout[cp + (lane >> 4)] = sum;
  }
}

// the 32 panels of one tile, next panel's loads issued before this panel's reduction
// NBUF panel buffers: NBUF - 1 panels (4 KB each per wave) in flight while one is consumed.  The launch is ONE
// generation of one-tile waves (3160 tiles on 256 CUs at n = 10^4: 12.3 waves per CU, set by the tile count, not by
// registers), so the bytes in flight per CU are 12.3 x (NBUF - 1) x 4 KB (+ the panel being waited for).
template <bool DIAG, bool NT, bool NP = true, bool TP = true, int NBUF = 2>
__device__ __forceinline__ void sy_tile(const SyLane& s, int64_t c0, double& n0, double& n1,
                                        double* __restrict__ tout, int lane) {
  constexpr int kPanels = kTile / kSyPanel, kFull = (kPanels / NBUF) * NBUF;
  static_assert(NBUF >= 2 && NBUF <= 8, "ring of panel buffers");
  double2_t buf[NBUF][kSyPanel];
#pragma unroll
  for (int b = 0; b + 1 < NBUF; ++b) sy_load<NT>(s, c0 + b * kSyPanel, buf[b]);
#pragma unroll 1
  for (int g = 0; g < kFull; g += NBUF) {
#pragma unroll
    for (int b = 0; b < NBUF; ++b) {
      // panel g + b is consumed from buf[b]; the panel NBUF - 1 ahead goes into the buffer freed last
      const int nxt = g + b + NBUF - 1;
      if (kFull - NBUF + b + NBUF - 1 < kPanels || nxt < kPanels)  // (first test: compile time, true for every g)
        sy_load<NT>(s, c0 + nxt * kSyPanel, buf[(b + NBUF - 1) % NBUF]);
      sy_compute<DIAG, NP, TP>(s, c0 + (g + b) * kSyPanel, buf[b], n0, n1, tout, lane);
    }
  }
#pragma unroll
  for (int b = 0; b < kPanels - kFull; ++b) {  // the panels a ring that does not divide 32 leaves over
    if (kFull + b + NBUF - 1 < kPanels) sy_load<NT>(s, c0 + (kFull + b + NBUF - 1) * kSyPanel, buf[(b + NBUF - 1) % NBUF]);
    sy_compute<DIAG, NP, TP>(s, c0 + (kFull + b) * kSyPanel, buf[b], n0, n1, tout, lane);
  }
}

}  // namespace admm
