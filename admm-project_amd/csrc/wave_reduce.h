// wave_reduce.h -- cross-lane sums of a 64-lane wave WITHOUT the LDS crossbar: gfx950 v_permlane{32,16}_swap exchange
// steps and a DPP butterfly inside each 16-lane row (measured in the symmetric x-solve: 25 us cheaper per 400 MB pass
// than the ds_bpermute / __shfl_xor form).  Shared by tri_tile.h (symv.hip, trsv.hip) and unwrapped.hip.
#pragma once
#include "common.h"

namespace admm {

constexpr int kSyPanel = 4;   // values reduced together: columns per panel of the symmetric kernel

// a.upper32 <-> b.lower32: afterwards a + b holds, in the lower 32 lanes, the 2-way sum of the old
// a and, in the upper 32 lanes, the 2-way sum of the old b.
__device__ __forceinline__ void swap_half(double& a, double& b) {
  const unsigned alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
  const auto r0 = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
  a = __hiloint2double(r1[0], r0[0]);
  b = __hiloint2double(r1[1], r0[1]);
}
// odd 16-lane rows of a <-> even rows of b: same idea one level down
__device__ __forceinline__ void swap_row(double& a, double& b) {
  const unsigned alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
  const auto r0 = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
  const auto r1 = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
  a = __hiloint2double(r1[0], r0[0]);
  b = __hiloint2double(r1[1], r0[1]);
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// the sum of v over the L consecutive lanes of a group (L a power of two), valid in every lane of the group: a
// butterfly whose pairing depends on L alone.  Inside a 16-lane row the exchanges are DPP moves; 32 and 64 lanes add
// the permlane swaps above.  Every lane of the wave must be active.  (spmv.hip, spmm.hip: the lanes that share a row)
template <int L>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (L >= 64) {
    double w = v;
    swap_half(v, w);  // v = the lower half's value in both halves, w = the upper half's
    v += w;
  }
  if constexpr (L >= 32) {
    double w = v;
    swap_row(v, w);   // v = the even row's value in both rows of a pair, w = the odd row's
    v += w;
  }
  if constexpr (L >= 16) v += dpp_mov<0x128>(v);      // row_ror:8
  if constexpr (L >= 16) v += dpp_mov<0x124>(v);      // row_ror:4 (both halves of the row hold the same sums by now)
  else if constexpr (L == 8) v += dpp_mov<0x141>(v);  // row_half_mirror: lane i <- lane 7 - i of its 8
  if constexpr (L >= 4) v += dpp_mov<0x4E>(v);        // quad_perm [2,3,0,1]
  if constexpr (L >= 2) v += dpp_mov<0xB1>(v);        // quad_perm [1,0,3,2]
  return v;
}

// wave-wide maximum, valid in every lane (setup kernels: the tile maxima of the compact storage, tri_tile.h)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// reduce-scatter of 4 per-lane values over the 64 lanes: every lane returns the wave-wide sum of
// element (lane >> 4)  [lane bit 5 -> +2, bit 4 -> +1].
__device__ __forceinline__ double reduce_scatter4(double (&t)[kSyPanel]) {
  swap_half(t[0], t[2]);
  swap_half(t[1], t[3]);
  t[0] += t[2];
  t[1] += t[3];
  swap_row(t[0], t[1]);
  double r = t[0] + t[1];
  r += dpp_mov<0x128>(r);  // row_ror:8
  r += dpp_mov<0x124>(r);  // row_ror:4
  r += dpp_mov<0x4E>(r);   // quad_perm [2,3,0,1]
  r += dpp_mov<0xB1>(r);   // quad_perm [1,0,3,2]
  return r;
}

}  // namespace admm
