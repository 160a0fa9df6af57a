// trsv.hip -- x = L' \ (L \ y): the cached-factor x-update (getProxOps.m:1200 `U \ (L \ y)`,
// 1514 `Rt \ (R \ .)`, 1455, 1247) on a dense lower Cholesky factor.  Two forms, both over tile-packed triangles of
// 128 x 128 tiles (tri_tile.h): blocked substitution (tri_step_kernel; described here) and, further down, the one-block
// form (tri1_*: the whole factor as one pre-inverted block, two passes).
//
// A triangular solve is a dependent chain; what bounds it on this part is the number of dependent steps, not
// bytes (round 1: 2*n/64 launches of 6 us = 0.05 of the HBM roofline).  So the chain is cut into K COARSE blocks
// (16 tiles of 128 = 2048 rows; K = 5 at n = 10^4) and each step is one bandwidth-bound launch:
//
//   forward  step k:  w_k = inv(L_kk) y_k ;   y_below -= L_below,k w_k
//   backward step k:  x_k = inv(L_kk)' w_k ;  w_above -= L_k,above' x_k
//
// With the diagonal-block inverse folded into its panel at build time (a block Gauss transform),
//   Fm[:, block k] = [ inv(L_kk) ; -L_below,k inv(L_kk) ]      (lower, block column k)
//   Um[:, block k] = [ -L_k,above' inv(L_kk)' ; inv(L_kk)' ]   (upper, block column k)
// a step is ONE column-panel GEMV  out = M[:, block k] * in_k  whose result rows inside the block are the
// solution block and whose other rows are added to the running right-hand side.  Both sweeps use the same
// kernel: lanes along rows (column-major => 16-byte coalesced non-temporal loads), register accumulation per
// row, one workgroup per 128 x 128 tile with 1..16 waves splitting its columns (chosen per step so that the grid
// keeps >= ~1500 waves), the input block broadcast inside the wave by v_readlane.  Each tile writes ONE partial
// row (its 128 columns); nothing synchronises inside a launch: the partial sums of step k are folded by step
// k+1 itself -- every tile sums the <= 16 partial rows of its own input columns while its matrix panel is already
// in flight, the first column tile of a row tile also carries the running right-hand side of its rows, and a few
// extra one-wave workgroups write out the previous solution block -- in fixed order: deterministic, no float
// atomics, no reduce launches.  2K + 1 launches per solve pair (K = 5 at n = 10^4); the explicit inverses are
// only of the K diagonal blocks (forward error eps*cond(L_kk), like any blocked TRSV with pre-inverted diagonal
// blocks), so this is the numerically safe fallback of the `inverse` form.
// (Split cache policy of the tile loads -- the first ncached tiles default, the rest non-temporal: symv.hip.)
#include <algorithm>

#include "finalize_device.h"
#include "kernels.h"
#include "slot_reduce.h"
#include "tri_tile.h"

namespace admm {

constexpr int kTsPanel = 8;    // columns per load group (kTile rows per wave = tile granularity of the blocks)
constexpr int kTsBlockTiles = 16;  // 2048-row blocks: K = 5 at n = 10^4 (per-launch fixed cost ~6 us: 10 -> 217 us, 16 -> 182 us, 27 -> 177 us per pair)

struct TriStepArgs {
  const double* M;         // Fm or Um, tile-packed: the 128 x 128 tiles of the lower (Fm) / upper (Um) triangle back to
                           // back, tile (R, C) at index R(R+1)/2 + C resp. C(C+1)/2 + R, column-major inside (ld 128)
  uint32_t ncached;        // tiles with index < ncached are read with default loads (they stay in the Infinity Cache from
                           // one solve to the next), the others non-temporally (symv.hip has the measurements)
  int64_t n;               // valid length of the vectors (caller vectors are not padded)
  const double* base_in;   // running right-hand side: rows outside the diagonal block carry base + partial sums
  double* base_out;
  double* diag_out;        // where the PREVIOUS step's solution block is written (w forward, x backward)
  const double* Pprev;     // [tiles of the previous block][ldp] column-tile partials of the previous step
  double* Pcur;            // same for this step
  int64_t ldp;
  int32_t dt0, dt1;        // this step's diagonal block = its columns (tile range)
  int32_t rt0, rt1;        // this step's panel rows (tile range)
  int32_t upper;           // 0 = forward sweep on Fm (lower), 1 = backward sweep on Um (upper)
  int32_t pd0, pd1;        // previous step: diagonal block,
  int32_t pr0, pr1;        //                panel rows (tiles that have partials; empty range = none),
  int32_t pupper;          //                orientation
  int32_t x_use_base;      // the input block is base_in + partial sums (0: partial sums only)
  int32_t ext0, ext1;      // row tiles of the previous solution block to write to diag_out (grid rows beyond the panel)
  const Ctrl* ctrl;
};

// partial-sum range of row tile T in the previous step
__device__ __forceinline__ void ts_prev_range(const TriStepArgs& a, int32_t T, int32_t& q0, int32_t& q1) {
  q0 = 0;
  q1 = 0;
  if (T < a.pr0 || T >= a.pr1) return;
  q1 = a.pd1 - a.pd0;
  if (T >= a.pd0 && T < a.pd1) {  // triangular diagonal block: only the tiles that exist
    if (!a.pupper) q1 = T - a.pd0 + 1;
    else q0 = T - a.pd0;
  }
}

// sum over the previous step's partials of the element pair at index e (fixed order; the loads of a group of
// sixteen are issued together: one memory round trip for a whole block of partials)
__device__ __forceinline__ double2_t ts_sum_prev(const TriStepArgs& a, int32_t q0, int32_t q1, int64_t e) {
  constexpr int G = 16;
  double2_t t{0.0, 0.0};
  const double* __restrict__ p = a.Pprev + e;
  for (int32_t q = q0; q < q1; q += G) {
    double2_t v[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int32_t qq = (q + k < q1) ? q + k : q1 - 1;  // clamped: loads stay unconditional
      v[k] = *reinterpret_cast<const double2_t*>(p + static_cast<int64_t>(qq) * a.ldp);
    }
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (q + k < q1) t += v[k];
  }
  return t;
}

__device__ __forceinline__ double2_t ts_load_vec(const double* __restrict__ b, int64_t e, int64_t n) {
  double2_t v{0.0, 0.0};
  if (e + 1 < n) v = double2_t{b[e], b[e + 1]};  // caller vectors are only 8-byte aligned
  else if (e < n) v.x = b[e];
  return v;
}

__device__ __forceinline__ void ts_store_vec(double* __restrict__ b, int64_t e, int64_t n, double2_t v) {
  if (e < n) b[e] = v.x;
  if (e + 1 < n) b[e + 1] = v.y;
}

// the tile itself: lc0 = this wave's first column inside the tile, cw0 = the same as a global column
template <int WAVES, bool NT>
__device__ __forceinline__ void tri_tile(const TriStepArgs& a, const double* __restrict__ Mr, int lc0, int64_t cw0,
                                         int64_t r, int32_t R, int32_t c, bool diag, int lane, int wave,
                                         double2_t (*red)[kWave]) {
  constexpr int WC = kTile / WAVES;
  double2_t bufA[kTsPanel], bufB[kTsPanel];
  panel_load<kTsPanel, NT>(Mr, kTile, lc0, bufA);  // the matrix does not depend on the vectors: in flight during the prologue
  // input block of this wave's columns: (base +) the previous step's partial sums, pair (2l, 2l+1) in lane l
  double2_t xp{0.0, 0.0};
  {
    int32_t q0, q1;
    ts_prev_range(a, a.dt0 + c, q0, q1);
    const int64_t e = cw0 + 2 * (lane < WC / 2 ? lane : 0);
    xp = ts_sum_prev(a, q0, q1, e);
    if (a.x_use_base) xp += ts_load_vec(a.base_in, e, a.n);
  }
  // rows outside the diagonal block carry on: base_out = base_in + previous partial sums (first column tile only)
  if (!diag && c == 0 && wave == 0) {
    int32_t q0, q1;
    ts_prev_range(a, R, q0, q1);
    if (q1 > q0 || a.base_out != a.base_in)
      ts_store_vec(a.base_out, r, a.n, ts_load_vec(a.base_in, r, a.n) + ts_sum_prev(a, q0, q1, r));
  }
  double a0 = 0.0, a1 = 0.0;
  if (WC > kTsPanel) {
#pragma unroll 1
    for (int co = 0; co < WC; co += 2 * kTsPanel) {
      panel_load<kTsPanel, NT>(Mr, kTile, lc0 + co + kTsPanel, bufB);
      panel_fma(xp, co, bufA, a0, a1);
      if (co + 2 * kTsPanel < WC) panel_load<kTsPanel, NT>(Mr, kTile, lc0 + co + 2 * kTsPanel, bufA);
      panel_fma(xp, co + kTsPanel, bufB, a0, a1);
    }
  } else {
    panel_fma(xp, 0, bufA, a0, a1);
  }
  double2_t acc{a0, a1};
  if (WAVES > 1) {
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    acc = red[0][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) acc += red[w][lane];
  }
  *reinterpret_cast<double2_t*>(a.Pcur + static_cast<int64_t>(c) * a.ldp + r) = acc;
}

// One workgroup = one 128 x 128 tile, WAVES waves of 128 x (128 / WAVES) columns each.
template <int WAVES, bool NT>
__global__ __launch_bounds__(WAVES * kWave) void tri_step_kernel(TriStepArgs a) {
  // (the control block's address together with the tile path's arguments: one scalar round trip less in front of the
  // loads of a workgroup that lives for one tile)
  asm volatile("" ::"s"(a.M), "s"(a.ncached), "s"(a.n), "s"(a.Pprev), "s"(a.Pcur), "s"(a.ldp), "s"(a.dt0), "s"(a.dt1),
               "s"(a.rt0), "s"(a.rt1), "s"(a.upper), "s"(a.ctrl));
  if (a.ctrl && a.ctrl->stop) return;
  constexpr int WC = kTile / WAVES;  // columns per wave
  __shared__ double2_t red[WAVES > 1 ? WAVES : 1][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t nrows = a.rt1 - a.rt0;
  const int32_t c = static_cast<int32_t>(blockIdx.y);
  if (static_cast<int32_t>(blockIdx.x) >= nrows) {  // write out the previous step's solution block
    if (c != 0 || wave != 0) return;
    const int32_t T = a.ext0 + static_cast<int32_t>(blockIdx.x) - nrows;
    int32_t q0, q1;
    ts_prev_range(a, T, q0, q1);
    const int64_t e = static_cast<int64_t>(T) * kTile + 2 * lane;
    ts_store_vec(a.diag_out, e, a.n, ts_sum_prev(a, q0, q1, e));
    return;
  }
  const int32_t R = a.rt0 + static_cast<int32_t>(blockIdx.x);  // row tile
  const bool diag = R >= a.dt0 && R < a.dt1;
  if (diag && (a.upper ? c < R - a.dt0 : c > R - a.dt0)) return;  // all-zero tile of the triangular block
  const int64_t r = static_cast<int64_t>(R) * kTile + 2 * lane;  // this lane's row pair
  const int64_t cw0 = static_cast<int64_t>(a.dt0 + c) * kTile + wave * WC;  // this wave's first column
  const uint32_t Ct = static_cast<uint32_t>(a.dt0 + c), Rt = static_cast<uint32_t>(R);
  const uint32_t lin = a.upper ? Ct * (Ct + 1u) / 2u + Rt : Rt * (Rt + 1u) / 2u + Ct;
  const double* __restrict__ Mr = a.M + static_cast<int64_t>(lin) * (kTile * kTile) + 2 * lane;
  if (NT && lin >= a.ncached) tri_tile<WAVES, true>(a, Mr, wave * WC, cw0, r, R, c, diag, lane, wave, red);
  else tri_tile<WAVES, false>(a, Mr, wave * WC, cw0, r, R, c, diag, lane, wave, red);
}

// x block of the last backward step: sum of its partials
__global__ __launch_bounds__(kWave) void tri_fold_kernel(TriStepArgs a) {
  if (a.ctrl && a.ctrl->stop) return;
  const int32_t T = a.ext0 + static_cast<int32_t>(blockIdx.x);
  int32_t q0, q1;
  ts_prev_range(a, T, q0, q1);
  const int64_t e = static_cast<int64_t>(T) * kTile + 2 * static_cast<int>(threadIdx.x);
  ts_store_vec(a.diag_out, e, a.n, ts_sum_prev(a, q0, q1, e));
}

// Um(j, i) = X(i, j) for the nb x nb lower-triangular block X (transposed copy of a diagonal block)
__global__ __launch_bounds__(kBlock) void ts_transpose_block_kernel(const double* __restrict__ X, int64_t ldx,
                                                                    double* __restrict__ U, int64_t ldu, int64_t nb) {
  __shared__ double T[32][33];
  const int64_t bi = blockIdx.x, bj = blockIdx.y;
  if (bi < bj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t i = bi * 32 + tx, j = bj * 32 + rr;
    T[rr][tx] = (i < nb && j < nb && i >= j) ? X[i + j * ldx] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int64_t i = bj * 32 + tx, j = bi * 32 + rr;  // U(i, j) = X(j, i)
    if (i < nb && j < nb) U[i + j * ldu] = T[tx][rr];
  }
}

// padded column-major square -> tile-packed triangle; tile t = (bi, bj), bi >= bj, holds M(bi, bj) of the lower triangle
// (upper = 0) or M(bj, bi) of the upper one (upper = 1)
__global__ __launch_bounds__(kBlock) void ts_pack_kernel(const double* __restrict__ M, int64_t ld, double* __restrict__ P,
                                                         int upper) {
  const unsigned t = blockIdx.x;
  unsigned bi, bj;
  tri_decode(t, bi, bj);
  const int64_t tr = upper ? bj : bi, tc = upper ? bi : bj;  // tile row / column in M
  const double* src = M + tc * kTile * ld + tr * kTile;
  double* dst = P + static_cast<int64_t>(t) * (kTile * kTile);
  for (int e = 2 * threadIdx.x; e < kTile * kTile; e += 2 * kBlock)
    *reinterpret_cast<double2_t*>(dst + e) =
        *reinterpret_cast<const double2_t*>(src + static_cast<int64_t>(e / kTile) * ld + (e % kTile));
}
void launch_tri_pack(const double* M, int64_t ld, double* P, unsigned ntri, int upper, hipStream_t stream) {
  hipLaunchKernelGGL(ts_pack_kernel, dim3(ntri), dim3(kBlock), 0, stream, M, ld, P, upper);
}

// geometry shared by trsv_plan_elems and trsv_build
struct TsGeom {
  int64_t npad, ntile, bt, nblk;
  size_t base_elems;  // Fm + Um (tile-packed triangles) + two partial buffers + v + w
};
static TsGeom ts_geom(int64_t n) {
  TsGeom g{};
  g.npad = round_up(n, kTile);
  g.ntile = g.npad / kTile;
  g.bt = std::min<int64_t>(kTsBlockTiles, g.ntile);
  g.nblk = ceil_div(g.ntile, g.bt);
  g.bt = ceil_div(g.ntile, g.nblk);  // balanced blocks
  g.base_elems = static_cast<size_t>(g.ntile * (g.ntile + 1) * kTile * kTile + 2 * g.bt * g.npad + 2 * g.npad);
  return g;
}

// ---------------------------------------------------------------- the one-block form (tri1_*)
// With the whole factor as ONE pre-inverted block the chain has no steps left: w = X y and x = X' w, X = inv(L), are
// two bandwidth-bound passes over the same tile-packed triangle (8 n(n+1) bytes per pair, what the substitution reads)
// and two launches (+ the fold between them).  The price is numerical: X is an explicit triangular inverse, forward error ~ eps * cond(L) per
// pass where the blocked form has eps * cond(L_kk) -- still the SQUARE ROOT of what the explicit inverse of L L' costs
// (`inverse` form).  Which of the two runs is decided by measurement at create (engine.hip: choose_trsv_form).
int trsv_resolve_form(int64_t n, int form) {
  if (const int forced = env_switches().trsv_form; forced >= 0) form = forced;
  if (n < 256) form = kTrsvBlocked;  // one or two tiles: nothing to gain
  return form;
}

struct T1Geom {
  int64_t npad, ntile, ntri;
  size_t x_elems, part_elems, w_elems;
};
static T1Geom t1_geom(int64_t n) {
  T1Geom g{};
  g.npad = round_up(n, kTile);
  g.ntile = g.npad / kTile;
  g.ntri = g.ntile * (g.ntile + 1) / 2;
  g.x_elems = static_cast<size_t>(g.ntri) * kTile * kTile;
  g.part_elems = static_cast<size_t>(g.ntile * g.npad);
  g.w_elems = static_cast<size_t>(g.npad);
  return g;
}

size_t trsv_plan_elems(int64_t n, int form) {
  if (form == kTrsvOne && n >= 256) {
    const T1Geom g = t1_geom(n);
    return g.x_elems + 2 * g.part_elems + g.w_elems;
  }
  return ts_geom(n).base_elems;
}

// The two passes: the N-part alone (w = X y: rows in registers, the panel of the blocked form at 4 columns), then the
// T-part alone (x = X' w: sy_tile's column sums, tri_tile.h) -- so both sweeps share ONE array and its Infinity-Cache
// resident share.  Forward: tile (bi, bj) writes the partial row npart[bj][rows of bi]; w = their sum over bj <= bi, by
// tri1_fold_kernel (the backward pass needs w as a vector: two values per lane).  Tiles are dealt in DEscending order
// and the backward pass in ascending order: what one pass read last the next one reads first.
// Backward: tile (bi, bj) writes tpart[bi][columns of bj]; x = sum over bi >= bj, taken by the consumer
// (prox_fin_kernel's gather, or tri1_reduce_kernel).  Every sum in a fixed order.
// (Measured, n = 10^4: forward 60 us + fold + backward 62 us = 6.4 TB/s per pass, the ceiling of a read stream that
// does not fit L2 on this part (dev/gemv_pattern: 6.8 - 7.0).  A last-arriver fold inside the forward pass -- write-through
// partial rows, a drained counter add per tile, the row tile's last tile summing it -- was built first and is gone:
// 74 us for the pass instead of 60 + 4; 3 or 4 panel buffers instead of 2 change nothing, here and in symv_lower_*.)
constexpr int kT1Panel = 4;  // forward pass: columns per load group (8: 144 VGPRs = 3 waves per SIMD = 12 tile slots per CU
                             // for 12.3 tiles per CU at n = 10^4: a second generation for the last 88 tiles)

// yp: lane l holds the input pair of the tile's columns (2l, 2l + 1)
template <bool NT, int NBUF>
__device__ __forceinline__ void t1_forward_tile(const double* __restrict__ Mr, double2_t yp, double& a0, double& a1) {
  constexpr int kPanels = kTile / kT1Panel, kFull = (kPanels / NBUF) * NBUF;
  double2_t buf[NBUF][kT1Panel];
#pragma unroll
  for (int b = 0; b + 1 < NBUF; ++b) panel_load<kT1Panel, NT>(Mr, kTile, b * kT1Panel, buf[b]);
#pragma unroll 1
  for (int g = 0; g < kFull; g += NBUF) {
#pragma unroll
    for (int b = 0; b < NBUF; ++b) {  // (the ring of sy_tile)
      const int nxt = g + b + NBUF - 1;
      if (kFull + b - 1 < kPanels || nxt < kPanels)
        panel_load<kT1Panel, NT>(Mr, kTile, nxt * kT1Panel, buf[(b + NBUF - 1) % NBUF]);
      panel_fma(yp, (g + b) * kT1Panel, buf[b], a0, a1);
    }
  }
#pragma unroll
  for (int b = 0; b < kPanels - kFull; ++b) {
    if (kFull + b + NBUF - 1 < kPanels)
      panel_load<kT1Panel, NT>(Mr, kTile, (kFull + b + NBUF - 1) * kT1Panel, buf[(b + NBUF - 1) % NBUF]);
    panel_fma(yp, (kFull + b) * kT1Panel, buf[b], a0, a1);
  }
}

template <int NBUF>
__device__ __forceinline__ void tri1_forward_body(unsigned lin, const Tri1Args& a) {
  unsigned bi, bj;
  tri_decode(lin, bi, bj);
  const int lane = threadIdx.x & 63;
  const int64_t gr = static_cast<int64_t>(bi) * kTile + 2 * lane;  // this lane's row pair
  double* __restrict__ po = a.npart + static_cast<int64_t>(bj) * a.ldp + gr;
  const double* __restrict__ Mr = a.X + static_cast<int64_t>(lin) * (kTile * kTile) + 2 * lane;
  const int64_t e = static_cast<int64_t>(bj) * kTile + 2 * lane;  // the tile's input columns: pair (2l, 2l + 1)
  double2_t yp{0.0, 0.0};  // (the caller's vector is only 8-byte aligned and not padded)
  yp.x = a.y[e < a.n ? e : a.n - 1];
  yp.y = a.y[e + 1 < a.n ? e + 1 : a.n - 1];
  if (e >= a.n) yp.x = 0.0;
  if (e + 1 >= a.n) yp.y = 0.0;
  double a0 = 0.0, a1 = 0.0;
  if (lin < a.ncached) t1_forward_tile<false, NBUF>(Mr, yp, a0, a1);
  else t1_forward_tile<true, NBUF>(Mr, yp, a0, a1);
  *reinterpret_cast<double2_t*>(po) = double2_t{a0, a1};
}

// workgroup 0 is the passenger of symv_lower_fin_kernel: the deferred finalize logic of the previous iteration
__global__ __launch_bounds__(kWave) void tri1_forward_kernel(Tri1Args a, FinArgs f, int32_t fin_pending,
                                                             const Ctrl* __restrict__ ctrl) {
  asm volatile("" ::"s"(a.X), "s"(a.n), "s"(a.npart), "s"(a.ldp), "s"(a.ncached), "s"(a.ntri), "s"(fin_pending),
               "s"(ctrl));
  if (ctrl && ctrl->stop) return;
  if (blockIdx.x == 0) {
    if (fin_pending) finalize_body<false, kWave>(f);
    return;
  }
  tri1_forward_body<2>(a.ntri - blockIdx.x, a);  // blockIdx 1 .. ntri -> tiles ntri - 1 .. 0
}

__global__ __launch_bounds__(kWave) void tri1_backward_kernel(Tri1Args a, const Ctrl* __restrict__ ctrl) {
  asm volatile("" ::"s"(a.X), "s"(a.n), "s"(a.tpart), "s"(a.ldp), "s"(a.ncached), "s"(ctrl));
  if (ctrl && ctrl->stop) return;
  const unsigned lin = blockIdx.x;
  unsigned bi, bj;
  tri_decode(lin, bi, bj);
  const int lane = threadIdx.x & 63;
  const int64_t gr = static_cast<int64_t>(bi) * kTile + 2 * lane;
  SyLane s;
  s.M = a.X + static_cast<int64_t>(lin) * (kTile * kTile);
  s.x = nullptr;
  s.ld = kTile;
  s.n = 0;
  s.r = 2 * lane;
  const double2_t wr = *reinterpret_cast<const double2_t*>(a.w + gr);
  s.xr0 = wr.x;
  s.xr1 = wr.y;
  double* __restrict__ tout = a.tpart + static_cast<int64_t>(bi) * a.ldp + static_cast<int64_t>(bj) * kTile;
  double n0 = 0.0, n1 = 0.0;
  if (lin < a.ncached) sy_tile<false, false, false, true>(s, 0, n0, n1, tout, lane);
  else sy_tile<false, true, false, true>(s, 0, n0, n1, tout, lane);
}

// x[i] = sum_{p >= d} tpart[p][i],  d = i / 128  (the stand-alone form of what prox_fin_kernel's gather does)
__global__ __launch_bounds__(kBlock) void tri1_reduce_kernel(const double* __restrict__ tpart, int64_t ldp, int64_t n,
                                                             int32_t ntile, double* __restrict__ x,
                                                             const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int slot = threadIdx.x >> 4;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 16 + (threadIdx.x & 15);
  double s = 0.0;
  if (i < n) {
    const int32_t d = static_cast<int32_t>(i / kTile);
#pragma unroll 4
    for (int32_t p = d + slot; p < ntile; p += 16) s += tpart[static_cast<int64_t>(p) * ldp + i];
  }
  fold_slots_store(s, x, i, i < n);
}

// w[i] = sum_{p <= d} npart[p][i], d = i / 128
__global__ __launch_bounds__(kBlock) void tri1_fold_kernel(const double* __restrict__ npart, int64_t ldp, int64_t npad,
                                                           double* __restrict__ w, const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int slot = threadIdx.x >> 4;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 16 + (threadIdx.x & 15);
  double s = 0.0;
  if (i < npad) {
    const int32_t d = static_cast<int32_t>(i / kTile);
#pragma unroll 4
    for (int32_t p = slot; p <= d; p += 16) s += npart[static_cast<int64_t>(p) * ldp + i];
  }
  fold_slots_store(s, w, i, i < npad);
}

void launch_tri1_forward(const Tri1Args& a, const FinArgs* fin, bool fin_pending, const Ctrl* ctrl, hipStream_t stream) {
  const FinArgs f = fin ? *fin : FinArgs{};
  hipLaunchKernelGGL(tri1_forward_kernel, dim3(a.ntri + 1u), dim3(kWave), 0, stream, a, f, (fin && fin_pending) ? 1 : 0,
                     ctrl);
  const int64_t npad = static_cast<int64_t>(a.ntile) * kTile;
  hipLaunchKernelGGL(tri1_fold_kernel, dim3(static_cast<unsigned>(ceil_div(npad, int64_t{16}))), dim3(kBlock), 0, stream,
                     a.npart, a.ldp, npad, a.w, ctrl);
}
void launch_tri1_backward(const Tri1Args& a, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(tri1_backward_kernel, dim3(a.ntri), dim3(kWave), 0, stream, a, ctrl);
}
void launch_tri1_reduce(const Tri1Args& a, double* x, const Ctrl* ctrl, hipStream_t stream) {
  hipLaunchKernelGGL(tri1_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(a.n, int64_t{16}))), dim3(kBlock), 0,
                     stream, a.tpart, a.ldp, a.n, a.ntile, x, ctrl);
}

static int tri1_build(const double* L, int64_t n, int64_t ldl, const double* dinv64, double* buf, TrsvPlan* plan,
                      hipStream_t stream) {
  TrsvPlan& p = *plan;
  p = TrsvPlan{};
  const T1Geom g = t1_geom(n);
  p.n = n;
  p.npad = g.npad;
  p.ntile = static_cast<int32_t>(g.ntile);
  p.nblk = 1;
  p.bt = p.ntile;
  p.ldm = p.npad;
  p.ldp = p.npad;
  p.one = true;
  p.X1 = buf;
  p.np1 = p.X1 + g.x_elems;
  p.tp1 = p.np1 + g.part_elems;
  p.w1 = p.tp1 + g.part_elems;
  p.streaming = stream_hint(static_cast<int64_t>(g.x_elems) * 8);
  // ONE array serves both passes: the whole Infinity-Cache budget of symv.hip goes to its first tiles
  p.ncached = p.streaming ? static_cast<int64_t>(kSymvCacheBytes / (8 * kTile * kTile)) : INT64_MAX;
  ADMM_HIP_TRY(hipMemsetAsync(buf, 0, trsv_plan_elems(n, kTrsvOne) * sizeof(double), stream));
  double* dense = nullptr;  // X = inv(L) as a padded column-major square (zero above the diagonal and outside n x n)
  const size_t msz = static_cast<size_t>(p.npad) * p.npad;
  ADMM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dense), msz * sizeof(double)));
  hipError_t se = hipMemsetAsync(dense, 0, msz * sizeof(double), stream);
  int rc = (se == hipSuccess) ? trtri_lower_from_diag(L, n, ldl, dinv64, dense, p.ldm, stream, false)
                              : fail(ADMM_E_DEVICE, "hipMemsetAsync failed");
  if (rc == ADMM_OK)
    launch_tri_pack(dense, p.ldm, p.X1, static_cast<unsigned>(g.ntri), 0, stream);
  se = hipStreamSynchronize(stream);
  (void)hipFree(dense);
  ADMM_TRY(rc);
  ADMM_HIP_TRY(se);
  return ADMM_OK;
}

Tri1Args tri1_args(const TrsvPlan& p, const double* y) {
  Tri1Args a{};
  a.X = p.X1;
  a.n = p.n;
  a.y = y;
  a.npart = p.np1;
  a.tpart = p.tp1;
  a.w = p.w1;
  a.ldp = p.ldp;
  a.ncached = static_cast<uint32_t>(p.ncached > 0xffffffffLL ? 0xffffffffLL : (p.ncached < 0 ? 0 : p.ncached));
  a.ntile = p.ntile;
  a.ntri = static_cast<uint32_t>(p.ntile) * static_cast<uint32_t>(p.ntile + 1) / 2u;
  return a;
}

void launch_tri1_pair(const TrsvPlan& p, const double* y, double* x, const FinArgs* fin, bool fin_pending,
                      const Ctrl* ctrl, hipStream_t stream) {
  const Tri1Args a = tri1_args(p, y);
  launch_tri1_forward(a, fin, fin_pending, ctrl, stream);
  launch_tri1_backward(a, ctrl, stream);
  if (x) launch_tri1_reduce(a, x, ctrl, stream);
}

// L: n x n lower factor (upper part ignored); dinv64: its inverted 64x64 diagonal blocks.
// `buf` must hold trsv_plan_elems(n) doubles and is owned by the caller.
int trsv_build(const double* L, int64_t n, int64_t ldl, const double* dinv64, double* buf, TrsvPlan* plan,
               hipStream_t stream, int form) {
  if (form == kTrsvOne && n >= 256) return tri1_build(L, n, ldl, dinv64, buf, plan, stream);
  TrsvPlan& p = *plan;
  p = TrsvPlan{};
  p.n = n;
  const TsGeom g = ts_geom(n);
  p.npad = g.npad;
  p.ntile = static_cast<int32_t>(g.ntile);
  p.bt = static_cast<int32_t>(g.bt);
  p.nblk = static_cast<int32_t>(g.nblk);
  p.ldm = p.npad;
  p.ldp = p.npad;
  const size_t msz = static_cast<size_t>(p.npad) * p.npad;                                // the dense squares they are built in
  const size_t psz = static_cast<size_t>(p.ntile) * (p.ntile + 1) / 2 * kTile * kTile;  // a packed triangle
  double* const packedF = buf;
  double* const packedU = buf + psz;
  p.P[0] = packedU + psz;
  p.P[1] = p.P[0] + static_cast<int64_t>(p.bt) * p.npad;
  p.v = p.P[1] + static_cast<int64_t>(p.bt) * p.npad;
  p.w = p.v + p.npad;
  p.streaming = stream_hint(static_cast<int64_t>(psz) * 2 * 8);
  // the split cache policy of symv.hip: both triangles are read once per solve pair and share the budget
  p.ncached = p.streaming ? static_cast<int64_t>(kSymvCacheBytes / 2 / (8 * kTile * kTile)) : INT64_MAX;
  ADMM_HIP_TRY(hipMemsetAsync(buf, 0, trsv_plan_elems(n, kTrsvBlocked) * sizeof(double), stream));
  double* dense = nullptr;  // Fm | Um as padded column-major squares: GEMM outputs, packed below
  ADMM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dense), 2 * msz * sizeof(double)));
  ADMM_HIP_TRY(hipMemsetAsync(dense, 0, 2 * msz * sizeof(double), stream));
  p.Fm = dense;
  p.Um = dense + msz;
  for (int32_t k = 0; k < p.nblk; ++k) {
    const int64_t k0 = static_cast<int64_t>(k) * p.bt * kTile;
    const int64_t nb = std::min<int64_t>(static_cast<int64_t>(p.bt) * kTile, n - k0);
    if (nb <= 0) break;
    double* Xk = p.Fm + k0 + k0 * p.ldm;
    // X_k = inv(L_kk) into Fm's (already zero) diagonal block
    ADMM_TRY(trtri_lower_from_diag(L + k0 + k0 * ldl, nb, ldl, dinv64 + (k0 / 64) * 64 * 64, Xk, p.ldm, stream, false));
    const int64_t below = n - k0 - nb;
    if (below > 0)  // Fm_below = -L_below,k * X_k
      launch_gemm(0, 0, below, nb, nb, -1.0, L + (k0 + nb) + k0 * ldl, ldl, Xk, p.ldm, 0.0, p.Fm + (k0 + nb) + k0 * p.ldm,
                  p.ldm, false, stream);
    const unsigned tb = static_cast<unsigned>(ceil_div(nb, 32));
    hipLaunchKernelGGL(ts_transpose_block_kernel, dim3(tb, tb), dim3(kBlock), 0, stream, Xk, p.ldm,
                       p.Um + k0 + k0 * p.ldm, p.ldm, nb);
    if (k0 > 0)  // Um_above = -(L_k,above)' * X_k'
      launch_gemm(1, 1, k0, nb, nb, -1.0, L + k0, ldl, Xk, p.ldm, 0.0, p.Um + k0 * p.ldm, p.ldm, false, stream);
  }
  const unsigned ntri = static_cast<unsigned>(p.ntile) * static_cast<unsigned>(p.ntile + 1) / 2u;
  launch_tri_pack(p.Fm, p.ldm, packedF, ntri, 0, stream);
  launch_tri_pack(p.Um, p.ldm, packedU, ntri, 1, stream);
  const hipError_t se = hipStreamSynchronize(stream);
  (void)hipFree(dense);
  ADMM_HIP_TRY(se);
  p.Fm = packedF;
  p.Um = packedU;
  return ADMM_OK;
}

template <int WAVES>
static void ts_launch(const TriStepArgs& a, dim3 grid, bool nt, hipStream_t stream) {
  if (nt) hipLaunchKernelGGL((tri_step_kernel<WAVES, true>), grid, dim3(WAVES * kWave), 0, stream, a);
  else hipLaunchKernelGGL((tri_step_kernel<WAVES, false>), grid, dim3(WAVES * kWave), 0, stream, a);
}

static void ts_step(const TriStepArgs& a, bool nt, hipStream_t stream) {
  const int32_t rows = a.rt1 - a.rt0, cols = a.dt1 - a.dt0;
  // waves per 128 x 128 tile: as few as still give the grid ~1500 waves (HBM needs tens of KB in flight per CU)
  int waves = 1;
  while (waves < 16 && static_cast<int64_t>(rows) * cols * waves < 1536) waves <<= 1;
  const dim3 grid(static_cast<unsigned>(rows + (a.ext1 - a.ext0)), static_cast<unsigned>(cols));
  switch (waves) {
    case 1: ts_launch<1>(a, grid, nt, stream); break;
    case 2: ts_launch<2>(a, grid, nt, stream); break;
    case 4: ts_launch<4>(a, grid, nt, stream); break;
    case 8: ts_launch<8>(a, grid, nt, stream); break;
    default: ts_launch<16>(a, grid, nt, stream); break;
  }
}

// y, x: n elements (not padded); x may alias y.
void launch_trsv_pair(const TrsvPlan& p, const double* y, double* x, const Ctrl* ctrl, hipStream_t stream) {
  if (p.one) {
    launch_tri1_pair(p, y, x, nullptr, false, ctrl, stream);
    return;
  }
  TriStepArgs a{};
  a.ncached = static_cast<uint32_t>(p.ncached > 0xffffffffLL ? 0xffffffffLL : p.ncached);
  a.ldp = p.ldp;
  a.n = p.n;
  a.ctrl = ctrl;
  int cur = 0;
  auto block = [&](int32_t k, int32_t& t0, int32_t& t1) {
    t0 = k * p.bt;
    t1 = std::min(p.ntile, t0 + p.bt);
  };
  // forward sweep: w = inv(L) y
  a.M = p.Fm;
  a.upper = 0;
  a.x_use_base = 1;
  a.diag_out = p.w;
  for (int32_t k = 0; k < p.nblk; ++k, cur ^= 1) {
    block(k, a.dt0, a.dt1);
    a.rt0 = a.dt0;
    a.rt1 = p.ntile;
    a.base_in = (k == 0) ? y : p.v;
    a.base_out = p.v;
    a.Pcur = p.P[cur];
    a.Pprev = p.P[cur ^ 1];
    if (k == 0) {
      a.pd0 = a.pd1 = a.pr0 = a.pr1 = a.ext0 = a.ext1 = 0;
    } else {
      block(k - 1, a.pd0, a.pd1);
      a.pr0 = a.pd0;
      a.pr1 = p.ntile;
      a.ext0 = a.pd0;  // w_{k-1}
      a.ext1 = a.pd1;
    }
    a.pupper = 0;
    ts_step(a, p.streaming, stream);
  }
  // backward sweep: x = inv(L)' w
  a.M = p.Um;
  a.upper = 1;
  a.diag_out = x;
  a.base_in = p.w;
  a.base_out = p.w;
  for (int32_t k = p.nblk - 1; k >= 0; --k, cur ^= 1) {
    block(k, a.dt0, a.dt1);
    a.rt0 = 0;
    a.rt1 = a.dt1;
    a.Pcur = p.P[cur];
    a.Pprev = p.P[cur ^ 1];
    if (k == p.nblk - 1) {  // the last forward step's partials ARE w of the last block
      block(k, a.pd0, a.pd1);
      a.pr0 = a.pd0;
      a.pr1 = p.ntile;
      a.pupper = 0;
      a.x_use_base = 0;
      a.ext0 = a.ext1 = 0;
    } else {
      block(k + 1, a.pd0, a.pd1);
      a.pr0 = 0;
      a.pr1 = a.pd1;
      a.pupper = 1;
      a.x_use_base = 1;
      a.ext0 = a.pd0;  // x_{k+1}
      a.ext1 = a.pd1;
    }
    ts_step(a, p.streaming, stream);
  }
  // x of block 0 from the last step's partials
  block(0, a.pd0, a.pd1);
  a.pr0 = 0;
  a.pr1 = a.pd1;
  a.pupper = 1;
  a.Pprev = p.P[cur ^ 1];
  a.ext0 = a.pd0;
  a.ext1 = a.pd1;
  hipLaunchKernelGGL(tri_fold_kernel, dim3(static_cast<unsigned>(a.ext1 - a.ext0)), dim3(kWave), 0, stream, a);
}

}  // namespace admm
