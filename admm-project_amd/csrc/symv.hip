// symv.hip -- y = M*x for a SYMMETRIC M reading only its lower triangle (half the bytes of a GEMV).
// Used for the explicit-inverse x-update  x = inv(D'D + rho I) * y  (getProxOps.m:1200 semantics).
//
// Every element M[r,j] (r >= j) is loaded once and used twice:
//   N-part  yN[r] += M[r,j]*x[j]        register accumulation per row (like gemv_n)
//   T-part  yT[j] += M[r,j]*x[r], r > j per-column sums over the rows (like gemv_t)
// A WAVE is the unit of work (one-wave workgroups on 128x128 tiles, 16-byte loads, lane owns a row
// pair), so the triangular tile set load-balances finely and nothing synchronises.  The storage is
// padded to whole tiles with zeros (SymvPlan::npad), so the hot loop has no edge handling at all.
// The T-part column sums of a 4-column panel are combined inside the wave WITHOUT the LDS crossbar:
// two gfx950 v_permlane{32,16}_swap exchange steps (a reduce-scatter over lane bits 5 and 4) and a
// DPP butterfly inside each 16-lane row -- measured 25 us cheaper per 400 MB pass than the
// ds_bpermute (__shfl_xor) form, which was the limiter (dev/symv_bench.hip).  The next panel's
// loads are issued before the reduction of the current one.
// Partials (npart per 128-column group, tpart per 128-row wave chunk) are added by a second small
// kernel in a fixed order: bitwise reproducible, no float atomics.
// Storage (r2c): the explicit inverses are kept TILE-PACKED -- only the lower-triangle tiles, each 128x128 tile
// contiguous (column-major inside, 128 KB), tiles in row-major triangle order (SymvPlan::packed) -- half the memory of
// the padded square, one workgroup per stored tile (no empty workgroups above the diagonal) and every wave streaming
// one contiguous 128 KB run.  Cache policy: the first SymvPlan::ncached tiles are read with default loads, the rest
// non-temporally.  The matrix is re-read every iteration and only ~180 MB of it can stay in the 256 MB Infinity Cache:
// with default loads everywhere the LRU evicts every line before its reuse (5.4 TB/s), with non-temporal loads
// everywhere nothing is kept (5.9), with the split the cacheable part is served on-die from the second pass on:
// n = 10000 (414 MB): 73.7 us column-major / all NT -> 62.6 us packed / 160 MB cacheable (dev/symv_packed.hip).
// (r2: 8-column panels -- 16 loads in flight, a three-level reduce-scatter ending in row_half_mirror -- measured
// slower than this 4-column form: 78.4 vs 76.5 us event-timed per pass.  A pure N-part pass over the same tiles,
// tri_step_kernel in trsv.hip, streams at 6.0 TB/s, so the T-part's cross-lane work is what holds this kernel at 5.4.)
// Compact storage (tri_tile.h): the kernel sits at the ingest rate of the part for the bytes it reads, so the streamed
// explicit inverse of the engine's own x-solve is stored with its off-diagonal tiles as 48-bit tile-scaled fixed point,
// 3/4 of the bytes (n = 10000: 313 MB for 414), decoded by two conversions and one FMA per element that hide behind
// the loads: 64.1 -> 50.8 us per launch, the same 6.2 TB/s over the stored bytes (EXPERIMENTS.md).  Where even that store
// is larger than kSymvCacheBytes the engine tries the 40-bit width of the same format first (5/8 of the bytes, n = 10000:
// 263 MB; engine.hip: choose_symv_storage), and where even the 40-bit store is larger, 36 and 38 bits before it (9/16
// and 19/32 of the bytes; n = 10000: 38 bits, 250 MB -- 36 bits fails the acceptance rule there): one code path, the
// width a template parameter.
// The tile pass itself (SyLane, sy_tile) is in tri_tile.h: the backward pass of the one-block triangular solve
// (trsv.hip: tri1_backward_kernel) is its T-part alone.

#include <algorithm>
#include <type_traits>

#include "finalize_device.h"
#include "kernels.h"
#include "slot_reduce.h"
#include "tri_tile.h"

namespace admm {

// PACKED = false: M is npad x npad (npad = round_up(n, 128)) column-major with ld >= npad, zero outside n x n; grid
// (ntile, ntile).  PACKED = true: M holds the lower-triangle tiles back to back (launch_symv_pack); grid = their count.
// x: n elements.  Tiles with linear index < ncached use default loads, the others non-temporal ones.
// CBITS = 36 / 38 / 40 / 48 (PACKED only): M is the compact storage of tri_tile.h -- fp64 diagonal tiles, fixed-point
// off-diagonal tiles of that width -- and scales its per-tile powers of two.  CBITS = 0: fp64 tiles.
template <bool PACKED, int CBITS = 0, int NBUF = 2>
__device__ __forceinline__ void symv_lower_body(unsigned block_x, unsigned block_y, const double* __restrict__ M,
                                                int64_t n, int64_t ld, const double* __restrict__ x,
                                                double* __restrict__ npart, double* __restrict__ tpart, int64_t ldp,
                                                int32_t part_rank, int32_t part_count, uint32_t ncached,
                                                const double* __restrict__ scales = nullptr) {
  static_assert(PACKED || !CBITS, "the compact storage is tile-packed");
  constexpr bool COMPACT = CBITS != 0;
  constexpr int BITS = COMPACT ? CBITS : 48;  // (names a format where the compact branches are compiled out)
  unsigned bi, bj, lin;
  if (PACKED) {
    lin = block_x;
    tri_decode(lin, bi, bj);
  } else {
    bi = block_x;
    bj = block_y;
    if (bi < bj) return;  // tile strictly above the diagonal
    lin = bi * (bi + 1u) / 2u + bj;
  }
  // multi-GPU: the lower-triangle tiles are dealt round-robin to the ranks; the slots of the tiles a rank
  // does not own stay at their initial zero and the partial results are summed by one all-reduce of n doubles
  if (part_count > 1 && static_cast<int32_t>(lin % static_cast<unsigned>(part_count)) != part_rank) return;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = static_cast<int64_t>(bi) * kTile;  // wave's first row
  const int64_t c0 = static_cast<int64_t>(bj) * kTile;
  const int64_t gr = w0 + 2 * lane;  // this lane's row pair
  SyLane s;
  int64_t cbase;  // first column as sy_tile counts it
  double* __restrict__ tout = tpart + static_cast<int64_t>(bi) * ldp;
  if (PACKED) {  // the tile is its own 128 x 128 matrix: local row / column numbers, x and tout shifted to its columns
    s.M = COMPACT ? reinterpret_cast<const double*>(reinterpret_cast<const char*>(M) + cq_tile_offset<BITS>(lin, bi))
                  : M + static_cast<int64_t>(lin) * (kTile * kTile);
    s.x = x + c0;
    s.ld = kTile;
    s.n = n - c0;
    s.r = 2 * lane;
    cbase = 0;
    tout += c0;
  } else {
    s.M = M;
    s.x = x;
    s.ld = ld;
    s.n = n;
    s.r = static_cast<int>(gr);
    cbase = c0;
  }
  s.xr0 = x[gr < n ? gr : n - 1];  // rows >= n multiply zero padding
  s.xr1 = x[gr + 1 < n ? gr + 1 : n - 1];
  double n0 = 0.0, n1 = 0.0;
  if (lin < ncached) {
    if (bi == bj) sy_tile<true, false, true, true, NBUF>(s, cbase, n0, n1, tout, lane);
    else if (COMPACT) sy_tile_cq<false, BITS, NBUF>(s, scales[lin], n0, n1, tout, lane);
    else sy_tile<false, false, true, true, NBUF>(s, cbase, n0, n1, tout, lane);
  } else {
    if (bi == bj) sy_tile<true, true, true, true, NBUF>(s, cbase, n0, n1, tout, lane);
    else if (COMPACT) sy_tile_cq<true, BITS, NBUF>(s, scales[lin], n0, n1, tout, lane);
    else sy_tile<false, true, true, true, NBUF>(s, cbase, n0, n1, tout, lane);
  }
  *reinterpret_cast<double2_t*>(npart + static_cast<int64_t>(bj) * ldp + gr) = double2_t{n0, n1};
}

template <bool PACKED, int CBITS = 0>
__global__ __launch_bounds__(kWave) void symv_lower_kernel(const double* __restrict__ M, int64_t n, int64_t ld,
                                                           const double* __restrict__ x, double* __restrict__ npart,
                                                           double* __restrict__ tpart, int64_t ldp,
                                                           int32_t part_rank, int32_t part_count, uint32_t ncached,
                                                           const Ctrl* __restrict__ ctrl,
                                                           const double* __restrict__ scales) {
  if (ctrl && ctrl->stop) return;
  symv_lower_body<PACKED, CBITS>(blockIdx.x, blockIdx.y, M, n, ld, x, npart, tpart, ldp, part_rank, part_count,
                                   ncached, scales);
}

// The packed x-solve with a passenger: workgroup 0 runs the finalize logic of the PREVIOUS iteration (norms, tolerances,
// stop decision: ~6 us of one workgroup's serial work) while the other workgroups stream the matrix.  Nothing in this
// launch depends on that decision, and the fused element update that follows starts after it and no-ops when it has
// raised ctrl->stop: the tail of an iteration shrinks to the element update itself (engine_run_general.hip, defer_fin).
template <int CBITS>
__global__ __launch_bounds__(kWave) void symv_lower_fin_kernel(const double* __restrict__ M, int64_t n,
                                                               const double* __restrict__ x,
                                                               double* __restrict__ npart, double* __restrict__ tpart,
                                                               int64_t ldp, int32_t part_rank, int32_t part_count,
                                                               uint32_t ncached, FinArgs f, int32_t fin_pending,
                                                               const Ctrl* __restrict__ ctrl,
                                                               const double* __restrict__ scales) {
  // Every argument of the tile path but x requested at once (fetched where first used they cost four dependent scalar
  // round trips behind the stop test, in a one-tile workgroup that lives ~15 us).  NOT x: with its pointer live this
  // early hipcc allocates 100 VGPRs instead of 84 -- five waves per SIMD instead of six, and 3 % slower, measured.
  // The compact instantiations allocate 82, all four widths (12 / 10 / 10 / 9 dwords per panel buffer instead of 16, the
  // decoded panel in 16 more): the same occupancy as the fp64 one, scales included in the early request.
  asm volatile("" ::"s"(M), "s"(n), "s"(npart), "s"(tpart), "s"(ldp), "s"(part_rank), "s"(part_count), "s"(ncached),
               "s"(fin_pending), "s"(ctrl));
  if (CBITS) asm volatile("" ::"s"(scales));
  if (ctrl->stop) return;
  if (blockIdx.x == 0) {
    if (fin_pending) finalize_body<false, kWave>(f);
    return;
  }
  symv_lower_body<true, CBITS>(blockIdx.x - 1u, 0u, M, n, 0, x, npart, tpart, ldp, part_rank, part_count, ncached,
                                 scales);
}

// K packed matrices of one size in ONE launch (consensus lasso: the K slice inverses of a rank; blockIdx.y = slice):
// x, npart, tpart of slice k at x0 + k*xstride, npart0 + k*pstride, tpart0 + k*pstride
// (workgroup (0, 0) is a passenger: the deferred finalize logic of the previous iteration, as in symv_lower_fin_kernel)
__global__ __launch_bounds__(kWave) void symv_lower_batch_kernel(const double* const* __restrict__ Ms, int64_t n,
                                                                 const double* __restrict__ x0, int64_t xstride,
                                                                 double* __restrict__ npart0,
                                                                 double* __restrict__ tpart0, int64_t pstride,
                                                                 int64_t ldp, uint32_t ncached, FinArgs f,
                                                                 int32_t fin_pending, const Ctrl* __restrict__ ctrl) {
  asm volatile("" ::"s"(Ms), "s"(n), "s"(xstride), "s"(npart0), "s"(tpart0), "s"(pstride), "s"(ldp), "s"(ncached),
               "s"(fin_pending), "s"(ctrl));  // (as in symv_lower_fin_kernel: everything but the vector pointer)
  if (ctrl && ctrl->stop) return;
  if (blockIdx.x == 0) {
    if (blockIdx.y == 0 && fin_pending) finalize_body<false, kWave>(f);
    return;
  }
  const int64_t k = blockIdx.y;
  symv_lower_body<true>(blockIdx.x - 1u, 0u, Ms[k], n, 0, x0 + k * xstride, npart0 + k * pstride, tpart0 + k * pstride,
                        ldp, 0, 1, ncached);
}

// y[i] = sum_{g <= d} npart[g][i] + sum_{w >= d} tpart[w][i],  d = i / 128 (i's diagonal tile).
// The 16 slots of a workgroup split the T+1 partial rows (slot_reduce.h: fold_slots_store).
__global__ __launch_bounds__(kBlock) void symv_reduce_kernel(const double* __restrict__ npart,
                                                             const double* __restrict__ tpart, int64_t ldp,
                                                             int64_t n, int32_t ntile, double* __restrict__ y,
                                                             const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int slot = threadIdx.x >> 4;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 16 + (threadIdx.x & 15);
  double s = 0.0;
  if (i < n) {
    const int32_t d = static_cast<int32_t>(i / kTile);
    // unified partial index p in [0, ntile]: p <= d -> npart[p], else tpart[p - 1]
#pragma unroll 4
    for (int32_t p = slot; p <= ntile; p += 16) {
      const double* src = (p <= d) ? npart + static_cast<int64_t>(p) * ldp : tpart + static_cast<int64_t>(p - 1) * ldp;
      s += src[i];
    }
  }
  fold_slots_store(s, y, i, i < n);
}

// Small symmetric M (n < ~1500: cache-resident, latency-bound): y_j = column j of M dot x, one wave per
// column, result written directly (no partials, no second kernel).  n = 400: 3 us against 12 + 4 us for the
// chunked column-dot GEMV + its reduction.
__global__ __launch_bounds__(kBlock) void symv_small_kernel(const double* __restrict__ M, int64_t n, int64_t ld,
                                                            const double* __restrict__ x, double* __restrict__ y,
                                                            const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * 4 + wid;
  if (j >= n) return;
  const double* __restrict__ col = M + j * ld;  // ld is even and M 16-byte aligned: pairs are aligned
  const int64_t npairs = n >> 1;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t p = lane; p < npairs; p += 64) {
    const double2_t m2 = *reinterpret_cast<const double2_t*>(col + 2 * p);
    const double2_t x2 = *reinterpret_cast<const double2_t*>(x + 2 * p);
    a0 = __builtin_fma(m2.x, x2.x, a0);
    a1 = __builtin_fma(m2.y, x2.y, a1);
  }
  double s = a0 + a1;
  if ((n & 1) && lane == 0) s = __builtin_fma(col[n - 1], x[n - 1], s);
  s = wave_sum(s);
  if (lane == 0) y[j] = s;
}

void launch_symv_small(const double* M, int64_t n, int64_t ld, const double* x, double* y, const Ctrl* ctrl,
                       hipStream_t stream) {
  hipLaunchKernelGGL(symv_small_kernel, dim3(static_cast<unsigned>(ceil_div(n, 4))), dim3(kBlock), 0, stream, M, n,
                     ld, x, y, ctrl);
}

// ---------------------------------------------------------------- fp64 tiles -> compact storage (tri_tile.h)
// One workgroup per tile, no atomics: the tile maximum by a wave butterfly and four LDS slots, then every thread writes
// 16-byte pieces of the panel records.  src: the tile as a column-major 128 x 128 block (ld = 128 inside a tile-packed
// triangle, the matrix's own ld inside the padded square).  deq (optional): the fp64 tile-packed triangle of the matrix
// the compact storage represents (scale * q; diagonal tiles as they are) -- what the operator tests compare.
template <int BITS>
__device__ __forceinline__ int64_t cq_quantise(double v, int shift) {  // rint(v * 2^shift), clamped
  constexpr double lim = static_cast<double>((int64_t{1} << (BITS - 1)) - 1);
  double q = rint(ldexp(v, shift));
  q = q > lim ? lim : (q < -lim ? -lim : q);
  return static_cast<int64_t>(q);
}

template <int BITS>
__global__ __launch_bounds__(kBlock) void symv_compact_pack_kernel(const double* __restrict__ M, int64_t ld, int packed,
                                                                   char* __restrict__ C, double* __restrict__ scales,
                                                                   double* __restrict__ deq) {
  __shared__ double wmax[kBlock / kWave];
  const unsigned t = blockIdx.x;
  unsigned bi, bj;
  tri_decode(t, bi, bj);
  const int64_t sld = packed ? kTile : ld;
  const double* src = packed ? M + static_cast<int64_t>(t) * (kTile * kTile)
                             : M + static_cast<int64_t>(bj) * kTile * ld + static_cast<int64_t>(bi) * kTile;
  typedef CqFormat<BITS> F;
  char* dst = C + cq_tile_offset<BITS>(t, bi);
  double* dq = deq ? deq + static_cast<int64_t>(t) * (kTile * kTile) : nullptr;
  if (bi == bj) {  // fp64 as it is
    for (int e = 2 * threadIdx.x; e < kTile * kTile; e += 2 * kBlock) {
      const double2_t v = *reinterpret_cast<const double2_t*>(src + static_cast<int64_t>(e / kTile) * sld + (e % kTile));
      *reinterpret_cast<double2_t*>(reinterpret_cast<double*>(dst) + e) = v;
      if (dq) *reinterpret_cast<double2_t*>(dq + e) = v;
    }
    if (threadIdx.x == 0) scales[t] = 1.0;
    return;
  }
  double mx = 0.0;
  for (int e = 2 * threadIdx.x; e < kTile * kTile; e += 2 * kBlock) {
    const double2_t v = *reinterpret_cast<const double2_t*>(src + static_cast<int64_t>(e / kTile) * sld + (e % kTile));
    mx = fmax(mx, fmax(fabs(v.x), fabs(v.y)));
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  int ex = 0;
  if (mx > 0.0) (void)frexp(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1): mx < 2^ex.  No logarithm of an all-zero tile.
  const int shift = BITS - 1 - ex;
  const double scale = mx > 0.0 ? ldexp(1.0, -shift) : 0.0;
  if (threadIdx.x == 0) scales[t] = scale;
  constexpr int kRuns = 3 * kWave;  // lane pieces per panel record: 16 bytes in runs 0 and 1, the hi dwords in run 2
  for (int c = threadIdx.x; c < (kTile / kSyPanel) * kRuns; c += kBlock) {
    const int p = c / kRuns, run = (c % kRuns) / kWave, l = c % kWave, r = 2 * l;
    char* rec = dst + p * F::kPanelBytes + run * 1024;
    if (run < 2) {
      uint4_t out;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int col = kSyPanel * p + 2 * run + k;
        const double2_t v = *reinterpret_cast<const double2_t*>(src + col * sld + r);
        const int64_t q0 = cq_quantise<BITS>(v.x, shift), q1 = cq_quantise<BITS>(v.y, shift);
        out[2 * k] = static_cast<unsigned>(q0 & 0xffffffff);
        out[2 * k + 1] = static_cast<unsigned>(q1 & 0xffffffff);
        if (dq) *reinterpret_cast<double2_t*>(dq + col * kTile + r) =
            double2_t{static_cast<double>(q0) * scale, static_cast<double>(q1) * scale};
      }
      *reinterpret_cast<uint4_t*>(rec + l * 16) = out;
    } else {
      uintn_t<F::kHiDwords> out = {};
      constexpr unsigned mask = (1u << F::kHiBits) - 1u;
#pragma unroll
      for (int k = 0; k < kSyPanel; ++k) {
        const double2_t v = *reinterpret_cast<const double2_t*>(src + (kSyPanel * p + k) * sld + r);
        const int64_t q0 = cq_quantise<BITS>(v.x, shift), q1 = cq_quantise<BITS>(v.y, shift);
        const int bit = 2 * k * F::kHiBits;  // fields 2k and 2k + 1 of the lane
        const unsigned f0 = static_cast<unsigned>(q0 >> 32) & mask, f1 = static_cast<unsigned>(q1 >> 32) & mask;
        if (bit % 32 + 2 * F::kHiBits <= 32) {  // share a dword
          out[bit / 32] |= (f0 << (bit % 32)) | (f1 << (bit % 32 + F::kHiBits));
        } else {  // (38 bit, k = 2: bits 24 .. 29 and 30 .. 35) the second one straddles two
          out[bit / 32] |= (f0 << (bit % 32)) | (f1 << (bit % 32 + F::kHiBits));
          out[bit / 32 + 1] |= f1 >> (32 - bit % 32 - F::kHiBits);
        }
      }
      if constexpr (BITS == 38) {  // the dword run, then the 16-bit run
        *reinterpret_cast<unsigned*>(rec + l * 4) = out[0];
        *reinterpret_cast<unsigned short*>(rec + 256 + l * 2) = static_cast<unsigned short>(out[1]);
      } else {
        *reinterpret_cast<uintn_t<F::kHiDwords>*>(rec + l * (4 * F::kHiDwords)) = out;
      }
    }
  }
}

bool symv_cbits_ok(int32_t bits) { return bits == 36 || bits == 38 || bits == 40 || bits == 48; }

// fn(std::integral_constant<int, BITS>) for the plan's compact width: the one place the widths are listed.  Any other
// value is a programming error of the caller (the engine and the operators check symv_cbits_ok): nothing is launched.
template <class Fn>
static bool with_cbits(int32_t bits, Fn&& fn) {
  switch (bits) {
    case 36: fn(std::integral_constant<int, 36>{}); return true;
    case 38: fn(std::integral_constant<int, 38>{}); return true;
    case 40: fn(std::integral_constant<int, 40>{}); return true;
    case 48: fn(std::integral_constant<int, 48>{}); return true;
    default: return false;
  }
}

SymvPlan symv_plan(int64_t n) {
  SymvPlan p{};
  p.n = n;
  p.npad = round_up(n, kTile);
  p.ldp = p.npad;
  p.ntile = static_cast<int32_t>(p.npad / kTile);
  p.packed = false;
  p.cbits = 0;
  p.scales = nullptr;
  p.ncached = symv_cached_tiles(p, kSymvCacheBytes);
  return p;
}

int64_t symv_tiles(const SymvPlan& p) { return static_cast<int64_t>(p.ntile) * (p.ntile + 1) / 2; }
size_t symv_packed_elems(const SymvPlan& p) { return static_cast<size_t>(symv_tiles(p)) * kTile * kTile; }

int64_t symv_tile_prefix_bytes(const SymvPlan& p, int64_t t) {
  if (!p.cbits) return t * int64_t{8} * kTile * kTile;
  unsigned bi, bj;
  tri_decode(static_cast<unsigned>(t), bi, bj);  // (also right for t = tiles: the row after the last)
  int64_t bytes = -1;  // (a width with_cbits refuses)
  with_cbits(p.cbits, [&](auto w) { bytes = cq_tile_offset<decltype(w)::value>(static_cast<unsigned>(t), bi); });
  return bytes;
}
size_t symv_compact_elems(const SymvPlan& p) {  // (p.cbits set)
  return static_cast<size_t>(symv_tile_prefix_bytes(p, symv_tiles(p)) / 8 + symv_tiles(p));
}
double* symv_compact_scales(const SymvPlan& p, double* C) { return C + symv_tile_prefix_bytes(p, symv_tiles(p)) / 8; }

int64_t symv_cached_tiles(const SymvPlan& p, int64_t budget_bytes) {
  const int64_t tiles = symv_tiles(p);
  if (!stream_hint(symv_tile_prefix_bytes(p, tiles))) return tiles;  // small enough to stay cache-resident as a whole
  if (!p.cbits) return std::min(tiles, budget_bytes / (int64_t{8} * kTile * kTile));
  int64_t lo = 0, hi = tiles;  // the largest t whose leading t tiles fit
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (symv_tile_prefix_bytes(p, mid) <= budget_bytes) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

void launch_symv_pack(const SymvPlan& p, const double* M, int64_t ld, double* P, hipStream_t stream) {
  launch_tri_pack(M, ld, P, static_cast<unsigned>(symv_tiles(p)), 0, stream);
}

void launch_symv_compact_pack(const SymvPlan& p, const double* M, int64_t ld, bool src_packed, double* C, double* deq,
                              hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(symv_tiles(p)));
  with_cbits(p.cbits, [&](auto w) {
    hipLaunchKernelGGL(symv_compact_pack_kernel<decltype(w)::value>, grid, dim3(kBlock), 0, stream, M, ld,
                       src_packed ? 1 : 0, reinterpret_cast<char*>(C), symv_compact_scales(p, C), deq);
  });
}

void launch_symv_reduce(const SymvPlan& p, const double* npart, const double* tpart, double* y, const Ctrl* ctrl,
                        hipStream_t stream) {
  hipLaunchKernelGGL(symv_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(p.n, 16))), dim3(kBlock), 0, stream, npart,
                     tpart, p.ldp, p.n, p.ntile, y, ctrl);
}

void launch_symv_lower(const SymvPlan& p, const double* M, int64_t ld, const double* x, double* npart, double* tpart,
                       double* y, const Ctrl* ctrl, hipStream_t stream, int part_rank, int part_count, bool reduce) {
  const uint32_t ncached = static_cast<uint32_t>(p.ncached < 0 ? 0 : p.ncached);
  const double* none = nullptr;
  if (p.packed && p.cbits)
    with_cbits(p.cbits, [&](auto w) {
      hipLaunchKernelGGL((symv_lower_kernel<true, decltype(w)::value>), dim3(static_cast<unsigned>(symv_tiles(p))),
                         dim3(kWave), 0, stream, M, p.n, ld, x, npart, tpart, p.ldp, part_rank, part_count, ncached,
                         ctrl, p.scales);
    });
  else if (p.packed)
    hipLaunchKernelGGL(symv_lower_kernel<true>, dim3(static_cast<unsigned>(symv_tiles(p))), dim3(kWave), 0, stream, M,
                       p.n, ld, x, npart, tpart, p.ldp, part_rank, part_count, ncached, ctrl, none);
  else
    hipLaunchKernelGGL(symv_lower_kernel<false>, dim3(static_cast<unsigned>(p.ntile), static_cast<unsigned>(p.ntile)),
                       dim3(kWave), 0, stream, M, p.n, ld, x, npart, tpart, p.ldp, part_rank, part_count, ncached,
                       ctrl, none);
  if (reduce) launch_symv_reduce(p, npart, tpart, y, ctrl, stream);  // else the consumer sums the rows (prox_fin_kernel)
}

void launch_symv_lower_batch(const SymvPlan& p, const double* const* Ms_dev, int32_t K, const double* x0, int64_t xstride,
                             double* npart0, double* tpart0, int64_t pstride, const Ctrl* ctrl, hipStream_t stream,
                             const FinArgs* fin) {
  const uint32_t ncached = static_cast<uint32_t>(p.ncached < 0 ? 0 : p.ncached);
  const FinArgs f = fin ? *fin : FinArgs{};
  const dim3 grid(static_cast<unsigned>(symv_tiles(p)) + 1u, static_cast<unsigned>(K));
  hipLaunchKernelGGL(symv_lower_batch_kernel, grid, dim3(kWave), 0, stream, Ms_dev, p.n, x0, xstride, npart0, tpart0,
                     pstride, p.ldp, ncached, f, fin ? 1 : 0, ctrl);
}

void launch_symv_lower_fin(const SymvPlan& p, const double* M, const double* x, double* npart, double* tpart,
                           const FinArgs& f, bool fin_pending, const Ctrl* ctrl, hipStream_t stream, int part_rank,
                           int part_count, double* y) {
  const uint32_t ncached = static_cast<uint32_t>(p.ncached < 0 ? 0 : p.ncached);
  const dim3 grid(static_cast<unsigned>(symv_tiles(p)) + 1u);
  const double* none = nullptr;
  if (p.cbits)
    with_cbits(p.cbits, [&](auto w) {
      hipLaunchKernelGGL(symv_lower_fin_kernel<decltype(w)::value>, grid, dim3(kWave), 0, stream, M, p.n, x, npart,
                         tpart, p.ldp, part_rank, part_count, ncached, f, fin_pending ? 1 : 0, ctrl, p.scales);
    });
  else
    hipLaunchKernelGGL(symv_lower_fin_kernel<0>, grid, dim3(kWave), 0, stream, M, p.n, x, npart, tpart, p.ldp,
                       part_rank, part_count, ncached, f, fin_pending ? 1 : 0, ctrl, none);
  if (y) launch_symv_reduce(p, npart, tpart, y, ctrl, stream);  // else the consumer sums the partial rows itself
}

}  // namespace admm
