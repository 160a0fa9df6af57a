// symm.hip -- X(:, k) = M * Y(:, k) for a SYMMETRIC M stored as the fp64 tile-packed lower triangle of symv.hip and the
// fits k of one chunk of kSpmmChunk right-hand sides: the x-update of the dense multi-lasso, the cached
// inverse of D'D + rho*I applied to every fit in ONE read of its tiles.
//
// Every stored element M[r, c] (r >= c) is loaded from memory once per chunk and used for
//   N-part  X[r, k] += M[r, c] * Y[c, k]            T-part  X[c, k] += M[r, c] * Y[r, k], r > c
// of all ten fits: 20 FMAs per 8 bytes.  symv.hip's T-part sums a column across the lanes of a wave (a reduce-scatter per
// four columns); ten fits through that form would pay the cross-lane work ten times.  Here NO sum crosses a lane:
//   * a workgroup of four waves owns one 128 x 128 tile and walks its four 64 x 64 quadrants;
//   * a quadrant is loaded with 16-byte non-temporal loads (lane = row pair, two columns per instruction, a quarter of
//     the quadrant per wave) and written to LDS column-major with a column stride of 65 doubles;
//   * N-part (waves 0 and 2): lane l owns ROW l and reads S[c][l] (consecutive lanes, consecutive banks), wave 0 over
//     the columns c = 0 .. 31 and wave 2 over 32 .. 63;
//     T-part (waves 1 and 3): lane l owns COLUMN l and reads S[l][r] (stride 65: no bank conflict), over the rows
//     r = 0 .. 31 and 32 .. 63;
//     in both the ten values of Y belong to an index every lane shares, so they are scalar loads of 80 contiguous bytes
//     of the fit-interleaved layout, and an accumulator never leaves its lane;
//   * the two halves of a sum meet once per tile half in the staging buffer, first half + second half;
//   * the next quadrant's loads are issued before the current quadrant's FMAs.
// The scalar loads of Y come from L2 (a chunk's Y is 800 KB at n = 10^4, the scalar cache 16 KB) and every wait on one
// is a wait on all that are in flight, so the kernel is bound by that latency, not by the 20 FMAs per element: what
// helps is waves per SIMD.  Measured at n = 10^4, ten fits, tile pass alone (dev/symm_bench.hip, EXPERIMENTS.md): one
// wave per tile doing both parts 255 us (one wave per SIMD: 33 KB of LDS each), two waves (one per part) 162 us, this
// form 105 us (four waves per SIMD); a pure read of the same tiles takes 63 us.
// The row sums of a tile go to partial rows in the layout of the result, part[chunk][p][npad][kSpmmChunk] with the
// unified partial index of symv_reduce_kernel: the N-part of tile (bi, bj) is partial p = bj of the rows of bi, its T-part
// partial p = bi + 1 of the rows of bj -- every one of the ntile + 1 partials of a row is written by exactly one tile in
// every launch.  symm_reduce_kernel adds them in the order p = 0 .. ntile: no atomics, an order fixed by n alone, and a
// fit's sums never meet another fit's values.
// A fit whose MultiRec::stop is set keeps its X column (the reduce skips it); a chunk whose fits have all stopped returns
// before it reads a tile.  The storage is padded to whole tiles with zeros (SymvPlan::npad) and a diagonal tile is masked
// element by element with selects, so what lies above the diagonal is never used (quadrant (0, 1) of a diagonal tile is
// not even read).
#include "kernels.h"
#include "multi_device.h"
#include "spmm.h"
#include "tri_tile.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;
constexpr int kSub = kTile / 2;   // side of a quadrant = lanes of the wave
constexpr int kSubLd = kSub + 1;  // LDS column stride in doubles
static_assert(kSub == kWave, "a lane owns one row (N-part) and one column (T-part) of a quadrant");
static_assert(KC % 2 == 0, "a row of partials is a whole number of 16-byte stores");

constexpr int kSymmWaves = 4;  // waves 0, 2: the N-part of a quadrant over its columns 0 .. 31 / 32 .. 63; 1, 3: the T-part
constexpr int kSymmLoads = kSub / 2 / kSymmWaves;  // 16-byte loads of a lane per quadrant
constexpr int kSymmSpan = kSub / 2;                // columns (N-part) or rows (T-part) of a quadrant one wave sums
static_assert(3 * kWave * KC <= kSub * kSubLd, "the halves' sums meet in the staging buffer");

// this wave's quarter of the pairs of quadrant (hr, hc) of tile T: wave w loads the columns 16 w .. 16 w + 15, lane =
// (row pair rp, column parity cs), load j = column 16 w + 2j + cs
__device__ __forceinline__ void symm_load(const double* __restrict__ T, int hr, int hc, int wave, int lane,
                                          admm_double2 (&d)[kSymmLoads]) {
  const double* q = T + (hc * kSub + 2 * kSymmLoads * wave + (lane >> 5)) * kTile + hr * kSub + 2 * (lane & 31);
#pragma unroll
  for (int j = 0; j < kSymmLoads; ++j) d[j] = load2<true>(q + 2 * j * kTile);
}

__device__ __forceinline__ void symm_stage(double* S, int wave, int lane, const admm_double2 (&d)[kSymmLoads]) {
  double* s = S + (2 * kSymmLoads * wave + (lane >> 5)) * kSubLd + 2 * (lane & 31);
#pragma unroll
  for (int j = 0; j < kSymmLoads; ++j) {
    s[2 * j * kSubLd] = d[j].x;
    s[2 * j * kSubLd + 1] = d[j].y;
  }
}

// one part of one staged quadrant over the local indices ib .. ib + 31.  NPART: lane = row, the loop runs over the
// columns, i0 = global index of the quadrant's first column; else lane = column, the loop runs over the rows, i0 = global
// index of its first row.  MASK: the quadrant sits on the diagonal (local row and column numbers compare as the global
// ones do): the N-part takes column <= row, the T-part row > column.  CLAMP: the quadrant reaches past n (a padding row
// or column multiplies stored zeros, and Y is not read there).  Y: the chunk's right-hand sides; Y[i0 + i] is
// wave-uniform, ten scalar loads.
template <bool MASK, bool NPART, bool CLAMP>
__device__ __forceinline__ void symm_part(const double* S, int lane, const double* __restrict__ Y, int64_t n, int64_t i0,
                                          int ib, double (&acc)[KC]) {
#pragma unroll 4
  for (int i = ib; i < ib + kSymmSpan; ++i) {
    double m = NPART ? S[i * kSubLd + lane] : S[lane * kSubLd + i];
    if (MASK) m = (NPART ? (i <= lane) : (i > lane)) ? m : 0.0;
    const int64_t g = (!CLAMP || i0 + i < n) ? i0 + i : n - 1;
    const double* __restrict__ y = Y + g * KC;
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = __builtin_fma(m, y[k], acc[k]);
  }
}

template <bool NPART>
__device__ __forceinline__ void symm_quadrant(bool mask, const double* S, int lane, const double* __restrict__ Y,
                                              int64_t n, int64_t i0, int ib, double (&acc)[KC]) {
  const bool clamp = i0 + kSub > n;  // (uniform)
  if (mask) {
    if (clamp) symm_part<true, NPART, true>(S, lane, Y, n, i0, ib, acc);
    else symm_part<true, NPART, false>(S, lane, Y, n, i0, ib, acc);
  } else {
    if (clamp) symm_part<false, NPART, true>(S, lane, Y, n, i0, ib, acc);
    else symm_part<false, NPART, false>(S, lane, Y, n, i0, ib, acc);
  }
}

__device__ __forceinline__ void symm_store_row(double* __restrict__ dst, const double (&acc)[KC]) {
#pragma unroll
  for (int k = 0; k < KC; k += 2) store2<false>(dst + k, admm_double2{acc[k], acc[k + 1]});
}

// grid (lower-triangle tiles, chunks), four waves.  part: [chunks][ntile + 1][npad][KC]
__global__ __launch_bounds__(kSymmWaves* kWave) void symm_packed_kernel(const double* __restrict__ P, int64_t n,
                                                                        int64_t npad, int32_t ntile,
                                                                        const double* __restrict__ Y,
                                                                        double* __restrict__ part,
                                                                        const MultiRec* __restrict__ rec, int32_t K) {
  __shared__ double S[kSub * kSubLd];
  const int64_t chunk = blockIdx.y;
  bool any = false;
  for (int k = 0; k < KC; ++k) {
    const int64_t fit = chunk * KC + k;
    if (fit < K && (!rec || rec[fit].stop == 0)) any = true;
  }
  if (!any) return;  // (uniform) every fit of the chunk has stopped: nothing is read
  unsigned bi, bj;
  tri_decode(blockIdx.x, bi, bj);
  bi = __builtin_amdgcn_readfirstlane(bi);  // (tri_decode's square root leaves them in vector registers)
  bj = __builtin_amdgcn_readfirstlane(bj);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool tpart = wave & 1;             // the wave's part
  const int ib = (wave >> 1) * kSymmSpan;  // ... and its half of the quadrant's columns (N) or rows (T)
  const bool diag = bi == bj;
  const double* __restrict__ T = P + static_cast<int64_t>(blockIdx.x) * (kTile * kTile);
  const double* __restrict__ Yc = Y + chunk * n * KC;
  double* __restrict__ pc = part + chunk * (ntile + 1) * npad * KC;
  const int64_t row0 = static_cast<int64_t>(bi) * kTile, col0 = static_cast<int64_t>(bj) * kTile;

  // N waves: acc[0] = the rows of the tile's current half, stored and cleared after its two quadrants;
  // T waves: acc[hc] = the columns of the tile's half hc, stored at the end
  double acc[2][KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) acc[0][k] = acc[1][k] = 0.0;
  admm_double2 d[kSymmLoads];
  symm_load(T, 0, 0, wave, lane, d);
#pragma unroll
  for (int hr = 0; hr < 2; ++hr) {
#pragma unroll
    for (int hc = 0; hc < 2; ++hc) {
      const bool above = diag && hr == 0 && hc == 1;  // wholly above the diagonal: neither loaded nor used
      __syncthreads();                                // (every wave is done with what the buffer held)
      if (!above) symm_stage(S, wave, lane, d);
      __syncthreads();
      if (hr == 0 && hc == 0) {  // the next quadrant's loads ahead of this one's arithmetic
        if (!diag) symm_load(T, 0, 1, wave, lane, d);
        else symm_load(T, 1, 0, wave, lane, d);
      } else if (hr == 0 && hc == 1) {
        if (!diag) symm_load(T, 1, 0, wave, lane, d);  // (a diagonal tile has it already)
      } else if (hr == 1 && hc == 0) {
        symm_load(T, 1, 1, wave, lane, d);
      }
      if (above) continue;
      const int64_t r0 = row0 + hr * kSub, c0 = col0 + hc * kSub;
      if (!tpart) symm_quadrant<true>(diag && hr == hc, S, lane, Yc, n, c0, ib, acc[0]);
      else symm_quadrant<false>(diag && hr == hc, S, lane, Yc, n, r0, ib, acc[hc]);
    }
    // the two halves of a sum meet in the staging buffer, first half + second half: the N-part's rows of this tile half
    // now, and behind the last quadrant the T-part's columns as well
    __syncthreads();
    if (ib != 0) {
      if (!tpart) {
#pragma unroll
        for (int k = 0; k < KC; ++k) S[lane * KC + k] = acc[0][k];
      } else if (hr == 1) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          S[(kWave + lane) * KC + k] = acc[0][k];
          S[(2 * kWave + lane) * KC + k] = acc[1][k];
        }
      }
    }
    __syncthreads();
    if (ib == 0 && !tpart) {
#pragma unroll
      for (int k = 0; k < KC; ++k) acc[0][k] += S[lane * KC + k];
      symm_store_row(pc + (static_cast<int64_t>(bj) * npad + row0 + hr * kSub + lane) * KC, acc[0]);
    }
    if (!tpart) {
#pragma unroll
      for (int k = 0; k < KC; ++k) acc[0][k] = 0.0;
    }
  }
  if (ib == 0 && tpart) {
#pragma unroll
    for (int hc = 0; hc < 2; ++hc) {
#pragma unroll
      for (int k = 0; k < KC; ++k) acc[hc][k] += S[((1 + hc) * kWave + lane) * KC + k];
      symm_store_row(pc + (static_cast<int64_t>(bi + 1) * npad + col0 + hc * kSub + lane) * KC, acc[hc]);
    }
  }
}

// X[chunk][i][k] = sum_{p = 0 .. ntile} part[chunk][p][i][k], one thread per stored value, eight loads in flight and
// the additions in the order of p
__global__ __launch_bounds__(kBlock) void symm_reduce_kernel(const double* __restrict__ part, int64_t n, int64_t npad,
                                                             int32_t ntile, double* __restrict__ X,
                                                             const MultiRec* __restrict__ rec, int32_t K) {
  const int64_t chunk = blockIdx.y;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n * KC) return;
  const int64_t fit = chunk * KC + e % KC;
  if (fit >= K || (rec && rec[fit].stop != 0)) return;  // a stopped fit keeps its column bit for bit
  const int64_t stride = npad * KC;
  const double* __restrict__ src = part + chunk * (ntile + 1) * stride + e;
  const int32_t np = ntile + 1;
  double s = 0.0;
  int32_t p = 0;
  for (; p + 8 <= np; p += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = src[(p + q) * stride];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  for (; p < np; ++p) s += src[p * stride];
  X[chunk * n * KC + e] = s;
}

}  // namespace

size_t symm_part_elems(const SymvPlan& p, int32_t K) {
  return static_cast<size_t>(spmm_chunks(K)) * (p.ntile + 1) * p.npad * KC;
}

void launch_symm_packed(const SymvPlan& p, const double* P, const double* Y, double* X, double* part,
                        const MultiRec* rec, int32_t K, hipStream_t stream) {
  const unsigned chunks = static_cast<unsigned>(spmm_chunks(K));
  hipLaunchKernelGGL(symm_packed_kernel, dim3(static_cast<unsigned>(symv_tiles(p)), chunks), dim3(kSymmWaves * kWave), 0,
                     stream, P, p.n, p.npad, p.ntile, Y, part, rec, K);
  hipLaunchKernelGGL(symm_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(p.n * KC, kBlock)), chunks), dim3(kBlock),
                     0, stream, part, p.n, p.npad, p.ntile, X, rec, K);
}

}  // namespace admm
