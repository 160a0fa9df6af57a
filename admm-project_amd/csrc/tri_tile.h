// tri_tile.h -- device helpers of the kernels that walk 128 x 128 tiles of a tile-packed triangle (symv.hip, trsv.hip):
// the tile numbering, the N-part column panel (lane owns a row pair, the input broadcast by v_readlane) and the T-part
// tile pass (column sums by the reduce-scatter of wave_reduce.h).  Also the one double2_t of the library.
#pragma once
#include "wave_reduce.h"

namespace admm {

typedef double double2_t __attribute__((ext_vector_type(2)));

constexpr int kTile = 128;  // rows per wave (64 lanes x 2) = columns per tile

// tile t of the lower triangle in row-major order (0,0), (1,0), (1,1), (2,0), ... -> (bi, bj)
__host__ __device__ __forceinline__ void tri_decode(unsigned t, unsigned& bi, unsigned& bj) {
  unsigned r = static_cast<unsigned>((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1u) / 2u > t) --r;
  while ((r + 1u) * (r + 2u) / 2u <= t) ++r;
  bi = r;
  bj = t - r * (r + 1u) / 2u;
}

// ---------------------------------------------------------------- compact storage of a symmetric tile-packed triangle
// (symv.hip: the cached explicit inverse of the streamed x-solve).  Same tiles in the same order; a DIAGONAL tile keeps
// its fp64 layout (128 KB: its diagonal entries are hundreds of times larger than the rest of the tile), an OFF-DIAGONAL
// tile t is BITS-bit signed fixed point with one power-of-two scale per tile, BITS = 48 (96 KB), 40 (80 KB), 38 (76 KB)
// or 36 (72 KB):
//   e = binary exponent of the tile's largest magnitude (max < 2^e),  scale_t = 2^(e - (BITS - 1))   (all-zero tile: 0)
//   q = rint(M / scale_t) clamped to +-(2^(BITS-1) - 1),  q = hi * 2^32 + lo,  hi signed BITS - 32 bits, lo unsigned 32
// A tile is 32 panel records, record p = columns 4p .. 4p + 3 as three runs, one piece per lane in each:
//   run 0 (1 KB, 16 bytes per lane): lo of (r, 4p), (r + 1, 4p), (r, 4p + 1), (r + 1, 4p + 1)   r = 2 * lane, the row pair
//   run 1 (1 KB): the same of columns 4p + 2, 4p + 3
//   run 2: the lane's eight hi fields in the order (r, 4p), (r + 1, 4p), (r, 4p + 1), ... (r + 1, 4p + 3), lowest bits
//          first, BITS - 32 bytes per lane -- 48 bit: 16 bytes, dword k = column 4p + k;  40 bit: 8 bytes, one byte per
//          field;  36 bit: one dword, a nibble per field;  38 bit: 48 bits, stored as a dword run (bits 0 .. 31, 256 B)
//          followed by a 16-bit run (bits 32 .. 47, 128 B) -- field 5 has its low two bits in the dword and its high
//          four in the halfword
// so every lane load is aligned to its size and a wave reads one contiguous record (3 KB / 2.5 KB / 2.375 KB / 2.25 KB)
// per panel.  Tile offsets count in units of 32 / 16 / 4 / 8 KB -- a diagonal tile is 4 / 8 / 32 / 16 of them, a compact
// one 3 / 5 / 19 / 9 -- and the rows before tile (bi, bj) hold bi diagonal tiles, so tile t starts at
// (3 t + bi) * 32 KB / (5 t + 3 bi) * 16 KB / (19 t + 13 bi) * 4 KB / (9 t + 7 bi) * 8 KB.  The scales are one
// double per tile (diagonal tiles: 1, unused) in an array of their own.  The kernel decodes fma(cvt(hi), 2^32, cvt(lo))
// -- exact, BITS bits fit the mantissa -- and applies the scale once per tile (sy_tile_cq): the product over the
// quantised matrix rounds exactly where the fp64 kernel's does.
template <int BITS>
struct CqFormat {
  static_assert(BITS == 36 || BITS == 38 || BITS == 40 || BITS == 48, "compact tile widths");
  static constexpr int kHiBits = BITS - 32;                      // one hi field
  static constexpr int kHiDwords = (8 * kHiBits + 31) / 32;      // run 2 per lane, as the kernel holds it
  static constexpr int kPanelBytes = 2048 + 64 * kHiBits;        // one panel record (run 2: kHiBits bytes per lane)
  // tile offsets count in these
  static constexpr int64_t kUnit = BITS == 48 ? 32768 : BITS == 40 ? 16384 : BITS == 38 ? 4096 : 8192;
  static constexpr int kTileUnits = (kTile / 4) * kPanelBytes / kUnit;  // 3 / 5 / 19 / 9: a tile is its 32 panel records
  static constexpr int kDiagUnits = 8 * kTile * kTile / kUnit;          // 4 / 8 / 32 / 16
  static_assert(kTileUnits * kUnit == (kTile / 4) * kPanelBytes && kTileUnits * kUnit * 8 == int64_t{BITS} * kTile * kTile,
                "whole units");
};
template <int BITS>
__host__ __device__ __forceinline__ int64_t cq_tile_offset(unsigned t, unsigned bi) {
  typedef CqFormat<BITS> F;
  return (int64_t{F::kTileUnits} * t + int64_t{F::kDiagUnits - F::kTileUnits} * bi) * F::kUnit;
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

// one panel buffer of the ring in sy_tile: the fp64 form holds the panel itself, the compact form its BITS bytes per lane
template <bool NT>
struct SyBuf64 {
  double2_t d[kSyPanel];
  __device__ __forceinline__ void load(const SyLane& s, int64_t cp) { sy_load<NT>(s, cp, d); }
  __device__ __forceinline__ void get(double2_t (&o)[kSyPanel]) const {
#pragma unroll
    for (int k = 0; k < kSyPanel; ++k) o[k] = d[k];
  }
};

typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
template <int N>
using uintn_t = unsigned __attribute__((ext_vector_type(N)));
template <bool NT, int N>
__device__ __forceinline__ uintn_t<N> loadn(const char* p) {  // N dwords, aligned to their size
  const uintn_t<N>* q = reinterpret_cast<const uintn_t<N>*>(p);
  return NT ? __builtin_nontemporal_load(q) : *q;
}
__device__ __forceinline__ double cq_value(unsigned lo, int hi) {
  return __builtin_fma(static_cast<double>(hi), 4294967296.0, static_cast<double>(lo));
}
// s.M: the compact tile; cp: first column of the panel within the tile (a multiple of 4)
template <bool NT, int BITS>
struct SyBufCq {
  typedef CqFormat<BITS> F;
  uint4_t lo[2];
  uintn_t<F::kHiDwords> hi;
  __device__ __forceinline__ void load(const SyLane& s, int64_t cp) {
    const char* p = reinterpret_cast<const char*>(s.M) + (cp >> 2) * F::kPanelBytes;
    lo[0] = loadn<NT, 4>(p + s.r * 8);
    lo[1] = loadn<NT, 4>(p + 1024 + s.r * 8);
    if constexpr (BITS == 38) {  // 48 bits per lane: the dword run, then the 16-bit run
      hi[0] = loadn<NT, 1>(p + 2048 + s.r * 2)[0];
      const unsigned short* q = reinterpret_cast<const unsigned short*>(p + 2304 + s.r);
      hi[1] = NT ? __builtin_nontemporal_load(q) : *q;
    } else {
      hi = loadn<NT, F::kHiDwords>(p + 2048 + s.r * (2 * F::kHiDwords));
    }
  }
  // hi field i of the lane (i = 2 k: row r of column k, 2 k + 1: row r + 1), sign-extended
  __device__ __forceinline__ int hi_field(int i) const {
    const int bit = i * F::kHiBits;
    if (bit % 32 + F::kHiBits > 32) {  // (38 bit, field 5) the field straddles two dwords
      const unsigned v = (hi[bit / 32] >> (bit % 32)) | (hi[bit / 32 + 1] << (32 - bit % 32));
      return static_cast<int>(v << (32 - F::kHiBits)) >> (32 - F::kHiBits);
    }
    return static_cast<int>(hi[bit / 32] << (32 - F::kHiBits - bit % 32)) >> (32 - F::kHiBits);
  }
  __device__ __forceinline__ void get(double2_t (&o)[kSyPanel]) const {
#pragma unroll
    for (int k = 0; k < kSyPanel; ++k) {
      o[k].x = cq_value(lo[k >> 1][2 * (k & 1)], hi_field(2 * k));
      o[k].y = cq_value(lo[k >> 1][2 * (k & 1) + 1], hi_field(2 * k + 1));
    }
  }
};

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
template <bool DIAG, class BUF, bool NP, bool TP, int NBUF>
__device__ __forceinline__ void sy_tile_ring(const SyLane& s, int64_t c0, double& n0, double& n1,
                                             double* __restrict__ tout, int lane) {
  constexpr int kPanels = kTile / kSyPanel, kFull = (kPanels / NBUF) * NBUF;
  static_assert(NBUF >= 2 && NBUF <= 8, "ring of panel buffers");
  BUF buf[NBUF];
  double2_t d[kSyPanel];
#pragma unroll
  for (int b = 0; b + 1 < NBUF; ++b) buf[b].load(s, c0 + b * kSyPanel);
#pragma unroll 1
  for (int g = 0; g < kFull; g += NBUF) {
#pragma unroll
    for (int b = 0; b < NBUF; ++b) {
      // panel g + b is consumed from buf[b]; the panel NBUF - 1 ahead goes into the buffer freed last
      const int nxt = g + b + NBUF - 1;
      if (kFull - NBUF + b + NBUF - 1 < kPanels || nxt < kPanels)  // (first test: compile time, true for every g)
        buf[(b + NBUF - 1) % NBUF].load(s, c0 + nxt * kSyPanel);
      buf[b].get(d);
      sy_compute<DIAG, NP, TP>(s, c0 + (g + b) * kSyPanel, d, n0, n1, tout, lane);
    }
  }
#pragma unroll
  for (int b = 0; b < kPanels - kFull; ++b) {  // the panels a ring that does not divide 32 leaves over
    if (kFull + b + NBUF - 1 < kPanels) buf[(b + NBUF - 1) % NBUF].load(s, c0 + (kFull + b + NBUF - 1) * kSyPanel);
    buf[b].get(d);
    sy_compute<DIAG, NP, TP>(s, c0 + (kFull + b) * kSyPanel, d, n0, n1, tout, lane);
  }
}

template <bool DIAG, bool NT, bool NP = true, bool TP = true, int NBUF = 2>
__device__ __forceinline__ void sy_tile(const SyLane& s, int64_t c0, double& n0, double& n1,
                                        double* __restrict__ tout, int lane) {
  sy_tile_ring<DIAG, SyBuf64<NT>, NP, TP, NBUF>(s, c0, n0, n1, tout, lane);
}

// an off-diagonal tile of the compact storage (s.M: the tile, c0 = 0).  scale: the tile's power of two, folded into the
// lane's x pair before the pass (T-part) and into the N accumulators after it -- four multiplications per tile, exact
template <bool NT, int BITS, int NBUF = 2>
__device__ __forceinline__ void sy_tile_cq(SyLane& s, double scale, double& n0, double& n1, double* __restrict__ tout,
                                           int lane) {
  s.xr0 *= scale;
  s.xr1 *= scale;
  sy_tile_ring<false, SyBufCq<NT, BITS>, true, true, NBUF>(s, 0, n0, n1, tout, lane);
  n0 *= scale;
  n1 *= scale;
}

}  // namespace admm
