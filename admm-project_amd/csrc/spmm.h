// spmm.h -- Y = M*X for a sparse M stored by rows (spmv.h) and a multi-vector X of kSpmmChunk columns per chunk: the two
// products of the one-vs-rest linear SVM on a sparse design matrix.  One read of the 12 B per nonzero
// serves every column of a chunk.
// Layout: a multi-vector of `len` rows is stored chunk by chunk, [chunks][len][kSpmmChunk]: the kSpmmChunk values of one
// row are contiguous (leading dimension kSpmmChunk), so the gather for one nonzero is one contiguous 80-byte read.
// Column k lives in chunk k / kSpmmChunk at offset k % kSpmmChunk; the columns past K of the last chunk are zero.
#pragma once
#include "spmv.h"

namespace admm {

constexpr int kSpmmChunk = 10;  // columns one pass over M serves: 10 accumulators and two rows of X in flight take 68 VGPRs
                                // and no scratch; even, so that a row of X is a whole number of 16-byte loads

// which columns a launch computes and stores: column k < K is live unless one of its two flag words is nonzero.  A flag
// array is addressed as flag[k * stride] (stride in 32-bit words: the flags sit inside per-column records); null = no flag.
// A workgroup whose chunk has no live column returns at once.
struct SpmmMask {
  const int32_t* flag_a = nullptr;
  int32_t stride_a = 0;
  const int32_t* flag_b = nullptr;
  int32_t stride_b = 0;
  int32_t K = 0;
};

// Y[chunks][rows][kSpmmChunk] = M * X[chunks][cols][kSpmmChunk].  The lane layout, the per-lane order of the products and
// the in-wave butterfly are those of launch_spmv, once per accumulator: column k of Y has the bits launch_spmv gives for
// column k alone.  An empty row stores +0.0.  No LDS, no atomics.
void launch_spmm(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask, hipStream_t stream);

// row weights of a forward product, one operator per column: column k stores omega_ik * (M X)_ik with
// omega_ik = obsw_i * [fold_i != held_k].  obsw null: 1; fold null: no row is held out; held_k = -1: column k holds
// nothing out.  All three live on the device.
struct SpmmRowWeights {
  const double* obsw = nullptr;   // rows shared observation weights >= 0
  const int32_t* fold = nullptr;  // rows fold ids >= 0
  const int32_t* held = nullptr;  // K values: the fold column k holds out, or -1 (never null)
  int32_t K = 0;
};

// launch_spmm with the row-weighted store: the lane that stores row i writes, per live column k, +0.0 where
// held[k] == fold[i] (a select: whatever the accumulator holds, NaN included) and otherwise acc * obsw[i] (one rounding
// on top of launch_spmm's bits), or acc itself without obsw.  4 B (+ 8 B with obsw) more per row read; no LDS, no atomics.
void launch_spmm_weighted(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask,
                          const SpmmRowWeights& roww, hipStream_t stream);

// what admm_sparse_lasso_set_observations and admm_op_spmm_weighted refuse, in the same words (ADMM_E_INVALID; host
// arrays, rows and K the sizes): a negative or non-finite weight (its index named), nfolds < 1 with fold given, a fold id
// outside [0, nfolds) (its row named), a heldout outside [-1, nfolds) (its fit named), heldout without fold
int check_observations(int64_t rows, int32_t K, const double* obsweights, int32_t nfolds, const int32_t* fold,
                       const int32_t* heldout);

// host <-> device layout: column-major src (ld x K) into [chunks][len][kSpmmChunk] (padding columns zero) and back
void spmm_pack(const double* src, int64_t ld, int64_t len, int32_t K, double* dst);
void spmm_unpack(const double* src, int64_t len, int32_t K, double* dst, int64_t ld);
inline int32_t spmm_chunks(int32_t K) { return (K + kSpmmChunk - 1) / kSpmmChunk; }

}  // namespace admm
