// kernels.h -- host-side launchers of the HIP kernels (all enqueue on `stream`, never sync).
#pragma once
#include <vector>

#include "common.h"

namespace admm {

// ---------------------------------------------------------------- GEMV (gemv.hip)
// Plan for y = D*x with column-chunk partials: ypart is [nchunk][ldy].
struct GemvNPlan {
  int64_t m, n, ld;
  int64_t ldy;          // >= m, row stride between chunk partials
  int32_t nchunk;       // number of column chunks (partials to sum)
  int64_t cols_per_chunk;
  size_t part_elems() const { return static_cast<size_t>(nchunk) * ldy; }
};
GemvNPlan gemv_n_plan(int64_t m, int64_t n, int64_t ld);
// ypart[c][i] = sum_{j in chunk c} D[i,j]*x[j]; x may be given as the sum alpha*(xa - xb) + xc
void launch_gemv_n(const GemvNPlan& p, const double* D, const double* x, double* ypart, const Ctrl* ctrl,
                   hipStream_t stream);
// y[i] = sum_c ypart[c][i]  (stand-alone reduce, used outside the fused consumers)
void launch_sum_partials(const double* part, int32_t nchunk, int64_t ld, int64_t len, double* y, const Ctrl* ctrl,
                         hipStream_t stream);

// Plan for G = D'*[v0 v1 v2] with row-chunk partials: gpart is [nchunk][nrhs][ldg].
struct GemvTPlan {
  int64_t m, n, ld;
  int64_t ldg;           // >= n
  int32_t nchunk;        // row chunks
  int32_t rows_per_chunk;
  size_t part_elems(int nrhs) const { return static_cast<size_t>(nchunk) * nrhs * ldg; }
};
GemvTPlan gemv_t_plan(int64_t m, int64_t n, int64_t ld);
void launch_gemv_t(const GemvTPlan& p, const double* D, const double* v0, const double* v1, const double* v2,
                   int nrhs, double* gpart, const Ctrl* ctrl, hipStream_t stream);
// g[r][j] = sum_c gpart[c][r][j]; g has row stride ldg_out
void launch_sum_partials_t(const GemvTPlan& p, const double* gpart, int nrhs, double* g, int64_t ldg_out,
                           const Ctrl* ctrl, hipStream_t stream);

// y = M*x for symmetric M from its lower triangle only (half the bytes of a full GEMV).
// M must be stored npad x npad (npad = round_up(n,128), ld >= npad) with zeros outside n x n.
struct SymvPlan {
  int64_t n, npad;
  int64_t ldp;     // row stride of the partial arrays (= npad)
  int32_t ntile;   // 128-row wave chunks = 128-column groups: npart and tpart are [ntile][ldp]
  bool packed;     // M is tile-packed (launch_symv_pack): lower-triangle 128x128 tiles back to back, ld unused
  int64_t ncached; // tiles (linear index < ncached) read with default loads; the rest stream non-temporally
  int32_t cbits;   // 36 / 38 / 40 / 48: packed, off-diagonal tiles as tile-scaled fixed point of that width
                   // (tri_tile.h), M is that storage; 0: fp64 tiles
  const double* scales;  // compact: one power of two per tile
  size_t npart_elems() const { return static_cast<size_t>(ntile) * ldp; }
  size_t tpart_elems() const { return static_cast<size_t>(ntile) * ldp; }
};
SymvPlan symv_plan(int64_t n);
// Share of a re-read symmetric matrix that can stay in the 256 MB Infinity Cache next to the rest of an iteration's
// traffic (measured plateau 105 .. 290 MB at n = 10000, dev/symv_packed.hip; the compact storage, 313 MB in all, has
// the same plateau: 49.8 us at 105 MB, 48.9 at 168, 48.3 .. 48.5 at 200 .. 232, 48.8 at 264, 56 at 290; the 40-bit store, 263 MB: 42.0 at 168, 41.5 at 232, 42.5 read
// with default loads throughout -- no cliff, and not measured inside the loop)
constexpr int64_t kSymvCacheBytes = int64_t{168} << 20;
int64_t symv_tiles(const SymvPlan& p);          // lower-triangle tiles
size_t symv_packed_elems(const SymvPlan& p);    // doubles of the tile-packed storage
int64_t symv_cached_tiles(const SymvPlan& p, int64_t budget_bytes);
// K tile-packed matrices of one plan in one launch (partial rows left unsummed): Ms_dev = device array of K pointers
// fin != null: workgroup (0, 0) runs the finalize logic of the previous iteration with these arguments
struct FinArgs;
void launch_symv_lower_batch(const SymvPlan& p, const double* const* Ms_dev, int32_t K, const double* x0, int64_t xstride,
                             double* npart0, double* tpart0, int64_t pstride, const Ctrl* ctrl, hipStream_t stream,
                             const FinArgs* fin = nullptr);
// P (symv_packed_elems doubles) <- the lower-triangle tiles of the padded column-major M (npad x npad, ld)
void launch_symv_pack(const SymvPlan& p, const double* M, int64_t ld, double* P, hipStream_t stream);
// The compact storage of a packed plan (tri_tile.h): diagonal tiles fp64, off-diagonal tiles p.cbits-bit fixed point with
// one power-of-two scale per tile, the scales behind the tiles in the same buffer of symv_compact_elems doubles.
// bytes of the leading t tiles in the plan's storage form (p.cbits); the plan's ncached counts tiles of that form
int64_t symv_tile_prefix_bytes(const SymvPlan& p, int64_t t);
bool symv_cbits_ok(int32_t bits);  // the widths of the format: a plan's cbits is 0 or one of these
size_t symv_compact_elems(const SymvPlan& p);
double* symv_compact_scales(const SymvPlan& p, double* C);
// C <- M, either the padded column-major square (ld) or the fp64 tile-packed triangle (src_packed); deq (optional,
// symv_packed_elems doubles): the fp64 tile-packed triangle of the matrix C stands for
void launch_symv_compact_pack(const SymvPlan& p, const double* M, int64_t ld, bool src_packed, double* C, double* deq,
                              hipStream_t stream);
// y = M*x for a small symmetric M (full storage, ld even, 16-byte aligned; x 16-byte aligned): one wave per column
void launch_symv_small(const double* M, int64_t n, int64_t ld, const double* x, double* y, const Ctrl* ctrl,
                       hipStream_t stream);
// part_rank / part_count: this launch processes every part_count-th lower-triangle tile (multi-GPU split of
// the x-solve); npart / tpart must have been zero-filled once, y is then this rank's PARTIAL result.
void launch_symv_lower(const SymvPlan& p, const double* M, int64_t ld, const double* x, double* npart, double* tpart,
                       double* y, const Ctrl* ctrl, hipStream_t stream, int part_rank = 0, int part_count = 1,
                       bool reduce = true);

// ---------------------------------------------------------------- symmetric M x a chunk of vectors (symm.hip)
// X(:, k) = M * Y(:, k) for every running fit k < K: M the fp64 tile-packed lower triangle of a packed plan (never the
// compact storage), X and Y multi-vectors of n rows in spmm.h's layout [chunks][n][kSpmmChunk], part the partial rows
// (symm_part_elems doubles; nothing in it has to be initialised).  rec: K records, or null when every fit runs; a fit
// whose stop word is set keeps its column of X, and a chunk without a running fit reads nothing.  One form for every n.
struct MultiRec;
size_t symm_part_elems(const SymvPlan& p, int32_t K);
void launch_symm_packed(const SymvPlan& p, const double* P, const double* Y, double* X, double* part,
                        const MultiRec* rec, int32_t K, hipStream_t stream);

// ---------------------------------------------------------------- dense setup (dense.hip)
// C = alpha*op(A)*op(B) + beta*C, column-major fp64 on the MFMA f64 path.  transA/transB: 0 = N, 1 = T.
// lower_only: compute only tiles that touch the lower triangle (SYRK-style symmetric results).
void launch_gemm(int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                 const double* B, int64_t ldb, double beta, double* C, int64_t ldc, bool lower_only,
                 hipStream_t stream);
// In-place blocked lower Cholesky; info (device int) gets the failing pivot (1-based) or 0.
// dinv (optional, [ceil(n/64)][64*64]) receives the inverted 64x64 diagonal blocks of the factor.
int cholesky_lower(double* A, int64_t n, int64_t lda, int32_t* info_dev, double* dinv, hipStream_t stream);
// invert the 64x64 diagonal blocks of an existing lower factor
void launch_trtri_diag(const double* L, int64_t n, int64_t ldl, double* dinv, hipStream_t stream);
// X = inv(L) (lower, upper part zero) from L and its inverted diagonal blocks
// clear = false: X (lower block and its upper-right scratch) is already zero
int trtri_lower_from_diag(const double* L, int64_t n, int64_t ldl, const double* dinv, double* X, int64_t ldx,
                          hipStream_t stream, bool clear = true);
// y = L (L' x), tmp: n doubles (setup-time probe of the x-solve forms)
void launch_llt_apply(const double* L, int64_t n, int64_t ld, const double* x, double* tmp, double* y,
                      hipStream_t stream);
// mirror the lower triangle into the upper one
void launch_symmetrize_lower(double* A, int64_t n, int64_t lda, hipStream_t stream);
void launch_add_diag(double* A, int64_t n, int64_t lda, double shift, hipStream_t stream);
void launch_fill(double* p, size_t n, double v, hipStream_t stream);

// ---------------------------------------------------------------- TRSV (trsv.hip)
// x = L' \ (L \ y) as blocked substitution over K coarse blocks whose diagonal-block inverses are folded
// into the panels (one bandwidth-bound launch per block and sweep).
struct TrsvPlan {
  int64_t n, npad;
  int64_t ldm, ldp;
  int32_t ntile, nblk, bt;   // 128-row tiles, coarse blocks, tiles per block
  double* Fm;                // forward panels  [inv(L_kk); -L_below,k inv(L_kk)]   (lower triangle, tile-packed)
  double* Um;                // backward panels [-L_k,above' inv(L_kk)'; inv(L_kk)'] (upper triangle, tile-packed)
  int64_t ncached;           // tiles of each triangle read with default loads (the rest stream non-temporally)
  double* P[2];              // [bt][npad] column-tile partials: the step in flight and the previous one
  double *v, *w;             // running right-hand sides (npad)
  bool streaming;            // non-temporal matrix loads (matrix larger than the caches)
  // one-block form (tri1_*): the whole factor as ONE pre-inverted block, X = inv(L) tile-packed, applied as
  // w = X y (N-part pass + fold) and x = X' w (T-part pass): 3 launches per pair.  When built, Fm / Um / P above
  // are absent (nblk = 1 and they would be the same matrix twice).
  bool one;
  double* X1;                // tile-packed lower triangle of inv(L)
  double *np1, *tp1;         // [ntile][ldp] partial rows of the forward / backward pass
  double* w1;                // [npad] forward result
};
// arguments of the one-block form's kernels
struct Tri1Args {
  const double* X;
  int64_t n;
  const double* y;           // forward input (n elements, 8-byte aligned)
  double* npart;
  double* tpart;
  double* w;
  int64_t ldp;
  uint32_t ncached;          // tiles with linear index < ncached are read with default loads (Infinity Cache share)
  uint32_t ntri;             // lower-triangle tiles
  int32_t ntile;
};
void launch_tri1_forward(const Tri1Args& a, const FinArgs* fin, bool fin_pending, const Ctrl* ctrl, hipStream_t stream);
void launch_tri1_backward(const Tri1Args& a, const Ctrl* ctrl, hipStream_t stream);
void launch_tri1_reduce(const Tri1Args& a, double* x, const Ctrl* ctrl, hipStream_t stream);
// y = the fixed-order sum of the partial rows a symv_lower_* launch of plan p left in npart / tpart
void launch_symv_reduce(const SymvPlan& p, const double* npart, const double* tpart, double* y, const Ctrl* ctrl,
                        hipStream_t stream);
Tri1Args tri1_args(const TrsvPlan& p, const double* y);
// both passes; x == nullptr leaves the backward pass's partial rows to the consumer (prox_fin_kernel)
void launch_tri1_pair(const TrsvPlan& p, const double* y, double* x, const FinArgs* fin, bool fin_pending,
                      const Ctrl* ctrl, hipStream_t stream);
// doubles the plan needs in one caller-owned device buffer
// form 0: blocked substitution over K = ceil(n / 2048) coarse blocks; 1: the one-block form (n >= 256, else blocked).
// trsv_resolve_form: `form` unless ADMM_TRSV_FORM=blocked|one says otherwise (tests, A/B measurements) -- consulted by
// the callers that have a choice (engine.hip: choose_trsv_form; ops.hip), never by trsv_build itself.
constexpr int kTrsvBlocked = 0, kTrsvOne = 1;
int trsv_resolve_form(int64_t n, int form);
size_t trsv_plan_elems(int64_t n, int form = kTrsvBlocked);
// dinv64: the inverted 64x64 diagonal blocks of L (cholesky_lower / launch_trtri_diag)
int trsv_build(const double* L, int64_t n, int64_t ldl, const double* dinv64, double* buf, TrsvPlan* plan,
               hipStream_t stream, int form = kTrsvBlocked);
void launch_trsv_pair(const TrsvPlan& p, const double* y, double* x, const Ctrl* ctrl, hipStream_t stream);
// P <- the ntri 128 x 128 tiles of a triangle of the padded column-major M (ld), back to back in row-major triangle
// order: tile t = (bi, bj), bi >= bj, is M's tile (bi, bj) (upper = 0) or (bj, bi) (upper = 1)
void launch_tri_pack(const double* M, int64_t ld, double* P, unsigned ntri, int upper, hipStream_t stream);

// ---------------------------------------------------------------- symmetric eigen-decomposition (jacobi.hip)
// W (n x n symmetric PSD, FULL storage) is overwritten by W*V; V gets the eigenvectors, lam_host the eigenvalues
// (paired with V's columns, unsorted).  lam_dev: n doubles, rot: one int32 (device scratch).
int jacobi_eig_psd(double* W, int64_t n, int64_t ldw, double* V, int64_t ldv, double* lam_dev, int32_t* rot,
                   std::vector<double>* lam_host, int* sweeps_out, hipStream_t stream);
void launch_scale_cols(double* V, int64_t ldv, int64_t n, const double* scale, hipStream_t stream);
// one-sided Jacobi one step at a time: V <- I; one round (n/2 disjoint column pairs of B and V rotated, `round` of the
// ne - 1 rounds of a sweep; rot counts the rotations; null2 = 0 rotates every non-zero column); lam[j] = ||B(:, j)||
void launch_jacobi_identity(double* V, int64_t ldv, int64_t n, hipStream_t stream);
void launch_jacobi_round(double* B, int64_t ldb, double* V, int64_t ldv, int64_t n, int32_t round, double tol,
                         double null2, int32_t* rot, hipStream_t stream);
void launch_jacobi_norms(const double* B, int64_t ldb, int64_t n, double* lam, hipStream_t stream);

}  // namespace admm
