// spmm.hip -- Y = M*X for a sparse M stored by rows and a chunked multi-vector X (spmm.h): spmv_kernel's lanes, order and
// butterfly with kSpmmChunk accumulators per lane, the row-weighted store of the forward product, and the
// stand-alone operators admm_op_spmm and admm_op_spmm_weighted.
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "spmm.h"
#include "wave_reduce.h"

namespace admm {

namespace {

// bit c: column blockIdx.y * KC + c exists and none of its flags is set (wave-uniform: scalar loads)
template <int KC>
__device__ __forceinline__ uint32_t live_columns(const SpmmMask& mk) {
  uint32_t act = 0;
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int32_t k = static_cast<int32_t>(blockIdx.y) * KC + c;
    const int32_t kc = k < mk.K ? k : mk.K - 1;
    bool on = k < mk.K;
    if (mk.flag_a) on = on && mk.flag_a[static_cast<int64_t>(kc) * mk.stride_a] == 0;
    if (mk.flag_b) on = on && mk.flag_b[static_cast<int64_t>(kc) * mk.stride_b] == 0;
    if (on) act |= 1u << c;
  }
  return __builtin_amdgcn_readfirstlane(act);
}

// per column of the chunk the fold it holds out (wave-uniform, as live_columns reads its flags: scalar loads)
template <int KC>
__device__ __forceinline__ void held_folds(const SpmmRowWeights& rw, int32_t (&hk)[KC]) {
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int32_t k = static_cast<int32_t>(blockIdx.y) * KC + c;
    hk[c] = __builtin_amdgcn_readfirstlane(rw.held[k < rw.K ? k : rw.K - 1]);
  }
}

struct SpmmNoRowWeights {};  // the argument of the RW = false instantiations: nothing is passed, nothing is read

// RW: the row-weighted store of launch_spmm_weighted.  It is a template parameter as SHIFT is in spmm_cg.hip: without it
// the epilogue is the plain store and the kernel is the one it was.
template <int L, int KC, bool NT, bool RW = false>
__global__ __launch_bounds__(kBlock) void spmm_kernel(int64_t rows, int64_t cols, const int64_t* __restrict__ start,
                                                      const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                      const double* __restrict__ X, double* __restrict__ Y, SpmmMask mk,
                                                      std::conditional_t<RW, SpmmRowWeights, SpmmNoRowWeights> rw) {
  static_assert(KC % 2 == 0, "a row of X is read as 16-byte pairs");
  const uint32_t act = live_columns<KC>(mk);
  if (act == 0) return;
  constexpr int kRows = kBlock / L;  // rows of a workgroup
  const double* __restrict__ x = X + static_cast<int64_t>(blockIdx.y) * cols * KC;
  double* __restrict__ y = Y + static_cast<int64_t>(blockIdx.y) * rows * KC;
  const int sub = threadIdx.x % L;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRows + threadIdx.x / L;
  const bool live = row < rows;
  double acc[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) acc[c] = 0.0;
  if (live) {
    const int64_t end = start[row + 1];
    int64_t k = start[row] + sub;
    // as spmv_kernel: two products' loads in flight; the additions of every column keep the order k, k + L, k + 2L, ...
    for (; k + L < end; k += 2 * L) {
      const int32_t c0 = NT ? __builtin_nontemporal_load(idx + k) : idx[k];
      const int32_t c1 = NT ? __builtin_nontemporal_load(idx + k + L) : idx[k + L];
      const double v0 = load1<NT>(val + k), v1 = load1<NT>(val + k + L);
      admm_double2 x0[KC / 2], x1[KC / 2];
#pragma unroll
      for (int c = 0; c < KC / 2; ++c) {
        x0[c] = load2<false>(x + static_cast<int64_t>(c0) * KC + 2 * c);
        x1[c] = load2<false>(x + static_cast<int64_t>(c1) * KC + 2 * c);
      }
#pragma unroll
      for (int c = 0; c < KC / 2; ++c) {
        acc[2 * c] += v0 * x0[c].x;
        acc[2 * c] += v1 * x1[c].x;
        acc[2 * c + 1] += v0 * x0[c].y;
        acc[2 * c + 1] += v1 * x1[c].y;
      }
    }
    if (k < end) {
      const int32_t c0 = NT ? __builtin_nontemporal_load(idx + k) : idx[k];
      const double v0 = load1<NT>(val + k);
#pragma unroll
      for (int c = 0; c < KC / 2; ++c) {
        const admm_double2 x0 = load2<false>(x + static_cast<int64_t>(c0) * KC + 2 * c);
        acc[2 * c] += v0 * x0.x;
        acc[2 * c + 1] += v0 * x0.y;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < KC; ++c) acc[c] = group_sum<L>(acc[c]);  // outside the branch: the cross-lane moves need the whole wave
  if constexpr (RW) {
    int32_t hk[KC];
    held_folds<KC>(rw, hk);
    if (live && sub == 0) {
      const int32_t f = rw.fold ? rw.fold[row] : -2;  // (-2: no column holds it out)
      if (rw.obsw) {
        const double w = rw.obsw[row];
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if ((act >> c) & 1u) y[row * KC + c] = hk[c] == f ? 0.0 : acc[c] * w;
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if ((act >> c) & 1u) y[row * KC + c] = hk[c] == f ? 0.0 : acc[c];
      }
    }
  } else {
    if (live && sub == 0) {
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if ((act >> c) & 1u) y[row * KC + c] = acc[c];
    }
  }
}

template <int L, bool RW, class RowW>
void launch_l(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mk, const RowW& rw,
              hipStream_t stream) {
  const SpmvPlan& p = M.plan;
  const dim3 grid(static_cast<unsigned>(p.grid), static_cast<unsigned>(chunks));
  if (p.stream)
    hipLaunchKernelGGL((spmm_kernel<L, kSpmmChunk, true, RW>), grid, dim3(kBlock), 0, stream, p.rows, p.cols, M.start,
                       M.idx, M.val, X, Y, mk, rw);
  else
    hipLaunchKernelGGL((spmm_kernel<L, kSpmmChunk, false, RW>), grid, dim3(kBlock), 0, stream, p.rows, p.cols, M.start,
                       M.idx, M.val, X, Y, mk, rw);
}

template <bool RW, class RowW>
void launch_lanes(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask, const RowW& rw,
                  hipStream_t stream) {
  switch (M.plan.lanes) {
    case 1: launch_l<1, RW>(M, X, Y, chunks, mask, rw, stream); break;
    case 2: launch_l<2, RW>(M, X, Y, chunks, mask, rw, stream); break;
    case 4: launch_l<4, RW>(M, X, Y, chunks, mask, rw, stream); break;
    case 8: launch_l<8, RW>(M, X, Y, chunks, mask, rw, stream); break;
    case 16: launch_l<16, RW>(M, X, Y, chunks, mask, rw, stream); break;
    case 32: launch_l<32, RW>(M, X, Y, chunks, mask, rw, stream); break;
    default: launch_l<64, RW>(M, X, Y, chunks, mask, rw, stream); break;
  }
}

}  // namespace

void launch_spmm(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask, hipStream_t stream) {
  launch_lanes<false>(M, X, Y, chunks, mask, SpmmNoRowWeights{}, stream);
}

void launch_spmm_weighted(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask,
                          const SpmmRowWeights& roww, hipStream_t stream) {
  launch_lanes<true>(M, X, Y, chunks, mask, roww, stream);
}

int check_observations(int64_t rows, int32_t K, const double* obsweights, int32_t nfolds, const int32_t* fold,
                       const int32_t* heldout) {
  if (obsweights)
    for (int64_t i = 0; i < rows; ++i)
      if (!finite_nonneg(obsweights[i]))
        return fail(ADMM_E_INVALID, "observations: weight " + std::to_string(i) + " is negative or not finite");
  if (heldout && !fold) return fail(ADMM_E_INVALID, "observations: heldout needs the fold ids (fold is NULL)");
  if (fold) {
    if (nfolds < 1) return fail(ADMM_E_INVALID, "observations: nfolds must be at least 1 when fold is given");
    for (int64_t i = 0; i < rows; ++i)
      if (fold[i] < 0 || fold[i] >= nfolds)
        return fail(ADMM_E_INVALID, "observations: the fold id of row " + std::to_string(i) + " is outside [0, nfolds)");
    for (int32_t k = 0; heldout && k < K; ++k)
      if (heldout[k] < -1 || heldout[k] >= nfolds)
        return fail(ADMM_E_INVALID, "observations: heldout of fit " + std::to_string(k) + " is outside [-1, nfolds)");
  }
  return ADMM_OK;
}

void spmm_pack(const double* src, int64_t ld, int64_t len, int32_t K, double* dst) {
  const int32_t chunks = spmm_chunks(K);
  std::memset(dst, 0, sizeof(double) * static_cast<size_t>(chunks) * len * kSpmmChunk);
  for (int32_t k = 0; k < K; ++k) {
    double* d = dst + static_cast<int64_t>(k / kSpmmChunk) * len * kSpmmChunk + k % kSpmmChunk;
    const double* s = src + static_cast<int64_t>(k) * ld;
    for (int64_t i = 0; i < len; ++i) d[i * kSpmmChunk] = s[i];
  }
}

void spmm_unpack(const double* src, int64_t len, int32_t K, double* dst, int64_t ld) {
  for (int32_t k = 0; k < K; ++k) {
    const double* s = src + static_cast<int64_t>(k / kSpmmChunk) * len * kSpmmChunk + k % kSpmmChunk;
    double* d = dst + static_cast<int64_t>(k) * ld;
    for (int64_t i = 0; i < len; ++i) d[i] = s[i * kSpmmChunk];
  }
}

}  // namespace admm

using namespace admm;

namespace {

// the body of both operators behind their checks; fold / heldout / obsweights all null: the plain product
int op_spmm_run(const admm_sparse_desc* D, int transpose, int K, const double* X, double* Y, const double* obsweights,
                const int32_t* fold, const int32_t* heldout, bool weighted) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  SparseDev sp;
  int rc = sparse_device_build(D, &sp, nullptr);
  if (rc != ADMM_OK) {
    sparse_device_free(&sp);
    return rc;
  }
  const SpmvMat& M = transpose ? sp.t : sp.n;
  const int32_t chunks = spmm_chunks(K);
  const size_t nx = static_cast<size_t>(chunks) * M.plan.cols * kSpmmChunk, ny = static_cast<size_t>(chunks) * M.plan.rows * kSpmmChunk;
  std::vector<double> hx(nx), hy(ny);
  spmm_pack(X, M.plan.cols, M.plan.cols, K, hx.data());
  double *dx = nullptr, *dy = nullptr;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&dx), sizeof(double) * nx);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&dy), sizeof(double) * ny);
  if (err == hipSuccess) err = hipMemcpy(dx, hx.data(), sizeof(double) * nx, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemset(dy, 0xff, sizeof(double) * ny);  // (NaN: a row that is not stored shows)
  const int64_t rows = M.plan.rows;
  double* dw = nullptr;
  int32_t *df = nullptr, *dh = nullptr;
  SpmmRowWeights rw;
  rw.K = K;
  if (weighted) {  // the three arrays as the object keeps them: held always there, -1 where nothing is held out
    std::vector<int32_t> hh(static_cast<size_t>(K), -1);
    for (int k = 0; heldout && k < K; ++k) hh[k] = heldout[k];
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&dh), sizeof(int32_t) * K);
    if (err == hipSuccess) err = hipMemcpy(dh, hh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice);
    if (err == hipSuccess && fold) err = hipMalloc(reinterpret_cast<void**>(&df), sizeof(int32_t) * rows);
    if (err == hipSuccess && fold) err = hipMemcpy(df, fold, sizeof(int32_t) * rows, hipMemcpyHostToDevice);
    if (err == hipSuccess && obsweights) err = hipMalloc(reinterpret_cast<void**>(&dw), sizeof(double) * rows);
    if (err == hipSuccess && obsweights) err = hipMemcpy(dw, obsweights, sizeof(double) * rows, hipMemcpyHostToDevice);
    rw.obsw = dw;
    rw.fold = df;
    rw.held = dh;
    // the columns past K of the last chunk start at +0.0, as a solver's buffers do: the check below proves they stay
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t e = 0; e < ny; ++e)
      hy[e] = static_cast<int32_t>(e / (static_cast<size_t>(rows) * kSpmmChunk)) * kSpmmChunk +
                          static_cast<int32_t>(e % kSpmmChunk) < K ? nan : 0.0;
    if (err == hipSuccess) err = hipMemcpy(dy, hy.data(), sizeof(double) * ny, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess) {
    SpmmMask mk;
    mk.K = K;
    if (weighted) launch_spmm_weighted(M, dx, dy, chunks, mk, rw, nullptr);
    else launch_spmm(M, dx, dy, chunks, mk, nullptr);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(hy.data(), dy, sizeof(double) * ny, hipMemcpyDeviceToHost);
  for (void* p : {static_cast<void*>(dx), static_cast<void*>(dy), static_cast<void*>(dw), static_cast<void*>(df),
                  static_cast<void*>(dh)})
    if (p) (void)hipFree(p);
  sparse_device_free(&sp);
  if (err != hipSuccess) return fail(ADMM_E_DEVICE, std::string("spmm: ") + hipGetErrorString(err));
  spmm_unpack(hy.data(), rows, K, Y, rows);
  if (weighted)  // the columns past K of the last chunk: +0.0 before the launch, and no lane may store there
    for (int32_t k = K; k < chunks * kSpmmChunk; ++k)
      for (int64_t i = 0; i < rows; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &hy[static_cast<size_t>(k / kSpmmChunk) * rows * kSpmmChunk + i * kSpmmChunk + k % kSpmmChunk],
                    sizeof(bits));
        if (bits != 0)
          return fail(ADMM_E_NUMERIC, "spmm_weighted: padding column " + std::to_string(k) + " is no longer 0.0 at row " +
                                          std::to_string(i));
      }
  return ADMM_OK;
}

}  // namespace

extern "C" int admm_op_spmm(const admm_sparse_desc* D, int transpose, int K, const double* X, double* Y) {
  if (!D || !X || !Y) return fail(ADMM_E_INVALID, "spmm: NULL argument");
  if (K < 1) return fail(ADMM_E_INVALID, "spmm: K must be at least 1");
  if (D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, "spmm: the operator takes host arrays");
  ADMM_TRY(sparse_csc_check(D));
  return op_spmm_run(D, transpose, K, X, Y, nullptr, nullptr, nullptr, false);
}

extern "C" int admm_op_spmm_weighted(const admm_sparse_desc* D, int32_t K, const double* X, const double* obsweights,
                                     int32_t nfolds, const int32_t* fold, const int32_t* heldout, double* Y) {
  if (!D || !X || !Y) return fail(ADMM_E_INVALID, "spmm_weighted: NULL argument");
  if (K < 1) return fail(ADMM_E_INVALID, "spmm_weighted: K must be at least 1");
  if (D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, "spmm_weighted: the operator takes host arrays");
  ADMM_TRY(sparse_csc_check(D));
  ADMM_TRY(check_observations(D->rows, K, obsweights, nfolds, fold, heldout));
  return op_spmm_run(D, 0, K, X, Y, obsweights, fold, heldout, true);
}
