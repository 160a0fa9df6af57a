// spmm.hip -- Y = M*X for a sparse M stored by rows and a chunked multi-vector X (spmm.h): spmv_kernel's lanes, order and
// butterfly with kSpmmChunk accumulators per lane, and the stand-alone operator admm_op_spmm.
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

template <int L, int KC, bool NT>
__global__ __launch_bounds__(kBlock) void spmm_kernel(int64_t rows, int64_t cols, const int64_t* __restrict__ start,
                                                      const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                      const double* __restrict__ X, double* __restrict__ Y, SpmmMask mk) {
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
  if (live && sub == 0) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if ((act >> c) & 1u) y[row * KC + c] = acc[c];
  }
}

template <int L>
void launch_l(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mk, hipStream_t stream) {
  const SpmvPlan& p = M.plan;
  const dim3 grid(static_cast<unsigned>(p.grid), static_cast<unsigned>(chunks));
  if (p.stream)
    hipLaunchKernelGGL((spmm_kernel<L, kSpmmChunk, true>), grid, dim3(kBlock), 0, stream, p.rows, p.cols, M.start, M.idx,
                       M.val, X, Y, mk);
  else
    hipLaunchKernelGGL((spmm_kernel<L, kSpmmChunk, false>), grid, dim3(kBlock), 0, stream, p.rows, p.cols, M.start, M.idx,
                       M.val, X, Y, mk);
}

}  // namespace

void launch_spmm(const SpmvMat& M, const double* X, double* Y, int32_t chunks, const SpmmMask& mask, hipStream_t stream) {
  switch (M.plan.lanes) {
    case 1: launch_l<1>(M, X, Y, chunks, mask, stream); break;
    case 2: launch_l<2>(M, X, Y, chunks, mask, stream); break;
    case 4: launch_l<4>(M, X, Y, chunks, mask, stream); break;
    case 8: launch_l<8>(M, X, Y, chunks, mask, stream); break;
    case 16: launch_l<16>(M, X, Y, chunks, mask, stream); break;
    case 32: launch_l<32>(M, X, Y, chunks, mask, stream); break;
    default: launch_l<64>(M, X, Y, chunks, mask, stream); break;
  }
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

extern "C" int admm_op_spmm(const admm_sparse_desc* D, int transpose, int K, const double* X, double* Y) {
  if (!D || !X || !Y) return fail(ADMM_E_INVALID, "spmm: NULL argument");
  if (K < 1) return fail(ADMM_E_INVALID, "spmm: K must be at least 1");
  if (D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, "spmm: the operator takes host arrays");
  ADMM_TRY(sparse_csc_check(D));
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
  if (err == hipSuccess) {
    SpmmMask mk;
    mk.K = K;
    launch_spmm(M, dx, dy, chunks, mk, nullptr);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(hy.data(), dy, sizeof(double) * ny, hipMemcpyDeviceToHost);
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  sparse_device_free(&sp);
  if (err != hipSuccess) return fail(ADMM_E_DEVICE, std::string("spmm: ") + hipGetErrorString(err));
  spmm_unpack(hy.data(), M.plan.rows, K, Y, M.plan.rows);
  return ADMM_OK;
}
