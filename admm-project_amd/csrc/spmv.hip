// spmv.hip -- y = M*x for a sparse M stored by rows (spmv.h): the two products of the matrix-free lasso x-update on a
// sparse design matrix, the host checks of the caller's CSC arrays, the one-time transpose, and the
// stand-alone operator admm_op_spmv.
#include <cmath>

#include "spmv.h"
#include "wave_reduce.h"

namespace admm {

namespace {

template <int L, bool NT>
__global__ __launch_bounds__(kBlock) void spmv_kernel(int64_t rows, const int64_t* __restrict__ start,
                                                      const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                      const double* __restrict__ x, double* __restrict__ y,
                                                      const Ctrl* __restrict__ ctrl) {
  if (ctrl && ctrl->stop) return;
  constexpr int kRows = kBlock / L;  // rows of a workgroup
  const int sub = threadIdx.x % L;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kRows + threadIdx.x / L;
  const bool live = row < rows;
  double acc = 0.0;
  if (live) {
    const int64_t end = start[row + 1];
    int64_t k = start[row] + sub;
    // two products' loads in flight; the additions keep the order k, k + L, k + 2L, ...
    for (; k + L < end; k += 2 * L) {
      const int32_t c0 = NT ? __builtin_nontemporal_load(idx + k) : idx[k];
      const int32_t c1 = NT ? __builtin_nontemporal_load(idx + k + L) : idx[k + L];
      const double v0 = load1<NT>(val + k), v1 = load1<NT>(val + k + L);
      const double x0 = x[c0], x1 = x[c1];
      acc += v0 * x0;
      acc += v1 * x1;
    }
    if (k < end) {
      const int32_t c0 = NT ? __builtin_nontemporal_load(idx + k) : idx[k];
      acc += load1<NT>(val + k) * x[c0];
    }
  }
  acc = group_sum<L>(acc);  // outside the branch: the cross-lane moves need the whole wave
  if (live && sub == 0) y[row] = acc;
}

template <int L>
void launch_l(const SpmvMat& M, const double* x, double* y, const Ctrl* ctrl, hipStream_t stream) {
  const SpmvPlan& p = M.plan;
  if (p.stream)
    hipLaunchKernelGGL((spmv_kernel<L, true>), dim3(p.grid), dim3(kBlock), 0, stream, p.rows, M.start, M.idx, M.val, x,
                       y, ctrl);
  else
    hipLaunchKernelGGL((spmv_kernel<L, false>), dim3(p.grid), dim3(kBlock), 0, stream, p.rows, M.start, M.idx, M.val, x,
                       y, ctrl);
}

constexpr int64_t kIndexLimit = int64_t{1} << 31;

}  // namespace

SpmvPlan spmv_plan(int64_t rows, int64_t cols, int64_t nnz, int64_t resident_bytes) {
  SpmvPlan p;
  p.rows = rows;
  p.cols = cols;
  p.nnz = nnz;
  const int64_t mean = rows > 0 ? ceil_div(nnz, rows) : 0;
  int32_t lanes = 1;
  while (lanes < kWave && lanes < mean) lanes *= 2;
  p.lanes = lanes;
  p.grid = static_cast<int32_t>(ceil_div(rows > 0 ? rows : 1, static_cast<int64_t>(kBlock / lanes)));
  p.stream = stream_hint(resident_bytes);
  return p;
}

void launch_spmv(const SpmvMat& M, const double* x, double* y, const Ctrl* ctrl, hipStream_t stream) {
  switch (M.plan.lanes) {
    case 1: launch_l<1>(M, x, y, ctrl, stream); break;
    case 2: launch_l<2>(M, x, y, ctrl, stream); break;
    case 4: launch_l<4>(M, x, y, ctrl, stream); break;
    case 8: launch_l<8>(M, x, y, ctrl, stream); break;
    case 16: launch_l<16>(M, x, y, ctrl, stream); break;
    case 32: launch_l<32>(M, x, y, ctrl, stream); break;
    default: launch_l<64>(M, x, y, ctrl, stream); break;
  }
}

int sparse_csc_check(const admm_sparse_desc* D) {
  if (!D) return fail(ADMM_E_INVALID, "sparse matrix: the description is NULL");
  if (D->struct_size != static_cast<int32_t>(sizeof(admm_sparse_desc)))
    return fail(ADMM_E_INVALID, "admm_sparse_desc.struct_size mismatch (ABI version skew)");
  if (D->rows < 1 || D->cols < 1 || D->nnz < 0)
    return fail(ADMM_E_INVALID, "sparse matrix: rows and cols must be at least 1 and nnz at least 0");
  if (D->rows >= kIndexLimit || D->cols >= kIndexLimit || D->nnz >= kIndexLimit)
    return fail(ADMM_E_INVALID, "sparse matrix: rows, cols and nnz must be below 2^31");
  if (!D->jc || (D->nnz > 0 && (!D->ir || !D->val)))
    return fail(ADMM_E_INVALID, "sparse matrix: val / ir / jc is NULL");
  const uint64_t nnz = static_cast<uint64_t>(D->nnz), rows = static_cast<uint64_t>(D->rows);
  if (D->jc[0] != 0) return fail(ADMM_E_INVALID, "sparse matrix: jc[0] is not 0 (column 0)");
  for (int64_t j = 0; j < D->cols; ++j) {
    const std::string col = "column " + std::to_string(j);
    const uint64_t b = D->jc[j], e = D->jc[j + 1];
    if (e < b) return fail(ADMM_E_INVALID, "sparse matrix: jc decreases at " + col);
    if (e > nnz) return fail(ADMM_E_INVALID, "sparse matrix: jc runs past nnz at " + col);
    for (uint64_t k = b; k < e; ++k) {
      if (D->ir[k] >= rows) return fail(ADMM_E_INVALID, "sparse matrix: a row index is out of range in " + col);
      if (k > b && D->ir[k] <= D->ir[k - 1])
        return fail(ADMM_E_INVALID, "sparse matrix: the row indices are not strictly increasing in " + col +
                                        " (unsorted or duplicate entries)");
      if (!std::isfinite(D->val[k])) return fail(ADMM_E_INVALID, "sparse matrix: a value is not finite in " + col);
    }
  }
  if (D->jc[D->cols] != nnz)
    return fail(ADMM_E_INVALID, "sparse matrix: jc[cols] differs from nnz (column " + std::to_string(D->cols - 1) + ")");
  return ADMM_OK;
}

void sparse_orientations(const admm_sparse_desc* D, SparseHost* h) {
  const int64_t rows = D->rows, cols = D->cols, nnz = D->nnz;
  h->start_t.resize(cols + 1);
  h->idx_t.resize(nnz);
  for (int64_t j = 0; j <= cols; ++j) h->start_t[j] = static_cast<int64_t>(D->jc[j]);
  for (int64_t k = 0; k < nnz; ++k) h->idx_t[k] = static_cast<int32_t>(D->ir[k]);
  // counting sort by row; the columns are walked in ascending order, so every row's column indices ascend
  h->start_n.assign(rows + 1, 0);
  for (int64_t k = 0; k < nnz; ++k) ++h->start_n[h->idx_t[k] + 1];
  for (int64_t i = 0; i < rows; ++i) h->start_n[i + 1] += h->start_n[i];
  std::vector<int64_t> fill(h->start_n.begin(), h->start_n.end() - 1);
  h->idx_n.resize(nnz);
  h->val_n.resize(nnz);
  for (int64_t j = 0; j < cols; ++j)
    for (int64_t k = h->start_t[j]; k < h->start_t[j + 1]; ++k) {
      const int64_t dst = fill[h->idx_t[k]]++;
      h->idx_n[dst] = static_cast<int32_t>(j);
      h->val_n[dst] = D->val[k];
    }
}

int sparse_to_host(const admm_sparse_desc* D, admm_sparse_desc* copy, std::vector<double>* val,
                   std::vector<uint64_t>* ir, std::vector<uint64_t>* jc) {
  if (!D) return fail(ADMM_E_INVALID, "sparse matrix: the description is NULL");
  *copy = *D;
  if (D->mem != ADMM_MEM_DEVICE) return ADMM_OK;
  if (D->rows < 1 || D->cols < 1 || D->nnz < 0 || D->rows >= kIndexLimit || D->cols >= kIndexLimit ||
      D->nnz >= kIndexLimit || !D->jc || (D->nnz > 0 && (!D->ir || !D->val)))
    return fail(ADMM_E_INVALID, "sparse matrix: bad sizes or a NULL array");
  val->resize(D->nnz);
  ir->resize(D->nnz);
  jc->resize(D->cols + 1);
  ADMM_HIP_TRY(hipMemcpy(jc->data(), D->jc, sizeof(uint64_t) * jc->size(), hipMemcpyDeviceToHost));
  if (D->nnz > 0) {
    ADMM_HIP_TRY(hipMemcpy(ir->data(), D->ir, sizeof(uint64_t) * ir->size(), hipMemcpyDeviceToHost));
    ADMM_HIP_TRY(hipMemcpy(val->data(), D->val, sizeof(double) * val->size(), hipMemcpyDeviceToHost));
  }
  copy->val = val->data();
  copy->ir = ir->data();
  copy->jc = jc->data();
  copy->mem = ADMM_MEM_HOST;
  return ADMM_OK;
}

void sparse_device_free(SparseDev* sp) {
  for (void*& p : sp->bufs) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
}

int sparse_device_build(const admm_sparse_desc* D, SparseDev* out, hipStream_t stream) {
  SparseHost h;
  sparse_orientations(D, &h);
  const int64_t nnz = D->nnz;
  const size_t nz = static_cast<size_t>(nnz > 0 ? nnz : 1);  // (an all-zero matrix still gets valid pointers)
  const size_t bytes[6] = {sizeof(int64_t) * h.start_n.size(), sizeof(int32_t) * nz, sizeof(double) * nz,
                           sizeof(int64_t) * h.start_t.size(), sizeof(int32_t) * nz, sizeof(double) * nz};
  const void* src[6] = {h.start_n.data(), h.idx_n.data(), h.val_n.data(), h.start_t.data(), h.idx_t.data(), D->val};
  for (int k = 0; k < 6; ++k) {
    const hipError_t err = hipMalloc(&out->bufs[k], bytes[k]);
    if (err != hipSuccess) {
      sparse_device_free(out);
      return fail(ADMM_E_DEVICE, std::string("hipMalloc (sparse matrix): ") + hipGetErrorString(err));
    }
    const bool starts = k == 0 || k == 3;
    if (starts || nnz > 0) ADMM_HIP_TRY(hipMemcpyAsync(out->bufs[k], src[k], bytes[k], hipMemcpyHostToDevice, stream));
  }
  ADMM_HIP_TRY(hipStreamSynchronize(stream));  // (the host vectors go out of scope)
  const int64_t resident = 2 * (12 * nnz) + 8 * (D->rows + D->cols + 2);
  out->nnz = nnz;
  out->n.plan = spmv_plan(D->rows, D->cols, nnz, resident);
  out->n.start = static_cast<const int64_t*>(out->bufs[0]);
  out->n.idx = static_cast<const int32_t*>(out->bufs[1]);
  out->n.val = static_cast<const double*>(out->bufs[2]);
  out->t.plan = spmv_plan(D->cols, D->rows, nnz, resident);
  out->t.start = static_cast<const int64_t*>(out->bufs[3]);
  out->t.idx = static_cast<const int32_t*>(out->bufs[4]);
  out->t.val = static_cast<const double*>(out->bufs[5]);
  return ADMM_OK;
}

}  // namespace admm

using namespace admm;

extern "C" int admm_op_spmv(const admm_sparse_desc* D, int transpose, const double* x, double* y) {
  if (!D || !x || !y) return fail(ADMM_E_INVALID, "spmv: NULL argument");
  if (D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, "spmv: the operator takes host arrays");
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
  double *dx = nullptr, *dy = nullptr;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&dx), sizeof(double) * M.plan.cols);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&dy), sizeof(double) * M.plan.rows);
  if (err == hipSuccess) err = hipMemcpy(dx, x, sizeof(double) * M.plan.cols, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    launch_spmv(M, dx, dy, nullptr, nullptr);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(y, dy, sizeof(double) * M.plan.rows, hipMemcpyDeviceToHost);
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  sparse_device_free(&sp);
  if (err != hipSuccess) return fail(ADMM_E_DEVICE, std::string("spmv: ") + hipGetErrorString(err));
  return ADMM_OK;
}
