// spmv.h -- sparse matrix-vector products for the matrix-free lasso x-update on a sparse design matrix.
// One kernel, y = M*x for M stored by rows (CSR: int64 row starts, int32 column indices, fp64 values: 12 B per nonzero);
// the engine keeps BOTH orientations of D resident -- D by rows for D*p, and D' by rows (the caller's CSC arrays as they
// arrive) for D'*(D p) -- so neither product needs atomics and each row has one fixed summation order.
#pragma once
#include <vector>

#include "common.h"

namespace admm {

// CSR-vector layout: `lanes` (a power of two, 1 .. 64) consecutive lanes of a wave share one row and walk it in strides
// of `lanes`; a workgroup of kBlock threads takes kBlock / lanes consecutive rows.  Chosen once per orientation.
struct SpmvPlan {
  int64_t rows = 0, cols = 0, nnz = 0;
  int32_t lanes = 1;   // the smallest power of two >= the mean number of nonzeros per row, at most 64
  int32_t grid = 1;    // ceil(rows / (kBlock / lanes)) workgroups
  bool stream = false; // both orientations together exceed what the caches hold: non-temporal loads of idx / val
};
SpmvPlan spmv_plan(int64_t rows, int64_t cols, int64_t nnz, int64_t resident_bytes);

struct SpmvMat {  // one orientation on the device
  SpmvPlan plan;
  const int64_t* start = nullptr;  // [rows + 1]
  const int32_t* idx = nullptr;    // [nnz] column of every stored value, ascending inside a row
  const double* val = nullptr;     // [nnz]
};

// y[rows] = M * x[cols].  Lane l of a row's group adds its products k = start + l, start + l + lanes, ... in that order;
// the `lanes` partial sums are combined by a butterfly inside the wave (DPP / permlane swaps, no LDS): two runs give the
// same bits.  An empty row stores 0.0.  ctrl (nullable): the launch is a no-op once ctrl->stop is set.
void launch_spmv(const SpmvMat& M, const double* x, double* y, const Ctrl* ctrl, hipStream_t stream);

// The checks of admm_engine_create_sparse / admm_binding_create on HOST arrays (no device): sizes below 2^31, jc[0] == 0,
// jc non-decreasing, jc[cols] == nnz, every ir < rows and strictly increasing inside a column, every value finite.
// ADMM_E_INVALID with a message that names the first offending column.
int sparse_csc_check(const admm_sparse_desc* D);

// D' by rows = the CSC arrays narrowed to 32-bit indices; D by rows = their transpose by a counting sort that walks the
// columns in ascending order, so the column indices of every row ascend as well
struct SparseHost {
  std::vector<int64_t> start_t, start_n;
  std::vector<int32_t> idx_t, idx_n;
  std::vector<double> val_n;  // (the values of D' by rows are the caller's array itself)
};
void sparse_orientations(const admm_sparse_desc* D, SparseHost* h);

// Both orientations of a checked HOST matrix on the device (24 B per nonzero), with their plans; owns its allocations
struct SparseDev {
  SpmvMat n;  // D by rows:  y[rows] = D * x[cols]
  SpmvMat t;  // D' by rows: y[cols] = D' * x[rows]
  void* bufs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t nnz = 0;
};
int sparse_device_build(const admm_sparse_desc* D, SparseDev* out, hipStream_t stream);  // complete on return
void sparse_device_free(SparseDev* sp);
// D (any ADMM_MEM_*) as checked HOST arrays: *host points at D itself, or at `copy` backed by the three vectors
int sparse_to_host(const admm_sparse_desc* D, admm_sparse_desc* copy, std::vector<double>* val,
                   std::vector<uint64_t>* ir, std::vector<uint64_t>* jc);

}  // namespace admm
