// ops.hip -- stand-alone operator entry points of the C ABI (HOST pointers in, HOST out).
// Thin wrappers: upload -> the same kernels the loop uses -> download.  They exist so the
// parity tests can pin every kernel against the oracle on its own, and for bindings that
// keep a user prox on the host but want the heavy linear algebra on the device.
#include <cstring>
#include <string>
#include <vector>

#include "dct.h"
#include "engine_internal.h"
#include "group_multi.h"
#include "kernels.h"
#include "loop_kernels.h"
#include "multi_device.h"
#include "spmm.h"
#include "tv2d.h"

using namespace admm;

namespace {

struct Scratch {  // frees everything on scope exit
  std::vector<void*> ptrs;
  ~Scratch() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T = double>
  int alloc(T** out, size_t elems) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (elems ? elems : 1) * sizeof(T));
    if (e != hipSuccess) return fail(ADMM_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
    ptrs.push_back(p);
    *out = static_cast<T*>(p);
    return ADMM_OK;
  }
  template <typename T>
  int put(T** dev, const T* host, size_t elems) {  // alloc + the host operand
    ADMM_TRY(alloc(dev, elems));
    ADMM_HIP_TRY(hipMemcpy(*dev, host, sizeof(T) * elems, hipMemcpyHostToDevice));
    return ADMM_OK;
  }
};

// the end of a vector operator: wait for its kernels, then the result back to the host
int fetch(double* host, const double* dev, size_t elems) {
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy(host, dev, sizeof(double) * elems, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int need_device() {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
    return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  return ADMM_OK;
}

int put_matrix(Scratch& sc, double** dst, int64_t* ld, const double* src, int64_t rows, int64_t cols, int64_t ld_src) {
  *ld = round_up(rows, 16);
  ADMM_TRY(sc.alloc(dst, static_cast<size_t>(*ld) * cols));
  ADMM_HIP_TRY(hipMemset(*dst, 0, sizeof(double) * (*ld) * cols));
  ADMM_HIP_TRY(hipMemcpy2D(*dst, (*ld) * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), cols,
                           hipMemcpyHostToDevice));
  return ADMM_OK;
}

// a column-major host matrix with the caller's leading dimension VERBATIM (put_matrix rounds it up): an odd ld must
// reach the kernel, it selects the guarded tile loader of the GEMM.  The device buffer is ld x cols and starts as
// all-ones bytes (NaN), so an element a kernel reads past the rows the caller gave poisons its result.
int put_verbatim(Scratch& sc, double** dst, const double* src, int64_t rows, int64_t cols, int64_t ld) {
  const size_t elems = static_cast<size_t>(ld) * cols;
  ADMM_TRY(sc.alloc(dst, elems));
  ADMM_HIP_TRY(hipMemset(*dst, 0xFF, sizeof(double) * elems));
  ADMM_HIP_TRY(hipMemcpy(*dst, src, sizeof(double) * (static_cast<size_t>(ld) * (cols - 1) + rows),
                         hipMemcpyHostToDevice));
  return ADMM_OK;
}

// the n x n part of a host matrix, exactly as given, into zero-filled npad x npad storage (SymvPlan's contract)
int put_padded(double* dst, int64_t npad, const double* src, int64_t n, int64_t ld_src) {
  ADMM_HIP_TRY(hipMemcpy2D(dst, npad * sizeof(double), src, ld_src * sizeof(double), n * sizeof(double), n,
                           hipMemcpyHostToDevice));
  return ADMM_OK;
}

// ---- the spectral x-update of 2-D total variation (dct.h)
// An H x W device image with ld = H, as the engine holds it, between kGuardCols columns on either side; the whole
// buffer starts as all-ones bytes (NaN): an element no kernel wrote shows in the result, a write outside the image in
// guards_intact.  (Two columns: 2H doubles keep the image at the 16-byte alignment the paired loads rely on.)
constexpr int64_t kGuardCols = 2;
int guarded_image(Scratch& sc, double** img, int64_t H, int64_t W) {
  const size_t elems = static_cast<size_t>(H) * (W + 2 * kGuardCols);
  double* base = nullptr;
  ADMM_TRY(sc.alloc(&base, elems));
  ADMM_HIP_TRY(hipMemset(base, 0xFF, sizeof(double) * elems));
  *img = base + kGuardCols * H;
  return ADMM_OK;
}
int guards_intact(const double* img, int64_t H, int64_t W, const char* what) {
  const size_t g = static_cast<size_t>(kGuardCols * H);
  std::vector<uint64_t> host(2 * g);
  ADMM_HIP_TRY(hipMemcpy(host.data(), img - g, sizeof(double) * g, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(host.data() + g, img + H * W, sizeof(double) * g, hipMemcpyDeviceToHost));
  for (uint64_t v : host)
    if (v != ~uint64_t{0}) return fail(ADMM_E_NUMERIC, std::string(what) + ": a kernel wrote outside the image");
  return ADMM_OK;
}
int put_image(double* dst, const double* src, int64_t H, int64_t W) {
  ADMM_HIP_TRY(hipMemcpy(dst, src, sizeof(double) * H * W, hipMemcpyHostToDevice));
  return ADMM_OK;
}
int get_image(double* dst, const double* src, int64_t H, int64_t W) {
  ADMM_HIP_TRY(hipMemcpy(dst, src, sizeof(double) * H * W, hipMemcpyDeviceToHost));
  return ADMM_OK;
}
int zeroed_ctrl(Scratch& sc, Ctrl** ctrl) {  // the kernels read ctrl->stop without a null test
  ADMM_TRY(sc.alloc(ctrl, 1));
  ADMM_HIP_TRY(hipMemset(*ctrl, 0, sizeof(Ctrl)));
  return ADMM_OK;
}
struct TableMem {  // owner of the device tables of dct_tables_create
  DevMem mem;
  ~TableMem() { mem.release(); }
};
bool tv2d_height_ok(int64_t H) { return dct_length_ok(H) || dct_chirp_length_ok(H); }

// the form an operator call runs: AUTO through the engine's rule, a forced one checked against its own precondition
int tv2d_op_form(const char* op, int64_t H, int64_t W, double rho, int32_t form, Tv2Rows* rows) {
  if (H <= 0 || W <= 0 || !tv2d_height_ok(H) || !finite_pos(rho) || form < ADMM_TV2D_ROWS_AUTO ||
      form > ADMM_TV2D_ROWS_THOMAS)
    return fail(ADMM_E_INVALID, std::string(op) + ": bad argument (H a column-transform length, W >= 1, rho finite and > 0, form 0..4)");
  *rows = form == ADMM_TV2D_ROWS_AUTO ? tv2d_row_stage(H, W, rho, dct_length_ok(W)) : static_cast<Tv2Rows>(form);
  if (!tv2d_rows_form_ok(*rows, H, W, rho))
    return fail(ADMM_E_INVALID, std::string(op) + ": the forced row stage does not apply to this width, height and rho");
  return ADMM_OK;
}

}  // namespace

namespace admm {

// the checks admm_engine_set_loss and admm_op_loss_prox share; len weights when desc->weights is set
int check_loss_desc(int32_t problem, const admm_loss_desc& d, int64_t len) {
  if (problem != ADMM_PROB_LAD && problem != ADMM_PROB_HUBERFIT)
    return fail(ADMM_E_INVALID, "the loss family belongs to ADMM_PROB_LAD and ADMM_PROB_HUBERFIT");
  if (!finite_pos(d.slope_pos) || !finite_pos(d.slope_neg))
    return fail(ADMM_E_INVALID, "loss: both slopes must be finite and > 0");
  if (!finite_nonneg(d.epsilon)) return fail(ADMM_E_INVALID, "loss: epsilon must be finite and >= 0");
  if (!finite_pos(d.delta)) return fail(ADMM_E_INVALID, "loss: delta must be finite and > 0");
  if (problem == ADMM_PROB_HUBERFIT && d.epsilon != 0.0)
    return fail(ADMM_E_INVALID, "loss: epsilon belongs to the LAD engine (a Huber engine takes 0)");
  if (problem == ADMM_PROB_LAD && d.delta != 1.0)
    return fail(ADMM_E_INVALID, "loss: delta belongs to the Huber engine (a LAD engine takes 1)");
  if (d.weights)
    for (int64_t i = 0; i < len; ++i)
      if (!finite_nonneg(d.weights[i])) return fail(ADMM_E_INVALID, "loss: weight " + std::to_string(i) + " is negative or not finite");
  return ADMM_OK;
}

// the checks admm_engine_set_svm_cost, admm_svm_ovr_set_cost and admm_op_svm_prox share: len HOST weights (or null) and
// ncosts HOST class costs (or null), every one finite and >= 0
int check_svm_cost(const double* weights, int64_t len, const double* costs, int64_t ncosts) {
  if (costs)
    for (int64_t i = 0; i < ncosts; ++i)
      if (!finite_nonneg(costs[i])) return fail(ADMM_E_INVALID, "svm cost: class cost " + std::to_string(i) + " is negative or not finite");
  if (weights)
    for (int64_t i = 0; i < len; ++i)
      if (!finite_nonneg(weights[i])) return fail(ADMM_E_INVALID, "svm cost: weight " + std::to_string(i) + " is negative or not finite");
  return ADMM_OK;
}

}  // namespace admm

extern "C" {

int admm_op_gemv_n(const double* D, int64_t m, int64_t n, int64_t ldD, const double* x, double* y) {
  if (!D || !x || !y || m <= 0 || n <= 0 || ldD < m) return fail(ADMM_E_INVALID, "gemv_n: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dD, *dx, *dpart, *dy;
  int64_t ld;
  ADMM_TRY(put_matrix(sc, &dD, &ld, D, m, n, ldD));
  ADMM_TRY(sc.alloc(&dx, n));
  ADMM_HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  GemvNPlan p = gemv_n_plan(m, n, ld);
  ADMM_TRY(sc.alloc(&dpart, p.part_elems()));
  ADMM_TRY(sc.alloc(&dy, round_up(m, 2)));
  launch_gemv_n(p, dD, dx, dpart, nullptr, nullptr);
  launch_sum_partials(dpart, p.nchunk, p.ldy, m, dy, nullptr, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy(y, dy, sizeof(double) * m, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_gemv_t(const double* D, int64_t m, int64_t n, int64_t ldD, const double* V, int64_t ldV, int32_t nrhs,
                   double* G, int64_t ldG) {
  if (!D || !V || !G || m <= 0 || n <= 0 || ldD < m || ldV < m || ldG < n || nrhs < 1 || nrhs > 3)
    return fail(ADMM_E_INVALID, "gemv_t: bad argument (1 <= nrhs <= 3)");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dD, *dV, *dpart, *dG;
  int64_t ld, ldv;
  ADMM_TRY(put_matrix(sc, &dD, &ld, D, m, n, ldD));
  ADMM_TRY(put_matrix(sc, &dV, &ldv, V, m, nrhs, ldV));
  GemvTPlan p = gemv_t_plan(m, n, ld);
  ADMM_TRY(sc.alloc(&dpart, p.part_elems(nrhs)));
  ADMM_TRY(sc.alloc(&dG, static_cast<size_t>(p.ldg) * nrhs));
  launch_gemv_t(p, dD, dV, nrhs > 1 ? dV + ldv : nullptr, nrhs > 2 ? dV + 2 * ldv : nullptr, nrhs, dpart, nullptr,
                nullptr);
  launch_sum_partials_t(p, dpart, nrhs, dG, p.ldg, nullptr, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy2D(G, ldG * sizeof(double), dG, p.ldg * sizeof(double), n * sizeof(double), nrhs,
                           hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_gemv_forms(int64_t m, int64_t n, int32_t out[5]) {
  if (!out || m <= 0 || n <= 0 || m > (int64_t{1} << 40) / n)
    return fail(ADMM_E_INVALID, "gemv_forms: bad argument (m, n >= 1, m * n <= 2^40)");
  const int64_t ld = round_up(m, 16);  // (put_matrix)
  const GemvNPlan pn = gemv_n_plan(m, n, ld);
  const GemvTPlan pt = gemv_t_plan(m, n, ld);
  out[0] = pn.nchunk;
  out[1] = static_cast<int32_t>(pn.cols_per_chunk);
  out[2] = pt.rows_per_chunk;
  out[3] = pt.nchunk;
  out[4] = stream_hint(8 * m * n) ? 1 : 0;  // (the launchers' own expression)
  return ADMM_OK;
}

int admm_op_gram(const double* D, int64_t m, int64_t n, int64_t ldD, double shift, double* W) {
  if (!D || !W || m <= 0 || n <= 0 || ldD < m) return fail(ADMM_E_INVALID, "gram: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dD, *dW;
  int64_t ld;
  ADMM_TRY(put_matrix(sc, &dD, &ld, D, m, n, ldD));
  const int64_t ldw = round_up(n, 16);
  ADMM_TRY(sc.alloc(&dW, static_cast<size_t>(ldw) * n));
  ADMM_HIP_TRY(hipMemset(dW, 0, sizeof(double) * ldw * n));
  launch_gemm(1, 0, n, n, m, 1.0, dD, ld, dD, ld, 0.0, dW, ldw, true, nullptr);
  if (shift != 0.0) launch_add_diag(dW, n, ldw, shift, nullptr);
  launch_symmetrize_lower(dW, n, ldw, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy2D(W, n * sizeof(double), dW, ldw * sizeof(double), n * sizeof(double), n,
                           hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_cholesky(double* A, int64_t n, int64_t ldA) {
  if (!A || n <= 0 || ldA < n) return fail(ADMM_E_INVALID, "cholesky: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dA, *dinfo;
  int64_t ld;
  ADMM_TRY(put_matrix(sc, &dA, &ld, A, n, n, ldA));
  ADMM_TRY(sc.alloc(&dinfo, 1));
  ADMM_TRY(cholesky_lower(dA, n, ld, reinterpret_cast<int32_t*>(dinfo), nullptr, nullptr));
  ADMM_HIP_TRY(hipDeviceSynchronize());
  int32_t info = 0;
  ADMM_HIP_TRY(hipMemcpy(&info, dinfo, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (info != 0)
    return fail(ADMM_E_NUMERIC, "Cholesky failed: matrix must be positive definite (pivot " + std::to_string(info) + ")");
  ADMM_HIP_TRY(hipMemcpy2D(A, ldA * sizeof(double), dA, ld * sizeof(double), n * sizeof(double), n,
                           hipMemcpyDeviceToHost));
  for (int64_t j = 1; j < n; ++j)
    for (int64_t i = 0; i < j; ++i) A[i + j * ldA] = 0.0;  // chol(.,'lower') returns a lower-triangular matrix
  return ADMM_OK;
}

int admm_op_trsv_pair(const double* L, int64_t n, int64_t ldL, const double* y, double* x) {
  if (!L || !y || !x || n <= 0 || ldL < n) return fail(ADMM_E_INVALID, "trsv_pair: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dL, *dy, *dx, *dinv, *buf;
  int64_t ld;
  ADMM_TRY(put_matrix(sc, &dL, &ld, L, n, n, ldL));
  ADMM_TRY(sc.alloc(&dy, round_up(n, 2)));
  ADMM_TRY(sc.alloc(&dx, round_up(n, 2)));
  ADMM_HIP_TRY(hipMemcpy(dy, y, sizeof(double) * n, hipMemcpyHostToDevice));
  TrsvPlan plan{};
  ADMM_TRY(sc.alloc(&dinv, static_cast<size_t>(ceil_div(n, 64)) * 64 * 64));
  launch_trtri_diag(dL, n, ld, dinv, nullptr);
  const int form = trsv_resolve_form(n, kTrsvBlocked);
  ADMM_TRY(sc.alloc(&buf, trsv_plan_elems(n, form)));
  ADMM_TRY(trsv_build(dL, n, ld, dinv, buf, &plan, nullptr, form));
  launch_trsv_pair(plan, dy, dx, nullptr, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

__global__ void soft_threshold_kernel(const double* __restrict__ v, int64_t n, double t, double* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const double a = fabs(v[i]) - t;
    const double p = a > 0.0 ? a : 0.0;
    out[i] = (v[i] > 0.0) ? p : ((v[i] < 0.0) ? -p : 0.0);
  }
}

int admm_op_soft_threshold(const double* v, int64_t n, double t, double* out) {
  if (!v || !out || n <= 0) return fail(ADMM_E_INVALID, "soft_threshold: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dout;
  ADMM_TRY(sc.put(&dv, v, n));
  ADMM_TRY(sc.alloc(&dout, n));
  const int blocks = grid_blocks(n, kBlock, 2048);
  hipLaunchKernelGGL(soft_threshold_kernel, dim3(blocks), dim3(kBlock), 0, nullptr, dv, n, t,
                     dout);
  return fetch(out, dout, n);
}

int admm_op_pair_soft_threshold(const double* v, int64_t N, double t, double* out) {
  if (!v || !out || N <= 0 || !(t >= 0.0)) return fail(ADMM_E_INVALID, "pair_soft_threshold: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dout;
  ADMM_TRY(sc.put(&dv, v, 2 * N));
  ADMM_TRY(sc.alloc(&dout, 2 * N));
  launch_tv2d_pair_soft_threshold(dv, N, t, dout, nullptr);
  return fetch(out, dout, 2 * N);
}

int admm_op_group_soft_threshold(const double* v, int64_t n, const int64_t* sizes, int32_t ngroups, const double* weights,
                                 double lambda_over_rho, double* out) {
  if (!v || !out || n <= 0 || !(lambda_over_rho >= 0.0))
    return fail(ADMM_E_INVALID, "group_soft_threshold: bad argument");
  GroupPlanHost h;
  ADMM_TRY(group_plan_build(sizes, ngroups, weights, n, &h));
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dout, *dplan;
  ADMM_TRY(sc.put(&dv, v, n));
  ADMM_TRY(sc.alloc(&dout, n));
  ADMM_TRY(sc.put<double>(&dplan, h.blob.data(), h.blob.size()));
  launch_group_soft_threshold(dv, h.bind(dplan), lambda_over_rho, dout, nullptr);
  return fetch(out, dout, n);
}

int admm_op_penalty_prox(const double* v, int64_t n, const int64_t* sizes, int32_t ngroups, const double* groupweights,
                         double lambda_over_rho, const admm_penalty_desc* desc, double rho, double* out) {
  if (!v || !out || n <= 0 || !finite_nonneg(lambda_over_rho) || !finite_pos(rho) || ngroups < 0)
    return fail(ADMM_E_INVALID, "penalty_prox: bad argument");
  const admm_penalty_desc none{nullptr, 0.0, 0.0, 0};
  const admm_penalty_desc& d = desc ? *desc : none;
  if (!finite_nonneg(d.l1) || !finite_nonneg(d.ridge) || (d.nonnegative != 0 && d.nonnegative != 1))
    return fail(ADMM_E_INVALID, "penalty_prox: l1 and ridge must be finite and >= 0, nonnegative 0 or 1");
  if (d.l1weights)
    for (int64_t i = 0; i < n; ++i)
      if (!finite_nonneg(d.l1weights[i])) return fail(ADMM_E_INVALID, "penalty_prox: an l1 weight is negative or not finite");
  const bool groups = sizes && ngroups > 0;
  GroupPlanHost h;
  if (groups) ADMM_TRY(group_plan_build(sizes, ngroups, groupweights, n, &h));
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dout, *dplan = nullptr, *dw = nullptr;
  ADMM_TRY(sc.put(&dv, v, n));
  ADMM_TRY(sc.alloc(&dout, n));
  if (d.l1weights) ADMM_TRY(sc.put(&dw, d.l1weights, n));
  PenaltyArgs pen{};  // (the objective's fields stay 0: the operator forms no objective)
  pen.w = dw;
  pen.tau = groups ? d.l1 / rho : lambda_over_rho;  // without groups lambda is the l1 weight itself
  pen.kappa = rho / (rho + d.ridge);
  pen.nonneg = d.nonnegative;
  GroupPlan gp{};
  if (groups) {
    ADMM_TRY(sc.put<double>(&dplan, h.blob.data(), h.blob.size()));
    gp = h.bind(dplan);
  }
  launch_penalty_prox(dv, n, groups ? &gp : nullptr, lambda_over_rho, pen, dout, nullptr);
  return fetch(out, dout, n);
}

int admm_op_loss_prox(const double* v, int64_t len, int32_t problem, const admm_loss_desc* desc, double rho, double* out) {
  if (!v || !out || len <= 0 || !finite_pos(rho))
    return fail(ADMM_E_INVALID, "loss_prox: bad argument");
  const admm_loss_desc none{nullptr, 1.0, 1.0, 0.0, 1.0};
  const admm_loss_desc& d = desc ? *desc : none;
  ADMM_TRY(check_loss_desc(problem, d, len));
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dout, *dw = nullptr;
  ADMM_TRY(sc.put(&dv, v, len));
  ADMM_TRY(sc.alloc(&dout, len));
  if (d.weights) ADMM_TRY(sc.put(&dw, d.weights, len));
  const LossArgs la{dw, d.slope_pos, d.slope_neg, d.epsilon, d.delta, rho, problem == ADMM_PROB_HUBERFIT ? 1 : 0, 0};
  launch_loss_prox(dv, len, la, dout, nullptr);
  return fetch(out, dout, len);
}

int admm_op_svm_prox(const double* v, const double* ell, int64_t len, int32_t loss, double C, double rho,
                     const admm_svm_cost_desc* desc, double* out) {
  if (!v || !ell || !out || len <= 0 || !finite_pos(rho) || !finite_nonneg(C))
    return fail(ADMM_E_INVALID, "svm_prox: bad argument");
  if (loss != ADMM_LOSS_HINGE && loss != ADMM_LOSS_01 && loss != ADMM_LOSS_HINGE_OBJ01 && loss != ADMM_LOSS_LOGISTIC &&
      loss != ADMM_LOSS_SQHINGE)
    return fail(ADMM_E_INVALID, "svm_prox: bad loss");
  const admm_svm_cost_desc none{nullptr, 1.0, 1.0};
  const admm_svm_cost_desc& d = desc ? *desc : none;
  const double costs[2] = {d.cost_pos, d.cost_neg};
  ADMM_TRY(check_svm_cost(d.weights, len, costs, 2));
  ADMM_TRY(need_device());
  Scratch sc;
  double *dv, *dl, *dout, *dw = nullptr;
  ADMM_TRY(sc.put(&dv, v, len));
  ADMM_TRY(sc.put(&dl, ell, len));
  ADMM_TRY(sc.alloc(&dout, len));
  if (d.weights) ADMM_TRY(sc.put(&dw, d.weights, len));
  const SvmCostArgs ka{dw, d.cost_pos, d.cost_neg, C, rho, loss, 0};
  launch_svm_cost_prox(dv, dl, len, ka, dout, nullptr);
  return fetch(out, dout, len);
}

int admm_op_symv(const double* M, int64_t n, int64_t ldM, const double* x, int32_t form, int64_t ncached,
                 int32_t part_count, double* y) {
  if (!M || !x || !y || n <= 0 || ldM < n || form < 0 || form > 3 || ncached < -1 || part_count < 1 ||
      (form == 0 && (part_count > 1 || (ldM & 1))))
    return fail(ADMM_E_INVALID, "symv: bad argument (form 0..3, ncached >= -1, part_count >= 1; form 0: one part, even ldM)");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dM, *dx, *dy;
  ADMM_TRY(sc.alloc(&dx, round_up(n, 2)));
  ADMM_TRY(sc.alloc(&dy, round_up(n, 2)));
  ADMM_HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  if (form == 0) {
    ADMM_TRY(put_verbatim(sc, &dM, M, n, n, ldM));
    launch_symv_small(dM, n, ldM, dx, dy, nullptr, nullptr);
    ADMM_HIP_TRY(hipDeviceSynchronize());
    ADMM_HIP_TRY(hipMemcpy(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost));
    return ADMM_OK;
  }
  SymvPlan plan = symv_plan(n);
  if (ncached >= 0) plan.ncached = ncached;
  ADMM_TRY(sc.alloc(&dM, static_cast<size_t>(plan.npad) * plan.npad));
  ADMM_HIP_TRY(hipMemset(dM, 0, sizeof(double) * plan.npad * plan.npad));
  ADMM_TRY(put_padded(dM, plan.npad, M, n, ldM));
  const double* dA = dM;
  if (form >= 2) {
    double* dP;
    ADMM_TRY(sc.alloc(&dP, symv_packed_elems(plan)));
    launch_symv_pack(plan, dM, plan.npad, dP, nullptr);
    plan.packed = true;
    dA = dP;
  }
  double *npart, *tpart;
  ADMM_TRY(sc.alloc(&npart, plan.npart_elems()));
  ADMM_TRY(sc.alloc(&tpart, plan.tpart_elems()));
  Ctrl* ctrl = nullptr;
  if (form == 3) {  // symv_lower_fin_kernel reads ctrl->stop without a null test: a zero-filled control block
    ADMM_TRY(sc.alloc(&ctrl, 1));
    ADMM_HIP_TRY(hipMemset(ctrl, 0, sizeof(Ctrl)));
  }
  // one part: every partial slot the sum reads is written by a tile, so the slots start as NaN and a missed one shows;
  // several parts: the launcher asks for zero-filled slots (the tiles of the other ranks stay zero)
  const int fill = part_count > 1 ? 0 : 0xFF;
  std::vector<double> part(static_cast<size_t>(n));
  for (int32_t r = 0; r < part_count; ++r) {
    ADMM_HIP_TRY(hipMemset(npart, fill, sizeof(double) * plan.npart_elems()));
    ADMM_HIP_TRY(hipMemset(tpart, fill, sizeof(double) * plan.tpart_elems()));
    if (form == 3)
      launch_symv_lower_fin(plan, dA, dx, npart, tpart, FinArgs{}, false, ctrl, nullptr, r, part_count, dy);
    else
      launch_symv_lower(plan, dA, plan.npad, dx, npart, tpart, dy, ctrl, nullptr, r, part_count);
    ADMM_HIP_TRY(hipDeviceSynchronize());
    ADMM_HIP_TRY(hipMemcpy(r == 0 ? y : part.data(), dy, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (r > 0)
      for (int64_t i = 0; i < n; ++i) y[i] += part[i];  // the ranks' partial results, in rank order
  }
  return ADMM_OK;
}

int admm_op_symm_packed(const double* M, int64_t n, int64_t ldM, double* X, int32_t K, const int32_t* stop_mask,
                        const double* Y) {
  if (!M || !X || !Y || n <= 0 || ldM < n || K < 1)
    return fail(ADMM_E_INVALID, "symm_packed: bad argument (n >= 1, ldM >= n, K >= 1)");
  ADMM_TRY(need_device());
  Scratch sc;
  SymvPlan plan = symv_plan(n);
  double *dM, *dP, *dX, *dY, *part;
  ADMM_TRY(sc.alloc(&dM, static_cast<size_t>(plan.npad) * plan.npad));
  ADMM_HIP_TRY(hipMemset(dM, 0, sizeof(double) * plan.npad * plan.npad));
  ADMM_TRY(put_padded(dM, plan.npad, M, n, ldM));
  ADMM_TRY(sc.alloc(&dP, symv_packed_elems(plan)));
  launch_symv_pack(plan, dM, plan.npad, dP, nullptr);
  plan.packed = true;
  const size_t elems = static_cast<size_t>(spmm_chunks(K)) * kSpmmChunk * n;
  std::vector<double> hb(elems);
  spmm_pack(Y, n, n, K, hb.data());
  ADMM_TRY(sc.put(&dY, static_cast<const double*>(hb.data()), elems));
  spmm_pack(X, n, n, K, hb.data());
  ADMM_TRY(sc.put(&dX, static_cast<const double*>(hb.data()), elems));
  // every partial slot the sum reads is written by a tile: the slots start as NaN, so a missed one shows
  ADMM_TRY(sc.alloc(&part, symm_part_elems(plan, K)));
  ADMM_HIP_TRY(hipMemset(part, 0xFF, sizeof(double) * symm_part_elems(plan, K)));
  MultiRec* rec = nullptr;
  if (stop_mask) {
    std::vector<MultiRec> rh(static_cast<size_t>(K), MultiRec{0, 0, 0, 0});
    for (int32_t k = 0; k < K; ++k) rh[k].stop = stop_mask[k] != 0;
    ADMM_TRY(sc.put(&rec, static_cast<const MultiRec*>(rh.data()), rh.size()));
  }
  launch_symm_packed(plan, dP, dY, dX, part, rec, K, nullptr);
  ADMM_TRY(fetch(hb.data(), dX, elems));
  spmm_unpack(hb.data(), n, K, X, n);
  return ADMM_OK;
}

int admm_op_group_soft_threshold_multi(const double* V, int64_t n, int32_t K, const int64_t* sizes, int32_t ngroups,
                                       const double* groupweights, const double* t, const int32_t* stop_mask, double* Z) {
  if (!V || !Z || !t || n <= 0 || K < 1)
    return fail(ADMM_E_INVALID, "group_soft_threshold_multi: bad argument (n >= 1, K >= 1)");
  for (int32_t k = 0; k < K; ++k)
    if (!finite_nonneg(t[k]))
      return fail(ADMM_E_INVALID, "group_soft_threshold_multi: t[" + std::to_string(k) + "] is negative or not finite");
  GroupPlanHost h;
  ADMM_TRY(group_plan_build(sizes, ngroups, groupweights, n, kGmLimits, &h));
  ADMM_TRY(need_device());
  Scratch sc;
  const size_t elems = static_cast<size_t>(spmm_chunks(K)) * kSpmmChunk * n;
  std::vector<double> hb(elems);
  double *dV, *dZ, *dplan, *dt;
  spmm_pack(V, n, n, K, hb.data());
  ADMM_TRY(sc.put(&dV, static_cast<const double*>(hb.data()), elems));
  spmm_pack(Z, n, n, K, hb.data());
  ADMM_TRY(sc.put(&dZ, static_cast<const double*>(hb.data()), elems));
  ADMM_TRY(sc.put<double>(&dplan, h.blob.data(), h.blob.size()));
  ADMM_TRY(sc.put(&dt, t, static_cast<size_t>(K)));
  MultiRec* rec = nullptr;
  std::vector<MultiRec> rh(static_cast<size_t>(K), MultiRec{0, 0, 0, 0});
  for (int32_t k = 0; stop_mask && k < K; ++k) rh[k].stop = stop_mask[k] != 0;
  ADMM_TRY(sc.put(&rec, static_cast<const MultiRec*>(rh.data()), rh.size()));
  launch_group_multi_shrink(dV, dZ, K, h.bind(dplan), dt, rec, nullptr);
  ADMM_TRY(fetch(hb.data(), dZ, elems));
  spmm_unpack(hb.data(), n, K, Z, n);
  return ADMM_OK;
}

int admm_group_multi_plan(int64_t n, const int64_t* sizes, int32_t ngroups, int64_t* wg_first, int32_t cap, int32_t* nwg,
                          int64_t* budget) {
  GroupPlanHost h;
  ADMM_TRY(group_plan_build(sizes, ngroups, nullptr, n, kGmLimits, &h));
  if (nwg) *nwg = h.nwg;
  if (budget) *budget = h.budget;
  if (wg_first) {
    if (cap < h.nwg + 1) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    std::memcpy(wg_first, h.blob.data() + h.o_wge, sizeof(int64_t) * (static_cast<size_t>(h.nwg) + 1));
  }
  return ADMM_OK;
}

int admm_op_symv_compact(const double* M, int64_t n, int64_t ldM, const double* x, int32_t fin, int64_t ncached,
                         int32_t part_count, double* y, double* Q, int64_t ldQ) {
  return admm_op_symv_compact_bits(M, n, ldM, x, fin, ncached, part_count, y, Q, ldQ, 48);
}

int admm_op_symv_compact_bits(const double* M, int64_t n, int64_t ldM, const double* x, int32_t fin, int64_t ncached,
                              int32_t part_count, double* y, double* Q, int64_t ldQ, int32_t bits) {
  if (!M || !x || !y || n <= 0 || ldM < n || ncached < -1 || part_count < 1 || (Q && ldQ < n))
    return fail(ADMM_E_INVALID, "symv_compact: bad argument (ncached >= -1, part_count >= 1, ldQ >= n)");
  if (!symv_cbits_ok(bits))
    return fail(ADMM_E_INVALID, "symv_compact: the compact tile widths are 36, 38, 40 and 48 bits");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dM, *dx, *dy, *dC, *dQ = nullptr, *npart, *tpart;
  ADMM_TRY(sc.alloc(&dx, round_up(n, 2)));
  ADMM_TRY(sc.alloc(&dy, round_up(n, 2)));
  ADMM_HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  SymvPlan plan = symv_plan(n);
  plan.packed = true;
  plan.cbits = bits;
  ADMM_TRY(sc.alloc(&dM, static_cast<size_t>(plan.npad) * plan.npad));
  ADMM_HIP_TRY(hipMemset(dM, 0, sizeof(double) * plan.npad * plan.npad));
  ADMM_TRY(put_padded(dM, plan.npad, M, n, ldM));
  ADMM_TRY(sc.alloc(&dC, symv_compact_elems(plan)));
  if (Q) ADMM_TRY(sc.alloc(&dQ, symv_packed_elems(plan)));
  launch_symv_compact_pack(plan, dM, plan.npad, false, dC, dQ, nullptr);
  plan.scales = symv_compact_scales(plan, dC);
  plan.ncached = ncached >= 0 ? ncached : symv_cached_tiles(plan, kSymvCacheBytes);
  ADMM_TRY(sc.alloc(&npart, plan.npart_elems()));
  ADMM_TRY(sc.alloc(&tpart, plan.tpart_elems()));
  Ctrl* ctrl = nullptr;
  if (fin) {  // (as in admm_op_symv: a zero-filled control block)
    ADMM_TRY(sc.alloc(&ctrl, 1));
    ADMM_HIP_TRY(hipMemset(ctrl, 0, sizeof(Ctrl)));
  }
  const int fill = part_count > 1 ? 0 : 0xFF;  // (as in admm_op_symv: one part -> a missed slot shows as NaN)
  std::vector<double> part(static_cast<size_t>(n));
  for (int32_t r = 0; r < part_count; ++r) {
    ADMM_HIP_TRY(hipMemset(npart, fill, sizeof(double) * plan.npart_elems()));
    ADMM_HIP_TRY(hipMemset(tpart, fill, sizeof(double) * plan.tpart_elems()));
    if (fin) launch_symv_lower_fin(plan, dC, dx, npart, tpart, FinArgs{}, false, ctrl, nullptr, r, part_count, dy);
    else launch_symv_lower(plan, dC, 0, dx, npart, tpart, dy, ctrl, nullptr, r, part_count);
    ADMM_HIP_TRY(hipDeviceSynchronize());
    ADMM_HIP_TRY(hipMemcpy(r == 0 ? y : part.data(), dy, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (r > 0)
      for (int64_t i = 0; i < n; ++i) y[i] += part[i];
  }
  if (Q) {  // tile (bi, bj) of the packed triangle -> Q's lower triangle, mirrored
    std::vector<double> P(symv_packed_elems(plan));
    ADMM_HIP_TRY(hipMemcpy(P.data(), dQ, sizeof(double) * P.size(), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = j; i < n; ++i) {
        const int64_t bi = i / 128, bj = j / 128, t = bi * (bi + 1) / 2 + bj;
        const double v = P[static_cast<size_t>(t) * 128 * 128 + (j % 128) * 128 + (i % 128)];
        Q[i + j * ldQ] = v;
        Q[j + i * ldQ] = v;
      }
  }
  return ADMM_OK;
}

int admm_op_symv_batch(const double* Ms, int64_t n, int64_t ldM, int32_t K, const double* X, int64_t ldX,
                       int64_t ncached, double* Y, int64_t ldY) {
  if (!Ms || !X || !Y || n <= 0 || ldM < n || K < 1 || ldX < n || ldY < n || ncached < -1)
    return fail(ADMM_E_INVALID, "symv_batch: bad argument (K >= 1, ncached >= -1)");
  ADMM_TRY(need_device());
  Scratch sc;
  SymvPlan plan = symv_plan(n);
  if (ncached >= 0) plan.ncached = ncached;
  plan.packed = true;
  const int64_t npad = plan.npad;
  const size_t pelems = symv_packed_elems(plan), pstride = plan.npart_elems();
  double *dM, *dP, *dX, *dY, *npart, *tpart;
  const double** dptr;  // the K matrix pointers of the batched launch
  ADMM_TRY(sc.alloc(&dM, static_cast<size_t>(npad) * npad));
  ADMM_TRY(sc.alloc(&dP, pelems * K));
  ADMM_TRY(sc.alloc(&dptr, K));
  ADMM_TRY(sc.alloc(&dX, static_cast<size_t>(npad) * K));
  ADMM_TRY(sc.alloc(&dY, static_cast<size_t>(npad) * K));
  ADMM_TRY(sc.alloc(&npart, pstride * K));
  ADMM_TRY(sc.alloc(&tpart, pstride * K));
  ADMM_HIP_TRY(hipMemset(dM, 0, sizeof(double) * npad * npad));
  ADMM_HIP_TRY(hipMemset(dX, 0, sizeof(double) * npad * K));
  ADMM_HIP_TRY(hipMemset(npart, 0xFF, sizeof(double) * pstride * K));  // (as in admm_op_symv: one part)
  ADMM_HIP_TRY(hipMemset(tpart, 0xFF, sizeof(double) * pstride * K));
  std::vector<const double*> ptrs(static_cast<size_t>(K));
  for (int32_t k = 0; k < K; ++k) {
    ADMM_TRY(put_padded(dM, npad, Ms + static_cast<size_t>(k) * ldM * n, n, ldM));
    launch_symv_pack(plan, dM, npad, dP + pelems * k, nullptr);
    ADMM_HIP_TRY(hipDeviceSynchronize());  // dM is overwritten by the next slice
    ptrs[k] = dP + pelems * k;
  }
  ADMM_HIP_TRY(hipMemcpy(dptr, ptrs.data(), sizeof(const double*) * K, hipMemcpyHostToDevice));
  ADMM_HIP_TRY(hipMemcpy2D(dX, npad * sizeof(double), X, ldX * sizeof(double), n * sizeof(double), K,
                           hipMemcpyHostToDevice));
  launch_symv_lower_batch(plan, dptr, K, dX, npad, npart, tpart,
                          static_cast<int64_t>(pstride), nullptr, nullptr, nullptr);
  for (int32_t k = 0; k < K; ++k)
    launch_symv_reduce(plan, npart + pstride * k, tpart + pstride * k, dY + npad * k, nullptr, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy2D(Y, ldY * sizeof(double), dY, npad * sizeof(double), n * sizeof(double), K,
                           hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_gemm(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
                 int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int32_t lower_only) {
  const bool flags_ok = (transA == 0 || transA == 1) && (transB == 0 || transB == 1) && (lower_only == 0 || lower_only == 1);
  if (!A || !B || !C || !flags_ok || M <= 0 || N <= 0 || K < 1 || lda < (transA ? K : M) || ldb < (transB ? N : K) ||
      ldc < M || (lower_only && M != N))
    return fail(ADMM_E_INVALID, "gemm: bad argument (K >= 1, ld >= stored rows, lower_only needs a square C)");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dA, *dB, *dC;
  ADMM_TRY(put_verbatim(sc, &dA, A, transA ? K : M, transA ? M : K, lda));
  ADMM_TRY(put_verbatim(sc, &dB, B, transB ? N : K, transB ? K : N, ldb));
  ADMM_TRY(sc.alloc(&dC, static_cast<size_t>(ldc) * N));
  ADMM_HIP_TRY(hipMemcpy(dC, C, sizeof(double) * ldc * N, hipMemcpyHostToDevice));
  launch_gemm(transA, transB, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc, lower_only != 0, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy(C, dC, sizeof(double) * ldc * N, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_trtri(const double* L, int64_t n, int64_t ldL, double* X, int64_t ldX) {
  if (!L || !X || n <= 0 || ldL < n || ldX < n) return fail(ADMM_E_INVALID, "trtri: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dL, *dX, *dinv;
  ADMM_TRY(put_verbatim(sc, &dL, L, n, n, ldL));
  ADMM_TRY(sc.alloc(&dX, static_cast<size_t>(ldX) * n));
  ADMM_HIP_TRY(hipMemset(dX, 0xFF, sizeof(double) * ldX * n));
  ADMM_TRY(sc.alloc(&dinv, static_cast<size_t>(ceil_div(n, 64)) * 64 * 64));
  launch_trtri_diag(dL, n, ldL, dinv, nullptr);
  ADMM_TRY(trtri_lower_from_diag(dL, n, ldL, dinv, dX, ldX, nullptr, true));
  ADMM_HIP_TRY(hipDeviceSynchronize());
  // the whole ldX x n buffer: the launcher clears it, padding rows included (padded storage wants them zero), and no
  // kernel behind the clear may store into those rows
  ADMM_HIP_TRY(hipMemcpy(X, dX, sizeof(double) * ldX * n, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_op_llt_apply(const double* L, int64_t n, int64_t ldL, const double* x, double* y) {
  if (!L || !x || !y || n <= 0 || ldL < n) return fail(ADMM_E_INVALID, "llt_apply: bad argument");
  ADMM_TRY(need_device());
  Scratch sc;
  double *dL, *dx, *dt, *dy;
  ADMM_TRY(put_verbatim(sc, &dL, L, n, n, ldL));
  ADMM_TRY(sc.alloc(&dx, n));
  ADMM_TRY(sc.alloc(&dt, n));
  ADMM_TRY(sc.alloc(&dy, n));
  ADMM_HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  launch_llt_apply(dL, n, ldL, dx, dt, dy, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_HIP_TRY(hipMemcpy(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

int admm_tv2d_rows_green_taps(double rho) {
  if (!finite_pos(rho)) return fail(ADMM_E_INVALID, "tv2d_rows_green_taps: rho must be finite and > 0");
  return tv2d_rows_green_taps(rho);
}

int admm_tv2d_row_stage(int64_t H, int64_t W, double rho) {
  if (H <= 0 || W <= 0 || !finite_pos(rho)) return fail(ADMM_E_INVALID, "tv2d_row_stage: bad argument");
  if (!tv2d_height_ok(H)) return ADMM_TV2D_ROWS_AUTO;  // no column transform: the x-update is CG, there is no row stage
  return static_cast<int>(tv2d_row_stage(H, W, rho, dct_length_ok(W)));
}

int admm_dct_tables(int64_t n, double* tw, double* c4, double* lam, double* chirp, double* hbr, int64_t counts[5]) {
  if (!counts || !tv2d_height_ok(n)) return fail(ADMM_E_INVALID, "dct_tables: n has no transform, or counts is null");
  const bool ch = !dct_length_ok(n);
  const int32_t L = static_cast<int32_t>(n), M = ch ? dct_chirp_fft_length(n) : L;
  counts[0] = M / 2;
  counts[1] = ch ? L : L / 2 + 1;
  counts[2] = L;
  counts[3] = ch ? L : 0;
  counts[4] = ch ? M : 0;
  if (!tw) return ADMM_OK;
  if (!c4 || !lam || (ch && (!chirp || !hbr))) return fail(ADMM_E_INVALID, "dct_tables: a table pointer is null");
  if (ch)
    dct_fill_chirp_tables(L, reinterpret_cast<admm_double2*>(tw), reinterpret_cast<admm_double2*>(c4), lam,
                          reinterpret_cast<admm_double2*>(chirp), reinterpret_cast<admm_double2*>(hbr));
  else
    dct_fill_tables(L, reinterpret_cast<admm_double2*>(tw), reinterpret_cast<admm_double2*>(c4), lam);
  return ADMM_OK;
}

int admm_op_dct_cols(const double* img, int64_t H, int64_t W, int32_t inverse, double* out) {
  if (!img || !out || H <= 0 || W <= 0 || !tv2d_height_ok(H) || (inverse != 0 && inverse != 1))
    return fail(ADMM_E_INVALID, "dct_cols: bad argument (H a power of two in 8..8192 or any other length in 8..4096, W >= 1)");
  ADMM_TRY(need_device());
  Scratch sc;
  TableMem tm;
  DctTables th{};
  ADMM_TRY(dct_tables_create(tm.mem, nullptr, H, &th));
  Ctrl* ctrl;
  ADMM_TRY(zeroed_ctrl(sc, &ctrl));
  double *dimg, *dout = nullptr;
  ADMM_TRY(guarded_image(sc, &dimg, H, W));
  ADMM_TRY(put_image(dimg, img, H, W));
  if (inverse) {
    ADMM_TRY(guarded_image(sc, &dout, H, W));
    launch_dct_cols_inverse(dimg, dout, H, W, th, ctrl, nullptr);
  } else {
    launch_dct_cols_forward(dimg, H, W, th, ctrl, nullptr);
  }
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_TRY(guards_intact(dimg, H, W, "dct_cols"));
  if (inverse) ADMM_TRY(guards_intact(dout, H, W, "dct_cols"));
  return get_image(out, inverse ? dout : dimg, H, W);
}

int admm_op_tv2d_rows(const double* src, int64_t H, int64_t W, double rho, int32_t form, double* out) {
  if (!src || !out) return fail(ADMM_E_INVALID, "tv2d_rows: null pointer");
  Tv2Rows rows;
  ADMM_TRY(tv2d_op_form("tv2d_rows", H, W, rho, form, &rows));
  ADMM_TRY(need_device());
  Scratch sc;
  TableMem tm;
  DctTables th{}, tw{};
  ADMM_TRY(dct_tables_create(tm.mem, nullptr, H, &th));  // (lamH comes from the column tables)
  Ctrl* ctrl;
  ADMM_TRY(zeroed_ctrl(sc, &ctrl));
  double *dsrc, *ddst;
  ADMM_TRY(guarded_image(sc, &dsrc, H, W));
  ADMM_TRY(guarded_image(sc, &ddst, H, W));
  ADMM_TRY(put_image(dsrc, src, H, W));
  const double* result = ddst;
  switch (rows) {
    case Tv2Rows::GREEN:
    case Tv2Rows::COOP:
      launch_tv2d_rows_green(dsrc, ddst, H, W, rho, th, ctrl, nullptr, nullptr, false, rows);
      break;
    case Tv2Rows::DCT:  // (in place)
      ADMM_TRY(dct_tables_create(tm.mem, nullptr, W, &tw));
      launch_dct_rows_solve_strided(dsrc, H, W, rho, th, tw, ctrl, nullptr);
      result = dsrc;
      break;
    default: {
      double *cp, *inv;
      ADMM_TRY(sc.alloc(&cp, static_cast<size_t>(H) * W));
      ADMM_TRY(sc.alloc(&inv, static_cast<size_t>(H) * W));
      launch_tv2d_rows_thomas_setup(H, W, rho, th, cp, inv, nullptr);
      launch_tv2d_rows_thomas(dsrc, ddst, H, W, rho, cp, inv, ctrl, nullptr);
      break;
    }
  }
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_TRY(guards_intact(dsrc, H, W, "tv2d_rows"));
  ADMM_TRY(guards_intact(ddst, H, W, "tv2d_rows"));
  return get_image(out, result, H, W);
}

int admm_op_tv2d_xsolve(const double* b, int64_t H, int64_t W, double rho, int32_t form, double* x) {
  if (!b || !x) return fail(ADMM_E_INVALID, "tv2d_xsolve: null pointer");
  Tv2Rows rows;
  ADMM_TRY(tv2d_op_form("tv2d_xsolve", H, W, rho, form, &rows));
  ADMM_TRY(need_device());
  Scratch sc;
  TableMem tm;
  DctTables th{}, tw{};
  ADMM_TRY(dct_tables_create(tm.mem, nullptr, H, &th));
  if (rows == Tv2Rows::DCT) ADMM_TRY(dct_tables_create(tm.mem, nullptr, W, &tw));
  Ctrl* ctrl;
  ADMM_TRY(zeroed_ctrl(sc, &ctrl));
  double *dy, *dx, *cp = nullptr, *inv = nullptr;
  ADMM_TRY(guarded_image(sc, &dy, H, W));
  ADMM_TRY(guarded_image(sc, &dx, H, W));
  ADMM_TRY(put_image(dy, b, H, W));
  if (rows == Tv2Rows::THOMAS) {
    ADMM_TRY(sc.alloc(&cp, static_cast<size_t>(H) * W));
    ADMM_TRY(sc.alloc(&inv, static_cast<size_t>(H) * W));
    launch_tv2d_rows_thomas_setup(H, W, rho, th, cp, inv, nullptr);
  }
  launch_tv2d_xsolve(dy, dx, H, W, rho, rows, th, tw, cp, inv, ctrl, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  ADMM_TRY(guards_intact(dy, H, W, "tv2d_xsolve"));
  ADMM_TRY(guards_intact(dx, H, W, "tv2d_xsolve"));
  return get_image(x, dx, H, W);
}

int admm_op_consensus_tail(int32_t form, int64_t n, int32_t K, int32_t Ntot, double rho, double lambda,
                           const double* rows, double* X, double* U, const double* Dts, double* xave, double* ubar,
                           const double* remote, int32_t with_q, double* Y, double* sums, double* z, double* xaveprev,
                           double* slots, double* q) {
  if (form < 0 || form > 2 || n < 1 || K < 1 || Ntot < K || !finite_pos(rho) || !finite_nonneg(lambda) ||
      (with_q != 0 && with_q != 1))
    return fail(ADMM_E_INVALID, "consensus_tail: bad argument (form 0..2, n >= 1, 1 <= K <= Ntot, rho finite and > 0, "
                                "lambda finite and >= 0, with_q 0 or 1)");
  if (!X || !U || !Dts || !xave || !ubar || !Y || !sums || !z || !xaveprev || !slots || (form != 0 && !rows) ||
      (with_q && !q))
    return fail(ADMM_E_INVALID, "consensus_tail: null pointer");
  if (static_cast<int64_t>(K) > (int64_t{1} << 40) / n)
    return fail(ADMM_E_INVALID, "consensus_tail: K * n is too large");
  const int64_t ldn = round_up(n, 2);  // the engine's cldn
  ConsArgs ca{};
  ca.n = n;
  ca.ldn = ldn;
  ca.K = K;
  ca.Ntot = Ntot;
  ca.rho = rho;
  ca.lambda = lambda;
  if (form == 2 && (!cons_gather_update_ok(ca) || remote || with_q))
    return fail(ADMM_E_INVALID, "consensus_tail: the one-launch tail takes at most 16 slices, no remote share and no q");
  ADMM_TRY(need_device());
  Scratch sc;
  const SymvPlan plan = symv_plan(n);
  const int32_t P = plan.ntile + 1;
  const size_t pstride = plan.npart_elems(), vec = static_cast<size_t>(K) * ldn;
  const int nqmax = static_cast<int>(ceil_div(n, 128) > kMaxPartBlocks ? ceil_div(n, 128) : kMaxPartBlocks);
  double *dX, *dU, *dDts, *dY, *dsums, *dz, *dxave, *dxprev, *dubar, *dpart, *dqpart, *dslots, *npart = nullptr,
         *tpart = nullptr;
  Ctrl* ctrl;
  ADMM_TRY(zeroed_ctrl(sc, &ctrl));
  // [K][ldn] and one guard row behind the last slice, all-ones bytes: the padding column of an odd n and the guard row
  // must come back as they were (below)
  for (double** p : {&dX, &dU, &dDts, &dY}) {
    ADMM_TRY(sc.alloc(p, vec + ldn));
    ADMM_HIP_TRY(hipMemset(*p, 0xFF, sizeof(double) * (vec + ldn)));
  }
  for (double** p : {&dz, &dxave, &dxprev, &dubar}) {
    ADMM_TRY(sc.alloc(p, ldn));
    ADMM_HIP_TRY(hipMemset(*p, 0xFF, sizeof(double) * ldn));
  }
  ADMM_TRY(sc.alloc(&dsums, 2 * ldn + 2));
  ADMM_TRY(sc.alloc(&dpart, static_cast<size_t>(S_COUNT) * kMaxPartBlocks));
  ADMM_TRY(sc.alloc(&dqpart, nqmax));
  ADMM_TRY(sc.alloc(&dslots, 5));
  ADMM_HIP_TRY(hipMemset(dsums, 0xFF, sizeof(double) * (2 * ldn + 2)));
  ADMM_HIP_TRY(hipMemset(dpart, 0xFF, sizeof(double) * S_COUNT * kMaxPartBlocks));  // a block past nblk reads as NaN
  ADMM_HIP_TRY(hipMemset(dqpart, 0xFF, sizeof(double) * nqmax));
  const size_t hrow = n * sizeof(double), drow = ldn * sizeof(double);
  if (form == 0) ADMM_HIP_TRY(hipMemcpy2D(dX, drow, X, hrow, hrow, K, hipMemcpyHostToDevice));
  ADMM_HIP_TRY(hipMemcpy2D(dU, drow, U, hrow, hrow, K, hipMemcpyHostToDevice));
  ADMM_HIP_TRY(hipMemcpy2D(dDts, drow, Dts, hrow, hrow, K, hipMemcpyHostToDevice));
  ADMM_HIP_TRY(hipMemcpy(dxave, xave, hrow, hipMemcpyHostToDevice));
  ADMM_HIP_TRY(hipMemcpy(dubar, ubar, hrow, hipMemcpyHostToDevice));
  if (form != 0) {
    // logical row p of element i where the lower-triangle x-solve leaves it: npart row p for p <= i / 128 (the tile
    // row of i), tpart row p - 1 otherwise; every other double of both buffers is the all-ones NaN
    // (one more row of it in front of either buffer: a T-part row index of -1 stays inside the allocation)
    const size_t lead = static_cast<size_t>(plan.ldp);
    std::vector<double> hn(lead + pstride * K), ht(lead + pstride * K);
    std::memset(hn.data(), 0xFF, sizeof(double) * hn.size());
    std::memset(ht.data(), 0xFF, sizeof(double) * ht.size());
    for (int32_t k = 0; k < K; ++k)
      for (int32_t p = 0; p < P; ++p) {
        const double* src = rows + (static_cast<size_t>(k) * P + p) * n;
        double* drn = hn.data() + lead + pstride * k + static_cast<size_t>(p) * plan.ldp;
        double* drt = ht.data() + lead + pstride * k + static_cast<size_t>(p > 0 ? p - 1 : 0) * plan.ldp;
        for (int64_t i = 0; i < n; ++i) {
          if (p <= i / 128) drn[i] = src[i];
          else drt[i] = src[i];
        }
      }
    ADMM_TRY(sc.put(&npart, static_cast<const double*>(hn.data()), hn.size()));
    ADMM_TRY(sc.put(&tpart, static_cast<const double*>(ht.data()), ht.size()));
    npart += lead;
    tpart += lead;
  }
  ca.sums = dsums;
  ca.X = dX;
  ca.U = dU;
  ca.zc = dz;
  ca.xave = dxave;
  ca.xaveprev = dxprev;
  ca.ubar = dubar;
  ca.part = dpart;
  ca.Dts = dDts;
  ca.Y = dY;
  int nblk = 0;
  if (form == 2) {
    launch_cons_gather_update(ca, npart, tpart, static_cast<int64_t>(pstride), plan.ldp, plan.ntile, ctrl, &nblk, nullptr);
  } else {
    const double* center = with_q ? dxave : nullptr;  // the sharded run: q about the mean every rank already holds
    double* qp = with_q ? dqpart : nullptr;
    const int nq = form == 1 ? launch_cons_gather_sum(n, ldn, K, npart, tpart, static_cast<int64_t>(pstride), plan.ldp,
                                                      plan.ntile, dX, dU, dsums, center, qp, ctrl, nullptr)
                             : launch_cons_sum(n, ldn, K, dX, dU, dsums, center, qp, ctrl, nullptr);
    if (with_q) launch_pack_sum(dqpart, nq, dsums + 2 * ldn, ctrl, nullptr);
    if (remote) {  // the other ranks' share of the all-reduce: test harness, not a kernel under test
      std::vector<double> hs(static_cast<size_t>(2 * ldn));
      ADMM_HIP_TRY(hipDeviceSynchronize());
      ADMM_HIP_TRY(hipMemcpy(hs.data(), dsums, sizeof(double) * 2 * ldn, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < n; ++i) {
        hs[i] += remote[i];
        hs[ldn + i] += remote[n + i];
      }
      ADMM_HIP_TRY(hipMemcpy(dsums, hs.data(), sizeof(double) * 2 * ldn, hipMemcpyHostToDevice));
    }
    launch_cons_update(ca, ctrl, &nblk, nullptr);
  }
  static const int kSlots[5] = {S_R2, S_AX2, S_G2, S_U2, S_DU2};
  for (int j = 0; j < 5; ++j)  // the nblk block partials of a slot, where the finalize step reads them
    launch_pack_sum(dpart + static_cast<size_t>(kSlots[j]) * kMaxPartBlocks, nblk, dslots + j, ctrl, nullptr);
  ADMM_HIP_TRY(hipDeviceSynchronize());
  {  // nothing stored past the n elements of a slice
    std::vector<uint64_t> h(vec + ldn);
    for (const double* d : {dX, dU, dY}) {
      ADMM_HIP_TRY(hipMemcpy(h.data(), d, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
      for (size_t j = 0; j < h.size(); ++j)
        if ((j >= vec || static_cast<int64_t>(j % ldn) >= n) && h[j] != ~uint64_t{0})
          return fail(ADMM_E_NUMERIC, "consensus_tail: a kernel wrote outside the n elements of a slice");
    }
  }
  ADMM_HIP_TRY(hipMemcpy2D(X, hrow, dX, drow, hrow, K, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy2D(U, hrow, dU, drow, hrow, K, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy2D(Y, hrow, dY, drow, hrow, K, hipMemcpyDeviceToHost));
  if (form != 2) ADMM_HIP_TRY(hipMemcpy2D(sums, hrow, dsums, drow, hrow, 2, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(z, dz, hrow, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(xave, dxave, hrow, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(xaveprev, dxprev, hrow, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(ubar, dubar, hrow, hipMemcpyDeviceToHost));
  ADMM_HIP_TRY(hipMemcpy(slots, dslots, sizeof(double) * 5, hipMemcpyDeviceToHost));
  if (with_q) ADMM_HIP_TRY(hipMemcpy(q, dsums + 2 * ldn, sizeof(double), hipMemcpyDeviceToHost));
  return ADMM_OK;
}

}  // extern "C"
