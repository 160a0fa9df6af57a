// multi_host.hip -- the host scaffold of the multi-fit solvers (multi_host.h).
#include "multi_host.h"

#include "spmv.h"
#include "svm_ovr.h"

namespace admm {

int alloc_common(MultiHost& h) {
  ADMM_TRY(alloc_words(h, &h.rec, static_cast<size_t>(h.K)));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h.rec_host), sizeof(MultiRec) * h.K));
  ADMM_HIP_TRY(hipEventCreate(&h.ev0));
  ADMM_HIP_TRY(hipEventCreate(&h.ev1));
  return ADMM_OK;
}

void destroy_common(MultiHost& h) {
  (void)hipSetDevice(h.device);
  if (h.stream) (void)hipStreamSynchronize(h.stream);
  if (h.ev0) (void)hipEventDestroy(h.ev0);
  if (h.ev1) (void)hipEventDestroy(h.ev1);
  h.mem.release();
  if (h.rec_host) (void)hipHostFree(h.rec_host);
}

int resize_histories(MultiHost& h, std::initializer_list<double**> hist, int32_t N) {
  if (h.hist_ld == N) return ADMM_OK;
  for (double** p : hist) {
    h.mem.free_one(*p);
    *p = nullptr;
    ADMM_TRY(h.mem.alloc(p, static_cast<size_t>(N) * h.K));
  }
  h.hist_ld = N;
  return ADMM_OK;
}

int fetch_history(const MultiHost& h, const double* src, double* dst, size_t cap, size_t* written) {
  const int32_t K = h.K;
  int32_t S = 0;
  for (int32_t s : h.steps) S = s > S ? s : S;
  const size_t need = static_cast<size_t>(S) * K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  if (S > 0)
    ADMM_HIP_TRY(hipMemcpy2D(dst, S * sizeof(double), src, h.hist_ld * sizeof(double), S * sizeof(double), K,
                             hipMemcpyDeviceToHost));
  for (int32_t c = 0; c < K; ++c)
    for (int32_t i = h.steps[c]; i < S; ++i) dst[static_cast<size_t>(c) * S + i] = __builtin_nan("");
  if (written) *written = need;
  return ADMM_OK;
}

int begin_run(MultiHost& h) {
  h.has_run = false;
  ADMM_HIP_TRY(hipMemsetAsync(h.rec, 0, sizeof(MultiRec) * h.K, h.stream));
  return ADMM_OK;
}

int begin_timing(MultiHost& h) {
  ADMM_HIP_TRY(hipEventRecord(h.ev0, h.stream));
  return ADMM_OK;
}

int poll_all_stopped(MultiHost& h, bool* all_stopped) {
  ADMM_HIP_TRY(hipMemcpyAsync(h.rec_host, h.rec, sizeof(MultiRec) * h.K, hipMemcpyDeviceToHost, h.stream));
  ADMM_HIP_TRY(hipStreamSynchronize(h.stream));
  bool all = true;
  for (int32_t c = 0; c < h.K; ++c) all = all && h.rec_host[c].stop != 0;
  *all_stopped = all;
  return ADMM_OK;
}

int finish_run_core(MultiHost& h, bool all_stopped, const char* unfinished, int32_t N, bool objevals, const double* objv,
                    double* runtime_s, std::vector<double>* objopt) {
  const int32_t K = h.K;
  ADMM_HIP_TRY(hipEventRecord(h.ev1, h.stream));
  ADMM_HIP_TRY(hipStreamSynchronize(h.stream));
  ADMM_HIP_TRY(hipGetLastError());
  if (!all_stopped) return fail(ADMM_E_DEVICE, unfinished);
  float ms = 0.f;
  ADMM_HIP_TRY(hipEventElapsedTime(&ms, h.ev0, h.ev1));
  if (runtime_s) *runtime_s = 1e-3 * static_cast<double>(ms);
  h.steps.assign(static_cast<size_t>(K), 0);
  std::vector<double> objh;
  if (objevals) {
    objh.resize(static_cast<size_t>(N) * K);
    ADMM_HIP_TRY(hipMemcpy(objh.data(), objv, sizeof(double) * N * K, hipMemcpyDeviceToHost));
  }
  objopt->assign(static_cast<size_t>(K), __builtin_nan(""));
  for (int32_t c = 0; c < K; ++c) {
    const MultiRec& r = h.rec_host[c];
    h.steps[c] = r.steps;
    if (objevals && r.steps > 0) (*objopt)[c] = objh[static_cast<size_t>(c) * N + r.steps - 1];
  }
  return ADMM_OK;
}

// ------------------------------------------------------------------------------------------- the frame of the C ABI
int check_sparse_D(const char* who, const admm_sparse_desc* D) {
  if (!D) return fail(ADMM_E_INVALID, std::string(who) + " needs D (admm_sparse_desc)");
  if (D->mem != ADMM_MEM_HOST) return fail(ADMM_E_INVALID, std::string(who) + " takes D in host arrays");
  return sparse_csc_check(D);
}

int check_response_columns(int32_t ns, int32_t K) {
  if (ns != 1 && ns != K)
    return fail(ADMM_E_INVALID, "S has " + std::to_string(ns) + " columns: one shared response or one per fit (" +
                                    std::to_string(K) + ")");
  return ADMM_OK;
}

int check_placement(const char* who, const admm_comm* comm, int device) {
  if (comm) return fail(ADMM_E_UNSUPPORTED, std::string(who) + " is not row-sharded");
  int ndev = 0;
  ADMM_TRY(admm_device_count(&ndev));
  if (ndev <= 0) return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(ADMM_E_INVALID, "bad device ordinal");
  return ADMM_OK;
}

int fetch_head(const MultiHost* h, const double* dst) {
  if (!h || !dst) return fail(ADMM_E_INVALID, "object/dst is NULL");
  if (!h->has_run) return fail(ADMM_E_INVALID, "fetch before the first run");
  ADMM_HIP_TRY(hipSetDevice(h->device));
  return ADMM_OK;
}

int fetch_kept_history(const MultiHost& h, bool kept, const char* refusal, const double* src, double* dst, size_t cap,
                       size_t* written) {
  if (!kept) return fail(ADMM_E_INVALID, refusal);
  return fetch_history(h, src, dst, cap, written);
}

// ---------------------------------------------------------------------------------------------- the regression pair
int check_reg_fits(int32_t K, const int32_t* kind, const double* a, const double* b, const double* epsilon,
                   const double* delta, std::vector<int32_t>* kh, std::vector<double>* ph) {
  kh->assign(static_cast<size_t>(K), 0);
  ph->assign(static_cast<size_t>(4) * K, 0.0);
  for (int32_t k = 0; k < K; ++k) {
    int32_t& kd = (*kh)[k];
    if (kind) kd = kind[k];
    if (kd != 0 && kd != 1)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": kind must be 0 (LAD family) or 1 (Huber family)");
    const admm_loss_desc ld{nullptr, a ? a[k] : 1.0, b ? b[k] : 1.0, epsilon ? epsilon[k] : 0.0, delta ? delta[k] : 1.0};
    if (check_loss_desc(kd ? ADMM_PROB_HUBERFIT : ADMM_PROB_LAD, ld, 0) != ADMM_OK)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": " + std::string(admm_last_error()));
    (*ph)[4 * k + 0] = ld.slope_pos;
    (*ph)[4 * k + 1] = ld.slope_neg;
    (*ph)[4 * k + 2] = ld.epsilon;
    (*ph)[4 * k + 3] = ld.delta;
  }
  return ADMM_OK;
}

int set_shared_weights(MultiHost& h, int64_t m, const double* weights, double** W) {
  if (weights)  // (a refused call changes nothing)
    for (int64_t i = 0; i < m; ++i)
      if (!finite_nonneg(weights[i]))
        return fail(ADMM_E_INVALID, "loss: weight " + std::to_string(i) + " is negative or not finite");
  ADMM_HIP_TRY(hipSetDevice(h.device));
  double* w = nullptr;
  if (weights) {
    ADMM_TRY(h.mem.alloc(&w, static_cast<size_t>(m)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, weights, sizeof(double) * m, hipMemcpyHostToDevice, h.stream));
    ADMM_HIP_TRY(hipStreamSynchronize(h.stream));  // (the caller's buffer is read until here)
  }
  if (*W) h.mem.free_one(*W);
  *W = w;
  return ADMM_OK;
}

// ----------------------------------------------------------------------------------------------------- the SVM pair
int check_svm_losses(int32_t K, const int32_t* loss) {
  if (loss)
    for (int32_t c = 0; c < K; ++c)
      if (loss[c] != ADMM_LOSS_HINGE && loss[c] != ADMM_LOSS_01 && loss[c] != ADMM_LOSS_HINGE_OBJ01 &&
          loss[c] != ADMM_LOSS_LOGISTIC && loss[c] != ADMM_LOSS_SQHINGE)
        return fail(ADMM_E_INVALID, "bad loss for class " + std::to_string(c));
  return ADMM_OK;
}

// ------------------------------------------------------------------------------------------------ the classifier pair
int check_l1class_fits(int32_t K, const int32_t* loss, const double* lambda, const double* ridge, const int32_t* nonneg,
                       std::vector<int32_t>* lh, std::vector<double>* ph, std::vector<int32_t>* nh) {
  lh->assign(static_cast<size_t>(K), ADMM_LOSS_LOGISTIC);
  ph->assign(static_cast<size_t>(2) * K, 0.0);
  nh->assign(static_cast<size_t>(K), 0);
  for (int32_t k = 0; k < K; ++k) {
    const std::string who = "fit " + std::to_string(k) + ": ";
    if (loss) (*lh)[k] = loss[k];
    const int32_t l = (*lh)[k];
    if (l == ADMM_LOSS_01 || l == ADMM_LOSS_HINGE_OBJ01)
      return fail(ADMM_E_INVALID, who + "the 0-1 loss is not convex and has no lambda_max: the l1 classifier takes "
                                        "hinge, sqhinge or logistic");
    if (l != ADMM_LOSS_HINGE && l != ADMM_LOSS_SQHINGE && l != ADMM_LOSS_LOGISTIC)
      return fail(ADMM_E_INVALID, who + "unknown loss (ADMM_LOSS_HINGE, _SQHINGE or _LOGISTIC)");
    (*ph)[2 * k] = lambda[k];
    if (!finite_nonneg((*ph)[2 * k])) return fail(ADMM_E_INVALID, who + "lambda is negative or not finite");
    if (ridge) (*ph)[2 * k + 1] = ridge[k];
    if (!finite_nonneg((*ph)[2 * k + 1])) return fail(ADMM_E_INVALID, who + "ridge is negative or not finite");
    if (nonneg) (*nh)[k] = nonneg[k];
    if ((*nh)[k] != 0 && (*nh)[k] != 1) return fail(ADMM_E_INVALID, who + "nonneg must be 0 or 1");
  }
  return ADMM_OK;
}

int check_labels(const double* ELL, int64_t m, int32_t nell) {
  const int64_t mk = m * static_cast<int64_t>(nell);
  for (int64_t i = 0; i < mk; ++i)
    if (ELL[i] != 1.0 && ELL[i] != -1.0)
      return fail(ADMM_E_INVALID, "label " + std::to_string(i % m) + " of column " + std::to_string(i / m) +
                                      " is neither +1 nor -1");
  return ADMM_OK;
}

int check_l1_weights(const double* l1weights, int64_t n) {
  if (l1weights)
    for (int64_t i = 0; i < n; ++i)
      if (!finite_nonneg(l1weights[i]))
        return fail(ADMM_E_INVALID, "penalty: weight " + std::to_string(i) + " is negative or not finite");
  return ADMM_OK;
}

std::vector<int32_t> svm_cost_chunks(int32_t K, int chunk, bool weights, const std::vector<int32_t>& loss,
                                     const std::vector<double>& cost) {
  std::vector<int32_t> cc(static_cast<size_t>((K + chunk - 1) / chunk), 0);
  for (int32_t c = 0; c < K; ++c)
    if (weights || loss[c] == ADMM_LOSS_SQHINGE || cost[2 * c] != 1.0 || cost[2 * c + 1] != 1.0) cc[c / chunk] = 1;
  return cc;
}

int set_svm_cost(MultiHost& h, int64_t m, const double* weights, const double* class_cost, double** W, double* CC,
                 std::vector<double>* cost_host) {
  ADMM_TRY(check_svm_cost(weights, m, class_cost, 2 * static_cast<int64_t>(h.K)));  // (a refused call changes nothing)
  ADMM_HIP_TRY(hipSetDevice(h.device));
  double* w = nullptr;
  if (weights) {
    ADMM_TRY(h.mem.alloc(&w, static_cast<size_t>(m)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, weights, sizeof(double) * m, hipMemcpyHostToDevice, h.stream));
  }
  std::vector<double> cc(static_cast<size_t>(2 * h.K), 1.0);
  if (class_cost) cc.assign(class_cost, class_cost + 2 * h.K);
  ADMM_HIP_TRY(hipMemcpyAsync(CC, cc.data(), sizeof(double) * 2 * h.K, hipMemcpyHostToDevice, h.stream));
  ADMM_HIP_TRY(hipStreamSynchronize(h.stream));  // (the caller's buffers are read until here)
  if (*W) h.mem.free_one(*W);
  *W = w;
  *cost_host = cc;
  return ADMM_OK;
}

// --------------------------------------------------------------------------------------------------- the dense pair
int upload_cols(MultiHost& h, double* dst, int64_t ld, const double* src, int64_t rows, int32_t cols, int kind) {
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * ld * cols, h.stream));
    return ADMM_OK;
  }
  ADMM_HIP_TRY(hipMemcpy2DAsync(dst, ld * sizeof(double), src, rows * sizeof(double), rows * sizeof(double), cols,
                                kind == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h.stream));
  return ADMM_OK;
}

int fetch_cols(const MultiHost& h, const double* src, int64_t ld, int64_t rows, double* dst, size_t cap, size_t* written) {
  const size_t need = static_cast<size_t>(rows) * h.K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  ADMM_HIP_TRY(hipMemcpy2D(dst, rows * sizeof(double), src, ld * sizeof(double), rows * sizeof(double), h.K,
                           hipMemcpyDeviceToHost));
  if (written) *written = need;
  return ADMM_OK;
}

int dense_setup(DenseMulti& d, int64_t m, int64_t n, int32_t K, int nslots, const char* suffix) {
  admm_engine* e = d.eng;
  d.stream = e->stream;
  d.device = e->device;
  d.m = m;
  d.n = n;
  d.K = K;
  d.ldx = round_up(n, 2);
  d.ldz = round_up(m, 2);
  d.nwg = ovr_pass_workgroups(m);
  if (d.M) {  // the caller's own map
  } else if (e->xfac.mode == ADMM_XSOLVE_INVERSE && e->xfac.Minv && !e->xfac.planSy.packed) {
    d.M = e->xfac.Minv;  // (D'D)^-1, or (D'D)^+ of a rank-deficient D: full symmetric storage below kSymvHalfMin
    d.ldM = e->xfac.ldM;
  } else if (e->xfac.mode == ADMM_XSOLVE_TRSV && e->xfac.F) {
    // create's accuracy probe kept the triangular solves: they run per fit (K small launches), nothing is forced
    ADMM_TRY(d.mem.alloc(&d.xtmp, static_cast<size_t>(d.ldx) * K));
    ADMM_HIP_TRY(hipMemsetAsync(d.xtmp, 0, sizeof(double) * d.ldx * K, d.stream));
  } else {
    return fail(ADMM_E_UNSUPPORTED, std::string("the engine built no n x n form of the x-update for this D") + suffix);
  }
  ADMM_TRY(d.mem.alloc(&d.X, static_cast<size_t>(d.ldx) * K));
  ADMM_TRY(d.mem.alloc(&d.gsum, static_cast<size_t>(d.ldx) * K));
  ADMM_HIP_TRY(hipMemsetAsync(d.gsum, 0, sizeof(double) * d.ldx * K, d.stream));
  ADMM_TRY(d.mem.alloc(&d.Z, static_cast<size_t>(d.ldz) * K));
  ADMM_TRY(d.mem.alloc(&d.U, static_cast<size_t>(d.ldz) * K));
  ADMM_TRY(d.mem.alloc(&d.gpart, static_cast<size_t>(d.nwg) * K * d.ldx));
  ADMM_TRY(d.mem.alloc(&d.part, static_cast<size_t>(K) * nslots * kMultiMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(d.part, 0, sizeof(double) * K * nslots * kMultiMaxWg, d.stream));
  return alloc_common(d);
}

int dense_start(DenseMulti& d, const double* x0, const double* z0, const double* u0) {
  ADMM_TRY(begin_run(d));
  ADMM_TRY(upload_cols(d, d.X, d.ldx, x0, d.n, d.K, ADMM_MEM_HOST));
  ADMM_TRY(upload_cols(d, d.Z, d.ldz, z0, d.m, d.K, ADMM_MEM_HOST));
  ADMM_TRY(upload_cols(d, d.U, d.ldz, u0, d.m, d.K, ADMM_MEM_HOST));
  ADMM_HIP_TRY(hipStreamSynchronize(d.stream));  // (host buffers were read)
  return ADMM_OK;
}

int dense_xupdate(DenseMulti& d) {
  if (d.M) {
    const OvrSolveArgs sa{d.M, d.ldM, d.n, d.gsum, d.X, d.ldx, d.rec};
    launch_ovr_xsolve(sa, d.K, d.stream);
    return 1;
  }
  for (int32_t c = 0; c < d.K; ++c)
    launch_trsv_pair(d.eng->xfac.trsv, d.gsum + static_cast<int64_t>(c) * d.ldx,
                     d.xtmp + static_cast<int64_t>(c) * d.ldx, nullptr, d.stream);
  launch_ovr_xcopy(d.xtmp, d.X, d.ldx, d.n, d.K, d.rec, d.stream);
  return d.K + 1;
}

void dense_destroy(DenseMulti& d) {
  destroy_common(d);
  if (d.eng) admm_engine_destroy(d.eng);
}

}  // namespace admm
