// multi_host.h -- the host scaffold of the "K runs over one D" solvers (svm_ovr.hip, reg_multi.hip, sparse_svm.hip,
// sparse_reg.hip, sparse_lasso.hip): the part of an object every one of them has, the option refusals and defaults, the
// histories, the poll of the per-fit records, the bookkeeping around a run and the teardown; the frame of the C ABI
// around an object -- the create-time checks of a sparse D, of the response columns and of the placement, the tail of
// create, the head of fetch, the gated histories, and the end of a run and the destroy of the sparse three; and what only
// a pair shares: the regression's fit parameters and weights, the SVM's cost plan, the dense pair's n x n x-update.
// A solver keeps its kernels, its argument blocks, the create-time checks of its own fields and the body of its
// iteration loop.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "multi_device.h"

namespace admm {

struct MultiHost {
  hipStream_t stream = nullptr;
  DevMem mem;
  int device = 0;
  int32_t K = 0;
  MultiRec* rec = nullptr;
  MultiRec* rec_host = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int32_t hist_ld = 0;  // histories of the last run: [K][hist_ld]
  bool has_run = false;
  std::vector<int32_t> steps;
};

// `count` zeroed values of a type that is no double, out of the object's allocator
template <class T>
int alloc_words(MultiHost& h, T** out, size_t count) {
  double* raw = nullptr;
  ADMM_TRY(h.mem.alloc(&raw, (count * sizeof(T) + 7) / 8));
  ADMM_HIP_TRY(hipMemsetAsync(raw, 0, (count * sizeof(T) + 7) / 8 * 8, h.stream));
  *out = reinterpret_cast<T*>(raw);
  return ADMM_OK;
}

// the records, their pinned mirror and the two events (stream and K are set)
int alloc_common(MultiHost& h);
// the first half of every destroy: the stream drained, the events, every device allocation and the pinned mirror freed.
// What owns the stream (the engine, or the object itself) goes after it.
void destroy_common(MultiHost& h);

// what no multi-fit loop runs, in its own words: "<feature> is not part of the <label> loop<suffix>"
template <class Options>
int check_run_options(const char* label, const char* suffix, Options* op) {
  const std::string tail = std::string(" is not part of the ") + label + " loop" + suffix;
  if (op->fast != ADMM_FAST_OFF) return fail(ADMM_E_UNSUPPORTED, "fast / accelerated ADMM" + tail);
  if (op->relax != 1.0) return fail(ADMM_E_UNSUPPORTED, "relaxation" + tail);
  if (op->convtest) return fail(ADMM_E_UNSUPPORTED, "convtest" + tail);
  if (!(op->rho > 0.0)) return fail(ADMM_E_INVALID, "options.rho must be positive");
  if (op->maxiters <= 0) op->maxiters = 1000;  // admm.m:334-339
  if (op->check_every <= 0) op->check_every = op->domaxiters ? 64 : 8;  // iterations between two polls of the records
  return ADMM_OK;
}
// the same for the sparse three, whose loop names carry no suffix, and the bounds of a CG solve left open
template <class Options>
int check_sparse_run_options(const char* label, Options* op) {
  ADMM_TRY(check_run_options(label, "", op));
  if (!(op->cg_tol > 0.0)) op->cg_tol = 1e-12;
  if (op->cg_maxit <= 0) op->cg_maxit = 200;
  return ADMM_OK;
}

// every history [K][N]: reallocated when N is not the last run's
int resize_histories(MultiHost& h, std::initializer_list<double**> hist, int32_t N);
// [K][S] with S = the most steps of a fit; a fit's entries past its own steps are NaN
int fetch_history(const MultiHost& h, const double* src, double* dst, size_t cap, size_t* written);
// has_run off and the records zeroed: a run starts
int begin_run(MultiHost& h);
int begin_timing(MultiHost& h);
int poll_all_stopped(MultiHost& h, bool* all_stopped);
// the end of a run: drains the stream, refuses with `unfinished` if a fit is still running, then the elapsed time, the
// steps and, per fit, the objective at its last step (NaN without objevals)
int finish_run_core(MultiHost& h, bool all_stopped, const char* unfinished, int32_t N, bool objevals, const double* objv,
                    double* runtime_s, std::vector<double>* objopt);
template <class Summary>
int finish_run(MultiHost& h, bool all_stopped, const char* unfinished, int32_t N, bool objevals, const double* objv,
               double* runtime_s, Summary* summaries) {
  std::vector<double> objopt;
  ADMM_TRY(finish_run_core(h, all_stopped, unfinished, N, objevals, objv, runtime_s, &objopt));
  for (int32_t c = 0; summaries && c < h.K; ++c) {
    summaries[c].steps = h.rec_host[c].steps;
    summaries[c].stopped_early = h.rec_host[c].early;
    summaries[c].objopt = objopt[c];
  }
  return ADMM_OK;
}

// ---- the frame of the C ABI around an object
// D of a sparse object: "<who> needs D (admm_sparse_desc)", "<who> takes D in host arrays", then the CSC rules
int check_sparse_D(const char* who, const admm_sparse_desc* D);
// "S has <ns> columns: one shared response or one per fit (<K>)"
int check_response_columns(int32_t ns, int32_t K);
// the last checks of a sparse create, so that every refusal above them needs no device: "<who> is not row-sharded", a
// visible device and the ordinal
int check_placement(const char* who, const admm_comm* comm, int device);
// the tail of every create: a new object, its setup, and on failure the object destroyed behind the setup's own message
template <class Obj, class Setup>
int create_object(Obj** out, void (*destroy)(Obj*), Setup setup) {
  Obj* o = new Obj();
  const int rc = setup(o);
  if (rc != ADMM_OK) {
    const std::string msg = admm_last_error();
    destroy(o);
    return fail(rc, msg);
  }
  *out = o;
  return ADMM_OK;
}
// the end of a sparse run behind finish_run: the CG counters, and the options fetch consults
template <class Obj, class Options, class Summary>
int end_sparse_run(Obj* o, const Options& op, Summary* summaries) {
  ADMM_TRY(o->cg.fill_counters(summaries, o->K));
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}
template <class Obj>
void destroy_sparse(Obj* o) {  // (SpmmCg::destroy is the whole teardown of its host)
  if (!o) return;
  o->cg.destroy();
  delete o;
}
// the head of every fetch: the object and dst given, a run behind it, its device current
int fetch_head(const MultiHost* h, const double* dst);
// a history the last run kept only with `kept`; otherwise ADMM_E_INVALID with `refusal`
constexpr const char* kNoObjevals = "the last run did not evaluate the objective (objevals = 0)";
constexpr const char* kNoDual = "the last run did not evaluate the dual residual (nodualerror = 1)";
int fetch_kept_history(const MultiHost& h, bool kept, const char* refusal, const double* src, double* dst, size_t cap,
                       size_t* written);

// ---- the regression pair
// per fit, exactly as admm_engine_set_loss checks it: kh[k] the kind, ph[4k ..] = (a, b, epsilon, delta)
int check_reg_fits(int32_t K, const int32_t* kind, const double* a, const double* b, const double* epsilon,
                   const double* delta, std::vector<int32_t>* kh, std::vector<double>* ph);
// *W <- m shared weights on the device, or null: every weight is 1 again.  A refused call changes nothing
int set_shared_weights(MultiHost& h, int64_t m, const double* weights, double** W);

// ---- the SVM pair
int check_svm_losses(int32_t K, const int32_t* loss);
// which chunks run the cost form of the element update: the squared hinge lives there alone, and so does every cost
std::vector<int32_t> svm_cost_chunks(int32_t K, int chunk, bool weights, const std::vector<int32_t>& loss,
                                     const std::vector<double>& cost);
// *W, CC (K x 2 on the device) and cost_host from the caller's arrays; null restores ones.  A refused call changes
// nothing; the caller plans its chunks again behind it
int set_svm_cost(MultiHost& h, int64_t m, const double* weights, const double* class_cost, double** W, double* CC,
                 std::vector<double>* cost_host);

// ---- the classifier pair (l1class.hip, sparse_l1class.hip): the create-time checks of the fields both descs carry, each
// refusal ADMM_E_INVALID with the fit, the label or the index named
// per fit the loss (hinge, sqhinge or logistic; null = logistic), lambda, ridge (null = 0) and nonneg (null = 0):
// lh[k] the loss, ph[2k ..] = (lambda, mu), nh[k] = nonneg
int check_l1class_fits(int32_t K, const int32_t* loss, const double* lambda, const double* ridge, const int32_t* nonneg,
                       std::vector<int32_t>* lh, std::vector<double>* ph, std::vector<int32_t>* nh);
// "label <row> of column <col> is neither +1 nor -1"
int check_labels(const double* ELL, int64_t m, int32_t nell);
// "penalty: weight <i> is negative or not finite" (null passes)
int check_l1_weights(const double* l1weights, int64_t n);

// ---- the dense pair: D and the factor of D'D belong to an ordinary engine that never runs
struct DenseMulti : MultiHost {
  admm_engine* eng = nullptr;  // stream = eng->stream
  int64_t m = 0, n = 0, ldx = 0, ldz = 0;
  int32_t nwg = 0;
  const double* M = nullptr;  // the explicit symmetric n x n map of the x-update; null: triangular solves
  int64_t ldM = 0;
  double *X = nullptr, *Z = nullptr, *U = nullptr, *gpart = nullptr, *gsum = nullptr, *part = nullptr, *xtmp = nullptr;
};
// behind admm_engine_create(&d.eng): the sizes, M (unless the caller has set one), X, Z, U, the partial rows, the
// nslots block partials per fit and MultiHost's own
int dense_setup(DenseMulti& d, int64_t m, int64_t n, int32_t K, int nslots, const char* suffix);
int dense_start(DenseMulti& d, const double* x0, const double* z0, const double* u0);  // begin_run and the start vectors
// X(:, k) = M gsum(:, k), or the triangular solves, for every running fit; returns the number of launches
int dense_xupdate(DenseMulti& d);
int upload_cols(MultiHost& h, double* dst, int64_t ld, const double* src, int64_t rows, int32_t cols, int kind);
int fetch_cols(const MultiHost& h, const double* src, int64_t ld, int64_t rows, double* dst, size_t cap, size_t* written);
void dense_destroy(DenseMulti& d);

}  // namespace admm
