// engine.hip -- what create() (engine_create.hip) builds its engines from: uploads, the cached factor of the x-update
// and the probes that choose how it is applied, the eliminated maps of basis pursuit / LP / QP -- and the rest of the
// C ABI (include/admm_engine.h) around the loop: defaults, result fetch, info, timers, destroy.  The loop itself
// (admm.m:252-767) is engine_run.hip and the engine_run_*.hip files.
#include "engine_internal.h"
#include "loop_kernels.h"

namespace admm {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

EnvSwitches env_switches() {
  EnvSwitches s{};
  s.graph = std::getenv("ADMM_HIP_GRAPH") != nullptr;
  const char* form = std::getenv("ADMM_TRSV_FORM");
  s.trsv_form = !form ? -1 : form[0] == 'b' ? kTrsvBlocked : form[0] == 'o' ? kTrsvOne : -1;
  const char* split = std::getenv("ADMM_HIP_XSPLIT");
  s.xsplit = !split ? -1 : split[0] == '1' ? 1 : 0;
  s.no_unwrapped_fused = std::getenv("ADMM_HIP_NO_UNWRAPPED_FUSED") != nullptr;
  s.no_onepass = std::getenv("ADMM_HIP_NO_ONEPASS") != nullptr;
  return s;
}

int upload(DevMem& mem, double** dst, const double* src, size_t elems, int memkind, hipStream_t stream) {
  ADMM_TRY(mem.alloc(dst, elems));
  ADMM_HIP_TRY(hipMemcpyAsync(*dst, src, elems * sizeof(double),
                              memkind == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  return ADMM_OK;
}

// copy a column-major m x n matrix into a zero-padded device buffer with leading dimension ld
int upload_matrix(DevMem& mem, double** dst, int64_t* ld_out, const double* src, int64_t rows, int64_t cols,
                  int64_t ld_src, int memkind, hipStream_t stream) {
  // 128-byte aligned columns always; 4 KiB aligned columns for tall matrices: measured +5 % on the
  // gemv_n stream (dev/gemv_real.hip, ld 100000 vs 98304) for 0.35 % more memory
  const int64_t ld = rows >= 8192 ? round_up(rows, 512) : round_up(rows, 16);
  ADMM_TRY(mem.alloc(dst, static_cast<size_t>(ld) * cols));
  if (ld != rows) ADMM_HIP_TRY(hipMemsetAsync(*dst, 0, sizeof(double) * ld * cols, stream));
  ADMM_HIP_TRY(hipMemcpy2DAsync(*dst, ld * sizeof(double), src, ld_src * sizeof(double), rows * sizeof(double), cols,
                                memkind == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                stream));
  *ld_out = ld;
  return ADMM_OK;
}

void free_hist(admm_engine* e) {
  for (void* p : e->hist_ptrs) (void)hipFree(p);
  e->hist_ptrs.clear();
  e->xhist = e->zhist = e->uhist = e->vhist = e->uhathist = e->zthist = e->vthist = nullptr;
  e->pnorm = e->dnorm = e->perr = e->derr = e->objv = e->hnorm = e->avals = e->dvals = e->restarted = nullptr;
  e->hist_cap = 0;
}

int hist_alloc(admm_engine* e, double** out, size_t elems) {
  void* p = nullptr;
  if (elems == 0) elems = 1;
  hipError_t err = hipMalloc(&p, elems * sizeof(double));
  if (err != hipSuccess)
    return fail(ADMM_E_DEVICE, std::string("hipMalloc(history ") + std::to_string(elems * sizeof(double)) +
                                   " B): " + hipGetErrorString(err));
  e->hist_ptrs.push_back(p);
  *out = static_cast<double*>(p);
  return ADMM_OK;
}

int allreduce_scalar(admm_engine* e, double* value, double* slot) {
  if (!e->comm || comm_nranks(e->comm) <= 1) return ADMM_OK;
  if (!slot) ADMM_TRY(e->mem.alloc(&slot, 2));
  ADMM_HIP_TRY(hipMemcpyAsync(slot, value, sizeof(double), hipMemcpyHostToDevice, e->stream));
  ADMM_TRY(comm_allreduce_device(e->comm, slot, 1, e->stream));
  ADMM_HIP_TRY(hipMemcpyAsync(value, slot, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  return ADMM_OK;
}

int device_sumsq_host(admm_engine* e, const double* dev, int64_t count, double* out) {
  std::vector<double> h(static_cast<size_t>(count));
  ADMM_HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(double) * count, hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  double ss = 0.0;
  for (double v : h) ss += v * v;
  *out = ss;
  return ADMM_OK;
}

int gram_lower(admm_engine* e, const double* D, int64_t ldD, int64_t rows, int64_t cols, bool of_rows, double scale,
               double* W, int64_t ldW) {
  const int64_t k = of_rows ? rows : cols;
  ADMM_HIP_TRY(hipMemsetAsync(W, 0, sizeof(double) * ldW * k, e->stream));
  launch_gemm(of_rows ? 0 : 1, of_rows ? 1 : 0, k, k, of_rows ? cols : rows, scale, D, ldD, D, ldD, 0.0, W, ldW, true,
              e->stream);
  return ADMM_OK;
}

void collect_timers(admm_engine* e) {
  for (int w = 0; w < ADMM_K_COUNT; ++w) {
    KTimer& t = e->timers[w];
    t.total_ms = 0.0;
    t.launches = 0;
    for (size_t k = 0; k + 1 < t.used; k += 2) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, t.ev[k], t.ev[k + 1]) == hipSuccess) {
        t.total_ms += ms;
        t.launches += 1;
      }
    }
    t.used = 0;
  }
}

// ---- factor setup ------------------------------------------------------------------
// partial-sum buffers of the lower-triangle kernel, shared by every factor of the engine (same n)
static int ensure_sy_buffers(admm_engine* e, const SymvPlan& plan) {
  const size_t need = plan.npart_elems();
  if (e->syN && e->sy_elems >= need) return ADMM_OK;
  e->mem.free_one(e->syN);
  e->mem.free_one(e->syT);
  e->syN = e->syT = nullptr;
  ADMM_TRY(e->mem.alloc(&e->syN, need));
  ADMM_TRY(e->mem.alloc(&e->syT, plan.tpart_elems()));
  e->sy_elems = need;
  // zero once: with the tiles split over ranks, the slots of foreign tiles are never written
  ADMM_HIP_TRY(hipMemsetAsync(e->syN, 0, sizeof(double) * need, e->stream));
  ADMM_HIP_TRY(hipMemsetAsync(e->syT, 0, sizeof(double) * plan.tpart_elems(), e->stream));
  return ADMM_OK;
}

// The padded column-major inverse of a factor -> tile-packed storage (symv.hip): half the memory, and the layout the
// lower-triangle kernel streams fastest.  Small factors (symv_small_kernel reads whole columns) stay as they are.
static int pack_inverse(admm_engine* e, SliceFactor& f) {
  if (f.n < kSymvHalfMin || f.planSy.packed) return ADMM_OK;
  double* P = nullptr;
  ADMM_TRY(e->mem.alloc(&P, symv_packed_elems(f.planSy)));
  launch_symv_pack(f.planSy, f.Minv, f.ldM, P, e->stream);
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->mem.free_one(f.Minv);
  f.Minv = P;
  f.ldM = 0;
  f.planSy.packed = true;
  return ADMM_OK;
}

// f.Minv (tile-padded, zeros outside n x n) = X' X with X = inv(L): the explicit inverse of L L'; pack = false keeps
// the padded column-major square (full symmetric storage) for callers that multiply with it as a dense matrix
static int build_explicit_inverse(admm_engine* e, SliceFactor& f, bool pack = true) {
  const int64_t n = f.n, ld = f.ld;
  double* X = nullptr;
  ADMM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&X), sizeof(double) * ld * n));
  int rc = trtri_lower_from_diag(f.F, n, ld, f.dinv, X, ld, e->stream);
  f.planSy = symv_plan(n);
  f.ldM = f.planSy.npad;  // (4 / 8 / 16 KiB-aligned columns were measured: no effect on the lower-triangle kernel)
  if (rc == ADMM_OK) rc = e->mem.alloc(&f.Minv, static_cast<size_t>(f.ldM) * f.planSy.npad);
  if (rc == ADMM_OK) {
    (void)hipMemsetAsync(f.Minv, 0, sizeof(double) * f.ldM * f.planSy.npad, e->stream);
    launch_gemm(1, 0, n, n, n, 1.0, X, ld, X, ld, 0.0, f.Minv, f.ldM, true, e->stream);
    launch_symmetrize_lower(f.Minv, n, f.ldM, e->stream);
  }
  (void)hipStreamSynchronize(e->stream);
  (void)hipFree(X);
  ADMM_TRY(rc);
  if (pack) ADMM_TRY(pack_inverse(e, f));
  if (n >= kSymvHalfMin) ADMM_TRY(ensure_sy_buffers(e, f.planSy));
  return ADMM_OK;
}

static void apply_inverse(admm_engine* e, const SliceFactor& f, const double* y, double* out, const Ctrl* ctrl) {
  if (f.n >= kSymvHalfMin) launch_symv_lower(f.planSy, f.Minv, f.ldM, y, e->syN, e->syT, out, ctrl, e->stream);
  else launch_symv_small(f.Minv, f.n, f.ldM, y, out, ctrl, e->stream);
}

// the probe itself: two ways of applying inv(L L') on (L L') x = L (L' x0) with a known x0 (max-norm errors relative to
// ||x0||_inf), then on a second, unstructured right-hand side where they are compared with each other
template <class ApplyA, class ApplyB>
static int probe_two_forms(admm_engine* e, const SliceFactor& f, ApplyA&& apply_a, ApplyB&& apply_b, double* err_a,
                           double* err_b, double* diff_ab) {
  const int64_t n = f.n, n2 = round_up(n, 2);
  std::vector<double> x0(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) x0[i] = 1.0 + 0.5 * std::sin(1.0 + 0.7 * static_cast<double>(i));
  double* buf = nullptr;
  ADMM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), sizeof(double) * 5 * n2));
  double *dx0 = buf, *dt = buf + n2, *dy = buf + 2 * n2, *dxi = buf + 3 * n2, *dxt = buf + 4 * n2;
  int rc = ADMM_OK;
  std::vector<double> xi(static_cast<size_t>(n)), xt(static_cast<size_t>(n));
  auto run = [&]() -> int {
    ADMM_HIP_TRY(hipMemcpyAsync(dx0, x0.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
    launch_llt_apply(f.F, n, f.ld, dx0, dt, dy, e->stream);  // y = L (L' x0)
    apply_a(dy, dxi);
    apply_b(dy, dxt);
    ADMM_HIP_TRY(hipMemcpyAsync(xi.data(), dxi, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipMemcpyAsync(xt.data(), dxt, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    return ADMM_OK;
  };
  rc = run();
  double ei = 0.0, et = 0.0;
  if (rc == ADMM_OK) {
    for (int64_t i = 0; i < n; ++i) {
      const double a = std::fabs(xi[i] - x0[i]), b = std::fabs(xt[i] - x0[i]);
      ei = (a > ei || a != a) ? a : ei;
      et = (b > et || b != b) ? b : et;
    }
    // second right-hand side: signs and sizes with no structure (its solution is dominated by the small singular
    // directions); no exact answer, so the two forms are compared with each other
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    for (int64_t i = 0; i < n; ++i) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      const double u01 = static_cast<double>(lcg >> 11) * (1.0 / 9007199254740992.0);
      x0[i] = (u01 < 0.5 ? -1.0 : 1.0) * (0.5 + u01);
    }
    auto run2 = [&]() -> int {
      ADMM_HIP_TRY(hipMemcpyAsync(dy, x0.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
      apply_a(dy, dxi);
      apply_b(dy, dxt);
      ADMM_HIP_TRY(hipMemcpyAsync(xi.data(), dxi, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
      ADMM_HIP_TRY(hipMemcpyAsync(xt.data(), dxt, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
      ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
      return ADMM_OK;
    };
    rc = run2();
  }
  (void)hipFree(buf);
  ADMM_TRY(rc);
  double dmax = 0.0, xmax = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double d = std::fabs(xi[i] - xt[i]), a = std::fabs(xt[i]);
    dmax = (d > dmax || d != d) ? d : dmax;
    xmax = a > xmax ? a : xmax;
  }
  *err_a = ei / 1.5;  // relative to ||x0||_inf
  *err_b = et / 1.5;
  *diff_ab = xmax > 0.0 ? dmax / xmax : dmax;
  return ADMM_OK;
}

// Which form applies inv(L L')?  The explicit inverse is one bandwidth-bound pass but its forward error grows like
// cond(LL')^1.5 * eps; the blocked triangular solves stay at the cond(LL') * eps of a backward-stable solve.  The
// engine does not guess from a condition estimate: it builds both, solves  (L L') x = L (L' x0)  for a known x0 with
// each, compares them on a second, unstructured right-hand side, and keeps the explicit inverse only while it is
// as accurate as the triangular solves (within 2x / 4x) or below 1e-9 (three orders under the 1e-6 parity bar);
// otherwise the triangular solves run, also when `inverse` was requested explicitly.
static int probe_and_choose(admm_engine* e, SliceFactor& f) {
  ADMM_TRY(probe_two_forms(
      e, f, [&](const double* y, double* x) { apply_inverse(e, f, y, x, nullptr); },
      [&](const double* y, double* x) { launch_trsv_pair(f.trsv, y, x, nullptr, e->stream); }, &f.err_inv, &f.err_trsv,
      &f.probe_diff));
  f.probed = true;
  // keep the one-pass form while it is as good as the backward-stable solves (or simply good enough)
  const bool ok1 = f.err_inv <= std::max(1e-9, 2.0 * f.err_trsv);
  const bool ok2 = f.probe_diff <= std::max(1e-9, 4.0 * f.err_trsv);
  f.mode = (ok1 && ok2) ? ADMM_XSOLVE_INVERSE : ADMM_XSOLVE_TRSV;
  return ADMM_OK;
}

// The triangular solves themselves have two forms (trsv.hip): blocked substitution over K = ceil(n / 2048) coarse blocks
// with pre-inverted DIAGONAL blocks (2K + 1 dependent launches per pair), and the one-block form -- the whole factor
// pre-inverted, X = inv(L), two passes and two launches per pair, same 8 n(n+1) bytes.  X costs forward error
// eps * cond(L) per pass where a diagonal block costs eps * cond(L_kk).  Same rule as above: the blocked form (already
// built: f.trsv) is the yardstick, and the one-block form replaces it only while it is as accurate on both probe
// systems (within 4x / 8x) or below 1e-11 -- five orders under the parity bar.  ADMM_TRSV_FORM=one|blocked forces it.
static int choose_trsv_form(admm_engine* e, SliceFactor& f) {
  f.err_trsv_one = NAN;
  const bool forced_one = env_switches().trsv_form == kTrsvOne;
  if (trsv_resolve_form(f.n, kTrsvOne) != kTrsvOne) return ADMM_OK;
  if (f.n < kSymvHalfMin && !forced_one) return ADMM_OK;  // a few tiles: the steps are cheap
  double* work1 = nullptr;
  ADMM_TRY(e->mem.alloc(&work1, trsv_plan_elems(f.n, kTrsvOne)));
  TrsvPlan one{};
  int rc = trsv_build(f.F, f.n, f.ld, f.dinv, work1, &one, e->stream, kTrsvOne);
  double e1 = NAN, eb = NAN, diff = NAN;
  if (rc == ADMM_OK)
    rc = probe_two_forms(
        e, f, [&](const double* y, double* x) { launch_trsv_pair(one, y, x, nullptr, e->stream); },
        [&](const double* y, double* x) { launch_trsv_pair(f.trsv, y, x, nullptr, e->stream); }, &e1, &eb, &diff);
  if (rc != ADMM_OK) {
    e->mem.free_one(work1);
    return rc;
  }
  f.err_trsv_one = e1;
  if (!f.probed) f.err_trsv = eb;
  const bool ok = forced_one || (e1 <= std::max(1e-11, 4.0 * eb) && diff <= std::max(1e-11, 8.0 * eb));
  if (ok) {
    e->mem.free_one(f.work);
    f.work = work1;
    f.trsv = one;
  } else {
    e->mem.free_one(work1);
  }
  return ADMM_OK;
}

// W (n x n, ld) holds an SPD matrix in its lower triangle (or receives the caller's factor Lgiven) -> f: the
// Cholesky factor in place, its inverted 64 x 64 diagonal blocks, and ONE way of applying inv(L L'):
// want = TRSV: blocked triangular solves; INVERSE / AUTO: the explicit inverse if the probe allows it.
int build_slice_factor(admm_engine* e, SliceFactor& f, double* W, int64_t n, int64_t ld, int want, const double* Lgiven,
                       int memkind) {
  f.F = W;
  f.n = n;
  f.ld = ld;
  const int64_t nblk = ceil_div(n, 64);
  ADMM_TRY(e->mem.alloc(&f.dinv, static_cast<size_t>(nblk) * 64 * 64));
  if (Lgiven) {
    ADMM_HIP_TRY(hipMemsetAsync(W, 0, sizeof(double) * ld * n, e->stream));
    ADMM_HIP_TRY(hipMemcpy2DAsync(W, ld * sizeof(double), Lgiven, n * sizeof(double), n * sizeof(double), n,
                                  memkind == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                  e->stream));
    launch_trtri_diag(W, n, ld, f.dinv, e->stream);
  } else {
    double* infod = nullptr;
    ADMM_TRY(e->mem.alloc(&infod, 1));
    int32_t* info_dev = reinterpret_cast<int32_t*>(infod);
    ADMM_TRY(cholesky_lower(W, n, ld, info_dev, f.dinv, e->stream));
    int32_t info = 0;
    ADMM_HIP_TRY(hipMemcpyAsync(&info, info_dev, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    e->mem.free_one(infod);
    if (info != 0) {
      f.chol_info = info;
      return fail(ADMM_E_NUMERIC, "Cholesky failed: matrix must be positive definite (pivot " + std::to_string(info) + ")");
    }
  }
  {  // cond(L L') >= (max L_ii / min L_ii)^2: a lower bound that costs one strided copy of the diagonal
    std::vector<double> dg(static_cast<size_t>(n));
    ADMM_HIP_TRY(hipMemcpy2DAsync(dg.data(), sizeof(double), W, (ld + 1) * sizeof(double), sizeof(double), n,
                                  hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    double lo = INFINITY, hi = 0.0;
    for (double v : dg) {
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    f.diag_min = lo;
    f.diag_max = hi;
    f.cond_diag = (lo > 0.0) ? (hi / lo) * (hi / lo) : INFINITY;
  }
  // AUTO: the explicit inverse at every size while the probe below allows it -- one launch per x-update where the
  // triangular solves take three or more, which is all a small problem pays for (256 x 64, the testers' default:
  // 20 -> 13 us per iteration)
  if (want == ADMM_XSOLVE_AUTO) want = ADMM_XSOLVE_INVERSE;
  // the blocked triangular solves are built in every case: they are the fallback and the probe's yardstick
  ADMM_TRY(e->mem.alloc(&f.work, trsv_plan_elems(n)));
  ADMM_TRY(trsv_build(W, n, ld, f.dinv, f.work, &f.trsv, e->stream));
  f.mode = ADMM_XSOLVE_TRSV;
  if (want == ADMM_XSOLVE_INVERSE) {
    ADMM_TRY(build_explicit_inverse(e, f));
    ADMM_TRY(probe_and_choose(e, f));
    if (f.mode == ADMM_XSOLVE_INVERSE) {  // the triangular-solve plan was only the yardstick
      e->mem.free_one(f.work);
      f.work = nullptr;
      f.trsv = TrsvPlan{};
    } else {
      e->mem.free_one(f.Minv);
      f.Minv = nullptr;
    }
  }
  if (f.mode == ADMM_XSOLVE_TRSV) ADMM_TRY(choose_trsv_form(e, f));
  return ADMM_OK;
}

// The rule of choose_symv_storage: the one choose_trsv_form applies to a cheaper form against its yardstick.
bool symv_compact_accept(double err_compact, double err_fp64, double diff) {
  return err_compact <= std::max(1e-11, 4.0 * err_fp64) && diff <= std::max(1e-11, 8.0 * err_fp64);
}

// How the explicit inverse of the engine's own factor is STORED.  The packed x-solve of a matrix too large for the
// caches runs at the ingest rate of the part, so its time is its byte count: the compact storage (tri_tile.h: 48-bit
// tile-scaled fixed point off the diagonal, 3/4 of the bytes) is built where the fp64 packed triangle streams, probed
// as form A against that triangle as form B on the two systems of probe_two_forms, and adopted -- the fp64 triangle
// freed -- while it is as accurate (within 4x / 8x) or below 1e-11.  Where even the 48-bit store is larger than
// kSymvCacheBytes -- part of it comes from HBM in every iteration -- the 40-bit form (5/8 of the bytes) is tried first,
// under the same rule, and where even the 40-bit store is larger than that, the 36-bit (9/16) and 38-bit (19/32) forms
// before it: the ladder 36, 38, 40, 48, fp64, the first width accepted kept and the others freed; a rejected rung
// leaves its probe numbers in f.cq_rejected.  A cache-resident matrix is latency-bound and gains nothing; the
// consensus slices (batched launch), the pseudo-inverse (no factor to probe with) and the row-sharded split x-solve keep
// fp64.
static int try_symv_storage(admm_engine* e, SliceFactor& f, int bits, bool* kept);
static int choose_symv_storage(admm_engine* e, SliceFactor& f) {
  if (f.mode != ADMM_XSOLVE_INVERSE || !f.Minv || !f.F || f.pinv || !f.planSy.packed || f.planSy.cbits ||
      f.n < kSymvHalfMin || e->sy_split || e->keep_fp64)
    return ADMM_OK;
  if (!stream_hint(symv_tile_prefix_bytes(f.planSy, symv_tiles(f.planSy)))) return ADMM_OK;
  auto streams = [&](int bits) {  // the store of that width is larger than the cacheable share
    SymvPlan c = f.planSy;
    c.cbits = bits;
    return symv_tile_prefix_bytes(c, symv_tiles(c)) > kSymvCacheBytes;
  };
  bool kept = false;
  f.cq_nrejected = 0;
  if (streams(48) && streams(40)) {
    ADMM_TRY(try_symv_storage(e, f, 36, &kept));
    if (!kept) ADMM_TRY(try_symv_storage(e, f, 38, &kept));
  }
  if (!kept && streams(48)) ADMM_TRY(try_symv_storage(e, f, 40, &kept));
  if (!kept) ADMM_TRY(try_symv_storage(e, f, 48, &kept));
  return ADMM_OK;
}

// build the compact form of that width, probe it, adopt it or free it; the probe numbers of the last form tried stay
static int try_symv_storage(admm_engine* e, SliceFactor& f, int bits, bool* kept) {
  if (!symv_cbits_ok(bits))
    return fail(ADMM_E_INVALID, "compact x-solve storage: no tile width of " + std::to_string(bits) + " bits");
  SymvPlan cp = f.planSy;
  cp.cbits = bits;
  double* C = nullptr;
  ADMM_TRY(e->mem.alloc(&C, symv_compact_elems(cp)));
  launch_symv_compact_pack(cp, f.Minv, 0, true, C, nullptr, e->stream);
  cp.scales = symv_compact_scales(cp, C);
  cp.ncached = symv_cached_tiles(cp, kSymvCacheBytes);
  double ea = NAN, eb = NAN, diff = NAN;
  const int rc = probe_two_forms(
      e, f, [&](const double* y, double* x) { launch_symv_lower(cp, C, 0, y, e->syN, e->syT, x, nullptr, e->stream); },
      [&](const double* y, double* x) { apply_inverse(e, f, y, x, nullptr); }, &ea, &eb, &diff);
  if (rc != ADMM_OK) {
    e->mem.free_one(C);
    return rc;
  }
  f.err_cq = ea;
  f.err_cq_ref = eb;
  f.cq_diff = diff;
  *kept = symv_compact_accept(ea, eb, diff);
  if (*kept) {
    e->mem.free_one(f.Minv);
    f.Minv = C;
    f.planSy = cp;
  } else {
    e->mem.free_one(C);
    if (f.cq_nrejected < SliceFactor::kCqRungs) f.cq_rejected[f.cq_nrejected++] = {bits, ea, eb, diff};
  }
  return ADMM_OK;
}

void release_slice_factor(admm_engine* e, SliceFactor& f) {
  e->mem.free_one(f.Minv);
  e->mem.free_one(f.work);
  e->mem.free_one(f.dinv);
  f = SliceFactor{};
}

void apply_slice_factor(admm_engine* e, const SliceFactor& f, const double* y, double* out) {
  if (f.mode == ADMM_XSOLVE_INVERSE) apply_inverse(e, f, y, out, e->ctrl);
  else launch_trsv_pair(f.trsv, y, out, e->ctrl, e->stream);
}

// engine-level multi-GPU refinement of the explicit-inverse x-solve: split the tiles over the ranks?
static int decide_sy_split(admm_engine* e) {
  const SliceFactor& f = e->xfac;
  e->sy_split = false;
  const int nr = e->comm ? comm_nranks(e->comm) : 1;
  if (nr <= 1 || f.mode != ADMM_XSOLVE_INVERSE || f.n < kSymvHalfMin) return ADMM_OK;
  // Splitting the tiles over the ranks removes t*(1 - 1/N) of streaming time per x-solve and adds one all-reduce
  // of n doubles.  Decide with the latency this communicator actually has (measured here, the mean over the
  // ranks so that every rank takes the same decision): t = 4*npad^2 bytes at ~5.5 TB/s.
  double* probe = e->syN;  // any device buffer of >= n + 1 doubles
  for (int k = 0; k < 3; ++k) ADMM_TRY(comm_allreduce_device(e->comm, probe, static_cast<size_t>(f.n), e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  const auto c0 = std::chrono::steady_clock::now();
  const int reps = 10;
  for (int k = 0; k < reps; ++k) ADMM_TRY(comm_allreduce_device(e->comm, probe, static_cast<size_t>(f.n), e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  double lat_us = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count() * 1e6 / reps;
  ADMM_TRY(allreduce_scalar(e, &lat_us, probe));
  lat_us /= nr;
  // (6.4e6 bytes/us: the packed kernel with the split cache policy; the unsplit path also keeps the deferred finalize
  // and needs no reduce launch for its partial rows: ~8 us the split has to win back on top of the collective)
  const double t_us = 4.0 * static_cast<double>(f.planSy.npad) * static_cast<double>(f.planSy.npad) / 6.4e6;
  e->sy_split = t_us * (1.0 - 1.0 / nr) > 1.15 * lat_us + 8.0;
  if (const int forced = env_switches().xsplit; forced >= 0) e->sy_split = forced == 1;  // tests force either form
  // the probe (and the latency measurement) left partial sums behind; with the tiles split over ranks the slots
  // of foreign tiles are never written again and must read as zero
  ADMM_HIP_TRY(hipMemsetAsync(e->syN, 0, sizeof(double) * f.planSy.npart_elems(), e->stream));
  ADMM_HIP_TRY(hipMemsetAsync(e->syT, 0, sizeof(double) * f.planSy.tpart_elems(), e->stream));
  return ADMM_OK;
}

// pinv(D) as an explicit n x m matrix for the two-launch unwrapped iteration (unwrapped.hip): the caller's args.Dplus as
// it is, or inv(D'D)*D' from the factor create() has just built -- its explicit inverse when that is the form in use
// (or the pseudo-inverse of a rank-deficient D'D), a temporary one for the small factors that default to triangular
// solves.  Not built when the accuracy probe rejected the explicit inverse, when the caller asked for another x-solve
// form, on sharded engines, or for sizes the kernel does not cover: the generic A = D iteration runs then.
int build_unwrapped_pinv(admm_engine* e, const double* Dp_given) {
  const int64_t m = e->m, n = e->n;
  if (env_switches().no_unwrapped_fused) return ADMM_OK;
  if (!uw_supported(m, n) || (e->comm && comm_nranks(e->comm) > 1)) return ADMM_OK;
  if (static_cast<double>(m) * static_cast<double>(n) * 8.0 > 1.5e9) return ADMM_OK;
  const int64_t ldp = round_up(n, 2);
  if (Dp_given) {
    ADMM_TRY(e->mem.alloc(&e->Dp, static_cast<size_t>(ldp) * m));
    ADMM_HIP_TRY(hipMemcpy2DAsync(e->Dp, ldp * sizeof(double), Dp_given, n * sizeof(double), n * sizeof(double), m,
                                  hipMemcpyDeviceToDevice, e->stream));
  } else {
    SliceFactor& f = e->xfac;
    if (e->xsolve_requested == ADMM_XSOLVE_TRSV || e->xsolve_requested == ADMM_XSOLVE_CG) return ADMM_OK;
    SliceFactor tmp{};
    const double* Minv = nullptr;
    int64_t ldM = 0;
    if (f.mode == ADMM_XSOLVE_INVERSE && f.Minv && !f.planSy.packed) {
      Minv = f.Minv;
      ldM = f.ldM;
    } else if (f.mode == ADMM_XSOLVE_TRSV && !f.probed && f.F) {
      tmp.F = f.F;
      tmp.n = f.n;
      tmp.ld = f.ld;
      tmp.dinv = f.dinv;
      ADMM_TRY(build_explicit_inverse(e, tmp, false));
      Minv = tmp.Minv;
      ldM = tmp.ldM;
    } else {
      return ADMM_OK;
    }
    ADMM_TRY(e->mem.alloc(&e->Dp, static_cast<size_t>(ldp) * m));
    ADMM_HIP_TRY(hipMemsetAsync(e->Dp, 0, sizeof(double) * ldp * m, e->stream));
    launch_gemm(0, 1, n, m, n, 1.0, Minv, ldM, e->D, e->ldD, 0.0, e->Dp, ldp, false, e->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    if (tmp.Minv) e->mem.free_one(tmp.Minv);
  }
  e->ldDp = ldp;
  e->uwR = uw_rows_per_block(m);
  e->uwnblk = static_cast<int32_t>(ceil_div(m, static_cast<int64_t>(e->uwR)));
  e->uwldg = round_up(n, 2);
  ADMM_TRY(e->mem.alloc(&e->uwG, static_cast<size_t>(2) * e->uwnblk * e->uwldg));
  ADMM_HIP_TRY(hipMemsetAsync(e->uwG, 0, sizeof(double) * 2 * e->uwnblk * e->uwldg, e->stream));
  e->uwnchunk = uw_chunks(n);
  e->uwldax = round_up(m, 2);
  ADMM_TRY(e->mem.alloc(&e->uwAx, static_cast<size_t>(e->uwnchunk) * e->uwldax));
  ADMM_TRY(e->mem.alloc(&e->uwX, static_cast<size_t>(2) * e->uwldg));
  return ADMM_OK;
}

// ---- one-time reductions some solvers do before the loop, on the device ---------------------------------------------
// W (n x n, ld, lower triangle valid, SPD) -> its explicit inverse, full symmetric storage (tile-padded, ld *ldM).
// W is destroyed; the result is owned by e->mem (release with DevMem::free_one).
static int spd_inverse(admm_engine* e, double* W, int64_t n, int64_t ld, double** Minv, int64_t* ldM) {
  SliceFactor f{};
  f.F = W;
  f.n = n;
  f.ld = ld;
  ADMM_TRY(e->mem.alloc(&f.dinv, static_cast<size_t>(ceil_div(n, 64)) * 64 * 64));
  double* infod = nullptr;
  ADMM_TRY(e->mem.alloc(&infod, 1));
  ADMM_TRY(cholesky_lower(W, n, ld, reinterpret_cast<int32_t*>(infod), f.dinv, e->stream));
  int32_t info = 0;
  ADMM_HIP_TRY(hipMemcpyAsync(&info, infod, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->mem.free_one(infod);
  if (info != 0)
    return fail(ADMM_E_NUMERIC, "Cholesky failed: matrix must be positive definite (pivot " + std::to_string(info) +
                                    "): the constraint matrix needs full row rank");
  ADMM_TRY(build_explicit_inverse(e, f, false));
  e->mem.free_one(f.dinv);
  *Minv = f.Minv;
  *ldM = f.ldM;
  return ADMM_OK;
}

// out[n] = alpha * T' * v for T (m x n, ldt)
static int scaled_tdot(admm_engine* e, const double* T, int64_t m, int64_t n, int64_t ldt, const double* v, double alpha,
                       double* out) {
  const GemvTPlan pt = gemv_t_plan(m, n, ldt);
  double *part = nullptr, *tmp = nullptr;
  ADMM_TRY(e->mem.alloc(&part, pt.part_elems(1)));
  ADMM_TRY(e->mem.alloc(&tmp, round_up(n, 2)));
  launch_gemv_t(pt, T, v, nullptr, nullptr, 1, part, nullptr, e->stream);
  launch_sum_partials_t(pt, part, 1, tmp, round_up(n, 2), nullptr, e->stream);
  launch_combine(tmp, 1, 0, alpha, nullptr, 0.0, nullptr, out, n, nullptr, e->stream);
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->mem.free_one(part);
  e->mem.free_one(tmp);
  return ADMM_OK;
}

// The affine maps built below (x = K*y + k0 of the eliminated KKT system; x = P*v + q of basis pursuit) go through
// explicit inverses of D*inv(M)*D' resp. D*D', whose condition number is cond(D)^2 -- where the reference solves the
// KKT system by pivoted backslash in every iteration (getProxOps.m:1363, 1410) or forms P by backslash
// (basispursuit.m:116-120).  What must survive is the constraint: every x the map produces satisfies D*x = s.  Probe it
// once, for an unstructured argument: relative violation max|D*x - s| / (max|s| + max|D*x|) above 1e-9 refuses the
// problem (ADMM_E_NUMERIC) instead of iterating on iterates that silently leave the feasible set.
static int probe_affine_map(admm_engine* e, const double* D, int64_t m, int64_t n, int64_t ldD, const double* s_dev,
                            const double* Kmat, int64_t ldK, const double* k0, const char* what) {
  std::vector<double> yh(static_cast<size_t>(n)), xh(static_cast<size_t>(n)), rh(static_cast<size_t>(m)),
      sh(static_cast<size_t>(m));
  for (int64_t i = 0; i < n; ++i) yh[i] = std::sin(0.7 * static_cast<double>(i) + 0.3) + 0.25;
  double *y = nullptr, *x = nullptr, *r = nullptr, *partK = nullptr, *partD = nullptr;
  ADMM_TRY(e->mem.alloc(&y, round_up(n, 2)));
  ADMM_TRY(e->mem.alloc(&x, round_up(n, 2)));
  ADMM_TRY(e->mem.alloc(&r, round_up(m, 2)));
  ADMM_HIP_TRY(hipMemcpyAsync(y, yh.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
  const GemvTPlan pk = gemv_t_plan(n, n, ldK);  // K (P) is symmetric: K*y as column dots
  ADMM_TRY(e->mem.alloc(&partK, pk.part_elems(1)));
  launch_gemv_t(pk, Kmat, y, nullptr, nullptr, 1, partK, nullptr, e->stream);
  launch_sum_partials_t(pk, partK, 1, x, round_up(n, 2), nullptr, e->stream);
  launch_combine(x, 1, 0, 1.0, nullptr, 0.0, k0, x, n, nullptr, e->stream);  // x = K*y + k0
  const GemvNPlan pd = gemv_n_plan(m, n, ldD);
  ADMM_TRY(e->mem.alloc(&partD, pd.part_elems()));
  launch_gemv_n(pd, D, x, partD, nullptr, e->stream);
  launch_sum_partials(partD, pd.nchunk, pd.ldy, m, r, nullptr, e->stream);
  ADMM_HIP_TRY(hipMemcpyAsync(rh.data(), r, sizeof(double) * m, hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipMemcpyAsync(sh.data(), s_dev, sizeof(double) * m, hipMemcpyDeviceToHost, e->stream));
  // the size of D*(an unstructured vector): with s = 0 (or tiny) D*x and s are both rounding noise, and their own
  // magnitudes would make a relative violation of order 1 out of nothing (found by the solver sweep: 1 x 2, s = 0)
  std::vector<double> dyh(static_cast<size_t>(m));
  launch_gemv_n(pd, D, y, partD, nullptr, e->stream);
  launch_sum_partials(partD, pd.nchunk, pd.ldy, m, r, nullptr, e->stream);
  ADMM_HIP_TRY(hipMemcpyAsync(dyh.data(), r, sizeof(double) * m, hipMemcpyDeviceToHost, e->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  for (double* p : {y, x, r, partK, partD}) e->mem.free_one(p);
  double viol = 0.0, scale = 0.0;
  bool finite = true;
  for (int64_t i = 0; i < m; ++i) {
    finite = finite && std::isfinite(rh[i]);
    viol = std::max(viol, std::fabs(rh[i] - sh[i]));
    scale = std::max(scale, std::max(std::max(std::fabs(rh[i]), std::fabs(sh[i])), std::fabs(dyh[i])));
  }
  const double rel = viol / (scale > 0.0 ? scale : 1.0);
  if (!finite || !(rel <= 1e-9))
    return fail(ADMM_E_NUMERIC, std::string(what) + ": the constraint matrix D is too ill-conditioned for the eliminated "
                                    "solve (cond(D)^2 enters it): D*x = s is violated by " + std::to_string(rel) +
                                    " (relative) for a probe vector; the reference's pivoted KKT solve would be needed");
  return ADMM_OK;
}

// basispursuit.m:116-120: P = I - D'(DD')^-1 D, q = D'(DD')^-1 s for a fat D (m x n, m < n) -- MFMA GEMMs, the
// Cholesky factorisation and the explicit m x m inverse on the device (the reference computes them in MATLAB)
int build_bp_projector(admm_engine* e, const double* D, int64_t m, int64_t n, int64_t ldD, const double* s_dev) {
  const int64_t ldw = round_up(m, 16);
  double *W = nullptr, *Ginv = nullptr, *X = nullptr;
  int64_t ldG = 0;
  ADMM_TRY(e->mem.alloc(&W, static_cast<size_t>(ldw) * m));
  ADMM_TRY(gram_lower(e, D, ldD, m, n, true, 1.0, W, ldw));  // D*D'
  ADMM_TRY(spd_inverse(e, W, m, ldw, &Ginv, &ldG));
  ADMM_TRY(e->mem.alloc(&X, static_cast<size_t>(ldw) * n));
  launch_gemm(0, 0, m, n, m, 1.0, Ginv, ldG, D, ldD, 0.0, X, ldw, false, e->stream);  // (DD')^-1 D
  e->ldP = round_up(n, 16);
  ADMM_TRY(e->mem.alloc(&e->Pmat, static_cast<size_t>(e->ldP) * n));
  ADMM_HIP_TRY(hipMemsetAsync(e->Pmat, 0, sizeof(double) * e->ldP * n, e->stream));
  launch_gemm(1, 0, n, n, m, -1.0, D, ldD, X, ldw, 0.0, e->Pmat, e->ldP, false, e->stream);  // -D'(DD')^-1 D
  launch_add_diag(e->Pmat, n, e->ldP, 1.0, e->stream);
  ADMM_TRY(e->mem.alloc(&e->q, round_up(n, 2)));
  ADMM_TRY(scaled_tdot(e, X, m, n, ldw, s_dev, 1.0, e->q));  // X' s
  e->mem.free_one(W);
  e->mem.free_one(Ginv);
  e->mem.free_one(X);
  return probe_affine_map(e, D, m, n, ldD, s_dev, e->Pmat, e->ldP, e->q, "basis pursuit");
}

// getProxOps.m:1363 / 1410 solve [M D'; D 0] [x; nu] = [y; s] every iteration, M = rho*I (linear program) or P + rho*I
// (standard-form QP).  Eliminating nu ONCE gives x = K*y + k0 with
//   K = inv(M) - inv(M) D' inv(S) D inv(M),  k0 = inv(M) D' inv(S) s,  S = D inv(M) D'
// -- built here with MFMA GEMMs and two explicit SPD inverses; the loop then runs one symmetric GEMV per x-update.
int build_kkt_map(admm_engine* e, const double* D, int64_t m, int64_t n, int64_t ldD, const double* s_dev,
                         const double* P /* null: LP */, int64_t ldPm, double rho) {
  const int64_t ldn = round_up(n, 16), ldm = round_up(m, 16);
  double *MD = nullptr, *S = nullptr, *Sinv = nullptr, *T2 = nullptr, *Mi = nullptr;
  int64_t ldS = 0, ldMi = 0;
  e->ldK = ldn;
  ADMM_TRY(e->mem.alloc(&e->Kmat, static_cast<size_t>(ldn) * n));
  ADMM_HIP_TRY(hipMemsetAsync(e->Kmat, 0, sizeof(double) * ldn * n, e->stream));
  ADMM_TRY(e->mem.alloc(&MD, static_cast<size_t>(ldn) * m));  // inv(M) D'  (n x m)
  if (P) {
    double* Mw = nullptr;
    ADMM_TRY(e->mem.alloc(&Mw, static_cast<size_t>(ldn) * n));
    ADMM_HIP_TRY(hipMemsetAsync(Mw, 0, sizeof(double) * ldn * n, e->stream));
    ADMM_HIP_TRY(hipMemcpy2DAsync(Mw, ldn * sizeof(double), P, ldPm * sizeof(double), n * sizeof(double), n,
                                  hipMemcpyDeviceToDevice, e->stream));
    launch_add_diag(Mw, n, ldn, rho, e->stream);
    ADMM_TRY(spd_inverse(e, Mw, n, ldn, &Mi, &ldMi));
    e->mem.free_one(Mw);
    launch_gemm(0, 1, n, m, n, 1.0, Mi, ldMi, D, ldD, 0.0, MD, ldn, false, e->stream);
    ADMM_HIP_TRY(hipMemcpy2DAsync(e->Kmat, ldn * sizeof(double), Mi, ldMi * sizeof(double), n * sizeof(double), n,
                                  hipMemcpyDeviceToDevice, e->stream));  // K starts as inv(M)
  } else {
    // inv(M) = I / rho:  MD = D'/rho  (a transposed, scaled copy through the GEMM with the identity left out:
    // MD(:, j) = D(j, :)'/rho is just the GEMM D' * (I/rho) -- done as a transpose-free product below)
    double* Ieye = nullptr;
    ADMM_TRY(e->mem.alloc(&Ieye, static_cast<size_t>(ldm) * m));
    ADMM_HIP_TRY(hipMemsetAsync(Ieye, 0, sizeof(double) * ldm * m, e->stream));
    launch_add_diag(Ieye, m, ldm, 1.0 / rho, e->stream);
    launch_gemm(1, 0, n, m, m, 1.0, D, ldD, Ieye, ldm, 0.0, MD, ldn, false, e->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    e->mem.free_one(Ieye);
    launch_add_diag(e->Kmat, n, ldn, 1.0 / rho, e->stream);  // K starts as I / rho
  }
  ADMM_TRY(e->mem.alloc(&S, static_cast<size_t>(ldm) * m));
  ADMM_HIP_TRY(hipMemsetAsync(S, 0, sizeof(double) * ldm * m, e->stream));
  launch_gemm(0, 0, m, m, n, 1.0, D, ldD, MD, ldn, 0.0, S, ldm, true, e->stream);  // S = D inv(M) D'
  ADMM_TRY(spd_inverse(e, S, m, ldm, &Sinv, &ldS));
  ADMM_TRY(e->mem.alloc(&T2, static_cast<size_t>(ldm) * n));  // inv(S) D inv(M)  (m x n)
  launch_gemm(0, 1, m, n, m, 1.0, Sinv, ldS, MD, ldn, 0.0, T2, ldm, false, e->stream);
  launch_gemm(0, 0, n, n, m, -1.0, MD, ldn, T2, ldm, 1.0, e->Kmat, ldn, false, e->stream);  // K -= MD * T2
  ADMM_TRY(e->mem.alloc(&e->k0, round_up(n, 2)));
  ADMM_TRY(scaled_tdot(e, T2, m, n, ldm, s_dev, 1.0, e->k0));  // k0 = T2' s = inv(M) D' inv(S) s
  for (double* p : {MD, S, Sinv, T2, Mi}) e->mem.free_one(p);
  return probe_affine_map(e, D, m, n, ldD, s_dev, e->Kmat, ldn, e->k0, P ? "quadratic program" : "linear program");
}

// the engine's own x-update factor
int factorize(admm_engine* e, double* W, int64_t nF, int64_t ld, const double* Lgiven, int memkind) {
  SliceFactor& f = e->xfac;
  // sharded engines must take the same decision on every rank: the factor is replicated bit for bit (all-reduced
  // Gram matrix, same kernels), so the probe is too
  ADMM_TRY(build_slice_factor(e, f, W, nF, ld, e->xsolve_requested, Lgiven, memkind));
  e->F = f.F;
  e->nF = nF;
  e->ldF = ld;
  e->xsolve = f.mode;
  ADMM_TRY(decide_sy_split(e));
  return choose_symv_storage(e, f);
}

// D'D is rank deficient (or numerically so): x = pinv(D)*(z-u) = (D'D)^+ D'(z-u)  (linearsvm.m:185,
// unwrappedadmm.m:76-78, getProxOps.m:1067).  W: the Gram matrix, lower triangle valid.  Builds
// (D'D)^+ = V diag(1/lambda_i : lambda_i > tol) V' with the Jacobi eigen-solver and applies it like the explicit
// inverse.  tol = n * eps * lambda_max: MATLAB's pinv rule max(size)*eps(norm) applied to D'D (the rank decisions
// agree with pinv(D)'s whenever the small singular values of D are zero to rounding, e.g. zero or duplicated columns).
int factorize_pinv(admm_engine* e, double* W, int64_t n, int64_t ld) {
  SliceFactor& f = e->xfac;
  f = SliceFactor{};
  f.n = n;
  f.ld = ld;
  launch_symmetrize_lower(W, n, ld, e->stream);
  double *V = nullptr, *lam = nullptr, *rotd = nullptr;
  const int64_t ldv = round_up(n, 16);
  ADMM_TRY(e->mem.alloc(&V, static_cast<size_t>(ldv) * n));
  ADMM_TRY(e->mem.alloc(&lam, n));
  ADMM_TRY(e->mem.alloc(&rotd, 1));
  std::vector<double> lh;
  int sweeps = 0;
  ADMM_TRY(jacobi_eig_psd(W, n, ld, V, ldv, lam, reinterpret_cast<int32_t*>(rotd), &lh, &sweeps, e->stream));
  double lmax = 0.0;
  for (double v : lh) lmax = v > lmax ? v : lmax;
  const double tol = static_cast<double>(n) * 2.220446049250313e-16 * lmax;
  int64_t rank = 0;
  double lmin = INFINITY;
  for (double& v : lh) {
    if (v > tol) {
      ++rank;
      lmin = v < lmin ? v : lmin;
      v = 1.0 / std::sqrt(v);
    } else {
      v = 0.0;
    }
  }
  ADMM_HIP_TRY(hipMemcpyAsync(lam, lh.data(), sizeof(double) * n, hipMemcpyHostToDevice, e->stream));
  launch_scale_cols(V, ldv, n, lam, e->stream);  // V <- V diag(lambda^-1/2)
  f.planSy = symv_plan(n);
  f.ldM = f.planSy.npad;  // (4 / 8 / 16 KiB-aligned columns were measured: no effect on the lower-triangle kernel)
  ADMM_TRY(e->mem.alloc(&f.Minv, static_cast<size_t>(f.ldM) * f.planSy.npad));
  ADMM_HIP_TRY(hipMemsetAsync(f.Minv, 0, sizeof(double) * f.ldM * f.planSy.npad, e->stream));
  launch_gemm(0, 1, n, n, n, 1.0, V, ldv, V, ldv, 0.0, f.Minv, f.ldM, true, e->stream);
  launch_symmetrize_lower(f.Minv, n, f.ldM, e->stream);
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->mem.free_one(V);
  e->mem.free_one(lam);
  e->mem.free_one(rotd);
  ADMM_TRY(pack_inverse(e, f));
  if (n >= kSymvHalfMin) ADMM_TRY(ensure_sy_buffers(e, f.planSy));
  f.mode = ADMM_XSOLVE_INVERSE;
  f.pinv = true;
  f.rank = rank;
  f.jacobi_sweeps = sweeps;
  f.cond_diag = rank > 0 ? lmax / lmin : INFINITY;  // over the retained spectrum
  e->F = nullptr;  // no Cholesky factor exists
  e->nF = n;
  e->ldF = ld;
  e->xsolve = ADMM_XSOLVE_INVERSE;
  return decide_sy_split(e);
}

// x = inv(LL')*y from the lower triangle of the explicit inverse; on a sharded engine every rank may stream 1/N of
// the tiles and ONE all-reduce of n doubles assembles x
int symv_apply(admm_engine* e, const double* y, double* out) {
  const SliceFactor& f = e->xfac;
  const int nr = e->comm ? comm_nranks(e->comm) : 1;
  if (nr > 1 && e->sy_split) {
    if (e->dfin && f.planSy.packed)  // the previous iteration's deferred finalize rides along (engine_run_general.hip)
      launch_symv_lower_fin(f.planSy, f.Minv, y, e->syN, e->syT, *e->dfin, e->dfin_pending, e->ctrl, e->stream,
                            comm_rank(e->comm), nr, out);
    else
      launch_symv_lower(f.planSy, f.Minv, f.ldM, y, e->syN, e->syT, out, e->ctrl, e->stream, comm_rank(e->comm), nr);
    return comm_allreduce_device(e->comm, out, static_cast<size_t>(f.n), e->stream);
  }
  apply_inverse(e, f, y, out, e->ctrl);
  return ADMM_OK;
}

// out = inv(L L') y with the engine's own factor
int solve_factor(admm_engine* e, const double* y, double* out) {
  if (e->xfac.mode == ADMM_XSOLVE_INVERSE) return symv_apply(e, y, out);
  launch_trsv_pair(e->xfac.trsv, y, out, e->ctrl, e->stream);
  return ADMM_OK;
}

}  // namespace admm

extern "C" {

int admm_abi_version(void) { return ADMM_ABI_VERSION; }
const char* admm_last_error(void) { return g_last_error.c_str(); }

int admm_device_count(int* count) {
  if (!count) return fail(ADMM_E_INVALID, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return fail(ADMM_E_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return ADMM_OK;
}

int admm_device_info(int device, char* name, size_t cap, int64_t* hbm_bytes, int32_t* cus) {
  hipDeviceProp_t prop;
  ADMM_HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (name && cap > 0) {
    std::strncpy(name, prop.gcnArchName, cap - 1);
    name[cap - 1] = 0;
  }
  if (hbm_bytes) *hbm_bytes = static_cast<int64_t>(prop.totalGlobalMem);
  if (cus) *cus = prop.multiProcessorCount;
  return ADMM_OK;
}

void admm_options_default(admm_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_options);
  o->maxiters = 1000;   // admm.m:58
  o->rho = 1.0;         // admm.m:57
  o->relax = 1.0;       // admm.m:60
  o->abstol = 1e-5;     // admm.m:71
  o->reltol = 1e-3;     // admm.m:72
  o->Hnormtol = 1e-6;   // admm.m:73
  o->convtol = 1e-10;   // admm.m:68
  o->restart = 0.999;   // admm.m:282
  o->dvaltol = 1e-8;    // admm.m:290
  o->record_history = 1;
}

void admm_problem_desc_default(admm_problem_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_problem_desc);
  d->rho = 1.0;
  d->cg_tol = 1e-12;
  d->cg_maxit = 200;
  d->nslices = 1;
}

int admm_engine_fetch(admm_engine* e, int field, double* dst, size_t cap, size_t* written) {
  if (!e || !dst) return fail(ADMM_E_INVALID, "engine/dst is NULL");
  if (!e->has_run && field != ADMM_F_FACTOR && field != ADMM_F_COVSEL_S)
    return fail(ADMM_E_INVALID, "no run to fetch results from");
  ADMM_HIP_TRY(hipSetDevice(e->device));
  const size_t steps = static_cast<size_t>(e->last.steps);
  const double* src = nullptr;
  size_t count = 0;
  bool need_vec_hist = false, need_fast = false;
  switch (field) {
    case ADMM_F_XOPT: src = e->x; count = e->nA; break;
    case ADMM_F_COVSEL_S:
      if (e->problem != ADMM_PROB_COVSEL) return fail(ADMM_E_INVALID, "ADMM_F_COVSEL_S: not a covariance-selection engine");
      src = e->cov_S;
      count = static_cast<size_t>(e->nA);
      break;
    case ADMM_F_ZOPT: src = e->bgen ? e->zt : e->z; count = e->bgen ? e->nBz : e->len; break;
    case ADMM_F_UOPT: src = e->u; count = e->len; break;
    case ADMM_F_XVALS: src = e->xhist; count = e->nA * steps; need_vec_hist = true; break;
    case ADMM_F_ZVALS:
      src = e->bgen ? e->zthist : e->zhist;
      count = (e->bgen ? e->nBz : e->len) * steps;
      need_vec_hist = true;
      break;
    case ADMM_F_UVALS: src = e->uhist; count = e->len * steps; need_vec_hist = true; break;
    case ADMM_F_VVALS:
      src = e->bgen ? e->vthist : e->vhist;
      count = (e->bgen ? e->nBz : e->len) * steps;
      need_vec_hist = true;
      need_fast = true;
      break;
    case ADMM_F_UHATVALS: src = e->uhathist; count = e->len * steps; need_vec_hist = true; need_fast = true; break;
    case ADMM_F_PNORM: src = e->pnorm; count = steps; break;
    case ADMM_F_DNORM: src = e->dnorm; count = steps; break;
    case ADMM_F_PERR: src = e->perr; count = steps; break;
    case ADMM_F_DERR: src = e->derr; count = steps; break;
    case ADMM_F_OBJEVALS: src = e->objv; count = steps; break;
    case ADMM_F_HNORMSQ: src = e->hnorm; count = steps; break;
    case ADMM_F_AVALS: src = e->avals; count = steps; need_fast = true; break;
    case ADMM_F_DVALS: src = e->dvals; count = steps; need_fast = true; break;
    case ADMM_F_RESTARTED: src = e->restarted; count = steps; need_fast = true; break;
    case ADMM_F_WVALS: {  // w = [x; z; rho*u] per iteration (admm.m:678-681)
      if (!e->hist_vectors) return fail(ADMM_E_INVALID, "vector histories were not recorded (options.record_history = 0)");
      const size_t nx = static_cast<size_t>(e->nA), nz = static_cast<size_t>(e->bgen ? e->nBz : e->len),
                   nu = static_cast<size_t>(e->len), nw = nx + nz + nu;
      count = nw * steps;
      if (cap < count) return fail(ADMM_E_CAPACITY, "destination too small");
      if (steps > 0) {
        const size_t pitch = nw * sizeof(double);
        ADMM_HIP_TRY(hipMemcpy2D(dst, pitch, e->xhist, nx * sizeof(double), nx * sizeof(double), steps, hipMemcpyDeviceToHost));
        ADMM_HIP_TRY(hipMemcpy2D(dst + nx, pitch, e->bgen ? e->zthist : e->zhist, nz * sizeof(double), nz * sizeof(double),
                                 steps, hipMemcpyDeviceToHost));
        ADMM_HIP_TRY(hipMemcpy2D(dst + nx + nz, pitch, e->uhist, nu * sizeof(double), nu * sizeof(double), steps,
                                 hipMemcpyDeviceToHost));
        const double rho = e->last_opts.rho;
        for (size_t i = 0; i < steps; ++i)
          for (size_t j = 0; j < nu; ++j) dst[i * nw + nx + nz + j] *= rho;
      }
      if (written) *written = count;
      return ADMM_OK;
    }
    case ADMM_F_CG_ITERS: {
      if (e->xsolve != ADMM_XSOLVE_CG) return fail(ADMM_E_INVALID, "field exists only for xsolve = cg");
      if (cap < 1) return fail(ADMM_E_CAPACITY, "destination too small");
      dst[0] = static_cast<double>(e->cg_total_last);
      if (cap >= 2) dst[1] = static_cast<double>(e->cg_capped_last);  // x-updates that ended on cg_maxit above cg_tol
      if (written) *written = cap >= 2 ? 2 : 1;
      return ADMM_OK;
    }
    case ADMM_F_SPARSE_NNZ:
      if (!e->sparse) return fail(ADMM_E_INVALID, "field exists only for an engine created from a sparse matrix");
      if (cap < 1) return fail(ADMM_E_CAPACITY, "destination too small");
      dst[0] = static_cast<double>(e->sp.nnz);
      if (cap >= 3) {
        dst[1] = static_cast<double>(e->sp.n.plan.lanes);
        dst[2] = static_cast<double>(e->sp.t.plan.lanes);
      }
      if (written) *written = cap >= 3 ? 3 : 1;
      return ADMM_OK;
    case ADMM_F_TV2D_ROW_STAGE:
      if (e->problem != ADMM_PROB_TV2D) return fail(ADMM_E_INVALID, "field exists only for 2-D total variation");
      if (cap < 1) return fail(ADMM_E_CAPACITY, "destination too small");
      dst[0] = static_cast<double>(e->tv2_rows_last);
      if (written) *written = 1;
      return ADMM_OK;
    case ADMM_F_ZCONSENSUS:
      if (e->problem != ADMM_PROB_LASSO_CONSENSUS) return fail(ADMM_E_INVALID, "field exists only for consensus lasso");
      src = e->czc;
      count = e->nA;
      break;
    case ADMM_F_CONS_X:
    case ADMM_F_CONS_U: {
      if (e->problem != ADMM_PROB_LASSO_CONSENSUS) return fail(ADMM_E_INVALID, "field exists only for consensus lasso");
      const size_t K = e->cslices.size();
      count = static_cast<size_t>(e->nA) * K;
      if (cap < count) return fail(ADMM_E_CAPACITY, "destination too small");
      ADMM_HIP_TRY(hipMemcpy2D(dst, e->nA * sizeof(double), field == ADMM_F_CONS_X ? e->cX : e->cU,
                               e->cldn * sizeof(double), e->nA * sizeof(double), K, hipMemcpyDeviceToHost));
      if (written) *written = count;
      return ADMM_OK;
    }
    case ADMM_F_FACTOR: {
      if (!e->F) return fail(ADMM_E_INVALID, "problem has no cached factor");
      count = static_cast<size_t>(e->nF) * e->nF;
      if (cap < count) return fail(ADMM_E_CAPACITY, "destination too small");
      ADMM_HIP_TRY(hipMemcpy2D(dst, e->nF * sizeof(double), e->F, e->ldF * sizeof(double), e->nF * sizeof(double),
                               e->nF, hipMemcpyDeviceToHost));
      // strictly-upper part of the buffer is not part of the factor
      for (int64_t j = 1; j < e->nF; ++j)
        for (int64_t i = 0; i < j; ++i) dst[i + j * e->nF] = 0.0;
      if (written) *written = count;
      return ADMM_OK;
    }
    default:
      return fail(ADMM_E_INVALID, "unknown result field");
  }
  if (need_vec_hist && !e->hist_vectors)
    return fail(ADMM_E_INVALID, "vector histories were not recorded (options.record_history = 0)");
  if (need_fast && !e->hist_fast) return fail(ADMM_E_INVALID, "field exists only for fast/accelerated ADMM runs");
  if (!src) return fail(ADMM_E_INVALID, "field not available for this run");
  if (cap < count) return fail(ADMM_E_CAPACITY, "destination too small");
  if (count) ADMM_HIP_TRY(hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost));
  if (written) *written = count;
  return ADMM_OK;
}

int admm_memcpy_d2h(void* host_dst, const void* device_src, size_t bytes, void* hip_stream) {
  if ((!host_dst || !device_src) && bytes) return fail(ADMM_E_INVALID, "NULL argument");
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ADMM_HIP_TRY(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, st));
  ADMM_HIP_TRY(hipStreamSynchronize(st));
  return ADMM_OK;
}

int admm_memcpy_h2d(void* device_dst, const void* host_src, size_t bytes, void* hip_stream) {
  if ((!device_dst || !host_src) && bytes) return fail(ADMM_E_INVALID, "NULL argument");
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  ADMM_HIP_TRY(hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, st));
  ADMM_HIP_TRY(hipStreamSynchronize(st));
  return ADMM_OK;
}

int admm_engine_info(admm_engine* e, admm_engine_info_t* info) {
  if (!e || !info) return fail(ADMM_E_INVALID, "NULL argument");
  if (info->struct_size != static_cast<int32_t>(sizeof(admm_engine_info_t)))
    return fail(ADMM_E_INVALID, "admm_engine_info_t.struct_size mismatch (ABI version skew)");
  const SliceFactor* f = &e->xfac;
  if (e->problem == ADMM_PROB_LASSO_CONSENSUS && !e->cslices.empty()) f = &e->cslices[0].fac;
  const bool has = f->F != nullptr || f->Minv != nullptr;
  info->xsolve_requested = e->xsolve_requested;
  info->xsolve_used = has ? f->mode : e->xsolve;  // ADMM_XSOLVE_PINV: the caller's Dplus is applied
  info->pinv_used = f->pinv ? 1 : 0;
  info->probed = f->probed ? 1 : 0;
  info->factor_n = has ? f->n : 0;
  info->rank = f->pinv ? f->rank : (has ? f->n : 0);
  info->trsv_blocks = (has && f->mode == ADMM_XSOLVE_TRSV) ? f->trsv.nblk : 0;
  info->jacobi_sweeps = (e->problem == ADMM_PROB_COVSEL) ? static_cast<int32_t>(e->cov_sweeps) : f->jacobi_sweeps;
  info->unwrapped_fused = e->Dp ? 1 : 0;
  info->cond_estimate = has ? f->cond_diag : NAN;
  info->probe_err_inverse = f->probed ? f->err_inv : NAN;
  info->probe_err_trsv = (f->probed || f->err_trsv_one == f->err_trsv_one) ? f->err_trsv : NAN;
  info->probe_err_trsv_one = f->err_trsv_one;
  info->probe_diff = f->probed ? f->probe_diff : NAN;
  // what one iteration's x-solve reads, by cache policy (symv.hip / trsv.hip: tiles below ncached use default loads)
  auto tally = [&](const SliceFactor& s) {
    const int64_t tile_bytes = int64_t{8} * 128 * 128;  // kTile (tri_tile.h)
    if (s.mode == ADMM_XSOLVE_INVERSE && s.Minv && s.n >= kSymvHalfMin) {
      const int64_t tiles = symv_tiles(s.planSy);  // (fp64 or compact tiles: the bytes of the form in use)
      const int64_t cached = std::min<int64_t>(tiles, std::max<int64_t>(0, s.planSy.ncached));
      const int64_t cbytes = symv_tile_prefix_bytes(s.planSy, cached);
      info->xsolve_cacheable_bytes += cbytes;
      info->xsolve_stream_bytes += symv_tile_prefix_bytes(s.planSy, tiles) - cbytes;
    } else if (s.mode == ADMM_XSOLVE_INVERSE && s.Minv) {
      info->xsolve_cacheable_bytes += int64_t{8} * s.n * s.n;  // one wave per column, cache-resident
    } else if (s.mode == ADMM_XSOLVE_TRSV && s.trsv.one) {  // ONE triangle, read by both passes
      const int64_t nt = s.trsv.ntile, tiles = nt * (nt + 1) / 2;
      const int64_t cached = s.trsv.streaming ? std::min<int64_t>(tiles, std::max<int64_t>(0, s.trsv.ncached)) : tiles;
      info->xsolve_cacheable_bytes += 2 * cached * tile_bytes;
      info->xsolve_stream_bytes += 2 * (tiles - cached) * tile_bytes;
    } else if (s.mode == ADMM_XSOLVE_TRSV && s.trsv.Fm) {
      const int64_t nt = s.trsv.ntile, tiles = nt * (nt + 1) / 2;  // per triangle
      const int64_t cached = s.trsv.streaming ? std::min<int64_t>(tiles, std::max<int64_t>(0, s.trsv.ncached)) : tiles;
      info->xsolve_cacheable_bytes += 2 * cached * tile_bytes;
      info->xsolve_stream_bytes += 2 * (tiles - cached) * tile_bytes;
    }
  };
  info->obj_bound_max = e->obj_bound_seen;
  info->obj_form_literal = (e->obj_alt && e->obj_auto && e->obj_gram_bad) ? 1 : 0;
  info->ngroups = e->ngroups;
  info->xsolve_cacheable_bytes = info->xsolve_stream_bytes = 0;
  if (e->problem == ADMM_PROB_LASSO_CONSENSUS) {
    for (const ConsSlice& sl : e->cslices) tally(sl.fac);
  } else if (has) {
    tally(*f);
  }
  return ADMM_OK;
}

int admm_engine_xsolve_storage(admm_engine* e, int32_t* form, int64_t* stored_bytes, double* probe_err_compact,
                               double* probe_err_fp64, double* probe_diff) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  const SliceFactor& f = e->xfac;
  const bool inv = f.mode == ADMM_XSOLVE_INVERSE && f.Minv;
  if (form)
    switch (inv ? f.planSy.cbits : 0) {
      case 0: *form = ADMM_STORAGE_FP64; break;
      case 48: *form = ADMM_STORAGE_COMPACT; break;
      case 40: *form = ADMM_STORAGE_COMPACT40; break;
      case 38: *form = ADMM_STORAGE_COMPACT38; break;
      case 36: *form = ADMM_STORAGE_COMPACT36; break;
      default: return fail(ADMM_E_UNSUPPORTED, "x-solve storage of an unknown width");
    }
  if (stored_bytes) {
    *stored_bytes = 0;
    if (inv && f.planSy.packed) *stored_bytes = symv_tile_prefix_bytes(f.planSy, symv_tiles(f.planSy));
    else if (inv) *stored_bytes = int64_t{8} * f.ldM * f.planSy.npad;
  }
  if (probe_err_compact) *probe_err_compact = f.err_cq;
  if (probe_err_fp64) *probe_err_fp64 = f.err_cq_ref;
  if (probe_diff) *probe_diff = f.cq_diff;
  return ADMM_OK;
}

int admm_engine_xsolve_rejected(admm_engine* e, int32_t cap, int32_t* count, int32_t* bits, double* err_compact,
                                double* err_fp64, double* diff) {
  if (!e || !count || cap < 0)
    return fail(ADMM_E_INVALID, "xsolve_rejected: NULL engine or count, or a negative capacity");
  const SliceFactor& f = e->xfac;
  *count = f.cq_nrejected;
  for (int32_t k = 0; k < f.cq_nrejected && k < cap; ++k) {
    if (bits) bits[k] = f.cq_rejected[k].bits;
    if (err_compact) err_compact[k] = f.cq_rejected[k].err;
    if (err_fp64) err_fp64[k] = f.cq_rejected[k].err_ref;
    if (diff) diff[k] = f.cq_rejected[k].diff;
  }
  return ADMM_OK;
}

int admm_symv_compact_tile_offset(int64_t n, int32_t bits, int64_t t, int64_t* offset) {
  if (n <= 0 || !offset || !symv_cbits_ok(bits))
    return fail(ADMM_E_INVALID, "symv_compact_tile_offset: bad argument (bits 36, 38, 40 or 48)");
  SymvPlan p = symv_plan(n);
  p.packed = true;
  p.cbits = bits;
  if (t < 0 || t > symv_tiles(p)) return fail(ADMM_E_INVALID, "symv_compact_tile_offset: t outside 0 .. tiles");
  *offset = symv_tile_prefix_bytes(p, t);
  return ADMM_OK;
}

int admm_xsolve_compact_accept(double err_compact, double err_fp64, double diff) {
  return symv_compact_accept(err_compact, err_fp64, diff) ? 1 : 0;
}

int admm_engine_setup_seconds(admm_engine* e, double* seconds) {
  if (!e || !seconds) return fail(ADMM_E_INVALID, "NULL argument");
  *seconds = e->setup_seconds;
  return ADMM_OK;
}

int admm_engine_set_profiling(admm_engine* e, int enabled) {
  if (!e) return fail(ADMM_E_INVALID, "engine is NULL");
  e->profiling = enabled < 0 ? 0xffffffffu : static_cast<uint32_t>(enabled);  // bitmask of (1 << ADMM_K_*)
  return ADMM_OK;
}

int admm_engine_set_profiling_stride(admm_engine* e, int stride) {
  if (!e || stride < 1) return fail(ADMM_E_INVALID, "bad argument");
  e->prof_stride = stride;
  return ADMM_OK;
}

int admm_engine_kernel_time(admm_engine* e, int which, double* total_ms, int64_t* launches) {
  if (!e || which < 0 || which >= ADMM_K_COUNT) return fail(ADMM_E_INVALID, "bad argument");
  if (total_ms) *total_ms = e->timers[which].total_ms;
  if (launches) *launches = e->timers[which].launches;
  return ADMM_OK;
}

void admm_engine_destroy(admm_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  free_hist(e);
  for (auto& t : e->timers)
    for (hipEvent_t ev : t.ev) (void)hipEventDestroy(ev);
  e->mem.release();
  sparse_device_free(&e->sp);
  if (e->ctrl_host) (void)hipHostFree(e->ctrl_host);
  if (e->cg_st_host) (void)hipHostFree(e->cg_st_host);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

}  // extern "C"
