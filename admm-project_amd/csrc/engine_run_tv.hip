// engine_run_tv.hip -- the iteration sequences of total variation (totalvariation.m:122-164) and of its 2-D extension
// (spectral or CG x-update): one function or loop object per iteration form, behind the two dispatchers that plan a run.
#include "engine_internal.h"

namespace admm {

// 2-D TV: CG with the direction update fused into the stencil apply (10 instead of 14 vector passes and 3 instead
// of 5 launches per inner iteration); p ping-pongs between cg_p and cg_tmp
int cg_solve_tv2d(admm_engine* e, const double* y) {
  CgArgs a{};
  a.n = e->n;
  a.shift = 1.0;
  a.tol = e->cg_tol;
  a.y = y;
  a.x = e->x;
  a.r = e->cg_r;
  a.p = e->cg_p;
  a.q = e->cg_q;
  a.part = e->cg_part;
  a.st = e->cg_st;
  a.ctrl = e->ctrl;
  const double rho = e->last_opts.rho;
  // the default cap follows the conditioning: I + rho*D'D has its spectrum in [1, 1 + 8 rho), and CG reaches a relative
  // residual tol within 1/2*sqrt(cond)*ln(2/tol) steps -- 500 steps stop short of 1e-11 from rho = 190 on, and the
  // x-update silently lost digits there (2e-4 at rho = 5000; found by the solver sweep on images without a spectral path)
  int32_t maxit = e->cg_maxit;
  if (e->cg_maxit_auto) {
    const double need = 0.5 * std::sqrt(1.0 + 8.0 * rho) * std::log(2.0 / e->cg_tol) + 20.0;
    if (need > maxit) maxit = need < 2.0e5 ? static_cast<int32_t>(need) : 200000;
  }
  a.maxit = maxit;
  ADMM_HIP_TRY(hipMemsetAsync(&e->cg_st->iters, 0, 2 * sizeof(int32_t), e->stream));
  // r = y - (I + rho*D'D) x, p = r, rs, ||y||
  launch_tv2d_laplace(e->tv2_H, e->tv2_W, rho, e->x, e->cg_tmp, e->ctrl, e->stream);
  CgArgs a0 = a;
  a0.p = e->x;
  launch_cg_q(a0, e->cg_tmp, 1, 0, false, e->stream);
  launch_cg_init(a, e->stream);
  double* pbuf[2] = {e->cg_p, e->cg_tmp};
  int cur = 0;
  launch_tv2d_cg_pq(e->tv2_H, e->tv2_W, rho, a, pbuf[1], true, e->stream);  // q = A p, p.q (beta = 0)
  cur = 1;
  const int chunk = e->cg_chunk;  // as long as the previous solve: launches after convergence are no-ops
  for (int done_it = 0; done_it < maxit;) {
    const int k = (maxit - done_it < chunk) ? maxit - done_it : chunk;
    for (int c = 0; c < k; ++c) {
      a.p = pbuf[cur];
      launch_cg_update(a, e->stream);   // alpha, x += alpha p, r -= alpha q, (r.r)_new partials
      launch_tv2d_cg_pq(e->tv2_H, e->tv2_W, rho, a, pbuf[cur ^ 1], false, e->stream);
      cur ^= 1;
      launch_cg_advance(a, e->stream);  // rs <- (r.r)_new, convergence flag
    }
    done_it += k;
    ADMM_HIP_TRY(hipMemcpyAsync(e->cg_st_host, e->cg_st, sizeof(CgState), hipMemcpyDeviceToHost, e->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->cg_st_host->done || e->ctrl_host->stop) break;
  }
  e->cg_chunk = std::min(64, std::max(4, static_cast<int>(e->cg_st_host->iters) + 2));
  return ADMM_OK;
}

// 2-D TV x-update, direct: x = C2' diag(1/(1 + rho*(lamH_i + lamW_j))) C2 y with the 2-D DCT-II C2 (dct.h).
// Three passes over the image (6 N doubles of traffic): column DCT in place, a row stage, inverse column DCT
// (dct.hip: launch_tv2d_xsolve).  The row stage is one of four, picked per run by the rule of dct.hip:
static Tv2Rows tv2d_rows(const admm_engine* e, double rho) {
  return tv2d_row_stage(e->tv2_H, e->tv2_W, rho, e->tv2_rows_dct);
}
static bool toeplitz(Tv2Rows rows) { return rows == Tv2Rows::GREEN || rows == Tv2Rows::COOP; }

// fin != nullptr: the forward transform's launch carries the finalize logic of the previous iteration (when pending)
static int dct_solve_tv2d(admm_engine* e, double* y, const FinArgs* fin = nullptr, bool fin_pending = false) {
  TimerScope ts(e, ADMM_K_XSOLVE);
  const double rho = e->last_opts.rho;
  // (THOMAS: factors in e->cg_p / e->cg_q, set up by run_total_variation_2d)
  launch_tv2d_xsolve(y, e->x, e->tv2_H, e->tv2_W, rho, tv2d_rows(e, rho), e->dctH, e->dctW, e->cg_p, e->cg_q, e->ctrl,
                     e->stream, fin, fin_pending);
  return ADMM_OK;
}

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// the initial iterates were written to e->z / e->u; make buffer A the current one
int make_buffer_a_current(admm_engine* e, int64_t len) {
  if (e->z == e->tv_zA) return ADMM_OK;
  ADMM_HIP_TRY(hipMemcpyAsync(e->tv_zA, e->z, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));
  ADMM_HIP_TRY(hipMemcpyAsync(e->tv_uA, e->u, sizeof(double) * len, hipMemcpyDeviceToDevice, e->stream));
  return ADMM_OK;
}

// The batch-and-poll loop of every form in this file: iterate(k, last) enqueues iteration k (last: the host polls
// behind it), at most `every` iterations between two polls (see engine_run_general.hip), until N are enqueued or the
// device has raised stop.  e->ctrl_host holds the last poll's control block afterwards.
template <class Iterate>
int run_batches(admm_engine* e, int32_t N, int32_t every, Iterate&& iterate) {
  int32_t done = 0;
  bool stop_seen = false;
  while (done < N && !stop_seen) {
    const int32_t batch = (N - done < every) ? N - done : every;
    for (int32_t b = 0; b < batch; ++b) ADMM_TRY(iterate(done + b, b + 1 == batch));
    done += batch;
    ADMM_TRY(poll_ctrl(e));
    if (e->ctrl_host->stop) stop_seen = true;
  }
  return ADMM_OK;
}

// One unfused iteration, 1-D and 2-D.  Fast / accelerated ADMM (admm.m:267-298, 563-600): the x-update takes
// (v, uhat), the generic fused prox kernel does the z/u update, extrapolation, histories and partial sums on the
// vector D*x, and the D' stencils of the dual residual come from dz = z - zprev and u.  What differs between the two
// problems is handed in: x_solve (right-hand side and x-update), dx (D*x into e->tmpA, the objective's partials and
// their count), relax_z (the over-relaxed z of the 1-D solver; a no-op otherwise) and dual (the D' stencils).
template <class XSolve, class Dx, class RelaxZ, class Dual>
int unfused_iteration(admm_engine* e, RunState& rs, XSolve&& x_solve, Dx&& dx, RelaxZ&& relax_z, Dual&& dual) {
  ProxArgs& pa = rs.pa;
  FinArgs& fa = rs.fa;
  ADMM_TRY(x_solve());
  int nob = 0, nblk = 1;
  dx(&nob);
  {
    TimerScope ts(e, ADMM_K_PROX);
    pa.axsrc = e->tmpA;
    pa.naxpart = 1;
    pa.axld = 0;
    relax_z();
    launch_prox(pa, e->ctrl, &nblk, e->stream);
  }
  fa.nblk = nblk;
  fa.slots_reduced = nullptr;
  fa.objp_reduced = nullptr;
  if (rs.alg == 2) {
    launch_fast_decide(fa, e->stream);
    launch_extrapolate(rs.xa, e->ctrl, e->stream);
  }
  dual(nblk);
  fa.objpart = rs.o.objevals ? e->objpart : nullptr;
  fa.nobjpart = rs.o.objevals ? nob : 0;
  TimerScope ts(e, ADMM_K_FINALIZE);
  launch_finalize(fa, e->stream);
  return ADMM_OK;
}

// ---- 2-D

// what both 2-D loops end with: z, u are in buffer A; the CG counters of the run
int finish_tv2d(admm_engine* e, const RunState& rs, double runtime, admm_run_summary* summary) {
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  e->z = e->tv_zA;
  e->u = e->tv_uA;
  ADMM_HIP_TRY(hipMemcpy(e->cg_st_host, e->cg_st, sizeof(CgState), hipMemcpyDeviceToHost));
  e->cg_total_last = e->cg_st_host->total;
  e->cg_capped_last = e->cg_st_host->capped;
  return finish_run(e, rs.o, rs.N, runtime, summary);
}

// the CG path synchronises inside every solve anyway and polls behind every iteration; the spectral path runs
// check_every iterations ahead (everything enqueued after the stop flag is a no-op)
int32_t tv2d_poll_every(const RunState& rs, bool spectral) { return spectral ? rs.check_every : 1; }

// Fast / accelerated ADMM, as for the 1-D solver (unfused_iteration).  z, u live in buffer A, updated in place.
int run_tv2d_fast(admm_engine* e, RunState& rs, Tv2Args& ta, bool spectral, admm_run_summary* summary) {
  const admm_options& o = rs.o;
  ProxArgs& pa = rs.pa;
  FinArgs& fa = rs.fa;
  ExtrapArgs& xa = rs.xa;
  const auto t0 = Clock::now();
  if (!e->dz) ADMM_TRY(e->mem.alloc(&e->dz, round_up(rs.len, 2)));
  if (!e->tmpA) ADMM_TRY(e->mem.alloc(&e->tmpA, round_up(rs.len, 2)));
  pa.z = e->tv_zA;
  pa.u = e->tv_uA;
  xa.z = e->tv_zA;
  xa.u = e->tv_uA;
  xa.rhs = nullptr;
  pa.dz = e->dz;
  pa.prox = ta.isotropic ? PROX_PAIR : PROX_SOFT;
  pa.t = e->lambda / o.rho;  // getProxOps.m:199
  pa.objz = OBJZ_NONE;
  pa.objx = OBJX_NONE;
  pa.x_out = nullptr;
  pa.xhist = nullptr;
  pa.rhs = nullptr;
  pa.rhs_kind = RHS_NONE;
  pa.a_identity = 0;
  pa.c = nullptr;
  pa.ax_t = nullptr;
  fa.obj_scale_x = 0.0;
  fa.obj_scale_z = 0.0;
  fa.obj_scale_part = o.objevals ? 1.0 : 0.0;
  if (pa.prox == PROX_PAIR && !prox_pair_ok(pa)) return fail(ADMM_E_INVALID, "the pair prox needs a vector of two halves");
  auto x_solve = [&]() -> int {
    ta.z = e->v;  // x = xminf(x, v, uhat, rho)   admm.m:506
    ta.u = e->uhat;
    {
      TimerScope ts(e, ADMM_K_XSOLVE);
      launch_tv2d_rhs(ta, e->rhs, e->ctrl, e->stream);
    }
    return spectral ? dct_solve_tv2d(e, e->rhs) : cg_solve(e, e->rhs);
  };
  auto dx = [&](int* nob) {
    launch_tv2d_dx(ta.H, ta.W, e->lambda, o.objevals, e->x, e->s, e->tmpA, e->objpart, nob, e->xhist, e->ctrl,
                   e->stream, ta.isotropic != 0);
  };
  auto dual = [&](int nblk) { launch_tv2d_dual_vec(ta.H, ta.W, e->dz, e->tv_uA, e->part, nblk, e->ctrl, e->stream); };
  ADMM_TRY(run_batches(e, rs.N, tv2d_poll_every(rs, spectral), [&](int32_t, bool) {
    return unfused_iteration(e, rs, x_solve, dx, [] {}, dual);
  }));
  return finish_tv2d(e, rs, seconds_since(t0), summary);
}

// Plain ADMM carries the compact state v = z + u between iterations (tv2d.hip): iteration 0 reads z, u from buffer A
// and writes v into V0 = tv_zB, iteration k reads V((k-1)&1) and writes V(k&1), V1 = tv_uB; the last executed
// iteration's v is expanded into buffer A after the loop.
// Deferred tail (spectral x-update): the finalize logic of iteration i rides in the first launch of iteration i + 1
// (dct_cols_forward_fin_kernel); a batch's last iteration gets the stand-alone launch.  A stop it raises turns the
// rest of iteration i + 1 into no-ops -- only the in-place transform of the right-hand side has run by then.
struct Tv2dPlainLoop {
  admm_engine* e;
  RunState& rs;
  Tv2Args& ta;
  // ---- fixed for the run
  const bool spectral;
  const bool glued;      // the three-launch iteration (iterate_glued); every other shape takes four launches, or CG
  // ---- carried between iterations
  bool pending = false;  // the previous iteration left its finalize to this iteration's first launch

  int run(admm_run_summary* summary) {
    const auto t0 = Clock::now();
    ADMM_TRY(run_batches(e, rs.N, tv2d_poll_every(rs, spectral),
                         [&](int32_t k, bool last) { return iterate(k, last); }));
    const double runtime = seconds_since(t0);
    const int32_t steps = e->ctrl_host->steps;
    if (steps > 0)  // z, u of the last executed iteration
      launch_tv2d_expand((steps - 1) & 1 ? e->tv_uB : e->tv_zB, ta.thresh, rs.len, e->tv_zA, e->tv_uA, e->stream,
                         ta.isotropic != 0);
    return finish_tv2d(e, rs, runtime, summary);
  }

  int iterate(int32_t k, bool last) {
    double* const vbuf[2] = {e->tv_zB, e->tv_uB};
    ta.z = k == 0 ? e->tv_zA : vbuf[(k - 1) & 1];
    ta.u = k == 0 ? e->tv_uA : nullptr;
    ta.zo = vbuf[k & 1];
    if (k == 0) {  // later right-hand sides come out of the fused z/u pass of the previous iteration
      TimerScope ts(e, ADMM_K_XSOLVE);
      launch_tv2d_rhs(ta, e->rhs, e->ctrl, e->stream);
      if (glued) launch_dct_cols_forward(e->rhs, ta.H, ta.W, e->dctH, e->ctrl, e->stream);
    }
    const bool passenger = pending;
    pending = !last;  // finalized by the next iteration's first launch (CG: every iteration is a batch's last)
    int nblk = 1;
    if (glued) iterate_glued(k, passenger, &nblk);
    else ADMM_TRY(iterate_four(k, passenger, &nblk));
    rs.fa.nblk = nblk;
    if (last) {
      TimerScope ts(e, ADMM_K_FINALIZE);
      launch_finalize(rs.fa, e->stream);
    }
    return ADMM_OK;
  }

  // Glued spectral form (Toeplitz row stage, power-of-two height): the fused pass hands its right-hand side to the
  // forward column transform inside one kernel (dct.hip: tv2d_fused_dct_kernel), so e->rhs holds the TRANSFORMED
  // right-hand side from one iteration to the next and an iteration is three launches: row stage (+ the previous
  // iteration's finalize as a passenger) into the scratch image e->cg_r, inverse column transform into x, fused pass +
  // forward transform.  (The row stage writes a scratch image, not x: it is the launch that carries the passenger, so
  // it still runs when the passenger raises stop.)
  void iterate_glued(int32_t k, bool passenger, int* nblk) {
    {
      TimerScope ts(e, ADMM_K_XSOLVE);
      launch_tv2d_rows_green(e->rhs, e->cg_r, ta.H, ta.W, rs.o.rho, e->dctH, e->ctrl, e->stream, &rs.fa, passenger);
      launch_dct_cols_inverse(e->cg_r, e->x, ta.H, ta.W, e->dctH, e->ctrl, e->stream);
    }
    TimerScope ts(e, ADMM_K_PROX);
    launch_tv2d_fused_dct(ta, k > 0, e->rhs, e->dctH, e->ctrl, nblk, e->stream);
  }

  // Every other spectral shape -- non-power-of-two heights (chirp column transform), the row DCT, the Thomas row
  // stage -- takes four launches: dct_solve_tv2d, then the fused pass.  Without a column transform the x-update
  // (I + rho*D'D) x = s + rho*D'(z - u) is warm-started CG (polls the device).
  int iterate_four(int32_t k, bool passenger, int* nblk) {
    if (spectral) ADMM_TRY(dct_solve_tv2d(e, e->rhs, &rs.fa, passenger));
    else ADMM_TRY(cg_solve(e, e->rhs));
    TimerScope ts(e, ADMM_K_PROX);
    launch_tv2d_fused(ta, k > 0, e->rhs, e->ctrl, nblk, e->stream);
    return ADMM_OK;
  }
};

}  // namespace

int run_total_variation_2d(admm_engine* e, RunState& rs, admm_run_summary* summary) {
  const admm_options& o = rs.o;
  FinArgs& fa = rs.fa;
  // the z-closure of totalvariation.m applies D to what it is handed (getProxOps.m:199); with D of size 2N x N the
  // relaxed Axhat (2N elements, admm.m:517) does not fit: a dimension error, as for the linear SVM (getProxOps.m:1088)
  if (o.relax != 1.0)
    return fail(ADMM_E_INVALID, "relaxation with the 2-D total-variation prox is a dimension error (D is 2N x N)");
  // spectral x-update whenever the height has a column transform (one of the three row stages always applies);
  // CG otherwise
  const bool spectral = e->tv2_dct;
  const Tv2Rows rows = tv2d_rows(e, o.rho);
  if (spectral && rows == Tv2Rows::THOMAS)  // the elimination factors of this run's rho
    launch_tv2d_rows_thomas_setup(e->tv2_H, e->tv2_W, o.rho, e->dctH, e->cg_p, e->cg_q, e->stream);
  e->tv2_rows_last = spectral ? static_cast<int32_t>(rows) : 0;
  ADMM_TRY(make_buffer_a_current(e, rs.len));
  Tv2Args ta{};
  ta.H = e->tv2_H;
  ta.W = e->tv2_W;
  ta.rho = o.rho;
  ta.thresh = e->lambda / o.rho;
  ta.s = e->s;
  ta.x = e->x;
  ta.objevals = o.objevals;
  ta.isotropic = e->tv2_isotropic;  // admm_engine_set_tv2d_isotropic: the pair prox and the pair norms in S_OBJZ
  ta.xhist = e->xhist;
  ta.zhist = e->zhist;
  ta.uhist = e->uhist;
  ta.part = e->part;
  fa.g = nullptr;
  fa.x = nullptr;
  fa.xhist = nullptr;
  fa.dual_from_slots = 1;
  if (o.objevals) {  // 1/2*||x - s||^2 + lambda*||D x||_1 (isotropic: lambda * the sum of the pair norms, the same scales)
    fa.obj_scale_x = 0.5;
    fa.obj_scale_z = e->lambda;
  }
  if (rs.alg != 0) return run_tv2d_fast(e, rs, ta, spectral, summary);
  const bool glued = spectral && toeplitz(rows) && e->dctH.bm == 0;
  return Tv2dPlainLoop{e, rs, ta, spectral, glued}.run(summary);
}

namespace {

// The form of a 1-D iteration (tv.hip), fixed for a run by the plan's halo, n and the ADMM variant
enum class TvForm {
  DIRECT,   // plain ADMM, halo <= 248: one launch without the y vector, 3-5 vector passes (launch_tv_direct)
  FUSED,    // plain ADMM, halo 250..256 (too wide for the direct kernels' margin) or n = 1: tv_fused_kernel, 7 passes
  SWEEP,    // plain ADMM, halo > 256 (rho >~ 37): two sweeps and tv_prox, three launches
  UNFUSED,  // fast / accelerated ADMM or over-relaxation: sweeps, tv_dx, the generic prox kernel, tv_dual
};
TvForm tv_form(const TvArgs& ta, int alg, double relax) {
  if (alg != 0 || relax != 1.0) return TvForm::UNFUSED;
  if (!tv_fused_ok(ta)) return TvForm::SWEEP;
  return tv_direct_ok(ta) ? TvForm::DIRECT : TvForm::FUSED;
}
// what only the direct kernels read: their window margin and tile, the Green's-function scale and r^1 .. r^8
void set_direct_fields(TvArgs& ta) {
  ta.margin = tv_direct_margin(ta);
  ta.ftile = 256 * kTvDirectE - 2 * ta.margin;
  const double rr = ta.rho / ta.bstar;
  ta.green = 1.0 / (ta.bstar * (1.0 - rr * rr));
  ta.rpow[0] = rr;
  for (int k = 1; k < 8; ++k) ta.rpow[k] = ta.rpow[k - 1] * rr;
}

// z, u ping-pong between buffers A and B: iteration k reads A when k is even
void tv_ping_pong(admm_engine* e, TvArgs& ta, int64_t k) {
  const bool a_cur = (k & 1) == 0;
  ta.z = a_cur ? e->tv_zA : e->tv_zB;
  ta.u = a_cur ? e->tv_uA : e->tv_uB;
  ta.zo = a_cur ? e->tv_zB : e->tv_zA;
  ta.uo = a_cur ? e->tv_uB : e->tv_uA;
}
// ... and the iterations executed on the device decide which of the two holds the final z, u
void tv_result_by_parity(admm_engine* e, int32_t steps) {
  e->z = (steps & 1) ? e->tv_zB : e->tv_zA;
  e->u = (steps & 1) ? e->tv_uB : e->tv_uA;
}

// UNFUSED: fast / accelerated ADMM (unfused_iteration); z, u are updated in place.  Over-relaxation (admm.m:515-532)
// takes the same route: the reference's z-closure applies D to the relaxed Axhat it is handed (getProxOps.m:199), so z
// comes from launch_tv_relax_z and the generic kernel does everything else with z given (PROX_GIVEN).
int run_tv_unfused(admm_engine* e, RunState& rs, TvArgs& ta, admm_run_summary* summary) {
  const admm_options& o = rs.o;
  const int alg = rs.alg;
  ProxArgs& pa = rs.pa;
  FinArgs& fa = rs.fa;
  const bool relaxed = o.relax != 1.0;
  if (relaxed && !e->zext) ADMM_TRY(e->mem.alloc(&e->zext, round_up(rs.len, 2)));
  if (!e->dz) ADMM_TRY(e->mem.alloc(&e->dz, round_up(rs.len, 2)));
  if (!e->tmpA) ADMM_TRY(e->mem.alloc(&e->tmpA, round_up(rs.len, 2)));
  pa.dz = e->dz;
  pa.t = e->lambda / o.rho;  // getProxOps.m:199
  pa.objz = OBJZ_NONE;
  pa.objx = OBJX_NONE;
  pa.x_out = nullptr;
  fa.obj_scale_x = 0.0;
  fa.obj_scale_z = 0.0;
  fa.obj_scale_part = o.objevals ? 1.0 : 0.0;
  ta.part = e->part;
  const auto t0 = Clock::now();
  auto x_solve = [&]() -> int {
    ta.z = alg ? e->v : e->z;  // x = xminf(x, v, uhat, rho)   admm.m:506 (plain ADMM: z, u)
    ta.u = alg ? e->uhat : e->u;
    ta.y = e->tv_y;
    TimerScope ts(e, ADMM_K_XSOLVE);
    launch_tv_sweep(ta, false, e->ctrl, e->stream);
    launch_tv_sweep(ta, true, e->ctrl, e->stream);
    return ADMM_OK;
  };
  auto dx = [&](int* nob) {
    launch_tv_dx(e->x, e->s, e->n, e->lambda, o.objevals, e->tmpA, e->objpart, nob, e->ctrl, e->stream);
  };
  auto relax_z = [&] {
    if (!relaxed) return;
    // admm.m:517-523: Axhat from z_prev; zming(Axhat, z, u | uhat, rho) -- fast ADMM hands it uhat
    launch_tv_relax_z(e->tmpA, e->z, alg ? e->uhat : e->u, e->n, o.relax, pa.t, e->zext, e->ctrl, e->stream);
    pa.prox = PROX_GIVEN;
    pa.zgiven = e->zext;
  };
  auto dual = [&](int nblk) { launch_tv_dual(e->dz, e->u, e->n, e->part, nblk, e->ctrl, e->stream); };
  ADMM_TRY(run_batches(e, rs.N, rs.check_every, [&](int32_t, bool) {
    return unfused_iteration(e, rs, x_solve, dx, relax_z, dual);
  }));
  ADMM_TRY(poll_ctrl(e));
  return finish_run(e, o, rs.N, seconds_since(t0), summary);
}

// SWEEP: two sweeps, tv_prox, finalize
int run_tv_sweep(admm_engine* e, RunState& rs, TvArgs& ta, admm_run_summary* summary) {
  FinArgs& fa = rs.fa;
  const auto t0 = Clock::now();
  ADMM_TRY(run_batches(e, rs.N, rs.check_every, [&](int32_t k, bool) {
    tv_ping_pong(e, ta, k);
    int nblk = 1;
    {
      TimerScope ts(e, ADMM_K_XSOLVE);
      launch_tv_sweep(ta, false, e->ctrl, e->stream);
      launch_tv_sweep(ta, true, e->ctrl, e->stream);
    }
    {
      TimerScope ts(e, ADMM_K_PROX);
      launch_tv_prox(ta, e->ctrl, &nblk, e->stream);
    }
    fa.nblk = nblk;
    TimerScope ts(e, ADMM_K_FINALIZE);
    launch_finalize(fa, e->stream);
    return ADMM_OK;
  }));
  ADMM_TRY(poll_ctrl(e));
  tv_result_by_parity(e, e->ctrl_host->steps);
  return finish_run(e, rs.o, rs.N, seconds_since(t0), summary);
}

// DIRECT and FUSED: one launch per iteration, tile partials (one column per tile) and the deferred tail.
// The tile-partial sums and the finalize logic of iteration i are done by one extra workgroup of iteration i + 1's
// launch, hidden behind its tiles; a batch's last iteration gets the two small launches.  A stop raised by that
// workgroup makes iteration i + 2 a no-op; iteration i + 1 has run speculatively into the OTHER ping-pong buffers, and
// the final z, u, x are picked by the device's step count.
struct TvOneLaunch {
  admm_engine* e;
  RunState& rs;
  TvArgs& ta;
  FinArgs& fa;
  // ---- fixed for the run
  const bool direct;
  int64_t ntiles = 0;
  // two sets of tile partials, pset doubles each: the deferred tail of iteration i reads its set while iteration i + 1
  // writes the other
  int64_t pset = 0;
  // The forward-sweep vector iteration i read must survive iteration i + 1 (the final x is rebuilt from it when no
  // history holds x): three y buffers in rotation instead of two.  The direct kernels have no y and carry the compact
  // state v = z + u (tv.hip): iteration 0 reads z, u from buffer A, iteration k reads v from vbuf[(k-1) % 3] and writes
  // vbuf[k % 3] -- three buffers, so that the speculative iteration behind a stop overwrites neither the last executed
  // iteration's output nor its input (the final x is recomputed from the z, u it read).
  double* ybuf[3] = {nullptr, nullptr, nullptr};
  double* vbuf[3] = {nullptr, nullptr, nullptr};
  // ---- carried between iterations
  bool pending = false;  // the last enqueued iteration's tail is still to be done
  Clock::time_point t0;

  TvOneLaunch(admm_engine* eng, RunState& r, TvArgs& t, bool dir) : e(eng), rs(r), ta(t), fa(r.fa), direct(dir) {}

  int run(admm_run_summary* summary) {
    ADMM_TRY(plan_partials());
    t0 = Clock::now();
    ADMM_TRY(prime());
    ADMM_TRY(run_batches(e, rs.N, rs.check_every, [&](int32_t k, bool last) {
      iterate(k);
      if (last) stand_alone_tail(k);
      return ADMM_OK;
    }));
    return finish(summary);
  }

  int plan_partials() {
    ta.part_stride = round_up(ceil_div(e->n, ta.ftile), 2);
    const size_t want = 2 * static_cast<size_t>(S_COUNT) * ta.part_stride;
    if (want > e->tv_part_cap) {  // (a per-run hipMalloc / hipFree pair costs more than 100 iterations at n = 2^24)
      ADMM_TRY(e->mem.alloc(&e->tv_part, want));
      e->tv_part_cap = want;
    }
    ta.part = e->tv_part;
    ntiles = ceil_div(e->n, ta.ftile);
    pset = static_cast<int64_t>(S_COUNT) * ta.part_stride;
    return ADMM_OK;
  }

  // x only leaves the 7-pass kernel when its history is recorded; otherwise one backward sweep after the loop rebuilds
  // the final x from the forward-sweep vector the last executed iteration read (x leaves the direct kernels only as a
  // history column; the final x is recomputed after the loop)
  int prime() {
    if (direct) {
      if (!e->tv_v3) ADMM_TRY(e->mem.alloc(&e->tv_v3, round_up(e->n, 2)));
    } else {
      ta.skip_x = e->xhist ? 0 : 1;
      {  // the forward sweep of iteration 0; every later one is produced by the fused kernel
        TimerScope ts(e, ADMM_K_XSOLVE);
        ta.z = e->tv_zA;
        ta.u = e->tv_uA;
        ta.y = e->tv_y;
        launch_tv_sweep(ta, false, e->ctrl, e->stream);
      }
      if (!e->tv_y3) ADMM_TRY(e->mem.alloc(&e->tv_y3, round_up(e->n, 2)));
    }
    ybuf[0] = e->tv_y, ybuf[1] = e->tv_y2, ybuf[2] = e->tv_y3;
    vbuf[0] = e->tv_zB, vbuf[1] = e->tv_uB, vbuf[2] = e->tv_v3;
    return ADMM_OK;
  }

  void iterate(int64_t k) {
    TimerScope ts(e, ADMM_K_XSOLVE);
    ta.deferred = 1;
    ta.iter_host = k;
    ta.part = e->tv_part + (k & 1) * pset;
    ta.prev_part = e->tv_part + ((k + 1) & 1) * pset;
    ta.prev_ntiles = static_cast<int32_t>(ntiles);
    ta.slots16 = e->red;
    ta.fin_pending = pending ? 1 : 0;
    fa.nblk = 1;
    fa.slots_reduced = e->red;
    if (direct) {
      ta.state_in = k > 0 ? 1 : 0;
      ta.z = k > 0 ? vbuf[(k - 1) % 3] : e->tv_zA;
      ta.u = k > 0 ? nullptr : e->tv_uA;
      ta.zo = vbuf[k % 3];
      ta.uo = nullptr;
      launch_tv_direct(ta, fa, e->ctrl, e->stream);
    } else {
      tv_ping_pong(e, ta, k);
      ta.yin = ybuf[k % 3];
      ta.yout = ybuf[(k + 1) % 3];
      launch_tv_fused(ta, fa, e->ctrl, e->stream);
    }
    pending = true;
  }

  // the batch's last iteration k: its tail as two small launches
  void stand_alone_tail(int64_t k) {
    launch_tv_pack(e->tv_part + (k & 1) * pset, ta.part_stride, static_cast<int32_t>(ntiles), e->red, e->ctrl,
                   e->stream);
    fa.slots_reduced = e->red;
    fa.nblk = 1;
    launch_finalize(fa, e->stream);
    pending = false;
  }

  // x, z, u of the last executed iteration, picked or rebuilt from the device's step count
  int finish(admm_run_summary* summary) {
    ADMM_TRY(poll_ctrl(e));
    const int32_t steps = e->ctrl_host->steps;
    ADMM_TRY(direct ? result_direct(steps) : result_fused(steps));
    return finish_run(e, rs.o, rs.N, seconds_since(t0), summary);
  }

  int result_direct(int32_t steps) {
    if (steps > 0) {
      if (e->xhist) ADMM_TRY(restore_x_from_history(steps));
      else rebuild_x_by_sweeps(steps);
      expand_state_into_a(vbuf[(steps - 1) % 3]);  // z, u of the last executed iteration
    }
    e->z = e->tv_zA;
    e->u = e->tv_uA;
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    return ADMM_OK;
  }

  int result_fused(int32_t steps) {
    tv_result_by_parity(e, steps);
    if (steps == 0) return ADMM_OK;
    return e->xhist ? restore_x_from_history(steps) : backward_sweep_from_y(steps);  // (no history: ta.skip_x)
  }

  // x was overwritten by the speculative iteration after a stop
  int restore_x_from_history(int32_t steps) {
    ADMM_HIP_TRY(hipMemcpyAsync(e->x, e->xhist + static_cast<int64_t>(steps - 1) * e->n, sizeof(double) * e->n,
                                hipMemcpyDeviceToDevice, e->stream));
    return ADMM_OK;
  }

  // x of the last executed iteration, from the z, u it read: two stand-alone sweeps
  void rebuild_x_by_sweeps(int32_t steps) {
    if (steps > 1) expand_state_into_a(vbuf[(steps - 2) % 3]);
    ta.z = e->tv_zA;
    ta.u = e->tv_uA;
    ta.y = e->tv_y;
    ta.x = e->x;
    ta.xhist = nullptr;
    launch_tv_sweep(ta, false, e->ctrl_idle, e->stream);  // the loop's own flag says "stopped" by now
    launch_tv_sweep(ta, true, e->ctrl_idle, e->stream);
  }

  // z, u out of the compact state v = z + u
  void expand_state_into_a(const double* v) {
    launch_tv2d_expand(v, ta.thresh, e->n, e->tv_zA, e->tv_uA, e->stream);
  }

  // x of the last executed iteration from the forward-sweep vector it read
  int backward_sweep_from_y(int32_t steps) {
    ta.y = ybuf[(steps - 1) % 3];
    launch_tv_sweep(ta, true, e->ctrl_idle, e->stream);  // the loop's own flag says "stopped" by now
    ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
    return ADMM_OK;
  }
};

}  // namespace

int run_total_variation(admm_engine* e, RunState& rs, admm_run_summary* summary) {
  const admm_options& o = rs.o;
  FinArgs& fa = rs.fa;
  std::vector<double> prefix;
  double bstar = 0.0;
  int halo = 0, elems = 0, tile = 0;
  ADMM_TRY(tv_plan(o.rho, e->n, &prefix, &bstar, &halo, &elems, &tile));
  if (prefix.size() > e->tv_bprefix_cap) {
    ADMM_TRY(e->mem.alloc(&e->tv_bprefix, prefix.size()));
    e->tv_bprefix_cap = prefix.size();
  }
  ADMM_HIP_TRY(hipMemcpyAsync(e->tv_bprefix, prefix.data(), sizeof(double) * prefix.size(), hipMemcpyHostToDevice,
                              e->stream));
  ADMM_TRY(make_buffer_a_current(e, rs.len));
  ADMM_HIP_TRY(hipStreamSynchronize(e->stream));
  TvArgs ta{};
  ta.n = e->n;
  ta.rho = o.rho;
  ta.thresh = e->lambda / o.rho;
  ta.s = e->s;
  ta.x = e->x;
  ta.y = e->tv_y;
  ta.bprefix = e->tv_bprefix;
  ta.nprefix = static_cast<int64_t>(prefix.size());
  ta.bstar = bstar;
  ta.halo = halo;
  ta.elems = elems;
  ta.tile = tile;
  ta.ftile = 256 * elems - 2 * halo - 4;
  ta.objevals = o.objevals;
  ta.xhist = e->xhist;
  ta.zhist = e->zhist;
  ta.uhist = e->uhist;
  ta.part = e->part;
  fa.g = nullptr;
  fa.x = nullptr;
  fa.xhist = nullptr;
  fa.dual_from_slots = 1;
  if (o.objevals) {  // totalvariation.m:134-135
    fa.obj_scale_x = 0.5;
    fa.obj_scale_z = e->lambda;
  }
  const TvForm form = tv_form(ta, rs.alg, o.relax);
  if (form == TvForm::UNFUSED) return run_tv_unfused(e, rs, ta, summary);
  if (form == TvForm::SWEEP) return run_tv_sweep(e, rs, ta, summary);
  if (form == TvForm::DIRECT) set_direct_fields(ta);
  return TvOneLaunch(e, rs, ta, form == TvForm::DIRECT).run(summary);
}

}  // namespace admm
