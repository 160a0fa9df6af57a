// spmm_cg.hip -- lock-step CG on (D'D + shift*I) x = y for K right-hand sides over one sparse product (spmm_cg.h;
// DESIGN.md q37, q39).  Nothing n x n: the first solve of a run starts from 0 and every later one from the previous x, so
// without a shift every iterate stays in range(D'); with shift > 0 the matrix is positive definite.  Per solve, every launch for all K fits at once (blockIdx.y = chunk of kSpmmChunk fits):
//   scg_init / _start             r = y - D'(D x), p = r, per-fit rs and ||y||
//   per inner iteration           T = D P, Q = D' T (two SpMM), scg_dot / _update / _direction / _advance
// A fit whose stop flag is set is FROZEN, and a fit whose solve is done is masked until the next solve: every kernel and
// every product skips it.  Every sum runs in a fixed order that depends on the sizes alone.
// The stand-alone operator admm_op_spmm_cg runs SpmmCg::solve once on host arrays.
#include "spmm_cg.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "multi_host.h"

namespace admm {

namespace {

constexpr int KC = kSpmmChunk;

// the sum of a slot's nb workgroup partials for every fit of `chunk`; each thread returns its own fit's.  Wave w
// sums the fits w, w + kScgWaves, ...: lane l adds the partials l, l + 64, ... in that order, then the shuffle tree.
__device__ __forceinline__ double scg_total(const double* part, int nstot, int slot, int chunk, int nb, double* lds) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int c = wid; c < KC; c += kScgWaves) {
    const double* __restrict__ p = part + ((static_cast<int64_t>(chunk) * KC + c) * nstot + slot) * kScgMaxWg;
    double v = 0.0;
    for (int b = lane; b < nb; b += kWave) v += p[b];
    v = wave_sum(v);
    if (lane == 0) lds[c] = v;
  }
  __syncthreads();
  return lds[threadIdx.x % KC];
}

// qv = Q[e] + shift * V[e] as ONE fma (spmm_cg.h); without SHIFT it is Q[e] and V is never read
template <bool SHIFT>
__device__ __forceinline__ double scg_qv(const ScgArgs& a, const double* V, int64_t e) {
  if constexpr (SHIFT) return fma(a.shift, V[e], a.Q[e]);
  else return a.Q[e];
}

// r = y - qv, p = r, partials of r.r and y.y.  FIRST: the first x-update of a run starts from x = 0 (r = y)
template <bool FIRST, bool SHIFT>
__global__ __launch_bounds__(kScgBlock) void scg_init_kernel(ScgArgs a) {
  __shared__ double lds[2 * kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[2] = {0.0, 0.0};
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (l.run && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      const double yv = a.Y[e];
      double rv = yv;
      if (FIRST) a.X[e] = 0.0;
      else rv = yv - scg_qv<SHIFT>(a, a.X, e);
      a.R[e] = rv;
      a.P[e] = rv;
      acc[0] += rv * rv;
      acc[1] += yv * yv;
    }
  }
  scg_sums<2>(acc, lds, a.part, 2, 0);
}

// one workgroup per chunk: rs, ||y||, and whether x is already good enough.  A zero right-hand side ends the solve with
// x = 0 (scg_update_kernel stores it)
__global__ __launch_bounds__(kScgBlock) void scg_start_kernel(ScgArgs a, int nb) {
  __shared__ double l0[KC], l1[KC];
  const ScgLane l = scg_lane(a.rec, a.K);
  if (!__syncthreads_or(l.run)) return;
  const double rs = scg_total(a.part, 2, 0, blockIdx.y, nb, l0);
  const double yy = scg_total(a.part, 2, 1, blockIdx.y, nb, l1);
  if (l.r == 0 && l.run) {
    ScgState* st = a.st + l.fit;
    const bool zero = yy == 0.0;
    st->rs = rs;
    st->ynorm = sqrt(yy);
    st->iters = 0;
    st->brk = 0;
    st->zero = zero ? 1 : 0;
    st->done = (zero || sqrt(rs) <= a.tol * sqrt(yy)) ? 1 : 0;
  }
}

template <bool SHIFT>
__global__ __launch_bounds__(kScgBlock) void scg_dot_kernel(ScgArgs a) {
  __shared__ double lds[kScgBlock];
  const ScgLane l = scg_lane(a.rec, a.K);
  const bool live = l.run && a.st[l.run ? l.fit : 0].done == 0;
  if (!__syncthreads_or(live)) return;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[1] = {0.0};
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (live && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      acc[0] += a.P[e] * scg_qv<SHIFT>(a, a.P, e);
    }
  }
  scg_sums<1>(acc, lds, a.part, 2, 0);
}

// alpha = rs / (p.qv); x += alpha p; r -= alpha qv; partial r.r.  p.qv == 0: nothing is divided or updated, the fit ends
template <bool SHIFT>
__global__ __launch_bounds__(kScgBlock) void scg_update_kernel(ScgArgs a, int nb) {
  __shared__ double lds[kScgBlock];
  __shared__ double lt[KC];
  const ScgLane l = scg_lane(a.rec, a.K);
  const ScgState st = a.st[l.run ? l.fit : 0];
  const bool live = l.run && st.done == 0;
  const bool zero = l.run && st.zero != 0;
  if (!__syncthreads_or(live || zero)) return;
  const double pq = scg_total(a.part, 2, 0, blockIdx.y, nb, lt);
  const bool brk = pq == 0.0;
  const double alpha = brk ? 0.0 : st.rs / pq;
  if (live && brk && blockIdx.x == 0 && l.r == 0) a.st[l.fit].brk = 1;
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  double acc[1] = {0.0};
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (i >= a.n) continue;
    const int64_t e = base + i * KC + l.c;
    if (zero) a.X[e] = 0.0;
    if (live && !brk) {
      a.X[e] = a.X[e] + alpha * a.P[e];
      const double rv = a.R[e] - alpha * scg_qv<SHIFT>(a, a.P, e);
      a.R[e] = rv;
      acc[0] += rv * rv;
    }
  }
  scg_sums<1>(acc, lds, a.part, 2, 1);
}

// beta = rs_new / rs; p = r + beta p.  Every workgroup reads st->rs here: the scalar state advances in its own launch
__global__ __launch_bounds__(kScgBlock) void scg_direction_kernel(ScgArgs a, int nb) {
  __shared__ double lt[KC];
  const ScgLane l = scg_lane(a.rec, a.K);
  const ScgState st = a.st[l.run ? l.fit : 0];
  const bool live = l.run && st.done == 0 && st.brk == 0;
  if (!__syncthreads_or(live)) return;
  const double rsn = scg_total(a.part, 2, 1, blockIdx.y, nb, lt);
  const double beta = live ? rsn / st.rs : 0.0;  // (rs > 0: a fit with rs = 0 was done at its start)
  const int64_t base = static_cast<int64_t>(blockIdx.y) * a.n * KC;
  const int64_t nrb = (a.n + kScgRows - 1) / kScgRows;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i = rb * kScgRows + l.r;
    if (live && i < a.n) {
      const int64_t e = base + i * KC + l.c;
      a.P[e] = a.R[e] + beta * a.P[e];
    }
  }
}

// ONE workgroup walks the chunks: rs <- r.r, the iteration counts, converged / capped, and the word the host polls
__global__ __launch_bounds__(kScgBlock) void scg_advance_kernel(ScgArgs a, int nb, int chunks) {
  __shared__ double lt[KC];
  __shared__ int longest;  // inner iterations of the slowest fit of this solve (sizes the host's next batch)
  const int c = threadIdx.x % KC, r = threadIdx.x / KC;
  if (threadIdx.x == 0) longest = 0;
  int all = 1;
  for (int ch = 0; ch < chunks; ++ch) {
    const int fit = ch * KC + c;
    const bool run = fit < a.K && a.rec[fit < a.K ? fit : a.K - 1].stop == 0;
    const double rsn = scg_total(a.part, 2, 1, ch, nb, lt);
    int fin = 1;
    if (run && r == 0) {
      ScgState* st = a.st + fit;
      if (st->done == 0) {
        const bool brk = st->brk != 0;
        if (!brk) st->rs = rsn;
        st->iters += 1;
        st->total += 1;
        const bool converged = sqrt(st->rs) <= a.tol * st->ynorm;
        if (converged || brk || st->iters >= a.maxit) {
          if (!converged) st->capped += 1;
          st->done = 1;
        }
      }
      fin = st->done;
      atomicMax(&longest, st->iters);
    }
    all &= __syncthreads_and(fin);  // (also the barrier in front of the next chunk's use of lt)
  }
  if (threadIdx.x == 0) {
    a.alldone[0] = all;
    a.alldone[1] = longest;
  }
}

}  // namespace

int scg_vec_workgroups(int64_t len) {
  return static_cast<int>(std::min<int64_t>(std::max<int64_t>(ceil_div(len, int64_t{kScgRows}), 1), kScgMaxWg));
}

void launch_scg_start(const ScgArgs& a, bool first, hipStream_t stream) {
  const int nb = scg_vec_workgroups(a.n);
  const unsigned chunks = static_cast<unsigned>(spmm_chunks(a.K));
  const dim3 grid(nb, chunks);
  if (first) hipLaunchKernelGGL((scg_init_kernel<true, false>), grid, dim3(kScgBlock), 0, stream, a);  // (r = y: no q)
  else if (a.shift != 0.0) hipLaunchKernelGGL((scg_init_kernel<false, true>), grid, dim3(kScgBlock), 0, stream, a);
  else hipLaunchKernelGGL((scg_init_kernel<false, false>), grid, dim3(kScgBlock), 0, stream, a);
  hipLaunchKernelGGL(scg_start_kernel, dim3(1, chunks), dim3(kScgBlock), 0, stream, a, nb);
}

void launch_scg_step(const ScgArgs& a, hipStream_t stream) {
  const int nb = scg_vec_workgroups(a.n);
  const int chunks = spmm_chunks(a.K);
  const dim3 grid(nb, static_cast<unsigned>(chunks));
  if (a.shift != 0.0) {
    hipLaunchKernelGGL(scg_dot_kernel<true>, grid, dim3(kScgBlock), 0, stream, a);
    hipLaunchKernelGGL(scg_update_kernel<true>, grid, dim3(kScgBlock), 0, stream, a, nb);
  } else {
    hipLaunchKernelGGL(scg_dot_kernel<false>, grid, dim3(kScgBlock), 0, stream, a);
    hipLaunchKernelGGL(scg_update_kernel<false>, grid, dim3(kScgBlock), 0, stream, a, nb);
  }
  hipLaunchKernelGGL(scg_direction_kernel, grid, dim3(kScgBlock), 0, stream, a, nb);
  hipLaunchKernelGGL(scg_advance_kernel, dim3(1), dim3(kScgBlock), 0, stream, a, nb, chunks);
}

// ------------------------------------------------------------------------------------------------------ the host side
int SpmmCg::build(MultiHost* host, int device, const admm_sparse_desc* D) {
  h = host;
  ADMM_HIP_TRY(hipSetDevice(device));
  h->device = device;
  ADMM_HIP_TRY(hipStreamCreate(&h->stream));
  ADMM_TRY(sparse_device_build(D, &sp, h->stream));
  m = D->rows;
  n = D->cols;
  chunks = spmm_chunks(h->K);
  const size_t kp = static_cast<size_t>(chunks) * kSpmmChunk;
  for (double** p : {&X, &R, &P, &Q, &Y}) {
    ADMM_TRY(h->mem.alloc(p, kp * n));
    ADMM_HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * kp * n, h->stream));
  }
  ADMM_TRY(h->mem.alloc(&T, kp * m));
  ADMM_HIP_TRY(hipMemsetAsync(T, 0, sizeof(double) * kp * m, h->stream));
  ADMM_TRY(h->mem.alloc(&cgpart, kp * 2 * kScgMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(cgpart, 0, sizeof(double) * kp * 2 * kScgMaxWg, h->stream));
  ADMM_TRY(alloc_words(*h, &alldone, 2));
  ADMM_TRY(alloc_words(*h, &cg, static_cast<size_t>(h->K)));
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&poll), sizeof(*poll)));
  return ADMM_OK;
}

void SpmmCg::destroy() {
  if (!h) return;
  destroy_common(*h);
  sparse_device_free(&sp);
  if (poll) (void)hipHostFree(poll);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

SpmmMask SpmmCg::mask(bool with_cg) const {
  SpmmMask mk;
  mk.flag_a = &h->rec->stop;
  mk.stride_a = kMultiRecWords;
  if (with_cg) {
    mk.flag_b = reinterpret_cast<const int32_t*>(cg) + kScgDoneWord;
    mk.stride_b = kScgStateWords;
  }
  mk.K = h->K;
  return mk;
}

int SpmmCg::upload(double* dst, const double* src, int64_t rows) {
  const size_t elems = static_cast<size_t>(chunks) * rows * kSpmmChunk;
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * elems, h->stream));
    return ADMM_OK;
  }
  std::vector<double> hb(elems);
  spmm_pack(src, rows, rows, h->K, hb.data());
  ADMM_HIP_TRY(hipMemcpyAsync(dst, hb.data(), sizeof(double) * elems, hipMemcpyHostToDevice, h->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(h->stream));  // (hb goes out of scope)
  return ADMM_OK;
}

int SpmmCg::fetch_matrix(const double* src, int64_t rows, double* dst, size_t cap, size_t* written) {
  const size_t need = static_cast<size_t>(rows) * h->K;
  if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
  std::vector<double> hb(static_cast<size_t>(chunks) * rows * kSpmmChunk);
  ADMM_HIP_TRY(hipMemcpy(hb.data(), src, sizeof(double) * hb.size(), hipMemcpyDeviceToHost));
  spmm_unpack(hb.data(), rows, h->K, dst, rows);
  if (written) *written = need;
  return ADMM_OK;
}

int SpmmCg::begin_run(double tol, int32_t maxit, ScgArgs* a, double shift) {
  ADMM_HIP_TRY(hipMemsetAsync(cg, 0, sizeof(ScgState) * h->K, h->stream));
  ADMM_TRY(upload(X, nullptr, n));  // (x0 is never read: the first x-update starts CG from 0)
  cg_batch = 8;                     // (a run never depends on the one before it)
  *a = ScgArgs{n, tol, maxit, h->K, Y, X, R, P, Q, cgpart, cg, h->rec, alldone, shift};
  return ADMM_OK;
}

int SpmmCg::solve(const ScgArgs& a, bool first) {
  const SpmmMask run = mask(false), live = mask(true);
  // T = D V, or omega_k o (D V) per fit under row weights (spmm_cg.h)
  auto forward = [&](const double* V, const SpmmMask& mk) {
    if (weighted) launch_spmm_weighted(sp.n, V, T, chunks, mk, roww, h->stream);
    else launch_spmm(sp.n, V, T, chunks, mk, h->stream);
  };
  if (!first) {  // q = D'(D x) in front of a warm start
    forward(X, run);
    launch_spmm(sp.t, T, Q, chunks, run, h->stream);
  }
  launch_scg_start(a, first, h->stream);
  for (int32_t done_it = 0; done_it < a.maxit;) {
    const int32_t k = std::min(a.maxit - done_it, static_cast<int32_t>(cg_batch));
    for (int32_t c = 0; c < k; ++c) {
      forward(P, live);
      launch_spmm(sp.t, T, Q, chunks, live, h->stream);
      launch_scg_step(a, h->stream);
    }
    done_it += k;
    ADMM_HIP_TRY(hipMemcpyAsync(poll, alldone, sizeof(*poll), hipMemcpyDeviceToHost, h->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(h->stream));
    if (poll->alldone) break;
  }
  // (a batch as long as the last solve took, as cg_solve sizes its own: one or two polls per solve)
  cg_batch = std::min(64, std::max(4, static_cast<int>(poll->longest) + 2));
  return ADMM_OK;
}

int SpmmCg::fetch_counters(std::vector<ScgState>* out) const {
  out->resize(static_cast<size_t>(h->K));
  ADMM_HIP_TRY(hipMemcpy(out->data(), cg, sizeof(ScgState) * h->K, hipMemcpyDeviceToHost));
  return ADMM_OK;
}

// ------------------------------------------------------------------------------------- the stand-alone operator (q45)
namespace {

// what a frozen fit's column of buffer `which` (0 X, 1 R, 2 P) holds before the solve: finite, nonzero, and different
// for every (buffer, fit, row)
double frozen_pattern(int which, int32_t k, int64_t i) {
  return -(1.0 + which) * 1024.0 - static_cast<double>(k) - static_cast<double>(i % 1021) / 1024.0;
}

struct ScgOpIn {
  const admm_sparse_desc* D;
  int32_t K;
  const double *Y, *X0;
  double shift, tol;
  int32_t maxit, batch;
  const int32_t* stop;
};

// one solve of the production path on a host of its own, then the operator's own checks of what the caller cannot see
int scg_op_run(MultiHost& h, SpmmCg& cg, const ScgOpIn& in, double* X, double* R, int64_t* state, int32_t* next_batch) {
  const int32_t K = in.K;
  h.K = K;
  ADMM_TRY(cg.build(&h, 0, in.D));
  ADMM_TRY(alloc_common(h));
  ADMM_TRY(begin_run(h));
  ScgArgs a{};
  ADMM_TRY(cg.begin_run(in.tol, in.maxit, &a, in.shift));
  if (in.batch > 0) cg.cg_batch = in.batch;
  const int64_t n = cg.n;
  ADMM_TRY(cg.upload(cg.Y, in.Y, n));
  if (in.X0) ADMM_TRY(cg.upload(cg.X, in.X0, n));

  const size_t elems = static_cast<size_t>(cg.chunks) * n * kSpmmChunk;
  auto at = [&](int32_t k, int64_t i) {
    return static_cast<size_t>(k / kSpmmChunk) * n * kSpmmChunk + static_cast<size_t>(i) * kSpmmChunk + k % kSpmmChunk;
  };
  double* const bufs[4] = {cg.X, cg.R, cg.P, cg.Q};
  static const char* const names[4] = {"X", "R", "P", "Q"};
  std::vector<double> before[3];
  bool frozen = false;
  for (int32_t k = 0; in.stop && k < K; ++k) frozen = frozen || in.stop[k] != 0;
  if (frozen) {  // the flags into the records, the pattern into the frozen fits' columns of X, R and P
    std::vector<MultiRec> rec(static_cast<size_t>(K), MultiRec{0, 0, 0, 0});
    for (int32_t k = 0; k < K; ++k) rec[k].stop = in.stop[k] != 0 ? 1 : 0;
    ADMM_HIP_TRY(hipMemcpyAsync(h.rec, rec.data(), sizeof(MultiRec) * K, hipMemcpyHostToDevice, h.stream));
    ADMM_HIP_TRY(hipStreamSynchronize(h.stream));  // (X0 is up, rec goes out of scope)
    for (int b = 0; b < 3; ++b) {
      before[b].resize(elems);
      ADMM_HIP_TRY(hipMemcpy(before[b].data(), bufs[b], sizeof(double) * elems, hipMemcpyDeviceToHost));
      for (int32_t k = 0; k < K; ++k)
        if (in.stop[k] != 0)
          for (int64_t i = 0; i < n; ++i) before[b][at(k, i)] = frozen_pattern(b, k, i);
      ADMM_HIP_TRY(hipMemcpy(bufs[b], before[b].data(), sizeof(double) * elems, hipMemcpyHostToDevice));
    }
  }

  ADMM_TRY(cg.solve(a, in.X0 == nullptr));
  ADMM_HIP_TRY(hipStreamSynchronize(h.stream));
  ADMM_HIP_TRY(hipGetLastError());

  std::vector<ScgState> st;
  ADMM_TRY(cg.fetch_counters(&st));
  std::vector<double> after(elems);
  const int32_t kpad = cg.chunks * kSpmmChunk;
  for (int b = 0; b < 4; ++b) {
    ADMM_HIP_TRY(hipMemcpy(after.data(), bufs[b], sizeof(double) * elems, hipMemcpyDeviceToHost));
    for (int32_t k = K; k < kpad; ++k)  // the padding columns of the last chunk: exactly +0.0, as build left them
      for (int64_t i = 0; i < n; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &after[at(k, i)], sizeof(bits));
        if (bits != 0)
          return fail(ADMM_E_NUMERIC, std::string("spmm_cg: padding column ") + std::to_string(k) + " of " + names[b] +
                                          " is no longer 0.0 at row " + std::to_string(i));
      }
    for (int32_t k = 0; frozen && b < 3 && k < K; ++k) {
      if (in.stop[k] == 0) continue;
      for (int64_t i = 0; i < n; ++i)
        if (std::memcmp(&after[at(k, i)], &before[b][at(k, i)], sizeof(double)) != 0)
          return fail(ADMM_E_NUMERIC, std::string("spmm_cg: the frozen fit ") + std::to_string(k) + " changed in " +
                                          names[b] + " at row " + std::to_string(i));
    }
  }
  for (int32_t k = 0; frozen && k < K; ++k) {
    static const ScgState zero{};
    if (in.stop[k] != 0 && std::memcmp(&st[k], &zero, sizeof(ScgState)) != 0)
      return fail(ADMM_E_NUMERIC, "spmm_cg: the CG state of the frozen fit " + std::to_string(k) + " moved");
  }

  ADMM_TRY(cg.fetch_matrix(cg.X, n, X, static_cast<size_t>(n) * K, nullptr));
  if (R) ADMM_TRY(cg.fetch_matrix(cg.R, n, R, static_cast<size_t>(n) * K, nullptr));
  for (int32_t k = 0; k < K; ++k) {
    int64_t* s = state + static_cast<size_t>(6) * k;
    s[0] = st[k].iters;
    s[1] = st[k].total;
    s[2] = st[k].capped;
    s[3] = st[k].done;
    s[4] = st[k].brk;
    s[5] = st[k].zero;
  }
  if (next_batch) *next_batch = cg.cg_batch;
  return ADMM_OK;
}

}  // namespace

}  // namespace admm

using namespace admm;

extern "C" int admm_op_spmm_cg(const admm_sparse_desc* D, int32_t K, const double* Y, const double* X0, double shift,
                               double tol, int32_t maxit, int32_t batch, const int32_t* stop, double* X, double* R,
                               int64_t* state, int32_t* next_batch) {
  if (!Y || !X || !state) return fail(ADMM_E_INVALID, "spmm_cg: Y, X or state is NULL");
  if (K < 1) return fail(ADMM_E_INVALID, "spmm_cg: K must be at least 1");
  if (!finite_pos(tol)) return fail(ADMM_E_INVALID, "spmm_cg: tol must be positive and finite");
  if (maxit < 1) return fail(ADMM_E_INVALID, "spmm_cg: maxit must be at least 1");
  if (!finite_nonneg(shift)) return fail(ADMM_E_INVALID, "spmm_cg: shift is negative or not finite");
  ADMM_TRY(check_sparse_D("spmm_cg", D));
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(ADMM_E_DEVICE, "no HIP device visible: the ADMM engine has no CPU fallback");
  MultiHost h;
  SpmmCg cg;
  const ScgOpIn in{D, K, Y, X0, shift, tol, maxit, batch, stop};
  const int rc = scg_op_run(h, cg, in, X, R, state, next_batch);
  const std::string msg = rc != ADMM_OK ? std::string(admm_last_error()) : std::string();
  cg.destroy();  // (the whole teardown of h; nothing to do before build)
  return rc != ADMM_OK ? fail(rc, msg) : ADMM_OK;
}
