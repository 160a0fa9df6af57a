// reg_multi.hip -- quantile / LAD / Huber regression, K fits at once: a set of quantiles of one design
// matrix, a Huber fit at several thresholds, one loss against several response columns.  The x-update of the A = D
// iteration is (D'D)^-1 D'(s + z - u) (getProxOps.m:1511-1515) and contains neither the loss nor its parameters; those
// enter the element-wise z-prox (loss_device.h: loss_prox_elem) and the objective (lad.m:148 / huberfit.m:180) alone.
// K fits are therefore K independent plain-ADMM runs (admm.m:496-743 with A = D, B = -1, c = s_k, stopcond = 'standard',
// nodualerror = 1) that share D, the map (D'D)^-1 and every byte an iteration reads from HBM.  Per iteration:
//   ovr_xsolve_kernel     x_k = M g_k for every running fit (svm_ovr.hip's kernel as it is: M symmetric n x n, n <= 448)
//   regm_pass_kernel      ONE read of D for a chunk of kRegmChunk fits, in the register / LDS layout of ovr_pass_kernel:
//                         the 64-row block in registers -- lane = row, wave w owns the columns j = w (mod 8) --, then per
//                         fit (D x_k)_r, the family's z-prox in a register (loss_form_z), the fused element update
//                         (prox_apply with PROX_GIVEN: the code every loop shares), and the block's contribution
//                         D_r' t_r to the fit's next right-hand side g_k = D'((s_k + z_k) - u_k)
//   regm_gsum_fin_kernel  sums the workgroups' partial rows of g_k in the fixed order of multi_gsum_tile; one extra
//                         workgroup per fit turns the block partials into pnorm, perr, the objective and the stop
//                         decision (admm.m:612-658, 706-713)
// The dual residual is not evaluated (two more transposed products per fit): a fit stops on pnorm < perr.
// A fit whose stop flag is set is FROZEN: every kernel skips it, so its X, Z, U columns and histories are those of an
// independent run with that many steps.  Every sum runs in a fixed order that does not depend on which chunk or slot a
// fit occupies: runs are bitwise reproducible, and a fit gets the same numbers wherever it lands.
// All loads of D are unconditional on clamped addresses (x is zero beyond n; rows beyond m carry t = 0).  No atomics.
#include <cmath>
#include <vector>

#include "loss_device.h"
#include "multi_host.h"
#include "reg_multi.h"
#include "wave_reduce.h"

namespace admm {

constexpr int kRmRows = 64, kRmWaves = 8, kRmCols = 56, kRmMaxN = kRmWaves * kRmCols;  // 448, as ovr_pass_kernel
static_assert(kRmMaxN == ADMM_REG_MULTI_MAX_N, "the header states the limit");
static_assert(kRmMaxN == ADMM_SVM_OVR_MAX_N, "ovr_xsolve_kernel's staging buffer holds this many entries");
constexpr int kRmSlotsPerWave = (kRegmChunk + kRmWaves - 1) / kRmWaves;  // fits whose element update one wave runs

// the ProxArgs of one fit: plain ADMM, B = -1, c = s_k, z given in a register, no histories (the compiler folds the
// constant fields)
__device__ __forceinline__ ProxArgs regm_prox_args(const RegmPassArgs& a, int fit) {
  ProxArgs pa{};
  pa.len = a.m;
  pa.z = a.Z + static_cast<int64_t>(fit) * a.ldz;
  pa.u = a.U + static_cast<int64_t>(fit) * a.ldz;
  pa.c = a.S + (a.ns == 1 ? int64_t{0} : static_cast<int64_t>(fit) * a.ldz);
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = PROX_GIVEN;
  pa.objx = OBJX_NONE;
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;
  pa.rhs_kind = RHS_NONE;
  return pa;
}

// INIT: only the partial rows of D'((s + z0) - u0), before the first iteration.
template <int KC, bool INIT>
__global__ __launch_bounds__(kRmWaves* kWave) void regm_pass_kernel(RegmPassArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[kRmMaxN * KC];  // [column][fit]: one column's KC values contiguous
  __shared__ double gacc[KC * kRmMaxN];
  __shared__ double axr[kRmWaves * KC * kRmRows];
  __shared__ double tsh[KC * kRmRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n = a.n, m = a.m;
  uint32_t actv = 0;  // bit c: fit c0 + c exists and is still running
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int fit = a.c0 + c;
    const int32_t st = a.rec[fit < a.K ? fit : a.K - 1].stop;
    if (fit < a.K && st == 0) actv |= 1u << c;
  }
  const uint32_t act = __builtin_amdgcn_readfirstlane(actv);
  if (act == 0) return;  // every fit of the chunk has stopped: a no-op
  for (int idx = tid; idx < kRmMaxN * KC; idx += kRmWaves * kWave) {
    const int j = idx / KC, c = idx - j * KC;
    const int fit = a.c0 + c;
    double xv = 0.0;
    if (!INIT && j < n && fit < a.K) xv = a.X[static_cast<int64_t>(fit) * a.ldx + j];
    xs[idx] = xv;
    gacc[idx] = 0.0;
  }
  __syncthreads();
  // the fits whose element update this wave runs: w, w + 8, ...
  double acc[kRmSlotsPerWave][S_COUNT];
  ProxArgs pas[kRmSlotsPerWave];
  LossArgs ls[kRmSlotsPerWave];
#pragma unroll
  for (int s = 0; s < kRmSlotsPerWave; ++s) {
#pragma unroll
    for (int q = 0; q < S_COUNT; ++q) acc[s][q] = 0.0;
    const int c = w + kRmWaves * s;
    const int fit = (a.c0 + c < a.K) ? a.c0 + c : a.K - 1;
    pas[s] = regm_prox_args(a, fit);
    const double* __restrict__ pp = a.par + 4 * fit;
    ls[s] = LossArgs{nullptr, pp[0], pp[1], pp[2], pp[3], a.rho, a.kind[fit], a.objevals};  // (the weight: wv below)
  }
  const int64_t nblocks = (m + kRmRows - 1) / kRmRows;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r = blk * kRmRows + lane;
    const int64_t rc = r < m ? r : m - 1;
    const double* __restrict__ drow = a.D + rc;
    double d[kRmCols];
#pragma unroll
    for (int k = 0; k < kRmCols; ++k) {  // clamped columns: the loads stay unconditional, x is zero beyond n
      const int64_t j = w + kRmWaves * k;
      d[k] = drow[(j < n ? j : n - 1) * a.ldD];
    }
    double zp[kRmSlotsPerWave], uo[kRmSlotsPerWave], sv[kRmSlotsPerWave];
    const double s1 = a.S[rc];  // the shared response: once per block, not once per fit
#pragma unroll
    for (int s = 0; s < kRmSlotsPerWave; ++s) {  // in flight with the block
      zp[s] = pas[s].z[rc];
      uo[s] = pas[s].u[rc];
      const double* ps = (a.ns == 1) ? pas[s].z : pas[s].c;  // (redirected to z: the load stays unconditional)
      const double sl = ps[rc];
      sv[s] = (a.ns == 1) ? s1 : sl;
    }
    // one m-vector for all fits: redirected to z without weights, so the load stays unconditional
    const double* pw = a.W ? a.W : pas[0].z;
    const double wl = pw[rc];
    const double wv = a.W ? wl : 1.0;
    if (!INIT) {
      double p[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) p[c] = 0.0;
#pragma unroll
      for (int k = 0; k < kRmCols; ++k) {
        const double* __restrict__ xk = xs + (w + kRmWaves * k) * KC;  // same address in every lane: LDS broadcast
#pragma unroll
        for (int c = 0; c < KC; ++c) p[c] = __builtin_fma(d[k], xk[c], p[c]);
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) axr[(w * KC + c) * kRmRows + lane] = p[c];
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < kRmSlotsPerWave; ++s) {
      const int c = w + kRmWaves * s;
      if (c < KC && ((act >> c) & 1u)) {  // wave-uniform
        double t = 0.0;
        if (INIT) {
          if (r < m) t = (sv[s] + zp[s]) - uo[s];  // (c + z0) - u0, as prox_apply forms it for RHS_T1
        } else {
          double ax = axr[c * kRmRows + lane];
#pragma unroll
          for (int q = 1; q < kRmWaves; ++q) ax += axr[(q * KC + c) * kRmRows + lane];
          ProxIn in{};
          in.zp = zp[s];
          in.u_old = uo[s];
          in.uhat_i = uo[s];
          in.c_i = sv[s];
          if (r < m) {
            loss_form_z(pas[s], ls[s], wv, ax, in, acc[s]);  // z = prox of the fit's loss at (ax + u) - s
            prox_apply<false>(pas[s], r, ax, 0, 0.0, in, acc[s], &t);
          }
        }
        tsh[c * kRmRows + lane] = t;  // rows beyond m contribute nothing
      }
    }
    __syncthreads();
    static_assert(kRmCols % kSyPanel == 0, "column sums are taken four at a time");
#pragma unroll 1
    for (int c = 0; c < KC; ++c) {
      if (!((act >> c) & 1u)) continue;  // wave-uniform
      const double t = tsh[c * kRmRows + lane];
#pragma unroll
      for (int k = 0; k < kRmCols; k += kSyPanel) {  // four column sums per permlane / DPP reduce-scatter (wave_reduce.h)
        double q[kSyPanel];
#pragma unroll
        for (int i = 0; i < kSyPanel; ++i) q[i] = d[k + i] * t;
        const double sum = reduce_scatter4(q);  // lanes 16i .. 16i+15 hold the sum of column k + i
        const int j = w + kRmWaves * (k + (lane >> 4));
        if ((lane & 15) == 0 && j < n) gacc[c * kRmMaxN + j] += sum;  // (each wave owns its columns)
      }
    }
    // (axr and tsh are rewritten only behind the next block's first barrier: every wave has left this block's reads by then)
    if (INIT) __syncthreads();  // (no such barrier without the D*x phase)
  }
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < KC; ++c) {
    if (!((act >> c) & 1u)) continue;
    double* __restrict__ gout = a.gpart + (static_cast<int64_t>(blockIdx.x) * a.K + (a.c0 + c)) * a.ldx;
    for (int j = tid; j < n; j += kRmWaves * kWave) gout[j] = gacc[c * kRmMaxN + j];
  }
  if (INIT) return;
  constexpr int slot_of[RM_COUNT] = {S_R2, S_AX2, S_Z2, S_OBJZ};
#pragma unroll
  for (int s = 0; s < kRmSlotsPerWave; ++s) {
    const int c = w + kRmWaves * s;
    if (c < KC && ((act >> c) & 1u)) {
#pragma unroll
      for (int q = 0; q < RM_COUNT; ++q) {
        const double v = wave_sum(acc[s][slot_of[q]]);
        if (lane == 0) a.part[(static_cast<int64_t>(a.c0 + c) * RM_COUNT + q) * kMultiMaxWg + blockIdx.x] = v;
      }
    }
  }
}

// blockIdx.y = fit.  blockIdx.x < tiles: g_k[64 columns] = sum over the workgroups' partial rows (multi_gsum_tile).
// The extra workgroup (a.fin): the finalize logic of the fit's iteration -- admm.m:612-658, 706-713 as
// oracle/admm_ref.py restates it, for plain ADMM with nodualerror = 1 and stopcond = 'standard'.
__global__ __launch_bounds__(kBlock) void regm_gsum_fin_kernel(RegmFinArgs a) {
  const int fit = blockIdx.y;
  MultiRec* rec = a.rec + fit;
  const int32_t stopped = rec->stop;
  const int32_t it = rec->iter;
  if (stopped) return;
  __shared__ double sq[4][kMultiTile];
  __shared__ double S[8];
  const int tid = threadIdx.x;
  const int tiles = static_cast<int>((a.n + kMultiTile - 1) / kMultiTile);
  if (static_cast<int>(blockIdx.x) < tiles) {
    multi_gsum_tile(a.gpart, a.gsum, fit, a.ldx, a.n, a.K, a.nwg, sq);
    return;
  }
  // ---- finalize of fit `fit`
  multi_slot_totals_unrolled(a.part, fit, RM_COUNT, a.nwg, S);
  __syncthreads();
  if (tid != 0) return;
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(fit) * a.hist_ld + it;
  if (a.objevals) a.objv[h] = S[RM_OBJ];  // lad.m:148 / huberfit.m:180 with the family inside: sum_i w_i*phi(z_i)
  const double pn = sqrt(S[RM_R2]);  // admm.m:621
  const double pe = sqrt(static_cast<double>(a.m)) * a.abstol +
                    a.reltol * fmax(fmax(sqrt(S[RM_AX2]), sqrt(S[RM_Z2])), a.snorm[fit]);  // admm.m:644-650, c = s_k
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  const bool stop = !a.domaxiters && pn < pe;  // admm.m:710-713, nodualerror
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

// one workgroup per fit: the squares of the fit's response summed per thread in a strided order, per wave by wave_sum,
// the four wave sums in wave order
__global__ __launch_bounds__(kBlock) void regm_snorm_kernel(const double* __restrict__ S, int64_t ldz, int64_t m,
                                                            int32_t ns, double* __restrict__ snorm) {
  __shared__ double ws[4];
  const int fit = blockIdx.x;
  const double* __restrict__ s = S + (ns == 1 ? int64_t{0} : static_cast<int64_t>(fit) * ldz);
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kBlock) v += s[i] * s[i];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) snorm[fit] = sqrt(((ws[0] + ws[1]) + ws[2]) + ws[3]);
}

void launch_regm_pass(const RegmPassArgs& a, bool init, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(ovr_pass_workgroups(a.m))), block(kRmWaves * kWave);
  if (init) hipLaunchKernelGGL((regm_pass_kernel<kRegmChunk, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((regm_pass_kernel<kRegmChunk, false>), grid, block, 0, stream, a);
}

void launch_regm_gsum_fin(const RegmFinArgs& a, hipStream_t stream) {
  const unsigned tiles = static_cast<unsigned>(ceil_div(a.n, int64_t{kMultiTile}));
  hipLaunchKernelGGL(regm_gsum_fin_kernel, dim3(tiles + (a.fin ? 1u : 0u), static_cast<unsigned>(a.K)), dim3(kBlock), 0,
                     stream, a);
}

void launch_regm_snorm(const double* S, int64_t ldz, int64_t m, int32_t K, int32_t ns, double* snorm, hipStream_t stream) {
  hipLaunchKernelGGL(regm_snorm_kernel, dim3(static_cast<unsigned>(K)), dim3(kBlock), 0, stream, S, ldz, m, ns, snorm);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_reg_multi : DenseMulti {  // eng: an ordinary ADMM_PROB_LAD engine
  int32_t ns = 1;
  double *S = nullptr, *par = nullptr, *snorm = nullptr;
  int32_t* kind = nullptr;
  double* W = nullptr;  // m shared weights on the device, or null: every weight is 1
  double *pnorm = nullptr, *perr = nullptr, *objv = nullptr;  // histories
  admm_reg_multi_options last{};
  int64_t launches[4] = {0, 0, 0, 0};  // of the last run: iterations, x-solve, pass, sum / finalize
};

namespace {

const char* kPerFit = ": run one ADMM_PROB_LAD / ADMM_PROB_HUBERFIT engine (admm_engine_create) per fit instead";

int regm_setup(admm_reg_multi* o, const admm_reg_multi_desc* desc, const std::vector<int32_t>& kh,
               const std::vector<double>& ph) {
  const int64_t m = desc->m, n = desc->n;
  const int32_t K = desc->K;
  admm_problem_desc d;
  admm_problem_desc_default(&d);
  d.problem = ADMM_PROB_LAD;
  d.m = m;
  d.n = n;
  d.D = desc->D;
  d.ldD = desc->ldD;
  d.s = desc->S;  // (the engine wants one response; it never runs)
  d.mem = desc->mem;
  d.device = desc->device;
  ADMM_TRY(admm_engine_create(&d, &o->eng));  // ADMM_E_NUMERIC: D'D numerically singular (setup_lad_huber_svm's rule)
  o->ns = desc->ns;
  ADMM_TRY(dense_setup(*o, m, n, K, RM_COUNT, kPerFit));
  ADMM_TRY(o->mem.alloc(&o->S, static_cast<size_t>(o->ldz) * o->ns));
  ADMM_HIP_TRY(hipMemsetAsync(o->S, 0, sizeof(double) * o->ldz * o->ns, o->stream));
  ADMM_TRY(upload_cols(*o, o->S, o->ldz, desc->S, m, o->ns, desc->mem));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(4) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 4 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(o->mem.alloc(&o->snorm, static_cast<size_t>(K)));
  ADMM_TRY(alloc_words(*o, &o->kind, static_cast<size_t>(K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->kind, kh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  launch_regm_snorm(o->S, o->ldz, m, K, o->ns, o->snorm, o->stream);  // perr needs max(||Dx||, ||z||, ||s_k||): once
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (kh, ph, and the caller's buffers, were read)
  ADMM_HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // namespace

extern "C" {

void admm_reg_multi_desc_default(admm_reg_multi_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_reg_multi_desc);
  d->K = 1;
  d->ns = 1;
}

void admm_reg_multi_options_default(admm_reg_multi_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_reg_multi_options);
  o->maxiters = 1000;  // admm.m:66
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->relax = 1.0;      // admm.m:60
}

int admm_reg_multi_chunk(void) { return kRegmChunk; }

int admm_reg_multi_create(const admm_reg_multi_desc* desc, admm_reg_multi** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_reg_multi_desc)))
    return fail(ADMM_E_INVALID, "admm_reg_multi_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the multi-fit regression needs at least one fit (K >= 1)");
  if (!desc->D || desc->m <= 0 || desc->n <= 0) return fail(ADMM_E_INVALID, "the multi-fit regression needs D (m x n)");
  if (!desc->S) return fail(ADMM_E_INVALID, "the multi-fit regression needs the responses S (m x ns)");
  ADMM_TRY(check_response_columns(desc->ns, desc->K));
  std::vector<int32_t> kh;
  std::vector<double> ph;
  ADMM_TRY(check_reg_fits(desc->K, desc->kind, desc->a, desc->b, desc->epsilon, desc->delta, &kh, &ph));
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, std::string("the multi-fit regression is not row-sharded") + kPerFit);
  if (desc->n > kRmMaxN)
    return fail(ADMM_E_UNSUPPORTED, "the multi-fit pass holds a 64-row block of D in registers: n <= " +
                                        std::to_string(kRmMaxN) + kPerFit);
  if (desc->m < desc->n)
    return fail(ADMM_E_UNSUPPORTED, "D must have full column rank (m >= n) for chol(D'*D) (lad.m:134)");
  return create_object(out, admm_reg_multi_destroy, [&](admm_reg_multi* o) { return regm_setup(o, desc, kh, ph); });
}

int admm_reg_multi_run(admm_reg_multi* o, const admm_reg_multi_options* opts, admm_reg_multi_summary* summaries,
                       double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_reg_multi_options)))
    return fail(ADMM_E_INVALID, "admm_reg_multi_options.struct_size mismatch (ABI version skew)");
  admm_reg_multi_options op = *opts;
  ADMM_TRY(check_run_options("multi-fit", kPerFit, &op));
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->objv}, N));
  ADMM_TRY(dense_start(*o, op.x0, op.z0, op.u0));

  RegmPassArgs pa{};
  pa.D = o->eng->D;
  pa.ldD = o->eng->ldD;
  pa.m = o->m;
  pa.n = o->n;
  pa.X = o->X;
  pa.ldx = o->ldx;
  pa.Z = o->Z;
  pa.U = o->U;
  pa.S = o->S;
  pa.ldz = o->ldz;
  pa.W = o->W;
  pa.par = o->par;
  pa.kind = o->kind;
  pa.gpart = o->gpart;
  pa.part = o->part;
  pa.rec = o->rec;
  pa.K = K;
  pa.ns = o->ns;
  pa.objevals = op.objevals;
  pa.rho = op.rho;
  RegmFinArgs fa{};
  fa.gpart = o->gpart;
  fa.gsum = o->gsum;
  fa.part = o->part;
  fa.snorm = o->snorm;
  fa.ldx = o->ldx;
  fa.n = o->n;
  fa.m = o->m;
  fa.K = K;
  fa.nwg = o->nwg;
  fa.rec = o->rec;
  fa.pnorm = o->pnorm;
  fa.perr = o->perr;
  fa.objv = o->objv;
  fa.hist_ld = N;
  fa.abstol = op.abstol;
  fa.reltol = op.reltol;
  fa.domaxiters = op.domaxiters;
  fa.objevals = op.objevals;
  fa.maxiters = N;
  const int32_t chunks = (K + kRegmChunk - 1) / kRegmChunk;
  auto pass = [&](bool init) {
    for (int32_t ch = 0; ch < chunks; ++ch) {
      pa.c0 = ch * kRegmChunk;
      launch_regm_pass(pa, init, o->stream);
    }
  };
  int64_t* cnt = o->launches;
  cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;

  ADMM_TRY(begin_timing(*o));
  pass(true);  // g = D'((s + z0) - u0)
  fa.fin = 0;
  launch_regm_gsum_fin(fa, o->stream);
  fa.fin = 1;
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    cnt[1] += dense_xupdate(*o);
    pass(false);
    launch_regm_gsum_fin(fa, o->stream);
    cnt[0] += 1;
    cnt[2] += chunks;
    cnt[3] += 1;
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the multi-fit loop ended with fits still running", N, op.objevals != 0, o->objv, runtime_s,
                      summaries));
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_reg_multi_set_weights(admm_reg_multi* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  return set_shared_weights(*o, o->m, weights, &o->W);
}

int admm_reg_multi_launches(admm_reg_multi* o, int64_t counts[5]) {
  if (!o || !counts) return fail(ADMM_E_INVALID, "object/counts is NULL");
  if (!o->has_run) return fail(ADMM_E_INVALID, "launch counts before the first run");
  for (int i = 0; i < 4; ++i) counts[i] = o->launches[i];
  counts[4] = o->M ? 1 : 0;
  return ADMM_OK;
}

int admm_reg_multi_fetch(admm_reg_multi* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_REGM_F_XOPT: return fetch_cols(*o, o->X, o->ldx, o->n, dst, cap, written);
    case ADMM_REGM_F_ZOPT: return fetch_cols(*o, o->Z, o->ldz, o->m, dst, cap, written);
    case ADMM_REGM_F_UOPT: return fetch_cols(*o, o->U, o->ldz, o->m, dst, cap, written);
    case ADMM_REGM_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_REGM_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_REGM_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the multi-fit regression");
  }
}

void admm_reg_multi_destroy(admm_reg_multi* o) {
  if (!o) return;
  dense_destroy(*o);
  delete o;
}

}  // extern "C"
