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
//   regm_gsum_fin_kernel  sums the workgroups' partial rows of g_k in the fixed order of ovr_gsum_fin_kernel; one extra
//                         workgroup per fit turns the block partials into pnorm, perr, the objective and the stop
//                         decision (admm.m:612-658, 706-713)
// The dual residual is not evaluated (two more transposed products per fit): a fit stops on pnorm < perr.
// A fit whose stop flag is set is FROZEN: every kernel skips it, so its X, Z, U columns and histories are those of an
// independent run with that many steps.  Every sum runs in a fixed order that does not depend on which chunk or slot a
// fit occupies: runs are bitwise reproducible, and a fit gets the same numbers wherever it lands.
// All loads of D are unconditional on clamped addresses (x is zero beyond n; rows beyond m carry t = 0).  No atomics.
#include <cmath>
#include <vector>

#include "engine_internal.h"
#include "loss_device.h"
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
        if (lane == 0) a.part[(static_cast<int64_t>(a.c0 + c) * RM_COUNT + q) * kOvrMaxWg + blockIdx.x] = v;
      }
    }
  }
}

// blockIdx.y = fit.  blockIdx.x < tiles: g_k[64 columns] = sum over the workgroups' partial rows, in the order of
// ovr_gsum_fin_kernel -- wave q takes rows q, q + 4, ... sixteen loads at a time, the four wave sums added in wave
// order.  The extra workgroup (a.fin): the finalize logic of the fit's iteration -- admm.m:612-658, 706-713 as
// oracle/admm_ref.py restates it, for plain ADMM with nodualerror = 1 and stopcond = 'standard'.
__global__ __launch_bounds__(kBlock) void regm_gsum_fin_kernel(RegmFinArgs a) {
  const int fit = blockIdx.y;
  OvrRec* rec = a.rec + fit;
  const int32_t stopped = rec->stop;
  const int32_t it = rec->iter;
  if (stopped) return;
  __shared__ double sq[4][kOvrTile];
  __shared__ double S[8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles = static_cast<int>((a.n + kOvrTile - 1) / kOvrTile);
  if (static_cast<int>(blockIdx.x) < tiles) {
    const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kOvrTile;
    const int64_t j = (j0 + lane < a.n) ? j0 + lane : a.n - 1;
    const double* __restrict__ G = a.gpart + static_cast<int64_t>(fit) * a.ldx + j;
    const int64_t rowstride = static_cast<int64_t>(a.K) * a.ldx;
    double s = 0.0;
    for (int32_t b0 = wid; b0 < a.nwg; b0 += 64) {
      double v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int32_t b = (b0 + 4 * k < a.nwg) ? b0 + 4 * k : a.nwg - 1;
        v[k] = G[static_cast<int64_t>(b) * rowstride];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) s += (b0 + 4 * k < a.nwg) ? v[k] : 0.0;
    }
    sq[wid][lane] = s;
    __syncthreads();
    if (wid == 0 && j0 + lane < a.n)
      a.gsum[static_cast<int64_t>(fit) * a.ldx + j0 + lane] = ((sq[0][lane] + sq[1][lane]) + sq[2][lane]) + sq[3][lane];
    return;
  }
  // ---- finalize of fit `fit`: 32 lanes per slot stride over the block partials, then a fixed shuffle tree
  {
    const int slot = tid >> 5, sub = tid & 31;
    double v = 0.0;
    if (slot < RM_COUNT) {
      const double* __restrict__ ps = a.part + (static_cast<int64_t>(fit) * RM_COUNT + slot) * kOvrMaxWg;
      double wv[kOvrMaxWg / 32];
#pragma unroll
      for (int k = 0; k < kOvrMaxWg / 32; ++k) {
        const int b = sub + 32 * k;
        wv[k] = ps[b < a.nwg ? b : a.nwg - 1];
      }
#pragma unroll
      for (int k = 0; k < kOvrMaxWg / 32; ++k)
        if (sub + 32 * k < a.nwg) v += wv[k];
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (sub == 0 && slot < 8) S[slot] = v;
  }
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
  rec->iter = i1;
  rec->steps = i1;
  if (stop) rec->early = 1;
  if (stop || i1 >= a.maxiters) rec->stop = 1;
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
  const unsigned tiles = static_cast<unsigned>(ceil_div(a.n, int64_t{kOvrTile}));
  hipLaunchKernelGGL(regm_gsum_fin_kernel, dim3(tiles + (a.fin ? 1u : 0u), static_cast<unsigned>(a.K)), dim3(kBlock), 0,
                     stream, a);
}

void launch_regm_snorm(const double* S, int64_t ldz, int64_t m, int32_t K, int32_t ns, double* snorm, hipStream_t stream) {
  hipLaunchKernelGGL(regm_snorm_kernel, dim3(static_cast<unsigned>(K)), dim3(kBlock), 0, stream, S, ldz, m, ns, snorm);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_reg_multi {
  admm_engine* eng = nullptr;  // an ordinary ADMM_PROB_LAD engine: owns D and the factor of D'D; never run
  hipStream_t stream = nullptr;  // = eng->stream
  DevMem mem;
  int device = 0;
  int64_t m = 0, n = 0, ldx = 0, ldz = 0;
  int32_t K = 0, ns = 1, nwg = 0;
  const double* M = nullptr;  // the explicit n x n map (D'D)^-1 of the engine; null: triangular solves
  int64_t ldM = 0;
  double *X = nullptr, *Z = nullptr, *U = nullptr, *S = nullptr, *gpart = nullptr, *gsum = nullptr, *part = nullptr,
         *xtmp = nullptr, *par = nullptr, *snorm = nullptr;
  int32_t* kind = nullptr;
  double* W = nullptr;  // m shared weights on the device, or null: every weight is 1
  OvrRec* rec = nullptr;
  OvrRec* rec_host = nullptr;  // pinned
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // histories of the last run: [K][hist_ld]
  double *pnorm = nullptr, *perr = nullptr, *objv = nullptr;
  int32_t hist_ld = 0;
  bool has_run = false;
  admm_reg_multi_options last{};
  std::vector<int32_t> steps;
  int64_t launches[4] = {0, 0, 0, 0};  // of the last run: iterations, x-solve, pass, sum / finalize
};

namespace {

const char* kPerFit = ": run one ADMM_PROB_LAD / ADMM_PROB_HUBERFIT engine (admm_engine_create) per fit instead";

int regm_upload_cols(admm_reg_multi* o, double* dst, int64_t ld, const double* src, int64_t rows, int32_t cols, int kind) {
  if (!src) {
    ADMM_HIP_TRY(hipMemsetAsync(dst, 0, sizeof(double) * ld * cols, o->stream));
    return ADMM_OK;
  }
  ADMM_HIP_TRY(hipMemcpy2DAsync(dst, ld * sizeof(double), src, rows * sizeof(double), rows * sizeof(double), cols,
                                kind == ADMM_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, o->stream));
  return ADMM_OK;
}

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
  admm_engine* e = o->eng;
  o->stream = e->stream;
  o->device = e->device;
  o->m = m;
  o->n = n;
  o->K = K;
  o->ns = desc->ns;
  o->ldx = round_up(n, 2);
  o->ldz = round_up(m, 2);
  o->nwg = ovr_pass_workgroups(m);
  if (e->xfac.mode == ADMM_XSOLVE_INVERSE && e->xfac.Minv && !e->xfac.planSy.packed) {
    o->M = e->xfac.Minv;  // (D'D)^-1: full symmetric storage below kSymvHalfMin
    o->ldM = e->xfac.ldM;
  } else if (e->xfac.mode == ADMM_XSOLVE_TRSV && e->xfac.F) {
    // create's accuracy probe kept the triangular solves: they run per fit (K small launches), nothing is forced
    ADMM_TRY(o->mem.alloc(&o->xtmp, static_cast<size_t>(o->ldx) * K));
    ADMM_HIP_TRY(hipMemsetAsync(o->xtmp, 0, sizeof(double) * o->ldx * K, o->stream));
  } else {
    return fail(ADMM_E_UNSUPPORTED, std::string("the engine built no n x n form of the x-update for this D") + kPerFit);
  }
  ADMM_TRY(o->mem.alloc(&o->X, static_cast<size_t>(o->ldx) * K));
  ADMM_TRY(o->mem.alloc(&o->gsum, static_cast<size_t>(o->ldx) * K));
  ADMM_HIP_TRY(hipMemsetAsync(o->gsum, 0, sizeof(double) * o->ldx * K, o->stream));
  ADMM_TRY(o->mem.alloc(&o->Z, static_cast<size_t>(o->ldz) * K));
  ADMM_TRY(o->mem.alloc(&o->U, static_cast<size_t>(o->ldz) * K));
  ADMM_TRY(o->mem.alloc(&o->S, static_cast<size_t>(o->ldz) * o->ns));
  ADMM_HIP_TRY(hipMemsetAsync(o->S, 0, sizeof(double) * o->ldz * o->ns, o->stream));
  ADMM_TRY(regm_upload_cols(o, o->S, o->ldz, desc->S, m, o->ns, desc->mem));
  ADMM_TRY(o->mem.alloc(&o->gpart, static_cast<size_t>(o->nwg) * K * o->ldx));
  ADMM_TRY(o->mem.alloc(&o->part, static_cast<size_t>(K) * RM_COUNT * kOvrMaxWg));
  ADMM_HIP_TRY(hipMemsetAsync(o->part, 0, sizeof(double) * K * RM_COUNT * kOvrMaxWg, o->stream));
  ADMM_TRY(o->mem.alloc(&o->par, static_cast<size_t>(4) * K));
  ADMM_HIP_TRY(hipMemcpyAsync(o->par, ph.data(), sizeof(double) * 4 * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(o->mem.alloc(&o->snorm, static_cast<size_t>(K)));
  double* raw = nullptr;
  ADMM_TRY(o->mem.alloc(&raw, (static_cast<size_t>(K) * sizeof(int32_t) + 7) / 8));
  o->kind = reinterpret_cast<int32_t*>(raw);
  ADMM_HIP_TRY(hipMemcpyAsync(o->kind, kh.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  ADMM_TRY(o->mem.alloc(&raw, (static_cast<size_t>(K) * sizeof(OvrRec) + 7) / 8));
  o->rec = reinterpret_cast<OvrRec*>(raw);
  ADMM_HIP_TRY(hipMemsetAsync(o->rec, 0, sizeof(OvrRec) * K, o->stream));
  launch_regm_snorm(o->S, o->ldz, m, K, o->ns, o->snorm, o->stream);  // perr needs max(||Dx||, ||z||, ||s_k||): once
  ADMM_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&o->rec_host), sizeof(OvrRec) * K));
  ADMM_HIP_TRY(hipEventCreate(&o->ev0));
  ADMM_HIP_TRY(hipEventCreate(&o->ev1));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (kh, ph, and the caller's buffers, were read)
  ADMM_HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int regm_poll(admm_reg_multi* o, bool* all_stopped) {
  ADMM_HIP_TRY(hipMemcpyAsync(o->rec_host, o->rec, sizeof(OvrRec) * o->K, hipMemcpyDeviceToHost, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  bool all = true;
  for (int32_t c = 0; c < o->K; ++c) all = all && o->rec_host[c].stop != 0;
  *all_stopped = all;
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
  if (desc->ns != 1 && desc->ns != desc->K)
    return fail(ADMM_E_INVALID, "S has " + std::to_string(desc->ns) + " columns: one shared response or one per fit (" +
                                    std::to_string(desc->K) + ")");
  const int32_t K = desc->K;
  std::vector<int32_t> kh(static_cast<size_t>(K), 0);
  std::vector<double> ph(static_cast<size_t>(4) * K);
  for (int32_t k = 0; k < K; ++k) {  // per fit, exactly as admm_engine_set_loss checks it
    if (desc->kind) kh[k] = desc->kind[k];
    if (kh[k] != 0 && kh[k] != 1)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": kind must be 0 (LAD family) or 1 (Huber family)");
    const admm_loss_desc ld{nullptr, desc->a ? desc->a[k] : 1.0, desc->b ? desc->b[k] : 1.0,
                            desc->epsilon ? desc->epsilon[k] : 0.0, desc->delta ? desc->delta[k] : 1.0};
    if (check_loss_desc(kh[k] ? ADMM_PROB_HUBERFIT : ADMM_PROB_LAD, ld, 0) != ADMM_OK)
      return fail(ADMM_E_INVALID, "fit " + std::to_string(k) + ": " + std::string(admm_last_error()));
    ph[4 * k + 0] = ld.slope_pos;
    ph[4 * k + 1] = ld.slope_neg;
    ph[4 * k + 2] = ld.epsilon;
    ph[4 * k + 3] = ld.delta;
  }
  if (desc->comm) return fail(ADMM_E_UNSUPPORTED, std::string("the multi-fit regression is not row-sharded") + kPerFit);
  if (desc->n > kRmMaxN)
    return fail(ADMM_E_UNSUPPORTED, "the multi-fit pass holds a 64-row block of D in registers: n <= " +
                                        std::to_string(kRmMaxN) + kPerFit);
  if (desc->m < desc->n)
    return fail(ADMM_E_UNSUPPORTED, "D must have full column rank (m >= n) for chol(D'*D) (lad.m:134)");
  admm_reg_multi* o = new admm_reg_multi();
  const int rc = regm_setup(o, desc, kh, ph);
  if (rc != ADMM_OK) {
    const std::string msg = admm_last_error();
    admm_reg_multi_destroy(o);
    return fail(rc, msg);
  }
  *out = o;
  return ADMM_OK;
}

int admm_reg_multi_run(admm_reg_multi* o, const admm_reg_multi_options* opts, admm_reg_multi_summary* summaries,
                       double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_reg_multi_options)))
    return fail(ADMM_E_INVALID, "admm_reg_multi_options.struct_size mismatch (ABI version skew)");
  admm_reg_multi_options op = *opts;
  if (op.fast != ADMM_FAST_OFF)
    return fail(ADMM_E_UNSUPPORTED, std::string("fast / accelerated ADMM is not part of the multi-fit loop") + kPerFit);
  if (op.relax != 1.0) return fail(ADMM_E_UNSUPPORTED, std::string("relaxation is not part of the multi-fit loop") + kPerFit);
  if (op.convtest) return fail(ADMM_E_UNSUPPORTED, std::string("convtest is not part of the multi-fit loop") + kPerFit);
  if (!(op.rho > 0.0)) return fail(ADMM_E_INVALID, "options.rho must be positive");
  if (op.maxiters <= 0) op.maxiters = 1000;  // admm.m:334-339
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  if (o->hist_ld != N) {
    for (double** p : {&o->pnorm, &o->perr, &o->objv}) {
      o->mem.free_one(*p);
      *p = nullptr;
      ADMM_TRY(o->mem.alloc(p, static_cast<size_t>(N) * K));
    }
    o->hist_ld = N;
  }
  o->has_run = false;
  ADMM_HIP_TRY(hipMemsetAsync(o->rec, 0, sizeof(OvrRec) * K, o->stream));
  ADMM_TRY(regm_upload_cols(o, o->X, o->ldx, op.x0, o->n, K, ADMM_MEM_HOST));
  ADMM_TRY(regm_upload_cols(o, o->Z, o->ldz, op.z0, o->m, K, ADMM_MEM_HOST));
  ADMM_TRY(regm_upload_cols(o, o->U, o->ldz, op.u0, o->m, K, ADMM_MEM_HOST));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (host buffers were read)

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
  OvrSolveArgs sa{};
  sa.M = o->M;
  sa.ldM = o->ldM;
  sa.n = o->n;
  sa.gsum = o->gsum;
  sa.X = o->X;
  sa.ldx = o->ldx;
  sa.rec = o->rec;
  const int32_t chunks = (K + kRegmChunk - 1) / kRegmChunk;
  auto pass = [&](bool init) {
    for (int32_t ch = 0; ch < chunks; ++ch) {
      pa.c0 = ch * kRegmChunk;
      launch_regm_pass(pa, init, o->stream);
    }
  };
  const int check_every = op.check_every > 0 ? op.check_every : (op.domaxiters ? 64 : 8);
  int64_t* cnt = o->launches;
  cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;

  ADMM_HIP_TRY(hipEventRecord(o->ev0, o->stream));
  pass(true);  // g = D'((s + z0) - u0)
  fa.fin = 0;
  launch_regm_gsum_fin(fa, o->stream);
  fa.fin = 1;
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    if (o->M) {
      launch_ovr_xsolve(sa, K, o->stream);
      cnt[1] += 1;
    } else {
      for (int32_t c = 0; c < K; ++c)
        launch_trsv_pair(o->eng->xfac.trsv, o->gsum + static_cast<int64_t>(c) * o->ldx,
                         o->xtmp + static_cast<int64_t>(c) * o->ldx, nullptr, o->stream);
      launch_ovr_xcopy(o->xtmp, o->X, o->ldx, o->n, K, o->rec, o->stream);
      cnt[1] += K + 1;
    }
    pass(false);
    launch_regm_gsum_fin(fa, o->stream);
    cnt[0] += 1;
    cnt[2] += chunks;
    cnt[3] += 1;
    if ((it + 1) % check_every == 0 || it + 1 == N) ADMM_TRY(regm_poll(o, &all));
  }
  ADMM_HIP_TRY(hipEventRecord(o->ev1, o->stream));
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
  ADMM_HIP_TRY(hipGetLastError());
  if (!all) return fail(ADMM_E_DEVICE, "the multi-fit loop ended with fits still running");
  float ms = 0.f;
  ADMM_HIP_TRY(hipEventElapsedTime(&ms, o->ev0, o->ev1));
  if (runtime_s) *runtime_s = 1e-3 * static_cast<double>(ms);
  o->steps.assign(static_cast<size_t>(K), 0);
  std::vector<double> objh;
  if (op.objevals) {
    objh.resize(static_cast<size_t>(N) * K);
    ADMM_HIP_TRY(hipMemcpy(objh.data(), o->objv, sizeof(double) * N * K, hipMemcpyDeviceToHost));
  }
  for (int32_t c = 0; c < K; ++c) {
    const OvrRec& r = o->rec_host[c];
    o->steps[c] = r.steps;
    if (summaries) {
      summaries[c].steps = r.steps;
      summaries[c].stopped_early = r.early;
      summaries[c].objopt = (op.objevals && r.steps > 0) ? objh[static_cast<size_t>(c) * N + r.steps - 1]
                                                         : __builtin_nan("");
    }
  }
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_reg_multi_set_weights(admm_reg_multi* o, const double* weights) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  if (weights)  // (a refused call changes nothing)
    for (int64_t i = 0; i < o->m; ++i)
      if (!finite_nonneg(weights[i]))
        return fail(ADMM_E_INVALID, "loss: weight " + std::to_string(i) + " is negative or not finite");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  double* w = nullptr;
  if (weights) {
    ADMM_TRY(o->mem.alloc(&w, static_cast<size_t>(o->m)));
    ADMM_HIP_TRY(hipMemcpyAsync(w, weights, sizeof(double) * o->m, hipMemcpyHostToDevice, o->stream));
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the caller's buffer is read until here)
  }
  if (o->W) o->mem.free_one(o->W);
  o->W = w;
  return ADMM_OK;
}

int admm_reg_multi_launches(admm_reg_multi* o, int64_t counts[5]) {
  if (!o || !counts) return fail(ADMM_E_INVALID, "object/counts is NULL");
  if (!o->has_run) return fail(ADMM_E_INVALID, "launch counts before the first run");
  for (int i = 0; i < 4; ++i) counts[i] = o->launches[i];
  counts[4] = o->M ? 1 : 0;
  return ADMM_OK;
}

int admm_reg_multi_fetch(admm_reg_multi* o, int field, double* dst, size_t cap, size_t* written) {
  if (!o || !dst) return fail(ADMM_E_INVALID, "object/dst is NULL");
  if (!o->has_run) return fail(ADMM_E_INVALID, "fetch before the first run");
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t K = o->K;
  auto matrix = [&](const double* src, int64_t ld, int64_t rows) -> int {
    const size_t need = static_cast<size_t>(rows) * K;
    if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    ADMM_HIP_TRY(hipMemcpy2D(dst, rows * sizeof(double), src, ld * sizeof(double), rows * sizeof(double), K,
                             hipMemcpyDeviceToHost));
    if (written) *written = need;
    return ADMM_OK;
  };
  auto history = [&](const double* src) -> int {
    int32_t S = 0;
    for (int32_t s : o->steps) S = s > S ? s : S;
    const size_t need = static_cast<size_t>(S) * K;
    if (cap < need) return fail(ADMM_E_CAPACITY, "destination buffer too small");
    if (S > 0)
      ADMM_HIP_TRY(hipMemcpy2D(dst, S * sizeof(double), src, o->hist_ld * sizeof(double), S * sizeof(double), K,
                               hipMemcpyDeviceToHost));
    for (int32_t c = 0; c < K; ++c)
      for (int32_t i = o->steps[c]; i < S; ++i) dst[static_cast<size_t>(c) * S + i] = __builtin_nan("");
    if (written) *written = need;
    return ADMM_OK;
  };
  switch (field) {
    case ADMM_REGM_F_XOPT: return matrix(o->X, o->ldx, o->n);
    case ADMM_REGM_F_ZOPT: return matrix(o->Z, o->ldz, o->m);
    case ADMM_REGM_F_UOPT: return matrix(o->U, o->ldz, o->m);
    case ADMM_REGM_F_PNORM: return history(o->pnorm);
    case ADMM_REGM_F_PERR: return history(o->perr);
    case ADMM_REGM_F_OBJEVALS:
      if (!o->last.objevals) return fail(ADMM_E_INVALID, "the last run did not evaluate the objective (objevals = 0)");
      return history(o->objv);
    default: return fail(ADMM_E_INVALID, "unknown field of the multi-fit regression");
  }
}

void admm_reg_multi_destroy(admm_reg_multi* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  if (o->stream) (void)hipStreamSynchronize(o->stream);
  if (o->ev0) (void)hipEventDestroy(o->ev0);
  if (o->ev1) (void)hipEventDestroy(o->ev1);
  o->mem.release();
  if (o->rec_host) (void)hipHostFree(o->rec_host);
  if (o->eng) admm_engine_destroy(o->eng);
  delete o;
}

}  // extern "C"
