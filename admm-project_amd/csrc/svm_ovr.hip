// svm_ovr.hip -- the linear SVM for all one-vs-rest classes at once (examples/mnistsvm.m:88-102: one linearsvm call per
// digit and loss on the same D).  xminLinearSVM is Dplus*(z - u) (getProxOps.m:1062-1068) and does not contain ell; the
// labels enter the element-wise z-prox (getProxOps.m:1084-1103) and the objective (linearsvm.m:231-237) alone.  K classes
// are therefore K independent plain-ADMM runs (unwrappedadmm.m:76-92) that share D, the map (D'D)^-1 and every byte an
// iteration reads from HBM.  Per iteration:
//   ovr_xsolve_kernel    x_c = M g_c for every running class (M symmetric n x n, n <= 448: small)
//   ovr_pass_kernel      ONE read of D for a chunk of kOvrChunk classes: the 64-row block in registers as in
//                        ad_onepass_kernel (unwrapped.hip) -- lane = row, wave w owns the columns j = w (mod 8) --, then
//                        per class (D x_c)_r, the fused element update (prox_apply: the code every loop shares), and the
//                        block's contribution D_r' t_r to the class's next right-hand side g_c = D'(z_c - u_c)
//   ovr_gsum_fin_kernel  sums the workgroups' partial rows of g_c; one extra workgroup per class turns the block partials
//                        into pnorm, perr, Hnormsq, the objective and the stop decision (admm.m:612-722)
// A class whose stop flag is set is FROZEN: every kernel skips it, so its X, Z, U columns and histories are those of an
// independent run with that many steps.  Every sum runs in a fixed order that does not depend on which chunk or slot a
// class occupies: runs are bitwise reproducible, and a class gets the same numbers wherever it lands.
// All loads of D are unconditional on clamped addresses (x is zero beyond n; rows beyond m carry t = 0).
#include <vector>

#include "multi_host.h"
#include "prox_device.h"
#include "svm_cost_device.h"
#include "svm_ovr.h"
#include "wave_reduce.h"

namespace admm {

constexpr int kOvRows = 64, kOvWaves = 8, kOvCols = 56, kOvMaxN = kOvWaves * kOvCols;  // 448, as ad_onepass_kernel
static_assert(kOvMaxN == ADMM_SVM_OVR_MAX_N, "the header states the limit");
constexpr int kOvSlotsPerWave = (kOvrChunk + kOvWaves - 1) / kOvWaves;  // classes whose element update one wave runs

// the ProxArgs of one class: plain ADMM, B = -1, c = 0, no histories (the compiler folds the constant fields)
template <bool LOGI>
__device__ __forceinline__ ProxArgs ovr_prox_args(const OvrPassArgs& a, int cls, int32_t loss) {
  ProxArgs pa{};
  pa.len = a.m;
  pa.z = a.Z + static_cast<int64_t>(cls) * a.ldz;
  pa.u = a.U + static_cast<int64_t>(cls) * a.ldz;
  pa.ell = a.ELL + static_cast<int64_t>(cls) * a.ldz;
  pa.rho = a.rho;
  pa.relax = 1.0;
  pa.prox = (loss == ADMM_LOSS_01) ? PROX_01 : PROX_HINGE;                   // getProxOps.m:1094
  pa.t = (loss == ADMM_LOSS_01) ? a.rho / a.C : a.C / a.rho;                 // getProxOps.m:1100 | 1096
  pa.objx = !a.objevals ? OBJX_NONE : (loss == ADMM_LOSS_HINGE ? OBJX_HINGE : OBJX_ZEROONE);  // linearsvm.m:231-237
  if (LOGI && loss == ADMM_LOSS_LOGISTIC) {
    pa.prox = PROX_LOGISTIC;
    pa.objx = a.objevals ? OBJX_LOGISTIC : OBJX_NONE;
  }
  pa.objz = OBJZ_NONE;
  pa.alg = 0;
  pa.a_identity = 0;
  pa.rhs_kind = RHS_NONE;
  return pa;
}

// the one element of ovr_pass_kernel's Cost... parameter pack
__device__ __forceinline__ const OvrCostArgs& ovr_cost_of(const OvrCostArgs& c) { return c; }

// INIT: only the partial rows of D'(z0 - u0), before the first iteration.  LOGI: the chunk holds a logistic class (the
// launcher knows the losses): the instantiation whose element update carries logistic_root (prox_device.h).
// Cost = OvrCostArgs: the chunk holds a class with costs or the squared hinge, or the run has weights:
// every class of the chunk takes the cost form of the element update (svm_cost_device.h), the weight of a row is loaded
// once per block beside the block of D and the class costs once per class.  An empty pack everywhere else.
template <int KC, bool INIT, bool LOGI, class... Cost>
__global__ __launch_bounds__(kOvWaves* kWave) void ovr_pass_kernel(OvrPassArgs a, Cost... oc) {
  constexpr bool COST = sizeof...(Cost) != 0;
  __shared__ __attribute__((aligned(16))) double xs[kOvMaxN * KC];  // [column][class]: one column's KC values contiguous
  __shared__ double gacc[KC * kOvMaxN];
  __shared__ double axr[kOvWaves * KC * kOvRows];
  __shared__ double tsh[KC * kOvRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n = a.n, m = a.m;
  uint32_t actv = 0;  // bit c: class c0 + c exists and is still running
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int cls = a.c0 + c;
    const int32_t st = a.rec[cls < a.K ? cls : a.K - 1].stop;
    if (cls < a.K && st == 0) actv |= 1u << c;
  }
  const uint32_t act = __builtin_amdgcn_readfirstlane(actv);
  if (act == 0) return;  // every class of the chunk has stopped: a no-op
  for (int idx = tid; idx < kOvMaxN * KC; idx += kOvWaves * kWave) {
    const int j = idx / KC, c = idx - j * KC;
    const int cls = a.c0 + c;
    double xv = 0.0;
    if (!INIT && j < n && cls < a.K) xv = a.X[static_cast<int64_t>(cls) * a.ldx + j];
    xs[idx] = xv;
    gacc[idx] = 0.0;
  }
  __syncthreads();
  // the classes whose element update this wave runs: w, w + 8, ...
  double acc[kOvSlotsPerWave][S_COUNT];
  ProxArgs pas[kOvSlotsPerWave];
#pragma unroll
  for (int s = 0; s < kOvSlotsPerWave; ++s) {
#pragma unroll
    for (int q = 0; q < S_COUNT; ++q) acc[s][q] = 0.0;
    const int c = w + kOvWaves * s;
    const int cls = (a.c0 + c < a.K) ? a.c0 + c : a.K - 1;
    pas[s] = ovr_prox_args<LOGI>(a, cls, a.loss[cls]);
  }
  [[maybe_unused]] SvmCostArgs ks[COST ? kOvSlotsPerWave : 1];
  if constexpr (COST) {
#pragma unroll
    for (int s = 0; s < kOvSlotsPerWave; ++s) {
      const int c = w + kOvWaves * s;
      const int cls = (a.c0 + c < a.K) ? a.c0 + c : a.K - 1;
      const double* __restrict__ cc = ovr_cost_of(oc...).class_cost + 2 * cls;
      ks[s] = SvmCostArgs{nullptr, cc[0], cc[1], a.C, a.rho, a.loss[cls], a.objevals};
      pas[s].prox = PROX_GIVEN;  // z reaches prox_apply in a register; the objective's terms are summed beside it
      pas[s].objx = OBJX_NONE;
    }
  }
  const int64_t nblocks = (m + kOvRows - 1) / kOvRows;
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int64_t r = blk * kOvRows + lane;
    const int64_t rc = r < m ? r : m - 1;
    const double* __restrict__ drow = a.D + rc;
    double d[kOvCols];
#pragma unroll
    for (int k = 0; k < kOvCols; ++k) {  // clamped columns: the loads stay unconditional, x is zero beyond n
      const int64_t j = w + kOvWaves * k;
      d[k] = drow[(j < n ? j : n - 1) * a.ldD];
    }
    double zp[kOvSlotsPerWave], uo[kOvSlotsPerWave], el[kOvSlotsPerWave];
#pragma unroll
    for (int s = 0; s < kOvSlotsPerWave; ++s) {  // in flight with the block
      zp[s] = pas[s].z[rc];
      uo[s] = pas[s].u[rc];
      el[s] = pas[s].ell[rc];
    }
    double wv = 1.0;
    if constexpr (COST) {  // one m-vector for all classes: redirected to z without weights, so the load stays unconditional
      const OvrCostArgs& k = ovr_cost_of(oc...);
      const double* pw = k.w ? k.w : pas[0].z;
      const double wl = pw[rc];
      wv = k.w ? wl : 1.0;
    }
    if (!INIT) {
      double p[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) p[c] = 0.0;
#pragma unroll
      for (int k = 0; k < kOvCols; ++k) {
        const double* __restrict__ xk = xs + (w + kOvWaves * k) * KC;  // same address in every lane: LDS broadcast
#pragma unroll
        for (int c = 0; c < KC; ++c) p[c] = __builtin_fma(d[k], xk[c], p[c]);
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) axr[(w * KC + c) * kOvRows + lane] = p[c];
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < kOvSlotsPerWave; ++s) {
      const int c = w + kOvWaves * s;
      if (c < KC && ((act >> c) & 1u)) {  // wave-uniform
        double t = 0.0;
        if (INIT) {
          if (r < m) t = (0.0 + zp[s]) - uo[s];  // (c + z0) - u0 with c = 0, as prox_apply forms it
        } else {
          double ax = axr[c * kOvRows + lane];
#pragma unroll
          for (int q = 1; q < kOvWaves; ++q) ax += axr[(q * KC + c) * kOvRows + lane];
          ProxIn in{};
          in.zp = zp[s];
          in.u_old = uo[s];
          in.uhat_i = uo[s];
          in.ell_i = el[s];
          if constexpr (COST) {
            if (r < m) {
              loss_form_z<LOGI>(pas[s], ks[s], wv, ax, in, acc[s]);
              prox_apply<false>(pas[s], r, ax, 0, 0.0, in, acc[s], &t);
            }
          } else {
            if (r < m) prox_apply<LOGI>(pas[s], r, ax, 0, 0.0, in, acc[s], &t);
          }
        }
        tsh[c * kOvRows + lane] = t;  // rows beyond m contribute nothing
      }
    }
    __syncthreads();
    static_assert(kOvCols % kSyPanel == 0, "column sums are taken four at a time");
#pragma unroll 1
    for (int c = 0; c < KC; ++c) {
      if (!((act >> c) & 1u)) continue;  // wave-uniform
      const double t = tsh[c * kOvRows + lane];
#pragma unroll
      for (int k = 0; k < kOvCols; k += kSyPanel) {  // four column sums per permlane / DPP reduce-scatter (wave_reduce.h)
        double q[kSyPanel];
#pragma unroll
        for (int i = 0; i < kSyPanel; ++i) q[i] = d[k + i] * t;
        const double sum = reduce_scatter4(q);  // lanes 16i .. 16i+15 hold the sum of column k + i
        const int j = w + kOvWaves * (k + (lane >> 4));
        if ((lane & 15) == 0 && j < n) gacc[c * kOvMaxN + j] += sum;  // (each wave owns its columns)
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
    for (int j = tid; j < n; j += kOvWaves * kWave) gout[j] = gacc[c * kOvMaxN + j];
  }
  if (INIT) return;
  constexpr int slot_of[OV_COUNT] = {S_R2, S_AX2, S_Z2, S_DZ2, S_DU2, S_OBJX};
#pragma unroll
  for (int s = 0; s < kOvSlotsPerWave; ++s) {
    const int c = w + kOvWaves * s;
    if (c < KC && ((act >> c) & 1u)) {
#pragma unroll
      for (int q = 0; q < OV_COUNT; ++q) {
        const double v = wave_sum(acc[s][slot_of[q]]);
        if (lane == 0) a.part[(static_cast<int64_t>(a.c0 + c) * OV_COUNT + q) * kMultiMaxWg + blockIdx.x] = v;
      }
    }
  }
}

// blockIdx.y = class.  blockIdx.x < tiles: g_c[64 columns] = sum over the workgroups' partial rows (multi_gsum_tile).
// The extra workgroup (a.fin): the finalize logic of the class's iteration -- admm.m:612-722 as oracle/admm_ref.py
// restates it, for plain ADMM with nodualerror = 1 and stopcond = 'both'.
__global__ __launch_bounds__(kBlock) void ovr_gsum_fin_kernel(OvrFinArgs a) {
  const int cls = blockIdx.y;
  MultiRec* rec = a.rec + cls;
  const int32_t stopped = rec->stop;
  const int32_t it = rec->iter;
  if (stopped) return;
  __shared__ double sq[4][kMultiTile];
  __shared__ double S[8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles = static_cast<int>((a.n + kMultiTile - 1) / kMultiTile);
  if (static_cast<int>(blockIdx.x) < tiles) {
    multi_gsum_tile(a.gpart, a.gsum, cls, a.ldx, a.n, a.K, a.nwg, sq);
    return;
  }
  // ---- finalize of class cls
  multi_slot_totals_unrolled(a.part, cls, OV_COUNT, a.nwg, S);
  double xx = 0.0;
  if (a.objevals) {
    const double* __restrict__ x = a.X + static_cast<int64_t>(cls) * a.ldx;
    for (int64_t j = tid; j < a.n; j += kBlock) xx += x[j] * x[j];
  }
  xx = wave_sum(xx);
  if (lane == 0) sq[0][wid] = xx;
  __syncthreads();
  if (tid != 0) return;
  const double nx2 = ((sq[0][0] + sq[0][1]) + sq[0][2]) + sq[0][3];
  const int i1 = it + 1;  // 1-based iteration number (admm.m loop variable)
  const int64_t h = static_cast<int64_t>(cls) * a.hist_ld + it;
  const double hn = a.rho * S[OV_DZ2] + a.rho * (a.rho * a.rho) * S[OV_DU2];  // admm.m:305-306, w = [x; z; rho*u]
  a.hnorm[h] = hn;
  if (a.objevals) a.objv[h] = a.C * S[OV_OBJX] + 0.5 * nx2;  // linearsvm.m:231-237
  const double pn = sqrt(S[OV_R2]);  // admm.m:621
  const double pe = sqrt(static_cast<double>(a.m)) * a.abstol +
                    a.reltol * fmax(fmax(sqrt(S[OV_AX2]), sqrt(S[OV_Z2])), 0.0);  // admm.m:644-650, c = 0
  a.pnorm[h] = pn;
  a.perr[h] = pe;
  bool stop = false;
  if (!a.domaxiters && pn < pe) stop = true;                        // admm.m:710-713, nodualerror
  if (!a.domaxiters && i1 > 2 && hn <= a.Hnormtol) stop = true;     // admm.m:719-722
  multi_stop_tail(rec, stop, i1, a.maxiters);
}

// x_c(64 rows) = M(64 rows, :) g_c: lane = row (M is symmetric: column-major reads are coalesced along the row index),
// wave q takes the columns j = q (mod 4), the four partial sums added in wave order
__global__ __launch_bounds__(kBlock) void ovr_xsolve_kernel(OvrSolveArgs a) {
  const int cls = blockIdx.y;
  if (a.rec[cls].stop) return;
  __shared__ double gs[kOvMaxN + 32];  // (the unrolled column loop reads up to 28 entries past its start: zeros)
  __shared__ double red[4][kMultiTile];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t n = a.n;
  for (int j = tid; j < kOvMaxN + 32; j += kBlock) gs[j] = j < n ? a.gsum[static_cast<int64_t>(cls) * a.ldx + j] : 0.0;
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kMultiTile + lane;
  const double* __restrict__ mrow = a.M + (i < n ? i : n - 1);
  double s = 0.0;
  for (int j0 = wid; j0 < n; j0 += 4 * 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t j = j0 + 4 * k;
      v[k] = mrow[(j < n ? j : n - 1) * a.ldM];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s = __builtin_fma(v[k], gs[j0 + 4 * k], s);  // gs is zero beyond n
  }
  red[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && i < n)
    a.X[static_cast<int64_t>(cls) * a.ldx + i] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

__global__ __launch_bounds__(kBlock) void ovr_xcopy_kernel(const double* __restrict__ Xnew, double* __restrict__ X,
                                                           int64_t ldx, int64_t n, const MultiRec* __restrict__ rec) {
  const int cls = blockIdx.y;
  if (rec[cls].stop) return;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < n) X[static_cast<int64_t>(cls) * ldx + j] = Xnew[static_cast<int64_t>(cls) * ldx + j];
}

int ovr_pass_workgroups(int64_t m) {
  return static_cast<int>(std::min<int64_t>(ceil_div(m, int64_t{kOvRows}), kMultiMaxWg));  // one per CU
}

void launch_ovr_pass(const OvrPassArgs& a, bool init, bool logistic, const OvrCostArgs* cost, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(ovr_pass_workgroups(a.m))), block(kOvWaves * kWave);
  if (init) hipLaunchKernelGGL((ovr_pass_kernel<kOvrChunk, true, false>), grid, block, 0, stream, a);  // (no element update)
  else if (cost && logistic)
    hipLaunchKernelGGL((ovr_pass_kernel<kOvrChunk, false, true, OvrCostArgs>), grid, block, 0, stream, a, *cost);
  else if (cost) hipLaunchKernelGGL((ovr_pass_kernel<kOvrChunk, false, false, OvrCostArgs>), grid, block, 0, stream, a, *cost);
  else if (logistic) hipLaunchKernelGGL((ovr_pass_kernel<kOvrChunk, false, true>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((ovr_pass_kernel<kOvrChunk, false, false>), grid, block, 0, stream, a);
}

void launch_ovr_gsum_fin(const OvrFinArgs& a, hipStream_t stream) {
  const unsigned tiles = static_cast<unsigned>(ceil_div(a.n, int64_t{kMultiTile}));
  hipLaunchKernelGGL(ovr_gsum_fin_kernel, dim3(tiles + (a.fin ? 1u : 0u), static_cast<unsigned>(a.K)), dim3(kBlock), 0,
                     stream, a);
}

void launch_ovr_xsolve(const OvrSolveArgs& a, int32_t K, hipStream_t stream) {
  hipLaunchKernelGGL(ovr_xsolve_kernel,
                     dim3(static_cast<unsigned>(ceil_div(a.n, int64_t{kMultiTile})), static_cast<unsigned>(K)),
                     dim3(kBlock), 0, stream, a);
}

void launch_ovr_xcopy(const double* Xnew, double* X, int64_t ldx, int64_t n, int32_t K, const MultiRec* rec,
                      hipStream_t stream) {
  hipLaunchKernelGGL(ovr_xcopy_kernel, dim3(static_cast<unsigned>(ceil_div(n, int64_t{kBlock})), static_cast<unsigned>(K)),
                     dim3(kBlock), 0, stream, Xnew, X, ldx, n, rec);
}

}  // namespace admm

// ---------------------------------------------------------------------------------------------------------- the object
struct admm_svm_ovr : DenseMulti {  // eng: an ordinary ADMM_PROB_LINEARSVM engine
  double C = 0.0;
  double* ELL = nullptr;
  int32_t* loss = nullptr;
  std::vector<char> chunk_logistic;  // per chunk of kOvrChunk classes: one of them has ADMM_LOSS_LOGISTIC
  // costs (admm_svm_ovr_set_cost): defaults = the kernels of a run without them, bit for bit
  std::vector<int32_t> loss_host;    // the K losses
  std::vector<double> cost_host;     // K x 2 (cost_pos, cost_neg); all ones by default
  double* W = nullptr;               // m shared weights on the device, or null: every weight is 1
  double* CC = nullptr;              // cost_host on the device
  std::vector<int32_t> chunk_cost;   // per chunk: weights, a class cost != 1 or ADMM_LOSS_SQHINGE -> the cost form
  double *pnorm = nullptr, *perr = nullptr, *hnorm = nullptr, *objv = nullptr;  // histories
  admm_svm_ovr_options last{};
};

namespace {

const char* kPerClass = ": run one ADMM_PROB_LINEARSVM engine (admm_engine_create) per class instead";

int ovr_setup(admm_svm_ovr* o, const admm_svm_ovr_desc* desc) {
  const int64_t m = desc->m, n = desc->n;
  const int32_t K = desc->K;
  admm_problem_desc d;
  admm_problem_desc_default(&d);
  d.problem = ADMM_PROB_LINEARSVM;
  d.m = m;
  d.n = n;
  d.D = desc->D;
  d.ldD = desc->ldD;
  d.ell = desc->ELL;  // (the engine wants one label vector; it never runs)
  d.C = desc->C;
  d.loss = ADMM_LOSS_HINGE;
  d.mem = desc->mem;
  d.device = desc->device;
  ADMM_TRY(admm_engine_create(&d, &o->eng));
  o->stream = o->eng->stream;
  o->C = desc->C;
  if (desc->Dplus) {  // (D'D)^+ = Dplus*Dplus' from the caller's pseudo-inverse (linearsvm.m:185-186)
    double *Dp = nullptr, *Mo = nullptr;
    ADMM_TRY(upload(o->mem, &Dp, desc->Dplus, static_cast<size_t>(n) * m, desc->mem, o->stream));
    const int64_t ld = round_up(n, 2);
    ADMM_TRY(o->mem.alloc(&Mo, static_cast<size_t>(ld) * n));
    ADMM_HIP_TRY(hipMemsetAsync(Mo, 0, sizeof(double) * ld * n, o->stream));
    launch_gemm(0, 1, n, n, m, 1.0, Dp, n, Dp, n, 0.0, Mo, ld, false, o->stream);
    ADMM_HIP_TRY(hipStreamSynchronize(o->stream));
    o->mem.free_one(Dp);
    o->M = Mo;
    o->ldM = ld;
  }
  ADMM_TRY(dense_setup(*o, m, n, K, OV_COUNT, kPerClass));
  ADMM_TRY(o->mem.alloc(&o->ELL, static_cast<size_t>(o->ldz) * K));
  ADMM_HIP_TRY(hipMemsetAsync(o->ELL, 0, sizeof(double) * o->ldz * K, o->stream));
  ADMM_TRY(upload_cols(*o, o->ELL, o->ldz, desc->ELL, m, K, desc->mem));
  ADMM_TRY(alloc_words(*o, &o->loss, static_cast<size_t>(K)));
  o->loss_host.assign(static_cast<size_t>(K), ADMM_LOSS_HINGE);
  if (desc->loss) o->loss_host.assign(desc->loss, desc->loss + K);
  o->chunk_logistic.assign(static_cast<size_t>((K + kOvrChunk - 1) / kOvrChunk), 0);
  for (int32_t c = 0; c < K; ++c)
    if (o->loss_host[c] == ADMM_LOSS_LOGISTIC) o->chunk_logistic[c / kOvrChunk] = 1;
  ADMM_HIP_TRY(hipMemcpyAsync(o->loss, o->loss_host.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, o->stream));
  o->cost_host.assign(static_cast<size_t>(2 * K), 1.0);
  ADMM_TRY(o->mem.alloc(&o->CC, static_cast<size_t>(2 * K)));
  ADMM_HIP_TRY(hipMemcpyAsync(o->CC, o->cost_host.data(), sizeof(double) * 2 * K, hipMemcpyHostToDevice, o->stream));
  o->chunk_cost = svm_cost_chunks(K, kOvrChunk, false, o->loss_host, o->cost_host);
  ADMM_HIP_TRY(hipStreamSynchronize(o->stream));  // (the host vectors, and the caller's buffers, were read)
  return ADMM_OK;
}

}  // namespace

extern "C" {

void admm_svm_ovr_desc_default(admm_svm_ovr_desc* d) {
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->struct_size = sizeof(admm_svm_ovr_desc);
  d->K = 1;
}

void admm_svm_ovr_options_default(admm_svm_ovr_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = sizeof(admm_svm_ovr_options);
  o->maxiters = 1000;  // unwrappedadmm.m:90
  o->rho = 1.0;        // admm.m:57
  o->abstol = 1e-5;    // admm.m:71
  o->reltol = 1e-3;    // admm.m:72
  o->Hnormtol = 1e-6;  // admm.m:73
  o->relax = 1.0;      // admm.m:60
}

int admm_svm_ovr_chunk(void) { return kOvrChunk; }

int admm_svm_ovr_create(const admm_svm_ovr_desc* desc, admm_svm_ovr** out) {
  if (!desc || !out) return fail(ADMM_E_INVALID, "desc/out is NULL");
  *out = nullptr;
  if (desc->struct_size != static_cast<int32_t>(sizeof(admm_svm_ovr_desc)))
    return fail(ADMM_E_INVALID, "admm_svm_ovr_desc.struct_size mismatch (ABI version skew)");
  if (desc->K < 1) return fail(ADMM_E_INVALID, "the one-vs-rest linear SVM needs at least one class (K >= 1)");
  if (!desc->D || desc->m <= 0 || desc->n <= 0) return fail(ADMM_E_INVALID, "the linear SVM needs D (m x n)");
  if (!desc->ELL) return fail(ADMM_E_INVALID, "the linear SVM needs the label matrix ELL (m x K)");
  if (!(desc->C >= 0.0)) return fail(ADMM_E_INVALID, "Given regularization parameter C is not a nonnegative number!");
  ADMM_TRY(check_svm_losses(desc->K, desc->loss));
  if (desc->comm)
    return fail(ADMM_E_UNSUPPORTED, std::string("the one-vs-rest linear SVM is not row-sharded") + kPerClass);
  if (desc->n > kOvMaxN)
    return fail(ADMM_E_UNSUPPORTED, "the one-vs-rest pass holds a 64-row block of D in registers: n <= " +
                                        std::to_string(kOvMaxN) + kPerClass);
  return create_object(out, admm_svm_ovr_destroy, [&](admm_svm_ovr* o) { return ovr_setup(o, desc); });
}

int admm_svm_ovr_run(admm_svm_ovr* o, const admm_svm_ovr_options* opts, admm_svm_ovr_summary* summaries,
                     double* runtime_s) {
  if (!o || !opts) return fail(ADMM_E_INVALID, "object/options is NULL");
  if (opts->struct_size != static_cast<int32_t>(sizeof(admm_svm_ovr_options)))
    return fail(ADMM_E_INVALID, "admm_svm_ovr_options.struct_size mismatch (ABI version skew)");
  admm_svm_ovr_options op = *opts;
  ADMM_TRY(check_run_options("one-vs-rest", kPerClass, &op));
  ADMM_HIP_TRY(hipSetDevice(o->device));
  const int32_t N = op.maxiters, K = o->K;
  ADMM_TRY(resize_histories(*o, {&o->pnorm, &o->perr, &o->hnorm, &o->objv}, N));
  ADMM_TRY(dense_start(*o, op.x0, op.z0, op.u0));

  OvrPassArgs pa{};
  pa.D = o->eng->D;
  pa.ldD = o->eng->ldD;
  pa.m = o->m;
  pa.n = o->n;
  pa.X = o->X;
  pa.ldx = o->ldx;
  pa.Z = o->Z;
  pa.U = o->U;
  pa.ELL = o->ELL;
  pa.ldz = o->ldz;
  pa.loss = o->loss;
  pa.gpart = o->gpart;
  pa.part = o->part;
  pa.rec = o->rec;
  pa.K = K;
  pa.objevals = op.objevals;
  pa.rho = op.rho;
  pa.C = o->C;
  OvrFinArgs fa{};
  fa.gpart = o->gpart;
  fa.gsum = o->gsum;
  fa.part = o->part;
  fa.X = o->X;
  fa.ldx = o->ldx;
  fa.n = o->n;
  fa.m = o->m;
  fa.K = K;
  fa.nwg = o->nwg;
  fa.rec = o->rec;
  fa.pnorm = o->pnorm;
  fa.perr = o->perr;
  fa.hnorm = o->hnorm;
  fa.objv = o->objv;
  fa.hist_ld = N;
  fa.rho = op.rho;
  fa.C = o->C;
  fa.abstol = op.abstol;
  fa.reltol = op.reltol;
  fa.Hnormtol = op.Hnormtol;
  fa.domaxiters = op.domaxiters;
  fa.objevals = op.objevals;
  fa.maxiters = N;
  const OvrCostArgs oc{o->W, o->CC};
  const int32_t chunks = (K + kOvrChunk - 1) / kOvrChunk;
  auto pass = [&](bool init) {
    for (int32_t ch = 0; ch < chunks; ++ch) {
      pa.c0 = ch * kOvrChunk;
      launch_ovr_pass(pa, init, o->chunk_logistic[ch] != 0, o->chunk_cost[ch] ? &oc : nullptr, o->stream);
    }
  };

  ADMM_TRY(begin_timing(*o));
  pass(true);  // g = D'(z0 - u0)
  fa.fin = 0;
  launch_ovr_gsum_fin(fa, o->stream);
  fa.fin = 1;
  bool all = false;
  for (int32_t it = 0; it < N && !all; ++it) {
    dense_xupdate(*o);
    pass(false);
    launch_ovr_gsum_fin(fa, o->stream);
    if ((it + 1) % op.check_every == 0 || it + 1 == N) ADMM_TRY(poll_all_stopped(*o, &all));
  }
  ADMM_TRY(finish_run(*o, all, "the one-vs-rest loop ended with classes still running", N, op.objevals != 0, o->objv,
                      runtime_s, summaries));
  o->last = op;
  o->has_run = true;
  return ADMM_OK;
}

int admm_svm_ovr_set_cost(admm_svm_ovr* o, const double* weights, const double* class_cost) {
  if (!o) return fail(ADMM_E_INVALID, "object is NULL");
  ADMM_TRY(set_svm_cost(*o, o->m, weights, class_cost, &o->W, o->CC, &o->cost_host));
  o->chunk_cost = svm_cost_chunks(o->K, kOvrChunk, o->W != nullptr, o->loss_host, o->cost_host);
  return ADMM_OK;
}

int admm_svm_ovr_fetch(admm_svm_ovr* o, int field, double* dst, size_t cap, size_t* written) {
  ADMM_TRY(fetch_head(o, dst));
  switch (field) {
    case ADMM_OVR_F_XOPT: return fetch_cols(*o, o->X, o->ldx, o->n, dst, cap, written);
    case ADMM_OVR_F_ZOPT: return fetch_cols(*o, o->Z, o->ldz, o->m, dst, cap, written);
    case ADMM_OVR_F_UOPT: return fetch_cols(*o, o->U, o->ldz, o->m, dst, cap, written);
    case ADMM_OVR_F_PNORM: return fetch_history(*o, o->pnorm, dst, cap, written);
    case ADMM_OVR_F_PERR: return fetch_history(*o, o->perr, dst, cap, written);
    case ADMM_OVR_F_HNORMSQ: return fetch_history(*o, o->hnorm, dst, cap, written);
    case ADMM_OVR_F_OBJEVALS: return fetch_kept_history(*o, o->last.objevals, kNoObjevals, o->objv, dst, cap, written);
    default: return fail(ADMM_E_INVALID, "unknown field of the one-vs-rest linear SVM");
  }
}

void admm_svm_ovr_destroy(admm_svm_ovr* o) {
  if (!o) return;
  dense_destroy(*o);
  delete o;
}

}  // extern "C"
