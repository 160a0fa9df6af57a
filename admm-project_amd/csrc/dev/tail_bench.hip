// tail_bench.hip -- developer microbenchmark (NOT part of libadmm_hip.so): the grid of the one-launch tail behind the
// packed lower-triangle x-solve (loop_kernels.hip: prox_fin_kernel<W, S>, deferred finalize) at the headline order,
// n = 10000: ntile = 79 tiles, 80 partial rows of ldp = 10112 doubles per element.
//   make dev        (or: hipcc -O3 --offload-arch=gfx950 -I.. -o tail_bench tail_bench.hip)   ./tail_bench [n] [reps]
// Forms: tile width W x slots S with W * S = 512, W in {128, 64, 32, 16}.  Per form three kernels:
//   tail     the production kernel: gather of the partial rows + plain lasso element update + block partials
//   nogather the same kernel and grid on ONE row (naxpart = 1): the floor of launch, update and stores
//   gather   the gather and the slot fold alone (x stored, nothing else)
// Before EVERY timed launch a streaming kernel of one-wave workgroups, one per tile of the triangle, reads ~96 KB (one
// compact tile's bytes) and writes the tile's two partial rows, so that the rows sit where the x-solve leaves them:
// written by waves spread over all XCDs, behind a stream that has passed through every L2.  A back-to-back replay of
// the tail alone would find them in its own L2 and is not what the loop does.  HIP events around the tail's launch
// only; forms alternate within a repetition; median, 10th-90th percentile and minimum over the repetitions.
#include "../loop_kernels.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace admm;

#define CK(e)                                                                   \
  do {                                                                          \
    hipError_t _e = (e);                                                        \
    if (_e != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

namespace admm {  // the library's error record (engine.hip), which this program does not link
int fail(int code, const std::string& msg) {
  fprintf(stderr, "%s\n", msg.c_str());
  return code;
}
}  // namespace admm

constexpr int kStreamDoubles = 12288;  // 96 KB read per one-wave workgroup

// workgroup t = tile (bi, bj) of the lower triangle, row-major; the N-part row bj of the elements of tile bi and the
// T-part row bi of the elements of tile bj, as symv_lower_fin_kernel writes them (the sum over the stream is there to
// keep the reads; it adds an exact zero)
__global__ __launch_bounds__(kWave) void fill_rows_kernel(const double* __restrict__ stream, int64_t nstream,
                                                          double* __restrict__ npart, double* __restrict__ tpart,
                                                          int64_t ldp, double seed) {
  const unsigned t = blockIdx.x;
  unsigned bi = static_cast<unsigned>((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > t) --bi;
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  const unsigned bj = t - bi * (bi + 1) / 2;
  const int lane = threadIdx.x;
  const double* src = stream + (static_cast<int64_t>(t) * kStreamDoubles) % (nstream - kStreamDoubles);
  double s = 0.0;
#pragma unroll 8
  for (int k = 0; k < kStreamDoubles / (2 * kWave); ++k) {
    const admm_double2 v = __builtin_nontemporal_load(reinterpret_cast<const admm_double2*>(src) + k * kWave + lane);
    s += v.x + v.y;
  }
  s *= 0.0;
  const int64_t r = static_cast<int64_t>(bi) * kTailXTile + 2 * lane, c = static_cast<int64_t>(bj) * kTailXTile + 2 * lane;
  const double a = seed + 1e-3 * static_cast<double>((bi * 131u + bj * 7u + lane) % 1009u) - 0.5;
  *reinterpret_cast<admm_double2*>(npart + static_cast<int64_t>(bj) * ldp + r) = admm_double2{a + s, -0.5 * a + s};
  *reinterpret_cast<admm_double2*>(tpart + static_cast<int64_t>(bi) * ldp + c) = admm_double2{0.25 * a + s, a - s};
}

// the gather and the fold of prox_fin_kernel<W, S>, nothing else
template <int W, int S>
__global__ __launch_bounds__(kTailBlock) void gather_only_kernel(ProxArgs a) {
  __shared__ double shares[S - 1][W];
  const int e = threadIdx.x & (W - 1), slot = threadIdx.x / W;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * W + e;
  const int64_t ic = i < a.len ? i : a.len - 1;
  const double share = tail_ax_share<S>(a, ic, static_cast<int32_t>(i / kTailXTile), slot);
  const double ax = tail_fold<W, S>(share, e, slot, shares);
  if (slot == 0 && i < a.len) a.x_out[i] = ax;
}

struct Form {
  std::string name;
  int W, kind;  // kind 0 tail, 1 nogather, 2 gather
  std::vector<float> us;
};

template <int W>
static void launch_form(int kind, const ProxArgs& full, const ProxArgs& one, Ctrl* ctrl, hipStream_t st) {
  constexpr int S = kTailBlock / W;
  const dim3 grid(static_cast<unsigned>(ceil_div(full.len, W)));
  if (kind == 2) hipLaunchKernelGGL((gather_only_kernel<W, S>), grid, dim3(kTailBlock), 0, st, full);
  else hipLaunchKernelGGL((prox_fin_kernel<W, S, false>), grid, dim3(kTailBlock), 0, st, kind == 0 ? full : one, FinArgs{}, ctrl, 1);
}

static void launch_any(const Form& f, const ProxArgs& full, const ProxArgs& one, Ctrl* ctrl, hipStream_t st) {
  switch (f.W) {
    case 128: return launch_form<128>(f.kind, full, one, ctrl, st);
    case 64: return launch_form<64>(f.kind, full, one, ctrl, st);
    case 32: return launch_form<32>(f.kind, full, one, ctrl, st);
    default: return launch_form<16>(f.kind, full, one, ctrl, st);
  }
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 10000;
  const int reps = argc > 2 ? atoi(argv[2]) : 200;
  const int64_t ntile = ceil_div(n, kTailXTile), ldp = ntile * kTailXTile;
  const unsigned ntri = static_cast<unsigned>(ntile * (ntile + 1) / 2);
  if (ceil_div(n, 16) > kMaxPartBlocks) {
    fprintf(stderr, "n = %lld: more than %d workgroups at W = 16\n", static_cast<long long>(n), kMaxPartBlocks);
    return 1;
  }
  const int64_t nstream = int64_t{40} << 20;  // 320 MB of doubles: the stored inverse's size
  double *stream, *npart, *tpart, *x, *z, *u, *rhs, *dts, *part;
  Ctrl* ctrl;
  CK(hipMalloc(&stream, nstream * sizeof(double)));
  CK(hipMemset(stream, 0, nstream * sizeof(double)));
  CK(hipMalloc(&npart, ntile * ldp * sizeof(double)));
  CK(hipMalloc(&tpart, ntile * ldp * sizeof(double)));
  CK(hipMemset(npart, 0, ntile * ldp * sizeof(double)));
  CK(hipMemset(tpart, 0, ntile * ldp * sizeof(double)));
  for (double** p : {&x, &z, &u, &rhs, &dts}) {
    CK(hipMalloc(p, ldp * sizeof(double)));
    CK(hipMemset(*p, 0, ldp * sizeof(double)));
  }
  CK(hipMalloc(&part, sizeof(double) * S_COUNT * kMaxPartBlocks));
  CK(hipMalloc(&ctrl, sizeof(Ctrl)));
  CK(hipMemset(ctrl, 0, sizeof(Ctrl)));

  // the plain lasso update of the headline loop: A = I, alg 0, soft threshold, next right-hand side rho*(z - u) + D's
  ProxArgs full{};
  full.len = n;
  full.axsrc = npart;
  full.ax_t = tpart;
  full.naxpart = static_cast<int32_t>(ntile);
  full.axld = ldp;
  full.x_out = x;
  full.z = z;
  full.u = u;
  full.rhs = rhs;
  full.rhs_add = dts;
  full.part = part;
  full.rho = 1.0;
  full.relax = 1.0;
  full.t = 0.1;
  full.rho_solve = 1.0;
  full.prox = PROX_SOFT;
  full.rhs_kind = RHS_RHO_DTS;
  full.objz = OBJZ_NONE;
  full.objx = OBJX_NONE;
  full.a_identity = 1;
  full = pruned_prox_operands(full);
  ProxArgs one = full;  // one row: what the tail sums behind an x-solve without partial rows
  one.ax_t = nullptr;
  one.naxpart = 1;
  one.axld = 0;

  std::vector<Form> forms;
  for (int W : {128, 64, 32, 16})
    for (int kind = 0; kind < 3; ++kind)
      forms.push_back({std::string(kind == 0 ? "tail" : kind == 1 ? "nogather" : "gather") + " W=" + std::to_string(W) +
                           " S=" + std::to_string(kTailBlock / W), W, kind, {}});

  hipStream_t st;
  CK(hipStreamCreate(&st));
  auto fill = [&](double seed) {
    hipLaunchKernelGGL(fill_rows_kernel, dim3(ntri), dim3(kWave), 0, st, stream, nstream, npart, tpart, ldp, seed);
  };

  // every form's x against the 128 x 4 form's on the same rows: the add order differs, the sum may in the last bits
  std::vector<double> xref(n), xh(n);
  double scale = 0.0;
  for (size_t f = 0; f < forms.size(); ++f) {
    if (forms[f].kind == 1) continue;
    fill(0.25);
    CK(hipMemsetAsync(x, 0, ldp * sizeof(double), st));
    launch_any(forms[f], full, one, ctrl, st);
    CK(hipMemcpyAsync(xh.data(), x, n * sizeof(double), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    if (f == 0) {
      xref = xh;
      for (double v : xref) scale = std::max(scale, std::fabs(v));
      continue;
    }
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) worst = std::max(worst, std::fabs(xh[i] - xref[i]));
    if (!(worst <= 1e-13 * scale)) {
      fprintf(stderr, "%s: x differs from the 128 x 4 form by %.3e (largest |x| %.3e)\n", forms[f].name.c_str(), worst, scale);
      return 1;
    }
  }

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int r = -5; r < reps; ++r)  // five untimed rounds first
    for (Form& f : forms) {
      fill(1e-3 * (r & 7));
      CK(hipEventRecord(e0, st));
      launch_any(f, full, one, ctrl, st);
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) f.us.push_back(ms * 1e3f);
    }
  CK(hipGetLastError());

  printf("n = %lld, %lld tiles, %lld partial rows of %lld doubles, %d launches per form (us per launch)\n",
         static_cast<long long>(n), static_cast<long long>(ntile), static_cast<long long>(ntile + 1),
         static_cast<long long>(ldp), reps);
  printf("%-24s %8s %8s %8s %8s %8s\n", "form", "grid", "median", "p10", "p90", "min");
  for (Form& f : forms) {
    std::sort(f.us.begin(), f.us.end());
    const size_t k = f.us.size();
    printf("%-24s %8lld %8.2f %8.2f %8.2f %8.2f\n", f.name.c_str(), static_cast<long long>(ceil_div(n, f.W)), f.us[k / 2],
           f.us[k / 10], f.us[(9 * k) / 10], f.us[0]);
  }
  return 0;
}
