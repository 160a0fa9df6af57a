// symm_bench.hip -- developer microbenchmark (NOT part of libadmm_hip.so): the symmetric tile-packed product over a
// chunk of right-hand sides (symm.hip) at the order of the benchmark problem, event-timed, beside the
// packed single-vector product of symv.hip on the same tiles and a pure read of them.
//   hipcc -O3 --offload-arch=gfx950 -I.. -o symm_bench symm_bench.hip && ./symm_bench [n] [reps]
// Prints per K (1, 5, 10, 20 fits): us per launch pair (tile pass + partial-row sum), each of the two alone, the stored
// bytes of the matrix over the tile pass's time, and the FMA rate; then K back-to-back symv launches for comparison.
#include "../symm.hip"
#include "../symv.hip"

#include <cstdio>
#include <cstdlib>
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

namespace admm {  // (trsv.hip is not linked: launch_symv_pack is never called here)
void launch_tri_pack(const double*, int64_t, double*, unsigned, int, hipStream_t) {}
}  // namespace admm

__global__ void fill_tiles(double* P, size_t elems) {
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < elems;
       i += static_cast<size_t>(gridDim.x) * blockDim.x)
    P[i] = 1e-3 * static_cast<double>((i * 131) % 1009) - 0.5;
}

// every tile read once with the product's own loads and nothing else: the stream rate the tile pass is held against
__global__ __launch_bounds__(kWave) void read_tiles(const double* __restrict__ P, double* __restrict__ out) {
  const double* T = P + static_cast<int64_t>(blockIdx.x) * (kTile * kTile);
  double s = 0.0;
  for (int q = 0; q < 4; ++q) {
    admm_double2 d[kTile / 4];
#pragma unroll
    for (int j = 0; j < kTile / 4; ++j)  // pair (32 q + j) * 64 + lane of the tile's 8192
      d[j] = load2<true>(T + 2 * (((q * (kTile / 4) + j) * kWave) + static_cast<int>(threadIdx.x)));
#pragma unroll
    for (int j = 0; j < kTile / 4; ++j) s += d[j].x + d[j].y;
  }
  if (s == 12345.678) out[blockIdx.x] = s;
}

template <class F>
static double time_us(F&& f, int reps) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) f();
  CK(hipDeviceSynchronize());
  std::vector<float> ms(reps);
  for (int i = 0; i < reps; ++i) {
    CK(hipEventRecord(a, nullptr));
    f();
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    CK(hipEventElapsedTime(&ms[i], a, b));
  }
  std::sort(ms.begin(), ms.end());
  return 1e3 * ms[reps / 2];
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 10000;
  const int reps = argc > 2 ? atoi(argv[2]) : 20;
  SymvPlan plan = symv_plan(n);
  plan.packed = true;
  plan.ncached = symv_cached_tiles(plan, kSymvCacheBytes);
  const size_t pel = symv_packed_elems(plan);
  const int64_t tiles = symv_tiles(plan);
  const int KMAX = 20;
  double *P, *Y, *X, *part, *np_, *tp_, *out;
  CK(hipMalloc(&P, pel * 8));
  CK(hipMalloc(&Y, static_cast<size_t>(spmm_chunks(KMAX)) * kSpmmChunk * n * 8));
  CK(hipMalloc(&X, static_cast<size_t>(spmm_chunks(KMAX)) * kSpmmChunk * n * 8));
  CK(hipMalloc(&part, symm_part_elems(plan, KMAX) * 8));
  CK(hipMalloc(&np_, plan.npart_elems() * 8));
  CK(hipMalloc(&tp_, plan.tpart_elems() * 8));
  CK(hipMalloc(&out, tiles * 8));
  hipLaunchKernelGGL(fill_tiles, dim3(1024), dim3(256), 0, nullptr, P, pel);
  hipLaunchKernelGGL(fill_tiles, dim3(1024), dim3(256), 0, nullptr, Y, static_cast<size_t>(spmm_chunks(KMAX)) * kSpmmChunk * n);
  CK(hipMemset(np_, 0, plan.npart_elems() * 8));
  CK(hipMemset(tp_, 0, plan.tpart_elems() * 8));
  CK(hipDeviceSynchronize());
  const double bytes = 8.0 * pel;
  printf("n = %lld: %lld tiles, %.1f MB stored, part rows %d x %lld x %d\n", static_cast<long long>(n),
         static_cast<long long>(tiles), bytes / 1e6, plan.ntile + 1, static_cast<long long>(plan.npad), kSpmmChunk);
  const double t_read = time_us([&] { hipLaunchKernelGGL(read_tiles, dim3(tiles), dim3(kWave), 0, nullptr, P, out); }, reps);
  printf("pure read of the tiles: %.1f us  (%.2f TB/s)\n", t_read, bytes / t_read / 1e6);
  for (int K : {1, 5, 10, 20}) {
    const unsigned chunks = spmm_chunks(K);
    const double t_pair = time_us([&] { launch_symm_packed(plan, P, Y, X, part, nullptr, K, nullptr); }, reps);
    const double t_tile = time_us([&] {
      hipLaunchKernelGGL(symm_packed_kernel, dim3(tiles, chunks), dim3(kSymmWaves * kWave), 0, nullptr, P, plan.n, plan.npad,
                         plan.ntile, Y, part, static_cast<const MultiRec*>(nullptr), K);
    }, reps);
    const double t_red = time_us([&] {
      hipLaunchKernelGGL(symm_reduce_kernel, dim3(ceil_div(plan.n * kSpmmChunk, kBlock), chunks), dim3(kBlock), 0,
                         nullptr, part, plan.n, plan.npad, plan.ntile, X, static_cast<const MultiRec*>(nullptr), K);
    }, reps);
    const double fma = 2.0 * pel * kSpmmChunk * chunks;  // both parts of every stored element, every lane of the chunk
    printf("K = %2d: pair %.1f us, tile pass %.1f us (%.2f TB/s of stored bytes per chunk, %.2f TFMA/s), sum %.1f us\n", K,
           t_pair, t_tile, bytes * chunks / t_tile / 1e6, fma / t_tile / 1e6, t_red);
  }
  const double t_symv = time_us([&] { launch_symv_lower(plan, P, 0, Y, np_, tp_, X, nullptr, nullptr); }, reps);
  printf("symv_lower (one vector, packed fp64, ncached %lld): %.1f us -> ten launches %.1f us\n",
         static_cast<long long>(plan.ncached), t_symv, 10.0 * t_symv);
  CK(hipDeviceSynchronize());
  return 0;
}
