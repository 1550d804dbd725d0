// The cell-local arithmetic of the reinitialisation (cutfemx_amd/csrc/cfx_reinit_cell.h) on the GPU, one lane per case
// (tests/test_gpu_reinit_cell.py): the header's functions and nothing else of the engine.  Cases and files:
// reinit_cell_io.h.  A case set that throws (a HIP error included) is named on stderr, and the probe exits with status
// 2 without running the ones behind it.
#include <hip/hip_runtime.h>

#include "../../cutfemx_amd/csrc/cfx_reinit_cell.h"
#include "reinit_cell_io.h"

using namespace cellio;

namespace
{
constexpr int kLanes = 256;

void check(hipError_t e, const char* what)
{
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T>
struct Dev
{
  T* p = nullptr;
  size_t n = 0;
  explicit Dev(size_t count) : n(count) { check(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * (n ? n : 1)), "hipMalloc"); }
  explicit Dev(const std::vector<T>& h) : Dev(h.size())
  {
    if (n) check(hipMemcpy(p, h.data(), sizeof(T) * n, hipMemcpyHostToDevice), "hipMemcpy to the device");
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() { (void)hipFree(p); }
  std::vector<T> fetch() const
  {
    std::vector<T> h(n);
    check(hipDeviceSynchronize(), "kernel");
    if (n) check(hipMemcpy(h.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost), "hipMemcpy to the host");
    return h;
  }
};

template <int TDIM>
__global__ void __launch_bounds__(kLanes) update_kernel(const double* __restrict__ P, const double* __restrict__ dv,
                                                        const uint8_t* __restrict__ okb, double inf, int64_t n, double* __restrict__ U)
{
  const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  double p[TDIM][TDIM], d[TDIM];
  bool ok[TDIM];
#pragma unroll
  for (int s = 0; s < TDIM; ++s)
  {
    ok[s] = okb[i * TDIM + s] != 0;
    d[s] = dv[i * TDIM + s];
#pragma unroll
    for (int k = 0; k < TDIM; ++k) p[s][k] = P[(i * TDIM + s) * TDIM + k];
  }
  U[i] = cfx::reinit::cell_update<TDIM>(p, d, ok, inf);
}

template <int TDIM>
__global__ void __launch_bounds__(kLanes) seed_kernel(const double* __restrict__ X, const double* __restrict__ f, int64_t n,
                                                      uint8_t* __restrict__ flag, double* __restrict__ dist)
{
  constexpr int NV = TDIM + 1;
  const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (i >= n) return;
  double x[NV][TDIM], fv[NV], out[NV];
#pragma unroll
  for (int s = 0; s < NV; ++s)
  {
    fv[s] = f[i * NV + s];
    out[s] = -1.0;
#pragma unroll
    for (int k = 0; k < TDIM; ++k) x[s][k] = X[(i * NV + s) * TDIM + k];
  }
  flag[i] = cfx::reinit::seed_cell<TDIM>(x, fv, out) ? 1 : 0;
#pragma unroll
  for (int s = 0; s < NV; ++s) dist[i * NV + s] = out[s];
}

unsigned blocks(int64_t n) { return (unsigned)((n + kLanes - 1) / kLanes); }

template <int TDIM>
void run_update(const Case& c)
{
  const int64_t n = c.num("n");
  Dev<double> P(read_file<double>(c.path("P", ".bin"), n * TDIM * TDIM)), dv(read_file<double>(c.path("dv", ".bin"), n * TDIM));
  Dev<uint8_t> ok(read_file<uint8_t>(c.path("ok", ".bin"), n * TDIM));
  Dev<double> U((size_t)n);
  if (n > 0)
  {
    hipLaunchKernelGGL(update_kernel<TDIM>, dim3(blocks(n)), dim3(kLanes), 0, 0, P.p, dv.p, ok.p, c.real("inf"), n, U.p);
    check(hipGetLastError(), "launch");
  }
  write_file(c.path("U", ".out"), U.fetch());
}

template <int TDIM>
void run_seed(const Case& c)
{
  constexpr int NV = TDIM + 1;
  const int64_t n = c.num("n");
  Dev<double> X(read_file<double>(c.path("X", ".bin"), n * NV * TDIM)), f(read_file<double>(c.path("f", ".bin"), n * NV));
  Dev<uint8_t> flag((size_t)n);
  Dev<double> dist((size_t)(n * NV));
  if (n > 0)
  {
    hipLaunchKernelGGL(seed_kernel<TDIM>, dim3(blocks(n)), dim3(kLanes), 0, 0, X.p, f.p, n, flag.p, dist.p);
    check(hipGetLastError(), "launch");
  }
  write_file(c.path("flag", ".out"), flag.fetch());
  write_file(c.path("dist", ".out"), dist.fetch());
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    fprintf(stderr, "usage: reinit_cell_probe DIR\n");
    return 1;
  }
  std::string at = "manifest";
  try
  {
    for (const Case& c : manifest(argv[1]))
    {
      at = c.name;
      const int tdim = tdim_of(c);
      if (c.kind[0] == 'u')
        tdim == 2 ? run_update<2>(c) : run_update<3>(c);
      else
        tdim == 2 ? run_seed<2>(c) : run_seed<3>(c);
    }
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "reinit_cell_probe: %s: %s\n", at.c_str(), e.what());
    return 2;
  }
  return 0;
}
