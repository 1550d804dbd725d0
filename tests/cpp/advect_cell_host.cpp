// The arithmetic of one cell visit of the characteristic walk (cutfemx_amd/csrc/cfx_advect_cell.h) on the CPU: the header
// compiled as plain host C++, no HIP and no GPU, with its own main (tests/test_advect_cell_reference.py builds it with the
// address and undefined-behaviour sanitizers).
//   usage: advect_cell_host IN OUT
//   IN   int64 dim, n; double inside_tol; X double [n][dim + 1][dim]; P double [n][dim] (the targets); F double [n][dim + 1]
//   OUT  lam double [n][dim + 1]; value double [n] (interpolate); D double [n][dim] (depart(P, 0.375, X[1])); facet int32 [n]
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../cutfemx_amd/csrc/cfx_advect_cell.h"

namespace
{
template <typename T>
std::vector<T> get(FILE* f, int64_t n)
{
  std::vector<T> v((size_t)n);
  if (n > 0 && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) throw std::runtime_error("short input file");
  return v;
}

template <typename T>
void put(FILE* f, const std::vector<T>& v)
{
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("cannot write the output file");
}

template <int TDIM>
void run(FILE* in, FILE* out, int64_t n, double tol)
{
  constexpr int NV = TDIM + 1;
  const auto X = get<double>(in, n * NV * TDIM), P = get<double>(in, n * TDIM), F = get<double>(in, n * NV);
  std::vector<double> lam((size_t)(n * NV)), value((size_t)n), D((size_t)(n * TDIM));
  std::vector<int32_t> facet((size_t)n);
  for (int64_t i = 0; i < n; ++i)
  {
    double x[NV][TDIM];
    for (int s = 0; s < NV; ++s)
      for (int k = 0; k < TDIM; ++k) x[s][k] = X[(i * NV + s) * TDIM + k];
    facet[i] = cfx::advect::visit<TDIM>(x, &P[i * TDIM], tol, &lam[i * NV]);
    value[i] = cfx::advect::interpolate<TDIM>(&lam[i * NV], &F[i * NV]);
    cfx::advect::depart<TDIM>(&P[i * TDIM], 0.375, x[1], &D[i * TDIM]);
  }
  put(out, lam);
  put(out, value);
  put(out, D);
  put(out, facet);
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: advect_cell_host IN OUT\n");
    return 1;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int status = 0;
  try
  {
    if (!in || !out) throw std::runtime_error("cannot open the files");
    const auto head = get<int64_t>(in, 2);
    const double tol = get<double>(in, 1)[0];
    if (head[0] == 2)
      run<2>(in, out, head[1], tol);
    else if (head[0] == 3)
      run<3>(in, out, head[1], tol);
    else
      throw std::runtime_error("dim is 2 or 3");
  }
  catch (const std::exception& e)
  {
    fprintf(stderr, "advect_cell_host: %s\n", e.what());
    status = 2;
  }
  if (in) fclose(in);
  if (out) fclose(out);
  return status;
}
