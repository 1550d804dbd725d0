// BiCGStab through the C++ facade (include/cutfemx_amd.hpp): a small nonsymmetric CSR system read from a file
// (int64 nrows, nnz, n_rows; indptr int64; indices int32; values, b double; rows int32), copied into HBM and solved by
// fem::bicgstab_solve over the listed rows (host b / x), then once more with device vectors and the info left in HBM.  Prints
// the reason, the iterations and |x|_2 for tests/test_gpu_cpp_bicgstab.py to compare with the Python call's.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "cutfemx_amd.hpp"

namespace cfx = cutfemx_amd;

template <typename T>
static std::vector<T> slurp(std::ifstream& f, std::int64_t n)
{
  std::vector<T> v(static_cast<std::size_t>(n));
  f.read(reinterpret_cast<char*>(v.data()), sizeof(T) * v.size());
  if (!f) throw std::runtime_error("short input file");
  return v;
}

template <typename T>
static T* to_hbm(const std::vector<T>& v)
{
  void* p = nullptr;
  if (cfx_device_alloc(&p, sizeof(T) * (v.empty() ? 1 : v.size())) != CFX_OK) throw std::runtime_error(cfx_last_error());
  if (!v.empty() && cfx_copy(p, v.data(), sizeof(T) * v.size()) != CFX_OK) throw std::runtime_error(cfx_last_error());
  return static_cast<T*>(p);
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::cerr << "usage: bicgstab_facade system.bin [rtol]\n";
    return 2;
  }
  try
  {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the system file");
    const std::vector<std::int64_t> head = slurp<std::int64_t>(f, 3);
    const std::int64_t nrows = head[0], nnz = head[1], n_rows = head[2];
    const std::vector<std::int64_t> indptr = slurp<std::int64_t>(f, nrows + 1);
    const std::vector<std::int32_t> indices = slurp<std::int32_t>(f, nnz);
    const std::vector<double> values = slurp<double>(f, nnz), b = slurp<double>(f, nrows);
    const std::vector<std::int32_t> rows = slurp<std::int32_t>(f, n_rows);

    if (cfx_init(0) != CFX_OK) throw std::runtime_error(cfx_last_error());
    std::int64_t* d_indptr = to_hbm(indptr);
    std::int32_t* d_indices = to_hbm(indices);
    double* d_values = to_hbm(values);
    std::int32_t* d_rows = to_hbm(rows);
    cfx::fem::SparsityPattern sp; // (a caller's arrays: no pattern handle behind the view)
    sp.view.nrows = nrows;
    sp.view.ncols = nrows;
    sp.view.nnz = nnz;
    sp.view.indptr = d_indptr;
    sp.view.indices = d_indices;

    cfx::fem::BicgstabOptions opt;
    if (opt.precond != CFX_PC_JACOBI || opt.check_every != 16) throw std::runtime_error("unexpected defaults");
    opt.rtol = argc > 2 ? std::atof(argv[2]) : 1e-10;
    std::vector<double> x(static_cast<std::size_t>(nrows), 0.0);
    const cfx_cg_info info = cfx::fem::bicgstab_solve(sp, d_values, b, x, opt, d_rows, n_rows);
    double s = 0.0;
    for (double v : x) s += v * v;

    // device vectors, the info left in HBM, no look of the host: the same bits
    double* d_b = to_hbm(b);
    double* d_x = to_hbm(std::vector<double>(static_cast<std::size_t>(nrows), 0.0));
    cfx_cg_info* d_info = to_hbm(std::vector<cfx_cg_info>(1));
    cfx::fem::BicgstabOptions quiet = opt;
    quiet.check_every = 0;
    quiet.max_iter = info.iterations + 40;
    cfx::fem::bicgstab_solve(sp, d_values, d_b, d_x, quiet, d_info, d_rows, n_rows);
    std::vector<double> x2(x.size());
    cfx_cg_info info2{};
    if (cfx_copy(x2.data(), d_x, sizeof(double) * x2.size()) != CFX_OK) throw std::runtime_error(cfx_last_error());
    if (cfx_copy(&info2, d_info, sizeof(info2)) != CFX_OK) throw std::runtime_error(cfx_last_error());
    if (x2 != x || info2.reason != info.reason || info2.iterations != info.iterations || info2.residual_norm != info.residual_norm)
      throw std::runtime_error("the device-info call differs from the host call");

    // a short right-hand side is refused
    bool threw = false;
    try { (void)cfx::fem::bicgstab_solve(sp, d_values, std::span<const double>(b.data(), b.size() - 1), x, opt); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::invalid_argument for a short right-hand side");

    for (void* p : {(void*)d_indptr, (void*)d_indices, (void*)d_values, (void*)d_rows, (void*)d_b, (void*)d_x, (void*)d_info})
      cfx_device_free(p);
    std::printf("bicgstab facade: reason %d iterations %d xnorm %.17g residual %.17g rhs %.17g\n", (int)info.reason,
                (int)info.iterations, std::sqrt(s), info.residual_norm, info.rhs_norm);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "bicgstab facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
