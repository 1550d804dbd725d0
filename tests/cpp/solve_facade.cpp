// The solve through the C++ facade (include/cutfemx_amd.hpp): the cut Poisson system of poisson_facade.cpp assembled
// into HBM, deactivated, solved by cg_solve over all rows (host b / x), and y = A x by spmv; the system, the solution and
// the product are written for tests/test_gpu_solve.py to compare with scipy.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "cutfemx_amd.hpp"

namespace cfx = cutfemx_amd;

template <typename T>
static void dump(std::ofstream& f, const std::vector<T>& v)
{
  const std::int64_t n = static_cast<std::int64_t>(v.size());
  f.write(reinterpret_cast<const char*>(&n), sizeof(n));
  f.write(reinterpret_cast<const char*>(v.data()), sizeof(T) * v.size());
}

static double* device_doubles(std::size_t n)
{
  void* p = nullptr;
  if (cfx_device_alloc(&p, sizeof(double) * (n > 0 ? n : 1)) != CFX_OK) throw std::runtime_error(cfx_last_error());
  if (cfx_device_memset(p, 0, sizeof(double) * n) != CFX_OK) throw std::runtime_error(cfx_last_error());
  return static_cast<double*>(p);
}

int main(int argc, char** argv)
{
  const int tdim = argc > 1 ? std::atoi(argv[1]) : 3;
  const int n = argc > 2 ? std::atoi(argv[2]) : 8;
  const char* out_path = argc > 3 ? argv[3] : "solve_facade.bin";
  try
  {
    if (cfx_init(0) != CFX_OK) throw std::runtime_error(cfx_last_error());
    cfx::Mesh mesh = cfx::Mesh::create_box(tdim, n);
    const std::vector<double> x = mesh.x();
    const std::vector<std::int32_t> conn = mesh.connectivity();
    const double c[3] = {0.47, 0.43, 0.41};
    std::vector<double> phi(static_cast<std::size_t>(mesh.num_nodes));
    for (std::int64_t v = 0; v < mesh.num_nodes; ++v)
    {
      double r2 = 0.0;
      for (int d = 0; d < tdim; ++d) r2 += (x[3 * v + d] - c[d]) * (x[3 * v + d] - c[d]);
      phi[v] = std::sqrt(r2) - 0.31;
    }
    const double* values[1] = {phi.data()};
    cfx::CutData cd = cfx::cut(mesh, conn, tdim + 1, mesh.num_nodes, values);
    const std::vector<std::int32_t> inside = cfx::locate_entities(cd, "phi<0");
    cfx::RuntimeQuadrature vol = cfx::runtime_quadrature(cd, "phi<0", 4);
    cfx::RuntimeQuadrature itf = cfx::runtime_quadrature(cd, "phi=0", 4);
    const std::vector<double> normals = cfx::level_set::evaluate_normals(cd, 0, itf);
    const std::vector<std::int32_t> ghost = cfx::ghost_penalty_facets(cd, "phi<0");
    cfx::fem::FunctionSpace V = cfx::fem::FunctionSpace::create(mesh, 1, 1, mesh.num_nodes, conn, tdim + 1);
    std::vector<cfx::fem::Integral> ai(3), Li(2);
    ai[0] = {CFX_CELL, CFX_K_STIFFNESS, inside, &vol, {}, 0, {}, 0};
    ai[1] = {CFX_CELL, CFX_K_NITSCHE, {}, &itf, normals, tdim, {40.0}, 0};
    ai[2] = {CFX_INTERIOR_FACET, CFX_K_GHOST_GRADJUMP, ghost, nullptr, {}, 0, {0.1}, 0};
    Li[0] = {CFX_CELL, CFX_L_SOURCE, inside, &vol, {}, 0, {double(CFX_F_POISSON_RHS), 1.0}, 4};
    Li[1] = {CFX_CELL, CFX_L_NITSCHE_RHS, {}, &itf, normals, tdim, {40.0, double(CFX_F_SINPROD), 1.0}, 0};
    cfx::fem::Form a = cfx::fem::Form::create(V, 2, ai);
    cfx::fem::Form L = cfx::fem::Form::create(V, 1, Li);

    // the matrix values live in HBM; b and the solution are host vectors here
    cfx::fem::SparsityPattern sp = cfx::fem::create_sparsity_pattern(a);
    const std::size_t nnz = static_cast<std::size_t>(sp.num_nonzeros()), nd = static_cast<std::size_t>(mesh.num_nodes);
    double* A = device_doubles(nnz);
    std::vector<double> b(nd, 0.0), u(nd, 0.0);
    cfx::fem::assemble_matrix(std::span<double>(A, nnz), a, sp);
    cfx::fem::assemble_vector(b, L);
    cfx::fem::ActiveDomain dom = cfx::fem::active_domain(a);
    cfx::fem::deactivate_outside(std::span<double>(A, nnz), sp, b, dom);

    cfx::fem::CGOptions opt;
    opt.rtol = 1e-10;
    const cfx_cg_info info = cfx::fem::cg_solve(sp, A, b, u, opt);

    // y = A u in HBM
    double *ud = device_doubles(nd), *yd = device_doubles(nd);
    if (cfx_copy(ud, u.data(), sizeof(double) * nd) != CFX_OK) throw std::runtime_error(cfx_last_error());
    cfx::fem::spmv(sp, A, ud, yd);
    std::vector<double> y(nd), Ah(nnz);
    if (cfx_copy(y.data(), yd, sizeof(double) * nd) != CFX_OK) throw std::runtime_error(cfx_last_error());
    if (cfx_copy(Ah.data(), A, sizeof(double) * nnz) != CFX_OK) throw std::runtime_error(cfx_last_error());

    // a non-square call is refused
    bool threw = false;
    try { (void)cfx::fem::cg_solve(sp, A, std::span<const double>(b.data(), nd - 1), u, opt); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::invalid_argument for a short right-hand side");

    std::ofstream f(out_path, std::ios::binary);
    dump(f, sp.row_ptr());
    dump(f, sp.cols());
    dump(f, Ah);
    dump(f, b);
    dump(f, u);
    dump(f, y);
    dump(f, std::vector<double>{double(info.reason), double(info.iterations), info.residual_norm, info.rhs_norm});
    cfx_device_free(A); cfx_device_free(ud); cfx_device_free(yd);
    std::printf("solve facade ok: %lld rows, nnz %zu, reason %d after %d iterations\n", (long long)mesh.num_nodes, nnz,
                (int)info.reason, (int)info.iterations);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "solve facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
