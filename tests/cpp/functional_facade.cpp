// A functional through the C++ facade (include/cutfemx_amd.hpp): the volume of {phi < 0} for the sphere level set of
// poisson_facade.cpp by assemble_scalar(Form) -- once to the host, once into HBM -- printed for
// tests/test_gpu_functionals.py to compare with the Python value.
#include <cmath>
#include <cstdio>
#include <iostream>

#include "cutfemx_amd.hpp"

namespace cfx = cutfemx_amd;

int main(int argc, char** argv)
{
  const int tdim = argc > 1 ? std::atoi(argv[1]) : 3;
  const int n = argc > 2 ? std::atoi(argv[2]) : 8;
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
    cfx::fem::FunctionSpace V = cfx::fem::FunctionSpace::create(mesh, 1, 1, mesh.num_nodes, conn, tdim + 1);
    std::vector<cfx::fem::Integral> mi(1);
    mi[0] = {CFX_CELL, CFX_M_FIELD, inside, &vol, {}, 0, {double(CFX_F_ONE), 1.0}, 1};
    cfx::fem::Form M = cfx::fem::Form::create(V, 0, mi);
    const double value = cfx::fem::assemble_scalar(M);

    // ... and into one double in HBM
    void* dev = nullptr;
    if (cfx_device_alloc(&dev, sizeof(double)) != CFX_OK) throw std::runtime_error(cfx_last_error());
    cfx::fem::assemble_scalar(M, static_cast<double*>(dev));
    double from_device = -1.0;
    if (cfx_copy(&from_device, dev, sizeof(double)) != CFX_OK) throw std::runtime_error(cfx_last_error());
    cfx_device_free(dev);

    // a functional is refused where rows are needed
    bool threw = false;
    try { (void)cfx::fem::create_sparsity_pattern(M); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::runtime_error for the sparsity of a rank-0 form");
    std::printf("functional ok: %zu inside, %zu cut rules\n%.17g %.17g\n", inside.size(), vol.num_rules(), value, from_device);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "functional facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
