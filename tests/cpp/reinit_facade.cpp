// Reinitialisation through the C++ facade (include/cutfemx_amd.hpp): a mesh and a level set read from a file (int64 tdim,
// nnodes, ncells; x double [nnodes * 3]; connectivity int32; phi double), distance::reinitialize on a host span, then once
// more with a device pointer, the info left in HBM and no look of the host.  Writes the new phi to the output file and
// prints the info for tests/test_gpu_cpp_reinit.py to compare with the Python call's.
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
  if (argc < 3)
  {
    std::cerr << "usage: reinit_facade case.bin out.bin [max_distance]\n";
    return 2;
  }
  try
  {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the case file");
    const std::vector<std::int64_t> head = slurp<std::int64_t>(f, 3);
    const int tdim = static_cast<int>(head[0]);
    const std::int64_t nnodes = head[1], ncells = head[2];
    const std::vector<double> x = slurp<double>(f, 3 * nnodes);
    const std::vector<std::int32_t> conn = slurp<std::int32_t>(f, ncells * (tdim + 1));
    const std::vector<double> phi0 = slurp<double>(f, nnodes);

    if (cfx_init(0) != CFX_OK) throw std::runtime_error(cfx_last_error());
    const cfx::Mesh mesh = cfx::Mesh::create(tdim, x, conn, tdim + 1);
    // the P1 space on the geometry dofmap: the mesh's own connectivity, as it lies in HBM
    const std::int32_t* dev_conn = nullptr;
    cfx::check(cfx_mesh_info(mesh.handle.h, nullptr, nullptr, nullptr, nullptr, nullptr, &dev_conn));
    const cfx::fem::FunctionSpace V = cfx::fem::FunctionSpace::create(
        mesh, 1, 1, nnodes, std::span<const std::int32_t>(dev_conn, static_cast<std::size_t>(ncells * (tdim + 1))), tdim + 1);

    cfx::distance::ReinitOptions opt;
    if (opt.max_iter != 1000 || opt.check_every != 8 || opt.tol != 1e-10 || opt.inf_value != 1e30 || opt.max_distance != 0.0)
      throw std::runtime_error("unexpected defaults");
    if (argc > 3) opt.max_distance = std::atof(argv[3]);
    std::vector<double> phi = phi0;
    const cfx_reinit_info info = cfx::distance::reinitialize(V, phi, opt);

    // a device pointer, the info left in HBM, no look of the host: the same bits
    double* d_phi = to_hbm(phi0);
    cfx_reinit_info* d_info = to_hbm(std::vector<cfx_reinit_info>(1));
    cfx::distance::ReinitOptions quiet = opt;
    quiet.check_every = 0;
    quiet.max_iter = info.sweeps + 5;
    std::int64_t syncs0 = 0, syncs1 = 0;
    cfx::check(cfx_sync_count(&syncs0));
    cfx::distance::reinitialize(V, d_phi, quiet, d_info);
    cfx::check(cfx_sync_count(&syncs1));
    if (syncs1 != syncs0) throw std::runtime_error("the device-info call made a host round trip");
    std::vector<double> phi2(phi.size());
    cfx_reinit_info info2{};
    cfx::check(cfx_copy(phi2.data(), d_phi, sizeof(double) * phi2.size()));
    cfx::check(cfx_copy(&info2, d_info, sizeof(info2)));
    if (phi2 != phi || info2.reason != info.reason || info2.sweeps != info.sweeps || info2.seeds != info.seeds ||
        info2.updates != info.updates)
      throw std::runtime_error("the device-info call differs from the host call");

    // a short phi is refused
    bool threw = false;
    try { (void)cfx::distance::reinitialize(V, std::span<double>(phi.data(), phi.size() - 1), opt); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::invalid_argument for a short phi");

    cfx_device_free(d_phi);
    cfx_device_free(d_info);
    std::ofstream o(argv[2], std::ios::binary);
    o.write(reinterpret_cast<const char*>(phi.data()), sizeof(double) * phi.size());
    if (!o) throw std::runtime_error("cannot write the output file");
    std::printf("reinit facade: reason %d sweeps %d seeds %lld updates %lld\n", (int)info.reason, (int)info.sweeps,
                (long long)info.seeds, (long long)info.updates);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "reinit facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
