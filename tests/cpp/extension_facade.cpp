// The normal extension through the C++ facade (include/cutfemx_amd.hpp): a mesh, a level set and an interface speed read
// from a file (int64 tdim, nnodes, ncells; x double [nnodes * 3]; connectivity int32; phi double; w double),
// distance::extend_normal_velocity on host spans, then once more with device pointers, the info left in HBM and no look
// of the host.  Writes speed, velocity and signed distance to the output file and prints the info for
// tests/test_gpu_cpp_extension.py to compare with the Python call's.
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

template <typename T>
static std::vector<T> from_hbm(const T* p, std::size_t n)
{
  std::vector<T> v(n);
  cfx::check(cfx_copy(v.data(), p, sizeof(T) * n));
  return v;
}

int main(int argc, char** argv)
{
  if (argc < 3)
  {
    std::cerr << "usage: extension_facade case.bin out.bin\n";
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
    const std::vector<double> phi = slurp<double>(f, nnodes);
    const std::vector<double> w = slurp<double>(f, nnodes);

    if (cfx_init(0) != CFX_OK) throw std::runtime_error(cfx_last_error());
    const cfx::Mesh mesh = cfx::Mesh::create(tdim, x, conn, tdim + 1);
    const std::int32_t* dev_conn = nullptr;
    cfx::check(cfx_mesh_info(mesh.handle.h, nullptr, nullptr, nullptr, nullptr, nullptr, &dev_conn));
    const cfx::fem::FunctionSpace V = cfx::fem::FunctionSpace::create(
        mesh, 1, 1, nnodes, std::span<const std::int32_t>(dev_conn, static_cast<std::size_t>(ncells * (tdim + 1))), tdim + 1);

    cfx::distance::ExtendOptions opt;
    const cfx::distance::ReinitOptions ropt;
    if (opt.max_iter != ropt.max_iter || opt.check_every != ropt.check_every || opt.tol != ropt.tol || opt.inf_value != ropt.inf_value ||
        opt.max_distance != ropt.max_distance || opt.normal_sign != 1.0)
      throw std::runtime_error("unexpected defaults");
    const std::vector<double> phi_before = phi;
    const cfx::distance::NormalExtensionResult r = cfx::distance::extend_normal_velocity(V, phi, w, opt);
    if (phi != phi_before) throw std::runtime_error("phi was changed");

    // device pointers, the info left in HBM, no look of the host, the velocity skipped: the same bits
    double* d_phi = to_hbm(phi);
    double* d_w = to_hbm(w);
    double* d_speed = to_hbm(std::vector<double>(phi.size(), -7.0));
    double* d_dist = to_hbm(std::vector<double>(phi.size(), -7.0));
    cfx_extend_info* d_info = to_hbm(std::vector<cfx_extend_info>(1));
    cfx::distance::ExtendOptions quiet = opt;
    quiet.check_every = 0;
    quiet.max_iter = r.info.sweeps + 5;
    std::int64_t syncs0 = 0, syncs1 = 0;
    cfx::check(cfx_sync_count(&syncs0));
    cfx::distance::extend_normal_velocity(V, d_phi, d_w, d_speed, nullptr, d_dist, quiet, d_info);
    cfx::check(cfx_sync_count(&syncs1));
    if (syncs1 != syncs0) throw std::runtime_error("the device-info call made a host round trip");
    const cfx_extend_info info2 = from_hbm(d_info, 1)[0];
    if (from_hbm(d_speed, phi.size()) != r.speed || from_hbm(d_dist, phi.size()) != r.signed_distance || from_hbm(d_phi, phi.size()) != phi ||
        info2.reason != r.info.reason || info2.sweeps != r.info.sweeps || info2.seeds != r.info.seeds || info2.updates != r.info.updates ||
        info2.transport_sweeps != r.info.transport_sweeps || info2.transported != r.info.transported)
      throw std::runtime_error("the device-info call differs from the host call");

    // a short interface speed is refused
    bool threw = false;
    try { (void)cfx::distance::extend_normal_velocity(V, phi, std::span<const double>(w.data(), w.size() - 1), opt); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::invalid_argument for a short interface speed");

    for (void* p : {(void*)d_phi, (void*)d_w, (void*)d_speed, (void*)d_dist, (void*)d_info}) cfx_device_free(p);
    std::ofstream o(argv[2], std::ios::binary);
    for (const std::vector<double>* a : {&r.speed, &r.velocity, &r.signed_distance})
      o.write(reinterpret_cast<const char*>(a->data()), sizeof(double) * a->size());
    if (!o) throw std::runtime_error("cannot write the output file");
    std::printf("extension facade: reason %d sweeps %d seeds %lld updates %lld transport_sweeps %d transported %lld\n", (int)r.info.reason,
                (int)r.info.sweeps, (long long)r.info.seeds, (long long)r.info.updates, (int)r.info.transport_sweeps,
                (long long)r.info.transported);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "extension facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
