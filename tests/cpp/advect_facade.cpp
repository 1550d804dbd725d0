// The advection through the C++ facade (include/cutfemx_amd.hpp): a mesh, a level set, a velocity and a time step read from
// a file (int64 tdim, nnodes, ncells; double dt; x double [nnodes * 3]; connectivity int32; phi double [nnodes]; velocity
// double [nnodes * tdim]), distance::advect on host spans, then once more with device pointers, into a second array, with
// the cells and the info left in HBM.  Writes the new phi to the output file and prints the info for
// tests/test_gpu_cpp_advect.py to compare with the Python call's.
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
    std::cerr << "usage: advect_facade case.bin out.bin\n";
    return 2;
  }
  try
  {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the case file");
    const std::vector<std::int64_t> head = slurp<std::int64_t>(f, 3);
    const int tdim = static_cast<int>(head[0]);
    const std::int64_t nnodes = head[1], ncells = head[2];
    const double dt = slurp<double>(f, 1)[0];
    const std::vector<double> x = slurp<double>(f, 3 * nnodes);
    const std::vector<std::int32_t> conn = slurp<std::int32_t>(f, ncells * (tdim + 1));
    const std::vector<double> phi = slurp<double>(f, nnodes);
    const std::vector<double> velocity = slurp<double>(f, nnodes * tdim);

    if (cfx_init(0) != CFX_OK) throw std::runtime_error(cfx_last_error());
    const cfx::Mesh mesh = cfx::Mesh::create(tdim, x, conn, tdim + 1);
    const std::int32_t* dev_conn = nullptr;
    cfx::check(cfx_mesh_info(mesh.handle.h, nullptr, nullptr, nullptr, nullptr, nullptr, &dev_conn));
    const cfx::fem::FunctionSpace V = cfx::fem::FunctionSpace::create(
        mesh, 1, 1, nnodes, std::span<const std::int32_t>(dev_conn, static_cast<std::size_t>(ncells * (tdim + 1))), tdim + 1);

    const cfx::distance::AdvectOptions opt;
    if (opt.order != 2 || opt.max_steps != 4096 || opt.inside_tol != 1e-12 || opt.max_distance != 0.0 || opt.dt != 0.0)
      throw std::runtime_error("unexpected defaults");
    std::vector<double> moved = phi;
    const cfx_advect_info info = cfx::distance::advect(V, moved, velocity, dt, opt);

    // device pointers, into a second array, the cells and the info left in HBM: the same bits and no host round trip
    double* d_phi = to_hbm(phi);
    double* d_vel = to_hbm(velocity);
    double* d_out = to_hbm(std::vector<double>(phi.size(), -7.0));
    std::int32_t* d_cells = to_hbm(std::vector<std::int32_t>(phi.size(), -7));
    cfx_advect_info* d_info = to_hbm(std::vector<cfx_advect_info>(1));
    std::int64_t syncs0 = 0, syncs1 = 0;
    cfx::check(cfx_sync_count(&syncs0));
    cfx::distance::advect(V, d_phi, d_vel, d_out, d_cells, dt, opt, d_info);
    cfx::check(cfx_sync_count(&syncs1));
    if (syncs1 != syncs0) throw std::runtime_error("the device-info call made a host round trip");
    const cfx_advect_info info2 = from_hbm(d_info, 1)[0];
    if (from_hbm(d_out, phi.size()) != moved || from_hbm(d_phi, phi.size()) != phi || info2.located != info.located ||
        info2.outside != info.outside || info2.capped != info.capped || info2.skipped != info.skipped || info2.steps != info.steps ||
        info2.max_walk != info.max_walk)
      throw std::runtime_error("the device call differs from the host call");
    const std::vector<std::int32_t> cells = from_hbm(d_cells, phi.size());
    std::int64_t in_a_cell = 0;
    for (std::int32_t c : cells)
    {
      if (c < -1 || c >= ncells) throw std::runtime_error("a cell index out of range");
      in_a_cell += c >= 0 ? 1 : 0;
    }
    if (in_a_cell != info.located + info.outside) throw std::runtime_error("cells and info disagree");

    // the read-only table the walk crosses facets with
    const std::int32_t* nbr = nullptr;
    cfx::check(cfx_mesh_cell_neighbours(mesh.handle.h, &nbr));
    std::int64_t boundary = 0;
    for (std::int32_t c : from_hbm(nbr, static_cast<std::size_t>(ncells * (tdim + 1)))) boundary += c < 0 ? 1 : 0;

    // a short velocity is refused
    bool threw = false;
    try { (void)cfx::distance::advect(V, moved, std::span<const double>(velocity.data(), velocity.size() - 1), dt, opt); }
    catch (const std::invalid_argument&) { threw = true; }
    if (!threw) throw std::runtime_error("expected std::invalid_argument for a short velocity");

    for (void* p : {(void*)d_phi, (void*)d_vel, (void*)d_out, (void*)d_cells, (void*)d_info}) cfx_device_free(p);
    std::ofstream o(argv[2], std::ios::binary);
    o.write(reinterpret_cast<const char*>(moved.data()), sizeof(double) * moved.size());
    if (!o) throw std::runtime_error("cannot write the output file");
    std::printf("advect facade: located %lld outside %lld capped %lld skipped %lld steps %lld max_walk %d boundary %lld\n",
                (long long)info.located, (long long)info.outside, (long long)info.capped, (long long)info.skipped, (long long)info.steps,
                (int)info.max_walk, (long long)boundary);
    return 0;
  }
  catch (const std::exception& e)
  {
    std::cerr << "advect facade FAILED: " << e.what() << "\n";
    return 1;
  }
}
