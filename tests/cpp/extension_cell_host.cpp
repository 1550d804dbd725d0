// The cell-local arithmetic of the normal extension (cell_update_argmin and seed_closest of
// cutfemx_amd/csrc/cfx_reinit_cell.h) on the CPU: the header compiled as plain host C++, no HIP and no GPU
// (tests/test_extension_cell_reference.py).  Manifest and input files: reinit_cell_io.h.  Beside the outputs named there
//   update2 / update3   U [n] is cell_update_argmin's (limit -infinity: the first sub-face that attains U is reported), and
//                       Uref [n] (cell_update), value [n], lam [n][TDIM]
//   seed2 / seed3       dist [n][NV] is seed_closest's, flag [n] seed_cell's, and dref [n][NV] (seed_cell), clam [n][NV][NV]
//                       (the weights of the cell's vertices for the point closest to each vertex in turn)
// A case set that throws is named on stderr, and the program exits with status 2 without running the ones behind it.
#include "../../cutfemx_amd/csrc/cfx_reinit_cell.h"
#include "reinit_cell_io.h"

using namespace cellio;

namespace
{
template <int TDIM>
void run_update(const Case& c)
{
  const int64_t n = c.num("n");
  const double inf = c.real("inf");
  const auto P = read_file<double>(c.path("P", ".bin"), n * TDIM * TDIM);
  const auto dv = read_file<double>(c.path("dv", ".bin"), n * TDIM);
  const auto okb = read_file<uint8_t>(c.path("ok", ".bin"), n * TDIM);
  std::vector<double> U((size_t)n), Uref((size_t)n), value((size_t)n), lam((size_t)(n * TDIM));
  for (int64_t i = 0; i < n; ++i)
  {
    double p[TDIM][TDIM];
    bool ok[TDIM];
    for (int s = 0; s < TDIM; ++s)
    {
      ok[s] = okb[i * TDIM + s] != 0;
      for (int k = 0; k < TDIM; ++k) p[s][k] = P[(i * TDIM + s) * TDIM + k];
    }
    Uref[i] = cfx::reinit::cell_update<TDIM>(p, &dv[i * TDIM], ok, inf);
    U[i] = cfx::reinit::cell_update_argmin<TDIM>(p, &dv[i * TDIM], ok, inf, -HUGE_VAL, value[i], &lam[i * TDIM]);
  }
  write_file(c.path("U", ".out"), U);
  write_file(c.path("Uref", ".out"), Uref);
  write_file(c.path("value", ".out"), value);
  write_file(c.path("lam", ".out"), lam);
}

template <int TDIM>
void run_seed(const Case& c)
{
  constexpr int NV = TDIM + 1;
  const int64_t n = c.num("n");
  const auto X = read_file<double>(c.path("X", ".bin"), n * NV * TDIM);
  const auto f = read_file<double>(c.path("f", ".bin"), n * NV);
  std::vector<double> dist((size_t)(n * NV), -1.0), dref((size_t)(n * NV), -1.0), clam((size_t)(n * NV * NV), 0.0);
  std::vector<uint8_t> flag((size_t)n);
  for (int64_t i = 0; i < n; ++i)
  {
    double x[NV][TDIM];
    for (int s = 0; s < NV; ++s)
      for (int k = 0; k < TDIM; ++k) x[s][k] = X[(i * NV + s) * TDIM + k];
    flag[i] = cfx::reinit::seed_cell<TDIM>(x, &f[i * NV], &dref[i * NV]) ? 1 : 0;
    for (int at = 0; at < NV; ++at) dist[i * NV + at] = cfx::reinit::seed_closest<TDIM>(x, &f[i * NV], at, &clam[(i * NV + at) * NV]);
  }
  write_file(c.path("flag", ".out"), flag);
  write_file(c.path("dist", ".out"), dist);
  write_file(c.path("dref", ".out"), dref);
  write_file(c.path("clam", ".out"), clam);
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    fprintf(stderr, "usage: extension_cell_host DIR\n");
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
    fprintf(stderr, "extension_cell_host: %s: %s\n", at.c_str(), e.what());
    return 2;
  }
  return 0;
}
