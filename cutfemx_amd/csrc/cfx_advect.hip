// cutfemx_amd: semi-Lagrangian advection of a P1 level set along a P1 velocity, in HBM -- the "move phi" stage of a
// moving-domain loop, between the normal extension (cfx_extend.hip) and the reinitialisation (cfx_reinit.hip).
//
// Answers _advect_level_set_characteristics of the reference's demo (python/demo/demo_compliance_optimization.py:2071-2095:
// midpoint rule, bounding-box tree, compute_colliding_cells, Function.eval on the host).  Here the departure points are
// located by a visibility walk through the mesh's cell -> cell table (cfx_mesh_s::cell_neighbours), one lane per vertex.
//
// Contract (include/cutfemx_amd.h has the full text):
//   skipped    band B > 0 and |phi_v| > B: out_v = phi_v
//   departure  order 2: x_half = x_v - dt/2 velocity_v, v_mid = (P1 velocity)(x_half), x_dep = x_v - dt v_mid;
//              order 1: x_dep = x_v - dt velocity_v.  x_half == x_v bit for bit: v_mid = velocity_v, no walk.
//              x_dep == x_v bit for bit: out_v = phi_v, located, a walk of 0 (a fixed dof)
//   location   from the lowest cell around v: lambda of the target (cfx_advect_cell.h); every lambda >= -inside_tol: found;
//              else across the facet opposite the most negative lambda (lowest index on ties); a boundary facet: outside,
//              the walk ends in that cell; more than max_steps crossings or a target that is not finite: capped, out_v = phi_v
//   value      sum lambda_i phi_i in the final cell with the unclamped lambda (outside: that cell's P1 extension)
//
// One launch, advect_walk: each vertex is one independent lane that reads only old arrays, so two calls give the same bits
// and there is no floating-point atomic.  The band test comes first (a skipped vertex reads its 8 bytes).  A crossing is a
// chain of two dependent gathers: the connectivity and the neighbour row of the next cell (one 16 B load each in 3-D,
// issued together as soon as the facet is chosen), then the coordinates of its vertices; phi or the velocity is gathered in
// the final cell only.  The counters are kept in registers over a grid-stride loop, joined in the block, and added by one lane
// per counter: a few thousand integer atomics per call.
#include <cfloat>

#include "cfx_advect_cell.h"
#include "cfx_device.h"
#include "cfx_reinit.h"

using namespace cfx;

namespace
{
enum : int { kNone = 0, kLocated = 1, kOutside = 2, kCapped = 3, kSkipped = 4 };

struct AdvectArgs
{
  const double* x;
  const int32_t* conn;
  const int32_t* nbr;   // [ncells][TDIM + 1] the cell across the facet opposite local vertex i, -1 on the boundary
  const int64_t* voff;
  const int32_t* vcells;
  int64_t nv;
  const double* phi;
  const double* vel;    // [nv][TDIM]
  double* out;          // never phi itself (the driver gives a workspace then)
  int32_t* cells;       // or null
  cfx_advect_info* info;
  double dt, half_dt, band, tol;
  int order, max_steps;
};

template <int TDIM>
struct Cell
{
  int32_t id;
  int32_t row[TDIM + 1], nb[TDIM + 1];
};

template <int TDIM>
__device__ __forceinline__ void load_cell(const AdvectArgs& A, int32_t c, Cell<TDIM>& K)
{
  K.id = c;
  if constexpr (TDIM == 3)
  {
    const int4 r = *reinterpret_cast<const int4*>(A.conn + (int64_t)c * 4);
    const int4 n = *reinterpret_cast<const int4*>(A.nbr + (int64_t)c * 4);
    K.row[0] = r.x; K.row[1] = r.y; K.row[2] = r.z; K.row[3] = r.w;
    K.nb[0] = n.x; K.nb[1] = n.y; K.nb[2] = n.z; K.nb[3] = n.w;
  }
  else
  {
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      K.row[i] = A.conn[(int64_t)c * 3 + i];
      K.nb[i] = A.nbr[(int64_t)c * 3 + i];
    }
  }
}

template <int TDIM>
__device__ __forceinline__ bool finite_point(const double* p)
{
  bool ok = true;
#pragma unroll
  for (int k = 0; k < TDIM; ++k) ok = ok && (fabs(p[k]) <= DBL_MAX); // (false for a NaN)
  return ok;
}

template <int TDIM>
__device__ __forceinline__ bool same_point(const double* p, const double* q)
{
  bool same = true;
#pragma unroll
  for (int k = 0; k < TDIM; ++k) same = same && __double_as_longlong(p[k]) == __double_as_longlong(q[k]);
  return same;
}

// the walk to p from the cell K (its rows loaded): K becomes the final cell, lam the coordinates of p there
template <int TDIM>
__device__ __forceinline__ int walk(const AdvectArgs& A, const double* p, Cell<TDIM>& K, double* lam, int& steps)
{
  constexpr int NV = TDIM + 1;
  for (;;)
  {
    double X[NV][TDIM];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < TDIM; ++k) X[i][k] = A.x[3 * (int64_t)K.row[i] + k];
    const int facet = advect::visit<TDIM>(X, p, A.tol, lam);
    if (facet < 0) return kLocated;
    int32_t next = K.nb[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) next = facet == i ? K.nb[i] : next;
    if (next < 0) return kOutside;
    if (steps >= A.max_steps) return kCapped;
    ++steps;
    load_cell<TDIM>(A, next, K);
  }
}

// one vertex: its new value and final cell written, its status returned, its crossings added to steps
template <int TDIM>
__device__ __forceinline__ int advect_vertex(const AdvectArgs& A, int64_t v, int& steps)
{
  constexpr int NV = TDIM + 1;
  int status = kNone;
  const double f = A.phi[v];
  double result = f;
  int32_t where = -1;
  if (A.band > 0.0 && fabs(f) > A.band)
    status = kSkipped;
  else
  {
    const int64_t j0 = A.voff[v], j1 = A.voff[v + 1];
    double xv[TDIM], w[TDIM];
#pragma unroll
    for (int k = 0; k < TDIM; ++k)
    {
      xv[k] = A.x[3 * v + k];
      w[k] = A.vel[v * TDIM + k];
    }
    if (j0 == j1)
      status = kOutside; // a vertex of no cell has nowhere to look
    else
    {
      const int32_t c0 = A.vcells[j0];
      Cell<TDIM> K;
      double lam[NV], p[TDIM];
      bool loaded = false;
      status = kLocated;
      if (A.order == 2)
      {
        advect::depart<TDIM>(xv, A.half_dt, w, p);
        if (!same_point<TDIM>(p, xv))
        {
          if (!finite_point<TDIM>(p))
            status = kCapped;
          else
          {
            load_cell<TDIM>(A, c0, K);
            loaded = true;
            if (walk<TDIM>(A, p, K, lam, steps) == kCapped)
              status = kCapped;
            else
            {
#pragma unroll
              for (int k = 0; k < TDIM; ++k)
              {
                double g[NV];
#pragma unroll
                for (int i = 0; i < NV; ++i) g[i] = A.vel[(int64_t)K.row[i] * TDIM + k];
                w[k] = advect::interpolate<TDIM>(lam, g);
              }
            }
          }
        }
      }
      if (status != kCapped)
      {
        advect::depart<TDIM>(xv, A.dt, w, p);
        if (same_point<TDIM>(p, xv))
          where = c0; // a fixed dof: phi_v as it stands
        else if (!finite_point<TDIM>(p))
          status = kCapped;
        else
        {
          if (!loaded) load_cell<TDIM>(A, c0, K);
          status = walk<TDIM>(A, p, K, lam, steps);
          if (status != kCapped)
          {
            double g[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) g[i] = A.phi[K.row[i]];
            result = advect::interpolate<TDIM>(lam, g);
            where = K.id;
          }
        }
      }
    }
  }
  A.out[v] = result;
  if (A.cells) A.cells[v] = where;
  return status;
}

constexpr int kMaxGrid = 2560; // blocks: two rounds of the 1280 that are resident in 3-D (5 waves per SIMD); a block ends with at most six atomics

// Grid-stride over the vertices (a block's 256 lanes take 256 consecutive vertices at a time, so the streams coalesce and
// every block sees every part of the mesh); the counters stay in registers, are joined in the wavefront by shuffles and in
// the block through LDS, and one lane per counter adds what is not zero.  (Atomics of every wavefront on the same few words
// serialise in L2: with 2.1 M wavefronts at 512^3 that form took 76.0 ms unbanded and 32.5 ms with 98 % of the vertices
// skipped, this one 22.9 and 1.54 ms.)
template <int TDIM>
__global__ void __launch_bounds__(kBlock) advect_walk_kernel(AdvectArgs A)
{
  int count[4] = {0, 0, 0, 0}, longest = 0; // located, outside, capped, skipped (a lane sees at most 2^31 / 2^19 vertices)
  long long crossings = 0;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < A.nv; v += (int64_t)gridDim.x * kBlock)
  {
    int steps = 0;
    const int status = advect_vertex<TDIM>(A, v, steps);
    count[0] += status == kLocated;
    count[1] += status == kOutside;
    count[2] += status == kCapped;
    count[3] += status == kSkipped;
    crossings += steps;
    longest = max(longest, steps);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
#pragma unroll
    for (int q = 0; q < 4; ++q) count[q] += __shfl_xor(count[q], o, 64);
    crossings += __shfl_xor(crossings, o, 64);
    longest = max(longest, __shfl_xor(longest, o, 64));
  }
  __shared__ long long s_count[kBlock / 64][6];
  if ((threadIdx.x & 63) == 0)
  {
#pragma unroll
    for (int q = 0; q < 4; ++q) s_count[threadIdx.x >> 6][q] = count[q];
    s_count[threadIdx.x >> 6][4] = crossings;
    s_count[threadIdx.x >> 6][5] = longest;
  }
  __syncthreads();
  if (threadIdx.x < 6)
  {
    const int q = threadIdx.x;
    long long total = s_count[0][q];
    for (int w = 1; w < kBlock / 64; ++w) total = q < 5 ? total + s_count[w][q] : max(total, s_count[w][q]);
    int64_t* word[5] = {&A.info->located, &A.info->outside, &A.info->capped, &A.info->skipped, &A.info->steps};
    if (total != 0)
    {
      if (q < 5)
        atomicAdd(reinterpret_cast<unsigned long long*>(word[q]), (unsigned long long)total);
      else
        atomicMax(&A.info->max_walk, (int)total);
    }
  }
}
} // namespace

extern "C" {

int cfx_advect_options_default(cfx_advect_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_advect_options_default: null argument");
  opt->dt = 0.0;
  opt->max_distance = 0.0;
  opt->inside_tol = 1e-12;
  opt->order = 2;
  opt->max_steps = 4096;
  CFX_API_END
}

int cfx_advect_level_set(cfx_space_t V, const double* phi, const double* velocity, double* out, int32_t* cells,
                         const cfx_advect_options* opt, cfx_advect_info* info)
{
  CFX_API_BEGIN
  cfx_advect_options o;
  if (opt)
    o = *opt;
  else
    cfx_advect_options_default(&o);
  require(V && phi && velocity && out, CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: null space, phi, velocity or out");
  cfx_reinit_options ro;
  cfx_reinit_options_default(&ro);
  reinit::check_arguments("cfx_advect_level_set", V, ro); // (the space: scalar, degree 1, geometry dofmap, simplices)
  require(o.order == 1 || o.order == 2, CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: order is 1 or 2");
  require(std::isfinite(o.dt), CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: dt is finite");
  require(o.max_steps >= 1, CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: max_steps is >= 1");
  require(o.inside_tol >= 0.0 && std::isfinite(o.inside_tol), CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: inside_tol is >= 0 and finite");
  require(!std::isnan(o.max_distance), CFX_ERR_INVALID_ARGUMENT, "cfx_advect_level_set: max_distance is a number");
  ctx().ensure();
  cfx_mesh_s* mesh = V->mesh;
  const int64_t nv = mesh->nnodes;
  const int tdim = mesh->tdim;
  const DevArray<double> dphi = to_device(phi, nv), dvel = to_device(velocity, nv * tdim);
  OutArray<double> oo(out, nv, false); // (every vertex is written)
  OutArray<int32_t> co(cells, cells ? nv : 0, false);
  // out on top of phi: the lanes read other vertices' old values, so the result goes to a workspace first
  const bool alias = oo.dev < dphi.p + nv && dphi.p < oo.dev + nv;
  DevArray<double> work;
  if (alias) work.alloc(nv);
  DevArray<cfx_advect_info> rec(1);
  rec.zero();
  // (both mesh-static: built by the first call on the mesh)
  const Adjacency& adj = V->dof_cells();
  const DevArray<int32_t>& nbr = mesh->cell_neighbours();
  AdvectArgs A{};
  A.x = mesh->x.p; A.conn = mesh->conn.p; A.nbr = nbr.p; A.voff = adj.offsets.p; A.vcells = adj.cells.p;
  A.nv = nv;
  A.phi = dphi.p; A.vel = dvel.p; A.out = alias ? work.p : oo.dev; A.cells = cells ? co.dev : nullptr;
  A.info = rec.p;
  A.dt = o.dt; A.half_dt = 0.5 * o.dt; A.band = o.max_distance > 0.0 ? o.max_distance : 0.0; A.tol = o.inside_tol;
  A.order = o.order; A.max_steps = o.max_steps;
  const dim3 grid((unsigned)std::min<int64_t>((nv + kBlock - 1) / kBlock, kMaxGrid));
  if (tdim == 2)
    launch("advect_walk", advect_walk_kernel<2>, grid, dim3(kBlock), 0, A);
  else
    launch("advect_walk", advect_walk_kernel<3>, grid, dim3(kBlock), 0, A);
  if (alias) CFX_HIP(hipMemcpyAsync(oo.dev, work.p, sizeof(double) * (size_t)nv, hipMemcpyDeviceToDevice, ctx().stream));
  if (info)
  {
    if (is_device_pointer(info))
      CFX_HIP(hipMemcpyAsync(info, rec.p, sizeof(cfx_advect_info), hipMemcpyDeviceToDevice, ctx().stream));
    else
      *info = read_scalar(rec.p);
  }
  oo.finish();
  if (cells) co.finish();
  CFX_API_END
}

} // extern "C"
