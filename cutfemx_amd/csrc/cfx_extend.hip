// cutfemx_amd: extension of an interface speed along the normals, in HBM -- the stage of a moving-domain loop between
// "take a normal speed on the interface" and "move phi".
//
// Answers cutfemx.distance.extend_normal_velocity (python/cutfemx/distance.py:176-240, cpp/cutfemx/distance/
// normal_extension.h:321-485), which transports the speed with the fast iterative method of the reinitialisation
// (fast_iterative.h:55-143).  The reference copies the payload of the "best source" at the moment a distance improves, so
// its result depends on the order of the updates; here the payload is a pure function of the FINAL distance.
//
// Contract (include/cutfemx_amd.h has the full text):
//   distance     d is the d of cfx_reinitialize on the same phi and options (cfx_reinit.hip runs it, unchanged)
//   near         a vertex whose d equals its near-field value d0 bit for bit: of the seed cells K around it with
//                dist(x_v, G_K) <= (1 + 1e-12) d0_v the one with the lowest index gives the closest point c of its piece;
//                F_v = (P1 interpolant of w in K)(c), n_v = normal_sign grad(phi)|_K / |grad(phi)|_K.  phi_v == 0: F_v = w_v,
//                the normal of the lowest incident seed cell, else of the lowest incident cell with a gradient, else 0
//   transported  every other reached vertex t: of the (cell, sub-face) candidates with U <= (1 + 1e-12) d_t on the final d
//                the lowest cell, then the first sub-face in cell_update's order (none in the window: the least U); of the
//                minimiser's weights those with d_s < d_t and lambda_s > 0 are kept and renormalised;
//                F_t = sum lambda_s F_s, n_t = m / |m| with m = sum lambda_s n_s (|m| = 0: the normal of the heaviest source)
//   output       speed = F, velocity = F n, signed_distance = s min(d, B); never reached, or d > B: F = 0, n = 0
// Every kept source is strictly closer than its target: the dependencies have no cycle, the payload is unique, and Jacobi
// sweeps reach it in as many sweeps as there are levels.
//
// Launches (after the distance stage).
//   extend_plan       once: kGroup lanes per vertex over its incident cells, the next connectivity row in flight, a shuffle
//                     joins the lanes on the key (window first, value, cell).  A near vertex gets its payload (in both
//                     buffers), a transported one a record of up to TDIM source ids and weights.
//   extend_transport  per sweep: one lane per vertex; a transported one gathers F and n of its sources from the buffer of
//                     the sweep before and writes the other buffer; bitwise changes are counted with a ballot and one
//                     integer atomic per wavefront.  A sweep after one without a change returns at once.
//   extend_finish     speed and velocity from the last buffer written; the info
// No floating-point atomics, and no lane reads what another lane of the same launch writes.
#include "cfx_device.h"
#include "cfx_reinit.h"
#include "cfx_reinit_cell.h"

using namespace cfx;
using namespace cfx::reinit;

namespace
{
constexpr int kGroup = 8; // lanes per vertex (the layout of reinit_sweep)
constexpr int kTargets = kBlock / kGroup;
constexpr int kMaxGrid = 4096;
constexpr double kWindow = 1.0 + 1e-12;

struct ExtendRecord
{
  cfx_extend_info info;
  unsigned long long changed[3]; // sweep s adds to changed[s % 3], reads changed[(s - 1) % 3] and clears changed[(s + 1) % 3]
};

struct ExtendArgs
{
  const double* x;
  const int32_t* conn;
  const int64_t* voff;
  const int32_t* vcells;
  int64_t nv;
  const double* phi;
  const double* w;   // the interface speed, one value per vertex
  const double* d;
  const double* d0;
  int32_t* src;      // [TDIM][nv] the sources of a transported vertex; src[0][v] < 0: not transported
  double* lam;       // [TDIM][nv] their weights
  double* pay[2];    // [nv][TDIM + 1]: F, n
  const ReinitRecord* dist;
  ExtendRecord* rec;
  double inf, band, sign;
  int sweep;
};

__device__ __forceinline__ bool usable(const ExtendArgs& A, double v) { return v < A.inf && (A.band <= 0.0 || v <= A.band); }

struct Key
{
  int tier;   // 0: in the window; 1: the least value decides; 3: no candidate
  double val; // (0 in the window)
  int32_t cell;
};
__device__ __forceinline__ bool before(const Key& a, const Key& b)
{
  if (a.tier != b.tier) return a.tier < b.tier;
  if (a.val != b.val) return a.val < b.val;
  return a.cell < b.cell;
}

template <int TDIM>
__device__ __forceinline__ void unit_normal(const double* g, double sign, double* n)
{
  double gg = 0.0;
#pragma unroll
  for (int k = 0; k < TDIM; ++k) gg += g[k] * g[k];
  const double len = sqrt(gg);
#pragma unroll
  for (int k = 0; k < TDIM; ++k) n[k] = len > 0.0 ? sign * (g[k] / len) : 0.0;
}

enum : int { kNone = 0, kZero = 1, kNear = 2, kTransported = 3 };

template <int TDIM>
__global__ void __launch_bounds__(kBlock) extend_plan_kernel(ExtendArgs A)
{
  constexpr int NV = TDIM + 1;
  if (A.dist->info.seeds == 0) return; // no interface: nothing is written
  const int sub = threadIdx.x % kGroup, group = threadIdx.x / kGroup;
  const int64_t tiles = (A.nv + kTargets - 1) / kTargets;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) // (uniform in the block: every lane reaches the shuffles)
  {
    const int64_t v = tile * kTargets + group;
    const bool live = v < A.nv;
    const int32_t t = live ? (int32_t)v : 0;
    int kind = kNone;
    int64_t j = 0, j1 = 0;
    double xt[TDIM], dt = 0.0, d0t = 0.0;
#pragma unroll
    for (int q = 0; q < TDIM; ++q) xt[q] = 0.0;
    if (live)
    {
      dt = A.d[t];
      d0t = A.d0[t];
      if (usable(A, dt)) kind = A.phi[t] == 0.0 ? kZero : (dt == d0t ? kNear : kTransported);
      if (kind != kNone)
      {
        j = A.voff[t] + sub;
        j1 = A.voff[t + 1];
#pragma unroll
        for (int q = 0; q < TDIM; ++q) xt[q] = A.x[3 * (int64_t)t + q];
      }
    }
    const double limit = kind == kNear ? kWindow * d0t : kWindow * dt;
    Key best{3, 0.0, 0};
    double rd[NV]; // near: F, n; transported: the weights
    int32_t ri[TDIM];
#pragma unroll
    for (int q = 0; q < NV; ++q) rd[q] = 0.0;
#pragma unroll
    for (int q = 0; q < TDIM; ++q) ri[q] = -1;
    // the next cell's id and connectivity row are in flight while this one is computed
    int32_t row[NV], row_next[NV];
    int32_t c = 0, c_next = 0;
    bool have = j < j1;
    if (have)
    {
      c = A.vcells[j];
#pragma unroll
      for (int i = 0; i < NV; ++i) row[i] = A.conn[(int64_t)c * NV + i];
    }
    while (have)
    {
      const int64_t jn = j + kGroup;
      const bool have_next = jn < j1;
      if (have_next)
      {
        c_next = A.vcells[jn];
#pragma unroll
        for (int i = 0; i < NV; ++i) row_next[i] = A.conn[(int64_t)c_next * NV + i];
      }
      if (kind == kTransported)
      {
        int32_t s[TDIM];
        {
          int q = 0;
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if (row[i] != t && q < TDIM) s[q++] = row[i];
          for (; q < TDIM; ++q) s[q] = t;
        }
        double P[TDIM][TDIM], dv[TDIM], lam[TDIM], value;
        bool ok[TDIM];
#pragma unroll
        for (int i = 0; i < TDIM; ++i)
        {
          dv[i] = A.d[s[i]];
#pragma unroll
          for (int q = 0; q < TDIM; ++q) P[i][q] = A.x[3 * (int64_t)s[i] + q] - xt[q];
          ok[i] = s[i] != t && usable(A, dv[i]);
        }
        cell_update_argmin<TDIM>(P, dv, ok, A.inf, limit, value, lam);
        if (value < A.inf)
        {
          const bool in = value <= limit;
          const Key k{in ? 0 : 1, in ? 0.0 : value, c};
          if (before(k, best))
          {
            best = k;
#pragma unroll
            for (int i = 0; i < TDIM; ++i)
            {
              rd[i] = lam[i];
              ri[i] = s[i];
            }
          }
        }
      }
      else // a zero or a near vertex: the cell's piece and gradient
      {
        double X[NV][TDIM], f[NV], wv[NV], lam[NV], g[TDIM];
        int at = 0, nneg = 0;
#pragma unroll
        for (int q = 0; q < TDIM; ++q) g[q] = 0.0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
        {
          f[i] = A.phi[row[i]];
          wv[i] = A.w[row[i]];
          nneg += f[i] < 0.0 ? 1 : 0;
          if (row[i] == t) at = i;
#pragma unroll
          for (int q = 0; q < TDIM; ++q) X[i][q] = A.x[3 * (int64_t)row[i] + q];
        }
        const bool seed = nneg != 0 && nneg != NV;
        Key k{3, 0.0, c};
        double F = 0.0;
        if (kind == kZero)
        {
          cell_gradient_direction<TDIM>(X, f, g);
          bool any = false;
#pragma unroll
          for (int q = 0; q < TDIM; ++q) any = any || g[q] != 0.0;
          k.tier = seed ? 0 : (any ? 1 : 3);
          F = A.w[t];
        }
        else if (seed)
        {
          const double dist = seed_closest<TDIM>(X, f, at, lam);
          const bool in = dist <= limit;
          k.tier = in ? 0 : 1;
          k.val = in ? 0.0 : dist;
#pragma unroll
          for (int i = 0; i < NV; ++i) F += lam[i] * wv[i];
          cell_gradient_direction<TDIM>(X, f, g);
        }
        if (k.tier != 3 && before(k, best))
        {
          best = k;
          rd[0] = F;
          unit_normal<TDIM>(g, A.sign, rd + 1);
        }
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) row[i] = row_next[i];
      c = c_next;
      j = jn;
      have = have_next;
    }
    // the lane of the group that holds the first key
    int owner = sub;
    Key win = best;
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1)
    {
      Key other;
      other.tier = __shfl_xor(win.tier, o, kGroup);
      other.val = __shfl_xor(win.val, o, kGroup);
      other.cell = __shfl_xor(win.cell, o, kGroup);
      const int other_owner = __shfl_xor(owner, o, kGroup);
      if (before(other, win) || (!before(win, other) && other_owner < owner))
      {
        win = other;
        owner = other_owner;
      }
    }
    bool transported = false;
    if (live && sub == owner)
    {
      const bool found = win.tier != 3;
      double pay[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) pay[q] = 0.0;
      int32_t ids[TDIM];
      double wt[TDIM];
#pragma unroll
      for (int q = 0; q < TDIM; ++q)
      {
        ids[q] = -1;
        wt[q] = 0.0;
      }
      if (kind == kZero)
      {
        pay[0] = A.w[t]; // (a zero without a cell around it keeps n = 0)
        if (found)
#pragma unroll
          for (int q = 1; q < NV; ++q) pay[q] = rd[q];
      }
      else if (kind == kNear && found)
      {
#pragma unroll
        for (int q = 0; q < NV; ++q) pay[q] = rd[q];
      }
      else if (kind == kTransported && found)
      {
        // causal sources only: strictly closer, and with a positive weight
        double sum = 0.0;
        int kept = 0;
#pragma unroll
        for (int i = 0; i < TDIM; ++i)
          if (ri[i] >= 0 && rd[i] > 0.0 && A.d[ri[i]] < dt)
          {
            ids[kept] = ri[i];
            wt[kept] = rd[i];
            sum += rd[i];
            ++kept;
          }
        for (int i = 0; i < kept; ++i) wt[i] /= sum;
        transported = kept > 0;
      }
#pragma unroll
      for (int q = 0; q < TDIM; ++q)
      {
        A.src[q * A.nv + t] = ids[q];
        A.lam[q * A.nv + t] = wt[q];
      }
#pragma unroll
      for (int q = 0; q < NV; ++q)
      {
        A.pay[0][(int64_t)t * NV + q] = pay[q];
        A.pay[1][(int64_t)t * NV + q] = pay[q];
      }
    }
    const unsigned long long m = __ballot(transported);
    if (m != 0ull && (threadIdx.x & 63) == __ffsll((long long)m) - 1)
      atomicAdd(reinterpret_cast<unsigned long long*>(&A.rec->info.transported), (unsigned long long)__popcll(m));
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) extend_transport_kernel(ExtendArgs A)
{
  constexpr int NV = TDIM + 1;
  const int s = A.sweep;
  if (A.dist->info.seeds == 0) return;
  const unsigned long long before_this = s > 0 ? A.rec->changed[(s + 2) % 3] : 1ull;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    A.rec->changed[(s + 1) % 3] = 0ull; // (the next sweep counts there)
    if (s > 0 && before_this > 0ull) A.rec->info.transport_sweeps += 1; // the sweep before changed a payload
  }
  if (before_this == 0ull) return; // converged: both buffers hold the result
  const double* __restrict__ from = A.pay[s & 1];
  double* __restrict__ to = A.pay[(s + 1) & 1];
  // (the grid covers nv rounded up to whole blocks: every lane of a wavefront reaches the ballot)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool changed = false;
  if (v < A.nv)
  {
    int32_t id[TDIM];
    id[0] = A.src[v];
    if (id[0] >= 0)
    {
      double wt[TDIM], F = 0.0, m[TDIM], heavy[TDIM], top = -1.0;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) m[k] = heavy[k] = 0.0;
      wt[0] = A.lam[v];
#pragma unroll
      for (int i = 1; i < TDIM; ++i)
      {
        id[i] = A.src[i * A.nv + v];
        wt[i] = A.lam[i * A.nv + v];
      }
#pragma unroll
      for (int i = 0; i < TDIM; ++i)
        if (id[i] >= 0)
        {
          const double* p = from + (int64_t)id[i] * NV;
          F += wt[i] * p[0];
#pragma unroll
          for (int k = 0; k < TDIM; ++k) m[k] += wt[i] * p[1 + k];
          if (wt[i] > top)
          {
            top = wt[i];
#pragma unroll
            for (int k = 0; k < TDIM; ++k) heavy[k] = p[1 + k];
          }
        }
      double mm = 0.0;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) mm += m[k] * m[k];
      const double len = sqrt(mm);
      double out[NV];
      out[0] = F;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) out[1 + k] = len > 0.0 ? m[k] / len : heavy[k];
#pragma unroll
      for (int q = 0; q < NV; ++q)
      {
        changed = changed || __double_as_longlong(out[q]) != __double_as_longlong(from[v * NV + q]);
        to[v * NV + q] = out[q];
      }
    }
  }
  const unsigned long long mask = __ballot(changed);
  if (mask != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&A.rec->changed[s % 3], (unsigned long long)__popcll(mask));
}

// `launched`: the transport sweeps launched; the last one that ran wrote buffer launched & 1 (converged: both are equal)
template <int TDIM>
__global__ void __launch_bounds__(kBlock) extend_finish_kernel(ExtendArgs A, int launched, double* speed, double* velocity)
{
  constexpr int NV = TDIM + 1;
  const bool none = A.dist->info.seeds == 0;
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v == 0)
  {
    cfx_extend_info& I = A.rec->info;
    const cfx_reinit_info& R = A.dist->info; // (reinit_finish has set its reason)
    const bool open = launched > 0 ? A.rec->changed[(launched - 1) % 3] > 0ull : I.transported > 0;
    if (launched > 0 && open) I.transport_sweeps += 1;
    I.reason = none ? CFX_REINIT_NO_INTERFACE : (R.reason == CFX_REINIT_CONVERGED && !open ? CFX_REINIT_CONVERGED : CFX_REINIT_MAX_ITER);
    I.sweeps = R.sweeps;
    I.seeds = R.seeds;
    I.updates = R.updates;
  }
  if (none || v >= A.nv) return;
  const double* p = A.pay[launched & 1] + v * NV;
  const double F = p[0];
  if (speed) speed[v] = F;
  if (velocity)
#pragma unroll
    for (int k = 0; k < TDIM; ++k) velocity[v * TDIM + k] = F * p[1 + k];
}

template <int TDIM>
void run(ExtendArgs A, const cfx_extend_options& o, double* speed, double* velocity)
{
  const dim3 gv = grid_for(A.nv, kBlock);
  const dim3 gp((unsigned)std::min<int64_t>((A.nv + kTargets - 1) / kTargets, kMaxGrid));
  launch("extend_plan", extend_plan_kernel<TDIM>, gp, dim3(kBlock), 0, A);
  int launched = 0;
  for (int s = 0; s < o.max_iter; ++s)
  {
    A.sweep = s;
    launch("extend_transport", extend_transport_kernel<TDIM>, gv, dim3(kBlock), 0, A);
    launched = s + 1;
    // the host looks every check_every sweeps; what it sees only ends the launches (a sweep after convergence does nothing)
    if (o.check_every > 0 && launched % o.check_every == 0 && launched < o.max_iter && read_scalar(&A.rec->changed[s % 3]) == 0ull)
      break;
  }
  launch("extend_finish", extend_finish_kernel<TDIM>, gv, dim3(kBlock), 0, A, launched, speed, velocity);
}
} // namespace

extern "C" {

int cfx_extend_options_default(cfx_extend_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_extend_options_default: null argument");
  opt->tol = 1e-10;
  opt->inf_value = 1e30;
  opt->max_distance = 0.0;
  opt->max_iter = 1000;
  opt->check_every = 8;
  opt->normal_sign = 1.0;
  CFX_API_END
}

int cfx_extend_normal_velocity(cfx_space_t V, const double* phi, const double* interface_speed, double* speed, double* velocity,
                               double* signed_distance, const cfx_extend_options* opt, cfx_extend_info* info)
{
  CFX_API_BEGIN
  cfx_extend_options o;
  if (opt)
    o = *opt;
  else
    cfx_extend_options_default(&o);
  require(V && phi && interface_speed, CFX_ERR_INVALID_ARGUMENT, "cfx_extend_normal_velocity: null space, phi or interface_speed");
  cfx_reinit_options ro;
  ro.tol = o.tol; ro.inf_value = o.inf_value; ro.max_distance = o.max_distance; ro.max_iter = o.max_iter; ro.check_every = o.check_every;
  check_arguments("cfx_extend_normal_velocity", V, ro);
  require(std::isfinite(o.normal_sign), CFX_ERR_INVALID_ARGUMENT, "cfx_extend_normal_velocity: normal_sign is finite");
  ctx().ensure();
  cfx_mesh_s* mesh = V->mesh;
  const int64_t nv = mesh->nnodes;
  const int tdim = mesh->tdim;
  const DevArray<double> dphi = to_device(phi, nv), dw = to_device(interface_speed, nv);
  // (a host output is staged with its content: without an interface nothing is written)
  OutArray<double> so(speed, speed ? nv : 0, true), vo(velocity, velocity ? nv * tdim : 0, true), po(signed_distance, signed_distance ? nv : 0, true);

  DistanceStage S;
  distance_stage(V, dphi.p, ro, true, S);
  write_signed_distance(V, S, dphi.p, signed_distance ? po.dev : nullptr);

  // workspace from the block cache: the records of the transported vertices, two payload buffers, the record
  DevArray<int32_t> src(nv * tdim);
  DevArray<double> lam(nv * tdim), pay0(nv * (tdim + 1)), pay1(nv * (tdim + 1));
  DevArray<ExtendRecord> rec(1);
  rec.zero();
  const Adjacency& adj = V->dof_cells();
  ExtendArgs A{};
  A.x = mesh->x.p; A.conn = mesh->conn.p; A.voff = adj.offsets.p; A.vcells = adj.cells.p;
  A.nv = nv;
  A.phi = dphi.p; A.w = dw.p; A.d = S.d.p; A.d0 = S.d0.p;
  A.src = src.p; A.lam = lam.p; A.pay[0] = pay0.p; A.pay[1] = pay1.p;
  A.dist = S.rec.p; A.rec = rec.p;
  A.inf = S.inf; A.band = S.band; A.sign = o.normal_sign;
  if (tdim == 2)
    run<2>(A, o, speed ? so.dev : nullptr, velocity ? vo.dev : nullptr);
  else
    run<3>(A, o, speed ? so.dev : nullptr, velocity ? vo.dev : nullptr);
  if (info)
  {
    if (is_device_pointer(info))
      CFX_HIP(hipMemcpyAsync(info, &rec.p->info, sizeof(cfx_extend_info), hipMemcpyDeviceToDevice, ctx().stream));
    else
      *info = read_scalar(&rec.p->info);
  }
  if (speed) so.finish();
  if (velocity) vo.finish();
  if (signed_distance) po.finish();
  CFX_API_END
}

} // extern "C"
