// cutfemx_amd: reinitialisation of a P1 level set in HBM -- signed distance by a fast iterative method.
//
// Replaces cutfemx.distance.reinitialize (cpp/cutfemx/distance/reinitialize.h:490-575, fast_iterative.h:146-468,
// eikonal_update.h) for the stage that runs between the steps of a moving-domain loop.  FP64, 2-D and 3-D by template.
// Plain launches on the engine's stream; no floating-point atomics, and no lane reads a value that another lane of the
// same launch writes, so two calls on the same inputs give the same bits.
//
// Contract (include/cutfemx_amd.h has the full text):
//   sign       s_v = +1 where phi_v >= 0, else -1
//   near field d0_v = min over the seed cells K around v of dist(x_v, G_K), G_K the convex hull of the crossing points
//              of K's crossed edges (a segment; a triangle or a planar quadrilateral); phi_v == 0 gives d0_v = 0; every
//              other vertex starts at inf_value
//   update     U(t, K) = min over y in conv{x_s : s in K \ {t}, d_s usable} of (interpolated d)(y) + |x_t - y|
//   iteration  d_t <- min(d_t, min_K U(t, K)) until nothing changes; the iteration is monotone, its limit does not
//              depend on the order
//   band       with max_distance = B > 0 a value is usable as a source only while it is <= B; the output is min(d, B)
//   result     phi_v <- s_v d_v
//
// U in closed form (cfx_reinit_cell.h has the arithmetic, and the near field's).  For a sub-face of two or three sources,
// in an orthogonal frame of the sub-face itself: g the gradient of the interpolated d within it, z the foot of the
// perpendicular from x_t on its plane, h the height of x_t; the minimum over the plane is d(z) + h sqrt(1 - |g|^2), at
// y = z - h g / sqrt(1 - |g|^2).  It is the sub-face's when y lies in it; otherwise (or with |g| >= 1) a smaller sub-face
// holds the minimum, so U is the least valid value over all sub-faces (a single vertex is always valid).  Every quantity
// is conditioned like the sub-face, none like the cell: a flat cell (h small) loses nothing.  A face of three sources
// counts as degenerate when the sin^2 of its angle at its first source is <= 1e-9 (kDegenerate), two sources when they
// coincide; the sub-faces decide then.
//
// Launches.
//   reinit_begin   d = inf_value, the mark bits and the record cleared
//   reinit_seed    one lane per cell: the vertex signs decide "seed cell" before any coordinate is read; a seed cell
//                  forms its crossing points (always from the negative towards the non-negative end, so both cells of an
//                  edge see the same point) and lowers d0 of its vertices with an integer atomicMin on the bit pattern of
//                  the non-negative doubles -- order-independent
//   reinit_start   one lane per vertex: exact zeros, the seed count, and the first list = the neighbours of the seeds
//   per sweep s:
//   reinit_sweep   kGroup lanes per target of list s & 1: lane g takes the target's incident cells g, g + kGroup, ... (the
//                  next cell's id and connectivity row are loaded while this one is computed), a shuffle-min joins the
//                  lanes; the candidate goes to cand[k] (-1: not smaller).  d is only READ.  The target's mark is cleared.
//   reinit_commit  the same groups: a smaller candidate is stored in d (only WRITTEN here), and, while it is a source,
//                  its neighbours -- Stencil::nbr where the space has the lists, else the other vertices of its cells -- are
//                  marked (atomicOr on a bit array: the lane that flips the bit owns the vertex) and appended to list
//                  (s + 1) & 1 through a queue per wavefront in LDS: one returning integer atomic per 512 entries, and one
//                  per block when the launch ends.  The ORDER of a list varies from run to run, its SET does not, and a
//                  target's candidate depends on d alone.
//   reinit_finish  phi = s min(d, B); the reason
// The list lengths, `sweeps` (sweeps that had targets) and `updates` (targets recomputed) live in the record in HBM.  A
// sweep launched on an empty list returns at once, so the result does not depend on how often the host looks
// (check_every); with check_every = 0, a device phi and a device info the call makes no host round trip.
#include "cfx_device.h"
#include "cfx_reinit.h"
#include "cfx_reinit_cell.h"

using namespace cfx;
using namespace cfx::reinit;

namespace
{
constexpr int kGroup = 8;        // lanes per target (24 tetrahedra / 6 triangles around a Kuhn vertex)
constexpr int kTargets = kBlock / kGroup;
constexpr int kMaxGrid = 4096;   // blocks of the sweep kernels (the list length is on the device: they stride)

struct ReinitArgs
{
  const double* x;       // [nv * 3]
  const int32_t* conn;   // [ncells * (TDIM + 1)]
  const int64_t* voff;   // vertex -> cells
  const int32_t* vcells;
  const int64_t* nbr_off; // the space's neighbour lists (the vertex itself included), or null: none
  const int32_t* nbr;
  int64_t nv, ncells;
  const double* phi;
  double* out;           // the signed result (phi itself for cfx_reinitialize)
  double* d;
  double* cand;          // by list position
  int32_t* list[2];
  unsigned* bits;        // [(nv + 31) / 32]: vertex is on the list being filled
  ReinitRecord* rec;
  double inf, band;      // band <= 0: none
  int sweep;
};

__device__ __forceinline__ bool usable(const ReinitArgs& A, double v) { return v < A.inf && (A.band <= 0.0 || v <= A.band); }

__device__ __forceinline__ void lower(double* d, int64_t v, double value)
{
  atomicMin(reinterpret_cast<unsigned long long*>(d + v), (unsigned long long)__double_as_longlong(value));
}

__global__ void __launch_bounds__(kBlock) reinit_begin_kernel(ReinitArgs A)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < A.nv) A.d[i] = A.inf;
  if (i < (A.nv + 31) / 32) A.bits[i] = 0u;
  if (i == 0)
  {
    ReinitRecord& R = *A.rec;
    R.info.reason = 0;
    R.info.sweeps = 0;
    R.info.seeds = 0;
    R.info.updates = 0;
    R.count[0] = R.count[1] = 0ull;
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) reinit_seed_kernel(ReinitArgs A)
{
  constexpr int NV = TDIM + 1;
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= A.ncells) return;
  int32_t v[NV];
  double f[NV];
  int nneg = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = A.conn[c * NV + i];
#pragma unroll
  for (int i = 0; i < NV; ++i)
  {
    f[i] = A.phi[v[i]];
    nneg += f[i] < 0.0 ? 1 : 0;
  }
  if (nneg == 0 || nneg == NV) return; // (no coordinate is read)
  double X[NV][TDIM], dist[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < TDIM; ++k) X[i][k] = A.x[3 * (int64_t)v[i] + k];
  seed_cell<TDIM>(X, f, dist);
#pragma unroll
  for (int i = 0; i < NV; ++i) lower(A.d, v[i], dist[i]);
}

// ---- marks and lists ---------------------------------------------------------------------------------------------------
// true for the one lane (of all launches between two clears) that flips the bit of u
__device__ __forceinline__ bool take_mark(unsigned* bits, int32_t u)
{
  const unsigned bit = 1u << (u & 31);
  unsigned* w = bits + (u >> 5);
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return false;
  return (atomicOr(w, bit) & bit) == 0u;
}

// The hits of a wavefront are packed in its own LDS queue (the position comes from a ballot: no LDS atomic) and go to the
// list kQueue at a time: one returning atomic on the list's length per flush, and coalesced stores.  Every lane of the
// wavefront arrives at every call; n is uniform in the wavefront.
constexpr int kQueue = 512;
struct WaveQueue
{
  int32_t* q; // [kQueue], this wavefront's
  int n;
};

__device__ __forceinline__ void queue_flush(WaveQueue& Q, int32_t* __restrict__ list, unsigned long long* count)
{
  if (Q.n == 0) return;
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (the lanes read what other lanes of the wavefront stored)
  __builtin_amdgcn_wave_barrier();
  unsigned long long base = 0ull;
  if (lane == 0) base = atomicAdd(count, (unsigned long long)Q.n);
  base = __shfl(base, 0, 64);
  for (int i = lane; i < Q.n; i += 64) list[base + i] = Q.q[i];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  Q.n = 0;
}

// the last flush of a launch, by the whole block (every thread arrives): one atomic per block instead of one per wavefront
// -- a single word takes about 90 returning atomics per microsecond, and a launch has 16 K wavefronts
__device__ __forceinline__ void queue_flush_block(WaveQueue& Q, int32_t* __restrict__ list, unsigned long long* count)
{
  __shared__ int s_n[kBlock / 64];
  __shared__ unsigned long long s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_n[wave] = Q.n;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    const int total = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    s_base = total ? atomicAdd(count, (unsigned long long)total) : 0ull;
  }
  __syncthreads();
  unsigned long long base = s_base;
  for (int w = 0; w < wave; ++w) base += (unsigned long long)s_n[w];
  for (int i = lane; i < Q.n; i += 64) list[base + i] = Q.q[i];
  Q.n = 0;
}

__device__ __forceinline__ void queue_push(WaveQueue& Q, bool hit, int32_t u, int32_t* __restrict__ list, unsigned long long* count)
{
  const unsigned long long m = __ballot(hit);
  if (m == 0ull) return;
  if (Q.n + 64 > kQueue) queue_flush(Q, list, count);
  const int lane = threadIdx.x & 63;
  if (hit) Q.q[Q.n + __popcll(m & ((1ull << lane) - 1ull))] = u;
  Q.n += __popcll(m);
}

// every lane of the wavefront arrives; a `src` lane marks the neighbours of t, its share `sub`, sub + stride, ... of them:
// from the space's neighbour lists where it has them, else the other vertices of the cells around t
template <int TDIM>
__device__ __forceinline__ void mark_neighbours(const ReinitArgs& A, bool src, int32_t t, int sub, int stride, WaveQueue& Q,
                                                int32_t* __restrict__ out, unsigned long long* count)
{
  constexpr int NV = TDIM + 1;
  const int64_t* off = A.nbr ? A.nbr_off : A.voff;
  int64_t j = 0, end = 0;
  if (src)
  {
    j = off[t] + sub;
    end = off[t + 1];
  }
  if (A.nbr) // (uniform in the launch)
  {
    while (__any(j < end))
    {
      const bool act = j < end;
      const int32_t u = act ? A.nbr[j] : t;
      queue_push(Q, act && u != t && take_mark(A.bits, u), u, out, count);
      j += stride;
    }
    return;
  }
  while (__any(j < end))
  {
    const bool act = j < end;
    const int64_t c = act ? (int64_t)A.vcells[j] : 0;
#pragma unroll
    for (int i = 0; i < NV; ++i)
    {
      const int32_t u = act ? A.conn[c * NV + i] : t;
      queue_push(Q, act && u != t && take_mark(A.bits, u), u, out, count);
    }
    j += stride;
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) reinit_start_kernel(ReinitArgs A)
{
  // (the grid covers nv rounded up to whole blocks: every lane of a wavefront reaches the ballots)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = v < A.nv;
  double dv = A.inf;
  if (live)
  {
    dv = A.d[v];
    if (A.phi[v] == 0.0)
    {
      dv = 0.0;
      A.d[v] = 0.0;
    }
  }
  const bool seed = live && dv < A.inf;
  if (seed) atomicAdd(reinterpret_cast<unsigned long long*>(&A.rec->info.seeds), 1ull);
  const bool src = seed && usable(A, dv);
  __shared__ int32_t s_queue[kBlock / 64][kQueue];
  WaveQueue Q{s_queue[threadIdx.x >> 6], 0};
  mark_neighbours<TDIM>(A, src, (int32_t)v, 0, 1, Q, A.list[0], &A.rec->count[0]);
  queue_flush_block(Q, A.list[0], &A.rec->count[0]);
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) reinit_sweep_kernel(ReinitArgs A)
{
  constexpr int NV = TDIM + 1;
  const int cur = A.sweep & 1;
  const int64_t n = (int64_t)A.rec->count[cur];
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    A.rec->count[cur ^ 1] = 0ull; // (the commit of this sweep fills that list)
    if (n > 0)
    {
      A.rec->info.sweeps += 1;
      A.rec->info.updates += n;
    }
  }
  if (n == 0) return;
  const int sub = threadIdx.x % kGroup, group = threadIdx.x / kGroup;
  const int64_t tiles = (n + kTargets - 1) / kTargets;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) // (uniform in the block: every lane reaches the shuffles)
  {
    const int64_t k = tile * kTargets + group;
    const bool live = k < n;
    int32_t t = 0;
    int64_t j = 0, j1 = 0;
    double xt[TDIM], dt = 0.0;
    if (live)
    {
      t = A.list[cur][k];
      j = A.voff[t] + sub;
      j1 = A.voff[t + 1];
      dt = A.d[t];
#pragma unroll
      for (int q = 0; q < TDIM; ++q) xt[q] = A.x[3 * (int64_t)t + q];
      if (sub == 0) atomicAnd(A.bits + (t >> 5), ~(1u << (t & 31)));
    }
    double best = dt;
    // the next cell's id and connectivity row are in flight while this one is computed
    int32_t row[NV], row_next[NV];
    bool have = j < j1;
    if (have)
    {
      const int64_t c = A.vcells[j];
#pragma unroll
      for (int i = 0; i < NV; ++i) row[i] = A.conn[c * NV + i];
    }
    while (have)
    {
      const int64_t jn = j + kGroup;
      const bool have_next = jn < j1;
      if (have_next)
      {
        const int64_t c = A.vcells[jn];
#pragma unroll
        for (int i = 0; i < NV; ++i) row_next[i] = A.conn[c * NV + i];
      }
      // the other vertices: the slot of t is filled from the last one
      int32_t s[TDIM];
      {
        int q = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
          if (row[i] != t && q < TDIM) s[q++] = row[i];
        for (; q < TDIM; ++q) s[q] = t; // (a cell that names t twice: the copy of t is no source, see ok[])
      }
      double P[TDIM][TDIM], dv[TDIM];
      bool ok[TDIM];
#pragma unroll
      for (int i = 0; i < TDIM; ++i)
      {
        dv[i] = A.d[s[i]];
#pragma unroll
        for (int q = 0; q < TDIM; ++q) P[i][q] = A.x[3 * (int64_t)s[i] + q] - xt[q];
        ok[i] = s[i] != t && usable(A, dv[i]);
      }
      best = fmin(best, cell_update<TDIM>(P, dv, ok, A.inf));
#pragma unroll
      for (int i = 0; i < NV; ++i) row[i] = row_next[i];
      j = jn;
      have = have_next;
    }
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1) best = fmin(best, __shfl_xor(best, o, kGroup));
    if (live && sub == 0) A.cand[k] = best < dt ? best : -1.0;
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) reinit_commit_kernel(ReinitArgs A)
{
  const int cur = A.sweep & 1;
  const int64_t n = (int64_t)A.rec->count[cur];
  if (n == 0) return;
  const int sub = threadIdx.x % kGroup, group = threadIdx.x / kGroup;
  const int64_t tiles = (n + kTargets - 1) / kTargets;
  __shared__ int32_t s_queue[kBlock / 64][kQueue];
  WaveQueue Q{s_queue[threadIdx.x >> 6], 0};
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) // (uniform in the block: every lane reaches the ballots)
  {
    const int64_t k = tile * kTargets + group;
    int32_t t = 0;
    double val = -1.0;
    if (k < n)
    {
      t = A.list[cur][k];
      val = A.cand[k];
    }
    const bool changed = val >= 0.0;
    if (changed && sub == 0) A.d[t] = val;
    const bool src = changed && usable(A, val);
    mark_neighbours<TDIM>(A, src, t, sub, kGroup, Q, A.list[cur ^ 1], &A.rec->count[cur ^ 1]);
  }
  queue_flush_block(Q, A.list[cur ^ 1], &A.rec->count[cur ^ 1]);
}

// `slot`: the list the last launched sweep filled (empty: converged)
__global__ void __launch_bounds__(kBlock) reinit_finish_kernel(ReinitArgs A, int slot)
{
  const bool none = A.rec->info.seeds == 0;
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v == 0)
    A.rec->info.reason = none ? CFX_REINIT_NO_INTERFACE : (A.rec->count[slot] == 0ull ? CFX_REINIT_CONVERGED : CFX_REINIT_MAX_ITER);
  if (none || v >= A.nv) return;
  const double f = A.phi[v], dv = A.d[v];
  const double mag = A.band > 0.0 ? fmin(dv, A.band) : dv;
  if (A.out) A.out[v] = f >= 0.0 ? mag : -mag;
}

template <int TDIM>
int sweeps(ReinitArgs A, const cfx_reinit_options& o, double* keep_near)
{
  const dim3 gv = grid_for(A.nv, kBlock), gc = grid_for(A.ncells, kBlock);
  launch("reinit_begin", reinit_begin_kernel, gv, dim3(kBlock), 0, A);
  launch("reinit_seed", reinit_seed_kernel<TDIM>, gc, dim3(kBlock), 0, A);
  launch("reinit_start", reinit_start_kernel<TDIM>, gv, dim3(kBlock), 0, A);
  if (keep_near) CFX_HIP(hipMemcpyAsync(keep_near, A.d, sizeof(double) * (size_t)A.nv, hipMemcpyDeviceToDevice, ctx().stream));
  const dim3 gs((unsigned)std::min<int64_t>((A.nv + kTargets - 1) / kTargets, kMaxGrid));
  const dim3 gm((unsigned)std::min<int64_t>((A.nv + kTargets - 1) / kTargets, kMaxGrid / 2)); // (one closing atomic per block)
  int launched = 0;
  for (int s = 0; s < o.max_iter; ++s)
  {
    A.sweep = s;
    launch("reinit_sweep", reinit_sweep_kernel<TDIM>, gs, dim3(kBlock), 0, A);
    launch("reinit_commit", reinit_commit_kernel<TDIM>, gm, dim3(kBlock), 0, A);
    launched = s + 1;
    // the host looks every check_every sweeps; what it sees only ends the launches (a sweep of an empty list does nothing)
    if (o.check_every > 0 && launched % o.check_every == 0 && launched < o.max_iter &&
        read_scalar(&A.rec->count[launched & 1]) == 0ull)
      break;
  }
  return launched & 1;
}

ReinitArgs arguments(cfx_space_t V, const DistanceStage& S, const double* phi, double* out)
{
  cfx_mesh_s* mesh = V->mesh;
  const Adjacency& adj = V->dof_cells();
  ReinitArgs A{};
  A.x = mesh->x.p; A.conn = mesh->conn.p; A.voff = adj.offsets.p; A.vcells = adj.cells.p;
  // (both mesh-static: built by the first call on the space, or by its first assembly)
  const Stencil& st = space_stencil(V);
  if (st.lists)
  {
    A.nbr_off = st.offsets.p;
    A.nbr = st.nbr.p;
  }
  A.nv = mesh->nnodes; A.ncells = mesh->ncells;
  A.phi = phi; A.out = out; A.d = S.d.p; A.cand = S.cand.p;
  A.list[0] = S.list0.p; A.list[1] = S.list1.p;
  A.bits = S.bits.p; A.rec = S.rec.p;
  A.inf = S.inf;
  A.band = S.band;
  return A;
}
} // namespace

namespace cfx
{
namespace reinit
{
void check_arguments(const char* who, cfx_space_t V, const cfx_reinit_options& o)
{
  const std::string w(who);
  auto need = [&](bool ok, const char* what) { if (!ok) throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": " + what); };
  need(V->bs == 1, "the space must be scalar (block size 1)");
  need(V->degree == 1, "the space must have degree 1");
  need(V->dofmap.p == V->mesh->conn.p && V->ndofs == V->mesh->nnodes,
       "the space must live on the geometry dofmap (created without a dofmap of its own)");
  need(V->mesh->tdim == V->mesh->gdim && (V->mesh->tdim == 2 || V->mesh->tdim == 3), "triangles in 2-D or tetrahedra in 3-D");
  need(o.tol >= 0.0, "tol is >= 0");
  need(o.inf_value > 0.0, "inf_value is > 0");
  need(o.max_iter >= 0 && o.check_every >= 0, "max_iter and check_every are >= 0");
  need(o.max_iter <= 0x3fffffff, "max_iter too large");
}

void distance_stage(cfx_space_t V, const double* phi, const cfx_reinit_options& o, bool keep_near, DistanceStage& S)
{
  const int64_t nv = V->mesh->nnodes;
  // workspace from the block cache: the distance, the candidates, two lists, the mark bits, the record
  S.d.alloc(nv);
  S.cand.alloc(nv);
  S.list0.alloc(nv);
  S.list1.alloc(nv);
  S.bits.alloc((nv + 31) / 32);
  S.rec.alloc(1);
  if (keep_near) S.d0.alloc(nv);
  S.inf = o.inf_value;
  S.band = o.max_distance > 0.0 ? o.max_distance : 0.0;
  const ReinitArgs A = arguments(V, S, phi, nullptr);
  S.slot = V->mesh->tdim == 2 ? sweeps<2>(A, o, keep_near ? S.d0.p : nullptr) : sweeps<3>(A, o, keep_near ? S.d0.p : nullptr);
}

void write_signed_distance(cfx_space_t V, const DistanceStage& S, const double* phi, double* out)
{
  const ReinitArgs A = arguments(V, S, phi, out);
  launch("reinit_finish", reinit_finish_kernel, grid_for(A.nv, kBlock), dim3(kBlock), 0, A, S.slot);
}
} // namespace reinit
} // namespace cfx

extern "C" {

int cfx_reinit_options_default(cfx_reinit_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_reinit_options_default: null argument");
  opt->tol = 1e-10;
  opt->inf_value = 1e30;
  opt->max_distance = 0.0;
  opt->max_iter = 1000;
  opt->check_every = 8;
  CFX_API_END
}

int cfx_reinitialize(cfx_space_t V, double* phi, const cfx_reinit_options* opt, cfx_reinit_info* info)
{
  CFX_API_BEGIN
  cfx_reinit_options o;
  if (opt)
    o = *opt;
  else
    cfx_reinit_options_default(&o);
  require(V && phi, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: null space or phi");
  check_arguments("cfx_reinitialize", V, o);
  ctx().ensure();
  OutArray<double> po(phi, V->mesh->nnodes, true);
  DistanceStage S;
  distance_stage(V, po.dev, o, false, S);
  write_signed_distance(V, S, po.dev, po.dev);
  if (info)
  {
    if (is_device_pointer(info))
      CFX_HIP(hipMemcpyAsync(info, &S.rec.p->info, sizeof(cfx_reinit_info), hipMemcpyDeviceToDevice, ctx().stream));
    else
      *info = read_scalar(&S.rec.p->info);
  }
  po.finish();
  CFX_API_END
}

} // extern "C"
