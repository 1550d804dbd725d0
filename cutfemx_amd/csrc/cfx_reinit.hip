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
// U in closed form.  For a sub-face with rows P_s = x_s - x_t, Gram matrix G = P P^T and the values shifted by the first
// one (delta_s = d_s - d_0: every term of the quadratic then has the size of the cell, nothing cancels against the
// distance itself), r = d - d_0 is the larger root of (e^T adj e) r^2 - 2 (e^T adj delta) r + delta^T adj delta - det = 0
// (adj = det G^-1).  It is the minimum over the sub-face's plane, and lies in the sub-face when adj (delta - r e) <= 0
// componentwise; otherwise a smaller sub-face holds the minimum, so U is the least valid value over all sub-faces (a
// single vertex is always valid).  A face counts as degenerate relative to its own size (det <= 1e-20 x the product of
// the diagonal); its sub-faces decide then.
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

using namespace cfx;

namespace
{
constexpr int kGroup = 8;        // lanes per target (24 tetrahedra / 6 triangles around a Kuhn vertex)
constexpr int kTargets = kBlock / kGroup;
constexpr int kMaxGrid = 4096;   // blocks of the sweep kernels (the list length is on the device: they stride)
constexpr double kDegenerate = 1e-20;

struct ReinitRecord
{
  cfx_reinit_info info;        // what the caller receives (copied out as it stands)
  unsigned long long count[2]; // sweep s walks list s & 1 of count[s & 1] targets and fills the other one
};

struct ReinitArgs
{
  const double* x;       // [nv * 3]
  const int32_t* conn;   // [ncells * (TDIM + 1)]
  const int64_t* voff;   // vertex -> cells
  const int32_t* vcells;
  const int64_t* nbr_off; // the space's neighbour lists (the vertex itself included), or null: none
  const int32_t* nbr;
  int64_t nv, ncells;
  double* phi;
  double* d;
  double* cand;          // by list position
  int32_t* list[2];
  unsigned* bits;        // [(nv + 31) / 32]: vertex is on the list being filled
  ReinitRecord* rec;
  double inf, band;      // band <= 0: none
  int sweep;
};

__device__ __forceinline__ bool usable(const ReinitArgs& A, double v) { return v < A.inf && (A.band <= 0.0 || v <= A.band); }

// ---- distances to the interface piece of a seed cell -------------------------------------------------------------------
template <int D>
__host__ __device__ __forceinline__ double seg_dist2(const double* p, const double* a, const double* b)
{
  double l2 = 0.0, t = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    l2 += (b[k] - a[k]) * (b[k] - a[k]);
    t += (b[k] - a[k]) * (p[k] - a[k]);
  }
  t = l2 > 0.0 ? fmin(fmax(t / l2, 0.0), 1.0) : 0.0;
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    const double w = (p[k] - a[k]) - t * (b[k] - a[k]);
    r2 += w * w;
  }
  return r2;
}

__host__ __device__ __forceinline__ void cross3(const double* u, const double* v, double* w)
{
  w[0] = u[1] * v[2] - u[2] * v[1];
  w[1] = u[2] * v[0] - u[0] * v[2];
  w[2] = u[0] * v[1] - u[1] * v[0];
}
__host__ __device__ __forceinline__ double dot3(const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// the three edges, and the foot of the perpendicular where it falls inside
__host__ __device__ __forceinline__ double tri_dist2(const double* p, const double* a, const double* b, const double* c)
{
  double r2 = fmin(fmin(seg_dist2<3>(p, a, b), seg_dist2<3>(p, b, c)), seg_dist2<3>(p, c, a));
  double ab[3], ac[3], bc[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    ab[k] = b[k] - a[k];
    ac[k] = c[k] - a[k];
    bc[k] = c[k] - b[k];
  }
  cross3(ab, ac, n);
  const double nn = dot3(n, n);
  if (nn > kDegenerate * dot3(ab, ab) * dot3(ac, ac))
  {
    double w[3], qa[3], qb[3], qc[3], t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = p[k] - a[k];
    const double s = dot3(n, w);
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      const double q = p[k] - n[k] * (s / nn);
      qa[k] = q - a[k];
      qb[k] = q - b[k];
      qc[k] = q - c[k];
    }
    cross3(ab, qa, t);
    const double e0 = dot3(t, n);
    cross3(bc, qb, t);
    const double e1 = dot3(t, n);
    double ca[3] = {-ac[0], -ac[1], -ac[2]};
    cross3(ca, qc, t);
    const double e2 = dot3(t, n);
    if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) r2 = fmin(r2, s * s / nn);
  }
  return r2;
}

// p = x_i + phi_i / (phi_i - phi_j) (x_j - x_i), i the negative end
template <int D>
__host__ __device__ __forceinline__ void crossing(const double (*X)[D], const double* f, int i, int j, double* p)
{
  if (!(f[i] < 0.0))
  {
    const int s = i;
    i = j;
    j = s;
  }
  const double t = f[i] / (f[i] - f[j]);
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = X[i][k] + t * (X[j][k] - X[i][k]);
}

// the distances of the NV vertices of a cell to its interface piece; false: no edge of the cell is crossed
template <int TDIM>
__host__ __device__ __forceinline__ bool seed_cell(const double (*X)[TDIM], const double* f, double* dist)
{
  constexpr int NV = TDIM + 1;
  int nneg = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) nneg += f[i] < 0.0 ? 1 : 0;
  if (nneg == 0 || nneg == NV) return false;
  if constexpr (TDIM == 2)
  {
    // the vertex alone on its side, and the two edges that leave it
    const bool lone_neg = nneg == 1;
    int l = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if ((f[i] < 0.0) == lone_neg) l = i;
    double p0[2], p1[2];
    crossing<2>(X, f, l, (l + 1) % 3, p0);
    crossing<2>(X, f, l, (l + 2) % 3, p1);
#pragma unroll
    for (int i = 0; i < 3; ++i) dist[i] = sqrt(seg_dist2<2>(X[i], p0, p1));
  }
  else
  {
    double P[4][3];
    int np = 3;
    if (nneg == 2)
    {
      int neg[2] = {0, 0}, pos[2] = {0, 0}, a = 0, b = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
      {
        if (f[i] < 0.0) neg[a++] = i;
        else pos[b++] = i;
      }
      // cyclic order ac, ad, bd, bc
      crossing<3>(X, f, neg[0], pos[0], P[0]);
      crossing<3>(X, f, neg[0], pos[1], P[1]);
      crossing<3>(X, f, neg[1], pos[1], P[2]);
      crossing<3>(X, f, neg[1], pos[0], P[3]);
      np = 4;
    }
    else
    {
      const bool lone_neg = nneg == 1;
      int l = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((f[i] < 0.0) == lone_neg) l = i;
      int q = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i != l) crossing<3>(X, f, l, i, P[q++]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
      double r2 = tri_dist2(X[i], P[0], P[1], P[2]);
      if (np == 4) r2 = fmin(r2, tri_dist2(X[i], P[0], P[2], P[3]));
      dist[i] = sqrt(r2);
    }
  }
  return true;
}

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

// ---- the update --------------------------------------------------------------------------------------------------------
// two sources: Gram entries a = |P1|^2, b = P1.P2, c = |P2|^2
__host__ __device__ __forceinline__ double pair_update(double a, double b, double c, double d1, double d2, double inf)
{
  const double det = a * c - b * b;
  if (!(det > kDegenerate * a * c)) return inf;
  const double qa = a + c - 2.0 * b, dl = d2 - d1;
  const double disc = det * (qa - dl * dl);
  if (!(disc >= 0.0)) return inf;
  const double r = ((a - b) * dl + sqrt(disc)) / qa;
  const double mu1 = -c * r - b * (dl - r), mu2 = b * r + a * (dl - r);
  return (mu1 <= 0.0 && mu2 <= 0.0) ? d1 + r : inf;
}

__host__ __device__ __forceinline__ double triple_update(const double (*G)[3], const double* dv, double inf)
{
  const double a00 = G[1][1] * G[2][2] - G[1][2] * G[1][2], a01 = G[0][2] * G[1][2] - G[0][1] * G[2][2],
               a02 = G[0][1] * G[1][2] - G[0][2] * G[1][1], a11 = G[0][0] * G[2][2] - G[0][2] * G[0][2],
               a12 = G[0][1] * G[0][2] - G[0][0] * G[1][2], a22 = G[0][0] * G[1][1] - G[0][1] * G[0][1];
  const double det = G[0][0] * a00 + G[0][1] * a01 + G[0][2] * a02;
  if (!(det > kDegenerate * G[0][0] * G[1][1] * G[2][2])) return inf;
  const double d1 = dv[1] - dv[0], d2 = dv[2] - dv[0];
  const double e0 = a00 + a01 + a02, e1 = a01 + a11 + a12, e2 = a02 + a12 + a22;
  const double f0 = a01 * d1 + a02 * d2, f1 = a11 * d1 + a12 * d2, f2 = a12 * d1 + a22 * d2;
  const double qa = e0 + e1 + e2, qb = f0 + f1 + f2, qc = d1 * f1 + d2 * f2 - det;
  const double disc = qb * qb - qa * qc;
  if (!(disc >= 0.0)) return inf;
  const double r = (qb + sqrt(disc)) / qa;
  return (f0 - r * e0 <= 0.0 && f1 - r * e1 <= 0.0 && f2 - r * e2 <= 0.0) ? dv[0] + r : inf;
}

// U(t, K): P[s] = x_s - x_t and dv[s] for the TDIM other vertices of K, ok[s]: usable as a source
template <int TDIM>
__host__ __device__ __forceinline__ double cell_update(const double (*P)[TDIM], const double* dv, const bool* ok, double inf)
{
  double G[TDIM][TDIM];
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
#pragma unroll
    for (int j = i; j < TDIM; ++j)
    {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) s += P[i][k] * P[j][k];
      G[i][j] = G[j][i] = s;
    }
  double best = inf;
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
    if (ok[i]) best = fmin(best, dv[i] + sqrt(G[i][i]));
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
#pragma unroll
    for (int j = i + 1; j < TDIM; ++j)
      if (ok[i] && ok[j]) best = fmin(best, pair_update(G[i][i], G[i][j], G[j][j], dv[i], dv[j], inf));
  if constexpr (TDIM == 3)
    if (ok[0] && ok[1] && ok[2]) best = fmin(best, triple_update(G, dv, inf));
  return best;
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
  A.phi[v] = f >= 0.0 ? mag : -mag;
}

template <int TDIM>
void run(ReinitArgs A, const cfx_reinit_options& o, cfx_reinit_info* info)
{
  const dim3 gv = grid_for(A.nv, kBlock), gc = grid_for(A.ncells, kBlock);
  launch("reinit_begin", reinit_begin_kernel, gv, dim3(kBlock), 0, A);
  launch("reinit_seed", reinit_seed_kernel<TDIM>, gc, dim3(kBlock), 0, A);
  launch("reinit_start", reinit_start_kernel<TDIM>, gv, dim3(kBlock), 0, A);
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
  launch("reinit_finish", reinit_finish_kernel, gv, dim3(kBlock), 0, A, launched & 1);
  if (!info) return;
  if (is_device_pointer(info))
    CFX_HIP(hipMemcpyAsync(info, &A.rec->info, sizeof(cfx_reinit_info), hipMemcpyDeviceToDevice, ctx().stream));
  else
    *info = read_scalar(&A.rec->info);
}
} // namespace

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
  require(V->bs == 1, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: the space must be scalar (block size 1)");
  require(V->degree == 1, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: the space must have degree 1");
  require(V->dofmap.p == V->mesh->conn.p && V->ndofs == V->mesh->nnodes, CFX_ERR_INVALID_ARGUMENT,
          "cfx_reinitialize: the space must live on the geometry dofmap (created without a dofmap of its own)");
  require(V->mesh->tdim == V->mesh->gdim && (V->mesh->tdim == 2 || V->mesh->tdim == 3), CFX_ERR_INVALID_ARGUMENT,
          "cfx_reinitialize: triangles in 2-D or tetrahedra in 3-D");
  require(o.tol >= 0.0, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: tol is >= 0");
  require(o.inf_value > 0.0, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: inf_value is > 0");
  require(o.max_iter >= 0 && o.check_every >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: max_iter and check_every are >= 0");
  require(o.max_iter <= 0x3fffffff, CFX_ERR_INVALID_ARGUMENT, "cfx_reinitialize: max_iter too large");
  ctx().ensure();
  cfx_mesh_s* mesh = V->mesh;
  const Adjacency& adj = V->dof_cells();
  const int64_t nv = mesh->nnodes;
  OutArray<double> po(phi, nv, true);
  // workspace from the block cache: the distance, the candidates, two lists, the mark bits, the record
  DevArray<double> d(nv), cand(nv);
  DevArray<int32_t> list0(nv), list1(nv);
  DevArray<unsigned> bits((nv + 31) / 32);
  DevArray<ReinitRecord> rec(1);

  ReinitArgs A{};
  A.x = mesh->x.p; A.conn = mesh->conn.p; A.voff = adj.offsets.p; A.vcells = adj.cells.p;
  // (both mesh-static: built by the first call on the space, or by its first assembly)
  const Stencil& st = space_stencil(V);
  if (st.lists)
  {
    A.nbr_off = st.offsets.p;
    A.nbr = st.nbr.p;
  }
  A.nv = nv; A.ncells = mesh->ncells;
  A.phi = po.dev; A.d = d.p; A.cand = cand.p;
  A.list[0] = list0.p; A.list[1] = list1.p;
  A.bits = bits.p; A.rec = rec.p;
  A.inf = o.inf_value;
  A.band = o.max_distance > 0.0 ? o.max_distance : 0.0;
  if (mesh->tdim == 2)
    run<2>(A, o, info);
  else
    run<3>(A, o, info);
  po.finish();
  CFX_API_END
}

} // extern "C"
