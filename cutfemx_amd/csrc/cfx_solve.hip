// cutfemx_amd: the solve of assembled CSR systems in HBM -- y = A x, Jacobi-preconditioned conjugate gradients,
// diagonally preconditioned MINRES and Jacobi-preconditioned BiCGStab.
//
// Replaces the host solve of the reference's demos (python/demo/demo_poisson.py:46-58, demo_moving_poisson.py:53-67:
// PETSc KSP on the assembled matrix) for the symmetric positive definite systems cfx_assemble_matrix +
// cfx_deactivate_outside produce.  FP64 only.  Plain launches on the engine's stream: no graph, no cooperative launch, no
// hand-off between workgroups inside a launch, no floating-point atomics (the library is built with
// -munsafe-fp-atomics: their order is not fixed).
//
// Layout.  First what the solvers share: the records, RowArgs and ChainPos, the fixed-order sums, start and publish,
// for_rows (the one element-wise loop) and spmv_rows (the one row loop; it takes a per-product policy).  Then each
// solver: its arguments (RowArgs + ChainPos + its own vectors and slabs), its product policies, its kernels.  Then the
// host: one driver (Solve, Chain) and the entry points: their workspace, the wiring of the arguments, the launch list.
//
// Rows.  Every kernel walks a list of n ITERATED rows: all rows, or the caller's `rows` (the active rows of a cut
// problem: 17 M of 135 M on the 512^3 sphere).  r, q and 1/diag are indexed by the position k in that list, x and p by
// the row itself (p is read through the column indices and stays 0 outside the list, so columns outside the list enter
// r0 = b - A x0 and nothing else).
//
// SpMV.  L lanes per row, L in {1, 4, 8, 16, 64}, 256 / L rows per block tile.  Lane s of a row's group adds the entries
// j0 + s, j0 + s + L, ... in ascending order, then a fixed shuffle tree (offsets L/2 ... 1) combines the L sums: two calls
// give the same bits.  The lanes of a group read consecutive indices / values, and consecutive groups hold consecutive
// rows, so a wave's loads cover one contiguous stretch of the CSR arrays.  L comes from the mean length of the iterated
// rows -- a property of the matrix -- which is counted ON THE DEVICE (solve_count_kernel: integer sums) and read by the
// kernels from the record, so that choosing it costs no host round trip; every variant sits behind one wave-uniform
// switch in the kernel.
//
// Dot products.  The grid is capped at kMaxGrid blocks; block b takes the tiles b, b + grid, b + 2 grid ... in ascending
// order, a thread keeps a running sum over its tiles, the block adds its 256 sums in a fixed order (wave shuffle tree,
// then the four wave sums) and stores ONE partial.  Every block of the NEXT kernel adds the slab of partials in one
// fixed order (slab_sum), so all blocks hold identical alpha / beta / norms and no reduce launch is needed.
//
// CG.  One iteration = three launches:
//   cg_spmv       q = A p, partials of p.q
//   cg_update     alpha = rho / p.q;  x += alpha p, r -= alpha q, z = r / diag;  partials of r.z and r.r
//   cg_direction  beta = rho' / rho;  p = z + beta p   (z is formed again from r and 1/diag: no z array)
// Set-up: cg_init (the row pass: r = b - A x0, 1/diag, p = z = r / diag, partials of r.z, r.r and b.b) and cg_start.
//
// State.  CgRecord (HBM) holds the caller's cfx_cg_info, the state word, rho and the threshold.  Every block takes each
// decision (breakdown: p.q <= 0; converged: |r| <= threshold) from the same partials; block 0 alone stores it.  No word
// of the record is read and written in the same launch: the state lives in two slots, launch number l reads slot l & 1
// and block 0 writes slot (l + 1) & 1; rho of iteration `it` lives in slot it & 1.  The launch numbers are consecutive
// because the host's Chain hands them out.  Once the state leaves "running" every later launch returns at once, so x
// and the iteration count are frozen at the converged iterate and the result does not depend on how often the host
// looks (check_every); with check_every = 0 and a device `info` the host never looks.
//
// MINRES (cfx_minres_solve) replaces the direct solve of the reference's Stokes demo (python/demo/demo_stokes.py:39-60)
// for SYMMETRIC, possibly indefinite matrices -- the saddle-point systems of merged Stokes blocks.  It obeys every rule
// above.  Paige-Saunders MINRES in the Lanczos form with an SPD diagonal M (|a_ii|, sum_j |a_ij| or 1):
//   v: Lanczos vectors (v_j with |v_j|_{M^-1} = gamma_j), z = M^-1 v_j / gamma_j, w: search directions
//   by list position: v, v_old, q, w, w_old, 1/m;  by row: z (read through the column indices, 0 outside the list), x
// One iteration = three launches (launch number 3 it + {1, 2, 3}; minres_normalise is launch 0):
//   minres_spmv     q = A z, partials of z.q = delta
//   minres_lanczos  v_new = q - (delta / gamma1) v - (gamma1 / gamma0) v_old over v_old; partials of v_new . M^-1 v_new
//   minres_update   gamma2 = sqrt of that sum; the rotations; w_new = (z - a3 w_old - a2 w) / a1 over w_old;
//                   x += c eta w_new; z = M^-1 v_new / gamma2; eta' = -s eta; the stopping test on |eta'| = |r|_{M^-1}
// (the host swaps v / v_old and w / w_old by iteration parity).  Set-up: minres_init (the row pass: r0 = b - A x0, 1/m,
// z = M^-1 r0, partials of r0 . M^-1 r0 and b . M^-1 b), minres_start (one block: gamma1, the threshold, the state) and
// minres_normalise (z /= gamma1, once).  MinresRecord continues CgRecord: the scalars of the recurrence -- gamma_k,
// gamma_{k+1}, c and s of the last two rotations, eta -- live in two slots, iteration `it` reads slot it & 1 and block 0
// of minres_update writes slot (it + 1) & 1; delta goes from minres_lanczos to minres_update through delta[it & 1].
//
// BiCGStab (cfx_bicgstab_solve) replaces the spsolve of the reference's SUPG level-set step
// (python/demo/demo_compliance_optimization.py:1302-1350) for NONSYMMETRIC matrices.  It obeys every rule above.
// van der Vorst's recurrence, right-preconditioned with M = diag(a_ii) (the sign kept) or I, so that the recurrence
// residual is the residual of the original system and the stopping rule is CG's:
//   by list position: r (s overwrites it in the half step), rhat = r0, v = A phat, t = A shat, p, 1/diag
//   by row: phat = M^-1 p, shat = M^-1 s (read through the column indices, 0 outside the list), x
// One iteration = five launches (launch number 5 it + {0 .. 4}):
//   bicg_spmv_v     v = A phat, partials of rhat.v = sigma
//   bicg_half       alpha = rho / sigma;  s = r - alpha v over r, shat = M^-1 s;  partials of s.s
//   bicg_spmv_t     t = A shat, partials of t.t and t.s
//   bicg_update     |s| <= threshold: x += alpha phat, converged.  Else omega = t.s / t.t;  x += alpha phat + omega shat,
//                   r = s - omega t;  partials of rhat.r and r.r
//   bicg_direction  the stopping test;  beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v), phat = M^-1 p
// (|s| is known to every block only one launch after the half step, so bicg_spmv_t runs before the half-step test is
// taken: on the converging iteration its product is not used.)  Set-up: bicg_init (cg_init's row pass, which also stores
// rhat = p = r0) and bicg_start (one block; rho_0 = r0.r0).  BicgRecord continues CgRecord: rho of iteration it in
// rho[it & 1] (bicg_direction writes [(it + 1) & 1]), alpha[it & 1] from bicg_half to bicg_update and bicg_direction,
// omega[it & 1] from bicg_update to bicg_direction.  Five slabs: sigma and t.t | s.s | t.s | rhat.r | r.r share none that
// one launch both reads and writes.  Workspace: r, rhat, v, t, p, 1/diag = 48 B per iterated row, phat and shat = 16 B
// per matrix row, the slabs (80 KB), the record.
#include "cfx_device.h"

using namespace cfx;

namespace
{
constexpr int kMaxGrid = 2048; // blocks of every solve kernel (8 waves per SIMD on 256 CUs); slabs of 16 KB
constexpr int kRunning = 0;    // state word; every other value is the cfx_cg_info::reason

struct CgRecord
{
  cfx_cg_info info;       // what the caller receives (copied out as it stands)
  int32_t state[2];       // launch l reads [l & 1]; block 0 writes [(l + 1) & 1]
  double rho[2];          // r.z of iteration it in [it & 1]
  double threshold;       // max(rtol |b|, atol)
  unsigned long long nnz; // stored entries of the iterated rows (solve_count_kernel)
  int32_t bad_diagonal;   // set by the init row pass: a listed row without a stored diagonal, or with a zero one
  int32_t reserved;
};

struct MinresScalars
{
  double gamma0, gamma1; // |v_{k-1}|, |v_k| in the M^-1 norm (gamma0 = 1 before the first iteration)
  double c0, s0, c1, s1; // the last two rotations
  double eta;            // |eta| = |r|_{M^-1}
  double reserved;
};

struct MinresRecord : CgRecord // (the shared helpers see the CgRecord)
{
  MinresScalars sc[2]; // iteration it reads [it & 1]; block 0 of minres_update writes [(it + 1) & 1]
  double delta[2];     // z.Az of iteration it in [it & 1]: minres_lanczos -> minres_update
};

struct BicgRecord : CgRecord // (the shared helpers see the CgRecord)
{
  double alpha[2]; // of iteration it in [it & 1]: bicg_half -> bicg_update, bicg_direction
  double omega[2]; // of iteration it in [it & 1]: bicg_update -> bicg_direction
};

// what the row loop itself reads; Rec: the record of the solver that launches it
template <class Rec>
struct RowArgs
{
  const int64_t* indptr;
  const int32_t* indices;
  const double* values;
  const int32_t* rows; // or null: all
  int64_t n;           // iterated rows
  int lanes;           // forced L, or 0: from rec->nnz
  Rec* rec;
  const double* x;     // the vector A multiplies
};

// where a launch stands in its solver's chain (set by the host's Chain and iteration loop)
struct ChainPos
{
  int launch; // the number of this launch: it reads state[launch & 1]
  int nslab;  // partials in the slabs the launch before wrote (its grid)
  int it;     // iteration (0-based)
  int last;   // it + 1 == max_iter
};

__host__ __device__ inline int lanes_for(int64_t nnz, int64_t n)
{
  // about two entries per lane (mean length <= 2: 1, <= 8: 4, <= 16: 8, <= 64: 16, longer: a wave per row)
  if (nnz <= 2 * n) return 1;
  if (nnz <= 8 * n) return 4;
  if (nnz <= 16 * n) return 8;
  if (nnz <= 64 * n) return 16;
  return 64;
}

// the sum of the block's 256 values in a fixed order, in EVERY thread.  Every thread of the block must arrive.
__device__ __forceinline__ double block_sum_all(double v, double* wave_sums /* shared [kBlock / 64] */)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads(); // (the previous sum has been read)
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
}

// the sum of a slab of n partials, the same bits in every thread of every block
__device__ __forceinline__ double slab_sum(const double* __restrict__ slab, int n, double* wave_sums)
{
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) s += slab[i];
  return block_sum_all(s, wave_sums);
}

// the state this launch acts on; block 0 carries it over to the slot the next launch reads
__device__ __forceinline__ int state_in(CgRecord* rec, const ChainPos& c)
{
  const int st = rec->state[c.launch & 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) rec->state[(c.launch + 1) & 1] = st; // (a decision of this launch overwrites it)
  return st;
}

// Block 0 publishes what every block of the launch has decided: the state the next launch reads and, when the step
// decides, the reason; `counted`: the step completed iteration c.it (the iteration count and the residual norm).  True
// in the one thread that stores, which then adds the kernel's own scalars.
__device__ __forceinline__ bool publish(CgRecord& R, const ChainPos& c, int st, bool counted = false, double rnorm = 0.0)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return false;
  if (counted)
  {
    R.info.iterations = c.it + 1;
    R.info.residual_norm = rnorm;
  }
  if (st != kRunning) R.info.reason = st;
  R.state[(c.launch + 1) & 1] = st;
  return true;
}

// What the start kernels share (thread 0 of their one block), from the squares rr and bb of the residual's and the right
// side's norms in the solver's norm: the norms, the threshold, the start decisions in their order, the info and the state
// the first launch reads.  Returns |r0|.
__device__ __forceinline__ double start(CgRecord& R, bool precond, double rr, double bb, bool test_finite, double rtol,
                                        double atol, int max_iter)
{
  const double bnorm = sqrt(bb), rnorm = sqrt(rr), threshold = fmax(rtol * bnorm, atol);
  int st = kRunning;
  if (precond && R.bad_diagonal)
    st = CFX_CG_BAD_DIAGONAL;
  else if (test_finite && !isfinite(rr))
    st = CFX_CG_BREAKDOWN;
  else if (rnorm <= threshold)
    st = CFX_CG_CONVERGED;
  else if (max_iter == 0)
    st = CFX_CG_MAX_ITER;
  R.info.reason = st;
  R.info.iterations = 0;
  R.info.residual_norm = rnorm;
  R.info.rhs_norm = bnorm;
  R.threshold = threshold;
  R.state[0] = st;
  return rnorm;
}

// The element-wise loop: f(k, row) for the list positions of this block's tiles b, b + grid, ... in ascending order (a
// thread's running sum adds tile t before tile t + grid).
template <class F>
__device__ __forceinline__ void for_rows(const int32_t* rows, int64_t n, F f)
{
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < n) f(k, rows ? (int64_t)rows[k] : k);
  }
}

// ---- the row loop ---------------------------------------------------------------------------------------------------
// A product's policy P names its argument struct (P::Args) and says
//   has_diag, gather(S, c, row, v, d)  which diagonal quantity d the inner loop gathers from the entry (c, v) of `row`
//   row(S, k, row, s, d, acc)          what lane 0 does with the finished row: s = (A x)[row]; acc: the thread's sums
//   sums, slab(S, i)                   how many partial sums the product yields and where sum i goes
//   guarded                            whether the launch returns at once when the state is not "running"
// Product: the constants, and the gather of d = a_ii (MINRES's init replaces it).
template <class A, bool Diag, int Sums, bool Guarded>
struct Product
{
  using Args = A;
  static constexpr bool has_diag = Diag, guarded = Guarded;
  static constexpr int sums = Sums;
  static __device__ __forceinline__ void gather(const A&, int32_t c, int64_t row, double v, double& d)
  {
    if (Diag && c == row) d += v;
  }
};

// The rows of this block's tiles, L lanes each.
// A row costs a chain of dependent loads (rows[k] -> indptr[row] -> indices[j] -> x[c]), so kTiles tiles of the block's
// sequence are walked side by side: their loads are in flight together.  The order of every sum is that of one tile
// after the other -- a lane adds its entries of a row in ascending order, the thread adds tile t before tile t + grid.
constexpr int kTiles = 2;

template <int L, class P>
__device__ __forceinline__ void spmv_rows(const typename P::Args& S, double* acc)
{
  constexpr int R = kBlock / L; // rows per tile
  const int sub = threadIdx.x % L, group = threadIdx.x / L;
  const int64_t tiles = (S.n + R - 1) / R;
  for (int64_t t = blockIdx.x; t < tiles; t += (int64_t)kTiles * gridDim.x) // (uniform in the block: every lane reaches the shuffles)
  {
    int64_t k[kTiles], row[kTiles], j[kTiles], j1[kTiles];
    bool live[kTiles];
    double s[kTiles], d[kTiles];
#pragma unroll
    for (int u = 0; u < kTiles; ++u)
    {
      const int64_t tu = t + (int64_t)u * gridDim.x;
      k[u] = tu * R + group;
      live[u] = tu < tiles && k[u] < S.n;
      row[u] = 0;
      if (live[u]) row[u] = S.rows ? (int64_t)S.rows[k[u]] : k[u];
    }
#pragma unroll
    for (int u = 0; u < kTiles; ++u)
    {
      j[u] = j1[u] = 0;
      s[u] = d[u] = 0.0;
      if (live[u])
      {
        j[u] = S.indptr[row[u]] + sub;
        j1[u] = S.indptr[row[u] + 1];
      }
    }
    bool more = false;
#pragma unroll
    for (int u = 0; u < kTiles; ++u) more = more || j[u] < j1[u];
    while (more)
    {
      int32_t c[kTiles];
      double v[kTiles], xv[kTiles];
#pragma unroll
      for (int u = 0; u < kTiles; ++u)
      {
        c[u] = 0;
        v[u] = 0.0;
        if (j[u] < j1[u])
        {
          c[u] = S.indices[j[u]];
          v[u] = S.values[j[u]];
        }
      }
#pragma unroll
      for (int u = 0; u < kTiles; ++u)
      {
        xv[u] = 0.0;
        if (j[u] < j1[u]) xv[u] = S.x[c[u]];
      }
      more = false;
#pragma unroll
      for (int u = 0; u < kTiles; ++u)
      {
        if (j[u] < j1[u])
        {
          s[u] += v[u] * xv[u];
          P::gather(S, c[u], row[u], v[u], d[u]);
          j[u] += L;
        }
        more = more || j[u] < j1[u];
      }
    }
#pragma unroll
    for (int u = 0; u < kTiles; ++u)
    {
#pragma unroll
      for (int o = L / 2; o > 0; o >>= 1)
      {
        s[u] += __shfl_down(s[u], o, L);
        if (P::has_diag) d[u] += __shfl_down(d[u], o, L);
      }
    }
#pragma unroll
    for (int u = 0; u < kTiles; ++u)
      if (live[u] && sub == 0) P::row(S, k[u], row[u], s[u], d[u], acc);
  }
}

// one product of policy P: the row loop, then the block's partial sums into P's slabs
template <class P>
__global__ void __launch_bounds__(kBlock) solve_spmv_kernel(typename P::Args S)
{
  __shared__ double wave_sums[kBlock / 64];
  if constexpr (P::guarded)
    if (state_in(S.rec, S) != kRunning) return;
  const int L = S.lanes ? S.lanes : lanes_for((int64_t)S.rec->nnz, S.n);
  double acc[3] = {0.0, 0.0, 0.0};
  switch (L) // (uniform in the launch)
  {
  case 1: spmv_rows<1, P>(S, acc); break;
  case 4: spmv_rows<4, P>(S, acc); break;
  case 8: spmv_rows<8, P>(S, acc); break;
  case 16: spmv_rows<16, P>(S, acc); break;
  default: spmv_rows<64, P>(S, acc); break;
  }
#pragma unroll
  for (int i = 0; i < P::sums; ++i)
  {
    const double si = block_sum_all(acc[i], wave_sums);
    if (threadIdx.x == 0) P::slab(S, i)[blockIdx.x] = si;
  }
}

// y[rows] = (A x)[rows]
struct PlainArgs : RowArgs<CgRecord>
{
  double* y; // by row
};

struct PlainProduct : Product<PlainArgs, false, 0, false>
{
  static __device__ __forceinline__ void row(const Args& S, int64_t, int64_t row, double s, double, double*) { S.y[row] = s; }
  static __device__ __forceinline__ double* slab(const Args&, int) { return nullptr; }
};

// q = A x with the partials of x.q into A::*Slab, guarded: CG's q = A p and MINRES's q = A z
template <class A, double* A::*Slab>
struct DotProduct : Product<A, false, 1, true>
{
  static __device__ __forceinline__ void row(const A& S, int64_t k, int64_t row, double s, double, double* acc)
  {
    S.q[k] = s;
    acc[0] += S.x[row] * s;
  }
  static __device__ __forceinline__ double* slab(const A& S, int) { return S.*Slab; }
};

// The init row pass of CG and BiCGStab: r = b - A x0, 1/diag, z = r / diag into `zrow` (by row), the thread's sums of
// r.z, r.r and b.b.  Returns r_k.
template <class A>
__device__ __forceinline__ double init_row(const A& S, double* zrow, int64_t k, int64_t row, double s, double d, double* acc)
{
  const double bk = S.b[row], rk = bk - s;
  double z = rk;
  if (S.dinv)
  {
    if (!(fabs(d) > 0.0)) S.rec->bad_diagonal = 1; // (every writer stores the same value)
    const double di = 1.0 / d;
    S.dinv[k] = di;
    z = rk * di;
  }
  S.r[k] = rk;
  zrow[row] = z;
  acc[0] += rk * z;
  acc[1] += rk * rk;
  acc[2] += bk * bk;
  return rk;
}

// stored entries of the iterated rows into rec->nnz (zeroed before): integer sums, any order gives the same value
__global__ void __launch_bounds__(kBlock) solve_count_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ rows,
                                                             int64_t n, CgRecord* rec)
{
  if (!rows) // all rows: one thread
  {
    if (blockIdx.x == 0 && threadIdx.x == 0) rec->nnz = (unsigned long long)(indptr[n] - indptr[0]);
    return;
  }
  long long s = 0;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock)
  {
    const int64_t row = rows[k];
    s += indptr[row + 1] - indptr[row];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&rec->nnz, (unsigned long long)s);
}

// ---- CG -------------------------------------------------------------------------------------------------------------
struct CgArgs : RowArgs<CgRecord>, ChainPos
{
  const double* b;
  double* xs;   // the iterate (by row)
  double* r;    // r, q, dinv by list position
  double* q;
  double* dinv; // or null: no preconditioner
  double* p;    // by row
  double* pq;   // partials of p.q: cg_spmv -> cg_update    (set-up: r.z, cg_init -> cg_start)
  double* rz;   // partials of r.z: cg_update -> cg_direction (set-up: r.r)
  double* rr;   // partials of r.r: cg_update -> cg_direction (set-up: b.b)
};

struct CgInit : Product<CgArgs, true, 3, false> // r = b - A x0, 1/diag, p = z = r / diag; partials of r.z, r.r, b.b
{
  static __device__ __forceinline__ void row(const Args& S, int64_t k, int64_t row, double s, double d, double* acc)
  {
    init_row(S, S.p, k, row, s, d, acc);
  }
  static __device__ __forceinline__ double* slab(const Args& S, int i) { return i == 0 ? S.pq : i == 1 ? S.rz : S.rr; }
};
using CgProduct = DotProduct<CgArgs, &CgArgs::pq>; // q = A p; partials of p.q

// ONE block, after cg_init: the norms, the threshold, rho of iteration 0 and the state the first launch reads
__global__ void __launch_bounds__(kBlock) cg_start_kernel(CgArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rz = slab_sum(S.pq, S.nslab, wave_sums), rr = slab_sum(S.rz, S.nslab, wave_sums),
               bb = slab_sum(S.rr, S.nslab, wave_sums); // (the set-up's sums in the iteration's slabs)
  if (threadIdx.x != 0) return;
  start(*S.rec, S.dinv != nullptr, rr, bb, false, rtol, atol, max_iter);
  S.rec->rho[0] = rz;
}

// alpha = rho / p.q;  x += alpha p, r -= alpha q, z = r / diag;  partials of r.z and r.r
__global__ void __launch_bounds__(kBlock) cg_update_kernel(CgArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double pq = slab_sum(S.pq, S.nslab, wave_sums);
  const bool breakdown = !(pq > 0.0); // (also a NaN)
  publish(*S.rec, S, breakdown ? CFX_CG_BREAKDOWN : kRunning);
  if (breakdown) return;
  const double alpha = S.rec->rho[S.it & 1] / pq;
  double rz = 0.0, rr = 0.0;
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    S.xs[row] += alpha * S.p[row];
    const double rk = S.r[k] - alpha * S.q[k];
    S.r[k] = rk;
    const double z = S.dinv ? rk * S.dinv[k] : rk;
    rz += rk * z;
    rr += rk * rk;
  });
  const double s0 = block_sum_all(rz, wave_sums), s1 = block_sum_all(rr, wave_sums);
  if (threadIdx.x == 0)
  {
    S.rz[blockIdx.x] = s0; // (not into pq, which other blocks of this launch may still be reading)
    S.rr[blockIdx.x] = s1;
  }
}

// the stopping test, then beta = rho' / rho and p = z + beta p
__global__ void __launch_bounds__(kBlock) cg_direction_kernel(CgArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double rz = slab_sum(S.rz, S.nslab, wave_sums), rr = slab_sum(S.rr, S.nslab, wave_sums);
  const double rnorm = sqrt(rr);
  const int st = rnorm <= S.rec->threshold ? CFX_CG_CONVERGED : (S.last ? CFX_CG_MAX_ITER : kRunning);
  if (publish(*S.rec, S, st, true, rnorm)) S.rec->rho[(S.it + 1) & 1] = rz;
  if (st != kRunning) return;
  const double beta = rz / S.rec->rho[S.it & 1];
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    const double rk = S.r[k];
    const double z = S.dinv ? rk * S.dinv[k] : rk;
    S.p[row] = z + beta * S.p[row];
  });
}

// ---- MINRES ---------------------------------------------------------------------------------------------------------
struct MinresArgs : RowArgs<MinresRecord>, ChainPos
{
  const double* b;
  double* xs;    // the iterate (by row)
  double* z;     // by row
  double* q;     // q, v, v_old, w, w_old, dinv by list position
  double* v;
  double* v_old; // minres_lanczos writes v_new here
  double* w;
  double* w_old; // minres_update writes w_new here
  double* dinv;  // 1 / m, or null: M = I
  int pc;        // minres_init: CFX_PC_NONE, CFX_PC_ABS_JACOBI or CFX_PC_ABS_ROWSUM
  double* zq;    // partials of z.q = delta: minres_spmv -> minres_lanczos  (set-up: r0 . M^-1 r0, minres_init -> minres_start)
  double* vv;    // partials of v_new . M^-1 v_new: minres_lanczos -> minres_update  (set-up: b . M^-1 b)
};

// r0 = b - A x0 into v, 1/m, z = M^-1 r0, v_old = w = w_old = 0; partials of r0 . M^-1 r0 and b . M^-1 b
struct MinresInit : Product<MinresArgs, true, 2, false>
{
  // m = |a_ii| or sum_j |a_ij|, by the run-time S.pc
  static __device__ __forceinline__ void gather(const Args& S, int32_t c, int64_t row, double v, double& d)
  {
    if (S.pc == CFX_PC_ABS_ROWSUM)
      d += fabs(v);
    else if (c == row)
      d += v;
  }
  static __device__ __forceinline__ void row(const Args& S, int64_t k, int64_t row, double s, double d, double* acc)
  {
    const double bk = S.b[row], rk = bk - s;
    double mi = 1.0;
    if (S.dinv)
    {
      const double m = fabs(d);
      if (!(m > 0.0)) S.rec->bad_diagonal = 1; // (every writer stores the same value)
      mi = 1.0 / m;
      S.dinv[k] = mi;
    }
    const double z = rk * mi;
    S.v[k] = rk;
    S.v_old[k] = 0.0;
    S.w[k] = 0.0;
    S.w_old[k] = 0.0;
    S.z[row] = z;
    acc[0] += rk * z;
    acc[1] += bk * (bk * mi);
  }
  static __device__ __forceinline__ double* slab(const Args& S, int i) { return i == 0 ? S.zq : S.vv; }
};

using MinresProduct = DotProduct<MinresArgs, &MinresArgs::zq>; // q = A z; partials of z.q

// ONE block, after minres_init: gamma1 = |r0|_{M^-1}, |b|_{M^-1}, the threshold, the scalars of iteration 0 and the state
// the first launch reads
__global__ void __launch_bounds__(kBlock) minres_start_kernel(MinresArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rz = slab_sum(S.zq, S.nslab, wave_sums), bb = slab_sum(S.vv, S.nslab, wave_sums); // (the set-up's sums)
  if (threadIdx.x != 0) return;
  const double rnorm = start(*S.rec, S.dinv != nullptr, rz, bb, true, rtol, atol, max_iter);
  MinresScalars& sc = S.rec->sc[0];
  sc.gamma0 = 1.0;
  sc.gamma1 = rnorm;
  sc.c0 = sc.c1 = 1.0;
  sc.s0 = sc.s1 = 0.0;
  sc.eta = rnorm;
}

// z = M^-1 r0 / gamma1 (once, launch 0)
__global__ void __launch_bounds__(kBlock) minres_normalise_kernel(MinresArgs S)
{
  if (state_in(S.rec, S) != kRunning) return;
  const double zs = 1.0 / S.rec->sc[0].gamma1;
  for_rows(S.rows, S.n, [&](int64_t, int64_t row) { S.z[row] *= zs; });
}

// delta = z.q;  v_new = q - (delta / gamma1) v - (gamma1 / gamma0) v_old, over v_old;  partials of v_new . M^-1 v_new
__global__ void __launch_bounds__(kBlock) minres_lanczos_kernel(MinresArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double delta = slab_sum(S.zq, S.nslab, wave_sums);
  const bool breakdown = !isfinite(delta);
  if (publish(*S.rec, S, breakdown ? CFX_CG_BREAKDOWN : kRunning)) S.rec->delta[S.it & 1] = delta;
  if (breakdown) return;
  const MinresScalars& sc = S.rec->sc[S.it & 1];
  const double a = delta / sc.gamma1, bcoef = sc.gamma1 / sc.gamma0;
  double acc = 0.0;
  for_rows(S.rows, S.n, [&](int64_t k, int64_t) {
    const double vn = S.q[k] - a * S.v[k] - bcoef * S.v_old[k];
    S.v_old[k] = vn;
    acc += vn * (S.dinv ? vn * S.dinv[k] : vn);
  });
  const double s0 = block_sum_all(acc, wave_sums);
  if (threadIdx.x == 0) S.vv[blockIdx.x] = s0; // (not into zq, which other blocks of this launch may still be reading)
}

// gamma2, the rotations, w_new over w_old, x += c eta w_new, z = M^-1 v_new / gamma2, the stopping test.  S.v_old is the
// v_new minres_lanczos wrote.
__global__ void __launch_bounds__(kBlock) minres_update_kernel(MinresArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double g2sq = slab_sum(S.vv, S.nslab, wave_sums);
  MinresRecord& R = *S.rec;
  const MinresScalars sc = R.sc[S.it & 1];
  const double delta = R.delta[S.it & 1];
  const double gamma2 = sqrt(g2sq);
  // every block computes the same rotations
  const double a0 = sc.c1 * delta - sc.c0 * sc.s1 * sc.gamma1;
  const double a1 = sqrt(a0 * a0 + g2sq);
  const double a2 = sc.s1 * delta + sc.c0 * sc.c1 * sc.gamma1;
  const double a3 = sc.s0 * sc.gamma1;
  const bool breakdown = !isfinite(g2sq) || !(a1 > 0.0) || !isfinite(a1); // (no update of x)
  if (breakdown)
  {
    publish(R, S, CFX_CG_BREAKDOWN);
    return;
  }
  const double c2 = a0 / a1, s2 = gamma2 / a1;
  const double eta2 = -s2 * sc.eta, rnorm = fabs(eta2);
  // gamma2 == 0: the Krylov space is exhausted -- the update is finished, then the rule decides
  const int st = rnorm <= R.threshold ? CFX_CG_CONVERGED
                 : !(gamma2 > 0.0)    ? CFX_CG_BREAKDOWN
                 : S.last             ? CFX_CG_MAX_ITER
                                      : kRunning;
  if (publish(R, S, st, true, rnorm))
  {
    MinresScalars& out = R.sc[(S.it + 1) & 1];
    out.gamma0 = sc.gamma1;
    out.gamma1 = gamma2;
    out.c0 = sc.c1;
    out.s0 = sc.s1;
    out.c1 = c2;
    out.s1 = s2;
    out.eta = eta2;
  }
  const double step = c2 * sc.eta, zs = gamma2 > 0.0 ? 1.0 / gamma2 : 0.0;
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    const double wn = (S.z[row] - a3 * S.w_old[k] - a2 * S.w[k]) / a1;
    S.w_old[k] = wn;
    S.xs[row] += step * wn;
    const double vn = S.v_old[k];
    S.z[row] = (S.dinv ? vn * S.dinv[k] : vn) * zs;
  });
}

// ---- BiCGStab -------------------------------------------------------------------------------------------------------
struct BicgArgs : RowArgs<BicgRecord>, ChainPos
{
  const double* b;
  double* xs;       // the iterate (by row)
  double* r;        // r, rhat, v, t, p, dinv by list position; bicg_half leaves s in r, bicg_update makes it r again
  double* rhat;
  double* v;
  double* t;
  double* p;
  double* dinv;     // or null: no preconditioner
  double* phat;     // phat, shat by row
  double* shat;
  double* sigma_tt; // partials of rhat.v = sigma: bicg_spmv_v -> bicg_half; then of t.t: bicg_spmv_t -> bicg_update
                    // (set-up: r.z, not read)
  double* ss;       // partials of s.s: bicg_half -> bicg_update  (set-up: r.r, bicg_init -> bicg_start)
  double* ts;       // partials of t.s: bicg_spmv_t -> bicg_update  (set-up: b.b)
  double* rho;      // partials of rhat.r: bicg_update -> bicg_direction
  double* rr;       // partials of r.r: bicg_update -> bicg_direction
  int nss;          // partials in ss when bicg_update reads it: the grid of bicg_half, TWO launches back (nslab: of bicg_spmv_t)
};

struct BicgInit : Product<BicgArgs, true, 3, false> // cg_init's row pass with z into phat, and rhat = p = r0 by list position
{
  static __device__ __forceinline__ void row(const Args& S, int64_t k, int64_t row, double s, double d, double* acc)
  {
    S.rhat[k] = S.p[k] = init_row(S, S.phat, k, row, s, d, acc);
  }
  static __device__ __forceinline__ double* slab(const Args& S, int i) { return i == 0 ? S.sigma_tt : i == 1 ? S.ss : S.ts; }
};

struct BicgProductV : Product<BicgArgs, false, 1, true> // v = A phat; partials of rhat.v
{
  static __device__ __forceinline__ void row(const Args& S, int64_t k, int64_t, double s, double, double* acc)
  {
    S.v[k] = s;
    acc[0] += S.rhat[k] * s;
  }
  static __device__ __forceinline__ double* slab(const Args& S, int) { return S.sigma_tt; }
};

struct BicgProductT : Product<BicgArgs, false, 2, true> // t = A shat; partials of t.t and t.s (s lives in r)
{
  static __device__ __forceinline__ void row(const Args& S, int64_t k, int64_t, double s, double, double* acc)
  {
    S.t[k] = s;
    acc[0] += s * s;
    acc[1] += s * S.r[k];
  }
  // (not into ss, which bicg_update still has to read)
  static __device__ __forceinline__ double* slab(const Args& S, int i) { return i == 0 ? S.sigma_tt : S.ts; }
};

// ONE block, after bicg_init: the norms, the threshold, rho of iteration 0 (rhat.r = r0.r0) and the state the first
// launch reads
__global__ void __launch_bounds__(kBlock) bicg_start_kernel(BicgArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rr = slab_sum(S.ss, S.nslab, wave_sums), bb = slab_sum(S.ts, S.nslab, wave_sums); // (the set-up's sums)
  if (threadIdx.x != 0) return;
  start(*S.rec, S.dinv != nullptr, rr, bb, false, rtol, atol, max_iter);
  S.rec->rho[0] = rr;
}

// sigma = rhat.v;  alpha = rho / sigma;  s = r - alpha v over r, shat = M^-1 s;  partials of s.s
__global__ void __launch_bounds__(kBlock) bicg_half_kernel(BicgArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double sigma = slab_sum(S.sigma_tt, S.nslab, wave_sums);
  const bool breakdown = sigma == 0.0 || !isfinite(sigma); // (x is the iterate before)
  const double alpha = S.rec->rho[S.it & 1] / sigma;
  if (publish(*S.rec, S, breakdown ? CFX_CG_BREAKDOWN : kRunning)) S.rec->alpha[S.it & 1] = alpha;
  if (breakdown) return;
  double ss = 0.0;
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    const double sk = S.r[k] - alpha * S.v[k];
    S.r[k] = sk;
    S.shat[row] = S.dinv ? sk * S.dinv[k] : sk;
    ss += sk * sk;
  });
  const double s0 = block_sum_all(ss, wave_sums);
  if (threadIdx.x == 0) S.ss[blockIdx.x] = s0; // (not into sigma_tt, which other blocks of this launch may still be reading)
}

// |s| <= threshold: x += alpha phat and the solve has converged.  Else omega = t.s / t.t;  x += alpha phat + omega shat,
// r = s - omega t;  partials of rhat.r and r.r.
__global__ void __launch_bounds__(kBlock) bicg_update_kernel(BicgArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double ss = slab_sum(S.ss, S.nss, wave_sums), tt = slab_sum(S.sigma_tt, S.nslab, wave_sums),
               ts = slab_sum(S.ts, S.nslab, wave_sums);
  BicgRecord& R = *S.rec;
  const double snorm = sqrt(ss), alpha = R.alpha[S.it & 1];
  const bool half = snorm <= R.threshold;
  const bool breakdown = !half && (!isfinite(tt) || !(tt > 0.0) || !isfinite(ts)); // (no update of x)
  const double omega = half ? 0.0 : ts / tt;
  if (publish(R, S, half ? CFX_CG_CONVERGED : (breakdown ? CFX_CG_BREAKDOWN : kRunning), half, snorm)) R.omega[S.it & 1] = omega;
  if (breakdown) return;
  double hr = 0.0, rr = 0.0;
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    if (half)
      S.xs[row] += alpha * S.phat[row];
    else
    {
      S.xs[row] += alpha * S.phat[row] + omega * S.shat[row];
      const double rk = S.r[k] - omega * S.t[k];
      S.r[k] = rk;
      hr += S.rhat[k] * rk;
      rr += rk * rk;
    }
  });
  if (half) return; // (uniform in the launch)
  const double s0 = block_sum_all(hr, wave_sums), s1 = block_sum_all(rr, wave_sums);
  if (threadIdx.x == 0)
  {
    S.rho[blockIdx.x] = s0; // (sigma_tt, ss and ts are being read by other blocks of this launch)
    S.rr[blockIdx.x] = s1;
  }
}

// the stopping test, then beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v), phat = M^-1 p
__global__ void __launch_bounds__(kBlock) bicg_direction_kernel(BicgArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S.rec, S) != kRunning) return;
  const double rho1 = slab_sum(S.rho, S.nslab, wave_sums), rr = slab_sum(S.rr, S.nslab, wave_sums);
  BicgRecord& R = *S.rec;
  const double rnorm = sqrt(rr), omega = R.omega[S.it & 1];
  const bool stuck = omega == 0.0 || !isfinite(omega) || rho1 == 0.0 || !isfinite(rho1); // (x is this iterate)
  const int st = rnorm <= R.threshold ? CFX_CG_CONVERGED : S.last ? CFX_CG_MAX_ITER : stuck ? CFX_CG_BREAKDOWN : kRunning;
  if (publish(R, S, st, true, rnorm)) R.rho[(S.it + 1) & 1] = rho1;
  if (st != kRunning) return;
  const double beta = (rho1 / R.rho[S.it & 1]) * (R.alpha[S.it & 1] / omega);
  for_rows(S.rows, S.n, [&](int64_t k, int64_t row) {
    const double pk = S.r[k] + beta * (S.p[k] - omega * S.v[k]);
    S.p[k] = pk;
    S.phat[row] = S.dinv ? pk * S.dinv[k] : pk;
  });
}

// ---- the host -------------------------------------------------------------------------------------------------------
bool lanes_ok(int l) { return l == 0 || l == 1 || l == 4 || l == 8 || l == 16 || l == 64; }

// blocks of a kernel over n items, `per` a block tile: at least one (every slab is written), at most kMaxGrid
int grid_blocks(int64_t n, int per) { return (int)std::min<int64_t>(std::max<int64_t>((n + per - 1) / per, 1), kMaxGrid); }

// the grid of the row kernels does not depend on L (it is chosen on the device): sized for a wave per row
int spmv_blocks(int64_t n) { return grid_blocks(n, kBlock / 64); }

void check_csr(const char* who, int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values,
               const int32_t* rows, int64_t n_rows, int lanes)
{
  const std::string w(who);
  if (nrows < 0 || nrows > 2147483647LL) throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": nrows out of range (int32 indices)");
  if (!indptr || !indices || !values) throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": null CSR array");
  if (rows && (n_rows < 0 || n_rows > nrows))
    throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": n_rows must lie in [0, nrows] when a row list is given");
  if (!lanes_ok(lanes)) throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": lanes_per_row is one of 0 (chosen), 1, 4, 8, 16, 64");
}

void require_device(const char* who, const void* p, const char* what)
{
  if (!is_device_pointer(p)) throw Error(CFX_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what + " must be a device pointer");
}

// rec->nnz for the automatic L (two launches: the record's fill and the count)
template <class Rec>
void count_entries(const RowArgs<Rec>& S, int64_t nrows)
{
  CgRecord* rec = S.rec;
  if (S.rows)
    launch("solve_count", solve_count_kernel, dim3(grid_blocks(S.n, kBlock)), dim3(kBlock), 0, S.indptr, S.rows, S.n, rec);
  else
    launch("solve_count", solve_count_kernel, dim3(1), dim3(kBlock), 0, S.indptr, (const int32_t*)nullptr, nrows, rec);
}

// what tells the three solvers' entry points apart before their first launch
struct SolverKind
{
  const char* who;      // the entry point: the prefix of every message
  int default_precond;
  unsigned preconds;    // bit p: preconditioner id p is accepted
  const char* preconds_text;
  int launches;         // per iteration: launch numbers are int32, so max_iter <= INT32_MAX / launches
};
constexpr unsigned kJacobiOrNone = 1u << CFX_PC_NONE | 1u << CFX_PC_JACOBI;
constexpr unsigned kAbsOrNone = 1u << CFX_PC_NONE | 1u << CFX_PC_ABS_JACOBI | 1u << CFX_PC_ABS_ROWSUM;
const SolverKind kCgSolver{"cfx_cg_solve", CFX_PC_JACOBI, kJacobiOrNone, "CFX_PC_NONE or CFX_PC_JACOBI", 3};
const SolverKind kMinresSolver{"cfx_minres_solve", CFX_PC_ABS_JACOBI, kAbsOrNone,
                               "CFX_PC_NONE, CFX_PC_ABS_JACOBI or CFX_PC_ABS_ROWSUM", 3};
const SolverKind kBicgSolver{"cfx_bicgstab_solve", CFX_PC_JACOBI, kJacobiOrNone, "CFX_PC_NONE or CFX_PC_JACOBI", 5};

int options_default(const char* who, const SolverKind& kind, cfx_cg_options* opt)
{
  CFX_API_BEGIN
  if (!opt) throw Error(CFX_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
  opt->rtol = 1e-10;
  opt->atol = 0.0;
  opt->max_iter = 10000;
  opt->check_every = 16;
  opt->precond = kind.default_precond;
  opt->lanes_per_row = 0;
  CFX_API_END
}

// The chain of a solve's launches.  It owns the launch counter: every step gets the next number, so the state slots
// alternate by construction; and every launch is told how many partials the launch before it wrote (its grid).
template <class Args>
struct Chain
{
  Args& S;
  int next = 0;  // the number of the next step
  int wrote = 0; // the grid of the launch before
  // a set-up launch: not guarded by the state, so not numbered (the start kernel writes the state step 0 reads)
  template <class K, class... Extra>
  void setup(const char* name, K kernel, int grid, Extra... extra)
  {
    S.nslab = wrote;
    launch(name, kernel, dim3(grid), dim3(kBlock), 0, S, extra...);
    wrote = grid;
  }
  template <class K>
  void step(const char* name, K kernel, int grid)
  {
    S.launch = next++;
    setup(name, kernel, grid);
  }
};

// What the three entry points share: the options, the validation, b and x on the device, the zeroed record, the entry
// count, the two grids; then the iteration loop with the host's look, and the copy-out.
template <class Rec>
struct Solve
{
  cfx_cg_options o;
  RowArgs<Rec> base; // what every kernel reads (x: set by the solver)
  DevArray<double> b;
  OutArray<double> x;
  DevArray<Rec> rec;
  int g_rows, g_vec; // the grids of the row kernels and of the element-wise kernels

  static cfx_cg_options checked(const SolverKind& kind, int64_t nrows, const int64_t* indptr, const int32_t* indices,
                                const double* values, const int32_t* rows, int64_t n_rows, const double* b, double* x,
                                const cfx_cg_options* opt, cfx_cg_info* info)
  {
    const std::string w(kind.who);
    const auto need = [&](bool ok, const char* what) {
      if (!ok) throw Error(CFX_ERR_INVALID_ARGUMENT, w + ": " + what);
    };
    cfx_cg_options o;
    if (opt)
      o = *opt;
    else
      options_default(kind.who, kind, &o);
    check_csr(kind.who, nrows, indptr, indices, values, rows, n_rows, o.lanes_per_row);
    need(b && x && info, "null b, x or info");
    need(o.rtol >= 0.0 && o.atol >= 0.0, "rtol and atol are >= 0");
    need(o.max_iter >= 0 && o.check_every >= 0, "max_iter and check_every are >= 0");
    need(o.max_iter <= INT32_MAX / kind.launches, "max_iter too large");
    need(o.precond >= 0 && o.precond < 32 && (kind.preconds >> o.precond & 1u),
         (std::string("precond is ") + kind.preconds_text).c_str());
    ctx().ensure();
    for (const void* p : {(const void*)indptr, (const void*)indices, (const void*)values})
      require_device(kind.who, p, "the CSR arrays");
    if (rows) require_device(kind.who, rows, "rows");
    return o;
  }

  Solve(const SolverKind& kind, int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values,
        const int32_t* rows, int64_t n_rows, const double* b_, double* x_, const cfx_cg_options* opt, cfx_cg_info* info)
      : o(checked(kind, nrows, indptr, indices, values, rows, n_rows, b_, x_, opt, info)),
        base{indptr, indices, values, rows, rows ? n_rows : nrows, o.lanes_per_row, nullptr, nullptr}, b(to_device(b_, nrows)),
        x(x_, nrows, true), rec(1), g_rows(spmv_blocks(base.n)), g_vec(grid_blocks(base.n, kBlock))
  {
    rec.zero();
    base.rec = rec.p;
    if (base.lanes == 0) count_entries(base, nrows);
  }

  // the solver's arguments with the row loop's part filled in
  template <class Args>
  Args args() const
  {
    Args S{};
    static_cast<RowArgs<Rec>&>(S) = base;
    return S;
  }

  // max_iter iterations of `launches(it)`, then `info` and x to the caller
  template <class Args, class Launches>
  void iterate(Args& S, cfx_cg_info* info, Launches launches)
  {
    for (int it = 0; it < o.max_iter; ++it)
    {
      S.it = it;
      S.last = it + 1 == o.max_iter;
      launches(it);
      // the host looks every check_every iterations; what it sees only ends the launches (the result is frozen in HBM)
      if (o.check_every > 0 && (it + 1) % o.check_every == 0 && !S.last && read_scalar(&rec.p->info.reason) != kRunning) break;
    }
    if (is_device_pointer(info))
      CFX_HIP(hipMemcpyAsync(info, &rec.p->info, sizeof(cfx_cg_info), hipMemcpyDeviceToDevice, ctx().stream));
    else
      *info = read_scalar(&rec.p->info);
    x.finish();
  }
};
} // namespace

extern "C" {

int cfx_csr_spmv(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                 int64_t n_rows, int lanes_per_row, const double* x, double* y)
{
  CFX_API_BEGIN
  check_csr("cfx_csr_spmv", nrows, indptr, indices, values, rows, n_rows, lanes_per_row);
  require(x && y, CFX_ERR_INVALID_ARGUMENT, "cfx_csr_spmv: null vector");
  ctx().ensure();
  for (const void* p : {(const void*)indptr, (const void*)indices, (const void*)values, (const void*)x, (const void*)y})
    require_device("cfx_csr_spmv", p, "the CSR arrays, x and y");
  if (rows) require_device("cfx_csr_spmv", rows, "rows");
  PlainArgs S{{indptr, indices, values, rows, rows ? n_rows : nrows, lanes_per_row, nullptr, x}, y};
  if (S.n == 0) return CFX_OK;
  DevArray<CgRecord> rec;
  if (S.lanes == 0)
  {
    rec.alloc(1);
    rec.zero();
    S.rec = rec.p;
    count_entries(S, nrows);
  }
  launch("solve_spmv", solve_spmv_kernel<PlainProduct>, dim3(spmv_blocks(S.n)), dim3(kBlock), 0, S);
  CFX_API_END
}

int cfx_cg_options_default(cfx_cg_options* opt) { return options_default("cfx_cg_options_default", kCgSolver, opt); }

int cfx_cg_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                 int64_t n_rows, const double* b, double* x, const cfx_cg_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  Solve<CgRecord> D(kCgSolver, nrows, indptr, indices, values, rows, n_rows, b, x, opt, info);
  const int64_t n = D.base.n;
  // workspace from the block cache: r, q, 1/diag by list position, p by row, three slabs
  DevArray<double> r(n), q(n), dinv(D.o.precond == CFX_PC_JACOBI ? n : 0), p(nrows), slabs(3 * (int64_t)kMaxGrid);
  if (rows) p.zero(); // p stays 0 outside the list

  CgArgs S = D.args<CgArgs>();
  S.b = D.b.p; S.xs = D.x.dev; S.r = r.p; S.q = q.p; S.p = p.p;
  S.dinv = D.o.precond == CFX_PC_JACOBI ? dinv.p : nullptr;
  S.pq = slabs.p; S.rz = slabs.p + kMaxGrid; S.rr = slabs.p + 2 * kMaxGrid;

  Chain<CgArgs> chain{S};
  S.x = D.x.dev;
  chain.setup("cg_init", solve_spmv_kernel<CgInit>, D.g_rows);
  chain.setup("cg_start", cg_start_kernel, 1, D.o.rtol, D.o.atol, (int)D.o.max_iter);
  S.x = p.p;
  D.iterate(S, info, [&](int) {
    chain.step("cg_spmv", solve_spmv_kernel<CgProduct>, D.g_rows);
    chain.step("cg_update", cg_update_kernel, D.g_vec);
    chain.step("cg_direction", cg_direction_kernel, D.g_vec);
  });
  CFX_API_END
}

int cfx_minres_options_default(cfx_minres_options* opt)
{
  return options_default("cfx_minres_options_default", kMinresSolver, opt);
}

int cfx_minres_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                     int64_t n_rows, const double* b, double* x, const cfx_minres_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  Solve<MinresRecord> D(kMinresSolver, nrows, indptr, indices, values, rows, n_rows, b, x, opt, info);
  const int64_t n = D.base.n;
  const bool pc = D.o.precond != CFX_PC_NONE;
  // workspace from the block cache: v, v_old, q, w, w_old, 1/m by list position, z by row, two slabs
  DevArray<double> va(n), vb(n), q(n), wa(n), wb(n), minv(pc ? n : 0), z(nrows), slabs(2 * (int64_t)kMaxGrid);
  if (rows) z.zero(); // z stays 0 outside the list

  MinresArgs S = D.args<MinresArgs>();
  S.pc = D.o.precond;
  S.b = D.b.p; S.xs = D.x.dev; S.z = z.p; S.q = q.p;
  S.v = va.p; S.v_old = vb.p; S.w = wa.p; S.w_old = wb.p;
  S.dinv = pc ? minv.p : nullptr;
  S.zq = slabs.p; S.vv = slabs.p + kMaxGrid;

  Chain<MinresArgs> chain{S};
  S.x = D.x.dev;
  chain.setup("minres_init", solve_spmv_kernel<MinresInit>, D.g_rows);
  chain.setup("minres_start", minres_start_kernel, 1, D.o.rtol, D.o.atol, (int)D.o.max_iter);
  chain.step("minres_normalise", minres_normalise_kernel, D.g_vec); // (step 0: iteration it takes 3 it + {1, 2, 3})
  S.x = z.p;
  D.iterate(S, info, [&](int it) {
    S.v = it & 1 ? vb.p : va.p; S.v_old = it & 1 ? va.p : vb.p;
    S.w = it & 1 ? wb.p : wa.p; S.w_old = it & 1 ? wa.p : wb.p;
    chain.step("minres_spmv", solve_spmv_kernel<MinresProduct>, D.g_rows);
    chain.step("minres_lanczos", minres_lanczos_kernel, D.g_vec);
    chain.step("minres_update", minres_update_kernel, D.g_vec);
  });
  CFX_API_END
}

int cfx_bicgstab_options_default(cfx_bicgstab_options* opt)
{
  return options_default("cfx_bicgstab_options_default", kBicgSolver, opt);
}

int cfx_bicgstab_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                       int64_t n_rows, const double* b, double* x, const cfx_bicgstab_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  Solve<BicgRecord> D(kBicgSolver, nrows, indptr, indices, values, rows, n_rows, b, x, opt, info);
  const int64_t n = D.base.n;
  const bool pc = D.o.precond == CFX_PC_JACOBI;
  // workspace from the block cache: r, rhat, v, t, p, 1/diag by list position, phat, shat by row, five slabs
  DevArray<double> r(n), rhat(n), v(n), t(n), p(n), dinv(pc ? n : 0), phat(nrows), shat(nrows), slabs(5 * (int64_t)kMaxGrid);
  if (rows) // phat and shat stay 0 outside the list
  {
    phat.zero();
    shat.zero();
  }

  BicgArgs S = D.args<BicgArgs>();
  S.b = D.b.p; S.xs = D.x.dev; S.r = r.p; S.rhat = rhat.p; S.v = v.p; S.t = t.p; S.p = p.p; S.phat = phat.p; S.shat = shat.p;
  S.dinv = pc ? dinv.p : nullptr;
  S.sigma_tt = slabs.p; S.ss = slabs.p + kMaxGrid; S.ts = slabs.p + 2 * kMaxGrid;
  S.rho = slabs.p + 3 * kMaxGrid; S.rr = slabs.p + 4 * kMaxGrid;
  S.nss = D.g_vec; // (bicg_half's grid)

  Chain<BicgArgs> chain{S};
  S.x = D.x.dev;
  chain.setup("bicg_init", solve_spmv_kernel<BicgInit>, D.g_rows);
  chain.setup("bicg_start", bicg_start_kernel, 1, D.o.rtol, D.o.atol, (int)D.o.max_iter);
  D.iterate(S, info, [&](int) {
    S.x = phat.p;
    chain.step("bicg_spmv_v", solve_spmv_kernel<BicgProductV>, D.g_rows);
    chain.step("bicg_half", bicg_half_kernel, D.g_vec);
    S.x = shat.p;
    chain.step("bicg_spmv_t", solve_spmv_kernel<BicgProductT>, D.g_rows);
    chain.step("bicg_update", bicg_update_kernel, D.g_vec); // (nslab: of t.t and t.s; s.s has S.nss partials)
    chain.step("bicg_direction", bicg_direction_kernel, D.g_vec);
  });
  CFX_API_END
}

} // extern "C"
