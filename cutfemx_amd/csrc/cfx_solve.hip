// cutfemx_amd: the solve of assembled CSR systems in HBM -- y = A x, Jacobi-preconditioned conjugate gradients,
// diagonally preconditioned MINRES and Jacobi-preconditioned BiCGStab.
//
// Replaces the host solve of the reference's demos (python/demo/demo_poisson.py:46-58, demo_moving_poisson.py:53-67:
// PETSc KSP on the assembled matrix) for the symmetric positive definite systems cfx_assemble_matrix +
// cfx_deactivate_outside produce.  FP64 only.  Plain launches on the engine's stream: no graph, no cooperative launch, no
// hand-off between workgroups inside a launch, no floating-point atomics (the library is built with
// -munsafe-fp-atomics: their order is not fixed).
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
// One iteration = three launches:
//   cg_spmv       q = A p, partials of p.q
//   cg_update     alpha = rho / p.q;  x += alpha p, r -= alpha q, z = r / diag;  partials of r.z and r.r
//   cg_direction  beta = rho' / rho;  p = z + beta p   (z is formed again from r and 1/diag: no z array)
//
// State.  CgRecord (HBM) holds the caller's cfx_cg_info, the state word, rho and the threshold.  Every block takes each
// decision (breakdown: p.q <= 0; converged: |r| <= threshold) from the same partials; block 0 alone stores it.  No word
// of the record is read and written in the same launch: the state lives in two slots, launch number l reads slot l & 1
// and block 0 writes slot (l + 1) & 1; rho of iteration `it` lives in slot it & 1.  Once the state leaves "running" every
// later launch returns at once, so x and the iteration count are frozen at the converged iterate and the result does
// not depend on how often the host looks (check_every); with check_every = 0 and a device `info` the host never looks.
//
// MINRES (cfx_minres_solve) replaces the direct solve of the reference's Stokes demo (python/demo/demo_stokes.py:39-60)
// for SYMMETRIC, possibly indefinite matrices -- the saddle-point systems of merged Stokes blocks.  It obeys every rule
// above.  Paige-Saunders MINRES in the Lanczos form with an SPD diagonal M (|a_ii|, sum_j |a_ij| or 1):
//   v: Lanczos vectors (v_j with |v_j|_{M^-1} = gamma_j), z = M^-1 v_j / gamma_j, w: search directions
//   by list position: v, v_old, q, w, w_old, 1/m;  by row: z (read through the column indices, 0 outside the list), x
// One iteration = three launches:
//   minres_spmv     q = A z, partials of z.q = delta                 (solve_spmv_kernel<kCg> with z in p's place)
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
//   bicg_spmv_v     v = A phat, partials of rhat.v = sigma                       (solve_spmv_kernel<kBicgV>)
//   bicg_half       alpha = rho / sigma;  s = r - alpha v over r, shat = M^-1 s;  partials of s.s
//   bicg_spmv_t     t = A shat, partials of t.t and t.s                          (solve_spmv_kernel<kBicgT>)
//   bicg_update     |s| <= threshold: x += alpha phat, converged.  Else omega = t.s / t.t;  x += alpha phat + omega shat,
//                   r = s - omega t;  partials of rhat.r and r.r
//   bicg_direction  the stopping test;  beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v), phat = M^-1 p
// (|s| is known to every block only one launch after the half step, so bicg_spmv_t runs before the half-step test is
// taken: on the converging iteration its product is not used.)  Set-up: bicg_init (solve_spmv_kernel<kBicgInit>: kInit's
// row pass, which also stores rhat = p = r0) and bicg_start (one block; rho_0 = r0.r0).  BicgRecord continues CgRecord:
// rho of iteration it in rho[it & 1] (bicg_direction writes [(it + 1) & 1]), alpha[it & 1] from bicg_half to bicg_update
// and bicg_direction, omega[it & 1] from bicg_update to bicg_direction.  Five slabs: sigma | s.s | t.t | t.s | rhat.r, r.r
// share none that one launch both reads and writes.  Workspace: r, rhat, v, t, p, 1/diag = 48 B per iterated row, phat and
// shat = 16 B per matrix row, the slabs (80 KB), the record.
#include "cfx_device.h"

using namespace cfx;

namespace
{
constexpr int kMaxGrid = 2048; // blocks of every solve kernel (8 waves per SIMD on 256 CUs); slabs of 16 KB
constexpr int kRunning = 0;    // state word; every other value is the cfx_cg_info::reason
enum { kPlain = 0, kInit = 1, kCg = 2, kMinresInit = 3, kBicgInit = 4, kBicgV = 5, kBicgT = 6 };

struct CgRecord
{
  cfx_cg_info info;       // what the caller receives (copied out as it stands)
  int32_t state[2];       // launch l reads [l & 1]; block 0 writes [(l + 1) & 1]
  double rho[2];          // r.z of iteration it in [it & 1]
  double threshold;       // max(rtol |b|, atol)
  unsigned long long nnz; // stored entries of the iterated rows (solve_count_kernel)
  int32_t bad_diagonal;   // set by cg_init: a listed row without a stored diagonal, or with a zero one
  int32_t reserved;
};

struct MinresScalars
{
  double gamma0, gamma1; // |v_{k-1}|, |v_k| in the M^-1 norm (gamma0 = 1 before the first iteration)
  double c0, s0, c1, s1; // the last two rotations
  double eta;            // |eta| = |r|_{M^-1}
  double reserved;
};

struct MinresRecord : CgRecord // (the kernels shared with CG see the CgRecord)
{
  MinresScalars sc[2]; // iteration it reads [it & 1]; block 0 of minres_update writes [(it + 1) & 1]
  double delta[2];     // z.Az of iteration it in [it & 1]: minres_lanczos -> minres_update
};

struct BicgRecord : CgRecord // (the kernels shared with CG see the CgRecord)
{
  double alpha[2]; // of iteration it in [it & 1]: bicg_half -> bicg_update, bicg_direction
  double omega[2]; // of iteration it in [it & 1]: bicg_update -> bicg_direction
};

struct SolveArgs
{
  const int64_t* indptr;
  const int32_t* indices;
  const double* values;
  const int32_t* rows; // or null: all
  int64_t n;           // iterated rows
  int lanes;           // forced L, or 0: from rec->nnz
  CgRecord* rec;
  const double* x;     // the vector A multiplies (x, x0 or p)
  double* y;           // kPlain: the product (indexed by row)
  // CG (r, q, dinv by list position; xs, p by row)
  const double* b;
  double* xs;
  double* r;
  double* p;
  double* q;
  double* dinv;        // or null: no preconditioner
  double* slab0;       // partials: kInit r.z, kCg p.q, cg_update r.z
  double* slab1;       //           kInit r.r,          cg_update r.r
  double* slab2;       //           kInit b.b
  // MINRES (v, v_old, q, w, w_old, dinv = 1 / m by list position; p = z by row)
  double* v;           // r is not used
  double* v_old;       // minres_lanczos writes v_new here
  double* w;
  double* w_old;       // minres_update writes w_new here
  MinresRecord* mrec;  // == rec
  int pc;              // kMinresInit: CFX_PC_NONE, CFX_PC_ABS_JACOBI or CFX_PC_ABS_ROWSUM
  int nslab;           // partials the PREVIOUS kernel of the chain wrote
  int it;              // iteration (0-based)
  int launch;          // 3 it + {0, 1, 2}
  int last;            // it + 1 == max_iter
  // BiCGStab (r, rhat, q = v, t, pl = p, dinv by list position; p = phat, shat by row); launch = 5 it + {0 .. 4}
  double* rhat;
  double* t;
  double* pl;
  double* shat;
  double* slab3;       // partials: slab0 rhat.v and t.t, slab1 s.s, slab2 t.s, slab3 rhat.r, slab4 r.r
  double* slab4;
  BicgRecord* brec;    // == rec
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
__device__ __forceinline__ int state_in(const SolveArgs& S)
{
  const int st = S.rec->state[S.launch & 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) S.rec->state[(S.launch + 1) & 1] = st; // (a decision of this launch overwrites it)
  return st;
}

// The rows of this block's tiles, L lanes each.  acc: the thread's running sums (kInit: r.z, r.r, b.b; kCg: p.q;
// kBicgV: rhat.v; kBicgT: t.t, t.s).
// A row costs a chain of dependent loads (rows[k] -> indptr[row] -> indices[j] -> x[c]), so kTiles tiles of the block's
// sequence are walked side by side: their loads are in flight together.  The order of every sum is that of one tile
// after the other -- a lane adds its entries of a row in ascending order, the thread adds tile t before tile t + grid.
constexpr int kTiles = 2;

template <int L, int MODE>
__device__ __forceinline__ void spmv_rows(const SolveArgs& S, double* acc)
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
          if ((MODE == kInit || MODE == kBicgInit) && c[u] == row[u]) d[u] += v[u];
          if (MODE == kMinresInit)
          {
            if (S.pc == CFX_PC_ABS_ROWSUM)
              d[u] += fabs(v[u]);
            else if (c[u] == row[u])
              d[u] += v[u];
          }
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
        if (MODE == kInit || MODE == kMinresInit || MODE == kBicgInit) d[u] += __shfl_down(d[u], o, L);
      }
    }
#pragma unroll
    for (int u = 0; u < kTiles; ++u)
    {
      if (!live[u] || sub != 0) continue;
      if (MODE == kPlain)
        S.y[row[u]] = s[u];
      else if (MODE == kCg)
      {
        S.q[k[u]] = s[u];
        acc[0] += S.x[row[u]] * s[u];
      }
      else if (MODE == kBicgV)
      {
        S.q[k[u]] = s[u];
        acc[0] += S.rhat[k[u]] * s[u];
      }
      else if (MODE == kBicgT)
      {
        S.t[k[u]] = s[u];
        acc[0] += s[u] * s[u];
        acc[1] += s[u] * S.r[k[u]];
      }
      else if (MODE == kMinresInit)
      {
        const double bk = S.b[row[u]], rk = bk - s[u];
        double mi = 1.0;
        if (S.dinv)
        {
          const double m = fabs(d[u]);
          if (!(m > 0.0)) S.rec->bad_diagonal = 1; // (every writer stores the same value)
          mi = 1.0 / m;
          S.dinv[k[u]] = mi;
        }
        const double z = rk * mi;
        S.v[k[u]] = rk;
        S.v_old[k[u]] = 0.0;
        S.w[k[u]] = 0.0;
        S.w_old[k[u]] = 0.0;
        S.p[row[u]] = z;
        acc[0] += rk * z;
        acc[1] += bk * (bk * mi);
      }
      else
      {
        const double bk = S.b[row[u]], rk = bk - s[u];
        double z = rk;
        if (S.dinv)
        {
          if (!(fabs(d[u]) > 0.0)) S.rec->bad_diagonal = 1; // (every writer stores the same value)
          const double di = 1.0 / d[u];
          S.dinv[k[u]] = di;
          z = rk * di;
        }
        S.r[k[u]] = rk;
        S.p[row[u]] = z;
        if (MODE == kBicgInit) S.rhat[k[u]] = S.pl[k[u]] = rk;
        acc[0] += rk * z;
        acc[1] += rk * rk;
        acc[2] += bk * bk;
      }
    }
  }
}

// kPlain: y[rows] = (A x)[rows].  kInit: r = b - A x0, 1/diag, z = r / diag, p = z, partials of r.z, r.r, b.b.
// kCg: q = A p, partials of p.q.  kMinresInit: r0 = b - A x0 into v, 1/m, z = M^-1 r0 into p, v_old = w = w_old = 0,
// partials of r0 . M^-1 r0 and b . M^-1 b.  kBicgInit: kInit, and rhat = p = r by list position.  kBicgV: q = A phat,
// partials of rhat.q.  kBicgT: t = A shat, partials of t.t (slab0) and t.s (slab2; s lives in r).
template <int MODE>
__global__ void __launch_bounds__(kBlock) solve_spmv_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if ((MODE == kCg || MODE == kBicgV || MODE == kBicgT) && state_in(S) != kRunning) return;
  const int L = S.lanes ? S.lanes : lanes_for((int64_t)S.rec->nnz, S.n);
  double acc[3] = {0.0, 0.0, 0.0};
  switch (L) // (uniform in the launch)
  {
  case 1: spmv_rows<1, MODE>(S, acc); break;
  case 4: spmv_rows<4, MODE>(S, acc); break;
  case 8: spmv_rows<8, MODE>(S, acc); break;
  case 16: spmv_rows<16, MODE>(S, acc); break;
  default: spmv_rows<64, MODE>(S, acc); break;
  }
  if (MODE == kPlain) return;
  const double s0 = block_sum_all(acc[0], wave_sums);
  if (threadIdx.x == 0) S.slab0[blockIdx.x] = s0;
  if (MODE == kMinresInit)
  {
    const double s1 = block_sum_all(acc[1], wave_sums);
    if (threadIdx.x == 0) S.slab1[blockIdx.x] = s1;
  }
  if (MODE == kBicgT)
  {
    const double s1 = block_sum_all(acc[1], wave_sums);
    if (threadIdx.x == 0) S.slab2[blockIdx.x] = s1; // (slab1 holds s.s, which bicg_update reads)
  }
  if (MODE == kInit || MODE == kBicgInit)
  {
    const double s1 = block_sum_all(acc[1], wave_sums), s2 = block_sum_all(acc[2], wave_sums);
    if (threadIdx.x == 0)
    {
      S.slab1[blockIdx.x] = s1;
      S.slab2[blockIdx.x] = s2;
    }
  }
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

// ONE block, after cg_init: the norms, the threshold, rho of iteration 0 and the state the first launch reads
__global__ void __launch_bounds__(kBlock) cg_start_kernel(SolveArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rz = slab_sum(S.slab0, S.nslab, wave_sums), rr = slab_sum(S.slab1, S.nslab, wave_sums),
               bb = slab_sum(S.slab2, S.nslab, wave_sums);
  if (threadIdx.x != 0) return;
  CgRecord& R = *S.rec;
  const double bnorm = sqrt(bb), rnorm = sqrt(rr), threshold = fmax(rtol * bnorm, atol);
  int st = kRunning;
  if (S.dinv && R.bad_diagonal)
    st = CFX_CG_BAD_DIAGONAL;
  else if (rnorm <= threshold)
    st = CFX_CG_CONVERGED;
  else if (max_iter == 0)
    st = CFX_CG_MAX_ITER;
  R.info.reason = st;
  R.info.iterations = 0;
  R.info.residual_norm = rnorm;
  R.info.rhs_norm = bnorm;
  R.threshold = threshold;
  R.rho[0] = rz;
  R.state[0] = st;
}

// alpha = rho / p.q;  x += alpha p, r -= alpha q, z = r / diag;  partials of r.z and r.r
__global__ void __launch_bounds__(kBlock) cg_update_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double pq = slab_sum(S.slab0, S.nslab, wave_sums);
  const bool breakdown = !(pq > 0.0); // (also a NaN)
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    S.rec->state[(S.launch + 1) & 1] = breakdown ? CFX_CG_BREAKDOWN : kRunning;
    if (breakdown) S.rec->info.reason = CFX_CG_BREAKDOWN;
  }
  if (breakdown) return;
  const double alpha = S.rec->rho[S.it & 1] / pq;
  double rz = 0.0, rr = 0.0;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      S.xs[row] += alpha * S.p[row];
      const double rk = S.r[k] - alpha * S.q[k];
      S.r[k] = rk;
      const double z = S.dinv ? rk * S.dinv[k] : rk;
      rz += rk * z;
      rr += rk * rk;
    }
  }
  const double s0 = block_sum_all(rz, wave_sums), s1 = block_sum_all(rr, wave_sums);
  if (threadIdx.x == 0)
  {
    S.slab1[blockIdx.x] = s0; // (slab0 holds p.q, which other blocks of this launch may still be reading)
    S.slab2[blockIdx.x] = s1;
  }
}

// the stopping test, then beta = rho' / rho and p = z + beta p
__global__ void __launch_bounds__(kBlock) cg_direction_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double rz = slab_sum(S.slab1, S.nslab, wave_sums), rr = slab_sum(S.slab2, S.nslab, wave_sums);
  const double rnorm = sqrt(rr);
  const int st = rnorm <= S.rec->threshold ? CFX_CG_CONVERGED : (S.last ? CFX_CG_MAX_ITER : kRunning);
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    CgRecord& R = *S.rec;
    R.rho[(S.it + 1) & 1] = rz;
    R.info.iterations = S.it + 1;
    R.info.residual_norm = rnorm;
    if (st != kRunning) R.info.reason = st;
    R.state[(S.launch + 1) & 1] = st;
  }
  if (st != kRunning) return;
  const double beta = rz / S.rec->rho[S.it & 1];
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      const double rk = S.r[k];
      const double z = S.dinv ? rk * S.dinv[k] : rk;
      S.p[row] = z + beta * S.p[row];
    }
  }
}

// ---- MINRES ---------------------------------------------------------------------------------------------------------
// ONE block, after minres_init: gamma1 = |r0|_{M^-1}, |b|_{M^-1}, the threshold, the scalars of iteration 0 and the state
// the first launch reads
__global__ void __launch_bounds__(kBlock) minres_start_kernel(SolveArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rz = slab_sum(S.slab0, S.nslab, wave_sums), bb = slab_sum(S.slab1, S.nslab, wave_sums);
  if (threadIdx.x != 0) return;
  MinresRecord& R = *S.mrec;
  const double bnorm = sqrt(bb), rnorm = sqrt(rz), threshold = fmax(rtol * bnorm, atol);
  int st = kRunning;
  if (S.dinv && R.bad_diagonal)
    st = CFX_CG_BAD_DIAGONAL;
  else if (!isfinite(rz))
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
  MinresScalars& sc = R.sc[0];
  sc.gamma0 = 1.0;
  sc.gamma1 = rnorm;
  sc.c0 = sc.c1 = 1.0;
  sc.s0 = sc.s1 = 0.0;
  sc.eta = rnorm;
  R.state[0] = st;
}

// z = M^-1 r0 / gamma1 (once, launch 0)
__global__ void __launch_bounds__(kBlock) minres_normalise_kernel(SolveArgs S)
{
  if (state_in(S) != kRunning) return;
  const double zs = 1.0 / S.mrec->sc[0].gamma1;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      S.p[row] *= zs;
    }
  }
}

// delta = z.q;  v_new = q - (delta / gamma1) v - (gamma1 / gamma0) v_old, over v_old;  partials of v_new . M^-1 v_new
__global__ void __launch_bounds__(kBlock) minres_lanczos_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double delta = slab_sum(S.slab0, S.nslab, wave_sums);
  const bool breakdown = !isfinite(delta);
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    S.mrec->state[(S.launch + 1) & 1] = breakdown ? CFX_CG_BREAKDOWN : kRunning;
    if (breakdown) S.mrec->info.reason = CFX_CG_BREAKDOWN;
    S.mrec->delta[S.it & 1] = delta;
  }
  if (breakdown) return;
  const MinresScalars& sc = S.mrec->sc[S.it & 1];
  const double a = delta / sc.gamma1, bcoef = sc.gamma1 / sc.gamma0;
  double acc = 0.0;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const double vn = S.q[k] - a * S.v[k] - bcoef * S.v_old[k];
      S.v_old[k] = vn;
      acc += vn * (S.dinv ? vn * S.dinv[k] : vn);
    }
  }
  const double s0 = block_sum_all(acc, wave_sums);
  if (threadIdx.x == 0) S.slab1[blockIdx.x] = s0; // (slab0 holds z.q, which other blocks of this launch may still be reading)
}

// gamma2, the rotations, w_new over w_old, x += c eta w_new, z = M^-1 v_new / gamma2, the stopping test.  S.v_old is the
// v_new minres_lanczos wrote.
__global__ void __launch_bounds__(kBlock) minres_update_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double g2sq = slab_sum(S.slab1, S.nslab, wave_sums);
  MinresRecord& R = *S.mrec;
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
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
      R.state[(S.launch + 1) & 1] = CFX_CG_BREAKDOWN;
      R.info.reason = CFX_CG_BREAKDOWN;
    }
    return;
  }
  const double c2 = a0 / a1, s2 = gamma2 / a1;
  const double eta2 = -s2 * sc.eta, rnorm = fabs(eta2);
  // gamma2 == 0: the Krylov space is exhausted -- the update is finished, then the rule decides
  const int st = rnorm <= R.threshold ? CFX_CG_CONVERGED
                 : !(gamma2 > 0.0)    ? CFX_CG_BREAKDOWN
                 : S.last             ? CFX_CG_MAX_ITER
                                      : kRunning;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    MinresScalars& out = R.sc[(S.it + 1) & 1];
    out.gamma0 = sc.gamma1;
    out.gamma1 = gamma2;
    out.c0 = sc.c1;
    out.s0 = sc.s1;
    out.c1 = c2;
    out.s1 = s2;
    out.eta = eta2;
    R.info.iterations = S.it + 1;
    R.info.residual_norm = rnorm;
    if (st != kRunning) R.info.reason = st;
    R.state[(S.launch + 1) & 1] = st;
  }
  const double step = c2 * sc.eta, zs = gamma2 > 0.0 ? 1.0 / gamma2 : 0.0;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      const double wn = (S.p[row] - a3 * S.w_old[k] - a2 * S.w[k]) / a1;
      S.w_old[k] = wn;
      S.xs[row] += step * wn;
      const double vn = S.v_old[k];
      S.p[row] = (S.dinv ? vn * S.dinv[k] : vn) * zs;
    }
  }
}

// ---- BiCGStab -------------------------------------------------------------------------------------------------------
// ONE block, after bicg_init: the norms, the threshold, rho of iteration 0 (rhat.r = r0.r0) and the state the first
// launch reads
__global__ void __launch_bounds__(kBlock) bicg_start_kernel(SolveArgs S, double rtol, double atol, int max_iter)
{
  __shared__ double wave_sums[kBlock / 64];
  const double rr = slab_sum(S.slab1, S.nslab, wave_sums), bb = slab_sum(S.slab2, S.nslab, wave_sums);
  if (threadIdx.x != 0) return;
  CgRecord& R = *S.rec;
  const double bnorm = sqrt(bb), rnorm = sqrt(rr), threshold = fmax(rtol * bnorm, atol);
  int st = kRunning;
  if (S.dinv && R.bad_diagonal)
    st = CFX_CG_BAD_DIAGONAL;
  else if (rnorm <= threshold)
    st = CFX_CG_CONVERGED;
  else if (max_iter == 0)
    st = CFX_CG_MAX_ITER;
  R.info.reason = st;
  R.info.iterations = 0;
  R.info.residual_norm = rnorm;
  R.info.rhs_norm = bnorm;
  R.threshold = threshold;
  R.rho[0] = rr;
  R.state[0] = st;
}

// sigma = rhat.v;  alpha = rho / sigma;  s = r - alpha v over r, shat = M^-1 s;  partials of s.s
__global__ void __launch_bounds__(kBlock) bicg_half_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double sigma = slab_sum(S.slab0, S.nslab, wave_sums);
  const bool breakdown = sigma == 0.0 || !isfinite(sigma); // (x is the iterate before)
  const double alpha = S.brec->rho[S.it & 1] / sigma;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    S.brec->state[(S.launch + 1) & 1] = breakdown ? CFX_CG_BREAKDOWN : kRunning;
    if (breakdown) S.brec->info.reason = CFX_CG_BREAKDOWN;
    S.brec->alpha[S.it & 1] = alpha;
  }
  if (breakdown) return;
  double ss = 0.0;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      const double sk = S.r[k] - alpha * S.q[k];
      S.r[k] = sk;
      S.shat[row] = S.dinv ? sk * S.dinv[k] : sk;
      ss += sk * sk;
    }
  }
  const double s0 = block_sum_all(ss, wave_sums);
  if (threadIdx.x == 0) S.slab1[blockIdx.x] = s0; // (slab0 holds rhat.v, which other blocks of this launch may still be reading)
}

// |s| <= threshold: x += alpha phat and the solve has converged.  Else omega = t.s / t.t;  x += alpha phat + omega shat,
// r = s - omega t;  partials of rhat.r and r.r.  (s.s comes from bicg_half, whose grid is this launch's.)
__global__ void __launch_bounds__(kBlock) bicg_update_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double ss = slab_sum(S.slab1, gridDim.x, wave_sums), tt = slab_sum(S.slab0, S.nslab, wave_sums),
               ts = slab_sum(S.slab2, S.nslab, wave_sums);
  BicgRecord& R = *S.brec;
  const double snorm = sqrt(ss), alpha = R.alpha[S.it & 1];
  const bool half = snorm <= R.threshold;
  const bool breakdown = !half && (!isfinite(tt) || !(tt > 0.0) || !isfinite(ts)); // (no update of x)
  const double omega = half ? 0.0 : ts / tt;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    if (half)
    {
      R.info.iterations = S.it + 1;
      R.info.residual_norm = snorm;
    }
    if (half || breakdown) R.info.reason = half ? CFX_CG_CONVERGED : CFX_CG_BREAKDOWN;
    R.state[(S.launch + 1) & 1] = half ? CFX_CG_CONVERGED : (breakdown ? CFX_CG_BREAKDOWN : kRunning);
    R.omega[S.it & 1] = omega;
  }
  if (breakdown) return;
  double hr = 0.0, rr = 0.0;
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      if (half)
        S.xs[row] += alpha * S.p[row];
      else
      {
        S.xs[row] += alpha * S.p[row] + omega * S.shat[row];
        const double rk = S.r[k] - omega * S.t[k];
        S.r[k] = rk;
        hr += S.rhat[k] * rk;
        rr += rk * rk;
      }
    }
  }
  if (half) return; // (uniform in the launch)
  const double s0 = block_sum_all(hr, wave_sums), s1 = block_sum_all(rr, wave_sums);
  if (threadIdx.x == 0)
  {
    S.slab3[blockIdx.x] = s0; // (slabs 0 .. 2 are being read by other blocks of this launch)
    S.slab4[blockIdx.x] = s1;
  }
}

// the stopping test, then beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v), phat = M^-1 p
__global__ void __launch_bounds__(kBlock) bicg_direction_kernel(SolveArgs S)
{
  __shared__ double wave_sums[kBlock / 64];
  if (state_in(S) != kRunning) return;
  const double rho1 = slab_sum(S.slab3, S.nslab, wave_sums), rr = slab_sum(S.slab4, S.nslab, wave_sums);
  BicgRecord& R = *S.brec;
  const double rnorm = sqrt(rr), omega = R.omega[S.it & 1];
  const bool stuck = omega == 0.0 || !isfinite(omega) || rho1 == 0.0 || !isfinite(rho1); // (x is this iterate)
  const int st = rnorm <= R.threshold ? CFX_CG_CONVERGED : S.last ? CFX_CG_MAX_ITER : stuck ? CFX_CG_BREAKDOWN : kRunning;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    R.rho[(S.it + 1) & 1] = rho1;
    R.info.iterations = S.it + 1;
    R.info.residual_norm = rnorm;
    if (st != kRunning) R.info.reason = st;
    R.state[(S.launch + 1) & 1] = st;
  }
  if (st != kRunning) return;
  const double beta = (rho1 / R.rho[S.it & 1]) * (R.alpha[S.it & 1] / omega);
  const int64_t tiles = (S.n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x)
  {
    const int64_t k = t * kBlock + threadIdx.x;
    if (k < S.n)
    {
      const int64_t row = S.rows ? (int64_t)S.rows[k] : k;
      const double pk = S.r[k] + beta * (S.pl[k] - omega * S.q[k]);
      S.pl[k] = pk;
      S.p[row] = S.dinv ? pk * S.dinv[k] : pk;
    }
  }
}

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
void count_entries(const SolveArgs& S, int64_t nrows)
{
  if (S.rows)
    launch("solve_count", solve_count_kernel, dim3(grid_blocks(S.n, kBlock)), dim3(kBlock), 0, S.indptr, S.rows, S.n, S.rec);
  else
    launch("solve_count", solve_count_kernel, dim3(1), dim3(kBlock), 0, S.indptr, (const int32_t*)nullptr, nrows, S.rec);
}
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
  SolveArgs S{};
  S.indptr = indptr; S.indices = indices; S.values = values; S.rows = rows;
  S.n = rows ? n_rows : nrows;
  S.lanes = lanes_per_row;
  S.x = x; S.y = y;
  if (S.n == 0) return CFX_OK;
  DevArray<CgRecord> rec;
  if (S.lanes == 0)
  {
    rec.alloc(1);
    rec.zero();
    S.rec = rec.p;
    count_entries(S, nrows);
  }
  launch("solve_spmv", solve_spmv_kernel<kPlain>, dim3(spmv_blocks(S.n)), dim3(kBlock), 0, S);
  CFX_API_END
}

int cfx_cg_options_default(cfx_cg_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_cg_options_default: null argument");
  opt->rtol = 1e-10;
  opt->atol = 0.0;
  opt->max_iter = 10000;
  opt->check_every = 16;
  opt->precond = CFX_PC_JACOBI;
  opt->lanes_per_row = 0;
  CFX_API_END
}

int cfx_cg_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                 int64_t n_rows, const double* b, double* x, const cfx_cg_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  cfx_cg_options o;
  if (opt)
    o = *opt;
  else
    cfx_cg_options_default(&o);
  check_csr("cfx_cg_solve", nrows, indptr, indices, values, rows, n_rows, o.lanes_per_row);
  require(b && x && info, CFX_ERR_INVALID_ARGUMENT, "cfx_cg_solve: null b, x or info");
  require(o.rtol >= 0.0 && o.atol >= 0.0, CFX_ERR_INVALID_ARGUMENT, "cfx_cg_solve: rtol and atol are >= 0");
  require(o.max_iter >= 0 && o.check_every >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_cg_solve: max_iter and check_every are >= 0");
  require(o.max_iter <= 0x2aaaaaaa, CFX_ERR_INVALID_ARGUMENT, "cfx_cg_solve: max_iter too large");
  require(o.precond == CFX_PC_NONE || o.precond == CFX_PC_JACOBI, CFX_ERR_INVALID_ARGUMENT,
          "cfx_cg_solve: precond is CFX_PC_NONE or CFX_PC_JACOBI");
  ctx().ensure();
  for (const void* p : {(const void*)indptr, (const void*)indices, (const void*)values})
    require_device("cfx_cg_solve", p, "the CSR arrays");
  if (rows) require_device("cfx_cg_solve", rows, "rows");

  const int64_t n = rows ? n_rows : nrows;
  DevArray<double> bd = to_device(b, nrows);
  OutArray<double> xo(x, nrows, true);
  // workspace from the block cache: r, q, 1/diag by list position, p by row, three slabs, the record
  DevArray<double> r(n), q(n), dinv(o.precond == CFX_PC_JACOBI ? n : 0), p(nrows), slabs(3 * (int64_t)kMaxGrid);
  DevArray<CgRecord> rec(1);
  rec.zero();
  if (rows) p.zero(); // p stays 0 outside the list

  SolveArgs S{};
  S.indptr = indptr; S.indices = indices; S.values = values; S.rows = rows;
  S.n = n;
  S.lanes = o.lanes_per_row;
  S.rec = rec.p;
  S.b = bd.p; S.xs = xo.dev; S.r = r.p; S.p = p.p; S.q = q.p;
  S.dinv = o.precond == CFX_PC_JACOBI ? dinv.p : nullptr;
  S.slab0 = slabs.p; S.slab1 = slabs.p + kMaxGrid; S.slab2 = slabs.p + 2 * kMaxGrid;
  if (S.lanes == 0) count_entries(S, nrows);

  const int g_rows = spmv_blocks(n), g_vec = grid_blocks(n, kBlock);
  S.x = xo.dev;
  launch("cg_init", solve_spmv_kernel<kInit>, dim3(g_rows), dim3(kBlock), 0, S);
  S.nslab = g_rows;
  launch("cg_start", cg_start_kernel, dim3(1), dim3(kBlock), 0, S, o.rtol, o.atol, (int)o.max_iter);

  S.x = p.p;
  for (int it = 0; it < o.max_iter; ++it)
  {
    S.it = it;
    S.last = it + 1 == o.max_iter;
    S.launch = 3 * it;
    launch("cg_spmv", solve_spmv_kernel<kCg>, dim3(g_rows), dim3(kBlock), 0, S);
    S.launch = 3 * it + 1;
    S.nslab = g_rows;
    launch("cg_update", cg_update_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    S.launch = 3 * it + 2;
    S.nslab = g_vec;
    launch("cg_direction", cg_direction_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    // the host looks every check_every iterations; what it sees only ends the launches (the result is frozen in HBM)
    if (o.check_every > 0 && (it + 1) % o.check_every == 0 && !S.last && read_scalar(&rec.p->info.reason) != kRunning) break;
  }
  if (is_device_pointer(info))
    CFX_HIP(hipMemcpyAsync(info, &rec.p->info, sizeof(cfx_cg_info), hipMemcpyDeviceToDevice, ctx().stream));
  else
    *info = read_scalar(&rec.p->info);
  xo.finish();
  CFX_API_END
}

int cfx_minres_options_default(cfx_minres_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_minres_options_default: null argument");
  opt->rtol = 1e-10;
  opt->atol = 0.0;
  opt->max_iter = 10000;
  opt->check_every = 16;
  opt->precond = CFX_PC_ABS_JACOBI;
  opt->lanes_per_row = 0;
  CFX_API_END
}

int cfx_minres_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                     int64_t n_rows, const double* b, double* x, const cfx_minres_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  cfx_minres_options o;
  if (opt)
    o = *opt;
  else
    cfx_minres_options_default(&o);
  check_csr("cfx_minres_solve", nrows, indptr, indices, values, rows, n_rows, o.lanes_per_row);
  require(b && x && info, CFX_ERR_INVALID_ARGUMENT, "cfx_minres_solve: null b, x or info");
  require(o.rtol >= 0.0 && o.atol >= 0.0, CFX_ERR_INVALID_ARGUMENT, "cfx_minres_solve: rtol and atol are >= 0");
  require(o.max_iter >= 0 && o.check_every >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_minres_solve: max_iter and check_every are >= 0");
  require(o.max_iter <= 0x2aaaaaaa, CFX_ERR_INVALID_ARGUMENT, "cfx_minres_solve: max_iter too large");
  require(o.precond == CFX_PC_NONE || o.precond == CFX_PC_ABS_JACOBI || o.precond == CFX_PC_ABS_ROWSUM, CFX_ERR_INVALID_ARGUMENT,
          "cfx_minres_solve: precond is CFX_PC_NONE, CFX_PC_ABS_JACOBI or CFX_PC_ABS_ROWSUM");
  ctx().ensure();
  for (const void* p : {(const void*)indptr, (const void*)indices, (const void*)values})
    require_device("cfx_minres_solve", p, "the CSR arrays");
  if (rows) require_device("cfx_minres_solve", rows, "rows");

  const int64_t n = rows ? n_rows : nrows;
  const bool pc = o.precond != CFX_PC_NONE;
  DevArray<double> bd = to_device(b, nrows);
  OutArray<double> xo(x, nrows, true);
  // workspace from the block cache: v, v_old, q, w, w_old, 1/m by list position, z by row, two slabs, the record
  DevArray<double> va(n), vb(n), q(n), wa(n), wb(n), minv(pc ? n : 0), z(nrows), slabs(2 * (int64_t)kMaxGrid);
  DevArray<MinresRecord> rec(1);
  rec.zero();
  if (rows) z.zero(); // z stays 0 outside the list

  SolveArgs S{};
  S.indptr = indptr; S.indices = indices; S.values = values; S.rows = rows;
  S.n = n;
  S.lanes = o.lanes_per_row;
  S.rec = rec.p; S.mrec = rec.p;
  S.pc = o.precond;
  S.b = bd.p; S.xs = xo.dev; S.p = z.p; S.q = q.p;
  S.v = va.p; S.v_old = vb.p; S.w = wa.p; S.w_old = wb.p;
  S.dinv = pc ? minv.p : nullptr;
  S.slab0 = slabs.p; S.slab1 = slabs.p + kMaxGrid;
  if (S.lanes == 0) count_entries(S, nrows);

  const int g_rows = spmv_blocks(n), g_vec = grid_blocks(n, kBlock);
  S.x = xo.dev;
  launch("minres_init", solve_spmv_kernel<kMinresInit>, dim3(g_rows), dim3(kBlock), 0, S);
  S.nslab = g_rows;
  launch("minres_start", minres_start_kernel, dim3(1), dim3(kBlock), 0, S, o.rtol, o.atol, (int)o.max_iter);
  S.launch = 0;
  launch("minres_normalise", minres_normalise_kernel, dim3(g_vec), dim3(kBlock), 0, S);

  S.x = z.p;
  for (int it = 0; it < o.max_iter; ++it)
  {
    S.it = it;
    S.last = it + 1 == o.max_iter;
    S.v = it & 1 ? vb.p : va.p; S.v_old = it & 1 ? va.p : vb.p;
    S.w = it & 1 ? wb.p : wa.p; S.w_old = it & 1 ? wa.p : wb.p;
    S.launch = 3 * it + 1;
    launch("minres_spmv", solve_spmv_kernel<kCg>, dim3(g_rows), dim3(kBlock), 0, S);
    S.launch = 3 * it + 2;
    S.nslab = g_rows;
    launch("minres_lanczos", minres_lanczos_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    S.launch = 3 * it + 3;
    S.nslab = g_vec;
    launch("minres_update", minres_update_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    // the host looks every check_every iterations; what it sees only ends the launches (the result is frozen in HBM)
    if (o.check_every > 0 && (it + 1) % o.check_every == 0 && !S.last && read_scalar(&rec.p->info.reason) != kRunning) break;
  }
  if (is_device_pointer(info))
    CFX_HIP(hipMemcpyAsync(info, &rec.p->info, sizeof(cfx_cg_info), hipMemcpyDeviceToDevice, ctx().stream));
  else
    *info = read_scalar(&rec.p->info);
  xo.finish();
  CFX_API_END
}

int cfx_bicgstab_options_default(cfx_bicgstab_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_bicgstab_options_default: null argument");
  opt->rtol = 1e-10;
  opt->atol = 0.0;
  opt->max_iter = 10000;
  opt->check_every = 16;
  opt->precond = CFX_PC_JACOBI;
  opt->lanes_per_row = 0;
  CFX_API_END
}

int cfx_bicgstab_solve(int64_t nrows, const int64_t* indptr, const int32_t* indices, const double* values, const int32_t* rows,
                       int64_t n_rows, const double* b, double* x, const cfx_bicgstab_options* opt, cfx_cg_info* info)
{
  CFX_API_BEGIN
  cfx_bicgstab_options o;
  if (opt)
    o = *opt;
  else
    cfx_bicgstab_options_default(&o);
  check_csr("cfx_bicgstab_solve", nrows, indptr, indices, values, rows, n_rows, o.lanes_per_row);
  require(b && x && info, CFX_ERR_INVALID_ARGUMENT, "cfx_bicgstab_solve: null b, x or info");
  require(o.rtol >= 0.0 && o.atol >= 0.0, CFX_ERR_INVALID_ARGUMENT, "cfx_bicgstab_solve: rtol and atol are >= 0");
  require(o.max_iter >= 0 && o.check_every >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_bicgstab_solve: max_iter and check_every are >= 0");
  require(o.max_iter <= 0x19999999, CFX_ERR_INVALID_ARGUMENT, "cfx_bicgstab_solve: max_iter too large"); // (5 launches each)
  require(o.precond == CFX_PC_NONE || o.precond == CFX_PC_JACOBI, CFX_ERR_INVALID_ARGUMENT,
          "cfx_bicgstab_solve: precond is CFX_PC_NONE or CFX_PC_JACOBI");
  ctx().ensure();
  for (const void* p : {(const void*)indptr, (const void*)indices, (const void*)values})
    require_device("cfx_bicgstab_solve", p, "the CSR arrays");
  if (rows) require_device("cfx_bicgstab_solve", rows, "rows");

  const int64_t n = rows ? n_rows : nrows;
  const bool pc = o.precond == CFX_PC_JACOBI;
  DevArray<double> bd = to_device(b, nrows);
  OutArray<double> xo(x, nrows, true);
  // workspace from the block cache: r, rhat, v, t, p, 1/diag by list position, phat, shat by row, five slabs, the record
  DevArray<double> r(n), rhat(n), v(n), t(n), pl(n), dinv(pc ? n : 0), phat(nrows), shat(nrows), slabs(5 * (int64_t)kMaxGrid);
  DevArray<BicgRecord> rec(1);
  rec.zero();
  if (rows) // phat and shat stay 0 outside the list
  {
    phat.zero();
    shat.zero();
  }

  SolveArgs S{};
  S.indptr = indptr; S.indices = indices; S.values = values; S.rows = rows;
  S.n = n;
  S.lanes = o.lanes_per_row;
  S.rec = rec.p; S.brec = rec.p;
  S.b = bd.p; S.xs = xo.dev; S.r = r.p; S.rhat = rhat.p; S.q = v.p; S.t = t.p; S.pl = pl.p; S.p = phat.p; S.shat = shat.p;
  S.dinv = pc ? dinv.p : nullptr;
  S.slab0 = slabs.p; S.slab1 = slabs.p + kMaxGrid; S.slab2 = slabs.p + 2 * kMaxGrid;
  S.slab3 = slabs.p + 3 * kMaxGrid; S.slab4 = slabs.p + 4 * kMaxGrid;
  if (S.lanes == 0) count_entries(S, nrows);

  const int g_rows = spmv_blocks(n), g_vec = grid_blocks(n, kBlock);
  S.x = xo.dev;
  launch("bicg_init", solve_spmv_kernel<kBicgInit>, dim3(g_rows), dim3(kBlock), 0, S);
  S.nslab = g_rows;
  launch("bicg_start", bicg_start_kernel, dim3(1), dim3(kBlock), 0, S, o.rtol, o.atol, (int)o.max_iter);

  for (int it = 0; it < o.max_iter; ++it)
  {
    S.it = it;
    S.last = it + 1 == o.max_iter;
    S.launch = 5 * it;
    S.x = phat.p;
    launch("bicg_spmv_v", solve_spmv_kernel<kBicgV>, dim3(g_rows), dim3(kBlock), 0, S);
    S.launch = 5 * it + 1;
    S.nslab = g_rows;
    launch("bicg_half", bicg_half_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    S.launch = 5 * it + 2;
    S.x = shat.p;
    launch("bicg_spmv_t", solve_spmv_kernel<kBicgT>, dim3(g_rows), dim3(kBlock), 0, S);
    S.launch = 5 * it + 3;
    S.nslab = g_rows; // (t.t and t.s; s.s has one partial per block of bicg_half)
    launch("bicg_update", bicg_update_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    S.launch = 5 * it + 4;
    S.nslab = g_vec;
    launch("bicg_direction", bicg_direction_kernel, dim3(g_vec), dim3(kBlock), 0, S);
    // the host looks every check_every iterations; what it sees only ends the launches (the result is frozen in HBM)
    if (o.check_every > 0 && (it + 1) % o.check_every == 0 && !S.last && read_scalar(&rec.p->info.reason) != kRunning) break;
  }
  if (is_device_pointer(info))
    CFX_HIP(hipMemcpyAsync(info, &rec.p->info, sizeof(cfx_cg_info), hipMemcpyDeviceToDevice, ctx().stream));
  else
    *info = read_scalar(&rec.p->info);
  xo.finish();
  CFX_API_END
}

} // extern "C"
