// cutfemx_amd: the arithmetic of one cell visit of the characteristic walk (cfx_advect.hip) -- the barycentric
// coordinates of a target in a simplex, the decision "inside, or which facet to cross", and the P1 value there.  Pure
// functions of a few doubles, __host__ __device__, no memory but their arguments: advect_walk calls them, and so does
// tests/cpp/advect_cell_host.cpp as plain host C++ without HIP.
//
// Every operation is homogeneous in the coordinates: scaling the cell and the target by a power of two gives the same
// lambda bits, and inside_tol is compared with lambda, a ratio.
#pragma once

#include <cmath>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif

// No contraction into fused multiply-adds in this header: the host build, the device build and a plain IEEE model of
// the same operand order (tests/advect_ref.py) then give the same bits, and so the same walks.
#if defined(__clang__)
#define CFX_ADVECT_EXACT _Pragma("clang fp contract(off)")
#else
#define CFX_ADVECT_EXACT
#endif

namespace cfx
{
namespace advect
{
// det [a b] and det [a b c] (columns), in one fixed operand order
__host__ __device__ __forceinline__ double det2(const double* a, const double* b)
{
  CFX_ADVECT_EXACT
  return a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ __forceinline__ double det3(const double* a, const double* b, const double* c)
{
  CFX_ADVECT_EXACT
  return a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// lambda [TDIM + 1] of the target p in the cell with vertices X: Cramer's rule on the edge matrix E_j = X_j - X_0 with
// the right-hand side p - X_0; lambda_0 = 1 - the others (the sum is 1 up to the rounding of those additions).  A cell
// without volume gives infinities or NaNs, which visit() below reads as "not inside".
template <int TDIM>
__host__ __device__ __forceinline__ void barycentric(const double X[TDIM + 1][TDIM], const double* p, double* lam)
{
  CFX_ADVECT_EXACT
  double E[TDIM][TDIM], r[TDIM];
#pragma unroll
  for (int k = 0; k < TDIM; ++k)
  {
    r[k] = p[k] - X[0][k];
#pragma unroll
    for (int j = 0; j < TDIM; ++j) E[j][k] = X[j + 1][k] - X[0][k];
  }
  if constexpr (TDIM == 2)
  {
    const double det = det2(E[0], E[1]);
    lam[1] = det2(r, E[1]) / det;
    lam[2] = det2(E[0], r) / det;
    lam[0] = 1.0 - (lam[1] + lam[2]);
  }
  else
  {
    const double det = det3(E[0], E[1], E[2]);
    lam[1] = det3(r, E[1], E[2]) / det;
    lam[2] = det3(E[0], r, E[2]) / det;
    lam[3] = det3(E[0], E[1], r) / det;
    lam[0] = 1.0 - ((lam[1] + lam[2]) + lam[3]);
  }
}

// One visit: lambda of the target, and -1 when every lambda_i >= -inside_tol (the cell is found), else the local index
// of the facet to cross: the one opposite the most negative lambda, the lowest index on ties.  The comparisons are
// written so that a NaN is never "inside" and never moves the choice: a walk through NaNs ends at the step limit.
template <int TDIM>
__host__ __device__ __forceinline__ int visit(const double X[TDIM + 1][TDIM], const double* p, double inside_tol, double* lam)
{
  barycentric<TDIM>(X, p, lam);
  bool inside = true;
  int facet = 0;
  double least = lam[0];
#pragma unroll
  for (int i = 0; i <= TDIM; ++i)
  {
    inside = inside && (lam[i] >= -inside_tol);
    if (lam[i] < least)
    {
      least = lam[i];
      facet = i;
    }
  }
  return inside ? -1 : facet;
}

// sum lambda_i f_i with the unclamped lambda: inside the cell the P1 interpolant, outside it the cell's P1 extension
template <int TDIM>
__host__ __device__ __forceinline__ double interpolate(const double* lam, const double* f)
{
  CFX_ADVECT_EXACT
  double s = lam[0] * f[0];
#pragma unroll
  for (int i = 1; i <= TDIM; ++i) s += lam[i] * f[i];
  return s;
}

// x - t w, the point a vertex at x came from after the time t at the velocity w
template <int TDIM>
__host__ __device__ __forceinline__ void depart(const double* x, double t, const double* w, double* p)
{
  CFX_ADVECT_EXACT
#pragma unroll
  for (int k = 0; k < TDIM; ++k) p[k] = x[k] - t * w[k];
}
} // namespace advect
} // namespace cfx
