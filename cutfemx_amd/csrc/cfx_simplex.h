// cutfemx_amd: the simplex geometry the rule kernels of cfx_rules.hip share.  Every helper keeps the operand order of
// the kernels it was taken from: the rules are pinned bit for bit (profiles/rules_refactor_fingerprint.json).
#pragma once

#include "cfx_cut.h"

namespace cfx
{

// sub-simplices of `part` in a sub-triangulation case (the three counts loaded, one selected: selecting the address and
// loading one cost cut_emit_kernel<3> four registers)
template <class Case>
__device__ __forceinline__ int sub_count(const Case& cs, int part)
{
  const int n_in = cs.n_in, n_out = cs.n_out, n_if = cs.n_if;
  return part == PART_IN ? n_in : (part == PART_OUT ? n_out : n_if);
}

// D! times the signed reference volume of the D-simplex with vertices V[0..D]
template <int D>
__device__ __forceinline__ double simplex_det(const double (*V)[D])
{
  if constexpr (D == 1) return V[1][0] - V[0][0];
  else if constexpr (D == 2)
    return (V[1][0] - V[0][0]) * (V[2][1] - V[0][1]) - (V[1][1] - V[0][1]) * (V[2][0] - V[0][0]);
  else
  {
    double a[3], b[3], e[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { a[d] = V[1][d] - V[0][d]; b[d] = V[2][d] - V[0][d]; e[d] = V[3][d] - V[0][d]; }
    return a[0] * (b[1] * e[2] - b[2] * e[1]) - a[1] * (b[0] * e[2] - b[2] * e[0]) + a[2] * (b[0] * e[1] - b[1] * e[0]);
  }
}

// physical measure factor of a facet with vertices xp[0..TDIM-1]: |x1 - x0| (segment) or |(x1 - x0) x (x2 - x0)| (triangle)
template <int TDIM>
__device__ __forceinline__ double facet_measure(const double (*xp)[TDIM])
{
  if constexpr (TDIM == 2)
  {
    const double dx = xp[1][0] - xp[0][0], dy = xp[1][1] - xp[0][1];
    return sqrt(dx * dx + dy * dy);
  }
  else
  {
    double a[3], b[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { a[d] = xp[1][d] - xp[0][d]; b[d] = xp[2][d] - xp[0][d]; }
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return sqrt(cx * cx + cy * cy + cz * cz);
  }
}

// out = x_0 + J X, J[d][t] = x_{t+1,d} - x_{0,d}: reference point X of the cell with vertices x
template <int TDIM>
__device__ __forceinline__ void to_physical(const double (*x)[TDIM], const double* X, double* out)
{
#pragma unroll
  for (int d = 0; d < TDIM; ++d)
  {
    double v = x[0][d];
#pragma unroll
    for (int t = 0; t < TDIM; ++t) v += (x[t + 1][d] - x[0][d]) * X[t];
    out[d] = v;
  }
}

// out = l_0 V_0 + sum_t xi_t V_{t+1}, l_0 = 1 - sum_t xi_t: reference point xi of the DIM-simplex with vertices V.
// The roundings are spelled out -- xi_0 V_1 rounded, l_0 V_0 fused onto it, every further term fused onto the sum --
// because "l0 * V[0][d] + xi[0] * V[1][d] + ..." leaves the choice of the product that is rounded to the compiler, which
// took this one at every site before they shared this function and the other one here.
template <int TDIM_OUT, int DIM>
__device__ __forceinline__ void bary_point(const double (*V)[TDIM_OUT], const double* xi, double* out)
{
  double l0 = 1.0;
#pragma unroll
  for (int t = 0; t < DIM; ++t) l0 -= xi[t];
#pragma unroll
  for (int d = 0; d < TDIM_OUT; ++d)
  {
    double v = __builtin_fma(l0, V[0][d], xi[0] * V[1][d]);
#pragma unroll
    for (int t = 1; t < DIM; ++t) v = __builtin_fma(xi[t], V[t + 1][d], v);
    out[d] = v;
  }
}

// reference coordinate of the zero of a P1 level set on a cut segment (mask 1: vertex 0 negative, 2: vertex 1):
// from the negative vertex a towards the other vertex b
__device__ __forceinline__ double segment_cut(const double* phi, int mask)
{
  const int a = mask == 1 ? 0 : 1;
  const double pa = a == 0 ? phi[0] : phi[1], pb = a == 0 ? phi[1] : phi[0];
  const double t = pa / (pa - pb);
  const double xa = a == 0 ? 0.0 : 1.0, xb = a == 0 ? 1.0 : 0.0;
  return xa + t * (xb - xa);
}

} // namespace cfx
