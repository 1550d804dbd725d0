// cutfemx_amd: the cell-local arithmetic of the reinitialisation (cfx_reinit.hip) -- the distances of a seed cell's
// vertices to its interface piece, and the update U(t, K) of one target from one cell.  Pure functions of a few doubles,
// __host__ __device__, no memory but their arguments: the kernels of cfx_reinit.hip call them, and so do the probes of
// tests/cpp (reinit_cell_probe.hip on the GPU, reinit_cell_host.cpp as plain host C++ without HIP).
#pragma once

#include <cmath>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace cfx
{
namespace reinit
{
constexpr double kDegenerate = 1e-9; // the update: a face of three sources whose sin^2 at the first one is not above it
constexpr double kFlatPiece = 1e-20; // the near field: an interface triangle this flat is its three edges

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
  if (nn > kFlatPiece * dot3(ab, ab) * dot3(ac, ac))
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

// ---- the update --------------------------------------------------------------------------------------------------------
// U over a sub-face, in the frame of the sub-face: with g the gradient of the interpolated d within the sub-face, h the
// height of the target over its plane (line) and z the foot of the perpendicular, the minimum over the plane is
//   U = d(z) + h sqrt(1 - |g|^2)   at   y = z - h g / sqrt(1 - |g|^2),
// valid when y lies in the sub-face (|g| >= 1: no minimum in the plane, a smaller sub-face holds it).  g and the
// position of y are conditioned like the sub-face; h comes from the components of a vector, so a target close to the
// plane -- a flat cell -- loses nothing: the errors are a few ulp of the cell's size whatever the cell's shape.

// two sources in D dimensions: p1, p2 = x_s - x_t
template <int D>
__host__ __device__ __forceinline__ double pair_update(const double* p1, const double* p2, double d1, double d2, double inf)
{
  double e[D], ee = 0.0, pe = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    e[k] = p2[k] - p1[k];
    ee += e[k] * e[k];
    pe += p1[k] * e[k];
  }
  if (!(ee > 0.0)) return inf; // coincident sources
  const double ie = 1.0 / ee, dl = d2 - d1;
  const double gg = 1.0 - dl * dl * ie; // 1 - |g|^2
  if (!(gg > 0.0)) return inf;
  const double t0 = -pe * ie; // z = p1 + t0 e
  double hh = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    const double z = p1[k] + t0 * e[k];
    hh += z * z;
  }
  const double hs = sqrt(hh * gg);
  const double s = t0 - (hs / gg) * dl * ie; // y = p1 + s e
  return (s >= 0.0 && s <= 1.0) ? d1 + t0 * dl + hs : inf;
}

// three sources: the frame is e1 = P1 - P0 and w = the part of e2 = P2 - P0 orthogonal to e1.  The face is degenerate
// when the sine of its angle at P0 is too small for g: sin^2 = |w|^2 / |e2|^2 <= kDegenerate
__host__ __device__ __forceinline__ double triple_update(const double (*P)[3], const double* dv, double inf)
{
  double e1[3], e2[3], w[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    e1[k] = P[1][k] - P[0][k];
    e2[k] = P[2][k] - P[0][k];
  }
  const double a = dot3(e1, e1), c = dot3(e2, e2);
  if (!(a > 0.0)) return inf;
  const double ia = 1.0 / a, m = dot3(e1, e2) * ia;
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = e2[k] - m * e1[k];
  const double ww = dot3(w, w);
  if (!(ww > kDegenerate * c)) return inf;
  const double iw = 1.0 / ww, d1 = dv[1] - dv[0], dw = (dv[2] - dv[0]) - m * d1; // g = (d1 / a) e1 + (dw / ww) w
  const double gg = 1.0 - d1 * d1 * ia - dw * dw * iw;
  if (!(gg > 0.0)) return inf;
  cross3(e1, e2, n); // |n|^2 = a ww
  const double p1 = dot3(P[0], e1), pw = dot3(P[0], w), pn = dot3(P[0], n);
  const double hs = sqrt(pn * pn * (ia * iw) * gg), rho = hs / gg;
  // y - P0 = alpha e1 + beta e2 = (alpha + beta m) e1 + beta w
  const double beta = -(pw + rho * dw) * iw, alpha = -(p1 + rho * d1) * ia - beta * m;
  return (alpha >= 0.0 && beta >= 0.0 && alpha + beta <= 1.0) ? dv[0] - (d1 * ia * p1 + dw * iw * pw) + hs : inf;
}

// U(t, K): P[s] = x_s - x_t and dv[s] for the TDIM other vertices of K, ok[s]: usable as a source
template <int TDIM>
__host__ __device__ __forceinline__ double cell_update(const double (*P)[TDIM], const double* dv, const bool* ok, double inf)
{
  double best = inf;
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
    if (ok[i])
    {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) s += P[i][k] * P[i][k];
      best = fmin(best, dv[i] + sqrt(s));
    }
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
#pragma unroll
    for (int j = i + 1; j < TDIM; ++j)
      if (ok[i] && ok[j]) best = fmin(best, pair_update<TDIM>(P[i], P[j], dv[i], dv[j], inf));
  if constexpr (TDIM == 3)
    if (ok[0] && ok[1] && ok[2]) best = fmin(best, triple_update(P, dv, inf));
  return best;
}

} // namespace reinit
} // namespace cfx
