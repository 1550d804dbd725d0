// cutfemx_amd: the cell-local arithmetic of the reinitialisation (cfx_reinit.hip) -- the distances of a seed cell's
// vertices to its interface piece, and the update U(t, K) of one target from one cell.  Pure functions of a few doubles,
// __host__ __device__, no memory but their arguments: the kernels of cfx_reinit.hip call them, and so do the probes of
// tests/cpp (reinit_cell_probe.hip on the GPU, reinit_cell_host.cpp as plain host C++ without HIP).  The second half --
// where the minima are taken -- serves the normal extension (cfx_extend.hip; extension_cell_host.cpp on the host).
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

// ---- where the minima are taken: the arithmetic of the normal extension (cfx_extend.hip) ---------------------------------
// The functions above answer "how far"; the ones below answer "from where", as weights of the vertices involved, with the
// same arithmetic for the value itself.

// seg_dist2 with the parameter of the closest point a + t (b - a)
template <int D>
__host__ __device__ __forceinline__ double seg_closest(const double* p, const double* a, const double* b, double& t)
{
  double l2 = 0.0;
  t = 0.0;
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

// tri_dist2 with the closest point as weights w[3] of a, b, c: the first of ab, bc, ca, interior that attains the least
__host__ __device__ __forceinline__ double tri_closest(const double* p, const double* a, const double* b, const double* c, double* w)
{
  double t, r2 = seg_closest<3>(p, a, b, t);
  w[0] = 1.0 - t, w[1] = t, w[2] = 0.0;
  double r = seg_closest<3>(p, b, c, t);
  if (r < r2) r2 = r, w[0] = 0.0, w[1] = 1.0 - t, w[2] = t;
  r = seg_closest<3>(p, c, a, t);
  if (r < r2) r2 = r, w[0] = t, w[1] = 0.0, w[2] = 1.0 - t;
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
    double v[3], qa[3], qb[3], qc[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = p[k] - a[k];
    const double s = dot3(n, v);
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
      const double q = p[k] - n[k] * (s / nn);
      qa[k] = q - a[k];
      qb[k] = q - b[k];
      qc[k] = q - c[k];
    }
    cross3(ab, qa, x);
    const double e0 = dot3(x, n); // the areas opposite c, a, b
    cross3(bc, qb, x);
    const double e1 = dot3(x, n);
    double ca[3] = {-ac[0], -ac[1], -ac[2]};
    cross3(ca, qc, x);
    const double e2 = dot3(x, n);
    if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0 && s * s / nn < r2)
    {
      r2 = s * s / nn;
      const double sum = e0 + e1 + e2;
      w[0] = e1 / sum, w[1] = e2 / sum, w[2] = e0 / sum;
    }
  }
  return r2;
}

// crossing() with the ends and the parameter: p = (1 - t) x_i + t x_j, i the negative end
template <int D>
__host__ __device__ __forceinline__ void crossing_ends(const double (*X)[D], const double* f, int& i, int& j, double& t, double* p)
{
  if (!(f[i] < 0.0))
  {
    const int s = i;
    i = j;
    j = s;
  }
  t = f[i] / (f[i] - f[j]);
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = X[i][k] + t * (X[j][k] - X[i][k]);
}

// The point of a seed cell's piece closest to the cell's vertex `at`, as weights lam[NV] of the cell's vertices (>= 0, sum
// 1 up to rounding); returns the distance (seed_cell's dist[at]), or -1 when the cell is no seed cell.  The pieces, their
// crossing points and their order are seed_cell's.
template <int TDIM>
__host__ __device__ __forceinline__ double seed_closest(const double (*X)[TDIM], const double* f, int at, double* lam)
{
  constexpr int NV = TDIM + 1;
  int nneg = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i)
  {
    nneg += f[i] < 0.0 ? 1 : 0;
    lam[i] = 0.0;
  }
  if (nneg == 0 || nneg == NV) return -1.0;
  double P[4][TDIM], t[4], w[4] = {0.0, 0.0, 0.0, 0.0}, r2;
  int ei[4] = {0, 0, 0, 0}, ej[4] = {0, 0, 0, 0}, np;
  if constexpr (TDIM == 2)
  {
    const bool lone_neg = nneg == 1;
    int l = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if ((f[i] < 0.0) == lone_neg) l = i;
    ei[0] = ei[1] = l;
    ej[0] = (l + 1) % 3;
    ej[1] = (l + 2) % 3;
    crossing_ends<2>(X, f, ei[0], ej[0], t[0], P[0]);
    crossing_ends<2>(X, f, ei[1], ej[1], t[1], P[1]);
    np = 2;
    double s;
    r2 = seg_closest<2>(X[at], P[0], P[1], s);
    w[0] = 1.0 - s, w[1] = s;
  }
  else
  {
    np = 3;
    if (nneg == 2)
    {
      int neg[2] = {0, 0}, pos[2] = {0, 0}, a = 0, b = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
      {
        if (f[i] < 0.0) neg[a++] = i;
        else pos[b++] = i;
      }
      ei[0] = neg[0], ej[0] = pos[0];
      ei[1] = neg[0], ej[1] = pos[1];
      ei[2] = neg[1], ej[2] = pos[1];
      ei[3] = neg[1], ej[3] = pos[0];
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
        if (i != l) ei[q] = l, ej[q] = i, ++q;
    }
    for (int q = 0; q < np; ++q) crossing_ends<3>(X, f, ei[q], ej[q], t[q], P[q]);
    r2 = tri_closest(X[at], P[0], P[1], P[2], w);
    if (np == 4)
    {
      double w2[3];
      const double r = tri_closest(X[at], P[0], P[2], P[3], w2);
      if (r < r2) r2 = r, w[0] = w2[0], w[1] = 0.0, w[2] = w2[1], w[3] = w2[2];
    }
  }
  for (int q = 0; q < np; ++q)
#pragma unroll
    for (int i = 0; i < NV; ++i)
    {
      if (i == ei[q]) lam[i] += w[q] * (1.0 - t[q]);
      if (i == ej[q]) lam[i] += w[q] * t[q];
    }
  return sqrt(r2);
}

// pair_update with the weight of the second source at the minimiser (the first one has 1 - s)
template <int D>
__host__ __device__ __forceinline__ double pair_update_at(const double* p1, const double* p2, double d1, double d2, double inf, double& s)
{
  double e[D], ee = 0.0, pe = 0.0;
  s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    e[k] = p2[k] - p1[k];
    ee += e[k] * e[k];
    pe += p1[k] * e[k];
  }
  if (!(ee > 0.0)) return inf;
  const double ie = 1.0 / ee, dl = d2 - d1;
  const double gg = 1.0 - dl * dl * ie;
  if (!(gg > 0.0)) return inf;
  const double t0 = -pe * ie;
  double hh = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
  {
    const double z = p1[k] + t0 * e[k];
    hh += z * z;
  }
  const double hs = sqrt(hh * gg);
  s = t0 - (hs / gg) * dl * ie;
  return (s >= 0.0 && s <= 1.0) ? d1 + t0 * dl + hs : inf;
}

// triple_update with the weights of the second and third source at the minimiser
__host__ __device__ __forceinline__ double triple_update_at(const double (*P)[3], const double* dv, double inf, double& alpha, double& beta)
{
  double e1[3], e2[3], w[3], n[3];
  alpha = beta = 0.0;
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
  const double iw = 1.0 / ww, d1 = dv[1] - dv[0], dw = (dv[2] - dv[0]) - m * d1;
  const double gg = 1.0 - d1 * d1 * ia - dw * dw * iw;
  if (!(gg > 0.0)) return inf;
  cross3(e1, e2, n);
  const double p1 = dot3(P[0], e1), pw = dot3(P[0], w), pn = dot3(P[0], n);
  const double hs = sqrt(pn * pn * (ia * iw) * gg), rho = hs / gg;
  beta = -(pw + rho * dw) * iw;
  alpha = -(p1 + rho * d1) * ia - beta * m;
  return (alpha >= 0.0 && beta >= 0.0 && alpha + beta <= 1.0) ? dv[0] - (d1 * ia * p1 + dw * iw * pw) + hs : inf;
}

// cell_update with the place of a minimum: returns U, the same value as cell_update.  The sub-faces are walked in
// cell_update's order (single sources, pairs, the triple); the one reported is the FIRST whose value is <= limit, or, when
// none is, the first that attains U (limit = -infinity: always that one).  `value`: the reported sub-face's own value; lam[TDIM]:
// the weights of its minimiser y = sum lam_s x_s (0 for the sources outside the sub-face; >= 0, sum 1).  Without a usable
// source U = value = inf and lam = 0.
template <int TDIM>
__host__ __device__ __forceinline__ double cell_update_argmin(const double (*P)[TDIM], const double* dv, const bool* ok, double inf,
                                                              double limit, double& value, double* lam)
{
  double best = inf;
  bool within = false; // a sub-face <= limit is reported: later ones only lower `best`
  value = inf;
#pragma unroll
  for (int i = 0; i < TDIM; ++i) lam[i] = 0.0;
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
    if (ok[i])
    {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < TDIM; ++k) s += P[i][k] * P[i][k];
      const double u = dv[i] + sqrt(s);
      if (!within && (u <= limit || u < value))
      {
        value = u;
#pragma unroll
        for (int q = 0; q < TDIM; ++q) lam[q] = q == i ? 1.0 : 0.0;
        within = u <= limit;
      }
      best = fmin(best, u);
    }
#pragma unroll
  for (int i = 0; i < TDIM; ++i)
#pragma unroll
    for (int j = i + 1; j < TDIM; ++j)
      if (ok[i] && ok[j])
      {
        double s;
        const double u = pair_update_at<TDIM>(P[i], P[j], dv[i], dv[j], inf, s);
        if (!within && u < inf && (u <= limit || u < value))
        {
          value = u;
#pragma unroll
          for (int q = 0; q < TDIM; ++q) lam[q] = q == i ? 1.0 - s : (q == j ? s : 0.0);
          within = u <= limit;
        }
        best = fmin(best, u);
      }
  if constexpr (TDIM == 3)
    if (ok[0] && ok[1] && ok[2])
    {
      double alpha, beta;
      const double u = triple_update_at(P, dv, inf, alpha, beta);
      if (!within && u < inf && (u <= limit || u < value))
      {
        value = u;
        lam[0] = 1.0 - (alpha + beta), lam[1] = alpha, lam[2] = beta; // (alpha + beta <= 1 as computed: not negative)
      }
      best = fmin(best, u);
    }
  return best;
}

// the gradient of the P1 function f on the cell X, up to the positive factor 1 / |det|: its direction
template <int TDIM>
__host__ __device__ __forceinline__ void cell_gradient_direction(const double (*X)[TDIM], const double* f, double* g)
{
  if constexpr (TDIM == 2)
  {
    const double ax = X[1][0] - X[0][0], ay = X[1][1] - X[0][1], bx = X[2][0] - X[0][0], by = X[2][1] - X[0][1];
    const double d1 = f[1] - f[0], d2 = f[2] - f[0], det = ax * by - ay * bx, sg = det < 0.0 ? -1.0 : 1.0;
    g[0] = sg * (by * d1 - ay * d2);
    g[1] = sg * (ax * d2 - bx * d1);
  }
  else
  {
    double e[3][3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) e[i][k] = X[i + 1][k] - X[0][k];
    cross3(e[1], e[2], c);
    const double det = dot3(e[0], c), sg = det < 0.0 ? -1.0 : 1.0;
    const double d1 = f[1] - f[0], d2 = f[2] - f[0], d3 = f[3] - f[0];
    double c2[3], c3[3];
    cross3(e[2], e[0], c2);
    cross3(e[0], e[1], c3);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = sg * (d1 * c[k] + d2 * c2[k] + d3 * c3[k]);
  }
}

} // namespace reinit
} // namespace cfx
