// cutfemx_amd: everything that writes or reads a cfx_rules_s -- cut-cell sub-triangulation + runtime quadrature on
// cell hosts (one or several level sets) and on facet hosts, whole-cell / whole-facet rules, and the per-point
// evaluators -- HIP kernels for gfx950 and their C ABI.  The classified cut these start from is cfx_cut.hip.
//
// Replaces (paths relative to the CutFEMx tree):
//   cpp/cutfemx/cut/cut.cpp:845-868   update()  -> cutcells::cut        (a2)
//   cpp/cutfemx/cut/cut.cpp:1311-1335 runtime_quadrature()               (a3)
//   cpp/cutfemx/level_set/normal.h:39-187, value.h:34-119                (a12)
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "cfx_cut.h"
#include "cfx_device.h"
#include "cfx_simplex.h"

#define CFX_QUAD_TABLE_QUALIFIER static __device__ const
#include "cfx_quadrature_tables.h"
#undef CFX_QUAD_TABLE_QUALIFIER

using namespace cfx;

namespace cfx
{
// number of points of the reference rule of `degree` on a `dim`-simplex (cfx_quadhost.cpp)
int quad_npoints(int dim, int degree);
} // namespace cfx

namespace
{

// ---------------------------------------------------------------------------
// a2 sub-triangulation tables.  A vertex is "negative" iff phi < 0 (zeros side
// with the positive part).  Local point ids: 0..tdim parent vertices, then the
// cut points on edges (a negative, b non-negative).  Built once on the host.
// ---------------------------------------------------------------------------
struct CutCase
{
  int8_t n_in, n_out, n_if, npts;
  int8_t edge[4][2];
  int8_t in[3][4];
  int8_t out[3][4];
  int8_t iface[2][3];
};

__constant__ CutCase c_cases[2][16];

void prism(int8_t dst[3][4], int a0, int a1, int a2, int b0, int b1, int b2)
{
  const int t[3][4] = {{a0, a1, a2, b2}, {a0, a1, b1, b2}, {a0, b0, b1, b2}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) dst[i][j] = (int8_t)t[i][j];
}

CutCase make_case(int tdim, int mask)
{
  CutCase s;
  memset(&s, 0, sizeof(s));
  const int nv = tdim + 1;
  int neg[4], pos[4], nn = 0, np = 0;
  for (int v = 0; v < nv; ++v)
    if ((mask >> v) & 1) neg[nn++] = v; else pos[np++] = v;
  int npts = nv;
  auto cutp = [&](int a, int b)
  {
    s.edge[npts - nv][0] = (int8_t)a; s.edge[npts - nv][1] = (int8_t)b;
    return npts++;
  };
  auto set = [](int8_t* d, int a, int b, int c, int e = 0) { d[0] = (int8_t)a; d[1] = (int8_t)b; d[2] = (int8_t)c; d[3] = (int8_t)e; };
  auto set3 = [](int8_t* d, int a, int b, int c) { d[0] = (int8_t)a; d[1] = (int8_t)b; d[2] = (int8_t)c; };
  if (tdim == 2)
  {
    if (nn == 0) { s.n_out = 1; set(s.out[0], 0, 1, 2); }
    else if (nn == 3) { s.n_in = 1; set(s.in[0], 0, 1, 2); }
    else if (nn == 1)
    {
      const int a = neg[0], b0 = pos[0], b1 = pos[1];
      const int q0 = cutp(a, b0), q1 = cutp(a, b1);
      s.n_in = 1; set(s.in[0], a, q0, q1);
      s.n_out = 2; set(s.out[0], q0, b0, b1); set(s.out[1], q0, b1, q1);
      s.n_if = 1; set3(s.iface[0], q0, q1, 0);
    }
    else
    {
      const int a0 = neg[0], a1 = neg[1], b = pos[0];
      const int q0 = cutp(a0, b), q1 = cutp(a1, b);
      s.n_in = 2; set(s.in[0], a0, a1, q1); set(s.in[1], a0, q1, q0);
      s.n_out = 1; set(s.out[0], b, q0, q1);
      s.n_if = 1; set3(s.iface[0], q0, q1, 0);
    }
  }
  else
  {
    if (nn == 0) { s.n_out = 1; set(s.out[0], 0, 1, 2, 3); }
    else if (nn == 4) { s.n_in = 1; set(s.in[0], 0, 1, 2, 3); }
    else if (nn == 1)
    {
      const int a = neg[0];
      const int q0 = cutp(a, pos[0]), q1 = cutp(a, pos[1]), q2 = cutp(a, pos[2]);
      s.n_in = 1; set(s.in[0], a, q0, q1, q2);
      s.n_out = 3; prism(s.out, q0, q1, q2, pos[0], pos[1], pos[2]);
      s.n_if = 1; set3(s.iface[0], q0, q1, q2);
    }
    else if (nn == 3)
    {
      const int b = pos[0];
      const int q0 = cutp(neg[0], b), q1 = cutp(neg[1], b), q2 = cutp(neg[2], b);
      s.n_in = 3; prism(s.in, q0, q1, q2, neg[0], neg[1], neg[2]);
      s.n_out = 1; set(s.out[0], b, q0, q1, q2);
      s.n_if = 1; set3(s.iface[0], q0, q1, q2);
    }
    else
    {
      const int a0 = neg[0], a1 = neg[1], b0 = pos[0], b1 = pos[1];
      const int q00 = cutp(a0, b0), q01 = cutp(a0, b1), q10 = cutp(a1, b0), q11 = cutp(a1, b1);
      s.n_in = 3; prism(s.in, a0, q00, q01, a1, q10, q11);
      s.n_out = 3; prism(s.out, b0, q00, q10, b1, q01, q11);
      s.n_if = 2; set3(s.iface[0], q00, q01, q11); set3(s.iface[1], q00, q11, q10);
    }
  }
  s.npts = (int8_t)npts;
  return s;
}

CutCase h_cases[2][16];
bool g_cases_ready = false;

template <int TDIM>
__device__ __forceinline__ int sign_mask(const double* phi)
{
  int m = 0;
#pragma unroll
  for (int v = 0; v <= TDIM; ++v) m |= (phi[v] < 0.0) ? (1 << v) : 0;
  return m;
}

constexpr int kPackShift = cfx::kCountPackShift; // (points, rules) of a cut cell packed into one int64 (see cfx_runtime_quadrature)
constexpr int64_t kPackMask = (1ll << kPackShift) - 1;

// rules of a cut cell with ns sub-simplices in `part`: one per sub-facet of the interface, one for a volume part
__device__ __forceinline__ int rule_count(int part, int ns) { return part == PART_IF ? ns : (ns > 0 ? 1 : 0); }

// per cut cell: number of rules and points it will emit for each of the (one or two) parts asked for
struct CountParts
{
  int n;
  int part[2], nref[2];
  int64_t* packed[2];
};
template <int TDIM>
__global__ void __launch_bounds__(kBlock) cut_count_kernel(DevN ncut_d, const int32_t* __restrict__ cut_cells,
                                                           const int32_t* __restrict__ ls_dofmap,
                                                           const double* __restrict__ phi_v, CountParts P)
{
  const int64_t ncut = dev_n(ncut_d);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncut)
  {
    if (i < ncut_d.cap) // list shorter than its capacity: the scans run over the capacity
      for (int k = 0; k < P.n; ++k) P.packed[k][i] = 0;
    return;
  }
  const int64_t c = cut_cells[i];
  double phi[TDIM + 1];
#pragma unroll
  for (int v = 0; v <= TDIM; ++v) phi[v] = phi_v[ls_dofmap[c * (TDIM + 1) + v]];
  const CutCase& cs = c_cases[TDIM - 2][sign_mask<TDIM>(phi)];
  for (int k = 0; k < P.n; ++k)
  {
    const int part = P.part[k];
    const int ns = sub_count(cs, part);
    // points in the low kPackShift bits, rules above: one scan gives both offsets
    P.packed[k][i] = (int64_t)(ns * P.nref[k]) | ((int64_t)rule_count(part, ns) << kPackShift);
  }
}

// parent-reference coordinates of local point p of the cut case
template <int TDIM>
__device__ __forceinline__ void local_point(const CutCase& cs, int p, const double* phi, double* X)
{
#pragma unroll
  for (int d = 0; d < TDIM; ++d) X[d] = 0.0;
  if (p <= TDIM)
  {
#pragma unroll
    for (int d = 0; d < TDIM; ++d) X[d] = (p == d + 1) ? 1.0 : 0.0;
    return;
  }
  const int a = cs.edge[p - (TDIM + 1)][0], b = cs.edge[p - (TDIM + 1)][1];
  double pa = 0.0, pb = 0.0;
#pragma unroll
  for (int v = 0; v <= TDIM; ++v)
  {
    pa = (v == a) ? phi[v] : pa;
    pb = (v == b) ? phi[v] : pb;
  }
  const double t = pa / (pa - pb); // a negative, b non-negative: t in [0,1]
#pragma unroll
  for (int d = 0; d < TDIM; ++d)
  {
    const double xa = (a == d + 1) ? 1.0 : 0.0, xb = (b == d + 1) ? 1.0 : 0.0;
    X[d] = xa + t * (xb - xa);
  }
}

template <int TDIM>
__device__ __forceinline__ const double* ref_points(int dim, int degree, int& n, const double*& w)
{
  if (dim == 1)
  {
    n = cfx_quad_offset_1d[degree + 1] - cfx_quad_offset_1d[degree];
    w = cfx_quad_weights_1d + cfx_quad_offset_1d[degree];
    return cfx_quad_points_1d + cfx_quad_offset_1d[degree];
  }
  if (dim == 2)
  {
    n = cfx_quad_offset_2d[degree + 1] - cfx_quad_offset_2d[degree];
    w = cfx_quad_weights_2d + cfx_quad_offset_2d[degree];
    return cfx_quad_points_2d + 2 * cfx_quad_offset_2d[degree];
  }
  n = cfx_quad_offset_3d[degree + 1] - cfx_quad_offset_3d[degree];
  w = cfx_quad_weights_3d + cfx_quad_offset_3d[degree];
  return cfx_quad_points_3d + 3 * cfx_quad_offset_3d[degree];
}

// ---------------------------------------------------------------------------
// a3 with several level sets: runtime_quadrature(cut([phi, phi1, ...]), "phi<0 and phi1>0", k)
// (cpp/cutfemx/cut/cut.h:122-181, docs/user-guide/element-classification.md:145-160).  One conjunction of
// clauses; each P1 level set is planar inside a cell, so the cell's part of the region is the parent simplex
// clipped by one half-space per clause, in the order the clauses are written: every simplex of the current list
// is sub-triangulated with the single-level-set case tables (phi_k interpolated at its vertices) and its negative
// ("<") or positive (">") part kept.  With an "=0" clause the list starts from that level set's
// interface sub-facets and the other clauses clip them.  One thread per rule cell, the simplex lists in
// private memory: a few thousand cells along the curves / surfaces where two level sets meet, not a hot path.
// ---------------------------------------------------------------------------
constexpr int kMultiMaxClauses = 4; // clauses of a conjunction (at most 3 of them clip)
constexpr int kMultiMaxSimp = 27;   // 3 clips of 3 sub-simplices each

struct MultiArgs
{
  int64_t n;                  // rule cells
  const int32_t* cells;
  const double* x;
  const int32_t* conn;
  const int32_t* ls_dofmap;
  const double* phi[kMultiMaxClauses]; // dof values of the clause's level set
  int ncl, eq;                // eq: index of the "=0" clause or -1
  int mask[kMultiMaxClauses];
  int order;
  int64_t* packed;            // count pass: (points | rules << kPackShift) per cell
  const int64_t* packed_off;  // emit pass
  double* points;
  double* weights;
  int32_t* offsets;
  int32_t* parent_map;
};

struct MultiRuleCell
{
  const int8_t* domain;
  int64_t ncells;
  int ncl;
  int ls[kMultiMaxClauses], mask[kMultiMaxClauses];
  __device__ bool operator()(int64_t c) const
  {
    bool ok = true, any_cut = false;
    for (int k = 0; k < ncl; ++k)
    {
      const int d = domain[(int64_t)ls[k] * ncells + c];
      if (d == CFX_INTERSECTED) any_cut = true;
      else if (d == CFX_NOT_CANDIDATE || mask[k] == 2 || !((mask[k] >> (d + 1)) & 1)) ok = false;
    }
    return ok && any_cut;
  }
};

template <int TDIM>
struct MSimp
{
  double V[TDIM + 1][TDIM]; // vertices in parent reference coordinates (DIM + 1 of them used)
};

// the psi < 0 part (keep_out false) or the psi > 0 part (keep_out: the "out" simplices of the same case, so that a
// ">" clause triangulates exactly like the single-level-set "phi>0" rules) of simplex `in` (dimension DIM),
// appended to out[m...]; returns the new m
template <int TDIM, int DIM>
__device__ int multi_clip_one(const MSimp<TDIM>& in, const double* psi, bool keep_out, MSimp<TDIM>* out, int m)
{
  if constexpr (DIM == 1)
  {
    const bool n0 = psi[0] < 0.0, n1 = psi[1] < 0.0;
    if (n0 == n1)
    {
      if (n0 != keep_out) { out[m] = in; return m + 1; } // wholly on the kept side
      return m;
    }
    // a = the negative end, b = the other; cut point q; negative part (a, q), positive part (q, b)
    const int a = n0 ? 0 : 1, b = 1 - a;
    const double t = psi[a] / (psi[a] - psi[b]);
    const double La = (a == 1) ? 1.0 : 0.0, Lb = (b == 1) ? 1.0 : 0.0; // local coordinate of the two ends
    const double Lq = La + t * (Lb - La);
    const double L0 = keep_out ? Lq : La, L1 = keep_out ? Lb : Lq;
#pragma unroll
    for (int d = 0; d < TDIM; ++d)
    {
      out[m].V[0][d] = in.V[0][d] + L0 * (in.V[1][d] - in.V[0][d]);
      out[m].V[1][d] = in.V[0][d] + L1 * (in.V[1][d] - in.V[0][d]);
    }
    return m + 1;
  }
  else
  {
    int sm = 0;
#pragma unroll
    for (int v = 0; v <= DIM; ++v) sm |= (psi[v] < 0.0) ? (1 << v) : 0;
    if (sm == (keep_out ? 0 : (1 << (DIM + 1)) - 1)) { out[m] = in; return m + 1; } // wholly on the kept side: unchanged
    const CutCase& cs = c_cases[DIM - 2][sm];
    const int ns = keep_out ? cs.n_out : cs.n_in;
    for (int k = 0; k < ns; ++k)
    {
      for (int v = 0; v <= DIM; ++v)
      {
        double L[DIM];
        local_point<DIM>(cs, keep_out ? cs.out[k][v] : cs.in[k][v], psi, L); // the sub-simplex vertex in the coordinates of `in`
#pragma unroll
        for (int d = 0; d < TDIM; ++d)
        {
          double xx = in.V[0][d];
#pragma unroll
          for (int t = 0; t < DIM; ++t) xx += L[t] * (in.V[t + 1][d] - in.V[0][d]);
          out[m].V[v][d] = xx;
        }
      }
      ++m;
    }
    return m;
  }
}

template <int TDIM>
__device__ __forceinline__ double multi_phi_at(const double* phi, const double* X)
{
  double l0 = 1.0;
#pragma unroll
  for (int t = 0; t < TDIM; ++t) l0 -= X[t];
  double v = l0 * phi[0];
#pragma unroll
  for (int t = 0; t < TDIM; ++t) v += X[t] * phi[t + 1];
  return v;
}

// DIM = TDIM: volume rules; DIM = TDIM - 1: rules on the interface of clause A.eq
template <int TDIM, int DIM, bool EMIT>
__global__ void __launch_bounds__(kBlock) multi_rules_kernel(MultiArgs A)
{
  constexpr int NV = TDIM + 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const int64_t c = A.cells[i];
  double phi[kMultiMaxClauses][NV];
  for (int k = 0; k < A.ncl; ++k)
#pragma unroll
    for (int v = 0; v < NV; ++v) phi[k][v] = A.phi[k][A.ls_dofmap[c * NV + v]];
  // base list: the parent simplex, or the interface sub-facets of the "=0" level set
  MSimp<TDIM> base[2];
  int nbase = 1;
  if constexpr (DIM == TDIM)
  {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int d = 0; d < TDIM; ++d) base[0].V[v][d] = (v == d + 1) ? 1.0 : 0.0;
  }
  else
  {
    const CutCase& cs = c_cases[TDIM - 2][sign_mask<TDIM>(phi[A.eq])];
    nbase = cs.n_if;
    for (int f = 0; f < nbase; ++f)
      for (int v = 0; v < TDIM; ++v) local_point<TDIM>(cs, cs.iface[f][v], phi[A.eq], base[f].V[v]);
  }
  int nref;
  const double* wref;
  const double* pref = ref_points<TDIM>(DIM, A.order, nref, wref);
  Geo<TDIM> g;
  int64_t pq = 0, pr = 0;
  if constexpr (EMIT)
  {
    load_cell<TDIM>(A.x, A.conn, c, g);
    jacobian<TDIM>(g);
    const int64_t po = A.packed_off[i];
    pq = po & kPackMask; pr = po >> kPackShift;
  }
  int total_pts = 0, total_rules = 0;
  const int ngroups = DIM == TDIM ? 1 : nbase;
  MSimp<TDIM> la[kMultiMaxSimp], lb[kMultiMaxSimp];
  for (int gi = 0; gi < ngroups; ++gi)
  {
    MSimp<TDIM>* cur = la;
    MSimp<TDIM>* nxt = lb;
    int n = 1;
    cur[0] = base[gi];
    for (int k = 0; k < A.ncl && n > 0; ++k)
    {
      if (k == A.eq) continue;
      const bool keep_out = !(A.mask[k] & 1);
      int m = 0;
      for (int q = 0; q < n; ++q)
      {
        double psi[DIM + 1];
#pragma unroll
        for (int v = 0; v <= DIM; ++v) psi[v] = multi_phi_at<TDIM>(phi[k], cur[q].V[v]);
        m = multi_clip_one<TDIM, DIM>(cur[q], psi, keep_out, nxt, m);
      }
      n = m;
      MSimp<TDIM>* t = cur; cur = nxt; nxt = t;
    }
    if (n == 0) continue;
    total_rules += 1;
    total_pts += n * nref;
    if constexpr (EMIT)
    {
      for (int q = 0; q < n; ++q)
      {
        double scale;
        if constexpr (DIM == TDIM) scale = fabs(simplex_det<TDIM>(cur[q].V)) * fabs(g.detJ);
        else
        {
          double xp[TDIM][TDIM]; // physical vertices of the piece
#pragma unroll
          for (int v = 0; v < TDIM; ++v) to_physical<TDIM>(g.x, cur[q].V[v], xp[v]);
          scale = facet_measure<TDIM>(xp);
        }
        for (int r = 0; r < nref; ++r)
        {
          double X[TDIM];
          bary_point<TDIM, DIM>(cur[q].V, pref + r * DIM, X);
#pragma unroll
          for (int d = 0; d < TDIM; ++d) A.points[(pq + r) * TDIM + d] = X[d];
          A.weights[pq + r] = wref[r] * scale;
        }
        pq += nref;
      }
      A.parent_map[pr] = (int32_t)c;
      A.offsets[pr + 1] = (int32_t)pq;
      ++pr;
    }
  }
  if constexpr (!EMIT) A.packed[i] = (int64_t)total_pts | ((int64_t)total_rules << kPackShift);
}

#ifndef CFX_EMIT_LANES
#define CFX_EMIT_LANES 4
#endif
constexpr int kEmitLanes = CFX_EMIT_LANES; // lanes per cut cell (64 = one wavefront per cell)
static_assert(kEmitLanes >= 4 && 64 % kEmitLanes == 0, "lanes 0..tdim of a group stage the cell's vertices");

// ---------------------------------------------------------------------------
// a2+a3 emit: a lane group per cut cell.  Lanes 0..tdim stage the cell's
// vertex coordinates and level-set values in LDS; every lane then owns one
// (sub-simplex, reference point) pair, so the wave writes one contiguous run
// of points/weights.  points = parent-reference coords; weights = physical
// measure (w_ref |det sub->parent| |det parent->phys|, surface measure for the
// interface).  Volume parts: one rule per cut cell; interface: one rule per
// sub-facet (cut.cpp:1286-1294).
// ---------------------------------------------------------------------------
struct EmitJobs
{
  int n;
  int part[2];
  const int64_t* packed_off[2];
  double* points[2];
  double* weights[2];
  int32_t* offsets[2];
  int32_t* parent_map[2];
};

// reference point xi of a sub-simplex of a cut cell in the cell's reference coordinates (-> X); returns the sub-simplex's
// physical measure factor.  DIM = TDIM: a sub-simplex of a volume part; DIM = TDIM - 1: a sub-facet of the interface.
// sub: its DIM + 1 local points; P: the cell's local points; detJ: |det| of the cell's Jacobian
template <int TDIM, int DIM>
__device__ __forceinline__ double emit_point(const int8_t* sub, const double (*P)[TDIM], const Geo<TDIM>& g, double detJ,
                                             const double* xi, double* X)
{
  double V[DIM + 1][TDIM];
#pragma unroll
  for (int j = 0; j <= DIM; ++j)
  {
    const int p = sub[j];
#pragma unroll
    for (int d = 0; d < TDIM; ++d) V[j][d] = P[p][d];
  }
  double scale;
  if constexpr (DIM == TDIM) scale = fabs(simplex_det<TDIM>(V)) * detJ;
  else
  {
    double xp[TDIM][TDIM]; // physical sub-facet vertices -> surface measure
#pragma unroll
    for (int j = 0; j < TDIM; ++j) to_physical<TDIM>(g.x, V[j], xp[j]);
    scale = facet_measure<TDIM>(xp);
  }
  bary_point<TDIM, DIM>(V, xi, X);
  return scale;
}

// one rule set of a cut cell: its points and weights by the lane group, its rule rows by lane 0.  po: the cell's packed
// (point, rule) offsets in the set; last: the cell is the last of the cut list
template <int TDIM>
__device__ __forceinline__ void emit_rule_set(const CutCase& cs, int part, int64_t po, bool last, int64_t c,
                                              const double (*P)[TDIM], Geo<TDIM>& g, int degree, int lane,
                                              double* __restrict__ points, double* __restrict__ weights,
                                              int32_t* __restrict__ offsets, int32_t* __restrict__ parent_map)
{
  const int ns = sub_count(cs, part);
  const int nrules = rule_count(part, ns);
  // the last cut cell closes the parent list with a sentinel (the list is allocated one entry longer): kernels that
  // walk "the rules of cell c" stop there without knowing the number of rules, which may still be in HBM
  if (lane == 0 && last) parent_map[(po >> kPackShift) + nrules] = -1;
  if (ns == 0) return;
  int nref;
  const double* wref;
  const double* pref = ref_points<TDIM>(part == PART_IF ? TDIM - 1 : TDIM, degree, nref, wref);
  const int npts = ns * nref;
  const int32_t pbase = (int32_t)(po & kPackMask), rbase = (int32_t)(po >> kPackShift);
  jacobian<TDIM>(g);
  const double detJ = fabs(g.detJ);
  for (int pt = lane; pt < npts; pt += kEmitLanes)
  {
    const int k = pt / nref, q = pt - k * nref;
    double* X = points + (int64_t)(pbase + pt) * TDIM;
    double scale;
    if (part == PART_IF) scale = emit_point<TDIM, TDIM - 1>(cs.iface[k], P, g, detJ, pref + (TDIM - 1) * q, X);
    else scale = emit_point<TDIM, TDIM>(part == PART_IN ? cs.in[k] : cs.out[k], P, g, detJ, pref + TDIM * q, X);
    weights[pbase + pt] = wref[q] * scale;
  }
  if (lane == 0)
  {
    if (rbase == 0) offsets[0] = 0; // (the first rule's first point: this cell opens the rule set)
    const int per_rule = part == PART_IF ? nref : npts;
    for (int f = 0; f < nrules; ++f)
    {
      parent_map[rbase + f] = (int32_t)c;
      offsets[rbase + f + 1] = pbase + (f + 1) * per_rule;
    }
  }
}

#ifndef CFX_EMIT_WAVES
#define CFX_EMIT_WAVES 4 // waves per SIMD the emit kernel is compiled for (112 registers in 3-D without a bound: 4)
#endif
template <int TDIM>
__global__ void __launch_bounds__(kBlock, CFX_EMIT_WAVES) cut_emit_kernel(
    DevN ncut_d, const int32_t* __restrict__ cut_cells, const double* __restrict__ x,
    const int32_t* __restrict__ conn, const int32_t* __restrict__ ls_dofmap, const double* __restrict__ phi_v,
    int degree, EmitJobs jobs)
{
  const int64_t ncut = dev_n(ncut_d);
  constexpr int NV = TDIM + 1;
  // kEmitLanes lanes share one cut cell (16 cells per wavefront): a cell emits
  // 6-42 points; measured at 256^3: 64 lanes 705 us, 32 -> 445, 16 -> 293, 8 -> 247: more cells in
  // flight wins for this latency-bound kernel; with the local points staged in LDS, at 512^3:
  // 16 lanes 928 us, 8 -> 763, 4 -> 648
  __shared__ double s_phi[kBlock / kEmitLanes][NV];
  __shared__ double s_x[kBlock / kEmitLanes][NV][TDIM];
  const int wave = threadIdx.x / kEmitLanes, lane = threadIdx.x % kEmitLanes; // group, lane in group
  const int64_t i = (int64_t)blockIdx.x * (kBlock / kEmitLanes) + wave;
  const bool live = i < ncut;
  const int64_t c = live ? cut_cells[i] : 0;
  if (live && lane < NV)
  {
    const int64_t v = conn[c * NV + lane];
    s_phi[wave][lane] = phi_v[ls_dofmap[c * NV + lane]];
#pragma unroll
    for (int d = 0; d < TDIM; ++d) s_x[wave][lane][d] = x[3 * v + d];
  }
  __syncthreads();

  double phi[NV];
  Geo<TDIM> g;
#pragma unroll
  for (int v = 0; v < NV; ++v)
  {
    phi[v] = s_phi[wave][v];
#pragma unroll
    for (int d = 0; d < TDIM; ++d) g.x[v][d] = s_x[wave][v][d];
  }
  const CutCase& cs = c_cases[TDIM - 2][sign_mask<TDIM>(phi)];
  // the cell's local points (vertices + edge cut points, at most 2 NV) once per cell: one lane each, so the
  // division of a cut point is done once instead of once per (quadrature point, sub-simplex vertex)
  __shared__ double s_P[kBlock / kEmitLanes][2 * NV][TDIM];
  if (live)
    for (int p = lane; p < cs.npts; p += kEmitLanes)
    {
      double X[TDIM];
      local_point<TDIM>(cs, p, phi, X);
#pragma unroll
      for (int d = 0; d < TDIM; ++d) s_P[wave][p][d] = X[d];
    }
  __syncthreads();
  if (!live) return;
  // one or two rule sets of the same cut (runtime_quadratures: e.g. "phi<0" and "phi=0"): the staging above is shared
  // (the offsets of both sets are requested before the first store: a load issued behind the first set's stores waits
  // for them -- vmcnt counts loads and stores in order on this architecture)
  int64_t po[2];
#pragma unroll
  for (int job = 0; job < 2; ++job) po[job] = job < jobs.n ? jobs.packed_off[job][i] : 0;
  for (int job = 0; job < jobs.n; ++job)
    emit_rule_set<TDIM>(cs, jobs.part[job], job == 0 ? po[0] : po[1], i == ncut - 1, c, s_P[wave], g, degree, lane,
                        jobs.points[job], jobs.weights[job], jobs.offsets[job], jobs.parent_map[job]);
}

// whole-cell rules: reference points, weights * |detJ|
// (python/tests/quadrature_utils.py:40-61)
template <int TDIM>
__global__ void __launch_bounds__(kBlock) full_rules_kernel(int64_t n, const int32_t* __restrict__ cells,
                                                            const double* __restrict__ x,
                                                            const int32_t* __restrict__ conn, int degree,
                                                            double* __restrict__ points, double* __restrict__ weights,
                                                            int32_t* __restrict__ offsets, int32_t* __restrict__ parent_map)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Geo<TDIM> g;
  load_cell<TDIM>(x, conn, cells[i], g);
  jacobian<TDIM>(g);
  int nref;
  const double* wref;
  const double* pref = ref_points<TDIM>(TDIM, degree, nref, wref);
  const double detJ = fabs(g.detJ);
  for (int q = 0; q < nref; ++q)
  {
#pragma unroll
    for (int d = 0; d < TDIM; ++d) points[(i * nref + q) * TDIM + d] = pref[q * TDIM + d];
    weights[i * nref + q] = wref[q] * detJ;
  }
  parent_map[i] = cells[i];
  offsets[i + 1] = (int32_t)((i + 1) * nref);
  if (i == 0) offsets[0] = 0;
}

// rule index of point q: largest r with offsets[r] <= q
__device__ __forceinline__ int64_t rule_of_point(const int32_t* __restrict__ offsets, int64_t nr, int64_t q)
{
  int64_t lo = 0, hi = nr; // offsets[lo] <= q < offsets[hi]
  while (hi - lo > 1)
  {
    const int64_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= q) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------
// a12 per-point evaluators (P1 level set over P1 geometry): one thread per
// point.  normal = sign * K^T grad_ref(phi) / max(|.|, 1e-14)
// (cpp/cutfemx/level_set/normal.h:150-186)
// ---------------------------------------------------------------------------
// one thread per rule: the normal of a P1 level set over P1 geometry is constant on the parent cell,
// so it is formed once per rule and written to the rule's points (no search of the rule, one cell load)
template <int TDIM>
__global__ void __launch_bounds__(kBlock) normals_rule_kernel(DevN nr_d, const int32_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ parent_map,
                                                              const double* __restrict__ x, const int32_t* __restrict__ conn,
                                                              const int32_t* __restrict__ ls_dofmap,
                                                              const double* __restrict__ phi_v, double sign,
                                                              double* __restrict__ out)
{
  const int64_t nr = dev_n(nr_d);
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nr) return;
  const int64_t c = parent_map[r];
  Geo<TDIM> g;
  load_cell<TDIM>(x, conn, c, g);
  jacobian<TDIM>(g);
  double phi[TDIM + 1];
#pragma unroll
  for (int v = 0; v <= TDIM; ++v) phi[v] = phi_v[ls_dofmap[c * (TDIM + 1) + v]];
  double gref[TDIM], gp[TDIM];
#pragma unroll
  for (int t = 0; t < TDIM; ++t) gref[t] = phi[t + 1] - phi[0];
  double norm = 0.0;
#pragma unroll
  for (int d = 0; d < TDIM; ++d)
  {
    double v = 0.0;
#pragma unroll
    for (int t = 0; t < TDIM; ++t) v += g.K[t][d] * gref[t];
    gp[d] = v;
    norm += v * v;
  }
  norm = sqrt(norm);
  if (norm < 1.0e-14) norm = 1.0e-14;
#pragma unroll
  for (int d = 0; d < TDIM; ++d) gp[d] = sign * gp[d] / norm;
  for (int64_t q = offsets[r]; q < offsets[r + 1]; ++q)
  {
#pragma unroll
    for (int d = 0; d < TDIM; ++d) out[q * TDIM + d] = gp[d];
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) values_kernel(int64_t nq, int64_t nr, const int32_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ parent_map,
                                                        const double* __restrict__ points,
                                                        const int32_t* __restrict__ ls_dofmap,
                                                        const double* __restrict__ phi_v, double* __restrict__ out)
{
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= nq) return;
  const int64_t c = parent_map[rule_of_point(offsets, nr, q)];
  double l0 = 1.0, v = 0.0;
#pragma unroll
  for (int t = 0; t < TDIM; ++t)
  {
    const double X = points[q * TDIM + t];
    l0 -= X;
    v += X * phi_v[ls_dofmap[c * (TDIM + 1) + t + 1]];
  }
  out[q] = v + l0 * phi_v[ls_dofmap[c * (TDIM + 1)]];
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) physical_points_kernel(int64_t nq, int64_t nr,
                                                                 const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ parent_map,
                                                                 const double* __restrict__ points,
                                                                 const double* __restrict__ x,
                                                                 const int32_t* __restrict__ conn,
                                                                 double* __restrict__ out)
{
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= nq) return;
  const int64_t c = parent_map[rule_of_point(offsets, nr, q)];
  Geo<TDIM> g;
  load_cell<TDIM>(x, conn, c, g);
  double X[TDIM], xq[TDIM];
#pragma unroll
  for (int t = 0; t < TDIM; ++t) X[t] = points[q * TDIM + t];
  bary_point<TDIM, TDIM>(g.x, X, xq);
#pragma unroll
  for (int d = 0; d < TDIM; ++d) out[q * TDIM + d] = xq[d];
}

// ---------------------------------------------------------------------------
// 8f-4 rules on facet hosts (cut.cpp:540-591, 788-830; the hosts themselves: facet_hosts_kernel, cfx_cut.hip).  The
// sub-triangulation of a host is the (tdim-1)-dimensional marching case of its P1 level-set values; points live on
// the host's reference simplex, weights carry the physical measure.
// ---------------------------------------------------------------------------
// sub-simplices of a host of dimension HD with sign mask `mask` in `part`
template <int HD>
__device__ __forceinline__ int host_subcount(int mask, int part)
{
  if constexpr (HD == 1)
  {
    const int nn = __popc(mask & 3);
    if (part == PART_IF) return nn == 1 ? 1 : 0; // the cut point
    return part == PART_IN ? (nn >= 1 ? 1 : 0) : (nn <= 1 ? 1 : 0);
  }
  else
    return sub_count(c_cases[0][mask & 7], part);
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_count_kernel(int64_t ncut, const int32_t* __restrict__ cut_hosts,
                                                             const int32_t* __restrict__ ls, const double* __restrict__ phi_v,
                                                             int part, int nref, int32_t* __restrict__ n_rules,
                                                             int32_t* __restrict__ n_points)
{
  constexpr int HD = TDIM - 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncut) return;
  const int64_t h = cut_hosts[i];
  double phi[HD + 1];
#pragma unroll
  for (int v = 0; v <= HD; ++v) phi[v] = phi_v[ls[h * TDIM + v]];
  const int ns = host_subcount<HD>(sign_mask<HD>(phi), part);
  n_rules[i] = ns > 0 ? 1 : 0;
  n_points[i] = ns * nref;
}

// one thread per cut host (there are O(N^(tdim-2)) .. O(N^(tdim-1)) of them): one rule per host
template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_emit_kernel(
    int64_t ncut, const int32_t* __restrict__ cut_hosts, const double* __restrict__ x, const int32_t* __restrict__ verts,
    const int32_t* __restrict__ ls, const double* __restrict__ phi_v, const int32_t* __restrict__ host_ids, int part,
    int degree, const int32_t* __restrict__ rule_off, const int32_t* __restrict__ point_off, double* __restrict__ points,
    double* __restrict__ weights, int32_t* __restrict__ offsets, int32_t* __restrict__ parent_map,
    int32_t* __restrict__ rule_host)
{
  constexpr int HD = TDIM - 1, NV = HD + 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncut) return;
  const int64_t h = cut_hosts[i];
  double phi[NV], xv[NV][TDIM];
#pragma unroll
  for (int v = 0; v < NV; ++v)
  {
    phi[v] = phi_v[ls[h * TDIM + v]];
    const int64_t g = verts[h * TDIM + v];
#pragma unroll
    for (int d = 0; d < TDIM; ++d) xv[v][d] = x[3 * g + d];
  }
  const int mask = sign_mask<HD>(phi);
  const int ns = host_subcount<HD>(mask, part);
  if (ns == 0) return;
  const double measure = facet_measure<TDIM>(xv);
  const int32_t pbase = point_off[i], rbase = rule_off[i];
  if (part == PART_IF)
  {
    // the set phi = 0 on the host (codimension 2 in the mesh): a point of a segment host (weight 1), a
    // straight segment across a triangle host (1-D rule, weights carry its physical length)
    if constexpr (HD == 1)
    {
      points[pbase] = segment_cut(phi, mask);
      weights[pbase] = 1.0;
      offsets[rbase + 1] = pbase + 1;
    }
    else
    {
      const CutCase& cs = c_cases[0][mask & 7];
      double V[2][HD], xp[2][TDIM];
#pragma unroll
      for (int j = 0; j < 2; ++j)
      {
        local_point<2>(cs, cs.iface[0][j], phi, V[j]);
        bary_point<TDIM, HD>(xv, V[j], xp[j]);
      }
      double len = 0.0;
#pragma unroll
      for (int d = 0; d < TDIM; ++d) len += (xp[1][d] - xp[0][d]) * (xp[1][d] - xp[0][d]);
      len = sqrt(len);
      int n1;
      const double* w1;
      const double* p1 = ref_points<TDIM>(1, degree, n1, w1);
      for (int q = 0; q < n1; ++q)
      {
#pragma unroll
        for (int d = 0; d < HD; ++d) points[(int64_t)(pbase + q) * HD + d] = V[0][d] + p1[q] * (V[1][d] - V[0][d]);
        weights[pbase + q] = w1[q] * len;
      }
      offsets[rbase + 1] = pbase + n1;
    }
    parent_map[rbase] = host_ids[h];
    rule_host[rbase] = (int32_t)h;
    return;
  }
  int nref;
  const double* wref;
  const double* pref = ref_points<TDIM>(HD, degree, nref, wref);
  for (int k = 0; k < ns; ++k)
  {
    double V[NV][HD];
    if constexpr (HD == 1)
    {
      // the negative part from the negative vertex to the cut point, the positive part from there to the other vertex
      V[0][0] = 0.0; V[1][0] = 1.0;
      if (mask == 1 || mask == 2)
      {
        const double xa = mask == 1 ? 0.0 : 1.0, q = segment_cut(phi, mask);
        V[0][0] = part == PART_IN ? xa : q;
        V[1][0] = part == PART_IN ? q : 1.0 - xa;
      }
    }
    else
    {
      const CutCase& cs = c_cases[0][mask & 7];
      const int8_t* sx = part == PART_IN ? cs.in[k] : cs.out[k];
#pragma unroll
      for (int j = 0; j < NV; ++j) local_point<2>(cs, sx[j], phi, V[j]);
    }
    const double scale = fabs(simplex_det<HD>(V)) * measure;
    for (int q = 0; q < nref; ++q)
    {
      const int64_t o = pbase + k * nref + q;
      double X[HD];
      bary_point<HD, HD>(V, pref + HD * q, X);
#pragma unroll
      for (int d = 0; d < HD; ++d) points[o * HD + d] = X[d];
      weights[o] = wref[q] * scale;
    }
  }
  parent_map[rbase] = host_ids[h];
  rule_host[rbase] = (int32_t)h;
  offsets[rbase + 1] = pbase + ns * nref;
}

// whole-host rules (the standard facets of a mixed measure): reference points, weights * host measure
template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_full_rules_kernel(int64_t n, const int32_t* __restrict__ hosts,
                                                                  const double* __restrict__ x,
                                                                  const int32_t* __restrict__ verts,
                                                                  const int32_t* __restrict__ host_ids, int degree,
                                                                  double* __restrict__ points, double* __restrict__ weights,
                                                                  int32_t* __restrict__ offsets, int32_t* __restrict__ parent_map,
                                                                  int32_t* __restrict__ rule_host)
{
  constexpr int HD = TDIM - 1, NV = HD + 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t h = hosts ? hosts[i] : i;
  double xv[NV][TDIM];
#pragma unroll
  for (int v = 0; v < NV; ++v)
  {
    const int64_t g = verts[h * TDIM + v];
#pragma unroll
    for (int d = 0; d < TDIM; ++d) xv[v][d] = x[3 * g + d];
  }
  const double measure = facet_measure<TDIM>(xv);
  int nref;
  const double* wref;
  const double* pref = ref_points<TDIM>(HD, degree, nref, wref);
  for (int q = 0; q < nref; ++q)
  {
#pragma unroll
    for (int d = 0; d < HD; ++d) points[(i * nref + q) * HD + d] = pref[q * HD + d];
    weights[i * nref + q] = wref[q] * measure;
  }
  parent_map[i] = host_ids[h];
  rule_host[i] = (int32_t)h;
  offsets[i + 1] = (int32_t)((i + 1) * nref);
  if (i == 0) offsets[0] = 0;
}

__global__ void __launch_bounds__(kBlock) gather_rows_kernel(int64_t n, const int32_t* __restrict__ idx, int width,
                                                             const int32_t* __restrict__ src, int32_t* __restrict__ dst)
{
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * width) return;
  const int64_t i = t / width;
  const int k = (int)(t - i * width);
  dst[t] = src[(int64_t)idx[i] * width + k];
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_physical_points_kernel(int64_t nq, int64_t nr,
                                                                       const int32_t* __restrict__ offsets,
                                                                       const int32_t* __restrict__ verts,
                                                                       const double* __restrict__ points,
                                                                       const double* __restrict__ x, double* __restrict__ out)
{
  constexpr int HD = TDIM - 1;
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= nq) return;
  const int64_t r = rule_of_point(offsets, nr, q);
  double lam[HD + 1];
  lam[0] = 1.0;
#pragma unroll
  for (int t = 0; t < HD; ++t) { lam[t + 1] = points[q * HD + t]; lam[0] -= lam[t + 1]; }
#pragma unroll
  for (int d = 0; d < TDIM; ++d)
  {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j <= HD; ++j) v += lam[j] * x[3 * (int64_t)verts[r * TDIM + j] + d];
    out[q * TDIM + d] = v;
  }
}

// facet-hosted rule r seen from cell `side` of its row: parent = that cell, points = the cell's reference
// coordinates of the same physical points (barycentric weights moved to the cell's local vertices) --
// what facet_runtime_quadrature_payload / interior_facet_runtime_quadrature_payload hand to the kernels
// (python/cutfemx/_runintgen_adapter.py:605-680).  Rule i of the output is rule perm[i] of the input.
template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_to_cell_kernel(int64_t nq, int64_t nr, const int32_t* __restrict__ new_off,
                                                               const int32_t* __restrict__ perm,
                                                               const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ rows, int width, int side,
                                                               const int32_t* __restrict__ verts,
                                                               const double* __restrict__ points,
                                                               const double* __restrict__ weights,
                                                               const int32_t* __restrict__ conn,
                                                               double* __restrict__ out_points, double* __restrict__ out_weights,
                                                               int32_t* __restrict__ out_parent)
{
  constexpr int HD = TDIM - 1, NV = TDIM + 1;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nq) return;
  const int64_t i = rule_of_point(new_off, nr, p);
  const int64_t r = perm[i];
  const int64_t q = offsets[r] + (p - new_off[i]);
  const int64_t c = rows[r * width + 2 * side];
  double lam[HD + 1];
  lam[0] = 1.0;
#pragma unroll
  for (int t = 0; t < HD; ++t) { lam[t + 1] = points[q * HD + t]; lam[0] -= lam[t + 1]; }
  double X[TDIM];
#pragma unroll
  for (int t = 0; t < TDIM; ++t) X[t] = 0.0;
#pragma unroll
  for (int j = 0; j <= HD; ++j)
  {
    const int32_t g = verts[r * TDIM + j];
#pragma unroll
    for (int t = 0; t < TDIM; ++t) X[t] += (conn[c * NV + t + 1] == g) ? lam[j] : 0.0;
  }
#pragma unroll
  for (int t = 0; t < TDIM; ++t) out_points[p * TDIM + t] = X[t];
  out_weights[p] = weights[q];
  if (p == new_off[i]) out_parent[i] = (int32_t)c;
}

__global__ void __launch_bounds__(kBlock) rule_cell_keys_kernel(int64_t nr, const int32_t* __restrict__ rows, int width,
                                                                int side, int32_t* __restrict__ keys, int* unsorted)
{
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= nr) return;
  const int32_t k = rows[r * width + 2 * side];
  keys[r] = k;
  if (r > 0 && rows[(r - 1) * width + 2 * side] > k) *unsorted = 1;
}

__global__ void __launch_bounds__(kBlock) permuted_counts_kernel(int64_t nr, const int32_t* __restrict__ perm,
                                                                 const int32_t* __restrict__ offsets, int32_t* __restrict__ counts)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nr) return;
  const int64_t r = perm ? perm[i] : i;
  counts[i] = offsets[r + 1] - offsets[r];
}

// an empty rule set of reference dimension `dim` on the mesh
std::unique_ptr<cfx_rules_s> new_rules(cfx_mesh_t mesh, int dim)
{
  auto r = std::make_unique<cfx_rules_s>();
  r->mesh = mesh; r->tdim = dim; r->gdim = mesh->gdim;
  return r;
}

// its arrays for nq points of dimension dim and nr rules, with offsets[0] = 0.  sentinel: one more parent_map slot for
// the -1 behind the last rule -- cut_emit_kernel writes that and offsets[0] (no fill launch in a step)
void size_rules(cfx_rules_s& r, const Count& nq, const Count& nr, int dim, bool sentinel = false)
{
  r.nq = nq; r.nr = nr;
  r.points.alloc(nq.cap() * dim); r.weights.alloc(nq.cap()); r.offsets.alloc(nr.cap() + 1);
  r.parent_map.alloc(nr.cap() + (sentinel ? 1 : 0));
  r.parent_sentinel = sentinel;
  if (!sentinel) dev_fill(r.offsets.p, 0, sizeof(int32_t));
}

void multi_runtime_quadrature(cfx_cut_t cut, const Selector& sel, int order, cfx_rules_t* out)
{
  cfx_mesh_t mesh = cut->mesh;
  const int tdim = mesh->tdim;
  require(sel.term[sel.n - 1] == 0, CFX_ERR_INVALID_ARGUMENT,
          "runtime quadrature over several level sets takes one conjunction (clauses joined by 'and')");
  require(sel.n <= kMultiMaxClauses, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature: too many clauses in the selector");
  MultiArgs A{};
  MultiRuleCell pred{cut->domain.p, mesh->ncells, sel.n, {}, {}};
  A.eq = -1;
  int nclip = 0;
  for (int k = 0; k < sel.n; ++k)
  {
    require(sel.mask[k] != 7 && sel.mask[k] != 5, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature: unsupported relation");
    if (sel.mask[k] == 2)
    {
      require(A.eq < 0, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature: at most one '=0' clause (a codimension-1 interface)");
      A.eq = k;
    }
    else ++nclip;
    A.mask[k] = sel.mask[k]; A.phi[k] = cut->ls_values[sel.ls[k]].p;
    pred.ls[k] = sel.ls[k]; pred.mask[k] = sel.mask[k];
  }
  require(nclip <= 3, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature: at most three clipping clauses per conjunction");
  A.ncl = sel.n; A.order = order;
  DevArray<int32_t> cells;
  A.n = compact("multi_rule_cells", mesh->ncells, pred, cells);
  A.cells = cells.p; A.x = mesh->x.p; A.conn = mesh->conn.p; A.ls_dofmap = cut->ls_dofmap.p;
  auto r = new_rules(mesh, tdim);
  DevArray<int64_t> packed(A.n), packed_off(A.n + 1);
  A.packed = packed.p;
  const bool iface = A.eq >= 0;
  auto run = [&](bool emit)
  {
    if (A.n == 0) return;
    for_tdim(tdim, [&](auto T) {
      auto pass = [&](auto D) {
        if (emit) launch("multi_rules_emit", multi_rules_kernel<T(), D(), true>, grid_for(A.n), dim3(kBlock), 0, A);
        else launch("multi_rules_count", multi_rules_kernel<T(), D(), false>, grid_for(A.n), dim3(kBlock), 0, A);
      };
      if (iface) pass(std::integral_constant<int, T() - 1>{});
      else pass(T);
    });
  };
  ensure_cases();
  run(false);
  require(A.n < (1ll << 26), CFX_ERR_RUNTIME, "runtime quadrature: more than 2^26 cut cells");
  exclusive_scan(packed.p, packed_off.p, A.n);
  const int64_t totals = read_scalar(packed_off.p + A.n);
  const int64_t nq = totals & kPackMask, nr = totals >> kPackShift;
  require(nq < 2147483647LL, CFX_ERR_RUNTIME, "runtime quadrature: more than 2^31 points (int32 offsets)");
  size_rules(*r, nq, nr, tdim);
  A.packed_off = packed_off.p; A.points = r->points.p; A.weights = r->weights.p; A.offsets = r->offsets.p;
  A.parent_map = r->parent_map.p;
  run(true);
  CFX_HIP(hipStreamSynchronize(ctx().stream)); // (`cells` and the count arrays die with this frame)
  *out = r.release();
}

// runtime rules of one level set on cell hosts for one or two parts (PART_IN / PART_OUT / PART_IF) of the same cut:
// one count + scan per part, ONE read-back of the totals, one emit launch that stages every cut cell once
void simple_rules(cfx_cut_t cut, int n, const int* parts, int order, cfx_rules_t* out)
{
  cfx_mesh_t mesh = cut->mesh;
  const int tdim = mesh->tdim;
  const DevArray<int32_t>& cutc = locate(cut, "phi=0");
  const DevN ncut_d = cutc.devn();
  const int64_t ncut = ncut_d.cap; // (the capacity of the list while its length is still in HBM: grids and scans run over it)
  const double* phi = cut->ls_values[0].p;
  require(ncut < (1ll << 26), CFX_ERR_RUNTIME, "runtime quadrature: more than 2^26 cut cells");
  std::unique_ptr<cfx_rules_s> r[2];
  DevArray<int64_t> packed[2], packed_off[2];
  CountParts cparts{};
  cparts.n = n;
  for (int k = 0; k < n; ++k)
  {
    r[k] = new_rules(mesh, tdim);
    packed[k].alloc(ncut);
    packed_off[k].alloc(ncut + 1);
    cparts.part[k] = parts[k];
    cparts.nref[k] = quad_npoints(parts[k] == PART_IF ? tdim - 1 : tdim, order);
    cparts.packed[k] = packed[k].p;
  }
  // (both parts from one pass over the cut cells)
  for_tdim(tdim, [&](auto T) {
    launch("cut_count", cut_count_kernel<T()>, grid_for(ncut), dim3(kBlock), 0, ncut_d, cutc.p, cut->ls_dofmap.p, phi, cparts);
  });
  // one scan for both totals of a part: a cut cell emits at most 3 sub-simplices x 64 points and 2 rules, so below
  // 2^26 cut cells the point prefix stays under 2^34 and the rule prefix under 2^27 (no carry, no sign bit).
  // the totals of all parts in one round trip (none inside a step: they stay in HBM, published by the last scan)
  const char* names[4] = {"rules.points.0", "rules.rules.0", "rules.points.1", "rules.rules.1"};
  CountSource src[4];
  Count totals[4];
  for (int k = 0; k < n; ++k)
  {
    src[2 * k] = CountSource{packed_off[k].p + ncut, kCountPackedLo, kCountUpTo};
    src[2 * k + 1] = CountSource{packed_off[k].p + ncut, kCountPackedHi, kCountUpTo};
  }
  CountPlan cp(2 * n, names, src);
  if (n == 2) exclusive_scan_pair(packed[0].p, packed_off[0].p, packed[1].p, packed_off[1].p, ncut, &cp);
  else
    for (int k = 0; k < n; ++k) exclusive_scan(packed[k].p, packed_off[k].p, ncut, k == n - 1 ? &cp : nullptr);
  cp.finish(totals);
  EmitJobs jobs{};
  jobs.n = n;
  for (int k = 0; k < n; ++k)
  {
    const int64_t nq = totals[2 * k].cap(), nr = totals[2 * k + 1].cap();
    // int32 offsets are part of the RuntimeQuadrature contract
    require(nq < 2147483647LL, CFX_ERR_RUNTIME, "runtime quadrature: more than 2^31 points (int32 offsets)");
    size_rules(*r[k], totals[2 * k], totals[2 * k + 1], tdim, true);
    // (offsets[0] = 0 is written by the cell that emits rule 0; an empty rule set gets it here)
    if (ncut == 0 || nr == 0) dev_fill(r[k]->offsets.p, 0, sizeof(int32_t));
    jobs.part[k] = parts[k]; jobs.packed_off[k] = packed_off[k].p;
    jobs.points[k] = r[k]->points.p; jobs.weights[k] = r[k]->weights.p;
    jobs.offsets[k] = r[k]->offsets.p; jobs.parent_map[k] = r[k]->parent_map.p;
  }
  for_tdim(tdim, [&](auto T) {
    launch("cut_emit", cut_emit_kernel<T()>, grid_for(ncut, kBlock / kEmitLanes), dim3(kBlock), 0, ncut_d, cutc.p, mesh->x.p,
           mesh->conn.p, cut->ls_dofmap.p, phi, order, jobs);
  });
  for (int k = 0; k < n; ++k) out[k] = r[k].release();
}

void facet_runtime_quadrature(cfx_cut_t cut, const char* selector, int order, bool whole_hosts, cfx_rules_t* out)
{
  cfx_mesh_t mesh = cut->mesh;
  const int tdim = mesh->tdim, hd = tdim - 1;
  require(cut->nls == 1, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature for several level sets is not implemented");
  auto r = new_rules(mesh, hd);
  r->host_width = cut->host_width;
  DevArray<int32_t> rule_host;
  const double* phi = cut->ls_values[0].p;
  if (whole_hosts)
  {
    const DevArray<int32_t>* hosts = selector ? &locate_exact(cut, selector) : nullptr;
    const int64_t n = hosts ? hosts->n : cut->n_hosts;
    const int nref = quad_npoints(hd, order);
    require(n * nref < 2147483647LL, CFX_ERR_RUNTIME, "too many points for int32 offsets");
    size_rules(*r, n * nref, n, hd);
    rule_host.alloc(n);
    for_tdim(tdim, [&](auto T) {
      launch("facet_full_rules", facet_full_rules_kernel<T()>, grid_for(n), dim3(kBlock), 0, n, hosts ? hosts->p : nullptr,
             mesh->x.p, cut->host_verts.p, cut->host_ids.p, order, r->points.p, r->weights.p, r->offsets.p,
             r->parent_map.p, rule_host.p);
    });
  }
  else
  {
    const Selector sel = parse_selector(selector, cut->nls);
    require(sel.n == 1, CFX_ERR_INVALID_ARGUMENT, "runtime quadrature expects a single-clause selector");
    const int part = part_of_mask(sel.mask[0]);
    // phi = 0 on a facet: a point (segment hosts) or a straight segment (triangle hosts)
    const int nref = part == PART_IF ? (hd == 1 ? 1 : quad_npoints(1, order)) : quad_npoints(hd, order);
    const DevArray<int32_t>& cuth = locate_exact(cut, "phi=0");
    const int64_t ncut = cuth.n;
    DevArray<int32_t> n_rules(ncut), n_points(ncut), rule_off(ncut + 1), point_off(ncut + 1);
    for_tdim(tdim, [&](auto T) {
      launch("facet_count", facet_count_kernel<T()>, grid_for(ncut), dim3(kBlock), 0, ncut, cuth.p, cut->ls_dofmap.p, phi,
             part, nref, n_rules.p, n_points.p);
    });
    DevArray<int64_t> point_off64(ncut + 1);
    exclusive_scan(n_points.p, point_off64.p, ncut);
    const int64_t nq = read_scalar(point_off64.p + ncut);
    require(nq < 2147483647LL, CFX_ERR_RUNTIME, "runtime quadrature: more than 2^31 points (int32 offsets)");
    exclusive_scan(n_points.p, point_off.p, ncut);
    exclusive_scan(n_rules.p, rule_off.p, ncut);
    const int64_t nr = read_scalar(rule_off.p + ncut);
    size_rules(*r, nq, nr, hd);
    rule_host.alloc(nr);
    for_tdim(tdim, [&](auto T) {
      launch("facet_emit", facet_emit_kernel<T()>, grid_for(ncut), dim3(kBlock), 0, ncut, cuth.p, mesh->x.p,
             cut->host_verts.p, cut->ls_dofmap.p, phi, cut->host_ids.p, part, order, rule_off.p, point_off.p,
             r->points.p, r->weights.p, r->offsets.p, r->parent_map.p, rule_host.p);
    });
  }
  // the rules carry their hosts' rows and vertices: they outlive the cut object
  const int64_t nrh = r->nr.value();
  r->host_rows.alloc(nrh * cut->host_width);
  r->host_verts.alloc(nrh * tdim);
  gather_rows("facet_gather_rows", nrh, rule_host.p, cut->host_width, cut->host_rows.p, r->host_rows.p);
  gather_rows("facet_gather_rows", nrh, rule_host.p, tdim, cut->host_verts.p, r->host_verts.p);
  CFX_HIP(hipStreamSynchronize(ctx().stream));
  *out = r.release();
}

} // namespace

namespace cfx
{

void ensure_cases()
{
  if (g_cases_ready) return;
  for (int t = 2; t <= 3; ++t)
    for (int m = 0; m < 16; ++m) h_cases[t - 2][m] = make_case(t, m & ((1 << (t + 1)) - 1));
  CFX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_cases), h_cases, sizeof(h_cases)));
  g_cases_ready = true;
}

void gather_rows(const char* name, int64_t n, const int32_t* idx, int width, const int32_t* src, int32_t* dst)
{
  launch(name, gather_rows_kernel, grid_for(n * width), dim3(kBlock), 0, n, idx, width, src, dst);
}

} // namespace cfx

extern "C" {

int cfx_runtime_quadrature(cfx_cut_t cut, const char* selector, int order, const char* backend, cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(cut && selector && out, CFX_ERR_INVALID_ARGUMENT, "cfx_runtime_quadrature: null argument");
  if (backend && strcmp(backend, "straight") != 0)
    throw Error(CFX_ERR_INVALID_ARGUMENT, std::string("unsupported runtime quadrature backend '") + backend
                                              + "' (only 'straight' is implemented)");
  require(order >= 0, CFX_ERR_INVALID_ARGUMENT, "quadrature order must be non-negative");
  require(order <= CFX_QUAD_MAX_DEGREE, CFX_ERR_INVALID_ARGUMENT, "quadrature order exceeds the built-in tables");
  if (cut->host_width != 0)
  {
    facet_runtime_quadrature(cut, selector, order, false, out);
    return CFX_OK;
  }
  cfx_mesh_t mesh = cut->mesh;
  const int tdim = mesh->tdim;
  require(cut->ls_ndofs_cell == tdim + 1, CFX_ERR_INVALID_ARGUMENT,
          "runtime quadrature requires a P1 level set (straight cuts)");
  const Selector sel = parse_selector(selector, cut->nls);
  if (cut->nls > 1 || sel.n > 1)
  {
    multi_runtime_quadrature(cut, sel, order, out);
    return CFX_OK;
  }
  const int part = part_of_mask(sel.mask[0]);
  simple_rules(cut, 1, &part, order, out);
  CFX_API_END
}

int cfx_runtime_quadratures(cfx_cut_t cut, int n, const char* const* selectors, int order, const char* backend,
                            cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(cut && selectors && out && n >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_runtime_quadratures: null argument");
  for (int k = 0; k < n; ++k) out[k] = nullptr;
  // pairs of plain selectors of one level set on cell hosts share one pass over the cut cells; everything else is
  // the single call, selector by selector
  int k = 0;
  auto plain_part = [&](const char* text, int& part) -> bool
  {
    if (!text || cut->host_width != 0 || cut->nls != 1 || cut->ls_ndofs_cell != cut->mesh->tdim + 1) return false;
    if (backend && strcmp(backend, "straight") != 0) return false;
    if (order < 0 || order > CFX_QUAD_MAX_DEGREE) return false;
    Selector sel;
    try { sel = parse_selector(text, cut->nls); } catch (const Error&) { return false; }
    if (sel.n != 1) return false;
    const int m = sel.mask[0];
    if (m != 1 && m != 2 && m != 4) return false; // "<", "=", ">" only: the unions keep the single call
    part = part_of_mask(m);
    return true;
  };
  // the handles produced so far are released on EVERY error path (a status code of the single call, or an exception
  // of the pair path: too many points, order out of range)
  auto release = [&]() { for (int q = 0; q < n; ++q) { delete out[q]; out[q] = nullptr; } };
  for (int q = 0; q < n; ++q) out[q] = nullptr;
  try
  {
    while (k < n)
    {
      int parts[2];
      if (k + 1 < n && plain_part(selectors[k], parts[0]) && plain_part(selectors[k + 1], parts[1]))
      {
        simple_rules(cut, 2, parts, order, out + k);
        k += 2;
        continue;
      }
      const int rc = cfx_runtime_quadrature(cut, selectors[k], order, backend, out + k);
      if (rc != CFX_OK)
      {
        release();
        return rc;
      }
      ++k;
    }
  }
  catch (...)
  {
    release();
    throw;
  }
  CFX_API_END
}

int cfx_full_cell_rules(cfx_mesh_t mesh, const int32_t* cells, int64_t n, int order, cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(mesh && out && (cells || n == 0), CFX_ERR_INVALID_ARGUMENT, "cfx_full_cell_rules: null argument");
  require(order >= 0 && order <= CFX_QUAD_MAX_DEGREE, CFX_ERR_INVALID_ARGUMENT, "quadrature order out of range");
  const int tdim = mesh->tdim;
  const int nref = quad_npoints(tdim, order);
  require(n * nref < 2147483647LL, CFX_ERR_RUNTIME, "too many points for int32 offsets");
  DevArray<int32_t> dcells = to_device(cells, n);
  auto r = new_rules(mesh, tdim);
  size_rules(*r, n * nref, n, tdim);
  for_tdim(tdim, [&](auto T) {
    launch("full_rules", full_rules_kernel<T()>, grid_for(n), dim3(kBlock), 0, n, dcells.p, mesh->x.p, mesh->conn.p,
           order, r->points.p, r->weights.p, r->offsets.p, r->parent_map.p);
  });
  CFX_HIP(hipStreamSynchronize(ctx().stream));
  *out = r.release();
  CFX_API_END
}

int cfx_rules_create(cfx_mesh_t mesh, int tdim, int64_t nq, int64_t nr, const double* points, const double* weights,
                     const int32_t* offsets, const int32_t* parent_map, cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(mesh && out, CFX_ERR_INVALID_ARGUMENT, "cfx_rules_create: null argument");
  require(tdim == mesh->tdim, CFX_ERR_INVALID_ARGUMENT, "rules tdim must match the mesh");
  require(nq >= 0 && nr >= 0 && offsets, CFX_ERR_INVALID_ARGUMENT, "cfx_rules_create: invalid sizes");
  auto r = new_rules(mesh, tdim);
  r->nq = nq; r->nr = nr;
  r->points = to_device(points, nq * tdim);
  r->weights = to_device(weights, nq);
  r->offsets = to_device(offsets, nr + 1);
  r->parent_map = to_device(parent_map, nr);
  *out = r.release();
  CFX_API_END
}

int cfx_rules_view_get(cfx_rules_t r, cfx_rules_view* v)
{
  CFX_API_BEGIN
  require(r && v, CFX_ERR_INVALID_ARGUMENT, "cfx_rules_view_get: null argument");
  // (capacities while the step that made the rules is open: the arrays are at least that long, cutfemx_amd.h)
  v->tdim = r->tdim; v->gdim = r->gdim; v->nq = r->nq.cap(); v->nr = r->nr.cap();
  v->points = r->points.p; v->weights = r->weights.p; v->offsets = r->offsets.p; v->parent_map = r->parent_map.p;
  v->host_width = r->host_width; v->reserved = 0;
  v->host_rows = r->host_width ? r->host_rows.p : nullptr;
  v->host_verts = r->host_width ? r->host_verts.p : nullptr;
  CFX_API_END
}

int cfx_rules_physical_points(cfx_rules_t r, double* out)
{
  CFX_API_BEGIN
  require(r && out, CFX_ERR_INVALID_ARGUMENT, "cfx_rules_physical_points: null argument");
  const int64_t nq = r->nq.value(), nr = r->nr.value(); // (a host array of nq points: the exact count)
  OutArray<double> o(out, nq * r->gdim, false);
  for_tdim(r->mesh->tdim, [&](auto T) {
    if (r->host_width != 0) // physical_points_for_host_mesh (cut.cpp:1344-1345)
      launch("physical_points", facet_physical_points_kernel<T()>, grid_for(nq), dim3(kBlock), 0, nq, nr,
             r->offsets.p, r->host_verts.p, r->points.p, r->mesh->x.p, o.dev);
    else
      launch("physical_points", physical_points_kernel<T()>, grid_for(nq), dim3(kBlock), 0, nq, nr,
             r->offsets.p, r->parent_map.p, r->points.p, r->mesh->x.p, r->mesh->conn.p, o.dev);
  });
  o.finish();
  CFX_API_END
}

int cfx_rules_destroy(cfx_rules_t r)
{
  CFX_API_BEGIN
  delete r;
  CFX_API_END
}

int cfx_evaluate_normals(cfx_cut_t cut, int ls, cfx_rules_t r, double sign, double* out)
{
  CFX_API_BEGIN
  require(cut && r && out, CFX_ERR_INVALID_ARGUMENT, "Cannot evaluate normals without a level set.");
  require(ls >= 0 && ls < cut->nls, CFX_ERR_OUT_OF_RANGE, "level-set index out of range");
  require(r->tdim == cut->mesh->tdim, CFX_ERR_RUNTIME, "Normal evaluation points must have cell reference dimension.");
  require(cut->ls_ndofs_cell == cut->mesh->tdim + 1, CFX_ERR_INVALID_ARGUMENT,
          "normal evaluation is implemented for P1 level sets");
  // a device destination takes the rules' capacity (nq.cap() doubles per component) while their length is in HBM;
  // a host destination needs the exact count
  if (!is_device_pointer(out)) (void)r->nq.value();
  OutArray<double> o(out, r->nq.cap() * r->gdim, false);
  if (r->nq.cap() > 0)
    for_tdim(r->tdim, [&](auto T) {
      launch("evaluate_normals", normals_rule_kernel<T()>, grid_for(r->nr.cap()), dim3(kBlock), 0, r->nr, r->offsets.p,
             r->parent_map.p, cut->mesh->x.p, cut->mesh->conn.p, cut->ls_dofmap.p, cut->ls_values[ls].p, sign, o.dev);
    });
  o.finish();
  CFX_API_END
}

int cfx_evaluate_values(cfx_cut_t cut, int ls, cfx_rules_t r, double* out)
{
  CFX_API_BEGIN
  require(cut && r && out, CFX_ERR_INVALID_ARGUMENT, "Cannot evaluate values without a level set.");
  require(ls >= 0 && ls < cut->nls, CFX_ERR_OUT_OF_RANGE, "level-set index out of range");
  require(cut->ls_ndofs_cell == cut->mesh->tdim + 1, CFX_ERR_INVALID_ARGUMENT,
          "value evaluation is implemented for P1 level sets");
  const int64_t nq = r->nq.value(), nr = r->nr.value();
  OutArray<double> o(out, nq, false);
  for_tdim(r->tdim, [&](auto T) {
    launch("evaluate_values", values_kernel<T()>, grid_for(nq), dim3(kBlock), 0, nq, nr, r->offsets.p,
           r->parent_map.p, r->points.p, cut->ls_dofmap.p, cut->ls_values[ls].p, o.dev);
  });
  o.finish();
  CFX_API_END
}

int cfx_full_facet_rules(cfx_cut_t cut, const char* selector, int order, cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(cut && out, CFX_ERR_INVALID_ARGUMENT, "cfx_full_facet_rules: null argument");
  require(cut->host_width != 0, CFX_ERR_INVALID_ARGUMENT, "cfx_full_facet_rules: the cut is hosted by cells");
  require(order >= 0 && order <= CFX_QUAD_MAX_DEGREE, CFX_ERR_INVALID_ARGUMENT, "quadrature order out of range");
  facet_runtime_quadrature(cut, selector, order, true, out);
  CFX_API_END
}

int cfx_facet_rules_to_cells(cfx_rules_t R, int side, cfx_rules_t* out)
{
  CFX_API_BEGIN
  require(R && out, CFX_ERR_INVALID_ARGUMENT, "cfx_facet_rules_to_cells: null argument");
  require(R->host_width != 0, CFX_ERR_INVALID_ARGUMENT, "cfx_facet_rules_to_cells: the rules are hosted by cells");
  require(side == 0 || (side == 1 && R->host_width == 4), CFX_ERR_INVALID_ARGUMENT,
          "cfx_facet_rules_to_cells: side is 0, or 1 for interior-facet rows");
  cfx_mesh_t mesh = R->mesh;
  const int tdim = mesh->tdim;
  const int64_t nr = R->nr.value(), nq = R->nq.value();
  auto r = new_rules(mesh, tdim);
  size_rules(*r, nq, nr, tdim);
  if (nr > 0)
  {
    // cell-hosted rules are consumed in ascending parent order (runs of one parent are contiguous)
    DevArray<int32_t> keys(nr), perm(nr), counts(nr);
    ZeroFlag unsorted;
    launch("facet_to_cells", rule_cell_keys_kernel, grid_for(nr), dim3(kBlock), 0, nr, R->host_rows.p, R->host_width, side,
           keys.p, unsorted.p);
    iota(nr, perm.p);
    if (read_scalar(unsorted.p))
    {
      DevArray<int32_t> keys_out(nr), perm_out(nr);
      size_t tmp_bytes = 0;
      CFX_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys.p, keys_out.p, perm.p, perm_out.p, (size_t)nr, 0, 32,
                                        ctx().stream));
      DevArray<uint8_t> tmp((int64_t)tmp_bytes);
      CFX_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, keys.p, keys_out.p, perm.p, perm_out.p, (size_t)nr, 0, 32,
                                        ctx().stream));
      CFX_HIP(hipStreamSynchronize(ctx().stream));
      perm = std::move(perm_out);
    }
    launch("facet_to_cells", permuted_counts_kernel, grid_for(nr), dim3(kBlock), 0, nr, perm.p, R->offsets.p, counts.p);
    exclusive_scan(counts.p, r->offsets.p, nr);
    for_tdim(tdim, [&](auto T) {
      launch("facet_to_cells", facet_to_cell_kernel<T()>, grid_for(nq), dim3(kBlock), 0, nq, nr, r->offsets.p, perm.p,
             R->offsets.p, R->host_rows.p, R->host_width, side, R->host_verts.p, R->points.p, R->weights.p, mesh->conn.p,
             r->points.p, r->weights.p, r->parent_map.p);
    });
    CFX_HIP(hipStreamSynchronize(ctx().stream));
  }
  *out = r.release();
  CFX_API_END
}

} // extern "C"
