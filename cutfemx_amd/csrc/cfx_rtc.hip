// cutfemx_amd: user-supplied integrands, compiled at run time with hipRTC.
//
// The reference compiles every form to its own tabulate_tensor kernel (runintgen / FFCx: Form.h:59-75,
// python/cutfemx/_runintgen_adapter.py:181-217) and calls that CPU function pointer per entity.  The GPU counterpart:
// the caller registers the SOURCE of a device function with the argument list below; the engine compiles it for
// gfx950 together with a stage-1 wrapper (one thread per entity: geometry, packed coefficient, rule slice -> the
// function -> local tensor staged in HBM) and the existing row gather -- or the entity-parallel atomic scatter --
// consumes the staged tensors exactly as it does for the built-in integrands that are not formed in line.
//
//   __device__ void NAME(double* A,                    // local tensor, zero on entry: [ND][ND] row-major (rank 2) or [ND]
//                        const double* w,              // packed coefficient: the ND cell dofs of `coefficient`, or NULL
//                        const double* c,              // constants: cfx_integral.params[8]
//                        const double* coordinate_dofs,// vertex coordinates of the cell, [(TDIM+1)][3] (UFCx layout)
//                        int nq, const double* points, // rule of this entity: [nq][TDIM] parent-reference coordinates
//                        const double* weights,        // [nq] PHYSICAL-measure weights (standard entities: reference
//                                                      // weights x |det J|; runtime rules: as the rules carry them)
//                        const double* point_data);    // [nq][point_stride] per-point data of the rules, or NULL
//
// CFX_TDIM, CFX_ND (scalar dofs per cell of the form's Lagrange space), CFX_BS (block size of the space) and CFX_NDB =
// CFX_ND * CFX_BS (local dimension: entry (i, a) = dof i, component a sits at i * CFX_BS + a) are defined when the source
// is compiled; the prelude below offers cfx_tabulate_p1 / cfx_tabulate_p2 (values and reference gradients) and
// cfx_inverse_jacobian.
//
// Interior-facet integrands (cfx_integrand_register_facet; the reference's call with entity_local_index = {lf0, lf1},
// assemble_matrix_impl.h:528-542):
//
//   __device__ void NAME(double* A,                     // macro tensor, zero on entry: [2 NDB][2 NDB] row-major, rows and
//                                                       // columns = [cell 0 dofs, cell 1 dofs]: [[00, 01], [10, 11]]
//                        const double* w,               // packed coefficient of both cells [2][ND], or NULL
//                        const double* c,               // constants: cfx_integral.params[8]
//                        const double* coordinate_dofs, // [2][(TDIM+1)][3]: cell 0, then cell 1
//                        const int* entity_local_index, // {lf0, lf1}: the local facet in either cell
//                        int nq,
//                        const double* points0,         // [nq][TDIM] the facet's points in the reference cell of cell 0
//                        const double* points1,         // ... and the SAME physical points in the reference cell of cell 1
//                        const double* weights);        // [nq] physical (facet-measure) weights
//
// Coefficient lists (cfx_form_set_coefficients; the reference's Form::coefficients() packed at coefficient_offsets(),
// pack_form.h:69-158): `w` then holds Function k of the integral's list -- CFX_W_ND<k> dofs per cell, CFX_W_BS<k>
// components per dof, gathered through the dofmap of its own space -- at CFX_W_OFF<k> = sum_{j<k} nd_j bs_j, dof i
// component b at CFX_W_OFF<k> + i * CFX_W_BS<k> + b, CFX_CSTRIDE doubles in all (CFX_NCOEF Functions).  Interior facets:
// 2 CFX_CSTRIDE doubles, Function k's block of cell 0 at 2 CFX_W_OFF<k> and of cell 1 directly after it.  At most 64
// doubles: `w` is a thread-private array the integrand indexes freely.
#include <dlfcn.h>

#include <array>
#include <mutex>
#include <set>

#include <hip/hiprtc.h>

#include "cfx_device.h"

namespace cfx
{
int quad_npoints(int dim, int degree);
const double* quad_points_host(int dim, int degree);  // cfx_quadhost.cpp
const double* quad_weights_host(int dim, int degree);
} // namespace cfx

using namespace cfx;

namespace
{
// what the compiled wrapper takes (the same struct is spelled out in the wrapper's source below)
struct RtcArgs
{
  const double* x;
  const int32_t* conn;
  const int32_t* dofmap;
  int64_t n_cap;
  const int64_t* n_dev;
  const int32_t* entities;
  const int32_t* offsets;
  const int32_t* parent_map;
  const double* points;
  const double* weights;
  const double* point_data;
  int point_stride, runtime, nref, rank;
  const double* ref_points;
  const double* ref_weights;
  double params[8];
  const double* coeff;
  double* out;
  int64_t out_stride; // out_mode 1 / 2: entry i of the local vector lives at out[i * out_stride + index]
  int out_mode;       // 0: [entity][NT]; 1: [i][stride] indexed by the entity; 2: [i][stride] indexed by the cell
  int coeff_bs;       // components per dof of `coeff` (rank 1 on a vector space: the space's block size; else 1)
};

const char* kPrelude = R"RTC(
typedef long long cfx_i64;
typedef int cfx_i32;
struct RtcArgs
{
  const double* x; const cfx_i32* conn; const cfx_i32* dofmap;
  cfx_i64 n_cap; const cfx_i64* n_dev;
  const cfx_i32* entities; const cfx_i32* offsets; const cfx_i32* parent_map;
  const double* points; const double* weights; const double* point_data;
  int point_stride, runtime, nref, rank;
  const double* ref_points; const double* ref_weights;
  double params[8];
  const double* coeff;
  double* out;
  cfx_i64 out_stride;
  int out_mode, coeff_bs;
};
// Lagrange bases on the reference simplex, vertex order of the mesh connectivity; degree 2: vertices, then the edge
// midpoints in the order of the engine's dofmaps (cutfemx_amd.lagrange_dofmap)
__device__ inline void cfx_tabulate_p1(const double* X, double* N, double (*dN)[CFX_TDIM])
{
  double l0 = 1.0;
  for (int t = 0; t < CFX_TDIM; ++t) l0 -= X[t];
  N[0] = l0;
  for (int t = 0; t < CFX_TDIM; ++t) { N[t + 1] = X[t]; dN[0][t] = -1.0; }
  for (int i = 0; i < CFX_TDIM; ++i)
    for (int t = 0; t < CFX_TDIM; ++t) dN[i + 1][t] = (i == t) ? 1.0 : 0.0;
}
// degree 2: vertices, then edges -- tri: (1,2),(0,2),(0,1); tet: (2,3),(1,3),(1,2),(0,3),(0,2),(0,1) (the Basix order)
__device__ inline void cfx_tabulate_p2(const double* X, double* N, double (*dN)[CFX_TDIM])
{
  double lam[CFX_TDIM + 1], g[CFX_TDIM + 1][CFX_TDIM];
  lam[0] = 1.0;
  for (int t = 0; t < CFX_TDIM; ++t) { lam[0] -= X[t]; lam[t + 1] = X[t]; }
  for (int i = 0; i <= CFX_TDIM; ++i)
    for (int t = 0; t < CFX_TDIM; ++t) g[i][t] = (i == 0) ? -1.0 : ((i - 1 == t) ? 1.0 : 0.0);
  for (int i = 0; i <= CFX_TDIM; ++i)
  {
    N[i] = lam[i] * (2.0 * lam[i] - 1.0);
    for (int t = 0; t < CFX_TDIM; ++t) dN[i][t] = (4.0 * lam[i] - 1.0) * g[i][t];
  }
#if CFX_TDIM == 2
  const int ne = 3, ea[3] = {1, 0, 0}, eb[3] = {2, 2, 1};
#else
  const int ne = 6, ea[6] = {2, 1, 1, 0, 0, 0}, eb[6] = {3, 3, 2, 3, 2, 1};
#endif
  for (int e = 0; e < ne; ++e)
  {
    N[CFX_TDIM + 1 + e] = 4.0 * lam[ea[e]] * lam[eb[e]];
    for (int t = 0; t < CFX_TDIM; ++t) dN[CFX_TDIM + 1 + e][t] = 4.0 * (lam[ea[e]] * g[eb[e]][t] + g[ea[e]][t] * lam[eb[e]]);
  }
}
#ifdef CFX_ND
// the basis of the form's space: CFX_ND dofs per cell
__device__ inline void cfx_tabulate(const double* X, double* N, double (*dN)[CFX_TDIM])
{
#if CFX_ND == CFX_TDIM + 1
  cfx_tabulate_p1(X, N, dN);
#else
  cfx_tabulate_p2(X, N, dN);
#endif
}
#else
// two-space variants: the basis of the test space (CFX_ND0 dofs per cell) and of the trial space (CFX_ND1)
__device__ inline void cfx_tabulate0(const double* X, double* N, double (*dN)[CFX_TDIM])
{
#if CFX_ND0 == CFX_TDIM + 1
  cfx_tabulate_p1(X, N, dN);
#else
  cfx_tabulate_p2(X, N, dN);
#endif
}
__device__ inline void cfx_tabulate1(const double* X, double* N, double (*dN)[CFX_TDIM])
{
#if CFX_ND1 == CFX_TDIM + 1
  cfx_tabulate_p1(X, N, dN);
#else
  cfx_tabulate_p2(X, N, dN);
#endif
}
#endif
// K[t][d] = d xi_t / d x_d and det J of the affine cell with vertices coordinate_dofs[(CFX_TDIM + 1)][3]
__device__ inline double cfx_inverse_jacobian(const double* xc, double (*K)[CFX_TDIM])
{
  double J[CFX_TDIM][CFX_TDIM];
  for (int d = 0; d < CFX_TDIM; ++d)
    for (int t = 0; t < CFX_TDIM; ++t) J[d][t] = xc[3 * (t + 1) + d] - xc[d];
#if CFX_TDIM == 2
  const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  K[0][0] = J[1][1] / det;  K[0][1] = -J[0][1] / det;
  K[1][0] = -J[1][0] / det; K[1][1] = J[0][0] / det;
#else
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
  K[0][0] = c00 / det;
  K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
  K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
  K[1][0] = c01 / det;
  K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
  K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
  K[2][0] = c02 / det;
  K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
  K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
#endif
  return det;
}
// UFL CellDiameter: the largest vertex-to-vertex distance
__device__ inline double cfx_cell_diameter(const double* xc)
{
  double h2 = 0.0;
  for (int i = 0; i <= CFX_TDIM; ++i)
    for (int j = i + 1; j <= CFX_TDIM; ++j)
    {
      double d2 = 0.0;
      for (int d = 0; d < CFX_TDIM; ++d) d2 += (xc[3 * i + d] - xc[3 * j + d]) * (xc[3 * i + d] - xc[3 * j + d]);
      h2 = d2 > h2 ? d2 : h2;
    }
  return sqrt(h2);
}
)RTC";

// the wrapper: CFX_USER_FN is the registered function.  CFXW_ND (dofs per cell of the test space: the coefficient's
// packing), CFXW_NR (rows: local dimension of the test space) and CFXW_NC (columns: of the trial space) are defined by
// the engine -- CFX_ND, CFX_NDB, CFX_NDB for a square form, CFX_ND0, CFX_NDB0, CFX_NDB1 for a two-space one
const char* kWrapper = R"RTC(
#define CFX_MAXQ 64
extern "C" __global__ void __launch_bounds__(256) cfx_user_stage1(RtcArgs A)
{
  const cfx_i64 e = (cfx_i64)blockIdx.x * 256 + threadIdx.x;
  cfx_i64 n = A.n_cap;
  if (A.n_dev) { const cfx_i64 v = *A.n_dev; n = v < n ? v : n; }
  if (e >= n) return;
  const cfx_i64 cell = A.runtime ? A.parent_map[e] : A.entities[e];
  double xc[(CFX_TDIM + 1) * 3];
  for (int v = 0; v <= CFX_TDIM; ++v)
  {
    const cfx_i64 node = A.conn[cell * (CFX_TDIM + 1) + v];
    for (int d = 0; d < 3; ++d) xc[3 * v + d] = A.x[3 * node + d];
  }
  // packed coefficient: [ND][coeff_bs] (a scalar Function of the test space's dofmap for bilinear forms, a Function of
  // the form's space -- CFX_BS components per dof -- for linear forms on vector spaces)
  double w[CFXW_NR];
  if (A.coeff)
    for (int j = 0; j < CFXW_ND; ++j)
      for (int b = 0; b < A.coeff_bs; ++b) w[j * A.coeff_bs + b] = A.coeff[(cfx_i64)A.dofmap[cell * CFXW_ND + j] * A.coeff_bs + b];
  const int NT = A.rank == 2 ? CFXW_NR * CFXW_NC : CFXW_NR;
  double T[CFXW_NR * CFXW_NC];
  for (int i = 0; i < CFXW_NR * CFXW_NC; ++i) T[i] = 0.0;
  if (A.runtime)
  {
    const int q0 = A.offsets[e], nq = A.offsets[e + 1] - q0;
    CFX_USER_FN(T, A.coeff ? w : (const double*)0, A.params, xc, nq, A.points + (cfx_i64)q0 * CFX_TDIM, A.weights + q0,
                A.point_data ? A.point_data + (cfx_i64)q0 * A.point_stride : (const double*)0);
  }
  else
  {
    double K[CFX_TDIM][CFX_TDIM];
    const double det = fabs(cfx_inverse_jacobian(xc, K));
    double wq[CFX_MAXQ];
    const int nq = A.nref < CFX_MAXQ ? A.nref : CFX_MAXQ;
    for (int q = 0; q < nq; ++q) wq[q] = A.ref_weights[q] * det;
    CFX_USER_FN(T, A.coeff ? w : (const double*)0, A.params, xc, nq, A.ref_points, wq, (const double*)0);
  }
  if (A.out_mode == 0)
    for (int i = 0; i < NT; ++i) A.out[e * NT + i] = T[i];
  else
  {
    const cfx_i64 at = A.out_mode == 2 ? cell : e;
    for (int i = 0; i < NT; ++i) A.out[(cfx_i64)i * A.out_stride + at] = T[i];
  }
}
)RTC";

// the facet wrapper: one thread per (c0, lf0, c1, lf1) row.  The points: the reference facet rule pushed to physical
// space from cell 0's facet lf0 (its vertices in ascending local order) and pulled back to both reference cells -- what
// the built-in facet kernels do (cfx_elem.h: facet_local_row) -- with the facet's measure in the weights.  Entities
// f >= n_std of an integral with facet-hosted rules integrate over rule f - n_std instead (assemble_facets_kernel with
// RT = true): its points live on the simplex of the host vertices, its weights are used as stored, and the pulled-back
// points go to `scratch` (two [nq capacity][TDIM] arrays at the rule's own offsets) -- a rule of any length, no
// truncation.  Macro tensor [2 CFXW_NR][2 CFXW_NC]: rows [cell 0, cell 1] of the test space, columns of the trial space.
struct RtcFacetArgs
{
  const double* x;
  const int32_t* conn;
  const int32_t* dofmap;
  int64_t n_cap;
  const int64_t* n_dev;
  const int32_t* rows;
  int nref, pad;
  const double* ref_points;
  const double* ref_weights;
  double params[8];
  const double* coeff;
  double* out;
  int64_t n_std, f0; // facet-hosted rules: entity f0 + f of the integral is rule f0 + f - n_std when >= n_std
  const int32_t* offsets;
  const double* rpoints;
  const double* rweights;
  const int32_t* host_verts;
  double* scratch;
  int64_t scratch_stride; // doubles per side in `scratch` (nq capacity * TDIM)
};
const char* kFacetWrapper = R"RTC(
struct RtcFacetArgs
{
  const double* x; const cfx_i32* conn; const cfx_i32* dofmap;
  cfx_i64 n_cap; const cfx_i64* n_dev;
  const cfx_i32* rows;
  int nref, pad;
  const double* ref_points; const double* ref_weights;
  double params[8];
  const double* coeff;
  double* out;
  cfx_i64 n_std, f0;
  const cfx_i32* offsets; const double* rpoints; const double* rweights; const cfx_i32* host_verts;
  double* scratch;
  cfx_i64 scratch_stride;
};
#define CFX_MAXQF 32
// RT: the launch covers facet-hosted rules (cfx_user_stage1_rules); the standard facets' entry point is compiled
// without that code (as assemble_facets_kernel<..., RT>), so its registers are those of a standard-facet kernel
template <bool RT>
__device__ __forceinline__ void cfx_facet_stage(const RtcFacetArgs& A)
{
  const cfx_i64 f = (cfx_i64)blockIdx.x * 256 + threadIdx.x;
  cfx_i64 n = A.n_cap;
  if (A.n_dev) { const cfx_i64 v = *A.n_dev; n = v < n ? v : n; }
  if (f >= n) return;
  const cfx_i64 c0 = A.rows[4 * f], c1 = A.rows[4 * f + 2];
  const int eli[2] = {A.rows[4 * f + 1], A.rows[4 * f + 3]};
  double xc[2 * (CFX_TDIM + 1) * 3];
  for (int s = 0; s < 2; ++s)
    for (int v = 0; v <= CFX_TDIM; ++v)
    {
      const cfx_i64 node = A.conn[(s ? c1 : c0) * (CFX_TDIM + 1) + v];
      for (int d = 0; d < 3; ++d) xc[(s * (CFX_TDIM + 1) + v) * 3 + d] = A.x[3 * node + d];
    }
  double w[2 * CFXW_ND];
  if (A.coeff)
    for (int s = 0; s < 2; ++s)
      for (int j = 0; j < CFXW_ND; ++j) w[s * CFXW_ND + j] = A.coeff[A.dofmap[(s ? c1 : c0) * CFXW_ND + j]];
  double K0[CFX_TDIM][CFX_TDIM], K1[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(xc, K0);
  (void)cfx_inverse_jacobian(xc + (CFX_TDIM + 1) * 3, K1);
  const cfx_i64 r = RT ? A.f0 + f - A.n_std : -1; // >= 0: a facet-hosted rule
  // the facet's vertices: those of cell 0 except lf0, ascending local index (a facet-hosted rule: its host vertices)
  double xf[CFX_TDIM][3];
  if (RT)
    for (int j = 0; j < CFX_TDIM; ++j)
    {
      const cfx_i64 v = A.host_verts[r * CFX_TDIM + j];
      for (int d = 0; d < 3; ++d) xf[j][d] = A.x[3 * v + d];
    }
  else
  {
    int k = 0;
    for (int i = 0; i <= CFX_TDIM; ++i)
    {
      if (i == eli[0]) continue;
      for (int d = 0; d < 3; ++d) xf[k][d] = xc[3 * i + d];
      ++k;
    }
  }
  double measure;
#if CFX_TDIM == 2
  {
    const double dx = xf[1][0] - xf[0][0], dy = xf[1][1] - xf[0][1];
    measure = sqrt(dx * dx + dy * dy);
  }
#else
  {
    double a[3], b[3];
    for (int d = 0; d < 3; ++d) { a[d] = xf[1][d] - xf[0][d]; b[d] = xf[2][d] - xf[0][d]; }
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    measure = sqrt(cx * cx + cy * cy + cz * cz);
  }
#endif
  // the points fp[nq][TDIM - 1] on the simplex xf, pushed to physical space and pulled back to both cells
  auto pull_back = [&](const double* fp, int nq, double* P0, double* P1) {
    for (int q = 0; q < nq; ++q)
    {
      double l0 = 1.0, xq[CFX_TDIM];
      for (int t = 0; t < CFX_TDIM - 1; ++t) l0 -= fp[q * (CFX_TDIM - 1) + t];
      for (int d = 0; d < CFX_TDIM; ++d)
      {
        double v = l0 * xf[0][d];
        for (int t = 0; t < CFX_TDIM - 1; ++t) v += fp[q * (CFX_TDIM - 1) + t] * xf[t + 1][d];
        xq[d] = v;
      }
      for (int t = 0; t < CFX_TDIM; ++t)
      {
        double a = 0.0, b = 0.0;
        for (int d = 0; d < CFX_TDIM; ++d)
        {
          a += K0[t][d] * (xq[d] - xc[d]);
          b += K1[t][d] * (xq[d] - xc[(CFX_TDIM + 1) * 3 + d]);
        }
        P0[q * CFX_TDIM + t] = a;
        P1[q * CFX_TDIM + t] = b;
      }
    }
  };
  double T[4 * CFXW_NR * CFXW_NC];
  for (int i = 0; i < 4 * CFXW_NR * CFXW_NC; ++i) T[i] = 0.0;
  if constexpr (RT)
  {
    const int q0 = A.offsets[r], nq = A.offsets[r + 1] - q0;
    double* P0 = A.scratch + (cfx_i64)q0 * CFX_TDIM;
    double* P1 = A.scratch + A.scratch_stride + (cfx_i64)q0 * CFX_TDIM;
    pull_back(A.rpoints + (cfx_i64)q0 * (CFX_TDIM - 1), nq, P0, P1);
    CFX_USER_FN(T, A.coeff ? w : (const double*)0, A.params, xc, eli, nq, P0, P1, A.rweights + q0);
  }
  else
  {
    const int nq = A.nref < CFX_MAXQF ? A.nref : CFX_MAXQF;
    double P0[CFX_MAXQF * CFX_TDIM], P1[CFX_MAXQF * CFX_TDIM], wq[CFX_MAXQF];
    pull_back(A.ref_points, nq, P0, P1);
    for (int q = 0; q < nq; ++q) wq[q] = A.ref_weights[q] * measure;
    CFX_USER_FN(T, A.coeff ? w : (const double*)0, A.params, xc, eli, nq, P0, P1, wq);
  }
  for (int i = 0; i < 4 * CFXW_NR * CFXW_NC; ++i) A.out[f * (4 * CFXW_NR * CFXW_NC) + i] = T[i];
}
extern "C" __global__ void __launch_bounds__(256) cfx_user_stage1(RtcFacetArgs A) { cfx_facet_stage<false>(A); }
extern "C" __global__ void __launch_bounds__(256) cfx_user_stage1_rules(RtcFacetArgs A) { cfx_facet_stage<true>(A); }
)RTC";

// hipRTC through dlopen: the engine does not link it (a process that never registers an integrand never loads it,
// and one that has PyTorch's copy mapped gets that copy)
struct Rtc
{
  void* lib = nullptr;
  decltype(&hiprtcCreateProgram) create = nullptr;
  decltype(&hiprtcCompileProgram) compile = nullptr;
  decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
  decltype(&hiprtcGetProgramLog) log = nullptr;
  decltype(&hiprtcGetCodeSize) code_size = nullptr;
  decltype(&hiprtcGetCode) code = nullptr;
  decltype(&hiprtcDestroyProgram) destroy = nullptr;
};

Rtc& rtc()
{
  static Rtc r;
  if (r.lib) return r;
  for (const char* name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"})
  {
    r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (r.lib) break;
  }
  if (!r.lib) throw Error(CFX_ERR_RUNTIME, std::string("cfx_integrand_register: cannot load hipRTC (") + dlerror() + ")");
  auto sym = [&](const char* s) {
    void* p = dlsym(r.lib, s);
    if (!p) throw Error(CFX_ERR_RUNTIME, std::string("hipRTC: missing symbol ") + s);
    return p;
  };
  r.create = reinterpret_cast<decltype(r.create)>(sym("hiprtcCreateProgram"));
  r.compile = reinterpret_cast<decltype(r.compile)>(sym("hiprtcCompileProgram"));
  r.log_size = reinterpret_cast<decltype(r.log_size)>(sym("hiprtcGetProgramLogSize"));
  r.log = reinterpret_cast<decltype(r.log)>(sym("hiprtcGetProgramLog"));
  r.code_size = reinterpret_cast<decltype(r.code_size)>(sym("hiprtcGetCodeSize"));
  r.code = reinterpret_cast<decltype(r.code)>(sym("hiprtcGetCode"));
  r.destroy = reinterpret_cast<decltype(r.destroy)>(sym("hiprtcDestroyProgram"));
  return r;
}

struct UserIntegrand
{
  std::string name, source;
  int rank = 2;
  int kind = 0;                                  // 0: cell integrand, 1: interior-facet integrand
  bool two = false;                              // a bilinear integrand between two spaces (cfx_integrand_register2)
  std::map<std::string, std::vector<char>> code; // variant key (Variant::key) -> code object for gfx950
  std::map<std::string, hipModule_t> module;
  std::map<std::string, hipFunction_t> function;
  // variants with a coefficient list compiled ahead of use (cfx_integrand_compile_coefficients): once there is one, a
  // list is launched with a variant of this set only -- the source was written for those shapes
  std::set<std::string> declared;
};

// (tdim, dofs per cell, block size) of the form's space; nd1 > 0: (tdim, nd0, bs0) of the test space, (nd1, bs1) of the
// trial space of a two-space integrand; coefs: (dofs per cell, block size) of every Function of the integral's
// coefficient list, in order (empty: the single `coefficient`)
struct Variant
{
  int tdim, nd0, bs0, nd1 = 0, bs1 = 0;
  std::vector<std::array<int, 2>> coefs;
  int cstride() const
  {
    int c = 0;
    for (const auto& k : coefs) c += k[0] * k[1];
    return c;
  }
  std::string signature() const
  {
    std::string s;
    for (const auto& k : coefs) s += (s.empty() ? "(" : ", (") + std::to_string(k[0]) + ", " + std::to_string(k[1]) + ")";
    return "[" + s + "]";
  }
  std::string key() const
  {
    std::string s = std::to_string(tdim) + "/" + std::to_string(nd0) + "x" + std::to_string(bs0) + "/" + std::to_string(nd1) + "x"
                    + std::to_string(bs1);
    for (const auto& k : coefs) s += "/w" + std::to_string(k[0]) + "x" + std::to_string(k[1]);
    return s;
  }
};

// what a wrapper compiled for a coefficient list takes next to its argument struct: per Function its dof values, the
// dofmap of its own space and its shape (the shape is compile-time in the wrapper: CFX_W_ND<k>, CFX_W_BS<k>)
constexpr int kMaxCoefficients = 8;
constexpr int kMaxPacked = 64; // doubles of the thread-private `w`
struct RtcCoefArgs
{
  struct { const double* values; const int32_t* dofmap; int nd, bs; } c[kMaxCoefficients];
};

// the limits of a coefficient list: n Functions of (nd[k], bs[k]); `w` holds cstride doubles for a cell integral and
// 2 cstride for an interior facet
void check_coefficient_shapes(const char* who, bool facet, int n, const int* nd, const int* bs)
{
  require(n >= 0 && n <= kMaxCoefficients, CFX_ERR_INVALID_ARGUMENT,
          (std::string(who) + ": a coefficient list holds at most 8 Functions (0 <= n <= 8)").c_str());
  require(n == 0 || (nd && bs), CFX_ERR_INVALID_ARGUMENT, (std::string(who) + ": null argument").c_str());
  int cstride = 0;
  for (int k = 0; k < n; ++k)
  {
    require(nd[k] >= 1 && nd[k] <= 64 && bs[k] >= 1 && bs[k] <= 64, CFX_ERR_INVALID_ARGUMENT,
            (std::string(who) + ": every coefficient has at least one dof per cell and one component").c_str());
    cstride += nd[k] * bs[k];
    require(cstride <= (facet ? kMaxPacked / 2 : kMaxPacked), CFX_ERR_INVALID_ARGUMENT,
            (std::string(who) + ": the packed coefficients `w` hold at most 64 doubles per thread: cstride = sum nd_k * bs_k <= "
             + (facet ? "32 per cell for interior facets" : "64 for cell integrals") + " (the list asks for more)").c_str());
  }
}

std::vector<UserIntegrand>& integrands()
{
  static std::vector<UserIntegrand> v;
  return v;
}

// compile for (tdim, nd); no GPU needed (the code object is loaded on first launch)
// (registry and per-variant maps are shared state: one lock around every use)
std::mutex& rtc_mutex()
{
  static std::mutex m;
  return m;
}

std::string variant_defines(const Variant& v)
{
  auto def = [](const char* k, const std::string& val) { return std::string("#define ") + k + " " + val + "\n"; };
  std::string d = def("CFX_TDIM", std::to_string(v.tdim));
  if (v.nd1 == 0)
    d += def("CFX_ND", std::to_string(v.nd0)) + def("CFX_BS", std::to_string(v.bs0)) + def("CFX_NDB", "(CFX_ND * CFX_BS)")
         + def("CFXW_ND", "CFX_ND") + def("CFXW_NR", "CFX_NDB") + def("CFXW_NC", "CFX_NDB");
  else
    d += def("CFX_ND0", std::to_string(v.nd0)) + def("CFX_BS0", std::to_string(v.bs0)) + def("CFX_NDB0", "(CFX_ND0 * CFX_BS0)")
         + def("CFX_ND1", std::to_string(v.nd1)) + def("CFX_BS1", std::to_string(v.bs1)) + def("CFX_NDB1", "(CFX_ND1 * CFX_BS1)")
         + def("CFXW_ND", "CFX_ND0") + def("CFXW_NR", "CFX_NDB0") + def("CFXW_NC", "CFX_NDB1");
  if (!v.coefs.empty())
  {
    // a coefficient list: the shape and the offset in `w` of every Function (pack_form.h:69-158)
    d += def("CFX_NCOEF", std::to_string(v.coefs.size())) + def("CFX_CSTRIDE", std::to_string(v.cstride()));
    int off = 0;
    for (size_t k = 0; k < v.coefs.size(); ++k)
    {
      const std::string ks = std::to_string(k);
      d += def(("CFX_W_ND" + ks).c_str(), std::to_string(v.coefs[k][0])) + def(("CFX_W_BS" + ks).c_str(), std::to_string(v.coefs[k][1]))
           + def(("CFX_W_OFF" + ks).c_str(), std::to_string(off));
      off += v.coefs[k][0] * v.coefs[k][1];
    }
  }
  return d;
}

// The wrappers of a variant with a coefficient list: the texts above with the single-coefficient gather replaced by
// the in-thread gather of the list -- every Function through the dofmap of its own space, into w[CFX_CSTRIDE] (cells) or
// w[2 CFX_CSTRIDE] (interior facets: the block of cell 0, then of cell 1, per Function), loops over compile-time shapes.
// The descriptors travel as a second kernel argument.  Variants without a list compile the texts above unchanged.
std::string replace_n(std::string s, const std::string& from, const std::string& to, int times)
{
  int n = 0;
  for (size_t at = s.find(from); at != std::string::npos; at = s.find(from, at + to.size()), ++n) s.replace(at, from.size(), to);
  if (n != times) throw Error(CFX_ERR_RUNTIME, "user integrand: the stage-1 wrapper text does not hold '" + from + "'");
  return s;
}

std::string coefficient_pack_source(const Variant& v)
{
  std::string s = "struct RtcCoefArgs\n{\n  struct { const double* values; const cfx_i32* dofmap; int nd, bs; } c["
                  + std::to_string(kMaxCoefficients)
                  + "];\n};\n"
                    "// side s of the entity: MUL = 1 for cells, 2 for interior facets\n"
                    "template <int MUL>\n"
                    "__device__ __forceinline__ void cfx_pack_w(const RtcCoefArgs& CW, cfx_i64 cell, int s, double* w)\n{\n";
  for (size_t k = 0; k < v.coefs.size(); ++k)
  {
    const std::string ks = std::to_string(k), nd = "CFX_W_ND" + ks, bs = "CFX_W_BS" + ks, off = "CFX_W_OFF" + ks;
    s += "  for (int j = 0; j < " + nd + "; ++j)\n  {\n    const cfx_i64 d = CW.c[" + ks + "].dofmap[cell * " + nd + " + j];\n"
         + "    for (int b = 0; b < " + bs + "; ++b)\n      w[MUL * " + off + " + s * (" + nd + " * " + bs + ") + j * " + bs
         + " + b] = CW.c[" + ks + "].values[d * " + bs + " + b];\n  }\n";
  }
  return s + "}\n";
}

// Rank-0 integrands (functionals): the same stage-1 texts with another ending.  The local tensor is ONE double that the
// integrand adds to; the block then sums its 256 values -- a wave64 sum by __shfl_down, the four wave sums through LDS,
// both in a fixed order -- and stores one partial per block at out[blockIdx.x] (the engine's own second kernel adds the
// partials: cfx_scalar.hip).  The sum has a barrier, so no thread may leave before it: the early `return` of the entity
// range check becomes a predicate around the body, and a block wholly past the count stores the partial 0.
const char* kBlockStore = R"RTC(
__device__ __forceinline__ void cfx_block_store(double v, double* out)
{
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __shared__ double cfx_wave_sums[4];
  if ((threadIdx.x & 63) == 0) cfx_wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (cfx_wave_sums[0] + cfx_wave_sums[1]) + (cfx_wave_sums[2] + cfx_wave_sums[3]);
}
)RTC";

std::string rank0_text(const UserIntegrand& u)
{
  std::string w;
  if (u.kind == 1)
  {
    w = replace_n(kFacetWrapper, "  if (f >= n) return;\n", "  double cfx_m = 0.0;\n  if (f < n)\n  {\n", 1);
    w = replace_n(w, "  double T[4 * CFXW_NR * CFXW_NC];\n  for (int i = 0; i < 4 * CFXW_NR * CFXW_NC; ++i) T[i] = 0.0;\n",
                  "  double T[1] = {0.0};\n", 1);
    w = replace_n(w, "  for (int i = 0; i < 4 * CFXW_NR * CFXW_NC; ++i) A.out[f * (4 * CFXW_NR * CFXW_NC) + i] = T[i];\n}\n",
                  "  cfx_m = T[0];\n  }\n  cfx_block_store(cfx_m, A.out);\n}\n", 1);
  }
  else
  {
    w = replace_n(kWrapper, "  if (e >= n) return;\n", "  double cfx_m = 0.0;\n  if (e < n)\n  {\n", 1);
    w = replace_n(w, "  const int NT = A.rank == 2 ? CFXW_NR * CFXW_NC : CFXW_NR;\n", "", 1);
    w = replace_n(w, "  double T[CFXW_NR * CFXW_NC];\n  for (int i = 0; i < CFXW_NR * CFXW_NC; ++i) T[i] = 0.0;\n",
                  "  double T[1] = {0.0};\n", 1);
    w = replace_n(w,
                  "  if (A.out_mode == 0)\n    for (int i = 0; i < NT; ++i) A.out[e * NT + i] = T[i];\n  else\n  {\n"
                  "    const cfx_i64 at = A.out_mode == 2 ? cell : e;\n"
                  "    for (int i = 0; i < NT; ++i) A.out[(cfx_i64)i * A.out_stride + at] = T[i];\n  }\n}\n",
                  "  cfx_m = T[0];\n  }\n  cfx_block_store(cfx_m, A.out);\n}\n", 1);
  }
  return kBlockStore + w;
}

std::string wrapper_source(const UserIntegrand& u, const Variant& v)
{
  const std::string cell_text = u.rank == 0 && u.kind == 0 ? rank0_text(u) : std::string(kWrapper);
  const std::string facet_text = u.rank == 0 && u.kind == 1 ? rank0_text(u) : std::string(kFacetWrapper);
  if (v.coefs.empty()) return u.kind == 1 ? facet_text : cell_text;
  std::string w;
  if (u.kind == 1)
  {
    w = replace_n(facet_text, "cfx_facet_stage(const RtcFacetArgs& A)", "cfx_facet_stage(const RtcFacetArgs& A, const RtcCoefArgs& CW)", 1);
    w = replace_n(w,
                  "  double w[2 * CFXW_ND];\n  if (A.coeff)\n    for (int s = 0; s < 2; ++s)\n"
                  "      for (int j = 0; j < CFXW_ND; ++j) w[s * CFXW_ND + j] = A.coeff[A.dofmap[(s ? c1 : c0) * CFXW_ND + j]];\n",
                  "  double w[2 * CFX_CSTRIDE];\n  cfx_pack_w<2>(CW, c0, 0, w);\n  cfx_pack_w<2>(CW, c1, 1, w);\n", 1);
    w = replace_n(w, "cfx_user_stage1(RtcFacetArgs A) { cfx_facet_stage<false>(A); }",
                  "cfx_user_stage1(RtcFacetArgs A, RtcCoefArgs CW) { cfx_facet_stage<false>(A, CW); }", 1);
    w = replace_n(w, "cfx_user_stage1_rules(RtcFacetArgs A) { cfx_facet_stage<true>(A); }",
                  "cfx_user_stage1_rules(RtcFacetArgs A, RtcCoefArgs CW) { cfx_facet_stage<true>(A, CW); }", 1);
  }
  else
  {
    w = replace_n(cell_text, "cfx_user_stage1(RtcArgs A)", "cfx_user_stage1(RtcArgs A, RtcCoefArgs CW)", 1);
    w = replace_n(w,
                  "  double w[CFXW_NR];\n  if (A.coeff)\n    for (int j = 0; j < CFXW_ND; ++j)\n"
                  "      for (int b = 0; b < A.coeff_bs; ++b) w[j * A.coeff_bs + b] = A.coeff[(cfx_i64)A.dofmap[cell * CFXW_ND + j] * "
                  "A.coeff_bs + b];\n",
                  "  double w[CFX_CSTRIDE];\n  cfx_pack_w<1>(CW, cell, 0, w);\n", 1);
  }
  w = replace_n(w, "A.coeff ? w : (const double*)0", "w", 2);
  return coefficient_pack_source(v) + w;
}

const std::vector<char>& compiled(UserIntegrand& u, const Variant& v)
{
  const std::string key = v.key();
  auto it = u.code.find(key);
  if (it != u.code.end()) return it->second;
  Rtc& r = rtc();
  const std::string src = variant_defines(v) + "#define CFX_USER_FN " + u.name + "\n" + kPrelude + "\n" + u.source + "\n"
                          + wrapper_source(u, v);
  hiprtcProgram prog = nullptr;
  if (r.create(&prog, src.c_str(), (u.name + ".hip").c_str(), 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    throw Error(CFX_ERR_RUNTIME, "hiprtcCreateProgram failed");
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast"};
  const hiprtcResult rc = r.compile(prog, 4, opts);
  size_t ls = 0;
  r.log_size(prog, &ls);
  std::string log(ls, '\0');
  if (ls > 1) r.log(prog, log.data());
  if (rc != HIPRTC_SUCCESS)
  {
    r.destroy(&prog);
    throw Error(CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_register: the integrand '" + u.name + "' does not compile:\n" + log);
  }
  size_t cs = 0;
  r.code_size(prog, &cs);
  std::vector<char> code(cs);
  r.code(prog, code.data());
  r.destroy(&prog);
  return u.code.emplace(key, std::move(code)).first->second;
}

hipFunction_t function_of(UserIntegrand& u, const Variant& v, bool rules = false)
{
  const std::string key = v.key(), fkey = key + (rules ? "/rules" : "");
  auto it = u.function.find(fkey);
  if (it != u.function.end()) return it->second;
  auto mt = u.module.find(key);
  hipModule_t mod = mt != u.module.end() ? mt->second : nullptr;
  if (!mod)
  {
    const std::vector<char>& code = compiled(u, v);
    CFX_HIP(hipModuleLoadData(&mod, code.data()));
    u.module[key] = mod;
  }
  hipFunction_t fn = nullptr;
  CFX_HIP(hipModuleGetFunction(&fn, mod, rules ? "cfx_user_stage1_rules" : "cfx_user_stage1"));
  u.function[fkey] = fn;
  return fn;
}

// the variant a form asks of integrand u: its space, or (test, trial) when they differ; the integrand must have been
// registered for that kind of form
Variant form_variant(const cfx_form_s* a, const UserIntegrand& u, const cfx_integral_dev& I)
{
  const cfx_space_s* V = a->V;
  const bool rect = a->rectangular();
  require(u.two == rect, CFX_ERR_INVALID_ARGUMENT,
          rect ? "user integrand: a form between two spaces takes an integrand registered with cfx_integrand_register2"
               : "user integrand: an integrand registered with cfx_integrand_register2 serves forms between two spaces "
                 "(cfx_form_create2)");
  Variant v{V->mesh->tdim, V->ndofs_cell, V->bs};
  if (rect) { v.nd1 = a->V1->ndofs_cell; v.bs1 = a->V1->bs; }
  for (const cfx_coefficient_dev& c : I.coefficients) v.coefs.push_back({c.space->ndofs_cell, c.space->bs});
  return v;
}

// a variant with a coefficient list about to be launched (or attached to a form): within the limits of `w`, and -- once
// variants with a list were compiled ahead for this integrand -- one of those
void check_list_variant(const UserIntegrand& u, const Variant& v)
{
  if (v.coefs.empty()) return;
  std::vector<int> nd, bs;
  for (const auto& k : v.coefs) { nd.push_back(k[0]); bs.push_back(k[1]); }
  check_coefficient_shapes("cfx_form_set_coefficients", u.kind == 1, (int)nd.size(), nd.data(), bs.data());
  require(u.declared.empty() || u.declared.count(v.key()) > 0, CFX_ERR_INVALID_ARGUMENT,
          ("cfx_form_set_coefficients: the shapes of the coefficient list " + v.signature() + " on (tdim " + std::to_string(v.tdim)
           + ", " + std::to_string(v.nd0) + " x " + std::to_string(v.bs0) + (v.nd1 ? ", " + std::to_string(v.nd1) + " x " + std::to_string(v.bs1) : "")
           + ") differ from the signatures the integrand '" + u.name
           + "' was compiled for (cfx_integrand_compile_coefficients compiles another variant)").c_str());
}

// the descriptors of the list of integral I for the wrapper
RtcCoefArgs coefficient_args(const cfx_integral_dev& I)
{
  RtcCoefArgs CW{};
  int k = 0;
  for (const cfx_coefficient_dev& c : I.coefficients)
    CW.c[k++] = {c.values.p, c.space->dofmap.p, c.space->ndofs_cell, c.space->bs};
  return CW;
}

// reference rule of (dim, degree) in HBM for the wrapper (the engine's own kernels read the tables from their module)
struct RuleCopy { DevArray<double> points, weights; int n = 0; };
RuleCopy& reference_rule(int dim, int degree)
{
  static std::map<int, RuleCopy> cache;
  RuleCopy& rc = cache[dim * 100 + degree];
  if (rc.n == 0)
  {
    rc.n = quad_npoints(dim, degree);
    rc.points = to_device(quad_points_host(dim, degree), (int64_t)rc.n * dim);
    rc.weights = to_device(quad_weights_host(dim, degree), (int64_t)rc.n);
  }
  return rc;
}

bool user_integrand_known_locked(int kernel) { return kernel >= CFX_K_USER_BASE && kernel - CFX_K_USER_BASE < (int)integrands().size(); }

// one thread per entity, 256 per block, on the library stream -- with what cfx::launch does for the engine's own
// kernels: the launch trace, the 2^32 work-item check, HIP-event bracketing when profiling
void module_launch(hipFunction_t fn, int64_t n, void* args, void* coef_args = nullptr)
{
  void* kargs[] = {args, coef_args}; // (a wrapper without a coefficient list takes the first alone)
  const int64_t blocks = (n + 255) / 256;
  if (blocks * 256 > 0xffffffffll) throw Error(CFX_ERR_RUNTIME, "user_integrand: launch exceeds 2^32 threads");
  const unsigned grid = (unsigned)blocks;
  Context& c = ctx();
  c.last_launch = "user_integrand";
  if (env_present_once<Sw::LAUNCH_TRACE>()) fprintf(stderr, "cutfemx_amd: launch user_integrand grid %u\n", grid);
  if (c.profile)
  {
    hipEvent_t e0 = c.get_event(), e1 = c.get_event();
    CFX_HIP(hipEventRecord(e0, c.stream));
    CFX_HIP(hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, c.stream, kargs, nullptr));
    CFX_HIP(hipEventRecord(e1, c.stream));
    c.pending.push_back({c.entry("user_integrand"), e0, e1});
  }
  else
    CFX_HIP(hipModuleLaunchKernel(fn, grid, 1, 1, 256, 1, 1, 0, c.stream, kargs, nullptr));
}
} // namespace

namespace cfx
{
bool user_integrand_known(int kernel)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  return user_integrand_known_locked(kernel);
}
int user_integrand_rank(int kernel)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel), CFX_ERR_INVALID_ARGUMENT, "unknown user integrand id");
  return integrands()[kernel - CFX_K_USER_BASE].rank;
}
bool user_integrand_two(int kernel)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel), CFX_ERR_INVALID_ARGUMENT, "unknown user integrand id");
  return integrands()[kernel - CFX_K_USER_BASE].two;
}
int user_integrand_kind(int kernel)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel), CFX_ERR_INVALID_ARGUMENT, "unknown user integrand id");
  return integrands()[kernel - CFX_K_USER_BASE].kind;
}

// cfx_form_set_coefficients: the list now held by integral I of form a is one its integrand can be launched with
void user_coefficients_check(const cfx_form_s* a, const cfx_integral_dev& I)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(I.kernel), CFX_ERR_INVALID_ARGUMENT,
          "cfx_form_set_coefficients: a coefficient list goes with a registered integrand (the built-in kernel ids keep their "
          "single `coefficient`)");
  const UserIntegrand& u = integrands()[I.kernel - CFX_K_USER_BASE];
  check_list_variant(u, form_variant(a, u, I));
}

// stage 1 of a user integrand over the standard entities (runtime = false) or the runtime rules of integral I of form a:
// local tensors into `out` (out_mode / out_stride: see RtcArgs); `first` / `count` >= 0 restrict the launch to one entity.
// A form between two spaces stages [NDB0][NDB1] tensors (rows: test space, columns: trial space).
int64_t user_stage1(const cfx_form_s* a, const cfx_integral_dev& I, bool runtime, double* out, int out_mode, int64_t out_stride,
                    int64_t only_index)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  const cfx_space_s* V = a->V;
  require(user_integrand_known_locked(I.kernel), CFX_ERR_INVALID_ARGUMENT, "unknown user integrand id");
  require((V->degree == 1 || V->degree == 2) && (a->V1->degree == 1 || a->V1->degree == 2) && I.type == CFX_CELL,
          CFX_ERR_INVALID_ARGUMENT, "user integrands serve cell integrals of Lagrange spaces of degree 1 or 2");
  UserIntegrand& u = integrands()[I.kernel - CFX_K_USER_BASE];
  require(u.kind == 0, CFX_ERR_INVALID_ARGUMENT, "this user integrand was registered for interior-facet integrals");
  require(u.rank == a->rank, CFX_ERR_INVALID_ARGUMENT, "user integrand: the integrand's rank does not match the form");
  const Variant var = form_variant(a, u, I);
  check_list_variant(u, var);
  RtcCoefArgs CW = coefficient_args(I);
  void* cw = var.coefs.empty() ? nullptr : &CW;
  require(V->ndofs_cell * V->bs <= 30 && a->V1->ndofs_cell * a->V1->bs <= 30, CFX_ERR_INVALID_ARGUMENT,
          "user integrands: at most 30 local dofs");
  RtcArgs A{};
  A.x = V->mesh->x.p; A.conn = V->mesh->conn.p; A.dofmap = V->dofmap.p;
  A.rank = a->rank; A.runtime = runtime ? 1 : 0;
  for (int k = 0; k < 8; ++k) A.params[k] = I.params[k];
  A.coeff = I.coefficient.n > 0 && var.coefs.empty() ? I.coefficient.p : nullptr; // (a list replaces `coefficient`)
  A.coeff_bs = a->rank != 2 ? V->bs : 1; // (as the built-in kernels pack it: cfx_fem.hip, assemble_cells_kernel)
  A.out = out; A.out_mode = out_mode; A.out_stride = out_stride;
  DevN n;
  if (runtime)
  {
    require(I.rules != nullptr, CFX_ERR_INVALID_ARGUMENT, "user integrand: no runtime rules");
    const int64_t o = only_index >= 0 ? only_index : 0;
    A.offsets = I.rules->offsets.p + o; A.parent_map = I.rules->parent_map.p + o;
    A.points = I.rules->points.p; A.weights = I.rules->weights.p;
    // (offsets are absolute: the slices of points / weights / point_data start at offsets[e])
    A.point_data = I.point_data.n > 0 ? I.point_data.p : nullptr; A.point_stride = I.point_stride;
    n = only_index >= 0 ? DevN(1) : I.rules->nr.devn();
  }
  else
  {
    RuleCopy& rc = reference_rule(var.tdim, I.qdegree);
    require(rc.n <= 64, CFX_ERR_INVALID_ARGUMENT, "user integrand: the standard rule has more than 64 points");
    A.ref_points = rc.points.p; A.ref_weights = rc.weights.p; A.nref = rc.n;
    A.entities = I.entities.p + (only_index >= 0 ? only_index : 0);
    n = only_index >= 0 ? DevN(1) : I.n_entities.devn();
  }
  A.n_cap = n.cap; A.n_dev = n.dev;
  if (n.cap == 0) return 0;
  module_launch(function_of(u, var), n.cap, &A, cw);
  return (n.cap + 255) / 256;
}

// stage 1 of a user interior-facet integrand over the (c0, lf0, c1, lf1) rows of integral I: macro tensors
// [facet][2 NDB0][2 NDB1] into `out` (the layout the row gather and the scatters read); only_index >= 0: one facet.
// Entities past the standard facets integrate over the integral's facet-hosted rules.
int64_t user_stage1_facets(const cfx_form_s* a, const cfx_integral_dev& I, double* out, int64_t only_index)
{
  std::lock_guard<std::mutex> lock(rtc_mutex());
  const cfx_space_s* V = a->V;
  const cfx_space_s* V1 = a->V1;
  require(user_integrand_known_locked(I.kernel), CFX_ERR_INVALID_ARGUMENT, "unknown user integrand id");
  UserIntegrand& u = integrands()[I.kernel - CFX_K_USER_BASE];
  require(u.kind == 1 && I.type == CFX_INTERIOR_FACET, CFX_ERR_INVALID_ARGUMENT,
          "this user integrand was registered for cell integrals (cfx_integrand_register_facet registers facet integrands)");
  require((V->degree == 1 || V->degree == 2) && (V1->degree == 1 || V1->degree == 2) && (a->rank == 2 || a->rank == 0)
              && u.rank == a->rank,
          CFX_ERR_INVALID_ARGUMENT, "user facet integrands serve bilinear forms and functionals on Lagrange spaces of degree 1 or 2");
  const Variant var = form_variant(a, u, I);
  check_list_variant(u, var);
  RtcCoefArgs CW = coefficient_args(I);
  void* cw = var.coefs.empty() ? nullptr : &CW;
  require(2 * V->ndofs_cell * V->bs <= 24 && 2 * V1->ndofs_cell * V1->bs <= 24, CFX_ERR_INVALID_ARGUMENT,
          "user facet integrands: at most 24 macro dofs (scalar spaces of degree 1 or 2, vector spaces of degree 1)");
  RtcFacetArgs A{};
  A.x = V->mesh->x.p; A.conn = V->mesh->conn.p; A.dofmap = V->dofmap.p;
  for (int k = 0; k < 8; ++k) A.params[k] = I.params[k];
  A.coeff = I.coefficient.n > 0 && var.coefs.empty() ? I.coefficient.p : nullptr;
  RuleCopy& rc = reference_rule(var.tdim - 1, I.qdegree);
  require(rc.n <= 32, CFX_ERR_INVALID_ARGUMENT, "user facet integrand: the facet rule has more than 32 points");
  A.ref_points = rc.points.p; A.ref_weights = rc.weights.p; A.nref = rc.n;
  hipFunction_t fn_std = function_of(u, var, false);
  if (!(I.rules && I.n_std >= 0))
  {
    // standard facets only: the whole list, whose length may still be in HBM
    A.rows = I.entities.p + 4 * (only_index >= 0 ? only_index : 0);
    A.out = out;
    A.f0 = only_index >= 0 ? only_index : 0;
    A.n_std = INT64_MAX;
    const DevN n = only_index >= 0 ? DevN(1) : I.n_entities.devn();
    A.n_cap = n.cap; A.n_dev = n.dev;
    if (n.cap > 0) module_launch(fn_std, n.cap, &A, cw);
    return (n.cap + 255) / 256;
  }
  // [standard facets, facet-hosted rules] (exact lengths: form creation refuses a pending list next to the rules); the
  // rules' entry point gets the pulled-back points of every rule point in two [points][TDIM] arrays indexed by the rules'
  // own offsets -- a rule of any length, no truncation
  const int64_t lo = only_index >= 0 ? only_index : 0, hi = only_index >= 0 ? only_index + 1 : I.n_entities.value();
  const int64_t mid = std::min(std::max(I.n_std, lo), hi);
  const int64_t nt = 4 * (int64_t)V->ndofs_cell * V->bs * V1->ndofs_cell * V1->bs;
  const int64_t std_blocks = (mid - lo + 255) / 256; // (a functional: one partial per block, the rules' after the facets')
  A.n_std = I.n_std;
  if (mid > lo)
  {
    A.rows = I.entities.p + 4 * lo; A.out = out; A.f0 = lo;
    A.n_cap = mid - lo; A.n_dev = nullptr;
    module_launch(fn_std, A.n_cap, &A, cw);
  }
  if (hi > mid)
  {
    const int64_t nq = std::max<int64_t>(I.rules->nq.key(), 1);
    DevArray<double> scratch(2 * nq * var.tdim);
    A.offsets = I.rules->offsets.p; A.rpoints = I.rules->points.p; A.rweights = I.rules->weights.p;
    A.host_verts = I.rules->host_verts.p;
    A.scratch = scratch.p; A.scratch_stride = nq * var.tdim;
    A.rows = I.entities.p + 4 * mid; A.out = a->rank == 0 ? out + std_blocks : out + (mid - lo) * nt; A.f0 = mid;
    A.n_cap = hi - mid; A.n_dev = nullptr;
    module_launch(function_of(u, var, true), A.n_cap, &A, cw);
  }
  return std_blocks + (hi - mid + 255) / 256;
}
} // namespace cfx

extern "C" {

static int register_integrand(const char* name, const char* source, int rank, int kind, int tdim, int nd, int bs, int nd1,
                              int bs1, int* kernel_id)
{
  CFX_API_BEGIN
  const char* fn = nd1 > 0 ? "cfx_integrand_register2" : "cfx_integrand_register";
  require(name && source && kernel_id, CFX_ERR_INVALID_ARGUMENT, (std::string(fn) + ": null argument").c_str());
  require(rank == 0 || rank == 1 || rank == 2, CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_register: rank must be 0, 1 or 2");
  require(kind == 0 || rank != 1, CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_register_facet: interior-facet integrands are bilinear (or functionals: rank 0)");
  for (const char* p = name; *p; ++p)
    require((*p >= 'a' && *p <= 'z') || (*p >= 'A' && *p <= 'Z') || *p == '_' || (p != name && *p >= '0' && *p <= '9'),
            CFX_ERR_INVALID_ARGUMENT, (std::string(fn) + ": the name must be a C identifier").c_str());
  auto lagrange = [&](int n, int b) { return (n == tdim + 1 || n == (tdim + 1) * (tdim + 2) / 2) && b >= 1 && b <= 3; };
  require((tdim == 2 || tdim == 3) && nd >= tdim + 1 && nd <= 10 && bs >= 1 && bs <= 3, CFX_ERR_INVALID_ARGUMENT,
          (std::string(fn) + ": variant to validate: tdim 2 or 3, dofs per cell of a degree-1 or degree-2 space, block size 1..3").c_str());
  if (nd1 != 0)
  {
    require(lagrange(nd, bs) && lagrange(nd1, bs1), CFX_ERR_INVALID_ARGUMENT,
            "cfx_integrand_register2: variant (tdim, nd0, bs0, nd1, bs1): tdim 2 or 3, dofs per cell of a degree-1 or "
            "degree-2 space (tdim + 1 or (tdim + 1)(tdim + 2) / 2) and block size 1..3 for both spaces");
    require(kind == 0 || (2 * nd * bs <= 24 && 2 * nd1 * bs1 <= 24), CFX_ERR_INVALID_ARGUMENT,
            "cfx_integrand_register2: interior-facet integrands take at most 24 macro dofs on each side");
  }
  std::lock_guard<std::mutex> lock(rtc_mutex());
  UserIntegrand u;
  u.name = name; u.source = source; u.rank = rank; u.kind = kind; u.two = nd1 != 0;
  // compiled here for ONE variant so that a source that does not compile is refused at registration (no GPU needed:
  // hipRTC targets gfx950 explicitly); the other variants are compiled on first use
  Variant v{tdim, nd, bs, nd1, bs1};
  (void)compiled(u, v);
  integrands().push_back(std::move(u));
  *kernel_id = CFX_K_USER_BASE + (int)integrands().size() - 1;
  CFX_API_END
}

int cfx_integrand_register(const char* name, const char* source, int rank, int* kernel_id)
{
  return register_integrand(name, source, rank, 0, 3, 4, 1, 0, 0, kernel_id);
}

int cfx_integrand_register_facet(const char* name, const char* source, int* kernel_id)
{
  return register_integrand(name, source, 2, 1, 3, 4, 1, 0, 0, kernel_id);
}

int cfx_integrand_register_variant(const char* name, const char* source, int rank, int facet, int tdim, int ndofs_cell, int bs,
                                   int* kernel_id)
{
  return register_integrand(name, source, rank, facet ? 1 : 0, tdim, ndofs_cell, bs, 0, 0, kernel_id);
}

int cfx_integrand_register2(const char* name, const char* source, int facet, int tdim, int nd0, int bs0, int nd1, int bs1,
                            int* kernel_id)
{
  // (nd1 <= 0 is no trial space: refused by the variant check as a two-space variant)
  return register_integrand(name, source, 2, facet ? 1 : 0, tdim, nd0, bs0, nd1 > 0 ? nd1 : -1, bs1, kernel_id);
}

int cfx_integrand_compile(int kernel_id, int tdim, int ndofs_cell)
{
  return cfx_integrand_compile_bs(kernel_id, tdim, ndofs_cell, 1);
}

int cfx_integrand_compile_bs(int kernel_id, int tdim, int ndofs_cell, int bs)
{
  CFX_API_BEGIN
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel_id), CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_compile: unknown id");
  require((tdim == 2 || tdim == 3) && ndofs_cell >= tdim + 1 && ndofs_cell <= 10 && bs >= 1 && bs <= 3, CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile: tdim 2 or 3, dofs per cell of a degree-1 or degree-2 space, block size 1..3");
  UserIntegrand& u = integrands()[kernel_id - CFX_K_USER_BASE];
  require(!u.two, CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_compile: a two-space integrand compiles with cfx_integrand_compile2");
  (void)compiled(u, Variant{tdim, ndofs_cell, bs});
  CFX_API_END
}

int cfx_integrand_compile2(int kernel_id, int tdim, int nd0, int bs0, int nd1, int bs1)
{
  CFX_API_BEGIN
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel_id), CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_compile2: unknown id");
  UserIntegrand& u = integrands()[kernel_id - CFX_K_USER_BASE];
  require(u.two, CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile2: the integrand was registered for square forms (cfx_integrand_compile_bs)");
  auto lagrange = [&](int n, int b) { return (n == tdim + 1 || n == (tdim + 1) * (tdim + 2) / 2) && b >= 1 && b <= 3; };
  require((tdim == 2 || tdim == 3) && lagrange(nd0, bs0) && lagrange(nd1, bs1), CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile2: tdim 2 or 3, dofs per cell of a degree-1 or degree-2 space, block size 1..3");
  require(u.kind == 0 || (2 * nd0 * bs0 <= 24 && 2 * nd1 * bs1 <= 24), CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile2: interior-facet integrands take at most 24 macro dofs on each side");
  (void)compiled(u, Variant{tdim, nd0, bs0, nd1, bs1});
  CFX_API_END
}

int cfx_integrand_compile_coefficients(int kernel_id, int tdim, int nd0, int bs0, int nd1, int bs1, int n, const int* nd,
                                       const int* bs)
{
  CFX_API_BEGIN
  std::lock_guard<std::mutex> lock(rtc_mutex());
  require(user_integrand_known_locked(kernel_id), CFX_ERR_INVALID_ARGUMENT, "cfx_integrand_compile_coefficients: unknown id");
  UserIntegrand& u = integrands()[kernel_id - CFX_K_USER_BASE];
  auto lagrange = [&](int m, int b) { return (m == tdim + 1 || m == (tdim + 1) * (tdim + 2) / 2) && b >= 1 && b <= 3; };
  require((tdim == 2 || tdim == 3) && lagrange(nd0, bs0) && (nd1 == 0 || lagrange(nd1, bs1)), CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile_coefficients: tdim 2 or 3, dofs per cell of a degree-1 or degree-2 space, block size 1..3 "
          "(nd1 = 0: a square form)");
  require(u.two == (nd1 != 0), CFX_ERR_INVALID_ARGUMENT,
          u.two ? "cfx_integrand_compile_coefficients: a two-space integrand names its trial space (nd1, bs1)"
                : "cfx_integrand_compile_coefficients: the integrand was registered for square forms (nd1 = 0)");
  require(u.kind == 0 || (2 * nd0 * bs0 <= 24 && (nd1 == 0 || 2 * nd1 * bs1 <= 24)), CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile_coefficients: interior-facet integrands take at most 24 macro dofs on each side");
  require(n >= 1 || n > kMaxCoefficients, CFX_ERR_INVALID_ARGUMENT,
          "cfx_integrand_compile_coefficients: a list of 1 to 8 coefficients (cfx_integrand_compile_bs / _compile2 compile the "
          "variant without a list)");
  check_coefficient_shapes("cfx_integrand_compile_coefficients", u.kind == 1, n, nd, bs);
  Variant v{tdim, nd0, bs0, nd1, nd1 ? bs1 : 0};
  for (int k = 0; k < n; ++k) v.coefs.push_back({nd[k], bs[k]});
  (void)compiled(u, v);
  u.declared.insert(v.key());
  CFX_API_END
}

} // extern "C"
