"""The SUPG level-set step of python/demo/demo_compliance_optimization.py:1302-1350 / :1973-1993 (the default
`--advection` method of the shape-optimisation demo) expressed with the engine's descriptors: one implicit Euler step of
phi_t + speed |grad phi| = 0 with streamline-upwind stabilisation, assembled over every cell of the mesh and solved in
HBM by BiCGStab (fem.bicgstab_solve) -- the demo hands the nonsymmetric matrix to spsolve.

V is scalar P1 on the geometry dofmap, 2-D or 3-D.  With n_K = grad(phi) / sqrt(|grad phi|^2 + 1e-14) (constant per
cell), a = speed n_K (speed P1), h the cell diameter (largest vertex distance) and
tau = tau_scale / sqrt((2 / dt)^2 + (2 sqrt(|a|^2 + 1e-14) / h)^2 + 1e-30):

    A(u, w) = int u w + dt (a . grad u) w + tau (u + dt a . grad u)(a . grad w) dx
    b(w)    = int phi w + tau phi (a . grad w) dx

(the regularisations are the demo's, :1316-1322).  phi and speed are the coefficient list of two registered (hipRTC)
integrands, dt and tau_scale their `Integral.params`.  The integrand is NOT a polynomial (tau is a rational function of
the point through speed), so the quadrature rule is part of the contract: every cell is integrated with the engine's
standard rule of `qdegree` (default 2; the rule of cutfemx_amd.full_cell_rules(mesh, cells, qdegree)).

The params of a live form cannot be changed: a new dt (or tau_scale) builds new forms with `with_dt`, from the same two
kernel ids and therefore without a new compilation; new VALUES of phi and speed need nothing (advect attaches the
current `system.phi.values` / `system.speed.values` on every call)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib, fem
from .mesh import Function

_COMMON = r"""
// the P1 gradients g[i][d] of the cell, n_K . g[i] (n_K the regularised unit gradient of phi) and n_K . n_K
__device__ inline void supg_cell(const double* coordinate_dofs, const double* phi, double* ng, double* nn)
{
  static_assert(CFX_ND == CFX_TDIM + 1, "a scalar P1 space (phi and speed are Functions of it: CFX_ND dofs each)");
  double K[CFX_TDIM][CFX_TDIM], N[CFX_ND], dN[CFX_ND][CFX_TDIM], g[CFX_ND][CFX_TDIM], gphi[CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  const double X0[3] = {0.0, 0.0, 0.0};
  cfx_tabulate(X0, N, dN);
  for (int d = 0; d < CFX_TDIM; ++d) gphi[d] = 0.0;
  for (int i = 0; i < CFX_ND; ++i)
    for (int d = 0; d < CFX_TDIM; ++d)
    {
      double v = 0.0;
      for (int t = 0; t < CFX_TDIM; ++t) v += dN[i][t] * K[t][d];
      g[i][d] = v;
      gphi[d] += phi[i] * v;
    }
  double g2 = 0.0;
  for (int d = 0; d < CFX_TDIM; ++d) g2 += gphi[d] * gphi[d];
  const double inv = 1.0 / sqrt(g2 + 1.0e-14);
  *nn = g2 * inv * inv;
  for (int i = 0; i < CFX_ND; ++i)
  {
    double v = 0.0;
    for (int d = 0; d < CFX_TDIM; ++d) v += gphi[d] * g[i][d];
    ng[i] = v * inv;
  }
}

// tau at a point where the speed is s: a = s n_K
__device__ inline double supg_tau(double s, double nn, double h, double dt, double tau_scale)
{
  const double adv = sqrt(s * s * nn + 1.0e-14), p = 2.0 / dt, q = 2.0 * adv / h;
  return tau_scale / sqrt(p * p + q * q + 1.0e-30);
}
"""

LHS_SOURCE = _COMMON + r"""
__device__ void cfx_supg_lhs(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                             const double* points, const double* weights, const double* point_data)
{
  const double dt = c[0], tau_scale = c[1], h = cfx_cell_diameter(coordinate_dofs);
  const double* speed = w + CFX_W_OFF1;
  double ng[CFX_ND], nn;
  supg_cell(coordinate_dofs, w + CFX_W_OFF0, ng, &nn);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    double s = 0.0;
    for (int j = 0; j < CFX_ND; ++j) s += N[j] * speed[j];
    const double tau = supg_tau(s, nn, h, dt, tau_scale);
    for (int i = 0; i < CFX_ND; ++i)       // test function
      for (int j = 0; j < CFX_ND; ++j)     // trial function
      {
        const double u = N[j], au = s * ng[j], aw = s * ng[i];
        A[i * CFX_ND + j] += weights[q] * (u * N[i] + dt * au * N[i] + tau * (u + dt * au) * aw);
      }
  }
}
"""

RHS_SOURCE = _COMMON + r"""
__device__ void cfx_supg_rhs(double* b, const double* w, const double* c, const double* coordinate_dofs, int nq,
                             const double* points, const double* weights, const double* point_data)
{
  const double dt = c[0], tau_scale = c[1], h = cfx_cell_diameter(coordinate_dofs);
  const double* phi = w + CFX_W_OFF0;
  const double* speed = w + CFX_W_OFF1;
  double ng[CFX_ND], nn;
  supg_cell(coordinate_dofs, phi, ng, &nn);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    double s = 0.0, f = 0.0;
    for (int j = 0; j < CFX_ND; ++j)
    {
      s += N[j] * speed[j];
      f += N[j] * phi[j];
    }
    const double tau = supg_tau(s, nn, h, dt, tau_scale);
    for (int i = 0; i < CFX_ND; ++i) b[i] += weights[q] * (f * N[i] + tau * f * s * ng[i]);
  }
}
"""

VARIANTS = ((2, 3, 1), (3, 4, 1))     # (tdim, dofs per cell, block size) of the registered variants
_kernels: dict = {}


def kernel_ids() -> tuple[int, int]:
    """(bilinear id, linear id) of the two integrands: registered once per process, both variants compiled (for gfx950
    with hipRTC; needs no GPU)."""
    if not _kernels:
        ids = []
        for name, src, rank in (("cfx_supg_lhs", LHS_SOURCE, 2), ("cfx_supg_rhs", RHS_SOURCE, 1)):
            tdim, nd, bs = VARIANTS[0]
            kid = fem.register_integrand(name, src, rank=rank, variant=VARIANTS[0], coefficients=[(nd, 1), (nd, 1)])
            for tdim, nd, bs in VARIANTS[1:]:
                fem.compile_integrand(kid, tdim, nd, bs, coefficients=[(nd, 1), (nd, 1)])
            ids.append(kid)
        _kernels["ids"] = tuple(ids)
    return _kernels["ids"]


@dataclass
class SupgSystem:
    function_space: object
    phi: Function           # the level set of the step: its CURRENT values are used by every advect call
    speed: Function         # the normal speed (P1 on the same space)
    dt: float
    tau_scale: float
    qdegree: int
    fixed_dofs: object      # int32 numpy array (may be empty)
    marker: object          # int8 marker of the fixed dofs, or None
    rows: object            # the free rows (int32), or None: all rows are solved
    cells: object
    a: object
    L: object


def _forms(V, phi, speed, dt, tau_scale, qdegree, cells):
    lhs, rhs = kernel_ids()
    params = (float(dt), float(tau_scale))
    a = fem.form([fem.Integral(lhs, cells=cells, params=params, qdegree=qdegree, coefficients=(phi, speed))], V)
    L = fem.form([fem.Integral(rhs, cells=cells, params=params, qdegree=qdegree, coefficients=(phi, speed))], V)
    return a, L


def build_forms(V, phi, speed, dt: float, *, tau_scale: float = 1.0, qdegree: int = 2, fixed_dofs=None) -> SupgSystem:
    """The two forms of the step over every cell of the mesh of `V` (scalar P1 on the geometry dofmap).  `phi`, `speed`:
    Functions of V or their dof values (numpy, or device torch tensors, which stay where they are).  `fixed_dofs`: dofs
    that keep their value of phi (the demo's DirichletBC with the old phi on the fixed facets)."""
    mesh = V.mesh
    if V.degree != 1 or V.bs != 1 or V.ndofs != mesh.num_nodes:
        raise ValueError("supg.build_forms: V is a scalar P1 space on the geometry dofmap")
    if not dt > 0.0:
        raise ValueError("supg.build_forms: dt > 0")
    phi = phi if isinstance(phi, Function) else Function(V, phi, "phi")
    speed = speed if isinstance(speed, Function) else Function(V, speed, "advection_speed")
    cells = np.arange(mesh.num_cells, dtype=np.int32)
    fixed = np.zeros(0, dtype=np.int32) if fixed_dofs is None else np.unique(np.asarray(fixed_dofs, dtype=np.int32))
    marker = rows = None
    if fixed.size > 0:
        if fixed[0] < 0 or fixed[-1] >= V.ndofs:
            raise ValueError("supg.build_forms: a fixed dof lies outside the space")
        marker = np.zeros(V.ndofs, dtype=np.int8)
        marker[fixed] = 1
        rows = np.flatnonzero(marker == 0).astype(np.int32)
    a, L = _forms(V, phi, speed, dt, tau_scale, qdegree, cells)
    return SupgSystem(V, phi, speed, float(dt), float(tau_scale), int(qdegree), fixed, marker, rows, cells, a, L)


def with_dt(system: SupgSystem, dt: float, tau_scale: float | None = None) -> SupgSystem:
    """`system` with another dt (and tau_scale): new forms from the same kernel ids -- no compilation; the Functions,
    the fixed dofs and the cell list are shared."""
    ts = system.tau_scale if tau_scale is None else float(tau_scale)
    a, L = _forms(system.function_space, system.phi, system.speed, dt, ts, system.qdegree, system.cells)
    return SupgSystem(system.function_space, system.phi, system.speed, float(dt), ts, system.qdegree, system.fixed_dofs,
                      system.marker, system.rows, system.cells, a, L)


def assemble(system: SupgSystem):
    """(A, b) of the step with the CURRENT values of system.phi / system.speed: assemble_matrix(bcs=marker) -- rows and
    columns of the fixed dofs zeroed --, assemble_vector, apply_lifting and set_bc with phi on the fixed dofs.  `b` is a
    device torch tensor when phi's values are one, a numpy array otherwise."""
    V = system.function_space
    for form in (system.a, system.L):
        form.set_coefficients(0, (system.phi, system.speed))
    A = fem.assemble_matrix(system.a, bcs=system.marker)
    values = system.phi.values
    if _lib.is_torch(values) and values.is_cuda:
        import torch
        b = torch.zeros(V.ndofs, dtype=torch.float64, device=values.device)
    else:
        b = np.zeros(V.ndofs)
    fem.assemble_vector(system.L, b)
    if system.marker is not None:
        fem.apply_lifting(b, system.a, system.marker, values)
        fem.set_bc(b, system.marker, values)
    return A, b


def advect(system: SupgSystem, *, rtol: float = 1e-10, max_iter: int | None = None, check_every: int | None = None,
           info_out=None):
    """One SUPG step: assemble(system), then Jacobi-preconditioned BiCGStab from x0 = phi over the free rows (the fixed
    dofs are not iterated: they keep phi bit for bit).  Returns (phi_new, info): phi_new of the kind of phi's values
    (device values stay on the device); system.phi is NOT modified -- the caller assigns `system.phi.values = phi_new`.
    Two calls give the same bits; with fixed dofs only to rounding (fem.apply_lifting adds with atomics).
    rtol, max_iter, check_every, info_out: those of fem.bicgstab_solve."""
    A, b = assemble(system)
    return fem.bicgstab_solve(A, b, x0=system.phi.values, rtol=rtol, max_iter=max_iter, check_every=check_every,
                              info_out=info_out, rows=system.rows)
