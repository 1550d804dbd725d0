"""Cut Brinkman / Stokes problem on the equal-order P1 vector x P1 pair, stabilised by ghost penalties, expressed with the
engine's integral descriptors: the block system of python/demo/demo_stokes.py and python/tests/test_assembly_stokes.py,
assembled, merged and solved without leaving HBM.

    [[A, B^T], [B, -G_p]] (u, p) = (b_u, b_p)
    A   = (grad u, grad v)_Omega + sigma (u, v)_Omega + gamma_u h_avg ([dn u], [dn v])_{F_G}
    B^T = -(div v, p)_Omega,   B = -(q, div u)_Omega
    G_p = gamma_p h_avg^3 ([dn p], [dn q])_{F_h}      F_h: every interior facet of the active cells (dS_pressure)

What this is NOT: the Nitsche traction terms and the Dirichlet data of demo_stokes.py:171-231 couple velocity and pressure
on the interface and need registered two-space interface integrands; they are not built here.  The velocity is pinned
by the reaction term sigma (u, v) instead, the right-hand side is the caller's.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import fem
from .cut import ghost_penalty_facets, interior_facets_for_cells, locate_entities, locate_entities_device, runtime_quadrature


@dataclass
class StokesSystem:
    cut_data: object
    velocity_space: object
    pressure_space: object
    inside_cells: tuple
    volume_rules: object
    ghost_facets: object
    pressure_facets: object
    forms: list             # [[a_uu, a_up], [a_pu, a_pp]]
    pressure_support: object  # the MASS form whose active domain is the pressure's


def build_blocks(VU, VP, cut_data, *, order: int = 4, sigma: float = 1.0, gamma_u: float = 0.1,
                 gamma_p: float = 0.1) -> StokesSystem:
    """The four block forms on `VU` (P1, bs = tdim) and `VP` (P1) over the domain {phi < 0} of `cut_data`."""
    mesh = VU.mesh
    if VU.degree != 1 or VP.degree != 1 or VU.bs != mesh.tdim or VP.bs != 1:
        raise ValueError("stokes.build_blocks takes a P1 velocity space with bs = tdim and a P1 pressure space")
    inside = locate_entities_device(cut_data, "phi<0")
    vol = runtime_quadrature(cut_data, "phi<0", order)
    ghost = ghost_penalty_facets(cut_data, "phi<0")
    skeleton = interior_facets_for_cells(mesh, locate_entities(cut_data, "phi<=0"))
    # sigma multiplies the mass integrand as a (constant) scalar coefficient of the form's element
    kappa = np.full(VU.ndofs * VU.bs, float(sigma))
    a_uu = [fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=0),
            fem.Integral(fem.MASS, cells=inside, rules=vol, qdegree=2, coefficient=kappa)]
    if ghost.size > 0:
        a_uu.append(fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(gamma_u,), qdegree=0))
    a_pp = [fem.Integral(fem.GHOST_GRADJUMP, facets=skeleton, params=(-gamma_p, 2.0), qdegree=0)]
    a_up = [fem.Integral(fem.DIV_TEST, cells=inside, rules=vol, params=(-1.0,), qdegree=1)]
    a_pu = [fem.Integral(fem.DIV_TRIAL, cells=inside, rules=vol, params=(-1.0,), qdegree=1)]
    forms = [[fem.form(a_uu, VU), fem.form(a_up, VU, trial_space=VP)],
             [fem.form(a_pu, VP, trial_space=VU), fem.form(a_pp, VP)]]
    support = fem.form([fem.Integral(fem.MASS, cells=inside, rules=vol, qdegree=2)], VP)
    return StokesSystem(cut_data, VU, VP, inside, vol, ghost, skeleton, forms, support)


def assemble(system: StokesSystem):
    """(M, rows, domains): the four blocks assembled, the diagonal blocks deactivated outside their active domains
    (fem.deactivate_outside_blocks: identity rows), merged into ONE CSR matrix in HBM (fem.merge_blocks, block-ordered
    dofs: velocity, then pressure); `rows`: the active rows of both blocks as an int32 device tensor -- the velocity
    rows, then nu + the pressure rows, ascending."""
    import torch
    blocks = [[fem.assemble_matrix(a) for a in row] for row in system.forms]
    domains = [fem.active_domain(system.forms[0][0]), fem.active_domain(system.pressure_support)]
    fem.deactivate_outside_blocks(blocks, domains)
    M = fem.merge_blocks(blocks)
    nu = system.velocity_space.ndofs * system.velocity_space.bs
    rows = torch.cat([fem.active_rows(domains[0]), fem.active_rows(domains[1]) + nu]).to(torch.int32).contiguous()
    return M, rows, domains


def solve(system: StokesSystem, b_u, b_p, **kw):
    """Assemble, deactivate, merge and solve the block system without leaving HBM: assemble(system), then MINRES over the
    active rows (fem.minres_solve, which takes `kw`: rtol, max_iter, precond, check_every ...) -- the spsolve of
    python/demo/demo_stokes.py:39-60.  `b_u` / `b_p`: the right-hand sides of the two block rows, numpy arrays or device
    tensors; their entries on inactive rows are not read.  Returns (u, p, info): float64 device tensors with 0 on the
    inactive dofs."""
    import torch
    M, rows, _ = assemble(system)
    dev = rows.device
    b = torch.cat([torch.as_tensor(b_u, dtype=torch.float64, device=dev).reshape(-1),
                   torch.as_tensor(b_p, dtype=torch.float64, device=dev).reshape(-1)]).contiguous()
    x, info = fem.minres_solve(M, b, rows=rows, **kw)
    nu = system.velocity_space.ndofs * system.velocity_space.bs
    return x[:nu], x[nu:], info
