"""Shared problem builders for the parity tests: the same synthetic inputs
 fed to the CPU oracle and to the HIP engine."""
from __future__ import annotations

import numpy as np

CIRCLE = (np.array([0.47, 0.43]), 0.31)           # python/tests/test_cut_api.py:36-38
SPHERE = (np.array([0.47, 0.43, 0.41]), 0.31)     # python/tests/test_cut_api.py:50-52


def level_set_values(x: np.ndarray, tdim: int, kind: str = "sphere") -> np.ndarray:
    if kind == "sphere":
        c, r = CIRCLE if tdim == 2 else SPHERE
        return np.linalg.norm(x[:, :tdim] - c, axis=1) - r
    if kind == "gyroid":
        k = 2.0 * np.pi * 4.0 if tdim == 3 else 2.0 * np.pi * 2.0
        X, Y = x[:, 0], x[:, 1]
        Z = x[:, 2] if tdim == 3 else 0.3 * np.ones_like(X)
        return (np.sin(k * X) * np.cos(k * Y) + np.sin(k * Y) * np.cos(k * Z)
                + np.sin(k * Z) * np.cos(k * X)) + 0.0137
    if kind == "plane":
        return x[:, 0] - 0.51
    raise ValueError(kind)


def oracle_poisson(O, mesh, phi, order=4, gamma=40.0, gamma_g=0.1, degree=1, dofmap=None, ndofs=None):
    """Oracle restatement of the demo_poisson.py system on `mesh`."""
    dom = O.classify(mesh.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    vol = O.runtime_quadrature(mesh, mesh.conn, phi, dom, "phi<0", order)
    itf = O.runtime_quadrature(mesh, mesh.conn, phi, dom, "phi=0", order)
    normals = O.evaluate_normals(mesh, mesh.conn, phi, itf)
    ghost = O.ghost_penalty_facets(mesh, dom, "phi<0")
    V = O.Space(mesh.conn if dofmap is None else dofmap, mesh.nnodes if ndofs is None else ndofs, degree)
    a = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=vol, qdegree=2 * (degree - 1)),
         O.Integral(O.CELL, O.K_NITSCHE, rules=itf, point_data=normals, params=(gamma,))]
    if len(ghost):
        a.append(O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=ghost, params=(gamma_g,),
                            qdegree=2 * (degree - 1)))
    L = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=vol, params=(O.F_POISSON_RHS, 1.0), qdegree=4),
         O.Integral(O.CELL, O.L_NITSCHE_RHS, rules=itf, point_data=normals, params=(gamma, O.F_SINPROD, 1.0))]
    indptr, indices = O.create_sparsity(mesh, V, a)
    values = O.assemble_matrix(mesh, V, a, indptr, indices)
    b = O.assemble_vector(mesh, V, L)
    active = O.active_cells(a, mesh.ncells)
    inactive = O.inactive_dofs(V, active)
    return dict(domain=dom, inside=inside, vol=vol, itf=itf, normals=normals, ghost=ghost, V=V, a=a, L=L,
                indptr=indptr, indices=indices, values=values, b=b, active=active, inactive=inactive)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.max(np.abs(b)) if b.size else 0.0, 1e-300)
    return float(np.max(np.abs(a - b)) / scale) if a.size else 0.0


def scrambled_mesh(O, tdim: int, n: int, seed: int = 11):
    """The n^tdim Kuhn box mesh made unstructured: interior vertices moved by up to 0.2 h,
    vertices and cells renumbered at random, local vertex order of every cell shuffled (both
    orientations occur).  Nothing of the generator's numbering survives."""
    rng = np.random.default_rng(seed)
    om = O.mesh_box(tdim, n)
    x = om.x.copy()
    interior = np.all((x[:, :tdim] > 1e-12) & (x[:, :tdim] < 1.0 - 1e-12), axis=1)
    x[interior, :tdim] += (0.2 / n) * rng.uniform(-1.0, 1.0, size=(int(interior.sum()), tdim))
    p = rng.permutation(om.nnodes)                 # new id of old vertex v: p[v]
    xn = np.empty_like(x)
    xn[p] = x
    conn = p[om.conn]
    conn = conn[rng.permutation(om.ncells)]
    conn = rng.permuted(conn, axis=1)
    return O.Mesh(tdim, xn, conn.astype(np.int32))


def cone_mesh(tdim: int, shape):
    """A double cone over a triangulated (tdim-1)-grid: vertices of high valence, which no Kuhn mesh has.  The base -- a
    chain of `shape` = m segments (2-D), or an mx x my grid of squares, each split into two triangles (3-D, `shape` =
    (mx, my) or one number for both) -- lies at height 0.5 in the last coordinate over [0,1]^(tdim-1); one apex sits at
    height 0 above (0.5, ..), the other at height 1 above (0.45, ..).  Every base cell is joined to each apex (lower
    cone first, then the upper one): 2 * (base cells) simplices.  The base vertices come first, then the lower and the
    upper apex.  The mesh-static P1 stencil of an apex, itself included, is every base vertex + 1."""
    from oracle import pyoracle
    if tdim == 2:
        m = int(shape)
        nb = m + 1
        x = np.zeros((nb + 2, 3))
        x[:nb, 0] = np.arange(nb) / m
        x[:nb, 1] = 0.5
        base = np.stack([np.arange(m), np.arange(m) + 1], axis=1)
        x[nb] = (0.5, 0.0, 0.0)
        x[nb + 1] = (0.45, 1.0, 0.0)
    elif tdim == 3:
        mx, my = (int(shape), int(shape)) if np.isscalar(shape) else (int(shape[0]), int(shape[1]))
        nb = (mx + 1) * (my + 1)
        i, j = np.meshgrid(np.arange(mx + 1), np.arange(my + 1), indexing="ij")
        x = np.zeros((nb + 2, 3))
        x[:nb, 0] = i.ravel() / mx
        x[:nb, 1] = j.ravel() / my
        x[:nb, 2] = 0.5
        vid = lambda a, b: a * (my + 1) + b
        ci, cj = np.meshgrid(np.arange(mx), np.arange(my), indexing="ij")
        ci, cj = ci.ravel(), cj.ravel()
        lo = np.stack([vid(ci, cj), vid(ci + 1, cj), vid(ci + 1, cj + 1)], axis=1)
        up = np.stack([vid(ci, cj), vid(ci + 1, cj + 1), vid(ci, cj + 1)], axis=1)
        base = np.stack([lo, up], axis=1).reshape(-1, 3)
        x[nb] = (0.5, 0.5, 0.0)
        x[nb + 1] = (0.45, 0.45, 1.0)
    else:
        raise ValueError(tdim)
    nbc = base.shape[0]
    conn = np.concatenate([np.column_stack([base, np.full(nbc, nb)]), np.column_stack([base, np.full(nbc, nb + 1)])])
    return pyoracle.Mesh(tdim, x, conn.astype(np.int32))


def mesh_union(a, b, shift):
    """Disjoint union of two meshes: `b` translated by `shift` (a vector, or a number for the x direction alone), its
    vertex ids offset by the vertices of `a`; the cells of `a` come first."""
    from oracle import pyoracle
    assert a.tdim == b.tdim
    s = np.zeros(3)
    s[:np.size(shift)] = np.atleast_1d(np.asarray(shift, dtype=np.float64))
    x = np.concatenate([a.x, b.x + s])
    conn = np.concatenate([a.conn, b.conn + a.nnodes])
    return pyoracle.Mesh(a.tdim, x, conn.astype(np.int32))


# The shapes of the high-valence tests.  (tdim, shape): (static P1 stencil of an apex, itself included; longest oracle row
# of the P1 Poisson system with Nitsche + ghost penalty; longest row of the stiffness over the inside cells alone), all on
# cone_mesh(tdim, shape) joined with mesh_box(tdim, 4).  With the ghost penalty both apex rows couple to each other and
# to the whole base (base + 2); without it the lower apex's row is its static stencil.  The 3-D box's own longest rows
# are 23 (Poisson) and 15.
HIGH_VALENCE_P1 = {
    (2, 14): (16, 17, 16), (2, 15): (17, 18, 17), (2, 30): (32, 33, 32), (2, 31): (33, 34, 33), (2, 61): (63, 64, 63),
    (2, 62): (64, 65, 64), (2, 70): (72, 73, 72),
    (3, (2, 4)): (16, 23, 16), (3, (3, 3)): (17, 23, 17), (3, (4, 4)): (26, 27, 26), (3, (3, 7)): (33, 34, 33),
    (3, (1, 30)): (63, 64, 63), (3, (6, 8)): (64, 65, 64), (3, (7, 7)): (65, 66, 65),
    (3, (6, 6)): (50, 51, 50), (3, (8, 8)): (82, 83, 82), (3, (10, 10)): (122, 123, 122),
}
# degree 2, 3-D, shape (m, m): (longest row of the P2 Poisson system, of the stiffness over the inside cells alone --
# from m = 3 on that is the lower apex's static list, on m = 2 the 65 of a Kuhn-mesh vertex)
HIGH_VALENCE_P2 = {2: (102, 65), 3: (102, 66), 4: (133, 107), 6: (269, 219), 7: (355, 290), 10: (685, 563)}


def _cone_plane(x, tdim, level):
    return x[:, tdim - 1] + 0.13 * x[:, 0] + (0.07 * x[:, 1] if tdim == 3 else 0.0) - level


def high_valence_case(O, tdim: int, shape, nbox: int = 4):
    """The mesh of the high-valence tests: cone_mesh(tdim, shape) joined with the Kuhn box mesh_box(tdim, nbox) moved
    by +2 in x, so that rows of 7 or 15 entries and the long apex rows go through the same launches.  Level set: on the
    cone the plane x_last + 0.13 x_0 (+ 0.07 x_1) = 0.8 -- every lower-cone cell inside, every upper-cone cell cut, the
    upper apex outside; on the box the same function lowered by 0.3, so that the box has inside, cut and outside cells.
    No value vanishes at a vertex.  Returns (mesh, phi, info): info has the cone's and the box's cell ranges, the two
    apex vertices and the number of base vertices."""
    cone = cone_mesh(tdim, shape)
    box = O.mesh_box(tdim, nbox)
    om = mesh_union(cone, box, 2.0)
    phi = _cone_plane(om.x, tdim, 0.8)
    phi[cone.nnodes:] -= 0.3
    assert np.all(phi != 0.0)
    nb = cone.nnodes - 2
    half = cone.ncells // 2
    info = dict(nbase=nb, lower_apex=nb, upper_apex=nb + 1, lower_cells=np.arange(half), upper_cells=np.arange(half, 2 * half),
                box_cells=np.arange(cone.ncells, om.ncells), cone_nodes=cone.nnodes)
    return om, phi, info


def oracle_stiffness_source(O, mesh, phi, degree=1, dofmap=None, ndofs=None):
    """Oracle system of the inside cells alone: the stiffness over locate_entities("phi<0") and the SOURCE / F_SINPROD
    linear form over the same cells, no rule, no facet term.  The rows of dofs that no cut cell touches are complete,
    uncut rows (the engine's plain rows)."""
    dom = O.classify(mesh.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    V = O.Space(mesh.conn if dofmap is None else dofmap, mesh.nnodes if ndofs is None else ndofs, degree)
    a = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, qdegree=2 * (degree - 1))]
    L = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, params=(O.F_SINPROD, 1.0), qdegree=4)]
    indptr, indices = O.create_sparsity(mesh, V, a)
    values = O.assemble_matrix(mesh, V, a, indptr, indices)
    b = O.assemble_vector(mesh, V, L)
    active = O.active_cells(a, mesh.ncells)
    inactive = O.inactive_dofs(V, active)
    return dict(domain=dom, inside=inside, V=V, a=a, L=L, indptr=indptr, indices=indices, values=values, b=b,
                active=active, inactive=inactive)


def oracle_dg_poisson(O, mesh, phi, degree=1, order=4, sigma=10.0, sigma_gamma=20.0, gamma_g=0.1):
    """Oracle restatement of python/demo/demo_dg_poisson.py:205-277 on `mesh`: cut DG Poisson problem on
    {phi < 0}: volume terms on [inside cells, cut-cell rules], symmetric interior penalty on the skeleton of the
    active mesh restricted to the domain ([facets inside, rules of the cut facets]), Nitsche on the interface,
    ghost penalty on the cut band."""
    nd = {1: mesh.tdim + 1, 2: (mesh.tdim + 1) * (mesh.tdim + 2) // 2}[degree]
    ndofs = mesh.ncells * nd
    dofmap = np.arange(ndofs, dtype=np.int32).reshape(mesh.ncells, nd)
    V = O.Space(dofmap, ndofs, degree)
    dom = O.classify(mesh.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    active = O.locate_entities(dom, "phi<=0")
    vol = O.runtime_quadrature(mesh, mesh.conn, phi, dom, "phi<0", order)
    itf = O.runtime_quadrature(mesh, mesh.conn, phi, dom, "phi=0", order)
    normals = O.evaluate_normals(mesh, mesh.conn, phi, itf)
    skeleton = O.interior_facets_for_cells(mesh, active)
    H = O.facet_hosts(mesh, skeleton, mesh.conn)
    fdom = O.facet_classify(H, phi)
    omega_facets = skeleton[O.facet_locate_entities(H, fdom, "phi<0")]
    facet_rules = O.facet_runtime_quadrature(mesh, H, phi, fdom, "phi<0", order)
    ghost = O.ghost_penalty_facets(mesh, dom, "phi<0")
    s2 = degree * degree
    a = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=vol, qdegree=2 * (degree - 1)),
         O.Integral(O.INTERIOR_FACET, O.K_SIP, entities=omega_facets, rules=facet_rules, params=(sigma * s2,),
                    qdegree=2 * degree),
         O.Integral(O.CELL, O.K_NITSCHE, rules=itf, point_data=normals, params=(sigma_gamma * s2,)),
         O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=ghost, params=(gamma_g,), qdegree=2 * (degree - 1))]
    L = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=vol, params=(O.F_POISSON_RHS, 1.0), qdegree=4),
         O.Integral(O.CELL, O.L_NITSCHE_RHS, rules=itf, point_data=normals, params=(sigma_gamma * s2, O.F_SINPROD, 1.0))]
    return dict(V=V, dofmap=dofmap, ndofs=ndofs, domain=dom, inside=inside, active=active, vol=vol, itf=itf,
                normals=normals, skeleton=skeleton, hosts=H, fdom=fdom, omega_facets=omega_facets,
                facet_rules=facet_rules, ghost=ghost, a=a, L=L)


def groups_expected() -> bool:
    """Whether the P1 series source term of a located list on a mesh of Kuhn hexes takes the hex-grouped kernel
    (`source_groups`).  The diagnostic modes that switch it, the row stencil, the row-ordered staging or the series
    kernel off, or send linear forms by cell block or through the entity-parallel atomics, take the per-cell path
    with the same results."""
    import os
    env = os.environ.get
    return not (env("CFX_SOURCE_GROUPS") == "0" or env("CFX_STENCIL") == "0" or env("CFX_VEC_BLOCKS") == "2"
                or env("CFX_VEC_ROWORDER") == "0" or env("CFX_SOURCE_SERIES") == "0" or env("CFX_ASSEMBLY") == "atomic")


def profiled(fn):
    """fn() with the engine's per-kernel profile on: (result, {kernel name: launches})."""
    import ctypes as C
    from cutfemx_amd import _lib
    l = _lib.lib()
    _lib.check(l.cfx_profile_enable(1))
    _lib.check(l.cfx_profile_reset())
    try:
        out = fn()
        names = {}
        for i in range(l.cfx_profile_count()):
            name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
            _lib.check(l.cfx_profile_get(i, C.byref(name), C.byref(ms), C.byref(cnt)))
            if cnt.value:
                names[name.value.decode()] = cnt.value
    finally:
        _lib.check(l.cfx_profile_enable(0))
    return out, names


