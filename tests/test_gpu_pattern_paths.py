"""Characterisation of the sparsity build (cfx_rowasm.hip: cfx::build_pattern and its phases): one fem.create_matrix per
case, on the smallest shapes of the suite that reach each path of the build -- the P1 stencil path with its deferred
read-back, the restart on the wide path, the short / long split of the neighbour lists, the 2048-slot sets, the copied
rows of vector spaces, the rows reused from the previous pattern, a rectangular block.  Each case asserts

  * indptr and indices equal to the oracle's, bit for bit,
  * the complete {launch name: launches} table of the call (helpers.profiled), the plan and the mesh-static tables
    that the call builds on its way included,
  * the host read-backs of the call (_lib.sync_count()).

The tables in EXPECTED were recorded by running these very cases on the commit BEFORE the build was split into its
phases (05131cb); the file passes unchanged on that commit and on the split one, which is what it is for: a change of
the host driver that adds, drops or renames a launch or a read-back shows here.  A table changes only together with a
deliberate change of the launches, never to make a refactoring pass.  One name is left out of the comparison, `fill`:
cfx::dev_fill launches its kernel for a 16-byte aligned pointer and takes hipMemsetAsync otherwise, and the 4-byte
flags it clears come from a pool -- how many of a call's flags are aligned depends on the flags that earlier calls
of the process took (recorded twice in different orders of the cases: `fill` moved by up to 3, nothing else moved).

When the whole run carries a switch of its own (tools/test_modes.sh) the tables of the default configuration do not
hold: the patterns are still compared, as tests/test_gpu_high_valence.py does.

Two cases of the issue's list do not reach the path it names them for and stay as what they are: the 6^3 box of the
degree-2 space and the 5^3 box of the vector space have no plain row (every vertex is next to the interface or
outside), so both take the purely hashed path, narrow then wide.  The short / long split with long rows, full_rows +
odd_rows, and full_rows (split) + rest_rows are reached on the high-valence cones of tests/test_gpu_high_valence.py
instead ("p2-cone-4", "p2-cone-4-stiffness", "vector-p2-bs3-cone-3").  "p1-cone-6x8" (apex stencil 64) has no row
stencil at all and goes narrow -> wide with a read-back; the restart of the stencil path itself -- a stencil of 63 and
a Poisson row of 64, found by the deferred read-back -- is "p1-cone-1x30".

The `lists_short_overflow` fallback (a split build whose short or wide sets overflow: all rows wide from then on) is
reached by "p2-cone-9": its static lists exist (the apex list has 462 entries) and the apex's Poisson row has 563
columns, so the split's 512-slot set overflows, the build falls back to the wide sets and from there to the 2048-slot
ones -- the table holds pattern_split and pattern_rows_short next to pattern_rows_huge.  (m = 9 is not among the
shapes of test_gpu_high_valence.py: on m = 10 the apex's static list itself, 563 entries, is beyond the 511 of the
lists, the space has none and the build is purely hashed.)

"p2-cone-10-second" is a second pattern of the space that "p2-cone-10" leaves behind (`huge_rows` set): it builds the
2048-slot sets at once, pattern_rows_huge without pattern_rows_wide.  The case switches CFX_PATTERN_REUSE off for
itself: on the same cut every hashed row would be clean, copy its columns from the first pattern, and no hash set
would be built at all.

One branch has no case: the short / long sets built again in place (pattern_rows_short_write and, after a split,
pattern_rows_wide_write), taken when the staging rows of a split build -- 128 or 512 columns per hashed row -- need
more than half of the card's free memory.  No mesh that a test can afford gets there, and the engine has no switch
for it."""
import os

import numpy as np
import pytest

from helpers import high_valence_case, level_set_values, oracle_poisson, oracle_stiffness_source, profiled

pytestmark = pytest.mark.gpu

_REFS = {}


def _foreign_switches():
    """Switches of the whole run.  (CFX_LIB names another build of the engine, which is how the tables are checked
    against the parent commit's library: no switch.)"""
    return [k for k in os.environ
            if k.startswith("CFX_") and k not in ("CFX_STEP_DEBUG", "CFX_COUNT_SYNC", "CFX_DEVICE", "CFX_LIB")]


def _once(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _poisson_box(O, tdim, n, degree):
    """Poisson + Nitsche + ghost penalty on the n^tdim box, sphere level set: (call, indptr, indices)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson

    def make():
        om = O.mesh_box(tdim, n)
        phi = level_set_values(om.x, tdim)
        kw = {}
        if degree == 2:
            dofmap, ndofs = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
            kw = dict(degree=2, dofmap=dofmap, ndofs=ndofs)
        ref = oracle_poisson(O, om, phi, **kw)
        return om, phi, kw, ref["indptr"], ref["indices"]
    om, phi, kw, ip, ix = _once(("box", tdim, n, degree), make)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V1 = cfx.FunctionSpace(mesh, 1)
    V = V1 if degree == 1 else cfx.FunctionSpace(mesh, 2, dofmap=kw["dofmap"], ndofs=kw["ndofs"])
    cd = cfx.cut(cfx.Function(V1, phi))
    s = poisson.build_forms(V, cd, order=4)
    return (lambda: fem.create_matrix(s.a)), ip, ix, (s, cd)


def _poisson_cone(O, shape, degree, second=None):
    """The Poisson system on helpers.high_valence_case(3, shape).  `second` (the monkeypatch): the space has built one
    pattern already, and this one hashes its rows again (CFX_PATTERN_REUSE=0: on the same cut every row would copy
    its columns from the first pattern and no hash set would be built)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson

    def make():
        om, phi, _info = high_valence_case(O, 3, shape)
        kw = {}
        if degree == 2:
            dofmap, ndofs = cfx.lagrange_dofmap(3, om.conn, om.nnodes, 2)
            kw = dict(degree=2, dofmap=dofmap, ndofs=ndofs)
        ref = oracle_poisson(O, om, phi, **kw)
        return om, phi, kw, ref["indptr"], ref["indices"]
    om, phi, kw, ip, ix = _once(("cone", shape, degree), make)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V1 = cfx.FunctionSpace(mesh, 1)
    V = V1 if degree == 1 else cfx.FunctionSpace(mesh, 2, dofmap=kw["dofmap"], ndofs=kw["ndofs"])
    cd = cfx.cut(cfx.Function(V1, phi))
    keep = [cd]
    if second:
        second.setenv("CFX_PATTERN_REUSE", "0")
        s0 = poisson.build_forms(V, cd, order=4)
        A0 = fem.create_matrix(s0.a)
        assert np.array_equal(A0.indices, ix)
        keep += [s0, A0]
    s = poisson.build_forms(V, cd, order=4)
    return (lambda: fem.create_matrix(s.a)), ip, ix, (s, keep)


def _stiffness_cone(O, shape):
    """Degree 2, the stiffness over the inside cells alone (test_gpu_high_valence's form (b)): every active row is a
    plain row, and the one integral is the closed-form stiffness."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem

    def make():
        om, phi, _info = high_valence_case(O, 3, shape)
        dofmap, ndofs = cfx.lagrange_dofmap(3, om.conn, om.nnodes, 2)
        ref = oracle_stiffness_source(O, om, phi, degree=2, dofmap=dofmap, ndofs=ndofs)
        return om, phi, dofmap, ndofs, ref["indptr"], ref["indices"]
    om, phi, dofmap, ndofs, ip, ix = _once(("cone-stiffness", shape), make)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 2, dofmap=dofmap, ndofs=ndofs)
    cd = cfx.cut(cfx.Function(cfx.FunctionSpace(mesh, 1), phi))
    inside = cfx.locate_entities_device(cd, "phi<0")
    a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, qdegree=2)], V)
    return (lambda: fem.create_matrix(a)), ip, ix, (cd, inside, a)


def _elasticity(O, tdim, n, degree, bs, cone=None):
    """Elasticity + ghost penalty on a vector space (test_gpu_spaces.elasticity_problem), on the n^tdim box or on
    helpers.high_valence_case(3, cone)."""
    import cutfemx_amd as cfx
    from test_gpu_spaces import elasticity_problem, setup
    mesh_phi = None if cone is None else _once(("cone-mesh", cone), lambda: high_valence_case(O, 3, cone)[:2])
    s = setup(O, tdim, n, degree, bs, mesh_phi=mesh_phi)
    _inside, oa, ga = elasticity_problem(s, degree)
    ip, ix = _once(("elasticity", tdim, n, degree, bs, cone), lambda: O.create_sparsity(s["om"], s["oV"], oa))
    a = cfx.fem.form(ga, s["V"])
    return (lambda: cfx.fem.create_matrix(a)), ip, ix, (s, a)


def _reuse(O, monkeypatch):
    """Second step of test_gpu_spaces' moving level set on the 14^2 box, degree 2: the rows around unchanged cells copy
    their columns from the first step's pattern."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    monkeypatch.setenv("CFX_PATTERN_REUSE", "1")
    tdim, n = 2, 14
    om = O.mesh_box(tdim, n)
    dofmap, ndofs = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 2, dofmap=dofmap, ndofs=ndofs)
    Vphi = cfx.FunctionSpace(mesh, 1)
    keep = []

    def step(k):
        phi = np.linalg.norm(om.x[:, :tdim] - np.array([0.40 + 0.013 * k, 0.45]), axis=1) - 0.27
        cd = cfx.cut(cfx.Function(Vphi, phi))
        inside = cfx.locate_entities(cd, "phi<0")
        vol = cfx.runtime_quadrature(cd, "phi<0", 2)
        ghost = cfx.ghost_penalty_facets(cd, "phi<0")
        a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=2),
                      fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(0.1,), qdegree=2)], V)
        keep.extend([cd, inside, vol, ghost, a])
        return a, phi
    a0, _phi = step(0)
    A0 = fem.create_matrix(a0)
    assert A0.reuse_stats[1] == 0
    keep.append(A0)
    a1, phi1 = step(1)

    def make():
        dom = O.classify(om.conn, phi1)
        o_ints = [O.Integral(O.CELL, O.K_STIFFNESS, entities=O.locate_entities(dom, "phi<0"),
                             rules=O.runtime_quadrature(om, om.conn, phi1, dom, "phi<0", 2), qdegree=2),
                  O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=O.ghost_penalty_facets(om, dom, "phi<0"),
                             params=(0.1,), qdegree=2)]
        return O.create_sparsity(om, O.Space(dofmap, ndofs, 2, 1), o_ints)
    ip, ix = _once("reuse", make)

    def call():
        A = fem.create_matrix(a1)
        hashed, reused = A.reuse_stats
        assert 0 < reused < hashed, (hashed, reused)
        return A
    return call, ip, ix, keep


def _rectangular(O):
    """B^T = -(div v, p), P2 vector x P1, of test_rectangular_forms.test_gpu_stokes_blocks_on_a_cut_domain (2-D, n = 8)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    from test_rectangular_forms import spaces
    tdim, n = 2, 8
    om, dm2, nd2, oVU, oVP, _oVS = spaces(O, tdim, n)
    phi = level_set_values(om.x, tdim)

    def make():
        dom = O.classify(om.conn, phi)
        oa = [O.Integral(O.CELL, O.K_DIV_TEST, entities=O.locate_entities(dom, "phi<0"),
                         rules=O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 4), params=(-1.0,), qdegree=3)]
        return O.create_sparsity2(om, oVU, oVP, oa)
    ip, ix = _once("rectangular", make)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    VU = cfx.FunctionSpace(mesh, 2, dofmap=dm2, ndofs=nd2, bs=tdim)
    VP = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(VP, phi))
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 4)
    a = fem.form([fem.Integral(fem.DIV_TEST, cells=inside, rules=vol, params=(-1.0,), qdegree=3)], VU, trial_space=VP)
    return (lambda: fem.create_matrix(a)), ip, ix, (cd, inside, vol, a)


CASES = {
    "p1-box-3d-6": lambda O, mp: _poisson_box(O, 3, 6, 1),                # P1 stencil, deferred read-back
    "p1-cone-6x8": lambda O, mp: _poisson_cone(O, (6, 8), 1),             # apex stencil 64: no stencil, narrow -> wide
    "p1-cone-1x30": lambda O, mp: _poisson_cone(O, (1, 30), 1),           # apex stencil 63, row 64: the deferred restart
    "p2-box-2d-12": lambda O, mp: _poisson_box(O, 2, 12, 2),              # neighbour lists, short / long split
    "p2-box-3d-6": lambda O, mp: _poisson_box(O, 3, 6, 2),
    "p2-cone-4": lambda O, mp: _poisson_cone(O, (4, 4), 2),               # lists of 107: short / long split with long rows
    "p2-cone-4-stiffness": lambda O, mp: _stiffness_cone(O, (4, 4)),      # one closed-form integral: full_rows + odd_rows
    "vector-p2-bs3-cone-3": lambda O, mp: _elasticity(O, 3, None, 2, 3, cone=(3, 3)),   # full_rows (split) / rest_rows
    "p2-cone-9": lambda O, mp: _poisson_cone(O, (9, 9), 2),               # lists + a row of 563: lists_short_overflow
    "p2-cone-10": lambda O, mp: _poisson_cone(O, (10, 10), 2),            # huge rows (685 / static 563)
    "p2-cone-10-second": lambda O, mp: _poisson_cone(O, (10, 10), 2, second=mp),   # reuse off: starts at huge_rows
    "vector-p2-bs3-3d-5": lambda O, mp: _elasticity(O, 3, 5, 2, 3),       # no plain row: purely hashed (docstring)
    "vector-p1-bs2-2d-12": lambda O, mp: _elasticity(O, 2, 12, 1, 2),
    "reuse-p2-2d-14": lambda O, mp: _reuse(O, mp),                        # dirty / clean rows
    "rectangular-Bt-2d-8": lambda O, mp: _rectangular(O),
}

# case: ({launch name: launches}, read-backs) of the one create_matrix call, recorded on the parent commit (docstring)
EXPECTED = {
    "p1-box-3d-6":
        ({"count_gather": 1, "facet_dof_count": 1, "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_rows": 1,
          "pattern_write": 1, "plan_bulk_init": 1, "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rules": 1,
          "scan_top": 5, "stencil_rows": 1, "stencil_rows_write": 1, "stencil_slots": 1}, 7),
    "p1-cone-6x8":
        ({"count_gather": 1, "facet_dof_count": 1, "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_long_rows": 4,
          "pattern_map_rows": 2, "pattern_reuse": 2, "pattern_rows": 1, "pattern_rows_wide": 1,
          "pattern_rows_wide_write": 1, "pattern_short_rows": 2, "plan_mark_entities": 1, "plan_pack_bits": 1,
          "plan_row_lists": 2, "plan_rules": 1, "scan_top": 7, "stencil_rows": 1}, 9),
    "p1-cone-1x30":
        ({"count_gather": 3, "facet_dof_count": 1, "facet_dof_fill": 1, "lattice_rows": 4, "pattern_indptr": 3,
          "pattern_plain": 1, "pattern_plain_write": 1, "pattern_rows": 1, "pattern_rows_wide": 1,
          "pattern_rows_wide_write": 1, "plan_bulk_init": 1, "plan_mix_rows": 1, "plan_plain_masks": 1,
          "plan_plain_tiles": 2, "plan_row_lists": 2, "plan_rules": 1, "scan_top": 8, "stencil_rows": 1,
          "stencil_rows_write": 1, "stencil_slots": 1, "stencil_tiles": 1, "stencil_tiles_write": 1}, 11),
    "p2-box-2d-12":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_plain_full": 3, "pattern_plain_write": 1,
          "pattern_reuse": 2, "pattern_rows_short": 1, "pattern_split": 3, "pattern_write": 1, "plan_bulk_init": 1,
          "plan_check_fold": 1, "plan_check_sorted": 2, "plan_mark_cells": 2, "plan_mark_rows": 4,
          "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rule_hash": 2, "scan_top": 8, "space_dof_verts": 1,
          "stencil_rows": 1, "stencil_rows_write": 1}, 9),
    "p2-box-3d-6":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_long_rows": 4, "pattern_map_rows": 2,
          "pattern_reuse": 2, "pattern_rows": 1, "pattern_rows_wide": 1, "pattern_rows_wide_write": 1,
          "pattern_short_rows": 2, "plan_bulk_init": 1, "plan_check_fold": 1, "plan_check_sorted": 2,
          "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rule_hash": 2,
          "scan_chained": 2, "scan_top": 7, "space_dof_verts": 1, "stencil_rows": 1, "stencil_rows_write": 1}, 11),
    "p2-cone-4":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_full_rows": 3, "pattern_indptr": 2, "pattern_long_rows": 4,
          "pattern_map_rows": 3, "pattern_plain_full": 3, "pattern_plain_write": 1, "pattern_reuse": 2,
          "pattern_rows_short": 1, "pattern_rows_wide": 1, "pattern_short_rows": 2, "pattern_split": 6,
          "pattern_write": 2, "plan_bulk_init": 1, "plan_check_fold": 1, "plan_check_sorted": 2,
          "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rule_hash": 2,
          "scan_top": 13, "space_dof_verts": 1, "stencil_rows": 1, "stencil_rows_write": 1,
          "stencil_slotn": 1}, 14),
    "p2-cone-4-stiffness":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "pattern_full_rows": 3,
          "pattern_indptr": 2, "pattern_long_rows": 4, "pattern_map_rows": 1, "pattern_plain_full": 4,
          "pattern_plain_write": 1, "pattern_reuse": 1, "pattern_rows_short": 1, "pattern_rows_wide": 1,
          "pattern_short_rows": 2, "pattern_split": 6, "pattern_write": 2, "plan_bulk_init": 1, "plan_mix_rows": 1,
          "plan_row_lists": 2, "scan_top": 12, "space_dof_verts": 1, "stencil_rows": 1, "stencil_rows_write": 1,
          "stencil_slotn": 1}, 14),
    "vector-p2-bs3-cone-3":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_full_rows": 9, "pattern_indptr": 2, "pattern_plain_full": 3,
          "pattern_plain_write": 1, "pattern_reuse": 2, "pattern_rows_short": 1, "pattern_rows_wide": 1,
          "pattern_split": 6, "pattern_write": 2, "plan_check_fold": 1, "plan_check_sorted": 2,
          "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_pack_bits": 1, "plan_row_lists": 2, "plan_rule_hash": 1,
          "scan_top": 12, "stencil_rows": 1, "stencil_rows_write": 1, "stencil_slotn": 1}, 13),
    "p2-cone-9":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_long_rows": 4, "pattern_map_rows": 3,
          "pattern_plain_full": 3, "pattern_plain_write": 1, "pattern_reuse": 2, "pattern_rows_huge": 1,
          "pattern_rows_huge_write": 1, "pattern_rows_short": 1, "pattern_rows_wide": 2, "pattern_short_rows": 2,
          "pattern_split": 6, "plan_bulk_init": 1, "plan_check_fold": 1, "plan_check_sorted": 2,
          "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rule_hash": 2,
          "scan_top": 12, "space_dof_verts": 1, "stencil_rows": 1, "stencil_rows_write": 1}, 15),
    "p2-cone-10":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_long_rows": 4, "pattern_map_rows": 3,
          "pattern_reuse": 2, "pattern_rows": 1, "pattern_rows_huge": 1, "pattern_rows_huge_write": 1,
          "pattern_rows_wide": 1, "pattern_short_rows": 2, "plan_bulk_init": 1, "plan_check_fold": 1,
          "plan_check_sorted": 2, "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_mix_rows": 1,
          "plan_row_lists": 2, "plan_rule_hash": 2, "scan_top": 8, "space_dof_verts": 1, "stencil_rows": 1}, 10),
    "p2-cone-10-second":
        ({"count_gather": 1, "facet_dof_count": 1, "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_long_rows": 4,
          "pattern_map_rows": 3, "pattern_rows_huge": 1, "pattern_rows_huge_write": 1, "pattern_short_rows": 2,
          "plan_bulk_init": 1, "plan_check_fold": 1, "plan_check_sorted": 2, "plan_mark_cells": 2, "plan_mark_rows": 4,
          "plan_mix_rows": 1, "plan_row_lists": 2, "plan_rule_hash": 2, "scan_top": 7}, 7),
    "vector-p2-bs3-3d-5":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "count_gather": 1, "facet_dof_count": 1,
          "facet_dof_fill": 1, "pattern_indptr": 2, "pattern_reuse": 2, "pattern_rows": 1, "pattern_rows_wide": 1,
          "pattern_rows_wide_write": 1, "plan_check_fold": 1, "plan_check_sorted": 2, "plan_mark_cells": 2,
          "plan_mark_rows": 4, "plan_pack_bits": 1, "plan_row_lists": 2, "plan_rule_hash": 1, "scan_top": 6,
          "stencil_rows": 1, "stencil_rows_write": 1}, 8),
    "vector-p1-bs2-2d-12":
        ({"count_gather": 1, "facet_dof_count": 1, "facet_dof_fill": 1, "pattern_indptr": 2,
          "pattern_plain_full": 3, "pattern_plain_write": 1, "pattern_reuse": 2, "pattern_rows_short": 1,
          "pattern_split": 3, "pattern_write": 1, "plan_mark_entities": 1, "plan_pack_bits": 1, "plan_row_lists": 2,
          "plan_rules": 1, "scan_top": 7, "stencil_rows": 1, "stencil_rows_write": 1}, 9),
    "reuse-p2-2d-14":
        ({"count_gather": 1, "facet_dof_count": 1, "facet_dof_fill": 1, "pattern_indptr": 2,
          "pattern_plain_full": 3, "pattern_plain_write": 1, "pattern_reuse": 10, "pattern_rows_short": 1,
          "pattern_split": 3, "pattern_write": 1, "plan_check_fold": 1, "plan_check_sorted": 2,
          "plan_mark_cells": 2, "plan_mark_rows": 4, "plan_pack_bits": 1, "plan_row_lists": 2, "plan_rule_hash": 1,
          "scan_top": 8}, 9),
    "rectangular-Bt-2d-8":
        ({"adj_count": 1, "adj_fill": 1, "adj_sort": 1, "pattern2_mark": 2, "pattern2_rows": 1,
          "pattern2_rows_write": 1, "scan_top": 2}, 3),
}


def measure(O, case, monkeypatch):
    """(matrix, oracle indptr, oracle indices, launch table, read-backs, foreign switches) of a case's create_matrix."""
    from cutfemx_amd import _lib
    foreign = _foreign_switches()
    call, ip, ix, _keep = CASES[case](O, monkeypatch)
    syncs = {}

    def counted():
        s0 = _lib.sync_count()
        A = call()
        syncs["n"] = _lib.sync_count() - s0
        return A
    A, names = profiled(counted)
    return A, ip, ix, names, syncs["n"], foreign


@pytest.mark.parametrize("case", list(CASES))
def test_pattern_path(oracle, case, monkeypatch):
    A, ip, ix, names, syncs, foreign = measure(oracle, case, monkeypatch)
    print(f"{case}: nnz {A.nnz} read-backs {syncs} {dict(sorted(names.items()))}")
    assert A.indptr.dtype == np.int64 and np.array_equal(A.indptr, ip), case
    assert A.indices.dtype == np.int32 and np.array_equal(A.indices, ix), case
    if foreign:
        return
    want_names, want_syncs = EXPECTED[case]
    names.pop("fill", None)                           # (docstring)
    assert names == want_names, (case, sorted(set(names.items()) ^ set(want_names.items())))
    assert syncs == want_syncs, case
