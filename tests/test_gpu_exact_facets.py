"""The HIP engine against the exact facet and interface terms of `exact_cut.py` (not against the oracle): the local
tensor of EVERY ghost facet, inside skeleton facet, cut skeleton facet rule and cut cell for the ghost penalty, the
value jump, the symmetric interior penalty and Nitsche; the assembled forms through every staging format of the facet
path; the Poisson and DG Poisson systems.

The oracle module only hands in mesh arrays (inputs); no assert reads an oracle value.  Per-entity tensors:
abs(got - exact) <= 1e-12 x the largest entry of the same term's exact tensor on the WHOLE facet (Nitsche: the interface
measure replaced by h^(tdim - 1)); assembled arrays: rel_err <= 1e-12.  Left out: `exact_cut.facet_case` /
`build_case` (selected from the inputs alone, at most 5 %, none for the regular level sets); every assembled case is a
regular level set.  Every group holds a scrambled case, where the two cells of a facet differ in diameter.

Kernel paths: the engine's profile files every stage-1 facet kernel (`assemble_facets_kernel` with `facet_local_row`,
`facet_jump_p1_kernel`, `facet_jumps_p2_kernel`) under the one name `assemble_facets`, so the staging formats
(`fold_facets` 0 / 1 / 2 / 3) are told apart by the switch and by the form alone (the comments of `prepare` in
cfx_gather.hip); `cut_tensors_p1` has a name of its own and is asserted in the default mode, `cut_tensors_p2` asserted absent with its
switch off.
Each test prints its worst value ("EXACT <group> ..."; run with -s to see them).
"""
import numpy as np
import pytest

import exact_cut as X
from helpers import profiled, rel_err
from test_gpu_exact_moments import _default_paths, _engine, _matrix_err, _space

pytestmark = pytest.mark.gpu
TOL = 1e-12
S3, G3 = "3d-n4-sphere-scrambled", "3d-n5-gyroid"
GAMMA = 40.0


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def _dg_space(cs, mesh, degree, bs=1):
    import cutfemx_amd as cfx
    dofmap, _ = cfx.lagrange_dofmap(cs["tdim"], cs["conn"], cs["x"].shape[0], degree)
    ndofs = cs["conn"].shape[0] * dofmap.shape[1]
    dofmap = np.arange(ndofs, dtype=np.int32).reshape(cs["conn"].shape[0], -1)
    return cfx.FunctionSpace(mesh, degree, dofmap=dofmap, ndofs=ndofs, bs=bs), dofmap, ndofs


def _coo(entries, n):
    import scipy.sparse as sp
    r, c, v = entries
    return sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()


def _skeleton(cs, fc, mesh, f, order):
    """All interior facets cut with the facets as hosts: (rows inside, rules of the cut ones), checked against the
    sets that `facet_case` takes from the inputs."""
    import cutfemx_amd as cfx
    rows = cfx.interior_facets_for_cells(mesh, np.arange(cs["conn"].shape[0], dtype=np.int32))
    assert np.array_equal(rows.rows, fc["rows"])
    cdf = cfx.cut(f, rows, cs["tdim"] - 1)
    inside = rows.rows[cfx.locate_entities(cdf, "phi<0")]
    assert np.array_equal(inside, fc["inside"])
    R = cfx.runtime_quadrature(cdf, "phi<0", order)
    assert {tuple(r) for r in R.host_rows.tolist()} <= {tuple(r) for r in fc["cut"].tolist()}
    return cdf, inside, R


def _ghost(cs, fc, cd):
    import cutfemx_amd as cfx
    g = cfx.ghost_penalty_facets(cd, "phi<0")
    assert sorted(map(tuple, g.rows.tolist())) == list(map(tuple, fc["ghost"].tolist()))
    return g


def test_the_cases_have_facets_of_both_kinds_and_cells_of_two_sizes(oracle):
    """From the inputs alone: every case has (cut, cut) and (cut, inside) ghost facets, at least 10 in all, at most
    5 % of its facets are left out (none for the regular level sets), and on H_CASE -- which is in every group below --
    the two cells of more than half of the ghost facets differ in diameter by more than 5 % of h_avg."""
    for name in X.FACET_CASES + [G3]:
        cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
        assert fc["n_cut_cut"] > 0 and fc["n_cut_inside"] > 0 and len(fc["ghost"]) >= 10, name
        for k in ("ghost_keep", "inside_keep", "cut_keep"):
            out = int((~fc[k]).sum())
            assert out <= 0.05 * fc[k].size and (cs["degenerate"] or out == 0), (name, k, out)
    h = X.facet_case(oracle, X.H_CASE)["h"]
    assert np.mean(np.abs(h[:, 0] - h[:, 1]) > 0.05 * h.mean(axis=1)) > 0.5
    for name in (X.H_CASE, S3, G3):
        cs = X.build_case(oracle, name)
        assert not cs["degenerate"] and cs["keep"].all() and cs["keep_itf"].all()


# ---- per entity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", X.FACET_CASES)
def test_facet_tensors_are_the_exact_ones(oracle, name, degree):
    """tabulate_entity (`facet_local_row`, whole facets and facet-hosted runtime rules) of every ghost facet, every
    inside skeleton facet and every cut skeleton facet rule: GHOST_GRADJUMP at e = 0 and e = 2 (degree 2: also
    bs = tdim), JUMP and SIP, on the per-cell (DG) dofmap."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    d = cs["tdim"]
    mesh, V1, fs, cd = _engine(cs)
    _ghost(cs, fc, cd)
    cdf, inside, R = _skeleton(cs, fc, mesh, fs[0], 2 * degree)
    whole = X.Moments(d - 1)
    cut_keep = {tuple(r) for r in fc["cut"][fc["cut_keep"]].tolist()}
    variants = [("ghost", fem.GHOST_GRADJUMP, (0.1, 0.0), 1), ("ghost", fem.GHOST_GRADJUMP, (0.1, 2.0), 1),
                ("jump", fem.JUMP, (0.3,), 1), ("sip", fem.SIP, (10.0,), 1)]
    if degree == 2:
        variants.append(("ghost", fem.GHOST_GRADJUMP, (0.1, 0.0), d))
    worst, n, n_cut = 0.0, 0, 0
    for kind, kernel, params, bs in variants:
        V, _, _ = _dg_space(cs, mesh, degree, bs)
        a = fem.form([fem.Integral(kernel, facets=fc["ghost"], params=params, qdegree=2 * degree),
                      fem.Integral(kernel, facets=inside, rules=R, params=params, qdegree=2 * degree)], V)
        todo = [(0, i, r, False) for i, r in enumerate(fc["ghost"]) if fc["ghost_keep"][i]]
        todo += [(1, i, r, False) for i, r in enumerate(inside) if fc["inside_keep"][i]]
        todo += [(1, len(inside) + i, r, True) for i, r in enumerate(R.host_rows) if tuple(r.tolist()) in cut_keep]
        for integral, idx, row, part in todo:
            fb = X.facet_basis(name, cs, row, degree)
            want = X.facet_tensor(kind, fb, X.facet_moments(name, cs, fb) if part else whole, params, bs).astype(np.float64)
            top = float(np.abs(X.facet_tensor(kind, fb, whole, params)).max())
            got = np.asarray(fem.tabulate_entity(a, integral, idx, False)).reshape(want.shape)
            worst = max(worst, np.abs(got - want).max() / top)
            n += 1
            n_cut += part
    _report("facet tensors", f"{name} P{degree} ({n} tensors, {n_cut} of cut facets)", worst)
    assert n_cut > 0 and 0.0 < worst <= TOL


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", X.FACET_CASES)
def test_nitsche_tensors_are_the_exact_ones(oracle, name, degree):
    """tabulate_entity(use_rule=True) of NITSCHE on every cut cell (a 3-D cell may have two rules: its tensor is their
    sum).  A kept cut cell without a rule is one whose piece of phi_h = 0 has no measure: its exact tensor is zero."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, _, _ = _space(cs, mesh, degree)
    R = cfx.runtime_quadrature(cd, "phi=0", 2 * degree)
    a = fem.form([fem.Integral(fem.NITSCHE, rules=R, point_data=cfx.normal(cd, R), params=(GAMMA,))], V)
    got = {}
    for idx, c in enumerate(R.parent_map):
        t = np.asarray(fem.tabulate_entity(a, 0, idx, True))
        got[int(c)] = got[int(c)] + t if int(c) in got else t
    kept = cs["cut"][cs["keep_itf"]].tolist()
    worst, n = 0.0, 0
    for c in kept:
        itf = X.interface(name, cs, c)
        want = X.nitsche(itf, degree, GAMMA).astype(np.float64)
        top = float(np.abs(X.nitsche(itf, degree, GAMMA, itf.whole)).max())
        if c not in got:
            assert itf.mom.m[tuple([0] * (cs["tdim"] + 1))] == 0 and np.abs(want).max() == 0
            continue
        worst = max(worst, np.abs(got[c].reshape(want.shape) - want).max() / top)
        n += 1
    _report("nitsche tensors", f"{name} P{degree} ({n} of {len(kept)} kept cut cells have a rule)", worst)
    assert (n == len(kept) or cs["degenerate"]) and 0.0 < worst <= TOL


# ---- assembled: the staging formats of the P1 ghost penalty -----------------------------------------------------------------
FOLD_MODES = {"default": {}, "fold-stage1-0": {"CFX_FACET_FOLD_STAGE1": "0"}, "fold-stage1-2": {"CFX_FACET_FOLD_STAGE1": "2"},
              "atomic": {"CFX_ASSEMBLY": "atomic"}}


@pytest.mark.parametrize("mode", list(FOLD_MODES))
@pytest.mark.parametrize("second", [False, True], ids=["ghost", "ghost+facet-rules"])
@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_assembled_p1_ghost_penalty_is_exact(oracle, monkeypatch, name, second, mode):
    """P1 ghost penalty + stiffness over [inside cells, rules].  Default: rank-one records, 10 doubles per facet
    (`facet_jump_p1_kernel`, fold_facets = 3).  CFX_FACET_FOLD_STAGE1=2: no records -- the 25-double folded tensor in
    3-D (2), the fold inside the gather in 2-D (1); =0: the full macro tensor, folded in the gather.
    CFX_ASSEMBLY=atomic: the entity-parallel kernel.  `second`: a second facet integral, the gradient jump over
    [facets inside, rules of the cut skeleton facets], makes the form's facet part not rank one in every mode and
    sends facet-hosted rules through the same staging."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    for k, v in FOLD_MODES[mode].items():
        monkeypatch.setenv(k, v)
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, V, fs, cd = _engine(cs)
    nn = cs["x"].shape[0]
    ghost = _ghost(cs, fc, cd)
    inside = cfx.locate_entities(cd, "phi<0")
    assert np.array_equal(inside, cs["inside"])
    vol = cfx.runtime_quadrature(cd, "phi<0", 2)
    ints = [fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=0),
            fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(0.1,), qdegree=0)]
    M = _coo(X.exact_entries(name, cs, cs["conn"], 1, "stiffness", 1, (), cs["inside"]), nn) + \
        _coo(X.exact_facet_entries(name, cs, cs["conn"], 1, "ghost", 1, (0.1, 0.0), fc["ghost"]), nn)
    if second:
        cdf, rows_in, Rf = _skeleton(cs, fc, mesh, fs[0], 2)
        ints.append(fem.Integral(fem.GHOST_GRADJUMP, facets=rows_in, rules=Rf, params=(0.7, 2.0), qdegree=0))
        M = M + _coo(X.exact_facet_entries(name, cs, cs["conn"], 1, "ghost", 1, (0.7, 2.0), fc["inside"], fc["cut"]), nn)
    A, names = profiled(lambda: fem.assemble_matrix(fem.form(ints, V)))
    assert "assemble_facets" in names, sorted(names)
    if mode == "atomic":
        assert not any(k.startswith("assemble_rows") for k in names), sorted(names)
    elif _default_paths():
        assert any(k.startswith("assemble_rows") or k.startswith("assemble_tiles") for k in names), sorted(names)
    err = _matrix_err(A, M)
    _report("assembled facets", f"{name} P1 {'ghost+facet-rules' if second else 'ghost'} {mode} {sorted(names)}", err)
    assert err <= TOL


# ---- assembled: P2 scalar ghost penalty, records and fallback ------------------------------------------------------------------
# points of the facet rule by quadrature degree: lines have at most 5 (every degree takes records), triangles 1, 3, 6 and
# then 7 at degree 5, the first beyond the records' `nq <= 6`
P2_Q = {2: {1: 1, 4: 3, 8: 5}, 3: {1: 1, 2: 3, 3: 6, 5: 7}}


@pytest.mark.parametrize("mode", ["default", "split"])
@pytest.mark.parametrize("name", [X.H_CASE, S3, G3])
def test_assembled_p2_ghost_penalty_is_exact(oracle, monkeypatch, name, mode):
    """Scalar P2 ghost penalty, alone and next to stiffness over [inside cells, rules], at facet quadrature degrees
    with nq = 1, 3, 6 points (`facet_jumps_p2_kernel`: 8 + 16 nq doubles per facet) and at the first degree with 7
    (staged macro tensors), also under CFX_ROWS_SPLIT=1, where `assemble_rows_cut` takes the facet rows.  The
    integrand has degree 2: every rule of degree >= 2 gives the integral, the one-point rule of degree 1 the
    integrand at the centroid times the measure."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "split":
        monkeypatch.setenv("CFX_ROWS_SPLIT", "1")
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    d = cs["tdim"]
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, 2)
    ghost = _ghost(cs, fc, cd)
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 4)
    K = _coo(X.exact_entries(name, cs, dofmap, 1, "stiffness", 2, (), cs["inside"]), ndofs)
    cdf = cfx.cut(fs[0], cfx.interior_facets_for_cells(mesh, np.arange(cs["conn"].shape[0], dtype=np.int32)), d - 1)
    worst = 0.0
    for q, nq in P2_Q[d].items():
        off = cfx.full_facet_rules(cdf, None, q).offsets
        assert np.all(np.diff(off) == nq), (q, nq)
        G = _coo(X.exact_facet_entries(name, cs, dofmap, 1, "ghost", 2, (0.1, 0.0), fc["ghost"], one_point=q == 1), ndofs)
        gp = fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(0.1,), qdegree=q)
        A, names = profiled(lambda: fem.assemble_matrix(fem.form([gp], V)))
        assert "assemble_facets" in names, sorted(names)
        e1 = _matrix_err(A, G)
        st = fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=2)
        A2, names2 = profiled(lambda: fem.assemble_matrix(fem.form([st, gp], V)))
        print("PATHS p2-ghost", name, mode, q, sorted(names), sorted(names2))
        e2 = _matrix_err(A2, K + G)
        _report("assembled facets", f"{name} P2 ghost q={q} nq={nq} {mode}: alone {e1:.3e} with stiffness", e2)
        worst = max(worst, e1, e2)
        assert e1 <= TOL and e2 <= TOL, (q, e1, e2)
    assert worst > 0.0


# ---- assembled: vector ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "no-block-gather"])
@pytest.mark.parametrize("name", [G3, S3])
def test_assembled_p2_vector_ghost_penalty_and_elasticity_are_exact(oracle, monkeypatch, name, mode):
    """P2-vector (bs = 3) ghost penalty next to elasticity over [inside cells, rules]: the block gather and
    CFX_BLOCK_GATHER=0."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "no-block-gather":
        monkeypatch.setenv("CFX_BLOCK_GATHER", "0")
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, 2, 3)
    ghost = _ghost(cs, fc, cd)
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 2)
    params = (1.0e3, 0.3)
    # the penalty weighted so that its entries are of the elasticity term's size (E h^-2 x h^2)
    gg = (50.0, 0.0)
    a = fem.form([fem.Integral(fem.ELASTICITY, cells=inside, rules=vol, params=params, qdegree=2),
                  fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=gg, qdegree=2)], V)
    E = _coo(X.exact_entries(name, cs, dofmap, 3, "elasticity", 2, params, cs["inside"]), 3 * ndofs)
    G = _coo(X.exact_facet_entries(name, cs, dofmap, 3, "ghost", 2, gg, fc["ghost"]), 3 * ndofs)
    assert 0.01 < abs(G).max() / abs(E).max() < 100
    A, names = profiled(lambda: fem.assemble_matrix(a))
    assert "assemble_facets" in names, sorted(names)
    err = _matrix_err(A, E + G)
    Ag = fem.assemble_matrix(fem.form([fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=gg, qdegree=2)], V))
    eg = _matrix_err(Ag, G)
    _report("assembled facets", f"{name} P2-vector elasticity + ghost {mode} {sorted(names)}: ghost alone {eg:.3e} both", err)
    assert err <= TOL and eg <= TOL


# ---- assembled: Nitsche -----------------------------------------------------------------------------------------------------
NITSCHE_MODES = {"default": {}, "no-cut-tensors-p1": {"CFX_CUT_TENSORS_P1": "0"}, "no-p2-cut-tensors": {"CFX_P2_CUT_TENSORS": "0"},
                 "no-vec-blocks": {"CFX_VEC_BLOCKS": "0"}, "atomic": {"CFX_ASSEMBLY": "atomic"},
                 "split": {"CFX_ROWS_SPLIT": "1"}}


@pytest.mark.parametrize("mode", list(NITSCHE_MODES))
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_assembled_nitsche_matrix_and_vector_are_exact(oracle, monkeypatch, name, degree, mode):
    """The Nitsche matrix next to stiffness over [inside cells, rules] (`cut_tensors_p1`; degree 2 under
    CFX_ROWS_SPLIT=1 in 3-D: `cut_tensors_p2`, one combined tensor per cut cell with Nitsche folded in) and the g = 1
    Nitsche vector (the vector kernels, CFX_VEC_BLOCKS=0: without the cell blocks), each with its switch off and
    through the entity-parallel atomics."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    default = _default_paths()
    for k, v in NITSCHE_MODES[mode].items():
        monkeypatch.setenv(k, v)
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, degree)
    inside = cfx.locate_entities(cd, "phi<0")
    vol, itf = cfx.runtime_quadrature(cd, "phi<0", 4), cfx.runtime_quadrature(cd, "phi=0", 4)
    nrm = cfx.normal(cd, itf)
    a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=2 * (degree - 1)),
                  fem.Integral(fem.NITSCHE, rules=itf, point_data=nrm, params=(GAMMA,))], V)
    N = _coo(X.exact_nitsche_entries(name, cs, dofmap, degree, GAMMA), ndofs)
    M = _coo(X.exact_entries(name, cs, dofmap, 1, "stiffness", degree, (), cs["inside"]), ndofs) + N
    A, names = profiled(lambda: fem.assemble_matrix(a))
    if default and degree == 1 and mode == "default":
        assert "cut_tensors_p1" in names, sorted(names)
    if degree == 1 and mode == "no-cut-tensors-p1":
        assert "cut_tensors_p1" not in names, sorted(names)
    if degree == 2 and mode == "no-p2-cut-tensors":
        assert "cut_tensors_p2" not in names, sorted(names)
    ea = _matrix_err(A, M)
    en = _matrix_err(fem.assemble_matrix(fem.form([fem.Integral(fem.NITSCHE, rules=itf, point_data=nrm, params=(GAMMA,))], V)), N)
    L = fem.form([fem.Integral(fem.NITSCHE_RHS, rules=itf, point_data=nrm, params=(GAMMA, fem.F_ONE, 1.0))], V)
    want = np.zeros(ndofs)
    np.add.at(want, *X.exact_nitsche_entries(name, cs, dofmap, degree, GAMMA, 1.0))
    eb = rel_err(fem.assemble_vector(L), want)
    _report("assembled nitsche", f"{name} P{degree} {mode} {sorted(names)}: with stiffness {ea:.3e} alone {en:.3e} vector", eb)
    assert ea <= TOL and en <= TOL and 0.0 < eb <= TOL


# ---- systems ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_poisson_system_is_the_sum_of_the_exact_terms(oracle, name, degree):
    """The matrix of poisson.build_forms: stiffness + Nitsche + ghost penalty."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, degree)
    g = poisson.build_forms(V, cd)
    assert sorted(map(tuple, g.ghost_facets.rows.tolist())) == list(map(tuple, fc["ghost"].tolist()))
    M = _coo(X.exact_entries(name, cs, dofmap, 1, "stiffness", degree, (), cs["inside"]), ndofs) + \
        _coo(X.exact_nitsche_entries(name, cs, dofmap, degree, 40.0), ndofs) + \
        _coo(X.exact_facet_entries(name, cs, dofmap, 1, "ghost", degree, (0.1, 0.0), fc["ghost"]), ndofs)
    A, names = profiled(lambda: cfx.fem.assemble_matrix(g.a))
    assert "assemble_facets" in names, sorted(names)
    err = _matrix_err(A, M)
    _report("systems", f"{name} P{degree} Poisson {sorted(names)}", err)
    assert 0.0 < err <= TOL


@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_dg_poisson_system_is_the_sum_of_the_exact_terms(oracle, name):
    """The matrix of poisson.build_dg_forms at degree 1: stiffness + SIP over [facets inside, rules of the cut ones] +
    Nitsche + ghost penalty on the per-cell dofmap."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    g = poisson.build_dg_forms(fs[0], 1)
    assert np.array_equal(g.omega_facets, fc["inside"])
    nd = cs["tdim"] + 1
    ndofs = cs["conn"].shape[0] * nd
    dofmap = np.arange(ndofs, dtype=np.int32).reshape(-1, nd)
    M = _coo(X.exact_entries(name, cs, dofmap, 1, "stiffness", 1, (), cs["inside"]), ndofs) + \
        _coo(X.exact_facet_entries(name, cs, dofmap, 1, "sip", 1, (10.0,), fc["inside"], fc["cut"]), ndofs) + \
        _coo(X.exact_nitsche_entries(name, cs, dofmap, 1, 20.0), ndofs) + \
        _coo(X.exact_facet_entries(name, cs, dofmap, 1, "ghost", 1, (0.1, 0.0), fc["ghost"]), ndofs)
    A, names = profiled(lambda: cfx.fem.assemble_matrix(g.a))
    assert "assemble_facets" in names and "assemble_facets_cut" in names, sorted(names)
    err = _matrix_err(A, M)
    _report("systems", f"{name} DG P1 Poisson {sorted(names)}", err)
    assert 0.0 < err <= TOL
