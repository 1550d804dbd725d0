"""The HIP engine against the exact values of `exact_cut.py` (not against the oracle) for the families that oracle
parity alone pinned before: rectangular blocks (`cfx_form_create2`: DIV_TEST, DIV_TRIAL, MASS and STIFFNESS between P2
and P1), kappa-weighted MASS / STIFFNESS / ELASTICITY, coefficient sources (scalar and vector-valued), Dirichlet
lifting and `set_bc`, and the interior-facet terms between two scalar spaces.  Each family per entity
(`fem.tabulate_entity` of every kept cut cell's rule / every kept ghost facet and of one in ten inside cells) and
assembled over [inside cells, phi<0 rules], through every switch that selects another kernel for it.

The oracle module only hands in mesh arrays (inputs); no assert reads an oracle value.  Every integrand is integrated
exactly: `qdegree` and the order of the runtime rules are at least its polynomial degree (asserted per family), so the
engine cannot pass by under-integrating the way a reference does.  Tolerances: tensors abs(got - exact) <=
1e-12 x the largest entry of the same tensor on the WHOLE cell or facet (x max abs of the cell's coefficient dofs where one
enters); assembled arrays rel_err <= 1e-12; the assembled two-space JUMP cancels and is measured on the scale of its
local tensors; lifting 1e-12 x max(abs(b0) + abs(A_exact) @ abs(alpha (g - x0))).  Left out: what `build_case`'s `keep`
leaves out (from the inputs alone, at most 5 %, none for the regular level sets; every assembled case is regular).
Each test prints its worst value ("EXACT <group> ..."; run with -s to see them); `test_exact_forms_reference.py` holds the
oracle to the same values on the CPU, so that a failure here can be placed.
"""
import os

import numpy as np
import pytest

import exact_cut as X
from helpers import profiled, rel_err
from test_exact_forms_reference import (ASSEMBLED_CASES, ENTITY_CASES, FACET2, G3, H2, LIFT_VARIANTS, PAIRS, RECT, RECT_ORDER,
                                        RECT_Q, S3, SOURCES, WEIGHTED_SPACES, _per_entity, coo, dofmaps, exact_poisson_entries,
                                        exact_rect, exact_source, exact_weighted, facet2_scale, kappa_values, left_out,
                                        lifting_data, rect_spec, weighted_degree, weighted_terms)
from test_gpu_exact_moments import _engine, _matrix_err, _space

pytestmark = pytest.mark.gpu
TOL = 1e-12
LD = X.LD
L3 = "3d-n4-sphere"             # the unscrambled lattice: closed-form and lattice rows exist there
KERNEL = {"mass": "MASS", "stiffness": "STIFFNESS", "elasticity": "ELASTICITY", "div_test": "DIV_TEST", "div_trial": "DIV_TRIAL"}


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _setup(cs, how="arrays"):
    import cutfemx_amd as cfx
    mesh, V1, fs, cd = _engine(cs, how)
    inside = cfx.locate_entities(cd, "phi<0")
    assert np.array_equal(inside, cs["inside"])
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), cs["cut"])
    left_out(cs)
    return mesh, cd, inside


def _vspace(cs, mesh, degree, bs=1):
    V, dofmap, ndofs = _space(cs, mesh, degree, bs)
    assert np.array_equal(dofmap, dofmaps(cs, degree)[0]) and ndofs == dofmaps(cs, degree)[1]
    return V


def _xc(cs):
    d = cs["tdim"]
    return lambda c: cs["x"][cs["conn"][c], :d]


# ---- 1. rectangular blocks ------------------------------------------------------------------------------------------------
def _rect_form(cs, mesh, cd, inside, block, shape="one"):
    import cutfemx_amd as cfx
    fem = cfx.fem
    kind, (d0, b0), (d1, b1), params, ideg = rect_spec(cs, block)
    assert RECT_Q >= ideg and RECT_ORDER >= ideg          # never below the integrand's degree
    R = cfx.runtime_quadrature(cd, "phi<0", RECT_ORDER)
    k = getattr(fem, KERNEL[kind])
    ints = [fem.Integral(k, cells=inside, rules=R, params=params, qdegree=RECT_Q)]
    if shape == "three":     # the uncut cells under one integral, the rules under another, and both once more
        ints = [fem.Integral(k, cells=inside, params=params, qdegree=RECT_Q), fem.Integral(k, rules=R, params=params, qdegree=RECT_Q)] + ints
    return fem.form(ints, _vspace(cs, mesh, d0, b0), trial_space=_vspace(cs, mesh, d1, b1)), R


@pytest.mark.parametrize("name", ENTITY_CASES)
def test_rectangular_tensors_are_the_exact_ones(oracle, name):
    """`Rect*` of cfx_elem.h through tabulate_entity: B^T (P2-vector x P1, DIV_TEST, scale -1), B (DIV_TRIAL), M21 (P2 x P1
    mass), K12 (P1 x P2 stiffness) on every kept cut cell's rule and one in ten inside cells."""
    import cutfemx_amd as cfx
    cs = X.build_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    d, xc, whole = cs["tdim"], _xc(cs), X.Moments(cs["tdim"])
    for block in RECT:
        kind, (d0, b0), (d1, b1), params, _ = rect_spec(cs, block)
        a, R = _rect_form(cs, mesh, cd, inside, block)
        worst, n = _per_entity(cs, name, R, lambda i, u: cfx.fem.tabulate_entity(a, 0, i, u),
                               lambda c, mom: X.rect_tensor(kind, mom, xc(c), d0, b0, d1, b1, params),
                               lambda c: np.abs(X.rect_tensor(kind, whole, xc(c), d0, b0, d1, b1, params)).max())
        _report("rect tensors", f"{name} {block} ({n} tensors)", worst)
        assert 0.0 < worst <= TOL, block


RECT_MODES = {"default": {}, "no-gather": {"CFX_RECT_GATHER": "0"}, "atomic": {"CFX_ASSEMBLY": "atomic"},
              "deterministic": {"CFX_DETERMINISTIC": "1"}}


@pytest.mark.parametrize("mode", list(RECT_MODES))
@pytest.mark.parametrize("shape", ["one", "three"])
@pytest.mark.parametrize("name", ASSEMBLED_CASES)
def test_assembled_rectangular_blocks_are_exact(oracle, monkeypatch, name, shape, mode):
    """The four blocks over [inside cells, rules] as one integral and as the three-integral form (twice the block): the
    row gather (`assemble_rows2`, one writer per row; bitwise reproducible under CFX_DETERMINISTIC=1), CFX_RECT_GATHER=0
    (`assemble_cells2_std` and atomics) and CFX_ASSEMBLY=atomic."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    outer_gather = os.environ.get("CFX_ASSEMBLY") != "atomic" and os.environ.get("CFX_RECT_GATHER") != "0"
    _set(monkeypatch, RECT_MODES[mode])
    cs = X.build_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    for block in RECT:
        a, _ = _rect_form(cs, mesh, cd, inside, block, shape)
        e, shp = exact_rect(name, cs, block)
        M = coo(e, shp) * (2.0 if shape == "three" else 1.0)
        A, names = profiled(lambda: fem.assemble_matrix(a))
        assert (A.nrows, A.ncols) == shp
        if mode in ("default", "deterministic") and outer_gather:
            assert "assemble_rows2" in names and "assemble_cells2_std" not in names, (block, sorted(names))
        if mode in ("no-gather", "atomic"):
            assert "assemble_rows2" not in names, (block, sorted(names))
        if mode == "no-gather":
            assert "assemble_cells2_std" in names, (block, sorted(names))
        err = _matrix_err(A, M)
        _report("rect assembled", f"{name} {block} {shape} {mode} {sorted(names)}", err)
        assert 0.0 < err <= TOL, block
        if mode == "deterministic" and outer_gather:
            assert np.array_equal(fem.assemble_matrix(a).data, A.data), block


# ---- 2. kappa-weighted forms ------------------------------------------------------------------------------------------------
def _weighted_form(cs, mesh, cd, inside, V, kind, params, ideg, degree, kappa):
    import cutfemx_amd as cfx
    fem = cfx.fem
    q = order = ideg
    assert q >= weighted_degree(kind, degree) and order >= weighted_degree(kind, degree)     # never below the integrand's degree
    R = cfx.runtime_quadrature(cd, "phi<0", order)
    return fem.form([fem.Integral(getattr(fem, KERNEL[kind]), cells=inside, rules=R, params=params, qdegree=q, coefficient=kappa)], V), R


@pytest.mark.parametrize("name", ENTITY_CASES)
def test_weighted_tensors_are_the_exact_ones(oracle, name):
    """`cell_local_row` with a coefficient through tabulate_entity: kappa x (mass, stiffness, elasticity) for P1, P2 and
    the vector spaces, kappa = 1 + U(0, 2) and kappa = U(-1, 1), each at the integrand's own degree (P2 mass: 6)."""
    import cutfemx_amd as cfx
    cs = X.build_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    d, xc = cs["tdim"], _xc(cs)
    for degree, bs in WEIGHTED_SPACES[d]:
        dm, nd = dofmaps(cs, degree)
        V = _vspace(cs, mesh, degree, bs)
        for which in (0, 1):
            kappa = kappa_values(nd, which)
            for kind, params, ideg in weighted_terms(name, degree, bs):
                md = max(4, ideg)
                a, R = _weighted_form(cs, mesh, cd, inside, V, kind, params, ideg, degree, kappa)
                whole = X.Moments(d, degree=md)
                blocks = (lambda T: X._diag_blocks(T, bs)) if kind != "elasticity" else (lambda T: T)
                worst, n = _per_entity(
                    cs, name, R, lambda i, u: cfx.fem.tabulate_entity(a, 0, i, u),
                    lambda c, mom: blocks(X.weighted(kind, mom, xc(c), degree, kappa[dm[c]], params)),
                    lambda c: np.abs(X.tensor(kind, whole, xc(c), degree, params)).max() * np.abs(kappa[dm[c]]).max(), md)
                _report("weighted tensors", f"{name} P{degree} bs {bs} {kind} q {ideg} kappa {which} ({n} tensors)", worst)
                assert 0.0 < worst <= TOL, (degree, bs, kind, which)


# every switch that selects another kernel for MASS / STIFFNESS / ELASTICITY (the `I.coefficient.n == 0` sites of
# cfx_gather.hip and cfx_rowasm.hip gate the closed-form rows, the lattice rows, the inline rows, cut_tensors_p1 and the
# P2 moments; the others choose between the gathers and the entity-parallel kernels)
WEIGHTED_MODES = {"rows": {}, "atomic": {"CFX_ASSEMBLY": "atomic"}, "no-p2-closed": {"CFX_P2_CLOSED": "0"},
                  "no-p2-moments": {"CFX_P2_MOMENTS": "0"}, "no-cut-tensors-p1": {"CFX_CUT_TENSORS_P1": "0"},
                  "no-vec-blocks": {"CFX_VEC_BLOCKS": "0"}, "no-block-gather": {"CFX_BLOCK_GATHER": "0"},
                  "no-stencil": {"CFX_STENCIL": "0"}, "no-bulk-rows": {"CFX_BULK_ROWS": "0"},
                  "no-lattice-rows": {"CFX_LATTICE_ROWS": "0"}, "split": {"CFX_ROWS_SPLIT": "1"},
                  "split-no-p2-cut-tensors": {"CFX_ROWS_SPLIT": "1", "CFX_P2_CUT_TENSORS": "0"}}


@pytest.mark.parametrize("mode", list(WEIGHTED_MODES))
@pytest.mark.parametrize("name", ASSEMBLED_CASES)
def test_assembled_weighted_forms_are_exact(oracle, monkeypatch, name, mode):
    """The same forms assembled over [inside cells, rules], both kappas, in every mode of WEIGHTED_MODES."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    _set(monkeypatch, WEIGHTED_MODES[mode])
    cs = X.build_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    worst = 0.0
    for degree, bs in WEIGHTED_SPACES[cs["tdim"]]:
        V = _vspace(cs, mesh, degree, bs)
        for which in (0, 1):
            kappa = kappa_values(dofmaps(cs, degree)[1], which)
            for kind, params, ideg in weighted_terms(name, degree, bs):
                a, _ = _weighted_form(cs, mesh, cd, inside, V, kind, params, ideg, degree, kappa)
                M = exact_weighted(name, cs, degree, bs, kind, params, kappa, ideg)
                A, names = profiled(lambda: fem.assemble_matrix(a))
                err = _matrix_err(A, M)
                _report("weighted assembled", f"{name} P{degree} bs {bs} {kind} q {ideg} kappa {which} {mode} {sorted(names)}", err)
                assert 0.0 < err <= TOL, (degree, bs, kind, which)
                worst = max(worst, err)
    assert worst > 0.0


MIXED_MODES = {"default": {}, "atomic": {"CFX_ASSEMBLY": "atomic"}, "no-lattice-rows": {"CFX_LATTICE_ROWS": "0"},
               "no-p2-closed": {"CFX_P2_CLOSED": "0"}, "no-bulk-rows": {"CFX_BULK_ROWS": "0"}}


@pytest.mark.parametrize("mode", list(MIXED_MODES))
@pytest.mark.parametrize("how", ["arrays", "box"])
def test_a_form_of_an_unweighted_and_a_weighted_integral_is_exact(oracle, monkeypatch, how, mode):
    """On the unscrambled 4^3 lattice, where complete rows are copied from a template or written in closed form: P1
    unweighted stiffness + kappa-weighted mass, and P2 unweighted stiffness + kappa-weighted stiffness, in one form.
    The special rows may serve the first integral and must not serve the second."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    _set(monkeypatch, MIXED_MODES[mode])
    cs = X.build_case(oracle, L3)
    mesh, cd, inside = _setup(cs, how)
    for degree, wkind in ((1, "mass"), (2, "stiffness")):
        dm, nd = dofmaps(cs, degree)
        V = _vspace(cs, mesh, degree)
        ideg = weighted_degree(wkind, degree)
        q0 = 2 * (degree - 1)
        R0, R1 = cfx.runtime_quadrature(cd, "phi<0", max(q0, 1)), cfx.runtime_quadrature(cd, "phi<0", ideg)
        for which in (0, 1):
            kappa = kappa_values(nd, which)
            a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=R0, qdegree=q0),
                          fem.Integral(getattr(fem, KERNEL[wkind]), cells=inside, rules=R1, qdegree=ideg, coefficient=kappa)], V)
            K = coo(X.exact_entries(L3, cs, dm, 1, "stiffness", degree, (), cs["inside"]), (nd, nd))
            W = exact_weighted(L3, cs, degree, 1, wkind, (), kappa, ideg)
            assert 1e-3 < abs(W).max() / abs(K).max() < 1e3
            A, names = profiled(lambda: fem.assemble_matrix(a))
            err = _matrix_err(A, K + W)
            _report("weighted assembled", f"{L3} ({how}) P{degree} stiffness + kappa {which} x {wkind} {mode} {sorted(names)}", err)
            assert 0.0 < err <= TOL, (degree, which)


# ---- 3. coefficient sources ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "no-vec-blocks", "atomic"])
@pytest.mark.parametrize("name", ENTITY_CASES + [G3])
def test_coefficient_sources_are_exact(oracle, monkeypatch, name, mode):
    """SOURCE with F_COEFFICIENT (`vec_local`, the cell-block sums): scalar (P1 3-D, P2 2-D) and vector-valued (P1 bs = 3,
    P2 bs = 2, scale 1.5), per entity and assembled; CFX_VEC_BLOCKS=0 and the entity-parallel atomics as well."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    _set(monkeypatch, {"no-vec-blocks": {"CFX_VEC_BLOCKS": "0"}, "atomic": {"CFX_ASSEMBLY": "atomic"}}.get(mode, {}))
    cs = X.build_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    d, xc, whole = cs["tdim"], _xc(cs), X.Moments(cs["tdim"])
    for degree, bs, scale in SOURCES[d]:
        dm, nd = dofmaps(cs, degree)
        w = np.random.default_rng(23 + bs).standard_normal(nd * bs)
        q = order = 2 * degree
        assert q >= 2 * degree and order >= 2 * degree             # f and v are both of the space's degree
        V = _vspace(cs, mesh, degree, bs)
        R = cfx.runtime_quadrature(cd, "phi<0", order)
        L = fem.form([fem.Integral(fem.SOURCE, cells=inside, rules=R, params=(fem.F_COEFFICIENT, scale), qdegree=q, coefficient=w)], V)
        wc = lambda c: w.reshape(nd, bs)[dm[c]]
        if name in ENTITY_CASES and mode == "default":
            worst, n = _per_entity(cs, name, R, lambda i, u: fem.tabulate_entity(L, 0, i, u),
                                   lambda c, mom: X.source_coeff(mom, xc(c), degree, wc(c), bs, scale),
                                   lambda c: scale * np.abs(X.mass(whole, xc(c), degree)).max() * np.abs(wc(c)).max())
            _report("source tensors", f"{name} P{degree} bs {bs} ({n} vectors)", worst)
            assert 0.0 < worst <= TOL, (degree, bs)
        if name in ASSEMBLED_CASES:
            b, names = profiled(lambda: fem.assemble_vector(L))
            err = rel_err(b, exact_source(name, cs, degree, bs, scale, w))
            _report("source assembled", f"{name} P{degree} bs {bs} {mode} {sorted(names)}", err)
            assert 0.0 < err <= TOL, (degree, bs)


# ---- 4. lifting and set_bc ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "atomic"])
@pytest.mark.parametrize("name", [H2, S3])
def test_lifting_is_exact(oracle, monkeypatch, name, mode):
    """apply_lifting through the square P1 Poisson matrix (stiffness + ghost penalty), the P2 stiffness and the rectangular
    B^T and M21 (trial-space data, test-space vector): seeded 10 % markers, random g, x0, b0, alpha 1 and 0.7, with and
    without x0, against b0 - A_exact alpha (g - x0) accumulated in longdouble."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "atomic":
        monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    R = cfx.runtime_quadrature(cd, "phi<0", 4)
    n1, n2 = dofmaps(cs, 1)[1], dofmaps(cs, 2)[1]
    forms = {"P1 poisson": (fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=R, qdegree=0),
                                      fem.Integral(fem.GHOST_GRADJUMP, facets=fc["ghost"], params=(0.1,), qdegree=0)], _vspace(cs, mesh, 1)),
                            exact_poisson_entries(name, cs, fc), (n1, n1)),
             "P2 stiffness": (fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=R, qdegree=2)], _vspace(cs, mesh, 2)),
                              X.exact_entries(name, cs, dofmaps(cs, 2)[0], 1, "stiffness", 2, (), cs["inside"]), (n2, n2))}
    for block in ("Bt", "M21"):
        forms[block] = (_rect_form(cs, mesh, cd, inside, block)[0],) + exact_rect(name, cs, block)
    for what, (a, entries, shape) in forms.items():
        marks, g, x0, b0 = lifting_data(entries, shape, 31)
        worst = 0.0
        for alpha, with_x0 in LIFT_VARIANTS:
            want, scale = X.exact_lift(entries, shape, marks, g, x0 if with_x0 else None, alpha, b0)
            got = fem.apply_lifting(b0.copy(), a, marks, g, x0=x0 if with_x0 else None, alpha=alpha)
            assert np.abs(want - b0).max() > 1e-3 * scale
            worst = max(worst, np.abs(got - want).max() / scale)
        _report("lifting", f"{name} {what} {mode}", worst)
        assert 0.0 < worst <= TOL, what


def test_set_bc_is_alpha_times_g_minus_x0_on_the_marked_dofs():
    """set_bc against alpha (g - x0) in longdouble, rounded once; unmarked entries keep their values bit for bit."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    n = 4099
    rng = np.random.default_rng(41)
    marks = (rng.random(n) < 0.1).astype(np.int8)
    g, x0, b0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    worst = 0.0
    for alpha, with_x0 in LIFT_VARIANTS:
        got = fem.set_bc(b0.copy(), marks, g, x0=x0 if with_x0 else None, alpha=alpha)
        want = (LD(alpha) * (g.astype(LD) - (x0.astype(LD) if with_x0 else 0))).astype(np.float64)
        scale = abs(alpha) * (np.abs(g) + (np.abs(x0) if with_x0 else 0.0)).max()
        assert np.array_equal(got[marks == 0], b0[marks == 0])
        worst = max(worst, np.abs(got - want)[marks != 0].max() / scale)
        assert np.abs(got - b0)[marks != 0].min() > 0
    _report("lifting", "set_bc", worst)
    assert worst <= TOL


# ---- 5. interior-facet terms between two scalar spaces -----------------------------------------------------------------------
def _facet2_integral(fem, kind, params, q, ideg, rows):
    assert q >= ideg                                            # never below the integrand's degree
    return fem.Integral(fem.GHOST_GRADJUMP if kind == "ghost" else fem.JUMP, facets=rows, params=params, qdegree=q)


@pytest.mark.parametrize("name", ENTITY_CASES)
def test_two_space_facet_tensors_are_the_exact_ones(oracle, name):
    """`facet_local_row2` through tabulate_entity: GHOST_GRADJUMP (0.3, 2.0) at qdegree 2 and JUMP (5.0,) at qdegree 3 for
    P2 x P1 and P1 x P2 on every kept ghost facet; on the scrambled cases the two cells' h differ."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    g = cfx.ghost_penalty_facets(cd, "phi<0")
    assert sorted(map(tuple, g.rows.tolist())) == list(map(tuple, fc["ghost"].tolist()))
    whole = X.Moments(cs["tdim"] - 1)
    for pair, (d0, d1) in PAIRS.items():
        V0, V1 = _vspace(cs, mesh, d0), _vspace(cs, mesh, d1)
        for kind, params, q, ideg in FACET2:
            a = fem.form([_facet2_integral(fem, kind, params, q, ideg, fc["ghost"])], V0, trial_space=V1)
            worst, n = 0.0, 0
            for i, row in enumerate(fc["ghost"]):
                if not fc["ghost_keep"][i]:
                    continue
                want = X.facet_tensor2(kind, X.facet_basis(name, cs, row, d0), X.facet_basis(name, cs, row, d1), whole, params)
                got = np.asarray(fem.tabulate_entity(a, 0, i, False))
                assert got.shape == want.shape
                worst = max(worst, np.abs(got - want.astype(np.float64)).max() / float(np.abs(want).max()))
                n += 1
            _report("facet2 tensors", f"{name} {pair} {kind} ({n} tensors)", worst)
            assert n > 0 and 0.0 < worst <= TOL, (pair, kind)


@pytest.mark.parametrize("mode", list(RECT_MODES))
@pytest.mark.parametrize("name", ASSEMBLED_CASES)
def test_assembled_two_space_facet_terms_are_exact(oracle, monkeypatch, name, mode):
    """The same terms assembled over the ghost facets, alone and next to the mass block over [inside cells, rules].  The
    value-jump block of two continuous spaces cancels in the assembled matrix: every difference is measured on the scale
    of the term's local tensors."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    _set(monkeypatch, RECT_MODES[mode])
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, cd, inside = _setup(cs)
    R = cfx.runtime_quadrature(cd, "phi<0", RECT_ORDER)
    for pair, (d0, d1) in PAIRS.items():
        V0, V1 = _vspace(cs, mesh, d0), _vspace(cs, mesh, d1)
        (dm0, n0), (dm1, n1) = dofmaps(cs, d0), dofmaps(cs, d1)
        Mx = coo(X.exact_entries(name, cs, dm0, 1, "mass", d0, (), cs["inside"], trial=(dm1, 1, d1)), (n0, n1))
        for kind, params, q, ideg in FACET2:
            If = _facet2_integral(fem, kind, params, q, ideg, fc["ghost"])
            scale = facet2_scale(name, cs, fc["ghost"], kind, params, d0, d1)
            G = coo(X.exact_facet_entries2(name, cs, dm0, d0, dm1, d1, kind, params, fc["ghost"]), (n0, n1))
            A, names = profiled(lambda: fem.assemble_matrix(fem.form([If], V0, trial_space=V1)))
            e1 = abs(A.to_scipy().tocsr() - G).max() / scale
            assert RECT_Q >= 3                                  # the P2 x P1 mass integrand
            Im = fem.Integral(fem.MASS, cells=inside, rules=R, qdegree=RECT_Q)
            A2 = fem.assemble_matrix(fem.form([If, Im], V0, trial_space=V1))
            e2 = abs(A2.to_scipy().tocsr() - (G + Mx)).max() / max(scale, abs(Mx).max())
            _report("facet2 assembled", f"{name} {pair} {kind} {mode} {sorted(names)}: alone {e1:.3e} with mass", e2)
            assert e1 <= TOL and 0.0 < e2 <= TOL, (pair, kind)
