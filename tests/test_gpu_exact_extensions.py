"""The HIP engine against the exact values of `exact_cut.py` (not against the oracle) for the extension penalty and the
cell aggregation that feeds it: `EXTENSION_L2` was the one polynomial integrand whose arithmetic kernel and oracle restate
line for line (full-cell rule of the bad cell, abs(det) of the bad cell, pull-back through the root's inverse Jacobian,
macro basis [N_bad, -N_root]), so a slip made on both sides passed `test_gpu_extensions.py`.

Per entity: `fem.tabulate_entity` of EVERY (bad, root) pair of every case (up to 1248), degree 1 and 2, scalar and on the
block spaces.  Assembled: (a) the pair form alone, (b) with cellwise beta (random, read through the public API), (c)
stiffness over [inside cells, phi<0 rules] + ghost penalty + pair form (folded and unfolded facet items in one form), (d)
a second assembly into the same matrix, (e) the empty pair list; through every switch that selects another kernel for
them; lifting through (c) and through the pair form.  The pairs come from the engine's own `create_cell_aggregation`; what
a valid aggregation is -- exact volume fractions, classes from mathematics, structure from the definition -- is stated
without the oracle in `test_exact_extension_reference.check_aggregation` and asserted here for both selectors, three
thresholds and both root policies.

The oracle module only hands in mesh arrays (inputs); no assert reads an oracle value.  Tolerances: a pair
tensor block by block, abs(got - exact) <= 1e-12 x sqrt(max|T_aa| max|T_bb|); assembled arrays entry by entry, 1e-12 x the
sum of the absolute exact contributions to the entry, and rel_err <= 1e-12 on the whole array; fractions absolute 1e-12;
lifting on `exact_lift`'s scale.  `qdegree = 2 degree` is the integrand's degree (asserted).  Nothing is left out.  Each
test prints its worst value ("EXACT <group> ..."; run with -s); `test_exact_extension_reference.py` holds the oracle to the
same values on the CPU, so that a failure here can be placed.
"""
import os

import numpy as np
import pytest

import exact_cut as X
from helpers import profiled
from test_exact_extension_reference import (AGG_CASES, AGG_THRESHOLDS, BETA, C2, G6, GHOST, PAIR_CASES, PAIR_IDS, POLICIES, S3, SELECTORS,
                                            beta_cells, block_spaces, check_aggregation, check_fractions, check_pair_case,
                                            entry_errors, exact_form_c, exact_pair, pair_errors, thresholds_are_decidable)
from test_exact_forms_reference import dofmaps, left_out, lifting_data
from test_gpu_exact_moments import _engine, _space

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def _foreign_switches():
    """Switches of the whole run (tools/test_modes.sh): the results hold under all of them, the kernel names of the
    default configuration do not."""
    return [k for k in os.environ if k.startswith("CFX_") and k not in ("CFX_STEP_DEBUG", "CFX_COUNT_SYNC", "CFX_DEVICE")]


def _setup(cs, thr):
    """Mesh, cut and the engine's own aggregation of `phi<0`; the case's entities from the inputs alone."""
    import cutfemx_amd as cfx
    mesh, V1, fs, cd = _engine(cs)
    inside = cfx.locate_entities(cd, "phi<0")
    assert np.array_equal(inside, cs["inside"]) and np.array_equal(np.flatnonzero(cd.domain() == 0), cs["cut"])
    left_out(cs)
    agg = cfx.extensions.create_cell_aggregation(cd, "phi<0", thr)
    assert agg.num_pairs == agg.pairs.shape[0]
    return mesh, cd, inside, agg


def _vspace(cs, mesh, degree, bs=1):
    V, dofmap, ndofs = _space(cs, mesh, degree, bs)
    assert np.array_equal(dofmap, dofmaps(cs, degree)[0]) and ndofs == dofmaps(cs, degree)[1]
    return V


def _pair_integral(agg, degree, beta=BETA):
    import cutfemx_amd as cfx
    q = 2 * degree
    assert q >= 2 * degree                                        # never below the integrand's degree
    return cfx.extensions.extension_penalty_integral(agg, beta, q)


def _errors(A, exact, factor=1.0):
    r, c, v, s = exact
    return entry_errors(A.indptr, A.indices, A.data, (r, c, factor * v, factor * s), A.ncols)


# ---- per entity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,thr,degrees", PAIR_CASES, ids=PAIR_IDS)
def test_pair_tensors_are_the_exact_ones(oracle, name, thr, degrees):
    """`facet_local_row` with EXTENSION_L2 through tabulate_entity: every pair, scalar and on the block spaces (P1 bs = 3
    in 3-D, P2 bs = 2 in 2-D), each of the four blocks on its own scale."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    mesh, cd, inside, agg = _setup(cs, thr)
    pairs = agg.pairs
    for degree in degrees:
        check_pair_case(cs, thr, degree, pairs)
        ndc = dofmaps(cs, degree)[0].shape[1]
        for bs in block_spaces(cs["tdim"], degree):
            a = fem.form([_pair_integral(agg, degree)], _vspace(cs, mesh, degree, bs))
            worst, whole = np.zeros(4), 0.0
            for i, row in enumerate(pairs):
                T = exact_pair(name, cs, degree, bs, row)
                got = np.asarray(fem.tabulate_entity(a, 0, i, False))
                assert got.shape == T.shape
                worst = np.maximum(worst, pair_errors(got, T, ndc * bs))
                whole = max(whole, np.abs(got - T).max() / np.abs(T).max())
            _report("pair tensors", f"{name} thr {thr} P{degree} bs {bs} ({len(pairs)} pairs): whole tensor {whole:.3e} "
                    f"blocks {' '.join(f'{v:.1e}' for v in worst)}", worst.max())
            assert 0.0 < worst.max() <= TOL, (degree, bs)


# ---- assembled ------------------------------------------------------------------------------------------------------------
MODES = {"default": {}, "atomic": {"CFX_ASSEMBLY": "atomic"}, "deterministic": {"CFX_DETERMINISTIC": "1"},
         "no-fold-stage1": {"CFX_FACET_FOLD_STAGE1": "0"}, "no-stencil": {"CFX_STENCIL": "0"}, "split": {"CFX_ROWS_SPLIT": "1"},
         "no-block-gather": {"CFX_BLOCK_GATHER": "0"}, "no-vec-blocks": {"CFX_VEC_BLOCKS": "0"}}
BLOCK_MODES = ("no-block-gather", "no-vec-blocks")               # on the block spaces only


def _form_c(cs, fc, cd, inside, agg, V, degree):
    import cutfemx_amd as cfx
    fem = cfx.fem
    qs, order = 2 * (degree - 1), 4
    assert order >= qs                                             # stiffness and gradient jump: degree 2 (degree - 1)
    R = cfx.runtime_quadrature(cd, "phi<0", order)
    return fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=R, qdegree=qs),
                     fem.Integral(fem.GHOST_GRADJUMP, facets=fc["ghost"], params=GHOST[:1], qdegree=qs),
                     _pair_integral(agg, degree)], V)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,thr,degrees", PAIR_CASES, ids=PAIR_IDS)
def test_assembled_pair_forms_are_exact(oracle, monkeypatch, name, thr, degrees, mode):
    """(a) the pair form, (b) with cellwise beta in [0.5, 2], (c) next to stiffness and ghost penalty (not on the 1248-pair
    case, which serves the pair form at P1), (d) assembled twice into one matrix; under CFX_DETERMINISTIC=1 two runs are
    bit-equal where the row gather assembles (the scalar spaces)."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    outer_atomic = os.environ.get("CFX_ASSEMBLY") == "atomic"
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    cs = X.build_case(oracle, name)
    fc = X.facet_case(oracle, name) if name != G6 else None
    mesh, cd, inside, agg = _setup(cs, thr)
    pairs = agg.pairs
    bcell = beta_cells(cs["conn"].shape[0])
    done = 0
    for degree in degrees:
        dm, nd = dofmaps(cs, degree)
        for bs in block_spaces(cs["tdim"], degree):
            if mode in BLOCK_MODES and bs == 1:
                continue
            V = _vspace(cs, mesh, degree, bs)
            forms = {"a": (fem.form([_pair_integral(agg, degree)], V), X.exact_pair_entries(name, cs, dm, bs, degree, pairs, BETA)),
                     "b": (fem.form([_pair_integral(agg, degree, bcell)], V), X.exact_pair_entries(name, cs, dm, bs, degree, pairs, 1.0, bcell))}
            if fc is not None:
                forms["c"] = (_form_c(cs, fc, cd, inside, agg, V, degree), exact_form_c(name, cs, fc, thr, degree, bs, pairs))
            for what, (a, ex) in forms.items():
                A, names = profiled(lambda: fem.assemble_matrix(a))
                assert (A.nrows, A.ncols) == (nd * bs, nd * bs)
                worst, rel = _errors(A, ex)
                _report("pair forms assembled", f"{name} thr {thr} P{degree} bs {bs} ({what}) {mode} {sorted(names)}: whole array {rel:.3e} "
                        "per entry", worst)
                assert 0.0 < worst <= TOL and rel <= TOL, (degree, bs, what)
                # the row gather serves the scalar spaces; on a block space a form with pairs keeps the entity-parallel
                # kernel and its global atomics (assemble_matrix_rows), which CFX_DETERMINISTIC does not order
                gathered = any(k.startswith("assemble_rows") for k in names)
                if _foreign_switches() == list(MODES[mode]) and mode != "atomic":
                    assert gathered == (bs == 1) and (gathered or "assemble_facets" in names), (degree, bs, what, sorted(names))
                if mode == "deterministic" and gathered and not outer_atomic:
                    assert np.array_equal(fem.assemble_matrix(a).data, A.data), (degree, bs, what)
                if what != "b":
                    fem.assemble_matrix(a, A=A)                    # (d) accumulates: twice the entries
                    worst, rel = _errors(A, ex, 2.0)
                    assert 0.0 < worst <= TOL and rel <= TOL, (degree, bs, what, "twice")
                done += 1
    assert done > 0 or mode in BLOCK_MODES


@pytest.mark.parametrize("mode", ["default", "atomic"])
def test_rows_beyond_512_columns_take_the_entity_parallel_kernels(oracle, monkeypatch, mode):
    """P2 bs = 3 on the scrambled 3-D n = 4 sphere at threshold 1.0: the root of 106 bad cells has rows of 3 x 262 = 786
    columns, in (512, 2047]: the entity-parallel kernel (`assemble_facets`) assembles, no row gather.  The sparsity of a
    block space is built on its nodes (262 columns: `pattern_rows_wide`, not the 2048-slot set).  Forms (a) and (c), and
    (a) twice."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "atomic":
        monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    cs, fc = X.build_case(oracle, S3), X.facet_case(oracle, S3)
    mesh, cd, inside, agg = _setup(cs, 1.0)
    pairs = agg.pairs
    dm, nd = dofmaps(cs, 2)
    longest = X.longest_pair_row(dm, 3, pairs, nd)
    assert longest == 786 and 512 < longest <= 2047
    V = _vspace(cs, mesh, 2, 3)
    for what, a, ex in (("a", fem.form([_pair_integral(agg, 2)], V), X.exact_pair_entries(S3, cs, dm, 3, 2, pairs, BETA)),
                        ("c", _form_c(cs, fc, cd, inside, agg, V, 2), exact_form_c(S3, cs, fc, 1.0, 2, 3, pairs))):
        A, names = profiled(lambda: fem.assemble_matrix(a))
        assert int(np.diff(A.indptr).max()) >= longest
        if what == "a":
            assert int(np.diff(A.indptr).max()) == longest
        if not _foreign_switches() or (mode == "atomic" and _foreign_switches() == ["CFX_ASSEMBLY"]):
            assert not any(k.startswith("assemble_rows") for k in names), sorted(names)
            assert "assemble_facets" in names and "pattern_rows_huge" not in names, sorted(names)
        worst, rel = _errors(A, ex)
        _report("pair forms assembled", f"{S3} thr 1.0 P2 bs 3 ({what}) {mode} {sorted(names)}: whole array {rel:.3e} per entry", worst)
        assert 0.0 < worst <= TOL and rel <= TOL, what
        if what == "a":
            fem.assemble_matrix(a, A=A)
            worst, rel = _errors(A, ex, 2.0)
            assert 0.0 < worst <= TOL and rel <= TOL


@pytest.mark.parametrize("name", [C2, S3])
def test_the_empty_pair_list_gives_the_diagonal_pattern_with_zero_values(oracle, name):
    """(e) threshold 0.0 with `interior_or_well_cut` makes every cut cell a root: no pairs.  `create_extension_penalty_matrix`
    and `extension_penalty_matrix` give the all-rows diagonal pattern (bs x bs blocks) with zero values and raise nothing."""
    import cutfemx_amd as cfx
    ext = cfx.extensions
    cs = X.build_case(oracle, name)
    mesh, cd, inside, agg = _setup(cs, 0.0)
    assert agg.num_pairs == 0 and agg.pairs.shape == (0, 4) and agg.ill_posed_cells.size == 0
    assert np.array_equal(agg.well_posed_cells, np.union1d(cs["inside"], cs["cut"]))
    for degree, bs in ((1, 1), (2, 1), (1, cs["tdim"])):
        V = _vspace(cs, mesh, degree, bs)
        n = dofmaps(cs, degree)[1] * bs
        for A in (ext.create_extension_penalty_matrix(V, cd, agg), ext.extension_penalty_matrix(V, cd, agg, BETA, 2 * degree),
                  ext.extension_penalty_matrix(V, cd, agg, beta_cells(cs["conn"].shape[0]), 2 * degree)):
            assert (A.nrows, A.ncols) == (n, n)
            # (the all-rows diagonal of a block space is the bs x bs block: patterns live in block-index space)
            assert np.array_equal(A.indptr, bs * np.arange(n + 1))
            assert np.array_equal(A.indices, (np.arange(n)[:, None] // bs * bs + np.arange(bs)).ravel())
            assert A.data.shape == (n * bs,) and np.all(A.data == 0.0)


# ---- lifting --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "atomic"])
@pytest.mark.parametrize("name,thr,degree", [(S3, 1.0, 1), (C2, 1.0, 2)], ids=["P1-3d", "P2-2d"])
def test_lifting_through_pair_forms_is_exact(oracle, monkeypatch, name, thr, degree, mode):
    """apply_lifting through form (c) and through the pair form alone: seeded 10 % markers, random g, x0, b0, alpha 0.7,
    with and without x0, against b0 - A_exact alpha (g - x0) accumulated in longdouble."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "atomic":
        monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    mesh, cd, inside, agg = _setup(cs, thr)
    pairs = agg.pairs
    dm, nd = dofmaps(cs, degree)
    V = _vspace(cs, mesh, degree)
    forms = {"pair form": (fem.form([_pair_integral(agg, degree)], V), X.exact_pair_entries(name, cs, dm, 1, degree, pairs, BETA)),
             "form (c)": (_form_c(cs, fc, cd, inside, agg, V, degree), exact_form_c(name, cs, fc, thr, degree, 1, pairs))}
    for what, (a, ex) in forms.items():
        entries = ex[:3]
        marks, g, x0, b0 = lifting_data(entries, (nd, nd), 31)
        worst = 0.0
        for with_x0 in (False, True):
            want, scale = X.exact_lift(entries, (nd, nd), marks, g, x0 if with_x0 else None, 0.7, b0)
            got = fem.apply_lifting(b0.copy(), a, marks, g, x0=x0 if with_x0 else None, alpha=0.7)
            assert np.abs(want - b0).max() > 1e-3 * scale
            worst = max(worst, np.abs(got - want).max() / scale)
        _report("pair lifting", f"{name} thr {thr} P{degree} {what} {mode}", worst)
        assert 0.0 < worst <= TOL, what


# ---- the aggregation, without the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", AGG_CASES)
def test_the_aggregation_is_a_valid_one(oracle, name, policy):
    """`create_cell_aggregation` for both selectors and thresholds 0.3, 0.6, 1.0: `cut_volume_fraction` is the exact fraction
    on the cut cells (absolute 1e-12) and 0 elsewhere, the two selectors add up to 1; well-posed = interior U {cut cells
    with exact fraction >= threshold} (or interior alone), no fraction within 1e-9 of a threshold; roots, depths, aggregate
    ids, the neighbour one step nearer the root, the rootless cells by connected components, and the pairs."""
    import cutfemx_amd as cfx
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), cs["cut"])
    thresholds_are_decidable(name, cs)
    for thr in AGG_THRESHOLDS:
        frac = {}
        for sel in SELECTORS:
            agg = cfx.extensions.create_cell_aggregation(cd, sel, thr, root_policy=policy, allow_rootless=True)
            frac[sel] = agg.cut_volume_fraction
            worst = check_fractions(name, cs, sel, frac[sel])
            pairs, deepest, lonely = check_aggregation(name, cs, sel, thr, policy, agg)
            assert np.array_equal(agg.pairs, pairs) and agg.num_pairs == len(pairs)
            _report("fractions", f"{name} {sel} thr {thr} {policy}: pairs {len(pairs)} deepest {deepest} rootless {lonely}", worst)
            assert 0.0 < worst <= TOL
        assert np.abs(frac["phi<0"] + frac["phi>0"] - 1.0)[cs["cut"]].max() <= TOL
