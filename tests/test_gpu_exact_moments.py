"""The HIP engine against the exact rational reference of `exact_cut.py` (not against the oracle): runtime rules of one
and several level sets and of facet hosts, rules after update(), the float32 boundary, the local tensor of EVERY cut
cell, assembled matrices / vectors on their named kernel paths, interface normals.

The oracle module only hands in mesh arrays (inputs); no assert reads an oracle value.  float64: abs(got - exact) <=
1e-12 x the same moment of the WHOLE cell (tensors: the largest entry of the whole cell's exact tensor; assembled
arrays: helpers.rel_err).  Cells left out: `exact_cut.build_case` (selected from the inputs alone, at most 5 %).
Each test prints its worst value ("EXACT <group> ..."; run with -s to see them).
"""
import os

import numpy as np
import pytest

import exact_cut as X
from helpers import profiled, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-12
SPHERES = ["2d-n8-sphere", "3d-n4-sphere"]
TENSOR_CASES = ["2d-n8-sphere", "3d-n4-sphere", "3d-n4-sphere-scrambled", "2d-n7-degenerate-scrambled"]
HOST_CASES = [(n, "interior") for n in SPHERES + ["3d-n4-degenerate", "2d-n7-degenerate-scrambled"]] + \
             [("3d-n5-gyroid", "exterior"), ("3d-n4-degenerate", "exterior")]
KERNEL = {"stiffness": "STIFFNESS", "mass": "MASS", "elasticity": "ELASTICITY"}


def _off(name):
    return os.environ.get(name) == "0"


def _default_paths():
    """Whether the run is in the default mode as far as the kernel names asserted below go (the diagnostic modes of
    tools/test_modes.sh switch single paths off with the same results; the names are then those of the generic path)."""
    env = os.environ.get
    return not (env("CFX_ASSEMBLY") == "atomic" or env("CFX_DETERMINISTIC") == "1" or _off("CFX_STENCIL")
                or _off("CFX_P2_CLOSED") or _off("CFX_P2_CUT_TENSORS") or _off("CFX_P2_MOMENTS") or _off("CFX_P2_PLAIN")
                or _off("CFX_BLOCK_PLAIN") or _off("CFX_TILES") or _off("CFX_BULK_ROWS") or _off("CFX_MFMA"))


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def _engine(cs, how="arrays", phis=None):
    import cutfemx_amd as cfx
    tdim = cs["tdim"]
    if how == "box":
        mesh = cfx.Mesh.create_box(tdim, cs["n"])
        assert np.array_equal(mesh.conn, cs["conn"]) and np.array_equal(mesh.x, cs["x"])
    else:
        mesh = cfx.Mesh.from_arrays(tdim, cs["x"], cs["conn"])
    V = cfx.FunctionSpace(mesh, 1)
    fs = [cfx.Function(V, p.copy()) for p in (phis if phis is not None else [cs["phi"]])]
    cd = cfx.cut(fs if phis is not None else fs[0])
    return mesh, V, fs, cd


def _check_volume_rules(cs, cd, sel, orders, key, group):
    import cutfemx_amd as cfx
    tdim, cut = cs["tdim"], cs["cut"]
    phis = cs.get("phis", [cs["phi"]])
    ex, alphas = X.exact_volume_moments(key, cs["x"], cs["conn"], phis, cut, sel, max(orders))
    full, vol = X.whole_moments(tdim, alphas), X.cell_measures(cs["x"], cs["conn"], tdim)
    deg = np.array([sum(a) for a in alphas])
    worst = 0.0
    for order in orders:
        R, names = profiled(lambda: cfx.runtime_quadrature(cd, sel, order))
        assert ("multi_rules_emit" if "phis" in cs else "cut_emit") in names, sorted(names)
        assert R.parent_map.size > 0 and np.all(np.isin(R.parent_map, cut)) and np.all(np.isfinite(R.weights))
        got = X.rule_moments(R, alphas, cs["conn"].shape[0])[cut] / vol[cut, None]
        err = (np.abs(got - ex) / full)[cs["keep"]][:, deg <= order].max()
        worst = max(worst, err)
        assert err <= TOL, (sel, order, err)
        # every point lies in the reference simplex and inside every clause (1e-14, as test_rule_array_contracts)
        lam = np.concatenate([1.0 - R.points.sum(axis=1, keepdims=True), R.points], axis=1)
        owner = np.repeat(R.parent_map, np.diff(R.offsets))
        assert lam.min() > -1e-14 and lam.max() < 1 + 1e-14
        for k, side in X.parse(sel):
            pv = phis[k][cs["conn"][owner]]
            assert np.all(side * np.einsum("qk,qk->q", lam, pv) >= -1e-14 * np.abs(pv).max(axis=1)), (sel, order)
    _report(group, f"{key} {sel} orders {tuple(orders)}", worst)


def _check_interface_rules(cs, cd, sel, orders, key, group, keep):
    import cutfemx_amd as cfx
    tdim, cut = cs["tdim"], cs["cut"]
    phis = cs.get("phis", [cs["phi"]])
    ex, alphas = X.exact_interface_moments(key, cs["x"], cs["conn"], phis, cut, sel, max(orders))
    scale = X.interface_scale(cs["x"], cs["conn"], cut, tdim)[:, None] * X.whole_moments(tdim, alphas)
    deg = np.array([sum(a) for a in alphas])
    worst = 0.0
    for order in orders:
        R = cfx.runtime_quadrature(cd, sel, order)
        got = X.rule_moments(R, alphas, cs["conn"].shape[0])[cut]
        err = (np.abs(got - ex) / scale)[keep][:, deg <= order].max()
        worst = max(worst, err)
        assert err <= TOL, (sel, order, err)
    _report(group, f"{key} {sel} orders {tuple(orders)}", worst)


def _left_out(cs, keep):
    n_out = int((~keep).sum())
    assert n_out <= 0.05 * cs["cut"].size and (cs["degenerate"] or n_out == 0), (n_out, cs["cut"].size)


# ---- rules --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how", [(n, "arrays") for n in X.CASES] + [(n, "box") for n in SPHERES])
def test_runtime_rules_have_the_exact_moments(oracle, name, how):
    """cut_emit_kernel: phi<0, phi>0, phi=0 at every order of the case; Mesh.from_arrays, scrambled meshes, and the
    generated box (whose culled classification feeds the rules)."""
    cs = X.build_case(oracle, name)
    mesh, V, fs, cd = _engine(cs, how)
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), cs["cut"])
    _left_out(cs, cs["keep"])
    _left_out(cs, cs["keep_itf"])
    for sel in ("phi<0", "phi>0"):
        _check_volume_rules(cs, cd, sel, cs["orders"], name, "rules")
    _check_interface_rules(cs, cd, "phi=0", cs["orders"], name, "rules", cs["keep_itf"])


@pytest.mark.parametrize("name", ["2d-n8-sphere", "3d-n4-sphere-scrambled"])
def test_rules_after_update_have_the_exact_moments(oracle, name):
    import cutfemx_amd as cfx
    cs, moved = X.build_case(oracle, name), X.moved_case(oracle, name)
    mesh, V, fs, cd = _engine(cs)
    assert cfx.runtime_quadrature(cd, "phi<0", 2).parent_map.size == cs["cut"].size
    fs[0].values[:] = moved["phi"]
    cd.update()
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), moved["cut"]) and not np.array_equal(moved["cut"], cs["cut"])
    for sel in ("phi<0", "phi>0"):
        _check_volume_rules(moved, cd, sel, (2, 4), moved["name"], "rules")
    _check_interface_rules(moved, cd, "phi=0", (2, 4), moved["name"], "rules", moved["keep"])


@pytest.mark.parametrize("name", SPHERES + ["3d-n4-sphere-scrambled"])
def test_multi_level_set_rules_have_the_exact_moments(oracle, name):
    """multi_rules_kernel with the selectors of tests/test_gpu_multi_level_set.py."""
    cs = X.multi_case(oracle, name)
    mesh, V, fs, cd = _engine(cs, phis=cs["phis"])
    keep = np.ones(cs["cut"].size, dtype=bool)
    cs = dict(cs, keep=keep)
    for sel in ("phi<0 and phi1>0", "phi<0 and phi1<0", "phi>0 and phi1<0", "phi1>0 and phi<0"):
        _check_volume_rules(cs, cd, sel, (2, 4), "multi-" + name, "multi")
    for sel in ("phi=0 and phi1<0", "phi1=0 and phi<0"):
        _check_interface_rules(cs, cd, sel, (2, 4), "multi-" + name, "multi", keep)


@pytest.mark.parametrize("name,which", HOST_CASES)
def test_facet_host_rules_have_the_exact_moments(oracle, name, which):
    """facet_emit_kernel: cut(f, rows, tdim - 1) on all interior / all exterior facets."""
    import cutfemx_amd as cfx
    cs, hc = X.build_case(oracle, name), X.host_case(oracle, name, which)
    mesh, V, fs, _ = _engine(cs)
    tdim = cs["tdim"]
    rows = cfx.exterior_facets(mesh) if which == "exterior" else \
        cfx.interior_facets_for_cells(mesh, np.arange(cs["conn"].shape[0], dtype=np.int32))
    assert np.array_equal(rows.rows, hc["rows"])
    cd = cfx.cut(fs[0], rows, tdim - 1)
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), hc["cut"]) and hc["cut"].size > 0
    assert int((~hc["keep"]).sum()) <= 0.05 * hc["cut"].size
    worst = 0.0
    for sel in ("phi<0", "phi>0"):
        ex, alphas = X.exact_volume_moments(f"{name}-{which}", cs["x"], hc["verts"], [cs["phi"]], hc["cut"], sel, 4)
        full, deg = X.whole_moments(tdim - 1, alphas), np.array([sum(a) for a in alphas])
        for order in (1, 2, 3, 4):
            R, names = profiled(lambda: cfx.runtime_quadrature(cd, sel, order))
            assert "facet_emit" in names, sorted(names)
            assert R.tdim == tdim - 1 and np.array_equal(R.host_rows, hc["rows"][R.parent_map])
            got = X.rule_moments(R, alphas, hc["rows"].shape[0])[hc["cut"]] / hc["measure"][:, None]
            err = (np.abs(got - ex) / full)[hc["keep"]][:, deg <= order].max()
            worst = max(worst, err)
            assert err <= TOL, (sel, order, err)
    _report("facet hosts", f"{name} {which}", worst)


# ---- the float32 boundary ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPHERES)
def test_f32_rules_have_the_exact_moments_of_the_widened_inputs(oracle, name):
    """The engine widens float32 inputs exactly, computes in fp64 and rounds points and weights once (to nearest).
    Integer outputs as for fp64.  Moments: a point coordinate and a weight each carry a relative error <= 2^-24, so
    sum(w x^alpha) is within (1 + abs(alpha)) 2^-24 sum(abs(w) abs(x^alpha)); asserted with the factor
    4 + 4 abs(alpha) of the 4-ulp contract of DESIGN 1, on top of the fp64 tolerance.  Weights: each within half a
    float32 ulp of the engine's own fp64 weight for the same widened inputs (which the other tests pin to exact)."""
    import cutfemx_amd as cfx
    cs = X.f32_case(oracle, name)
    tdim, cut = cs["tdim"], cs["cut"]
    mesh = cfx.Mesh.from_arrays(tdim, cs["x32"], cs["conn"])
    cd = cfx.cut(cfx.Function(cfx.FunctionSpace(mesh, 1), cs["phi32"]))
    mesh64, V64, fs64, cd64 = _engine(cs)
    assert cd.dtype == np.float32 and np.array_equal(cd.domain(), cd64.domain())
    assert np.array_equal(np.flatnonzero(cd.domain() == 0), cut)
    vol = X.cell_measures(cs["x"], cs["conn"], tdim)
    worst = 0.0
    for sel in ("phi<0", "phi>0"):
        ex, alphas = X.exact_volume_moments(cs["name"], cs["x"], cs["conn"], [cs["phi"]], cut, sel, 4)
        full, deg = X.whole_moments(tdim, alphas), np.array([sum(a) for a in alphas])
        for order in (1, 2, 4):
            R, R64 = cfx.runtime_quadrature(cd, sel, order), cfx.runtime_quadrature(cd64, sel, order)
            assert R.weights.dtype == np.float32 and R.points.dtype == np.float32
            assert np.array_equal(R.offsets, R64.offsets) and np.array_equal(R.parent_map, R64.parent_map)
            w32, w64 = R.weights.astype(np.float64), R64.weights
            assert np.all(np.abs(w32 - w64) <= 2.0 ** -24 * np.abs(w64) + 2.0 ** -149)
            got = X.rule_moments(R, alphas, cs["conn"].shape[0])[cut] / vol[cut, None]   # weights >= 0: also sum |w x^a|
            assert np.all(R.weights >= 0) and R.points.min() >= 0
            bound = (4 + 4 * deg)[None, :] * 2.0 ** -24 * got + TOL * full[None, :]
            use = deg <= order
            assert np.all(np.abs(got - ex)[:, use] <= bound[:, use]), (sel, order)
            worst = max(worst, (np.abs(got - ex) / full)[:, use].max())
    _report("f32", f"{name} (relative to the whole-cell moment; float32 eps = 6.0e-08)", worst)


# ---- local tensors of every cut cell --------------------------------------------------------------------------------------
def _space(cs, mesh, degree, bs=1):
    import cutfemx_amd as cfx
    dofmap, ndofs = cfx.lagrange_dofmap(cs["tdim"], cs["conn"], cs["x"].shape[0], degree)
    V = cfx.FunctionSpace(mesh, degree, dofmap=None if degree == 1 else dofmap, ndofs=ndofs, bs=bs)
    return V, dofmap, ndofs


def _tensor_worst(cs, name, a, R, kinds, degree):
    import cutfemx_amd as cfx
    tdim = cs["tdim"]
    whole = X.Moments(tdim)
    kept = set(cs["cut"][cs["keep"]].tolist())
    worst, n = 0.0, 0
    # a kept cut cell without a rule has no negative part: its exact tensor is zero
    for c in kept - set(R.parent_map.tolist()):
        assert X.cut_moments(name, cs, c).m[tuple([0] * (tdim + 1))] == 0
    assert np.unique(R.parent_map).size == R.parent_map.size
    for integral, (kind, params) in enumerate(kinds):
        for idx, c in enumerate(R.parent_map):
            if int(c) not in kept:
                continue
            xc = cs["x"][cs["conn"][c], :tdim]
            want = X.tensor(kind, X.cut_moments(name, cs, c), xc, degree, params)
            scale = np.abs(X.tensor(kind, whole, xc, degree, params)).max()
            got = cfx.fem.tabulate_entity(a, integral, idx, True)
            worst = max(worst, np.abs(got - want).max() / scale)
            n += 1
    assert n == len(kinds) * len(kept & set(R.parent_map.tolist())) and n > 0
    return worst


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", TENSOR_CASES)
def test_cut_cell_tensors_are_the_exact_ones(oracle, name, degree):
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, _, _ = _space(cs, mesh, degree)
    R = cfx.runtime_quadrature(cd, "phi<0", 4)
    a = fem.form([fem.Integral(fem.STIFFNESS, rules=R, qdegree=2 * (degree - 1)),
                  fem.Integral(fem.MASS, rules=R, qdegree=2 * degree)], V)
    worst = _tensor_worst(cs, name, a, R, [("stiffness", ()), ("mass", ())], degree)
    _report("tensors", f"{name} P{degree} stiffness + mass", worst)
    assert 0.0 < worst <= TOL


@pytest.mark.parametrize("name", ["3d-n4-sphere", "3d-n4-sphere-scrambled", "2d-n8-sphere"])
def test_cut_cell_elasticity_tensors_are_the_exact_ones(oracle, name):
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, _, _ = _space(cs, mesh, 2, cs["tdim"])
    R = cfx.runtime_quadrature(cd, "phi<0", 2)
    params = (1.0e3, 0.3)
    a = fem.form([fem.Integral(fem.ELASTICITY, rules=R, params=params, qdegree=2)], V)
    worst = _tensor_worst(cs, name, a, R, [("elasticity", params)], 2)
    _report("tensors", f"{name} P2-vector elasticity", worst)
    assert 0.0 < worst <= TOL


# ---- assembled ------------------------------------------------------------------------------------------------------------
def _exact_matrix(cs, name, dofmap, ndofs, bs, terms, degree, inside):
    import scipy.sparse as sp
    M = None
    for kind, params in terms:
        r, c, v = X.exact_entries(name, cs, dofmap, bs, kind, degree, params, inside)
        m = sp.coo_matrix((v, (r, c)), shape=(ndofs * bs, ndofs * bs)).tocsr()
        M = m if M is None else M + m
    return M


def _matrix_err(A, M):
    got = A.to_scipy().tocsr()
    diff = abs(got - M)
    return float(diff.max()) / float(abs(M).max())


def _forms(cs, cd, V, terms, degree, order, with_inside):
    import cutfemx_amd as cfx
    fem = cfx.fem
    R = cfx.runtime_quadrature(cd, "phi<0", order)
    inside = cfx.locate_entities(cd, "phi<0")
    assert np.array_equal(inside, cs["inside"]) and inside.size > 0
    q = {"stiffness": 2 * (degree - 1), "mass": 2 * degree, "elasticity": 2 * (degree - 1)}
    return fem.form([fem.Integral(getattr(fem, KERNEL[k]), cells=inside if with_inside else None, rules=R, params=p,
                                  qdegree=q[k]) for k, p in terms], V)


@pytest.mark.parametrize("mode", ["rows", "atomic"])
@pytest.mark.parametrize("with_inside", [False, True], ids=["rules", "inside+rules"])
@pytest.mark.parametrize("name", ["2d-n8-sphere", "3d-n5-gyroid", "3d-n4-sphere-scrambled"])
def test_assembled_p1_matrix_and_vector_are_exact(oracle, monkeypatch, name, with_inside, mode):
    """P1 stiffness + mass and the source term with f = 1, over the cut-cell rules alone and over [inside cells,
    rules]; row gather (default) and CFX_ASSEMBLY=atomic."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if mode == "atomic":
        monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    cs = X.build_case(oracle, name)
    mesh, V, fs, cd = _engine(cs)
    terms = [("stiffness", ()), ("mass", ())]
    inside = cs["inside"] if with_inside else None
    M = _exact_matrix(cs, name, cs["conn"], cs["x"].shape[0], 1, terms, 1, inside)
    a = _forms(cs, cd, V, terms, 1, 2, with_inside)
    A, names = profiled(lambda: fem.assemble_matrix(a))
    if mode == "atomic":
        assert "assemble_cells_cut" in names or "cut_tensors_p1" in names, sorted(names)
    elif _default_paths():     # the row gather over the staged tensors of the cut cells
        assert "assemble_rows" in names and "cut_tensors_p1" in names and "assemble_cells_cut" not in names, sorted(names)
    ea = _matrix_err(A, M)
    R = cfx.runtime_quadrature(cd, "phi<0", 2)
    L = fem.form([fem.Integral(fem.SOURCE, cells=cs["inside"] if with_inside else None, rules=R,
                               params=(fem.F_ONE, 1.0), qdegree=1)], V)
    b = fem.assemble_vector(L)
    r, v = X.exact_entries(name, cs, cs["conn"], 1, "source", 1, (1.0,), inside)
    want = np.zeros(cs["x"].shape[0])
    np.add.at(want, r, v)
    eb = rel_err(b, want)
    _report("assembled", f"{name} P1 {'inside+rules' if with_inside else 'rules'} {mode}: matrix {ea:.3e} vector", eb)
    assert ea <= TOL and eb <= TOL, (ea, eb)


P2_MODES = {"default": {}, "split": {"CFX_ROWS_SPLIT": "1"}, "split-no-cut-tensors": {"CFX_ROWS_SPLIT": "1", "CFX_P2_CUT_TENSORS": "0"},
            "no-moments": {"CFX_P2_MOMENTS": "0"}, "no-closed": {"CFX_P2_CLOSED": "0"}, "atomic": {"CFX_ASSEMBLY": "atomic"}}


@pytest.mark.parametrize("mode", list(P2_MODES))
@pytest.mark.parametrize("name", ["2d-n8-sphere", "3d-n5-gyroid"])
def test_assembled_p2_stiffness_is_exact(oracle, monkeypatch, name, mode):
    """P2 stiffness over [inside cells, rules] and over the rules alone.  Default: closed-form uncut rows and the 16
    barycentric moments per cut cell (cut_moments_kernel; the profile files it under `assemble_cells_cut`, as it does
    the generic cut tensors that CFX_P2_MOMENTS=0 selects).  CFX_ROWS_SPLIT=1 lets a mesh this small take the split
    rows, where a 3-D form gets one combined tensor per cut cell (cut_tensors_p2; CFX_P2_CUT_TENSORS=0 switches that
    off again).  CFX_P2_CLOSED=0: staged uncut tensors.  CFX_ASSEMBLY=atomic: the entity-parallel kernels."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    default = _default_paths()
    for k, v in P2_MODES[mode].items():
        monkeypatch.setenv(k, v)
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, 2)
    terms = [("stiffness", ())]
    M = _exact_matrix(cs, name, dofmap, ndofs, 1, terms, 2, cs["inside"])
    a = _forms(cs, cd, V, terms, 2, 4, True)
    A, names = profiled(lambda: fem.assemble_matrix(a))
    if default and mode in ("default", "no-moments", "split-no-cut-tensors"):
        assert "assemble_cells_cut" in names and "cut_tensors_p2" not in names and "assemble_cells_std" not in names, sorted(names)
    if default and mode == "split" and cs["tdim"] == 3:
        assert "cut_tensors_p2" in names and "assemble_cells_cut" not in names, sorted(names)
    if default and mode == "no-closed":
        assert "assemble_cells_std" in names and "assemble_cells_cut" in names, sorted(names)
    if default and mode == "atomic":
        assert "assemble_rows" not in names and "assemble_cells_cut" in names, sorted(names)
    err = _matrix_err(A, M)
    _report("assembled", f"{name} P2 stiffness inside+rules {mode} {sorted(names)}", err)
    assert err <= TOL
    # the rules alone
    a2 = _forms(cs, cd, V, terms, 2, 4, False)
    err2 = _matrix_err(fem.assemble_matrix(a2), _exact_matrix(cs, name, dofmap, ndofs, 1, terms, 2, None))
    _report("assembled", f"{name} P2 stiffness rules {mode}", err2)
    assert err2 <= TOL


@pytest.mark.parametrize("mode", ["default", "no-closed", "atomic"])
def test_assembled_p2_vector_elasticity_is_exact(oracle, monkeypatch, mode):
    """P2-vector elasticity over [inside cells, rules] on the 5^3 gyroid: closed-form uncut rows + the 30 x 30 cut
    tensors on the FP64 matrix cores (elasticity_tensors_mfma_cut), and CFX_P2_CLOSED=0, where the uncut cells take
    elasticity_tensors_mfma too: both kernels are compared with the exact matrix."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    default = _default_paths()
    for k, v in {"no-closed": {"CFX_P2_CLOSED": "0"}, "atomic": {"CFX_ASSEMBLY": "atomic"}}.get(mode, {}).items():
        monkeypatch.setenv(k, v)
    name = "3d-n5-gyroid"
    cs = X.build_case(oracle, name)
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, 2, 3)
    terms = [("elasticity", (1.0e3, 0.3))]
    M = _exact_matrix(cs, name, dofmap, ndofs, 3, terms, 2, cs["inside"])
    a = _forms(cs, cd, V, terms, 2, 2, True)
    A, names = profiled(lambda: fem.assemble_matrix(a))
    if default and mode == "default":
        assert "elasticity_tensors_mfma_cut" in names and "elasticity_tensors_mfma" not in names, sorted(names)
    if default and mode == "no-closed":
        assert "elasticity_tensors_mfma_cut" in names and "elasticity_tensors_mfma" in names, sorted(names)
    err = _matrix_err(A, M)
    _report("assembled", f"{name} P2-vector elasticity inside+rules {mode} {sorted(names)}", err)
    assert err <= TOL


# ---- normals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CASES))
def test_interface_normals_are_the_exact_cell_normals(oracle, name):
    """cfx.normal at the interface points = grad phi_h / max(abs(grad phi_h), 1e-14) of the parent cell."""
    import cutfemx_amd as cfx
    cs = X.build_case(oracle, name)
    mesh, V, fs, cd = _engine(cs)
    tdim = cs["tdim"]
    R = cfx.runtime_quadrature(cd, "phi=0", cs["orders"][-1])
    nrm = cfx.normal(cd, R)
    owner = np.repeat(R.parent_map, np.diff(R.offsets))
    ok = np.zeros(cs["conn"].shape[0], dtype=bool)
    ok[cs["cut"][cs["keep_itf"]]] = True
    use = ok[owner]
    want = {c: X.normal(X.cell_phi([cs["phi"]], cs["conn"][c])[0], X.frac_rows(cs["x"][cs["conn"][c], :tdim]))
            for c in np.unique(owner[use])}
    assert len(want) > 0.9 * np.unique(owner).size
    err = np.abs(nrm[use] - np.array([want[c] for c in owner[use]])).max()
    _report("normals", name, err)
    assert err <= TOL
