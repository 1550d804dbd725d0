"""Closed-form P1 series source term on complete lattice rows (round 8).  On a lattice row r (cfx_space_lattice_rows)
whose cells are all uncut entities of the source integral, every quadrature point of the vertex star sits at x_r + delta
with the deltas of the representative row, and sin(pi (x + delta)) = sin(pi x) cos(pi delta) + cos(pi x) sin(pi delta)
factors the quadrature sum of cpp/dolfinx_custom_data/fem/assemble_vector_impl.h over the star into eight mesh-static
moments T[sigma] times sin / cos of the row's own coordinates.  The fold evaluates that for such rows
(cfx_space_lattice_source_rows counts them), and the hex kernel computes only the hexes with a corner off those rows.

Every case: b against the oracle to 1e-12, against the same call under CFX_LATTICE_SOURCE=0 to 1e-13, and the counter
against the number of eligible rows from the oracle's classification (strictly interior to the mesh, all incident cells
in the entity list).  The grouped calls run with CFX_STAGING_NAN=1: a closed-form row that reads a corner plane, or a
slot of another row that no hex wrote, turns b into NaN.  `moments` / `closed_form` below are the numpy statement of
the formula in extended precision, the independent expectation for the closed-form rows."""
import os

import numpy as np
import pytest

from helpers import groups_expected, level_set_values, oracle_poisson, profiled, rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-12
NAN = {"CFX_STAGING_NAN": "1"}
OFF = {"CFX_LATTICE_SOURCE": "0"}


def closed_expected() -> bool:
    """The group path with lattice flags (helpers.groups_expected, the modes without flags as in test_gpu_lattice_rows)
    and the switch itself."""
    e = os.environ.get
    return groups_expected() and not (e("CFX_LATTICE_ROWS") == "0" or e("CFX_TILES") == "0" or e("CFX_LATTICE_SOURCE") == "0")


def bitwise() -> bool:
    return os.environ.get("CFX_ASSEMBLY") != "atomic"


# --------------------------------------------------------------------------- the formula, in numpy
def reference_rule(O, q):
    """Points and weights (sum 1/6) of the oracle's degree-q rule on the reference tet."""
    x = np.zeros((4, 3))
    x[1, 0] = x[2, 1] = x[3, 2] = 1.0
    r = O.full_cell_rules(O.Mesh(3, x, np.array([[0, 1, 2, 3]], dtype=np.int32)), np.array([0], dtype=np.int32), q)
    w = np.asarray(r.weights, dtype=np.float64)
    return np.asarray(r.points, dtype=np.float64).reshape(-1, 3), w / (6.0 * w.sum())


def moments(x, conn, rstar, pts, w):
    """T[sigma], sigma = sx + 2 sy + 4 sz (bit d: sin(pi delta_d) instead of cos), of the star of vertex rstar."""
    L = np.longdouble
    T = np.zeros(8, dtype=L)
    pi = L(np.pi) + L(1.2246467991473532e-16)          # pi to extended precision: double(pi) + its remainder
    for c in np.flatnonzero(np.any(conn == rstar, axis=1)):
        v = conn[c]
        loc = int(np.flatnonzero(v == rstar)[0])
        d = (x[v, :3] - x[rstar, :3]).astype(L)          # fl(x_v - x_r*), as the flag kernel compares them
        e = d[1:] - d[0]
        det = abs(np.linalg.det(e.astype(np.float64)))
        for X, wq in zip(pts, w):
            N = 1.0 - X.sum() if loc == 0 else X[loc - 1]
            delta = d[0] + X.astype(L) @ e
            sn, cs = np.sin(pi * delta), np.cos(pi * delta)
            for s in range(8):
                t = L(det) * L(wq) * L(N)
                for k in range(3):
                    t = t * (sn[k] if (s >> k) & 1 else cs[k])
                T[s] += t
    return T


def closed_form(T, xr, fscale):
    L = np.longdouble
    pi = L(np.pi) + L(1.2246467991473532e-16)
    S, C = np.sin(pi * xr.astype(L)), np.cos(pi * xr.astype(L))
    out = np.zeros(xr.shape[0], dtype=L)
    for s in range(8):
        t = T[s] * np.ones(xr.shape[0], dtype=L)
        for k in range(3):
            t = t * (C[:, k] if (s >> k) & 1 else S[:, k])
        out += t
    return (L(fscale) * out).astype(np.float64)


def fscale_of(O, field, scale):
    return scale * (3.0 * np.pi * np.pi if field == O.F_POISSON_RHS else 1.0)


def eligible_rows(om, entities):
    """Strictly interior to the mesh, and all incident cells in the entity list."""
    lo, hi = om.x[:, :3].min(axis=0), om.x[:, :3].max(axis=0)
    interior = np.all((om.x[:, :3] > lo) & (om.x[:, :3] < hi), axis=1)
    n_all = np.bincount(om.conn.ravel(), minlength=om.nnodes)
    n_in = np.bincount(om.conn[entities].ravel(), minlength=om.nnodes)
    return interior & (n_in == n_all) & (n_all == n_all.max())


def representative(om):
    """Any row with the largest cell count serves the numpy moments: the flagged rows are translates of each other."""
    n_all = np.bincount(om.conn.ravel(), minlength=om.nnodes)
    start = om.nnodes // 2
    k = np.flatnonzero(np.roll(n_all, -start) == n_all.max())[0]
    return int((start + k) % om.nnodes)


# --------------------------------------------------------------------------- one call
def gpu_b(cfx, V, cells, field, scale, q, env, monkeypatch, rules=None, b=None):
    from cutfemx_amd import fem
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ints = [fem.Integral(fem.SOURCE, cells=cells, params=(field, scale), qdegree=q)]
        if rules is not None:
            ints.insert(0, fem.Integral(fem.SOURCE, rules=rules, params=(field, scale), qdegree=q))
        L = fem.form(ints, V, rank=1)
        w0 = V.lattice_source_rows()
        out, names = profiled(lambda: fem.assemble_vector(L) if b is None else fem.assemble_vector(L, b))
        taken = V.lattice_source_rows() - w0
    return (out.cpu().numpy().copy() if hasattr(out, "cpu") else np.asarray(out).copy()), names, taken


def check_source(cfx, O, om, mesh, phi, monkeypatch, *, selector="phi<0", field="poisson", scale=1.25, q=4,
                 lattice=True, expect=None, grouped=True, proto=True):
    """One source integral over the located list of `selector`: on, off, oracle, counter.  Returns b (on) and count."""
    fg, fo = {"poisson": (cfx.fem.F_POISSON_RHS, O.F_POISSON_RHS), "sinprod": (cfx.fem.F_SINPROD, O.F_SINPROD)}[field]
    ents = O.locate_entities(O.classify(om.conn, phi), selector)
    oV = O.Space(om.conn, om.nnodes, 1)
    ref = O.assemble_vector(om, oV, [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(fo, scale), qdegree=q)])
    elig = eligible_rows(om, ents)
    want = int(elig.sum()) if expect is None else expect
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, selector)
    on, names, taken = gpu_b(cfx, V, cells, fg, scale, q, NAN, monkeypatch)
    off, names0, taken0 = gpu_b(cfx, V, cells, fg, scale, q, dict(NAN, **OFF), monkeypatch)
    print(f"lattice source: rows {taken} (eligible {want}), oracle {rel_err(on, ref):.2e}, on/off {rel_err(on, off):.2e}")
    assert ("source_groups" in names) == (grouped and groups_expected()), " ".join(sorted(names))
    if grouped and groups_expected():
        assert "vec_tensors_std" in names and "assemble_vec_plain" in names, " ".join(sorted(names))
    assert taken0 == 0
    assert taken == (want if lattice and grouped and closed_expected() else 0), (taken, want)
    assert np.all(np.isfinite(on)) and np.all(np.isfinite(off))
    assert rel_err(on, ref) < RTOL and rel_err(off, ref) < RTOL, (rel_err(on, ref), rel_err(off, ref))
    assert rel_err(on, off) < 1e-13, rel_err(on, off)
    if proto and want > 0:
        # the closed-form rows against the numpy statement of the formula: the rounding of the 8-term sum
        pts, w = reference_rule(O, q)
        T = moments(om.x, om.conn, representative(om), pts, w)
        rows = np.flatnonzero(elig)
        cf = closed_form(T, om.x[rows, :3], fscale_of(O, fo, scale))
        top = np.max(np.abs(ref))
        assert np.max(np.abs(cf - ref[rows])) < 1e-13 * top          # the formula itself, against the oracle
        if taken > 0:
            assert np.max(np.abs(on[rows] - cf)) < 2e-15 * top, np.max(np.abs(on[rows] - cf)) / top
    return on, taken, elig


# --------------------------------------------------------------------------- cases
@pytest.mark.parametrize("n", [8, 16, 32])
def test_generated_boxes(oracle, monkeypatch, n):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    _, taken, elig = check_source(cfx, oracle, om, cfx.Mesh.create_box(3, n), phi, monkeypatch)
    if n in (8, 16):
        assert int(elig.sum()) == {8: 8, 16: 223}[n]


def test_the_same_arrays_through_from_arrays(oracle, monkeypatch):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    b_box, t_box, _ = check_source(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch)
    b_arr, t_arr, _ = check_source(cfx, oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), phi, monkeypatch)
    assert t_box == t_arr
    if bitwise():
        assert np.array_equal(b_box, b_arr)
    else:
        assert rel_err(b_box, b_arr) < 1e-13


def test_a_box_that_is_no_exact_lattice(oracle, monkeypatch):
    """n = 20: 1 / 20 is no binary fraction, the differences vary from row to row: no flags, the path is not taken."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 20)
    phi = level_set_values(om.x, 3)
    mesh = cfx.Mesh.create_box(3, 20)
    check_source(cfx, oracle, om, mesh, phi, monkeypatch, lattice=False, proto=False)
    assert cfx.FunctionSpace(mesh, 1).lattice_rows() == 0


@pytest.mark.parametrize("shift", [-0.5, 0.75])
def test_shifted_boxes(oracle, monkeypatch, shift):
    """Negative coordinates, the range across x = 1, and sin(pi x) near 0 on closed-form rows."""
    import cutfemx_amd as cfx
    unit = oracle.mesh_box(3, 16)
    x = unit.x.copy()
    x[:, 0] += shift
    om = oracle.Mesh(3, x, unit.conn)
    phi = level_set_values(unit.x, 3)
    _, taken, elig = check_source(cfx, oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), phi, monkeypatch)
    assert int(elig.sum()) == 223


def test_one_moved_vertex(oracle, monkeypatch):
    """One interior vertex moved by 0.2 h: its 15 rows lose the closed form, the hexes around them become shell, and
    the counter drops by exactly those of them that were eligible."""
    import cutfemx_amd as cfx
    n = 16
    om0 = oracle.mesh_box(3, n)
    x = om0.x.copy()
    v = 6 + (n + 1) * (7 + (n + 1) * 7)
    x[v, 1] += 0.2 / n
    om = oracle.Mesh(3, x, om0.conn)
    phi = level_set_values(om.x, 3)
    touched = np.zeros(om.nnodes, dtype=bool)
    touched[om.conn[np.any(om.conn == v, axis=1)].ravel()] = True
    assert int(touched.sum()) == 15
    ents = oracle.locate_entities(oracle.classify(om.conn, phi), "phi<0")
    elig = eligible_rows(om, ents)
    assert np.all(elig[touched])
    want = int((elig & ~touched).sum())
    assert want == int(elig.sum()) - 15
    # (the numpy moments would need a representative off the moved rows: the on / off / oracle checks carry this case)
    check_source(cfx, oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), phi, monkeypatch, expect=want, proto=False)


def test_inside_reaches_the_box_faces(oracle, monkeypatch):
    """A sphere centred near a box corner: rows on the faces have all their cells inside but are never eligible."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.0, 0.1, 0.0]), axis=1) - 0.7
    _, taken, elig = check_source(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch)
    ents = oracle.locate_entities(oracle.classify(om.conn, phi), "phi<0")
    n_all = np.bincount(om.conn.ravel(), minlength=om.nnodes)
    n_in = np.bincount(om.conn[ents].ravel(), minlength=om.nnodes)
    assert int(((n_in == n_all) & ~elig).sum()) > 0 and int(elig.sum()) > 0


@pytest.mark.parametrize("n,z0", [(128, 60), (512, 255)])
def test_slabs_in_the_series_bands(oracle, monkeypatch, n, z0):
    """n x n x 2 slabs: complete rows on the middle plane, next to shell hexes in the u^7 (128) and u^5 (512) bands."""
    import cutfemx_amd as cfx
    slab = cfx.Mesh.create_slab(n, z0, 2)
    om = oracle.Mesh(3, slab.x, slab.conn)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.47, 0.43, (z0 + 1.0) / n]), axis=1) - 0.31
    _, taken, elig = check_source(cfx, oracle, om, slab, phi, monkeypatch)
    assert int(elig.sum()) > 0


@pytest.mark.parametrize("field,scale", [("sinprod", 2.5), ("poisson", -0.75)])
@pytest.mark.parametrize("q", [1, 2, 4, 8])
def test_functions_scales_and_degrees(oracle, monkeypatch, field, scale, q):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    check_source(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, field=field, scale=scale, q=q)


def test_the_outside_list(oracle, monkeypatch):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    _, taken, elig = check_source(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, selector="phi>0")
    assert int(elig.sum()) > 223


def test_source_integral_in_cell_slot_one(oracle, monkeypatch):
    """A rules-only cell integral first: the uncut entities sit in cell slot 1 (mark bit 2)."""
    import cutfemx_amd as cfx
    O = oracle
    om = O.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    d = O.classify(om.conn, phi)
    ents = O.locate_entities(d, "phi<0")
    o_rules = O.runtime_quadrature(om, om.conn, phi, d, "phi<0", 4)
    oV = O.Space(om.conn, om.nnodes, 1)
    par = (O.F_POISSON_RHS, 1.25)
    ref = O.assemble_vector(om, oV, [O.Integral(O.CELL, O.L_SOURCE, rules=o_rules, params=par, qdegree=4),
                                     O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=par, qdegree=4)])
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, "phi<0")
    rules = cfx.runtime_quadrature(cd, "phi<0", 4)
    on, names, taken = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, NAN, monkeypatch, rules=rules)
    off, _, taken0 = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, dict(NAN, **OFF), monkeypatch, rules=rules)
    assert ("source_groups" in names) == groups_expected()
    assert taken == (223 if closed_expected() else 0) and taken0 == 0
    assert rel_err(on, ref) < RTOL and rel_err(off, ref) < RTOL and rel_err(on, off) < 1e-13


def test_assembling_twice_into_an_unzeroed_vector(oracle, monkeypatch):
    """b += twice: the closed-form rows hold exactly twice their value (the same number is added to itself); the other
    rows add sums into what is there."""
    import torch

    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    elig = eligible_rows(om, oracle.locate_entities(oracle.classify(om.conn, phi), "phi<0"))

    def twice(env):
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
        cd = cfx.cut(cfx.Function(V, phi))
        cells = cfx.locate_entities_device(cd, "phi<0")
        b = torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)
        once, _, t1 = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, env, monkeypatch, b=b)
        both, _, t2 = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, env, monkeypatch, b=b)
        return once, both, t1, t2
    once, both, t1, t2 = twice(NAN)
    once0, both0, z1, z2 = twice(dict(NAN, **OFF))
    want = int(elig.sum()) if closed_expected() else 0
    assert (t1, t2, z1, z2) == (want, want, 0, 0)
    assert np.array_equal(both[elig], 2.0 * once[elig]) or not closed_expected()
    assert rel_err(both, 2.0 * once) < 1e-13 and rel_err(both, both0) < 1e-13 and rel_err(once, once0) < 1e-13
    if bitwise():
        # off the closed-form rows both paths add the same sums in the same order
        assert np.array_equal(once[~elig], once0[~elig]) and np.array_equal(both[~elig], both0[~elig])


def test_without_lattice_flags(oracle, monkeypatch):
    """CFX_LATTICE_ROWS=0 when the space builds its table: no flags, counter 0, today's results."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    monkeypatch.setenv("CFX_LATTICE_ROWS", "0")
    check_source(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, lattice=False, proto=False)


def test_linear_form_first_on_a_fresh_space(oracle, monkeypatch):
    """Nobody asked the space for its lattice table and no bilinear form was planned: the linear form builds it."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    om = O.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    ents = O.locate_entities(O.classify(om.conn, phi), "phi<0")
    ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                            [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(O.F_POISSON_RHS, 1.0), qdegree=4)])
    monkeypatch.setenv("CFX_STAGING_NAN", "1")
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, "phi<0")
    L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_POISSON_RHS, 1.0), qdegree=4)], V)
    b = fem.assemble_vector(L)                           # (first call on the space)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    assert rel_err(b, ref) < RTOL
    assert V.lattice_source_rows() == (223 if closed_expected() else 0)
    # ... and the Poisson system after it, whose matrix takes the template rows from the same table
    from cutfemx_amd import poisson
    A = cfx.fem.assemble_matrix(poisson.build_forms(V, cd, order=4).a)
    assert rel_err(A.data, oracle_poisson(O, om, phi)["values"]) < RTOL


def test_in_steps_with_and_without_forced_overflow(oracle, monkeypatch):
    """Eight steps of a moving sphere at 16^3, the Poisson system's linear form: the plain call sequence, sync-free
    steps and steps with forced overflow margins, each against the oracle, and the three against each other bit for
    bit (the summation order is fixed)."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    n, steps = 16, 8
    om = oracle.mesh_box(3, n)
    xt = torch.tensor(om.x.copy(), device="cuda")

    def phi_of(k):
        c = torch.tensor([0.40 + 0.3 / n * k, 0.45, 0.5], device="cuda", dtype=torch.float64)
        return torch.linalg.norm(xt - c, dim=1) - 0.27

    def body(V, f, state):
        if state.get("cd") is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        s = poisson.build_forms(V, state["cd"], order=4)
        return cfx.fem.assemble_vector(s.L, state["b"])

    def loop(tag, margin, in_steps):
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
        f = cfx.Function(V, phi)
        state = {"cd": None, "b": torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)}
        key = f"test-lattice-source-{tag}"
        cfx.forget_step_history(key)
        out, passes = [], []
        try:
            if margin is not None:
                cfx.set_step_margin(margin, 0)
            for k in range(steps):
                phi.copy_(phi_of(k))
                state["b"].zero_()
                info = {"passes": 1}
                b = cfx.run_step(lambda: body(V, f, state), key=key, info=info) if in_steps else body(V, f, state)
                passes.append(info["passes"])
                out.append(b.cpu().numpy().copy())
        finally:
            cfx.set_step_margin()
        assert (V.lattice_source_rows() > 0) == closed_expected(), tag
        return out, passes

    monkeypatch.setenv("CFX_STAGING_NAN", "1")
    plain, _ = loop("plain", None, False)
    for k in range(steps):
        ref = oracle_poisson(oracle, om, phi_of(k).cpu().numpy())
        assert rel_err(plain[k], ref["b"]) < RTOL, (k, rel_err(plain[k], ref["b"]))
    for tag, margin in (("steps", None), ("forced", 0.97)):
        got, passes = loop(tag, margin, True)
        print(tag, "passes", passes)
        if margin is not None and os.environ.get("CFX_STEP_SPECULATE") != "0":
            assert max(passes) == 2, passes
        for k in range(steps):
            if bitwise():
                assert np.array_equal(got[k], plain[k]), (tag, k)
            else:
                assert rel_err(got[k], plain[k]) < 1e-13, (tag, k)
