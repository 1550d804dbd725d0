"""Lattice rows (round 7): on a background mesh that is an exact lattice, every row of the uncut P1 stiffness matrix whose
incident cells are all entities of one inline integral is the same few numbers -- p1_stiffness_row works from the
differences fl(x_o - x_r) only, and those are bitwise equal from row to row.  The space flags such rows against one
representative row (cfx_space_lattice_rows: equal slot words and bit-equal differences), and the assembly copies them
from the row the deterministic tile kernel computes for the representative instead of running the element loop of
cpp/dolfinx_custom_data/fem/assemble_matrix_impl.h:103-188 over their cells.  Every case: pattern and values against the
oracle, and against the same run with CFX_LATTICE_ROWS=0 -- bit for bit in deterministic mode."""
import os

import numpy as np
import pytest

from helpers import level_set_values, oracle_poisson, rel_err, scrambled_mesh

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def lattice_expected() -> bool:
    """The switch itself, and the diagnostic modes without the row stencil, its tiles or the row gather: no template."""
    e = os.environ
    return not (e.get("CFX_LATTICE_ROWS") == "0" or e.get("CFX_STENCIL") == "0" or e.get("CFX_TILES") == "0"
                or e.get("CFX_ASSEMBLY") == "atomic")


def bitwise() -> bool:
    return os.environ.get("CFX_ASSEMBLY") != "atomic"      # (FP64 atomics: the order of the sums is the schedule's)


def complete_rows_inside(O, om, phi, poisson=False):
    """Per vertex: (all its cells are inside and it has the mesh's largest cell count, it has the largest cell count).
    poisson: ... and no ghost-penalty facet of the Poisson system touches it.  Such a vertex has a facet row, so its
    matrix row belongs to the interface kernel although all its cells are uncut: on the tests' sphere that leaves 0 of
    the 8 complete inside rows at n = 8 and 121 of 223 at n = 16 (the stiffness form alone has all 8 and 223)."""
    d = O.classify(om.conn, phi)
    cell_in = np.zeros(om.conn.shape[0], dtype=bool)
    cell_in[O.locate_entities(d, "phi<0")] = True
    n_all = np.bincount(om.conn.ravel(), minlength=om.nnodes)
    n_in = np.bincount(om.conn[cell_in].ravel(), minlength=om.nnodes)
    top = n_all == n_all.max()
    inside = top & (n_in == n_all)
    if poisson:
        g = np.asarray(O.ghost_penalty_facets(om, d, "phi<0")).reshape(-1, 4)
        touched = np.zeros(om.nnodes, dtype=bool)
        touched[om.conn[g[:, 0]].ravel()] = True
        touched[om.conn[g[:, 2]].ravel()] = True
        inside &= ~touched
    return inside, top


# On meshes this small the interface rows outnumber the others and the assembly would not split the rows into plain
# and interface ones at all: the Poisson cases force the split, as the 512^3 workload has it.
SPLIT = {"CFX_ROWS_SPLIT": "1"}


def stiffness_only(cfx, V, cd):
    from cutfemx_amd import fem
    cells = cfx.locate_entities_device(cd, "phi<0")
    return fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0)], V))


def stiffness_check(O, om, phi):
    d = O.classify(om.conn, phi)
    oV = O.Space(om.conn, om.nnodes, 1)
    one = [O.Integral(O.CELL, O.K_STIFFNESS, entities=O.locate_entities(d, "phi<0"), qdegree=0)]
    ip, ix = O.create_sparsity(om, oV, one)
    want = O.assemble_matrix(om, oV, one, ip, ix)

    def f(r):
        assert np.array_equal(r["indptr"], ip) and np.array_equal(r["indices"], ix)
        assert rel_err(r["data"], want) < RTOL, rel_err(r["data"], want)
    return f


def assemble(cfx, mesh, phi, env, monkeypatch, system=None, eager=True):
    """The Poisson system (or `system(cfx, V, cd)` -> matrix) on a NEW space under `env`: the space decides about its
    lattice table when it builds it -- asked for here before the first form (`eager`), or by the first plan of a
    bilinear form, as an application that never asks for the count has it."""
    from cutfemx_amd import poisson
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        V = cfx.FunctionSpace(mesh(), 1)
        w0 = V.lattice_template_rows() if eager else 0      # (a new space has written no row yet)
        cd = cfx.cut(cfx.Function(V, phi))
        if system is None:
            s = poisson.build_forms(V, cd, order=4)
            A = cfx.fem.create_matrix(s.a)
            cfx.fem.assemble_matrix(s.a, A=A)
            b = cfx.fem.assemble_vector(s.L)
            dom = cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(s.a))
            inactive = dom.inactive_dofs.copy()
        else:
            A, b, inactive = system(cfx, V, cd), None, None
        taken = V.lattice_template_rows() - w0
        flagged = V.lattice_rows()
        return dict(indptr=A.indptr.copy(), indices=A.indices.copy(), data=A.data.copy(), b=b, inactive=inactive,
                    flagged=flagged, taken=taken)


def same(r, q, exact):
    assert np.array_equal(r["indptr"], q["indptr"]) and np.array_equal(r["indices"], q["indices"])
    if exact and bitwise():
        assert np.array_equal(r["data"], q["data"])
    else:
        assert rel_err(r["data"], q["data"]) < 1e-13, rel_err(r["data"], q["data"])


def against_oracle(O, om, phi, r):
    ref = oracle_poisson(O, om, phi)
    vals, bb = ref["values"].copy(), ref["b"].copy()
    O.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb)
    assert np.array_equal(r["indptr"], ref["indptr"]) and np.array_equal(r["indices"], ref["indices"])
    assert rel_err(r["data"], vals) < RTOL and rel_err(r["b"], bb) < RTOL, (rel_err(r["data"], vals), rel_err(r["b"], bb))
    assert np.array_equal(r["inactive"], ref["inactive"])


def check_case(cfx, O, om, phi, mesh, monkeypatch, flagged, taken, system=None, oracle_check=None, env=SPLIT, eager=True):
    """The four runs of a case: default and deterministic, each with the path on and off.  `flagged` may be a
    predicate of the count; `taken` is the count of template rows of a space that has flagged rows."""
    on = assemble(cfx, mesh, phi, dict(env), monkeypatch, system, eager)
    off = assemble(cfx, mesh, phi, dict(env, CFX_LATTICE_ROWS="0"), monkeypatch, system, eager)
    det_on = assemble(cfx, mesh, phi, dict(env, CFX_DETERMINISTIC="1"), monkeypatch, system, eager)
    det_off = assemble(cfx, mesh, phi, dict(env, CFX_DETERMINISTIC="1", CFX_LATTICE_ROWS="0"), monkeypatch, system, eager)
    print(f"lattice rows: flagged {on['flagged']} (expected {flagged}), template rows {on['taken']} (expected {taken}), "
          f"on/off {rel_err(on['data'], off['data']):.2e}, deterministic on/off {rel_err(det_on['data'], det_off['data']):.2e}")
    for r in (on, det_on):
        if lattice_expected():
            if callable(flagged):
                assert flagged(r["flagged"]), r["flagged"]
            else:
                assert r["flagged"] == flagged, (r["flagged"], flagged)
            if callable(taken):
                assert taken(r), (r["taken"], r["flagged"])
            else:
                assert r["taken"] == (taken if r["flagged"] > 0 else 0), (r["taken"], taken)
        else:
            assert r["taken"] == 0
    for r in (off, det_off):
        assert r["flagged"] == 0 and r["taken"] == 0
    for r in (on, off, det_on, det_off):
        (oracle_check or (lambda q: against_oracle(O, om, phi, q)))(r)
    same(det_on, det_off, exact=True)
    same(on, off, exact=False)
    same(on, det_off, exact=False)


@pytest.mark.parametrize("tdim,n", [(3, 8), (3, 16), (2, 32)])
def test_generated_box_and_the_same_arrays(oracle, monkeypatch, tdim, n):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(tdim, n)
    phi = level_set_values(om.x, tdim)
    inside, top = complete_rows_inside(oracle, om, phi)
    plain, _ = complete_rows_inside(oracle, om, phi, poisson=True)
    assert int(top.sum()) == (n - 1) ** tdim
    if tdim == 3:
        assert int(inside.sum()) == {8: 8, 16: 223}[n] and int(plain.sum()) == {8: 0, 16: 121}[n]
    else:
        assert 0 < int(plain.sum()) < int(inside.sum())
    for mesh in (lambda: cfx.Mesh.create_box(tdim, n), lambda: cfx.Mesh.from_arrays(tdim, om.x, om.conn)):
        check_case(cfx, oracle, om, phi, mesh, monkeypatch, (n - 1) ** tdim, int(plain.sum()))
        # the stiffness form of the inside cells alone, unforced: every complete inside row is a template row
        check_case(cfx, oracle, om, phi, mesh, monkeypatch, (n - 1) ** tdim, int(inside.sum()), stiffness_only,
                   stiffness_check(oracle, om, phi), env={})


def test_a_box_that_is_no_exact_lattice_keeps_the_tile_kernel(oracle, monkeypatch):
    """n = 14: the bitwise translates form 343 classes of at most 27 rows -- dropped, or a handful of rows."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 14)
    phi = level_set_values(om.x, 3)
    check_case(cfx, oracle, om, phi, lambda: cfx.Mesh.create_box(3, 14), monkeypatch, lambda f: 0 <= f <= 27,
               lambda r: 0 <= r["taken"] <= r["flagged"])


def test_one_moved_vertex_unflags_its_fifteen_rows(oracle, monkeypatch):
    """The check must look at every cell and every component: one interior vertex moved by 0.2 h changes the rows of
    itself and of its 14 neighbours, nothing else."""
    import cutfemx_amd as cfx
    n = 16
    om0 = oracle.mesh_box(3, n)
    x = om0.x.copy()
    v = 6 + (n + 1) * (7 + (n + 1) * 7)
    assert np.allclose(x[v], np.array([6, 7, 7]) / n)
    x[v, 1] += 0.2 / n
    om = oracle.Mesh(3, x, om0.conn)
    phi = level_set_values(om.x, 3)
    assert phi[v] < -0.1
    touched = np.zeros(om.nnodes, dtype=bool)
    touched[om.conn[np.any(om.conn == v, axis=1)].ravel()] = True
    assert int(touched.sum()) == 15
    inside, top = complete_rows_inside(oracle, om, phi)
    plain, _ = complete_rows_inside(oracle, om, phi, poisson=True)
    assert np.all(inside[touched]) and int(plain[touched].sum()) >= 10    # template rows on the lattice, but for the vertex
    mesh = lambda: cfx.Mesh.from_arrays(3, om.x, om.conn)
    check_case(cfx, oracle, om, phi, mesh, monkeypatch, (n - 1) ** 3 - 15, int((plain & ~touched).sum()))
    check_case(cfx, oracle, om, phi, mesh, monkeypatch, (n - 1) ** 3 - 15, int((inside & ~touched).sum()), stiffness_only,
               stiffness_check(oracle, om, phi), env={})


def test_a_scrambled_mesh_has_no_lattice(oracle, monkeypatch):
    import cutfemx_amd as cfx
    sm = scrambled_mesh(oracle, 3, 8)
    phi = level_set_values(sm.x, 3)
    check_case(cfx, oracle, sm, phi, lambda: cfx.Mesh.from_arrays(3, sm.x, sm.conn), monkeypatch, 0, 0)


def test_forms_that_fall_back(oracle, monkeypatch):
    """The same cells in two inline integrals, boundary marks, and a host copy of the located list: computed rows."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    n = 16
    om = O.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    d = O.classify(om.conn, phi)
    o_in = O.locate_entities(d, "phi<0")
    oV = O.Space(om.conn, om.nnodes, 1)
    bc = np.zeros(om.nnodes, dtype=np.int8)
    bc[::7] = 1
    inside_rows, _ = complete_rows_inside(O, om, phi)

    def twice(cfx, V, cd):
        cells = cfx.locate_entities_device(cd, "phi<0")
        return fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0),
                                             fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0)], V))

    def marked(cfx, V, cd):
        cells = cfx.locate_entities_device(cd, "phi<0")
        return fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0)], V), bcs=bc)

    def host_list(cfx, V, cd):
        cells = cfx.locate_entities(cd, "phi<0")        # a numpy copy: no bulk provenance, the rows are still uniform
        return fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0)], V))

    one = [O.Integral(O.CELL, O.K_STIFFNESS, entities=o_in, qdegree=0)]
    ip, ix = O.create_sparsity(om, oV, one)
    want = {"twice": 2.0 * O.assemble_matrix(om, oV, one, ip, ix), "marked": O.assemble_matrix(om, oV, one, ip, ix, bc, bc),
            "host": O.assemble_matrix(om, oV, one, ip, ix)}

    def check(tag):
        def f(r):
            assert np.array_equal(r["indptr"], ip) and np.array_equal(r["indices"], ix)
            assert rel_err(r["data"], want[tag]) < RTOL, (tag, rel_err(r["data"], want[tag]))
        return f
    mesh = lambda: cfx.Mesh.create_box(3, n)
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, 0, twice, check("twice"), env={})
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, 0, marked, check("marked"), env={})
    # (a list without provenance is marked cell by cell; its complete rows are uniform all the same and take the template)
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, int(inside_rows.sum()), host_list, check("host"), env={})


def test_the_table_and_the_tile_list_built_on_demand(oracle, monkeypatch):
    """Nobody asks the space for its count before the first form: the first plan of a bilinear form builds the table.
    And a linear form over the same cell list, assembled first, builds the shared plan's plain-row masks and the full
    tile list; the bilinear form then finds them there and compacts its filtered tile list on its own
    (cfx::plain_lattice_tiles)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    n = 16
    om = O.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    inside, _ = complete_rows_inside(O, om, phi)
    plain, _ = complete_rows_inside(O, om, phi, poisson=True)
    o_in = O.locate_entities(O.classify(om.conn, phi), "phi<0")
    oV = O.Space(om.conn, om.nnodes, 1)
    want_b = O.assemble_vector(om, oV, [O.Integral(O.CELL, O.L_SOURCE, entities=o_in, params=(O.F_POISSON_RHS, 1.0),
                                                   qdegree=4)])

    def vector_first(cfx, V, cd):
        cells = cfx.locate_entities_device(cd, "phi<0")
        L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_POISSON_RHS, 1.0), qdegree=4)], V)
        a = fem.form([fem.Integral(fem.STIFFNESS, cells=cells, qdegree=0)], V)
        b = fem.assemble_vector(L)                  # (L stays alive: a shares its plan)
        A = fem.assemble_matrix(a)
        bb = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
        assert rel_err(bb, want_b) < RTOL, rel_err(bb, want_b)
        return A
    mesh = lambda: cfx.Mesh.create_box(3, n)
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, int(plain.sum()), eager=False)
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, int(inside.sum()), stiffness_only,
               stiffness_check(O, om, phi), env={}, eager=False)
    check_case(cfx, O, om, phi, mesh, monkeypatch, (n - 1) ** 3, int(inside.sum()), vector_first,
               stiffness_check(O, om, phi), env={}, eager=False)


def test_assembling_twice_adds_the_template_twice(oracle, monkeypatch):
    """Not zeroed in between (not `fresh`): the template rows hold exactly twice their values, and the whole matrix is
    bit for bit what the same two calls give with the path switched off (the interface rows add item by item into what
    is there, so they are twice their values only to rounding, with or without the template)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    n = 16
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    inside, _ = complete_rows_inside(oracle, om, phi, poisson=True)
    monkeypatch.setenv("CFX_DETERMINISTIC", "1")
    monkeypatch.setenv("CFX_ROWS_SPLIT", "1")

    def twice():
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        s = poisson.build_forms(V, cfx.cut(cfx.Function(V, phi)), order=4)
        A = cfx.fem.create_matrix(s.a)
        cfx.fem.assemble_matrix(s.a, A=A)
        once = A.data.copy()
        w0 = V.lattice_template_rows()
        cfx.fem.assemble_matrix(s.a, A=A)                    # added
        return once, A.data.copy(), A.indptr.copy(), V.lattice_template_rows() - w0
    once, both, indptr, taken = twice()
    assert taken == (int(inside.sum()) if lattice_expected() else 0)
    with monkeypatch.context() as mp:
        mp.setenv("CFX_LATTICE_ROWS", "0")
        once0, both0, _, taken0 = twice()
    assert taken0 == 0
    print("entries that are not exactly twice their value:", int(np.count_nonzero(both != 2.0 * once)), "of", both.size,
          "; without the template:", int(np.count_nonzero(both0 != 2.0 * once0)))
    rows = np.flatnonzero(inside)
    entries = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows])
    assert entries.size == 15 * rows.size
    assert rel_err(both, 2.0 * once) < 1e-13
    if bitwise():
        assert np.array_equal(both[entries], 2.0 * once[entries])
        assert np.array_equal(once, once0) and np.array_equal(both, both0)
    else:
        assert rel_err(both, both0) < 1e-13


def test_a_generated_slab(oracle, monkeypatch):
    import cutfemx_amd as cfx
    n, z0, nz = 16, 4, 4
    slab = cfx.Mesh.create_slab(n, z0, nz)
    om = oracle.Mesh(3, slab.x, slab.conn)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.47, 0.43, (z0 + 0.5 * nz) / n]), axis=1) - 0.31
    inside, top = complete_rows_inside(oracle, om, phi)
    plain, _ = complete_rows_inside(oracle, om, phi, poisson=True)
    assert int(top.sum()) == (n - 1) ** 2 * (nz - 1) and int(plain.sum()) > 0
    mesh = lambda: cfx.Mesh.create_slab(n, z0, nz)
    check_case(cfx, oracle, om, phi, mesh, monkeypatch, int(top.sum()), int(plain.sum()))
    check_case(cfx, oracle, om, phi, mesh, monkeypatch, int(top.sum()), int(inside.sum()), stiffness_only,
               stiffness_check(oracle, om, phi), env={})


def test_in_steps_with_and_without_forced_overflow(oracle, monkeypatch):
    """Eight steps of a sphere moving by 0.3 h: every accepted step equals the plain call sequence with the path switched
    off -- to 1e-13 in the default mode, the matrix bit for bit in deterministic mode; with capacities forced below the
    previous counts, steps are void and repeated.  No loop asks the space for its table before the first step: it is
    built by the first plan, inside a (speculative) step where the loop runs in steps."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    n, steps = 16, 8
    monkeypatch.setenv("CFX_ROWS_SPLIT", "1")
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
        A = cfx.fem.create_matrix(s.a)
        cfx.fem.assemble_matrix(s.a, A=A)
        b = cfx.fem.assemble_vector(s.L, state["b"])
        dom = cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(s.a))
        return A, b, dom

    def loop(tag, margin, in_steps, env):
        with monkeypatch.context() as mp:
            for name, v in env.items():
                mp.setenv(name, v)
            V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
            phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
            f = cfx.Function(V, phi)
            state = {"cd": None, "b": torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)}
            key = f"test-lattice-{tag}"
            cfx.forget_step_history(key)
            out, passes = [], []
            try:
                if margin is not None:
                    cfx.set_step_margin(margin, 0)
                for k in range(steps):
                    phi.copy_(phi_of(k))
                    state["b"].zero_()
                    info = {"passes": 1}
                    if in_steps:
                        A, b, dom = cfx.run_step(lambda: body(V, f, state), key=key, info=info)
                    else:
                        A, b, dom = body(V, f, state)
                    passes.append(info["passes"])
                    out.append((A.indptr.copy(), A.indices.copy(), A.data.copy(), b.cpu().numpy().copy(),
                                dom.inactive_dofs.copy()))
            finally:
                cfx.set_step_margin()
            taken = V.lattice_template_rows()            # (a new space: all of them are this loop's)
            assert (taken > 0) == (lattice_expected() and env.get("CFX_LATTICE_ROWS") != "0"), (tag, taken)
            assert (V.lattice_rows() > 0) == (taken > 0)
            return out, passes

    def equal(got, want, exact, what):
        for k in range(steps):
            for i in (0, 1, 4):
                assert np.array_equal(got[k][i], want[k][i]), (what, k, i)
            if exact and bitwise():
                assert np.array_equal(got[k][2], want[k][2]), (what, k)
            else:
                assert rel_err(got[k][2], want[k][2]) < 1e-13, (what, k, rel_err(got[k][2], want[k][2]))
            assert rel_err(got[k][3], want[k][3]) < 1e-13, (what, k)

    OFF, DET = {"CFX_LATTICE_ROWS": "0"}, {"CFX_DETERMINISTIC": "1"}
    plain_off, _ = loop("plain-off", None, False, OFF)
    for k in (0, steps - 1):
        ref = oracle_poisson(oracle, om, phi_of(k).cpu().numpy())
        vals, bb = ref["values"].copy(), ref["b"].copy()
        oracle.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb)
        assert np.array_equal(plain_off[k][0], ref["indptr"]) and np.array_equal(plain_off[k][1], ref["indices"])
        assert rel_err(plain_off[k][2], vals) < RTOL and rel_err(plain_off[k][3], bb) < RTOL
        assert np.array_equal(plain_off[k][4], ref["inactive"])
    plain, _ = loop("plain", None, False, {})
    equal(plain, plain_off, False, "plain")
    det_off, _ = loop("plain-det-off", None, False, dict(OFF, **DET))
    equal(det_off, plain_off, False, "plain-det-off")
    det, _ = loop("plain-det", None, False, DET)
    equal(det, det_off, True, "plain-det")
    for tag, margin in (("steps", None), ("forced", 0.97)):
        for mode, env, want, exact in (("", {}, plain_off, False), ("-det", DET, det_off, True)):
            got, passes = loop(tag + mode, margin, True, env)
            print(tag + mode, "passes", passes)
            if margin is not None and os.environ.get("CFX_STEP_SPECULATE") != "0":
                assert max(passes) == 2, passes      # the shrunk capacities really voided a step, and it was repeated
            equal(got, want, exact, tag + mode)
            equal(got, plain, False, tag + mode + " against the plain sequence")
