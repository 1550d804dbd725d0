"""Plain rows' column indices from one offset row (round 10).  On a generated Kuhn box the stencil of a lattice row
(cfx_space_lattice_rows) is a translate in the numbering too: neighbour k of row r is r + d_k, the same d for every such
row.  The sparsity build then writes the columns of a plain row that is a lattice row and holds its whole stencil as
r + d_k (the streaming role of pattern_plain_tiles_kernel; cfx_space_lattice_pattern_rows counts them) instead of copying
them from the neighbour list, which is what create_sparsity_pattern of cpp/dolfinx_custom_data/fem/assembler.h:567-592
yields for such a row anyway.  Every case: indptr / indices under CFX_LATTICE_PATTERN=2 and CFX_STAGING_NAN=1 (every
index starts as -1, whatever the block cache hands out) equal to the same call under CFX_LATTICE_PATTERN=0 and to the
oracle's create_sparsity, no index -1, and the counter equal to a numpy statement of the rule."""
import os

import numpy as np
import pytest

from helpers import level_set_values, oracle_poisson, rel_err, scrambled_mesh

pytestmark = pytest.mark.gpu
RTOL = 1e-12
ON = {"CFX_LATTICE_PATTERN": "2", "CFX_STAGING_NAN": "1"}
OFF = {"CFX_LATTICE_PATTERN": "0", "CFX_STAGING_NAN": "1"}


def path_expected() -> bool:
    """The diagnostic modes without lattice flags, the row stencil or its tiles: no offset row."""
    e = os.environ.get
    return not (e("CFX_LATTICE_ROWS") == "0" or e("CFX_STENCIL") == "0" or e("CFX_TILES") == "0")


_ORACLE = {}


def oracle_of(O, key, om, phi):
    """The oracle's Poisson system of a case, computed once and left unchanged."""
    if key not in _ORACLE:
        ref = oracle_poisson(O, om, phi)
        vals, bb = ref["values"].copy(), ref["b"].copy()
        O.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb)
        _ORACLE[key] = dict(indptr=ref["indptr"], indices=ref["indices"], values=vals, b=bb)
    return _ORACLE[key]


def top_rows(om):
    """Vertices with the mesh's largest cell count: on a box that is an exact lattice, the flagged rows."""
    n_all = np.bincount(om.conn.ravel(), minlength=om.nnodes)
    return n_all == n_all.max()


def rule_count(lists, indptr, flagged, full_len):
    """The rule in numpy: plain rows of the plan that are flagged and hold their whole stencil."""
    rows = lists["plain_rows"]
    length = np.diff(indptr)[rows]
    return int(np.count_nonzero(flagged[rows] & (length == full_len)))


def poisson_pattern(cfx, mesh, phi, env, monkeypatch, assemble=False):
    """create_matrix of the Poisson system on a NEW space under `env`."""
    from cutfemx_amd import poisson
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        V = cfx.FunctionSpace(mesh(), 1)
        cd = cfx.cut(cfx.Function(V, phi))
        s = poisson.build_forms(V, cd, order=4)
        w0 = V.lattice_pattern_rows()
        A = cfx.fem.create_matrix(s.a)
        taken = V.lattice_pattern_rows() - w0
        lists = s.a.lattice_tile_lists()
        out = dict(indptr=A.indptr.copy(), indices=A.indices.copy(), taken=taken, lists=lists, flagged=V.lattice_rows())
        if assemble:
            cfx.fem.assemble_matrix(s.a, A=A)
            b = cfx.fem.assemble_vector(s.L)
            cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(s.a))
            out["data"] = A.data.copy()
            out["b"] = b.cpu().numpy().copy() if hasattr(b, "cpu") else np.asarray(b).copy()
        return out


def check_pattern(on, off, ref, flagged, full_len, path=True):
    """The common checks; path: the case is meant to write rows from the offset row ("any": as many as the rule says,
    which may be none)."""
    assert off["taken"] == 0
    for r in (on, off):
        assert np.array_equal(r["indptr"], ref["indptr"]) and np.array_equal(r["indices"], ref["indices"])
        assert not np.any(r["indices"] == -1)
    assert np.array_equal(on["indptr"], off["indptr"]) and np.array_equal(on["indices"], off["indices"])
    if path and path_expected():
        assert on["lists"] is not None or path == "any"
        want = rule_count(on["lists"], on["indptr"], flagged, full_len) if on["lists"] is not None else 0
        # (one inline stiffness integral, every plain row inside it: the rule of the values' template is the same rows)
        print(f"pattern rows {on['taken']}, rule {want}, flagged {on['flagged']}, plain rows",
              None if on["lists"] is None else on["lists"]["plain_rows"].size)
        assert on["taken"] == want and (want > 0 or path == "any"), (on["taken"], want)
        assert on["lists"] is None or want == int(on["lists"]["templ"].sum())
    else:
        assert on["taken"] == 0, on["taken"]


@pytest.mark.parametrize("n", [8, 16, 32])
def test_boxes_with_the_benchmark_sphere(oracle, monkeypatch, n):
    """8^3: 8 complete rows inside the sphere, each with a ghost-penalty facet in the Poisson system (no plain row of
    the rule there; the stiffness form of the inside cells has all 8); 16^3, 32^3: tiles in which rows of the rule and
    other plain rows mix, x-lines whose end rows are boundary rows (no lattice rows)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    ref = oracle_of(oracle, ("box", n), om, phi)
    for mesh in (lambda: cfx.Mesh.create_box(3, n), lambda: cfx.Mesh.from_arrays(3, om.x, om.conn)):
        on = poisson_pattern(cfx, mesh, phi, ON, monkeypatch)
        off = poisson_pattern(cfx, mesh, phi, OFF, monkeypatch)
        check_pattern(on, off, ref, top_rows(om), 15, path=True if n > 8 else "any")
        if path_expected():
            assert on["flagged"] == (n - 1) ** 3
    sref = stiffness_ref(oracle, om, phi, oracle.K_STIFFNESS)
    on = one_integral(cfx, n, phi, ON, monkeypatch, fem.STIFFNESS, 0)
    off = one_integral(cfx, n, phi, OFF, monkeypatch, fem.STIFFNESS, 0)
    check_pattern(on, off, sref, top_rows(om), 15)
    for r in (on, off):
        assert rel_err(r["data"], sref["values"]) < RTOL
    if n == 8 and path_expected():
        assert on["taken"] == 8


def test_a_sphere_that_reaches_the_box_faces(oracle, monkeypatch):
    import cutfemx_amd as cfx
    n = 16
    om = oracle.mesh_box(3, n)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.5, 0.5, 0.5]), axis=1) - 0.56
    assert np.any(phi[np.any((om.x < 1e-12) | (om.x > 1 - 1e-12), axis=1)] < 0)
    ref = oracle_of(oracle, ("faces", n), om, phi)
    mesh = lambda: cfx.Mesh.create_box(3, n)
    check_pattern(poisson_pattern(cfx, mesh, phi, ON, monkeypatch), poisson_pattern(cfx, mesh, phi, OFF, monkeypatch), ref,
                  top_rows(om), 15)


def test_a_thin_slab(oracle, monkeypatch):
    """128 x 128 x 2: one plane of complete rows, 127 to an x-line."""
    import cutfemx_amd as cfx
    n, z0, nz = 128, 63, 2
    slab = cfx.Mesh.create_slab(n, z0, nz)
    om = oracle.Mesh(3, slab.x, slab.conn)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.47, 0.43, (z0 + 0.5 * nz) / n]), axis=1) - 0.31
    ref = oracle_of(oracle, ("slab", n), om, phi)
    top = top_rows(om)
    assert int(top.sum()) == (n - 1) ** 2 * (nz - 1)
    mesh = lambda: cfx.Mesh.create_slab(n, z0, nz)
    check_pattern(poisson_pattern(cfx, mesh, phi, ON, monkeypatch), poisson_pattern(cfx, mesh, phi, OFF, monkeypatch), ref,
                  top, 15)


def test_one_moved_vertex_takes_its_rows_off_the_path(oracle, monkeypatch):
    """An interior vertex moved by 0.2 h: itself and its 14 neighbours lose the flag, the counter drops by exactly those
    of them that are complete plain rows."""
    import cutfemx_amd as cfx
    n = 16
    om0 = oracle.mesh_box(3, n)
    x = om0.x.copy()
    v = 6 + (n + 1) * (7 + (n + 1) * 7)
    x[v, 1] += 0.2 / n
    om = oracle.Mesh(3, x, om0.conn)
    phi = level_set_values(om.x, 3)
    assert phi[v] < -0.1
    touched = np.zeros(om.nnodes, dtype=bool)
    touched[om.conn[np.any(om.conn == v, axis=1)].ravel()] = True
    assert int(touched.sum()) == 15
    ref = oracle_of(oracle, ("moved", n), om, phi)
    mesh = lambda: cfx.Mesh.from_arrays(3, om.x, om.conn)
    on = poisson_pattern(cfx, mesh, phi, ON, monkeypatch)
    off = poisson_pattern(cfx, mesh, phi, OFF, monkeypatch)
    check_pattern(on, off, ref, top_rows(om) & ~touched, 15)
    if path_expected():
        assert on["flagged"] == (n - 1) ** 3 - 15
        phi0 = level_set_values(om0.x, 3)
        whole = poisson_pattern(cfx, lambda: cfx.Mesh.from_arrays(3, om0.x, om0.conn), phi0, ON, monkeypatch)
        rows = whole["lists"]["plain_rows"]
        lost = int(np.count_nonzero(touched[rows] & top_rows(om0)[rows] & (np.diff(whole["indptr"])[rows] == 15)))
        assert lost >= 10 and whole["taken"] - on["taken"] == lost, (whole["taken"], on["taken"], lost)


def test_a_square(oracle, monkeypatch):
    """2-D, 16^2: the lattice table serves 2-D (7 columns to a complete row)."""
    import cutfemx_amd as cfx
    n = 16
    om = oracle.mesh_box(2, n)
    phi = level_set_values(om.x, 2)
    ref = oracle_of(oracle, ("square", n), om, phi)
    mesh = lambda: cfx.Mesh.create_box(2, n)
    on = poisson_pattern(cfx, mesh, phi, ON, monkeypatch)
    off = poisson_pattern(cfx, mesh, phi, OFF, monkeypatch)
    check_pattern(on, off, ref, top_rows(om), 7, path=on["flagged"] > 0 and on["lists"] is not None)


def test_a_box_that_is_no_exact_lattice(oracle, monkeypatch):
    """n = 12: no lattice rows (fl(x_o - x_r) differs from row to row), no offset row."""
    import cutfemx_amd as cfx
    n = 12
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    ref = oracle_of(oracle, ("box", n), om, phi)
    mesh = lambda: cfx.Mesh.create_box(3, n)
    check_pattern(poisson_pattern(cfx, mesh, phi, ON, monkeypatch), poisson_pattern(cfx, mesh, phi, OFF, monkeypatch), ref,
                  None, 15, path=False)


def test_a_scrambled_numbering(oracle, monkeypatch):
    """Vertices, cells and local orders renumbered at random: nothing is a translate."""
    import cutfemx_amd as cfx
    sm = scrambled_mesh(oracle, 3, 16)
    phi = level_set_values(sm.x, 3)
    ref = oracle_of(oracle, ("scrambled", 16), sm, phi)
    mesh = lambda: cfx.Mesh.from_arrays(3, sm.x, sm.conn)
    check_pattern(poisson_pattern(cfx, mesh, phi, ON, monkeypatch), poisson_pattern(cfx, mesh, phi, OFF, monkeypatch), ref,
                  None, 15, path=False)


def test_geometry_flags_without_an_index_lattice(oracle, monkeypatch):
    """The 16^3 box with the 27 vertices of a second, far-away component numbered in the middle of its own: the order of
    every neighbour list and every coordinate difference is the box's, so the geometry flags survive, but the rows
    whose stencil straddles the inserted numbers are no translate of the representative's.  One such row switches the
    path off for the space."""
    import cutfemx_amd as cfx
    n = 16
    box, small = oracle.mesh_box(3, n), oracle.mesh_box(3, 2)
    # (behind the representative row, which is the first complete row from row ndofs / 2 on)
    cut_at, extra = box.nnodes // 2 + 300, small.nnodes
    new_id = np.arange(box.nnodes) + np.where(np.arange(box.nnodes) >= cut_at, extra, 0)
    x = np.zeros((box.nnodes + extra, 3))
    x[new_id] = box.x
    x[cut_at:cut_at + extra] = small.x + np.array([4.0, 0.0, 0.0])
    conn = np.concatenate([new_id[box.conn], small.conn + cut_at]).astype(np.int32)
    om = oracle.Mesh(3, x, conn)
    phi = level_set_values(om.x, 3)
    assert np.all(phi[cut_at:cut_at + extra] > 1.0)
    ref = oracle_of(oracle, ("inserted", n), om, phi)
    mesh = lambda: cfx.Mesh.from_arrays(3, om.x, om.conn)
    on = poisson_pattern(cfx, mesh, phi, ON, monkeypatch)
    off = poisson_pattern(cfx, mesh, phi, OFF, monkeypatch)
    if path_expected():
        assert on["flagged"] == (n - 1) ** 3, on["flagged"]
    check_pattern(on, off, ref, None, 15, path=False)


def stiffness_ref(O, om, phi, kernel, bc=None):
    d = O.classify(om.conn, phi)
    oV = O.Space(om.conn, om.nnodes, 1)
    one = [O.Integral(O.CELL, kernel, entities=O.locate_entities(d, "phi<0"), qdegree=0 if kernel == O.K_STIFFNESS else 2)]
    ip, ix = O.create_sparsity(om, oV, one)
    vals = O.assemble_matrix(om, oV, one, ip, ix) if bc is None else O.assemble_matrix(om, oV, one, ip, ix, bc, bc)
    return dict(indptr=ip, indices=ix, values=vals)


def one_integral(cfx, n, phi, env, monkeypatch, kernel, qdegree, bc=None):
    from cutfemx_amd import fem
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        cd = cfx.cut(cfx.Function(V, phi))
        a = fem.form([fem.Integral(kernel, cells=cfx.locate_entities_device(cd, "phi<0"), qdegree=qdegree)], V)
        A = fem.create_matrix(a)
        taken = V.lattice_pattern_rows()
        w0 = V.lattice_template_rows()
        fem.assemble_matrix(a, bcs=bc, A=A)
        return dict(indptr=A.indptr.copy(), indices=A.indices.copy(), data=A.data.copy(), taken=taken,
                    lists=a.lattice_tile_lists(), flagged=V.lattice_rows(), template_rows=V.lattice_template_rows() - w0)


def test_a_form_without_an_inline_stiffness_integral(oracle, monkeypatch):
    """A mass form: no filtered tile list can be built, the full list and the copy run as before."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    n = 16
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    ref = stiffness_ref(oracle, om, phi, oracle.K_MASS)
    on = one_integral(cfx, n, phi, ON, monkeypatch, fem.MASS, 2)
    off = one_integral(cfx, n, phi, OFF, monkeypatch, fem.MASS, 2)
    check_pattern(on, off, ref, None, 15, path=False)
    for r in (on, off):
        assert rel_err(r["data"], ref["values"]) < RTOL


def test_boundary_marks_do_not_concern_the_pattern(oracle, monkeypatch):
    """bc0 / bc1 arrive with assemble_matrix: the pattern takes the path, the values whichever path they take today
    (the tile kernel: marks switch the template off)."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    n = 16
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    bc = np.zeros(om.nnodes, dtype=np.int8)
    bc[::7] = 1
    ref = stiffness_ref(oracle, om, phi, oracle.K_STIFFNESS, bc)
    on = one_integral(cfx, n, phi, ON, monkeypatch, fem.STIFFNESS, 0, bc)
    off = one_integral(cfx, n, phi, OFF, monkeypatch, fem.STIFFNESS, 0, bc)
    check_pattern(on, off, ref, top_rows(om), 15)
    for r in (on, off):
        assert r["template_rows"] == 0
        assert rel_err(r["data"], ref["values"]) < RTOL, rel_err(r["data"], ref["values"])


def test_the_default_refuses_the_path_on_a_small_mesh(oracle, monkeypatch):
    """Without the switch the path is taken from kLatticePatternMinRows = 6 M plain rows on (it is even with the copy at
    128^3 and 256^3): 16^3 has 121."""
    import cutfemx_amd as cfx
    n = 16
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    ref = oracle_of(oracle, ("box", n), om, phi)
    mesh = lambda: cfx.Mesh.create_box(3, n)
    monkeypatch.delenv("CFX_LATTICE_PATTERN", raising=False)
    dflt = poisson_pattern(cfx, mesh, phi, {"CFX_STAGING_NAN": "1"}, monkeypatch)
    off = poisson_pattern(cfx, mesh, phi, OFF, monkeypatch)
    check_pattern(dflt, off, ref, None, 15, path=False)


def test_the_poisson_system_after_assembly(oracle, monkeypatch):
    """32^3, the benchmark's system: values and b against the oracle, and bit for bit with and without the path in
    deterministic mode."""
    import cutfemx_amd as cfx
    n = 32
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    ref = oracle_of(oracle, ("box", n), om, phi)
    mesh = lambda: cfx.Mesh.create_box(3, n)
    split = {"CFX_ROWS_SPLIT": "1"}
    on = poisson_pattern(cfx, mesh, phi, dict(ON, **split), monkeypatch, assemble=True)
    off = poisson_pattern(cfx, mesh, phi, dict(OFF, **split), monkeypatch, assemble=True)
    check_pattern(on, off, ref, top_rows(om), 15)
    for r in (on, off):
        assert rel_err(r["data"], ref["values"]) < RTOL and rel_err(r["b"], ref["b"]) < RTOL
    det = dict(split, CFX_DETERMINISTIC="1")
    det_on = poisson_pattern(cfx, mesh, phi, dict(ON, **det), monkeypatch, assemble=True)
    det_off = poisson_pattern(cfx, mesh, phi, dict(OFF, **det), monkeypatch, assemble=True)
    check_pattern(det_on, det_off, ref, top_rows(om), 15)
    if os.environ.get("CFX_ASSEMBLY") != "atomic":
        assert np.array_equal(det_on["data"], det_off["data"]) and np.array_equal(det_on["b"], det_off["b"])
    assert rel_err(det_on["data"], ref["values"]) < RTOL


@pytest.mark.parametrize("n", [16, 32])
def test_in_steps_with_and_without_forced_overflow(oracle, monkeypatch, n):
    """Eight steps of a sphere moving by 0.3 h, as a plain sequence, as sync-free steps and with capacities forced below
    the previous counts (void steps, repeated): every accepted step has the arrays of the plain sequence under
    CFX_LATTICE_PATTERN=0, and a void pass leaves no HIP error behind."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    steps = 8
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
        return cfx.fem.create_matrix(s.a)

    def loop(tag, margin, in_steps, env):
        with monkeypatch.context() as mp:
            for name, v in env.items():
                mp.setenv(name, v)
            V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
            phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
            f = cfx.Function(V, phi)
            state = {"cd": None}
            key = f"test-lattice-pattern-{n}-{tag}"
            cfx.forget_step_history(key)
            out, passes, syncs = [], [], []
            try:
                if margin is not None:
                    cfx.set_step_margin(margin, 0)
                for k in range(steps):
                    phi.copy_(phi_of(k))
                    info = {"passes": 1}
                    A = cfx.run_step(lambda: body(V, f, state), key=key, info=info) if in_steps else body(V, f, state)
                    passes.append(info["passes"])
                    syncs.append(info.get("read_back"))
                    out.append((A.indptr.copy(), A.indices.copy()))
                    torch.cuda.synchronize()          # (a fault of a void pass would surface here)
            finally:
                cfx.set_step_margin()
            return out, passes, syncs, V.lattice_pattern_rows()

    want, _, _, taken_off = loop("off", None, False, OFF)
    assert taken_off == 0
    for k in (0, steps - 1):
        ref = oracle_poisson(oracle, om, phi_of(k).cpu().numpy())
        assert np.array_equal(want[k][0], ref["indptr"]) and np.array_equal(want[k][1], ref["indices"])
    speculative = os.environ.get("CFX_STEP_SPECULATE") != "0"
    for tag, margin, in_steps in (("plain", None, False), ("steps", None, True), ("forced", 0.97, True)):
        got, passes, syncs, taken = loop(tag, margin, in_steps, ON)
        print(tag, "passes", passes, "read-backs", syncs, "pattern rows", taken)
        assert (taken > 0) == path_expected(), (tag, taken)
        for k in range(steps):
            assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), (tag, k)
            assert not np.any(got[k][1] == -1), (tag, k)
        if tag == "steps" and speculative:
            assert passes[1:] == [1] * (steps - 1), passes
            assert all(s <= 1 for s in syncs[1:]), syncs        # (the arrays are copied out after the step's end)
        if tag == "forced" and speculative:
            assert max(passes) == 2, passes
