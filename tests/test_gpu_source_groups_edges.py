"""The hex-grouped P1 source term (vec_source_groups_kernel, cfx_mesh_s::hex_corners) at its edges, b against the
oracle (plain double-precision sin per quadrature point) to 1e-12: the exact / u^7 / u^5 branches of source_vector on
both sides of their thresholds, generated slabs (the box table) against the same arrays through from_arrays (the
checked table), meshes the check must accept or refuse, lists that must or must not take the group path, and a count
resolved in mid-step.  Every test asserts the path it expects (helpers.groups_expected in the diagnostic modes)."""
import os

import numpy as np
import pytest

from helpers import groups_expected, level_set_values, oracle_poisson, profiled, rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _oracle_b(O, om, entities, field, scale, q, rules=None):
    V = O.Space(om.conn, om.nnodes, 1)
    ints = [O.Integral(O.CELL, O.L_SOURCE, entities=entities, params=(field, scale), qdegree=q)]
    if rules is not None:
        ints.insert(0, O.Integral(O.CELL, O.L_SOURCE, rules=rules, params=(field, scale), qdegree=q))
    return O.assemble_vector(om, V, ints)


def _gpu_b(V, cells, field, scale, q, rules=None):
    from cutfemx_amd import fem
    ints = [fem.Integral(fem.SOURCE, cells=cells, params=(field, scale), qdegree=q)]
    if rules is not None:      # a rules-only cell integral first: the uncut entities sit in cell slot 1
        ints.insert(0, fem.Integral(fem.SOURCE, rules=rules, params=(field, scale), qdegree=q))
    L = fem.form(ints, V, rank=1)
    b, names = profiled(lambda: fem.assemble_vector(L))
    return np.asarray(b), names


def _assert_path(names, grouped):
    want = grouped and groups_expected()
    assert ("source_groups" in names) == want, " ".join(sorted(names))
    if want:
        assert "vec_tensors_std" in names and "assemble_vec_plain" in names, " ".join(sorted(names))


def _located(O, om, phi, selector="phi<0"):
    return O.locate_entities(O.classify(om.conn, phi), selector)


# --------------------------------------------------------------------------- A: series branches and thresholds
# umax = pi h picks the branch: > 0.03 exact sinpi, (0.0065, 0.03] the u^7 series, <= 0.0065 the u^5 series.  Only the
# series read the corner-0 sincospi that the group kernel shares across the six tets of a hex.
H_CASES = {
    "exact_above_0.03": 0.03 / np.pi * 1.001,
    "u7_below_0.03": 0.03 / np.pi * 0.999,
    "u7_above_0.0065": 0.0065 / np.pi * 1.001,
    "u5_below_0.0065": 0.0065 / np.pi * 0.999,
    "u5_far": 1.0 / 2048,
}
# box placements: sin(pi x) near 0, near its peak, across x = 1, and a negative offset
OFFSETS = {
    "zero": lambda s: np.array([0.0, 0.0, 0.0]),
    "peak": lambda s: np.full(3, 0.5 - 0.5 * s),
    "one": lambda s: np.full(3, 1.0 - 0.5 * s),
    "negative": lambda s: np.array([-0.61, -1.37, -0.5 * s]),
}


@pytest.mark.parametrize("offset", list(OFFSETS))
@pytest.mark.parametrize("hcase", list(H_CASES))
def test_series_branches_against_oracle(oracle, monkeypatch, hcase, offset):
    import cutfemx_amd as cfx
    O = oracle
    m = 10
    s = H_CASES[hcase] * m
    unit = O.mesh_box(3, m)
    x = unit.x.copy()
    x[:, :3] = OFFSETS[offset](s) + s * unit.x[:, :3]
    om = O.Mesh(3, x, unit.conn)
    phi = np.linalg.norm(unit.x[:, :3] - np.array([0.47, 0.43, 0.41]), axis=1) - 0.38   # plain, odd and cut cells
    inside = _located(O, om, phi)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, "phi<0")
    for fg, fo, scale in ((cfx.fem.F_SINPROD, O.F_SINPROD, 2.5), (cfx.fem.F_POISSON_RHS, O.F_POISSON_RHS, -0.75)):
        for q in (1, 2, 4, 8):
            ref = _oracle_b(O, om, inside, fo, scale, q)
            b1, n1 = _gpu_b(V, cells, fg, scale, q)
            assert rel_err(b1, ref) < RTOL, (fo, q, rel_err(b1, ref))
            _assert_path(n1, True)
            with monkeypatch.context() as mp:
                mp.setenv("CFX_SOURCE_GROUPS", "0")
                b0, n0 = _gpu_b(V, cells, fg, scale, q)
            assert "source_groups" not in n0
            assert rel_err(b0, ref) < RTOL, (fo, q, rel_err(b0, ref))
            assert rel_err(b1, b0) < 1e-13


# --------------------------------------------------------------------------- B: generated slabs
@pytest.mark.parametrize("n,z0,nz", [(12, 0, 1), (12, 11, 1), (13, 4, 3), (9, 2, 5), (128, 60, 2), (512, 255, 1)])
def test_slab_against_oracle_and_from_arrays(oracle, monkeypatch, n, z0, nz):
    """A ball through the whole thickness of the slab: rows on its bottom and top faces are plain, so a corner slot of
    a hex outside the slab in the box table (hex_corners) would add a value that no hex wrote."""
    import cutfemx_amd as cfx
    O = oracle
    slab = cfx.Mesh.create_slab(n, z0, nz)
    om = O.Mesh(3, slab.x, slab.conn)
    zc = (z0 + 0.5 * nz) / n
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.47, 0.43, zc]), axis=1) - 0.31
    inside = _located(O, om, phi)
    ref = _oracle_b(O, om, inside, O.F_POISSON_RHS, 1.25, 4)
    out = {}
    for tag, mesh in (("box", slab), ("arrays", cfx.Mesh.from_arrays(3, om.x, om.conn))):
        V = cfx.FunctionSpace(mesh, 1)
        cd = cfx.cut(cfx.Function(V, phi))
        cells = cfx.locate_entities_device(cd, "phi<0")
        with monkeypatch.context() as mp:
            mp.setenv("CFX_SOURCE_GROUPS", "0")
            b0, n0 = _gpu_b(V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4)
        assert "source_groups" not in n0
        # the corner planes start as NaN: a slot that the fold adds but no hex wrote makes b NaN
        with monkeypatch.context() as mp:
            mp.setenv("CFX_STAGING_NAN", "1")
            b1, n1 = _gpu_b(V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4)
        _assert_path(n1, True)
        assert rel_err(b0, ref) < RTOL, (tag, rel_err(b0, ref))
        assert rel_err(b1, ref) < RTOL, (tag, rel_err(b1, ref))
        assert rel_err(b1, b0) < 1e-13
        out[tag] = b1
    # the box table and the checked table: the same sums, bit for bit (FP64 atomics: in the order of the schedule)
    if os.environ.get("CFX_ASSEMBLY") == "atomic":
        assert rel_err(out["box"], out["arrays"]) < 1e-13
    else:
        assert np.array_equal(out["box"], out["arrays"])


# --------------------------------------------------------------------------- C: what the check accepts or refuses
def _variant(O, kind, m=10, seed=7):
    rng = np.random.default_rng(seed)
    om = O.mesh_box(3, m)
    x, conn = om.x.copy(), om.conn.copy()
    nhex = conn.shape[0] // 6
    if kind == "renumbered":
        p = rng.permutation(x.shape[0])
        xn = np.empty_like(x)
        xn[p] = x
        x, conn = xn, p[conn]
    elif kind == "hexes_permuted":
        conn = conn.reshape(nhex, 6, 4)[rng.permutation(nhex)].reshape(-1, 4)
    elif kind == "moved":
        interior = np.all((x[:, :3] > 1e-12) & (x[:, :3] < 1.0 - 1e-12), axis=1)
        x[interior, :3] += (0.2 / m) * rng.uniform(-1.0, 1.0, size=(int(interior.sum()), 3))
    elif kind == "mirrored":
        x[:, 1] = 1.0 - x[:, 1]
    elif kind == "tets_swapped":
        h = nhex // 2
        conn[[6 * h + 1, 6 * h + 2]] = conn[[6 * h + 2, 6 * h + 1]]
    elif kind == "tet_rotated":
        c = 6 * (nhex // 3) + 4
        conn[c] = np.roll(conn[c], 1)
    elif kind == "last_dropped":
        conn = conn[:-1]
    elif kind == "hex_appended":
        conn = np.vstack([conn, conn[:6]])           # corner k of hex 0 is corner k of a second hex
    else:
        raise ValueError(kind)
    return O.Mesh(3, x, np.ascontiguousarray(conn, dtype=np.int32))


@pytest.mark.parametrize("kind,accepted", [("renumbered", True), ("hexes_permuted", True), ("moved", True),
                                           ("mirrored", True), ("tets_swapped", False), ("tet_rotated", False),
                                           ("last_dropped", False), ("hex_appended", False)])
def test_hex_check_accepts_and_refuses(oracle, kind, accepted):
    import cutfemx_amd as cfx
    O = oracle
    om = _variant(O, kind)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    # the unit-box sphere, and a ball around the origin that holds hex 0 (and its appended copy)
    for phi in (level_set_values(om.x, 3, "sphere"), np.linalg.norm(om.x[:, :3], axis=1) - 0.45):
        cd = cfx.cut(cfx.Function(V, phi))
        for sel in ("phi<0", "phi>0"):
            ref = _oracle_b(O, om, _located(O, om, phi, sel), O.F_SINPROD, 1.0, 4)
            b, names = _gpu_b(V, cfx.locate_entities_device(cd, sel), cfx.fem.F_SINPROD, 1.0, 4)
            assert rel_err(b, ref) < RTOL, (kind, sel, rel_err(b, ref))
            _assert_path(names, accepted)


# --------------------------------------------------------------------------- D: which lists take the group path
def test_lists_take_the_path_their_provenance_allows(oracle):
    import torch

    import cutfemx_amd as cfx
    O = oracle
    om = O.mesh_box(3, 12)
    phi = level_set_values(om.x, 3, "sphere")
    dom = O.classify(om.conn, phi)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    dev = cfx.locate_entities_device(cd, "phi<0")
    host = cfx.locate_entities(cd, "phi<0")
    inside = O.locate_entities(dom, "phi<0")
    assert np.array_equal(host, inside)
    # a prefix that ends inside a hex: its last entity and the next one share a hex
    k = next(i for i in range(host.size // 2, host.size) if host[i - 1] // 6 == host[i] // 6)
    clone = torch.tensor(host, device="cuda")
    outside_dev = cfx.locate_entities_device(cd, "phi>0")
    outside = O.locate_entities(dom, "phi>0")
    assert outside[0] // 6 == 0 and outside[-1] // 6 == om.ncells // 6 - 1   # (it reaches the box faces)
    vol = cfx.runtime_quadrature(cd, "phi<0", 3)
    ovol = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 3)
    cases = [("host", host, inside, False, None, None), ("clone", clone, inside, False, None, None),
             ("prefix", (dev[0], k), inside[:k], False, None, None), ("phi>0", outside_dev, outside, True, None, None),
             ("slot1", dev, inside, True, vol, ovol), ("located", dev, inside, True, None, None)]
    for tag, cells, ent, grouped, rules, orules in cases:
        ref = _oracle_b(O, om, ent, O.F_POISSON_RHS, 0.5, 4, orules)
        b, names = _gpu_b(V, cells, cfx.fem.F_POISSON_RHS, 0.5, 4, rules)
        assert rel_err(b, ref) < RTOL, (tag, rel_err(b, ref))
        _assert_path(names, grouped)


# --------------------------------------------------------------------------- F: a count resolved in mid-step
@pytest.mark.parametrize("where", ["before_matrix", "between"])
@pytest.mark.parametrize("degree", [1, 2])
def test_count_resolved_mid_step(oracle, where, degree):
    """Inside cfx.step the located list's length is in HBM and Count::cap() is its capacity; reading the list back turns
    cap() into the value.  The records of the uncut cells, and the corner planes, must still be written at the stride
    at which they are read, whether the count was resolved before the matrix or between the matrix and the vector."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    O = oracle
    n = 14
    om = O.mesh_box(3, n)
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    Vphi = cfx.FunctionSpace(mesh, 1)
    if degree == 1:
        V, dofmap, ndofs = Vphi, None, None
    else:
        dofmap, ndofs = cfx.lagrange_dofmap(3, om.conn, om.nnodes, 2)
        V = cfx.FunctionSpace(mesh, 2, dofmap=dofmap, ndofs=ndofs)
    xt = torch.tensor(om.x[:, :3].copy(), device="cuda")
    phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
    f = cfx.Function(Vphi, phi)

    def body(state, resolve):
        if state.get("cd") is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        cd = state["cd"]
        s = poisson.build_forms(V, cd, order=4)
        if resolve and where == "before_matrix":
            assert len(cfx.locate_entities(cd, "phi<0")) > 0
        A = cfx.fem.create_matrix(s.a)
        cfx.fem.assemble_matrix(s.a, A=A)
        if resolve and where == "between":
            assert len(cfx.locate_entities(cd, "phi<0")) > 0
        b = np.asarray(cfx.fem.assemble_vector(s.L))
        return A, b

    key = f"test-groups-resolve-{where}-{degree}"
    cfx.forget_step_history(key)
    stepped, grouped = {}, 0
    for k in range(4):
        phi.copy_(torch.linalg.norm(xt - torch.tensor([0.45 + 0.01 * k, 0.47, 0.5], device="cuda", dtype=torch.float64),
                                    dim=1) - (0.3 + 0.004 * k))
        (A1, b1), names = profiled(lambda: cfx.run_step(lambda: body(stepped, True), key=key))
        grouped += "source_groups" in names
        A2, b2 = body({}, False)                          # the plain sequence, on a cut of its own
        assert np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices), k
        assert rel_err(A1.data, A2.data) < RTOL and rel_err(b1, b2) < RTOL, k
        ref = oracle_poisson(O, om, phi.cpu().numpy(), order=4, degree=degree, dofmap=dofmap, ndofs=ndofs)
        assert np.array_equal(A1.indptr, ref["indptr"]) and np.array_equal(A1.indices, ref["indices"]), k
        assert rel_err(A1.data, ref["values"]) < RTOL and rel_err(b1, ref["b"]) < RTOL, (k, rel_err(b1, ref["b"]))
    assert grouped == (4 if degree == 1 and groups_expected() else 0), grouped
