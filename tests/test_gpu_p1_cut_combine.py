"""Degree 1, scalar, bilinear forms: the rule integrals of a cut cell summed in stage 1 into ONE staged tensor per cell,
stored at the cell's host rule (`cut_combine_p1_kernel`; CFX_P1_CUT_COMBINE=0: one tensor per rule and integral, the
path before).  The host rule is the cell's first rule in the lowest cell slot in which it HAS a rule, read from that
slot's hash map (today the rule bits of the cell marks are set by the pass that fills those maps, so the lowest marked
slot is the same slot; the code does not rely on it).

The stage-1 launch keeps its profile name; what tells the two paths apart is the number of launches (one per form
instead of one per rule integral).  The sum is reordered by a handful of FP64 additions, so every comparison takes the
bound the exact tests use, 1e-12 relative to the largest entry.  Linear forms keep one staged vector per rule (the same
sum in their stage 1 cost what their gather saved): their vectors are compared with the
references all the same, with the switch on and off, by cell block and by the row gather (CFX_VEC_BLOCKS=0).
Each test prints its worst value ("COMBINE ..."; run with -s to see them).
"""
import os

import numpy as np
import pytest

import exact_cut as X
from helpers import oracle_poisson, profiled, rel_err
from test_gpu_exact_facets import GAMMA, S3, _coo
from test_gpu_exact_moments import _engine, _matrix_err

pytestmark = pytest.mark.gpu
TOL = 1e-12
# whether the run is in the default mode (tools/test_modes.sh switches single paths off: the results hold, the launch
# counts asserted below are those of the default paths)
PLAIN_ENV = not any(k.startswith("CFX_") and k not in ("CFX_DEVICE", "CFX_COUNT_SYNC", "CFX_STEP_DEBUG") for k in os.environ)
OFF = {"CFX_P1_CUT_COMBINE": "0"}
ROWS = {"CFX_VEC_BLOCKS": "0"}


def _report(what, worst):
    print(f"COMBINE {what}: worst {worst:.3e}")


class _Env:
    """Environment switches for the length of a `with` block (the engine reads them on every call)."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _matrix(a, **env):
    import cutfemx_amd as cfx
    with _Env(**env):
        return profiled(lambda: cfx.fem.assemble_matrix(a))


def _vector(L, **env):
    import cutfemx_amd as cfx
    with _Env(**env):
        return profiled(lambda: np.asarray(cfx.fem.assemble_vector(L)).copy())


def _csr(ref, n):
    import scipy.sparse as sp
    return sp.csr_matrix((ref["values"], ref["indices"], ref["indptr"]), shape=(n, n))


def _same(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def _poisson_reference(oracle, name):
    """The oracle's Poisson system of a case (with the ghost penalty), once per session."""
    cs = X.build_case(oracle, name)
    return X.cached(("combine-poisson", name), lambda: oracle_poisson(oracle, cs["om"], cs["phi"]))


def _poisson_forms(cs):
    """Stiffness over [inside cells, volume rules] + Nitsche, and the linear form of poisson.build_forms."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    fem = cfx.fem
    mesh, V, fs, cd = _engine(cs)
    g = poisson.build_forms(V, cd)
    inside = cfx.locate_entities(cd, "phi<0")
    a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=g.volume_rules, qdegree=0),
                  fem.Integral(fem.NITSCHE, rules=g.interface_rules, point_data=g.normals, params=(GAMMA,))], V)
    return V, g, a


# ---- 1. Poisson, both paths, exact reference -------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_poisson_matrix_and_vector_are_exact_on_both_paths(oracle, monkeypatch, name, split):
    """The matrix against the exact entries, b against the oracle, by default and with the switch off; unsplit
    (`assemble_rows`) and under CFX_ROWS_SPLIT=1 (`assemble_rows_cut`).  The default equals the switch-off result under
    the same bound."""
    if split:
        monkeypatch.setenv("CFX_ROWS_SPLIT", "1")
    cs = X.build_case(oracle, name)
    ref = _poisson_reference(oracle, name)
    V, g, a = _poisson_forms(cs)
    ndofs = cs["x"].shape[0]
    M = _coo(X.exact_entries(name, cs, cs["conn"], 1, "stiffness", 1, (), cs["inside"]), ndofs) + \
        _coo(X.exact_nitsche_entries(name, cs, cs["conn"], 1, GAMMA), ndofs)
    A1, n1 = _matrix(a)
    A0, n0 = _matrix(a, **OFF)
    if PLAIN_ENV:
        assert n1.get("cut_tensors_p1") == 1 and n0.get("cut_tensors_p1") == 2, (n1, n0)
        assert ("assemble_rows_cut" if split else "assemble_rows") in n1, sorted(n1)
    e1, e0 = _matrix_err(A1, M), _matrix_err(A0, M)
    e10 = _matrix_err(A1, A0.to_scipy().tocsr())
    worst = max(e1, e0, e10)
    for env in ({}, ROWS):
        b1, m1 = _vector(g.L, **env)
        b0, m0 = _vector(g.L, **env, **OFF)
        if PLAIN_ENV and env:
            assert "assemble_vec_rows" in m1 and m1 == m0, (m1, m0)
        worst = max(worst, rel_err(b1, ref["b"]), rel_err(b0, ref["b"]), rel_err(b1, b0))
    _report(f"poisson {name} {'split' if split else 'unsplit'} matrix {e1:.3e} off {e0:.3e} on/off {e10:.3e}", worst)
    assert 0.0 < e1 <= TOL and 0.0 < e0 <= TOL and worst <= TOL


# ---- 2. host selection ---------------------------------------------------------------------------------------------
def _two_sphere_case(oracle):
    """Two spheres shifted by about one cell at n = 6: the volume rules of phi_A < 0 and the interface rules of
    phi_B = 0, with the oracle's matrix and vector of the two-set forms."""
    def run():
        n = 6
        om = oracle.mesh_box(3, n)
        phis = [np.linalg.norm(om.x[:, :3] - np.array(c), axis=1) - 0.31
                for c in ((0.47, 0.43, 0.41), (0.47 + 1.0 / n, 0.43, 0.41))]
        doms = [oracle.classify(om.conn, p) for p in phis]
        vol = oracle.runtime_quadrature(om, om.conn, phis[0], doms[0], "phi<0", 4)
        itf = oracle.runtime_quadrature(om, om.conn, phis[1], doms[1], "phi=0", 4)
        nrm = oracle.evaluate_normals(om, om.conn, phis[1], itf)
        V = oracle.Space(om.conn, om.nnodes, 1)
        O = oracle
        a = [O.Integral(O.CELL, O.K_STIFFNESS, rules=vol, qdegree=0),
             O.Integral(O.CELL, O.K_NITSCHE, rules=itf, point_data=nrm, params=(GAMMA,))]
        L = [O.Integral(O.CELL, O.L_SOURCE, rules=vol, params=(O.F_POISSON_RHS, 1.0), qdegree=4),
             O.Integral(O.CELL, O.L_NITSCHE_RHS, rules=itf, point_data=nrm, params=(GAMMA, O.F_SINPROD, 1.0))]
        indptr, indices = O.create_sparsity(om, V, a)
        return dict(om=om, phis=phis, vol=vol, itf=itf, indptr=indptr, indices=indices,
                    values=O.assemble_matrix(om, V, a, indptr, indices), b=O.assemble_vector(om, V, L))
    return X.cached(("combine-two-spheres",), run)


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
def test_the_host_is_the_lowest_slot_that_holds_a_rule(oracle, monkeypatch, split):
    """Stiffness over the rules of one level set, Nitsche over the rules of another: cells with rules in slot 0 only,
    in slot 1 only and in both.  A walk that drops the rules of the other slot shows in the cells of the third kind, a
    record read at a rule that is not the host in all of them."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    if split:
        monkeypatch.setenv("CFX_ROWS_SPLIT", "1")
    ref = _two_sphere_case(oracle)
    om = ref["om"]
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    cda, cdb = (cfx.cut(cfx.Function(V, p.copy())) for p in ref["phis"])
    vol, itf = cfx.runtime_quadrature(cda, "phi<0", 4), cfx.runtime_quadrature(cdb, "phi=0", 4)
    nrm = cfx.normal(cdb, itf)
    pa, pb = set(np.asarray(vol.parent_map).tolist()), set(np.asarray(itf.parent_map).tolist())
    assert pa == set(ref["vol"].parent_map.tolist()) and pb == set(ref["itf"].parent_map.tolist())
    assert len(pa - pb) > 0 and len(pb - pa) > 0 and len(pa & pb) > 0, (len(pa - pb), len(pb - pa), len(pa & pb))
    a = fem.form([fem.Integral(fem.STIFFNESS, rules=vol, qdegree=0),
                  fem.Integral(fem.NITSCHE, rules=itf, point_data=nrm, params=(GAMMA,))], V)
    L = fem.form([fem.Integral(fem.SOURCE, rules=vol, params=(fem.F_POISSON_RHS, 1.0), qdegree=4),
                  fem.Integral(fem.NITSCHE_RHS, rules=itf, point_data=nrm, params=(GAMMA, fem.F_SINPROD, 1.0))], V)
    M = _csr(ref, om.nnodes)
    A1, n1 = _matrix(a)
    A0, n0 = _matrix(a, **OFF)
    if PLAIN_ENV:
        assert n1.get("cut_tensors_p1") == 1 and n0.get("cut_tensors_p1") == 2, (n1, n0)
    e1, e0, e10 = _matrix_err(A1, M), _matrix_err(A0, M), _matrix_err(A1, A0.to_scipy().tocsr())
    worst = max(e1, e0, e10)
    for env in ({}, ROWS):
        b1, m1 = _vector(L, **env)
        b0, m0 = _vector(L, **env, **OFF)
        if PLAIN_ENV and env:
            assert "assemble_vec_rows" in m1 and m1 == m0, (m1, m0)
        worst = max(worst, rel_err(b1, ref["b"]), rel_err(b0, ref["b"]), rel_err(b1, b0))
    _report(f"two spheres {'split' if split else 'unsplit'}: {len(pa - pb)} cells in slot 0 only, {len(pb - pa)} in slot 1 only, "
            f"{len(pa & pb)} in both; matrix {e1:.3e} off {e0:.3e}", worst)
    assert 0.0 < e1 <= TOL and 0.0 < e0 <= TOL and worst <= TOL


# ---- 3. a marked slot without a rule ---------------------------------------------------------------------------------
DEGENERATE = "3d-n4-degenerate"      # vertex values of exactly 0 on cut cells (exact_cut.nasty)


@pytest.mark.parametrize("bulk", [True, False], ids=["bulk-rows", "no-bulk-rows"])
def test_cut_cells_without_a_volume_rule_add_nothing(oracle, monkeypatch, bulk):
    """Vertex values of exactly 0: two thirds of the cut cells of this case have an empty negative part, for which no
    volume rule is emitted (checked on the oracle; such a cell has no interface rule either).  Rows next to them gather
    cut cells that no map holds.  Poisson system against the oracle, marks from the classification and from the
    entity lists."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    if not bulk:
        monkeypatch.setenv("CFX_BULK_ROWS", "0")
    cs = X.build_case(oracle, DEGENERATE)
    ref = _poisson_reference(oracle, DEGENERATE)
    cut = set(np.flatnonzero(ref["domain"] == 0).tolist())
    pv, pi = set(ref["vol"].parent_map.tolist()), set(ref["itf"].parent_map.tolist())
    assert len(cut - pv) > 0 and len(pv) > 0, "the case has no cut cell without a volume rule"
    mesh, V, fs, cd = _engine(cs)
    g = poisson.build_forms(V, cd)
    A1, n1 = _matrix(g.a)
    A0, n0 = _matrix(g.a, **OFF)
    if PLAIN_ENV:
        assert n1.get("cut_tensors_p1") == 1 and n0.get("cut_tensors_p1") == 2, (n1, n0)
    assert np.array_equal(A1.indptr, ref["indptr"]) and np.array_equal(A1.indices, ref["indices"])
    worst = max(rel_err(A1.data, ref["values"]), rel_err(A0.data, ref["values"]))
    for env in ({}, ROWS):
        b1, _ = _vector(g.L, **env)
        b0, _ = _vector(g.L, **env, **OFF)
        worst = max(worst, rel_err(b1, ref["b"]), rel_err(b0, ref["b"]))
    _report(f"cut cells without a volume rule ({'bulk' if bulk else 'entity'} marks): {len(cut - pv)} of {len(cut)}", worst)
    assert 0.0 < worst <= TOL


# ---- 4. fallback ---------------------------------------------------------------------------------------------------
def test_other_forms_keep_the_staging_per_rule(oracle, monkeypatch):
    """A coefficient-weighted rule integral next to Nitsche, a form with one rule-carrying slot, and linear forms: the
    same launches with the switch on and off, bitwise the same values (CFX_DETERMINISTIC=1), equal to the oracle."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    monkeypatch.setenv("CFX_DETERMINISTIC", "1")
    cs = X.build_case(oracle, S3)
    ref = _poisson_reference(oracle, S3)
    om, O = cs["om"], oracle
    V, g, _ = _poisson_forms(cs)
    kappa = 1.0 + 0.5 * np.sin(3.0 * om.x[:, 0]) * np.cos(2.0 * om.x[:, 1])
    Vo = O.Space(om.conn, om.nnodes, 1)
    nitsche_o = O.Integral(O.CELL, O.K_NITSCHE, rules=ref["itf"], point_data=ref["normals"], params=(GAMMA,))
    nitsche = fem.Integral(fem.NITSCHE, rules=g.interface_rules, point_data=g.normals, params=(GAMMA,))
    forms = {
        "weighted": (fem.form([fem.Integral(fem.STIFFNESS, rules=g.volume_rules, qdegree=0, coefficient=kappa), nitsche], V),
                     [O.Integral(O.CELL, O.K_STIFFNESS, rules=ref["vol"], qdegree=0, coefficient=kappa), nitsche_o]),
        "one slot": (fem.form([fem.Integral(fem.STIFFNESS, cells=g.inside_cells, rules=g.volume_rules, qdegree=0)], V),
                     [O.Integral(O.CELL, O.K_STIFFNESS, entities=ref["inside"], rules=ref["vol"], qdegree=0)]),
    }
    for what, (a, ao) in forms.items():
        indptr, indices = O.create_sparsity(om, Vo, ao)
        want = O.assemble_matrix(om, Vo, ao, indptr, indices)
        _matrix(a)      # (the first assembly of a form also builds its row plan)
        A1, n1 = _matrix(a)
        A0, n0 = _matrix(a, **OFF)
        assert n1 == n0, (what, n1, n0)
        if PLAIN_ENV and what == "weighted":
            assert "assemble_cells_cut" in n1 and n1.get("cut_tensors_p1") == 1, n1    # (the generic tensors; Nitsche alone)
        assert _same(A1, A0), what
        assert np.array_equal(A1.indptr, indptr) and np.array_equal(A1.indices, indices)
        err = rel_err(A1.data, want)
        _report(f"fallback, {what}: {sorted(n1)}", err)
        assert 0.0 < err <= TOL
    # ... and the linear forms: a coefficient source next to the Nitsche datum, the Nitsche datum alone, the Poisson one
    w = np.cos(2.0 * om.x[:, 0]) + om.x[:, 2]
    datum = fem.Integral(fem.NITSCHE_RHS, rules=g.interface_rules, point_data=g.normals, params=(GAMMA, fem.F_SINPROD, 1.0))
    datum_o = O.Integral(O.CELL, O.L_NITSCHE_RHS, rules=ref["itf"], point_data=ref["normals"], params=(GAMMA, O.F_SINPROD, 1.0))
    lforms = {
        "coefficient source": (fem.form([fem.Integral(fem.SOURCE, rules=g.volume_rules, params=(fem.F_COEFFICIENT, 1.0),
                                                      coefficient=w), datum], V),
                               [O.Integral(O.CELL, O.L_SOURCE, rules=ref["vol"], params=(O.F_COEFFICIENT, 1.0), coefficient=w),
                                datum_o]),
        "one slot": (fem.form([datum], V), [datum_o]),
        "poisson": (g.L, ref["L"]),
    }
    for what, (L, Lo) in lforms.items():
        want = O.assemble_vector(om, Vo, Lo)
        _vector(L, **ROWS)
        b1, m1 = _vector(L, **ROWS)
        b0, m0 = _vector(L, **ROWS, **OFF)
        assert m1 == m0, (what, m1, m0)
        assert np.array_equal(b1, b0), what
        err = rel_err(b1, want)
        _report(f"fallback, vector, {what}: {sorted(m1)}", err)
        assert 0.0 < err <= TOL


# ---- 5. sync-free step ---------------------------------------------------------------------------------------------
def _step_runs():
    """The benchmark's step sequence inside cutfemx_amd.run_step for three steps of a moving sphere at n = 8, by default
    and with the switch off, and the same steps outside run_step: (passes, read-backs per step) of both, worst
    difference of A and b."""
    def run():
        import ctypes as C

        import torch

        import cutfemx_amd as cfx
        from cutfemx_amd import _lib, poisson
        n = 8
        mesh = cfx.Mesh.create_box(3, n)
        V = cfx.FunctionSpace(mesh, 1)
        xt = torch.tensor(np.asarray(mesh.x)[:, :3].copy(), device="cuda")
        phi = torch.empty(mesh.num_nodes, device="cuda", dtype=torch.float64)
        f = cfx.Function(V, phi)
        values = torch.zeros(40 * mesh.num_nodes + 1000, device="cuda", dtype=torch.float64)
        b = torch.zeros(mesh.num_nodes, device="cuda", dtype=torch.float64)

        def step():      # bench.py: hot_path_step
            cd = cfx.cut(f)
            system = poisson.build_forms(V, cd, order=4)
            _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(b.data_ptr()), 0, C.c_size_t(8 * b.numel())))
            A = cfx.fem.create_matrix(system.a, values=values)
            A.set_value(0.0)
            cfx.fem.assemble_matrix(system.a, A=A)
            cfx.fem.assemble_vector(system.L, b)
            dom = cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(system.a))
            return system, A, dom

        def place(k):
            # (radius 0.38: at n = 8 a sphere of 0.31 leaves no row without a cut cell around it, and a plan without
            # plain rows takes the hashed pattern and the cell blocks, which read sizes back inside a step)
            c = torch.tensor([0.47 + 0.01 * k, 0.49, 0.5], device="cuda", dtype=torch.float64)
            phi.copy_(torch.linalg.norm(xt - c, dim=1) - 0.38)      # in place: the engine aliases this array

        def result(A):
            return A.indptr.copy(), A.indices.copy(), A.data.copy(), b.cpu().numpy().copy()

        out = {"worst": 0.0}
        got = {}
        for mode, env in (("on", {}), ("off", OFF)):
            key = f"test-p1-cut-combine-{mode}"
            cfx.forget_step_history(key)
            passes, syncs, got[mode] = [], [], []
            with _Env(**env):
                for k in range(3):
                    place(k)
                    torch.cuda.synchronize()
                    info = {}
                    s0 = _lib.sync_count()
                    system, A, dom = cfx.run_step(step, key=key, info=info)
                    torch.cuda.synchronize()
                    syncs.append(_lib.sync_count() - s0)
                    passes.append(info["passes"])
                    got[mode].append(result(A))
                    del system, A, dom
            out[mode] = (passes, syncs)
        for k in range(3):      # the same steps, every size read back where it is produced
            place(k)
            system, A, dom = step()
            want = result(A)
            assert np.abs(want[2]).max() > 0.0 and np.abs(want[3]).max() > 0.0
            for mode in got:
                assert np.array_equal(got[mode][k][0], want[0]) and np.array_equal(got[mode][k][1], want[1])
                out["worst"] = max(out["worst"], rel_err(got[mode][k][2], want[2]), rel_err(got[mode][k][3], want[3]))
        return out
    return X.cached(("combine-steps",), run)


def test_the_sync_free_step_is_one_pass_and_adds_no_read_back(oracle):
    """One pass per step, A and b of every step equal to the same step outside run_step, and from the second step on
    (the first also builds the mesh-static tables) as many read-backs as with the switch off."""
    r = _step_runs()
    _report(f"sync-free steps, (passes, read-backs) {r['on']}, switch off {r['off']}", r["worst"])
    assert r["on"][0] == [1, 1, 1] and r["off"][0] == [1, 1, 1], r
    assert r["on"][1][1:] == r["off"][1][1:], r
    assert r["worst"] <= TOL


def test_the_sync_free_step_has_one_read_back_per_step(oracle):
    """One read-back per step from the second step on (the first is sized by read-backs), as the benchmark reports
    for its sizes (`step_mode.read_backs_per_step`)."""
    r = _step_runs()
    if PLAIN_ENV:
        assert all(s == 1 for s in r["on"][1][1:]) and all(s == 1 for s in r["off"][1][1:]), r


# ---- 6. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [X.H_CASE, S3])
def test_two_deterministic_assemblies_are_bitwise_equal(oracle, monkeypatch, name):
    monkeypatch.setenv("CFX_DETERMINISTIC", "1")
    cs = X.build_case(oracle, name)
    V, g, a = _poisson_forms(cs)
    for env in ({}, {"CFX_ROWS_SPLIT": "1"}):
        A1, _ = _matrix(a, **env)
        A2, _ = _matrix(a, **env)
        assert _same(A1, A2), env
    b1, _ = _vector(g.L, **ROWS)
    b2, _ = _vector(g.L, **ROWS)
    assert np.array_equal(b1, b2) and np.abs(b1).max() > 0.0
