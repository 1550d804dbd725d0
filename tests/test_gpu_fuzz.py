"""Randomised edge cases against the oracle: level sets with many exact zeros and tiny values at the vertices
(a value == 0 makes the cell intersected, cut.cpp / docs/user-guide/level-sets.md:84-88; sub-simplices of zero
measure must give zero weights, never NaN), on unstructured meshes.  Integers bit-exact, FP64 to 1e-12."""
import numpy as np
import pytest

from helpers import groups_expected, oracle_poisson, profiled, rel_err, scrambled_mesh

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _nasty_level_set(rng, x, tdim):
    base = np.linalg.norm(x[:, :tdim] - 0.5, axis=1) - rng.uniform(0.2, 0.45)
    kind = rng.integers(0, 4, size=base.size)
    phi = base.copy()
    phi[kind == 0] = 0.0                                         # exact zeros on a quarter of the vertices
    phi[kind == 1] *= 1e-13                                      # nearly on the interface
    phi[kind == 2] = np.sign(base[kind == 2]) * rng.uniform(1e-300, 1e-200, size=int((kind == 2).sum()))
    return phi


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("tdim,n", [(2, 7), (3, 4)])
def test_degenerate_level_sets_match_oracle(oracle, tdim, n, seed):
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    O = oracle
    rng = np.random.default_rng(100 * tdim + seed)
    om = scrambled_mesh(O, tdim, n, seed=seed) if seed % 2 else O.mesh_box(tdim, n)
    phi = _nasty_level_set(rng, om.x, tdim)
    ref = oracle_poisson(O, om, phi, order=3)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    assert np.array_equal(cd.domain(), ref["domain"])
    for sel in ("phi<0", "phi=0", "phi>0", "phi<=0", "phi>=0"):
        assert np.array_equal(cfx.locate_entities(cd, sel), O.locate_entities(ref["domain"], sel))
    for sel, want in (("phi<0", ref["vol"]), ("phi=0", ref["itf"]),
                      ("phi>0", O.runtime_quadrature(om, om.conn, phi, ref["domain"], "phi>0", 3))):
        R = cfx.runtime_quadrature(cd, sel, 3)
        assert np.array_equal(R.offsets, want.offsets) and np.array_equal(R.parent_map, want.parent_map)
        assert np.all(np.isfinite(R.weights)) and np.all(R.weights >= 0.0) and np.all(np.isfinite(R.points))
        assert np.max(np.abs(R.weights - want.weights), initial=0.0) <= RTOL * max(np.max(want.weights, initial=0.0), 1e-300)
        assert np.max(np.abs(R.points - want.points), initial=0.0) < 1e-13
    s = poisson.build_forms(V, cd, order=3)
    assert np.array_equal(s.ghost_facets.rows.reshape(-1, 4), ref["ghost"].reshape(-1, 4))
    A = cfx.fem.assemble_matrix(s.a)
    b = cfx.fem.assemble_vector(s.L)
    assert np.array_equal(A.indptr, ref["indptr"]) and np.array_equal(A.indices, ref["indices"])
    assert np.all(np.isfinite(A.data)) and np.all(np.isfinite(b))
    assert rel_err(A.data, ref["values"]) < RTOL and rel_err(b, ref["b"]) < RTOL
    dom = cfx.fem.active_domain(s.a)
    assert np.array_equal(dom.active_cells, ref["active"]) and np.array_equal(dom.inactive_dofs, ref["inactive"])
    # the facets as hosts of the same level set
    orows = O.interior_facets_for_cells(om, np.arange(om.ncells, dtype=np.int32))
    H = O.facet_hosts(om, orows, om.conn)
    fdom = O.facet_classify(H, phi)
    fcd = cfx.cut(cfx.Function(V, phi), orows, tdim - 1)
    assert np.array_equal(fcd.domain(), fdom)
    for sel in ("phi<0", "phi>0", "phi=0"):
        R = cfx.runtime_quadrature(fcd, sel, 2)
        want = O.facet_runtime_quadrature(om, H, phi, fdom, sel, 2)
        assert np.array_equal(R.offsets, want.offsets) and np.array_equal(R.parent_map, want.parent_map)
        assert np.all(np.isfinite(R.weights)) and np.all(R.weights >= 0.0)
        assert np.max(np.abs(R.weights - want.weights), initial=0.0) <= RTOL * max(np.max(want.weights, initial=0.0), 1e-300)
        assert np.max(np.abs(R.points - want.points), initial=0.0) < 1e-13


@pytest.mark.parametrize("tdim,n,degree,bs,margin,mesh_kind", [
    pytest.param(*c, "scrambled" if c[4] is not None else "arrays", id="-".join(map(str, c)))
    for c in [(3, 8, 1, 1, None), (2, 16, 1, 1, None), (3, 5, 2, 1, None), (3, 6, 1, 3, None),
              (3, 40, 1, 1, None), (3, 20, 2, 1, None),
              (3, 8, 1, 1, 0.98), (3, 24, 1, 1, 0.97), (3, 6, 2, 1, 0.98)]] + [
    # forced margins on Kuhn-ordered meshes (from_arrays, generated box, generated slab): void steps on the hex-grouped
    # source term; and a moving sphere at h = 1/128, in the band of its u^7 series
    (3, 12, 1, 1, 0.97, "arrays"), (3, 12, 1, 1, 0.97, "box"), (3, 12, 1, 1, 0.97, "slab"), (3, 128, 1, 1, 0.97, "slab")])
def test_wandering_level_set_in_steps_equals_the_plain_sequence(oracle, tdim, n, degree, bs, margin, mesh_kind):
    """Differential run (tools/soak_fuzz.py is the long form): a level set that wanders, breathes, leaves the mesh and
    swallows it; every step is run as a sync-free step (sizes from the previous step, voided and repeated when they do
    not fit, python/demo/demo_moving_poisson.py:53-90) and as the plain sequence -- the CSR pattern must agree bit for
    bit, values / right-hand side / deactivated rows to 1e-12.  A domain without cells is refused as the reference does
    (deactivate.h:150-155) in both forms."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    fem = cfx.fem
    rng = np.random.default_rng(17 * tdim + n)
    if mesh_kind in ("box", "slab"):
        # generated in HBM (the box table of cfx_mesh_s::hex_corners); the slab: middle layers of the n^3 box
        nz = 4 if n < 64 else 2
        mesh = cfx.Mesh.create_box(tdim, n) if mesh_kind == "box" else cfx.Mesh.create_slab(n, n // 2 - nz // 2, nz)
        x, conn = mesh.x, mesh.conn
    else:
        x, conn = cfx.box_mesh_arrays(tdim, n)
        if mesh_kind == "scrambled":
            # capacities BELOW the previous counts (nearly every speculative pass is void) on a mesh without locality: vertices
            # and cells renumbered at random (tools/soak_fuzz.py seed 31 faulted here: a row-pointer pass over garbage lengths)
            pv = rng.permutation(x.shape[0])
            inv = np.empty_like(pv)
            inv[pv] = np.arange(pv.size)
            x = x[pv]
            conn = np.ascontiguousarray(inv[conn][rng.permutation(conn.shape[0])]).astype(np.int32)
        mesh = cfx.Mesh.from_arrays(tdim, x, conn)
    Vphi = cfx.FunctionSpace(mesh, 1)
    V = Vphi if (degree == 1 and bs == 1) else cfx.FunctionSpace(mesh, degree, bs=bs)
    xt = torch.tensor(x[:, :tdim].copy(), device="cuda")
    phi = torch.empty(x.shape[0], device="cuda", dtype=torch.float64)
    f = cfx.Function(Vphi, phi)

    def one(state):
        if state.get("cd") is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        cd = state["cd"]
        if bs == 1:
            s = poisson.build_forms(V, cd, order=3)
            a, L = s.a, s.L
        else:
            inside = cfx.locate_entities_device(cd, "phi<0")
            vol = cfx.runtime_quadrature(cd, "phi<0", 2)
            ghost = cfx.ghost_penalty_facets(cd, "phi<0")
            ints = [fem.Integral(fem.ELASTICITY, cells=inside, rules=vol, params=(1.0e3, 0.3), qdegree=0)]
            if ghost.size > 0:
                ints.append(fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(5.0,), qdegree=0))
            a, L = fem.form(ints, V), None
        A = fem.create_matrix(a)
        fem.assemble_matrix(a, A=A)
        b = fem.assemble_vector(L) if L is not None else None
        return A, b, fem.deactivate_outside(A, b, fem.active_domain(a))

    key = f"test-fuzz-{tdim}-{n}-{degree}-{bs}-{margin}"
    cfx.forget_step_history(key)
    if margin is not None:
        cfx.set_step_margin(margin, 0)
    sa, sb = {"cd": None}, {"cd": None}
    c, R, compared, refused = np.full(tdim, 0.5), 0.3, 0, 0
    # Kuhn-ordered meshes with forced margins: the group path must run in void and repeated steps, and every 8th accepted
    # step is checked against the oracle as well (an error of a path that both sides take escapes the differential)
    watch = None
    if margin is not None and mesh_kind != "scrambled":
        om = oracle.Mesh(tdim, x, conn)
        watch = {"passes": 0, "groups": 0, "groups_repeated": 0, "oracle": 0}

        def check(i, A1, b1, d1, info, names):
            # (names: the launches of the accepted pass)
            watch["passes"] = max(watch["passes"], info["passes"])
            watch["groups"] += "source_groups" in names
            watch["groups_repeated"] += "source_groups" in names and info["passes"] > 1
            if i % 8 == 0:
                ref = oracle_poisson(oracle, om, phi.cpu().numpy(), order=3)
                vals, bb = ref["values"].copy(), ref["b"].copy()
                oracle.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb)
                assert np.array_equal(A1.indptr, ref["indptr"]) and np.array_equal(A1.indices, ref["indices"]), i
                assert rel_err(A1.data, vals) < RTOL and rel_err(np.asarray(b1), bb) < RTOL, i
                assert np.array_equal(d1.inactive_dofs, ref["inactive"]), i
                watch["oracle"] += 1
    try:
        _wander(cfx, rng, tdim, xt, phi, one, sa, sb, key, c, R, None if watch is None else check)
    finally:
        cfx.set_step_margin()
    if watch is not None:
        import os
        assert watch["oracle"] >= 3, watch
        speculate = os.environ.get("CFX_STEP_SPECULATE") != "0"
        assert watch["passes"] > 1 or not speculate, watch
        assert (watch["groups"] > 0) == groups_expected(), watch
        assert (watch["groups_repeated"] > 0) == (groups_expected() and speculate), watch   # (after a void pass)


def _wander(cfx, rng, tdim, xt, phi, one, sa, sb, key, c, R, check=None):
    import torch
    compared = refused = 0
    for k in range(48):
        c = np.clip(c + rng.normal(0.0, 0.04, tdim) + 0.05 * (0.5 - c), 0.0, 1.0)
        R = float(np.clip(R + rng.normal(0.0, 0.04) + 0.05 * (0.3 - R), 0.05, 0.9))
        if k % 17 == 16:
            R = -0.05          # no domain at all
        if k % 23 == 22:
            R = 2.0            # the whole mesh inside: no cut cell
        phi.copy_(torch.linalg.norm(xt - torch.tensor(c, device="cuda"), dim=1) - R)
        try:
            if check is None:
                A1, b1, d1 = cfx.run_step(lambda: one(sa), key=key)
            else:
                from cutfemx_amd import _lib
                info = {}

                def body():
                    # the profile of the last pass only, the accepted one (a void pass launches the group list too)
                    _lib.check(_lib.lib().cfx_profile_reset())
                    return one(sa)
                (A1, b1, d1), names = profiled(lambda: cfx.run_step(body, key=key, info=info))
        except ValueError as e:
            assert "no active background cells" in str(e) and float(phi.min()) > 0.0, (k, R, str(e))
            with pytest.raises(ValueError, match="no active background cells"):
                one(sb)
            sa, sb = {"cd": None}, {"cd": None}
            cfx.forget_step_history(key)
            refused += 1
            continue
        A2, b2, d2 = one(sb)
        assert A1.nnz == A2.nnz and np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices), (k, R)
        assert rel_err(A1.data, A2.data) < RTOL, (k, R)
        if b1 is not None:
            assert rel_err(np.asarray(b1), np.asarray(b2)) < RTOL, (k, R)
        assert np.array_equal(d1.inactive_dofs, d2.inactive_dofs), (k, R)
        if check is not None:
            check(compared, A1, b1, d1, info, names)
        compared += 1
        del A1, b1, d1, A2, b2, d2
    assert compared >= 24 and refused >= 2, (compared, refused)


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("CFX_FUZZ_SEEDS", "6"))))   # (more seeds: a hunt, not a gate)
@pytest.mark.parametrize("tdim,n,degree", [(3, 9, 1), (2, 26, 1), (3, 6, 2), (2, 14, 2)])
def test_rough_level_sets_match_oracle(oracle, tdim, n, degree, seed):
    """Level sets with many components and features below the mesh size (a sum of random sinusoids: islands, holes, thin
    necks, cells cut next to cells cut) on box and scrambled meshes: the whole cut Poisson system against the oracle --
    classification and located lists bit for bit, rules, ghost facets, CSR pattern bit for bit, values / right-hand side to
    1e-12, active cells and deactivated rows."""
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    O = oracle
    rng = np.random.default_rng(1000 * tdim + 10 * degree + seed)
    om = scrambled_mesh(O, tdim, n, seed=seed) if seed % 2 else O.mesh_box(tdim, n)
    x = om.x[:, :tdim]
    phi = np.full(x.shape[0], rng.uniform(-0.15, 0.15))
    for _ in range(4):
        k = rng.uniform(2.0, 9.0, size=tdim)
        phi += rng.uniform(0.2, 0.5) * np.prod(np.sin(k * x + rng.uniform(0.0, 6.28, size=tdim)), axis=1)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    Vphi = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(Vphi, phi))
    dom = O.classify(om.conn, phi)
    assert np.array_equal(cd.domain(), dom)
    if degree == 1:
        ref = oracle_poisson(O, om, phi, order=3)
        V = Vphi
        s = poisson.build_forms(V, cd, order=3)
        assert np.array_equal(s.ghost_facets.rows.reshape(-1, 4), ref["ghost"].reshape(-1, 4))
        A = cfx.fem.assemble_matrix(s.a)
        b = cfx.fem.assemble_vector(s.L)
        assert np.array_equal(A.indptr, ref["indptr"]) and np.array_equal(A.indices, ref["indices"])
        assert rel_err(A.data, ref["values"]) < RTOL and rel_err(b, ref["b"]) < RTOL
        act = cfx.fem.active_domain(s.a)
        assert np.array_equal(act.active_cells, ref["active"]) and np.array_equal(act.inactive_dofs, ref["inactive"])
        return
    # degree 2 (hashed pattern rows, closed-form rows, moments): stiffness + mass on inside and cut cells + ghost penalty
    dofmap, ndofs = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
    oV = O.Space(dofmap, ndofs, 2, 1)
    V = cfx.FunctionSpace(mesh, 2, dofmap=dofmap, ndofs=ndofs)
    inside = O.locate_entities(dom, "phi<0")
    vol = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 3)
    ghost = O.ghost_penalty_facets(om, dom, "phi<0")
    oint = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=vol, qdegree=2),
            O.Integral(O.CELL, O.K_MASS, entities=inside, rules=vol, qdegree=4)]
    if len(ghost):
        oint.append(O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=ghost, params=(0.1,), qdegree=2))
    ip, ix = O.create_sparsity(om, oV, oint)
    want = O.assemble_matrix(om, oV, oint, ip, ix)
    fem = cfx.fem
    g_in = cfx.locate_entities_device(cd, "phi<0")
    g_vol = cfx.runtime_quadrature(cd, "phi<0", 3)
    g_ghost = cfx.ghost_penalty_facets(cd, "phi<0")
    ints = [fem.Integral(fem.STIFFNESS, cells=g_in, rules=g_vol, qdegree=2), fem.Integral(fem.MASS, cells=g_in, rules=g_vol, qdegree=4)]
    if g_ghost.size > 0:
        ints.append(fem.Integral(fem.GHOST_GRADJUMP, facets=g_ghost, params=(0.1,), qdegree=2))
    A = fem.assemble_matrix(fem.form(ints, V))
    assert np.array_equal(A.indptr, ip) and np.array_equal(A.indices, ix)
    assert rel_err(A.data, want) < RTOL


@pytest.mark.parametrize("tdim,n,margin", [(2, 18, None), (3, 5, None), (3, 5, 0.98), (2, 14, 0.98)])
def test_wandering_dg_system_in_steps_equals_the_plain_sequence(tdim, n, margin):
    """The cut DG system (python/demo/demo_dg_poisson.py: facet-hosted rules, several facet integrals, a space in which
    every active row is an interface row) inside sync-free steps against the plain sequence; with `margin` the capacities
    lie BELOW the previous counts, so that nearly every speculative pass is void.  tools/soak_fuzz.py found two faults
    here: a count read back in mid-step no longer dropped to 0 when the step turned void later (rule points written
    behind their capacity), and the joined facet lists of a form with several facet integrals have an exact length --
    the facet incidence indexed a counter array sized by the capacity of the row lists."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    fem = cfx.fem
    rng = np.random.default_rng(5 * tdim + n)
    x, conn = cfx.box_mesh_arrays(tdim, n)
    mesh = cfx.Mesh.from_arrays(tdim, x, conn)
    Vphi = cfx.FunctionSpace(mesh, 1)
    xt = torch.tensor(x[:, :tdim].copy(), device="cuda")
    phi = torch.empty(x.shape[0], device="cuda", dtype=torch.float64)
    f = cfx.Function(Vphi, phi)

    def one():
        g = poisson.build_dg_forms(f, 1)
        A = fem.assemble_matrix(g.a)
        b = fem.assemble_vector(g.L)
        return A, b, fem.deactivate_outside(A, b, fem.active_domain(g.a))

    key = f"test-fuzz-dg-{tdim}-{n}-{margin}"
    cfx.forget_step_history(key)
    if margin is not None:
        cfx.set_step_margin(margin, 0)
    try:
        c, R, compared = np.full(tdim, 0.5), 0.3, 0
        for k in range(40):
            c = np.clip(c + rng.normal(0.0, 0.04, tdim) + 0.05 * (0.5 - c), 0.0, 1.0)
            R = float(np.clip(R + rng.normal(0.0, 0.04) + 0.05 * (0.3 - R), 0.12, 0.45))
            phi.copy_(torch.linalg.norm(xt - torch.tensor(c, device="cuda"), dim=1) - R)
            try:
                A1, b1, d1 = cfx.run_step(one, key=key)
            except ValueError as e:
                assert "no active background cells" in str(e) and float(phi.min()) > 0.0, (k, R, str(e))
                cfx.forget_step_history(key)
                continue
            A2, b2, d2 = one()
            assert A1.nnz == A2.nnz and np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices), (k, R)
            assert rel_err(A1.data, A2.data) < RTOL and rel_err(np.asarray(b1), np.asarray(b2)) < RTOL, (k, R)
            assert np.array_equal(d1.inactive_dofs, d2.inactive_dofs), (k, R)
            compared += 1
            del A1, b1, d1, A2, b2, d2
        assert compared >= 30, compared
    finally:
        cfx.set_step_margin()
