"""Functionals on the GPU: rank-0 forms through cfx_assemble_scalar (functional_cells / functional_reduce, and the
rank-0 ending of the registered integrands' wrappers).

Exact references: sums of exactly representable terms compared with `==`; the rational cut-cell moments of
`exact_cut.py` (u_h, u_h^2 and |grad u_h|^2 are polynomials in the reference coordinates of a cell); assembly paths
that are pinned elsewhere (u^T M u, u^T K u, u^T J u); numpy restatements over the downloaded rules.  Tolerance: the
project's 1e-12, relative to the sum over the entities of the absolute exact entity values (per entity: to the same
polynomial with absolute coefficients over the whole cell).  Each test prints its worst value ("FUNCTIONAL ...")."""
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import exact_cut as X
from helpers import level_set_values
from test_functionals import FACET_JUMP_SRC, FIELD_SRC, H1_SRC, L2_SRC, TWO_SPACE_SRC
from test_gpu_exact_facets import _dg_space
from test_gpu_exact_moments import _engine, _space

pytestmark = pytest.mark.gpu
TOL = 1e-12
ROOT = Path(__file__).resolve().parent.parent


def _report(what, worst):
    print(f"FUNCTIONAL {what}: worst {worst:.3e}")


_IDS: dict = {}


def _registered(name):
    """ids of the registered rank-0 integrands of tests/test_functionals.py (one registration per process)"""
    from cutfemx_amd import fem
    if not _IDS:
        _IDS["field"] = fem.register_integrand("user_m_field", FIELD_SRC, rank=0)
        _IDS["l2"] = fem.register_integrand("user_m_l2", L2_SRC, rank=0)
        _IDS["h1"] = fem.register_integrand("user_m_h1", H1_SRC, rank=0)
        _IDS["jump"] = fem.register_integrand("user_m_jump", FACET_JUMP_SRC, rank=0, facet=True)
        _IDS["two"] = fem.register_integrand("user_m_two", TWO_SPACE_SRC, rank=0, variant=(2, 3, 1),
                                             coefficients=[(3, 1), (6, 1)])
    return _IDS[name]


# ---- polynomials in the reference coordinates: {exponents (tdim): coefficient} ----------------------------------------
def _pmul(p, q):
    out = {}
    for (a, ca), (b, cb) in itertools.product(p.items(), q.items()):
        k = tuple(x + y for x, y in zip(a, b))
        out[k] = out.get(k, 0.0) + ca * cb
    return out


def _padd(p, q, s=1.0):
    out = dict(p)
    for k, v in q.items():
        out[k] = out.get(k, 0.0) + s * v
    return out


def _pdiff(p, t):
    out = {}
    for a, c in p.items():
        if a[t] > 0:
            k = tuple(e - (1 if i == t else 0) for i, e in enumerate(a))
            out[k] = out.get(k, 0.0) + c * a[t]
    return out


def _basis(tdim, degree):
    """the Lagrange basis as polynomials, dof order of the engine (vertices, then the edges in Basix order)"""
    zero = tuple([0] * tdim)
    lam = [{zero: 1.0}] + [{tuple(1 if i == t else 0 for i in range(tdim)): 1.0} for t in range(tdim)]
    for t in range(tdim):
        lam[0] = _padd(lam[0], lam[t + 1], -1.0)
    if degree == 1:
        return lam
    N = [_padd(_pmul(l, l), l, -0.5) for l in lam]
    N = [{k: 2.0 * v for k, v in p.items()} for p in N]
    N += [{k: 4.0 * v for k, v in _pmul(lam[a], lam[b]).items()} for a, b in X.EDGES[tdim]]
    return N


def _function_poly(N, u, bs=1, comp=0):
    p = {}
    for j, Nj in enumerate(N):
        p = _padd(p, Nj, float(u[j * bs + comp]))
    return p


def _integrand_polys(tdim, degree, xc, u, bs=1):
    """the four integrands on one cell as polynomials: 1, u_h, |u_h|^2, |grad u_h|^2 (summed over the components)"""
    N = _basis(tdim, degree)
    zero = tuple([0] * tdim)
    J = (xc[1:, :tdim] - xc[0, :tdim]).T          # J[d][t]
    K = np.linalg.inv(J)                          # K[t][d]
    sq, h1 = {}, {}
    for b in range(bs):
        ub = _function_poly(N, u, bs, b)
        sq = _padd(sq, _pmul(ub, ub))
        dX = [_pdiff(ub, t) for t in range(tdim)]
        for d in range(tdim):
            g = {}
            for t in range(tdim):
                g = _padd(g, dX[t], float(K[t, d]))
            h1 = _padd(h1, _pmul(g, g))
    return {"one": {zero: 1.0}, "u": _function_poly(N, u, bs, 0), "u2": sq, "h1": h1}


def _apply(poly, moments, index):
    """(sum_a c_a m_a, sum_a |c_a| m_a) for the moment row `moments` indexed by (0,) + exponents"""
    v = sum(c * moments[index[(0,) + a]] for a, c in poly.items())
    s = sum(abs(c) * abs(moments[index[(0,) + a]]) for a, c in poly.items())
    return float(v), float(s)


KINDS = ("one", "u", "u2", "h1")


def _forms(fem, V, u, measure, qdegree):
    """the four built-in functionals over one measure (keyword arguments of Integral)"""
    return {"one": fem.form([fem.Integral(fem.M_FIELD, params=(fem.F_ONE, 1.0), qdegree=qdegree, **measure)], V),
            "u": fem.form([fem.Integral(fem.M_FIELD, params=(fem.F_COEFFICIENT, 1.0), qdegree=qdegree, coefficient=u, **measure)], V),
            "u2": fem.form([fem.Integral(fem.M_L2_DIFF, params=(fem.F_ONE, 1.0, 0.0), qdegree=qdegree, coefficient=u, **measure)], V),
            "h1": fem.form([fem.Integral(fem.M_H1_SEMI, params=(0, 1.0), qdegree=qdegree, coefficient=u, **measure)], V)}


def _exact_cells(cs, name, degree, dofmap, u, order):
    """per cell and kind (value, scale): the inside cells, the phi<0 part and the phi=0 part of every cut cell"""
    tdim, x, conn, cut = cs["tdim"], cs["x"], cs["conn"], cs["cut"]
    mdeg = 2 * degree
    exv, alphas = X.exact_volume_moments(name, x, conn, [cs["phi"]], cut, "phi<0", mdeg)
    exi, _ = X.exact_interface_moments(name, x, conn, [cs["phi"]], cut, "phi=0", mdeg)
    index = {a: k for k, a in enumerate(alphas)}
    full, vol = X.whole_moments(tdim, alphas), X.cell_measures(x, conn, tdim)
    hs = X.interface_scale(x, conn, cut, tdim)
    inside, vcut, icut = {}, {}, {}
    for c in cs["inside"]:
        P = _integrand_polys(tdim, degree, x[conn[c]], u[dofmap[c]])
        inside[int(c)] = {k: tuple(vol[c] * t for t in _apply(P[k], full, index)) for k in KINDS}
    for r, c in enumerate(cut):
        P = _integrand_polys(tdim, degree, x[conn[c]], u[dofmap[c]])
        vcut[int(c)] = {k: (vol[c] * _apply(P[k], exv[r], index)[0], vol[c] * _apply(P[k], full, index)[1]) for k in KINDS}
        icut[int(c)] = {k: (_apply(P[k], exi[r], index)[0], hs[r] * _apply(P[k], full, index)[1]) for k in KINDS}
    return inside, vcut, icut


# ---- 1. reduction edges: exact equality ------------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512]


def test_reduction_edges_are_exact():
    """512 triangles with dyadic vertices, the one-point rule (weight exactly 1/2): every cell adds exactly 2^-9, so any
    order of the sum gives k / 512 -- a lane, wave, block or slab offset that is lost or counted twice shows as an
    inequality."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    fem = cfx.fem
    mesh = cfx.Mesh.create_box(2, 16)
    assert mesh.num_cells == 512
    V = cfx.FunctionSpace(mesh, 1)
    perm = np.random.default_rng(7).permutation(512).astype(np.int32)
    kf = _registered("field")
    one = dict(params=(fem.F_ONE, 1.0), qdegree=1)
    dev = torch.full((1,), -1.0, device="cuda", dtype=torch.float64)
    for k in LENGTHS:
        cells = perm[:k]
        M = fem.form([fem.Integral(fem.M_FIELD, cells=cells, **one)], V, rank=0)
        v = fem.assemble_scalar(M)
        assert v == k / 512, (k, v)
        assert fem.assemble_scalar(M) == v                                  # the same bits again
        # three integrals of one form: consecutive offsets in the slab of partials
        a, b = k // 3, (2 * k) // 3
        M3 = fem.form([fem.Integral(fem.M_FIELD, cells=cells[lo:hi], **one) for lo, hi in ((0, a), (a, b), (b, k))], V, rank=0)
        assert fem.assemble_scalar(M3) == k / 512, k
        Mu = fem.form([fem.Integral(kf, cells=cells, **one)], V, rank=0)     # the registered wrapper's block sum
        assert fem.assemble_scalar(Mu) == k / 512, k
        s0 = _lib.sync_count()
        out = fem.assemble_scalar(M, out=dev)
        assert _lib.sync_count() == s0 and out is dev                        # no host round trip for a device value
        assert float(dev.cpu()[0]) == k / 512
        if k:
            assert fem.tabulate_entity(M, 0, k - 1, False).tolist() == [2.0 ** -9]
            assert fem.tabulate_entity(Mu, 0, 0, False).tolist() == [2.0 ** -9]
    M0 = fem.form([], V, rank=0)                                            # no integral: the functional 0
    assert fem.assemble_scalar(M0) == 0.0


# ---- 2. exact values on cut domains ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", [("2d-n8-sphere", 1), ("3d-n4-sphere", 1), ("3d-n4-sphere-scrambled", 1),
                                         ("3d-n5-gyroid", 1), ("2d-n8-sphere", 2)])
def test_functionals_on_cut_domains_are_the_exact_ones(oracle, name, degree):
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    assert cs["keep"].all() and cs["keep_itf"].all()      # no all-zero cell: the sums are free of the ownership convention
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, degree)
    u = np.random.default_rng(5).uniform(-1.0, 1.0, ndofs)
    inside = cfx.locate_entities(cd, "phi<0")
    assert np.array_equal(inside, cs["inside"])
    Rv, Ri = cfx.runtime_quadrature(cd, "phi<0", 4), cfx.runtime_quadrature(cd, "phi=0", 4)
    ex_in, ex_v, ex_i = _exact_cells(cs, name, degree, dofmap, u, 4)
    worst = 0.0
    for label, measure, parts in (("volume", dict(cells=inside, rules=Rv), (ex_in, ex_v)), ("interface", dict(rules=Ri), (ex_i,))):
        forms = _forms(fem, V, u, measure, 2 * degree)
        for kind in KINDS:
            want = sum(p[c][kind][0] for p in parts for c in p)
            scale = sum(abs(p[c][kind][0]) for p in parts for c in p)
            got = fem.assemble_scalar(forms[kind])
            err = abs(got - want) / scale
            worst = max(worst, err)
            assert err <= TOL, (label, kind, got, want, err)
    _report(f"{name} P{degree} cut domains", worst)
    assert worst > 0.0


# ---- 3. per entity on degenerate inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d-n4-degenerate", "2d-n7-degenerate-scrambled"])
def test_entity_values_on_degenerate_inputs_are_the_exact_ones(oracle, name):
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, name)
    for keep in (cs["keep"], cs["keep_itf"]):
        assert int((~keep).sum()) <= 0.05 * cs["cut"].size          # what exact_cut.CASES was seeded for
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _space(cs, mesh, 1)
    u = np.random.default_rng(6).uniform(-1.0, 1.0, ndofs)
    ex_in, ex_v, ex_i = _exact_cells(cs, name, 1, dofmap, u, 4)
    worst, n = 0.0, 0
    for sel, ex, keep in (("phi<0", ex_v, cs["keep"]), ("phi=0", ex_i, cs["keep_itf"])):
        R = cfx.runtime_quadrature(cd, sel, 4)
        forms = _forms(fem, V, u, dict(rules=R), 2)
        kept = set(cs["cut"][keep].tolist())
        for kind in KINDS:
            got = {}
            for idx, c in enumerate(R.parent_map):      # (a 3-D cell may have two interface rules: their sum)
                got[int(c)] = got.get(int(c), 0.0) + float(fem.tabulate_entity(forms[kind], 0, idx, True)[0])
            for c in kept:
                want, scale = ex[c][kind]
                if c not in got:
                    assert abs(want) <= TOL * scale     # a kept cell without a rule: a part without measure
                    continue
                worst = max(worst, abs(got[c] - want) / scale)
                n += 1
    _report(f"{name} entity values ({n})", worst)
    assert n > 0 and 0.0 < worst <= TOL


# ---- 4. identities against assembly paths that are pinned elsewhere ---------------------------------------------------
def _quadratic(A, u):
    """(u^T A u, sum |u_i A_ij u_j|)"""
    rows = np.repeat(np.arange(A.nrows), np.diff(A.indptr))
    t = u[rows] * A.data * u[A.indices]
    return float(t.sum()), float(np.abs(t).sum())


@pytest.mark.parametrize("tdim,n,degree,bs", [(3, 5, 1, 1), (2, 10, 2, 1), (2, 10, 1, 2)])
def test_norms_equal_the_quadratic_forms_of_mass_and_stiffness(tdim, n, degree, bs):
    import cutfemx_amd as cfx
    fem = cfx.fem
    mesh = cfx.Mesh.create_box(tdim, n)
    V1 = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V1, level_set_values(mesh.x, tdim)))
    V = cfx.FunctionSpace(mesh, degree, bs=bs)
    u = np.random.default_rng(8).uniform(-1.0, 1.0, V.ndofs * bs)
    measure = dict(cells=cfx.locate_entities(cd, "phi<0"), rules=cfx.runtime_quadrature(cd, "phi<0", 4))
    worst = 0.0
    for kernel, functional, params in ((fem.MASS, fem.M_L2_DIFF, (fem.F_ONE, 1.0, 0.0)), (fem.STIFFNESS, fem.M_H1_SEMI, (0, 1.0))):
        A = fem.assemble_matrix(fem.form([fem.Integral(kernel, qdegree=2 * degree, **measure)], V))
        want, scale = _quadratic(A, u)
        got = fem.assemble_scalar(fem.form([fem.Integral(functional, params=params, qdegree=2 * degree, coefficient=u, **measure)], V))
        worst = max(worst, abs(got - want) / scale)
    _report(f"{tdim}-D n{n} P{degree} bs{bs} norms vs u^T A u", worst)
    assert 0.0 < worst <= TOL


@pytest.mark.parametrize("degree", [1, 2])
def test_facet_functional_equals_the_quadratic_form_of_the_jump_penalty(oracle, degree):
    """gamma / h_avg [u]^2 by a registered rank-0 facet integrand on the per-cell (DG) dofmap: over the ghost facets,
    and over [inside skeleton facets, facet-hosted rules] of the scrambled case, against u^T J u with J from JUMP."""
    import cutfemx_amd as cfx
    fem = cfx.fem
    cs = X.build_case(oracle, X.H_CASE)
    tdim = cs["tdim"]
    mesh, V1, fs, cd = _engine(cs)
    V, dofmap, ndofs = _dg_space(cs, mesh, degree)
    u = np.random.default_rng(9).uniform(-1.0, 1.0, ndofs)
    ghost = cfx.ghost_penalty_facets(cd, "phi<0")
    rows = cfx.interior_facets_for_cells(mesh, np.arange(cs["conn"].shape[0], dtype=np.int32))
    cdf = cfx.cut(fs[0], rows, tdim - 1)
    inside = rows.rows[cfx.locate_entities(cdf, "phi<0")]
    R = cfx.runtime_quadrature(cdf, "phi<0", 2 * degree)
    assert ghost.size > 0 and len(inside) > 0 and R.parent_map.size > 0
    kj = _registered("jump")
    worst = 0.0
    for measure in (dict(facets=ghost), dict(facets=inside, rules=R)):
        J = fem.assemble_matrix(fem.form([fem.Integral(fem.JUMP, params=(0.3,), qdegree=2 * degree, **measure)], V))
        want, scale = _quadratic(J, u)
        M = fem.form([fem.Integral(kj, params=(0.3,), qdegree=2 * degree, coefficient=u, **measure)], V)
        assert M.rank == 0
        got = fem.assemble_scalar(M)
        worst = max(worst, abs(got - want) / scale)
        # ... and entity by entity: the values of all facets (the rules' after the standard ones) add up to it
        n_ent = (ghost.size if "rules" not in measure else len(inside) + R.parent_map.size)
        parts = [float(fem.tabulate_entity(M, 0, i, False)[0]) for i in range(n_ent)]
        assert abs(sum(parts) - got) <= TOL * scale
    _report(f"{X.H_CASE} P{degree} facet jump functional", worst)
    assert 0.0 < worst <= TOL


# ---- 5. registered equals built-in ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tdim,n,degree", [(3, 5, 1), (2, 10, 2)])
def test_registered_sources_agree_with_the_builtin_ids(tdim, n, degree):
    import cutfemx_amd as cfx
    fem = cfx.fem
    mesh = cfx.Mesh.create_box(tdim, n)
    V1 = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V1, level_set_values(mesh.x, tdim)))
    V = cfx.FunctionSpace(mesh, degree)
    u = np.random.default_rng(10).uniform(0.25, 1.25, V.ndofs)    # positive: no cancellation in int u_h, the relative error means something
    measure = dict(cells=cfx.locate_entities(cd, "phi<0"), rules=cfx.runtime_quadrature(cd, "phi<0", 4))
    pairs = [(fem.M_FIELD, "field", (fem.F_ONE, 1.5), None), (fem.M_FIELD, "field", (fem.F_COEFFICIENT, 1.5), u),
             (fem.M_L2_DIFF, "l2", (fem.F_ONE, 0.7, 0.0), u), (fem.M_L2_DIFF, "l2", (fem.F_SINPROD, 0.7, 1.0), u),
             (fem.M_H1_SEMI, "h1", (0, 2.0), u)]
    worst = 0.0
    for builtin, user, params, coeff in pairs:
        vals = [fem.assemble_scalar(fem.form([fem.Integral(k, params=params, qdegree=4, coefficient=coeff, **measure)], V))
                for k in (builtin, _registered(user))]
        err = abs(vals[0] - vals[1]) / abs(vals[0])
        worst = max(worst, err)
        assert vals[0] > 0.0 and err <= 1e-13, (builtin, params, vals)
    _report(f"{tdim}-D n{n} P{degree} registered vs built-in", worst)


# ---- 6. two Functions on two spaces -----------------------------------------------------------------------------------
def _tabulate_np(tdim, degree, P):
    lam = np.concatenate([1.0 - P.sum(axis=1, keepdims=True), P], axis=1)
    if degree == 1:
        return lam
    return np.concatenate([lam * (2.0 * lam - 1.0)] + [4.0 * lam[:, [a]] * lam[:, [b]] for a, b in X.EDGES[tdim]], axis=1)


def test_jump_between_two_spaces_over_interface_rules():
    import cutfemx_amd as cfx
    fem = cfx.fem
    tdim, n = 2, 10
    mesh = cfx.Mesh.create_box(tdim, n)
    V1, V2 = cfx.FunctionSpace(mesh, 1), cfx.FunctionSpace(mesh, 2)
    cd = cfx.cut(cfx.Function(V1, level_set_values(mesh.x, tdim)))
    R = cfx.runtime_quadrature(cd, "phi=0", 4)
    rng = np.random.default_rng(11)
    u1, u2 = cfx.Function(V1, rng.uniform(-1, 1, V1.ndofs)), cfx.Function(V2, rng.uniform(-1, 1, V2.ndofs))
    dm1, dm2 = mesh.conn, cfx.lagrange_dofmap(tdim, mesh.conn, mesh.num_nodes, 2)[0]
    owner = np.repeat(R.parent_map, np.diff(R.offsets))

    def expected(a, b):
        va = np.einsum("qj,qj->q", _tabulate_np(tdim, 1, R.points), a[dm1[owner]])
        vb = np.einsum("qj,qj->q", _tabulate_np(tdim, 2, R.points), b[dm2[owner]])
        return float(np.sum(R.weights * (va - vb) ** 2))

    M = fem.form([fem.Integral(_registered("two"), rules=R, params=(0, 1.0), coefficients=(u1, u2))], V1)
    assert M.rank == 0
    first = fem.assemble_scalar(M)
    want = expected(np.asarray(u1.values), np.asarray(u2.values))
    assert want > 0.0 and abs(first - want) <= TOL * want
    # new values on the live form: no new form
    w1, w2 = cfx.Function(V1, rng.uniform(-1, 1, V1.ndofs)), cfx.Function(V2, rng.uniform(-1, 1, V2.ndofs))
    M.set_coefficients(0, (w1, w2))
    second = fem.assemble_scalar(M)
    want2 = expected(np.asarray(w1.values), np.asarray(w2.values))
    assert abs(second - want2) <= TOL * want2 and abs(second - first) > 1e-3 * want
    _report("two spaces over interface rules", max(abs(first - want) / want, abs(second - want2) / want2))


# ---- 7. the older route ----------------------------------------------------------------------------------------------
def test_source_forms_keep_their_route_and_agree_with_the_functional():
    import cutfemx_amd as cfx
    fem = cfx.fem
    tdim, n = 3, 5
    mesh = cfx.Mesh.create_box(tdim, n)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, level_set_values(mesh.x, tdim)))
    measure = dict(cells=cfx.locate_entities(cd, "phi<0"), rules=cfx.runtime_quadrature(cd, "phi<0", 4))
    u = np.random.default_rng(12).uniform(0.5, 1.0, V.ndofs)
    for params, coeff in (((fem.F_ONE, 1.0), None), ((fem.F_SINPROD, 2.0), None), ((fem.F_COEFFICIENT, 1.0), u)):
        L = fem.form([fem.Integral(fem.SOURCE, params=params, qdegree=4, coefficient=coeff, **measure)], V)
        old = fem.assemble_scalar(L)
        assert L.rank == 1 and old == float(fem.assemble_vector(L).sum())
        new = fem.assemble_scalar(fem.form([fem.Integral(fem.M_FIELD, params=params, qdegree=4, coefficient=coeff, **measure)], V))
        assert old > 0.0 and abs(new - old) <= TOL * old, (params, old, new)
        with pytest.raises(ValueError, match="rank-0"):
            fem.assemble_scalar(L, out=np.zeros(1))


# ---- 8. inside a sync-free step ---------------------------------------------------------------------------------------
def test_functional_inside_a_step_that_overflows_once():
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    from test_gpu_step import centre_of
    fem = cfx.fem
    tdim, n = 3, 16
    mesh = cfx.Mesh.create_box(tdim, n)
    V = cfx.FunctionSpace(mesh, 1)
    xt = torch.tensor(mesh.x[:, :tdim].copy(), device="cuda")
    phi = torch.empty(mesh.num_nodes, device="cuda", dtype=torch.float64)
    f = cfx.Function(V, phi)
    state = {"cd": None, "syncs": []}
    dev = torch.zeros(1, device="cuda", dtype=torch.float64)

    def body():
        if state["cd"] is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        cd = state["cd"]
        inside = cfx.locate_entities_device(cd, "phi<0")
        rules = cfx.runtime_quadrature(cd, "phi<0", 4)
        M = fem.form([fem.Integral(fem.M_FIELD, cells=inside, rules=rules, params=(fem.F_ONE, 1.0), qdegree=1)], V)
        s0 = _lib.sync_count()
        fem.assemble_scalar(M, out=dev)
        state["syncs"].append(_lib.sync_count() - s0)
        return M, inside, rules

    key = "test-functional-step"
    cfx.forget_step_history(key)
    try:
        cfx.set_step_margin(0.9, 0)        # capacities = 0.9 x the previous counts while the domain grows
        passes = []
        for k in range(2):
            phi.copy_(torch.linalg.norm(xt - centre_of(tdim, 0), dim=1) - (0.22 + 0.03 * k))
            info = {}
            held = cfx.run_step(body, key=key, info=info)
            passes.append(info["passes"])
        stepped = float(dev.cpu()[0])
    finally:
        cfx.set_step_margin()
    import os
    if os.environ.get("CFX_STEP_SPECULATE") != "0":
        assert passes == [1, 2], passes            # the second step overflows once and is repeated (redo = 1)
    assert all(s == 0 for s in state["syncs"]), state["syncs"]     # the call itself never reads back
    # the plain sequence on the same level set, bit for bit
    cd2 = cfx.cut(f)
    M2 = fem.form([fem.Integral(fem.M_FIELD, cells=cfx.locate_entities_device(cd2, "phi<0"),
                                rules=cfx.runtime_quadrature(cd2, "phi<0", 4), params=(fem.F_ONE, 1.0), qdegree=1)], V)
    plain = fem.assemble_scalar(M2)
    sphere = 4.0 / 3.0 * np.pi * 0.25 ** 3
    assert stepped == plain and abs(plain - sphere) < 0.05 * sphere
    # a rank-0 form made before cut.update is stale after it, like any other form
    M, inside, rules = held
    phi.add_(0.01)
    cfx.update(state["cd"])
    with pytest.raises(RuntimeError, match="stale form"):
        fem.assemble_scalar(M)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    fem = cfx.fem
    mesh = cfx.Mesh.create_box(2, 4)
    V = cfx.FunctionSpace(mesh, 1)
    cells = np.arange(mesh.num_cells, dtype=np.int32)
    M = fem.form([fem.Integral(fem.M_FIELD, cells=cells, params=(fem.F_ONE, 1.0), qdegree=1)], V)
    L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_ONE, 1.0))], V)
    assert M.rank == 0 and fem.assemble_scalar(M) == 1.0
    M.prepare()                                                     # succeeds, builds nothing
    with pytest.raises(RuntimeError, match="not a bilinear"):
        fem.create_matrix(M)
    with pytest.raises(ValueError, match="not linear"):
        fem.assemble_vector(M)
    with pytest.raises(ValueError, match="rank-2 bilinear"):
        fem.active_domain(M)
    v = C.c_double()
    assert _lib.lib().cfx_assemble_scalar(L._h, C.byref(v)) == _lib.ERR_INVALID_ARGUMENT
    assert b"rank 0" in _lib.lib().cfx_last_error()
    with pytest.raises(ValueError, match="kernel rank does not match"):
        fem.form([fem.Integral(fem.MASS, cells=cells)], V, rank=0)
    with pytest.raises(ValueError, match="kernel rank does not match"):
        fem.form([fem.Integral(fem.M_FIELD, cells=cells, params=(fem.F_ONE, 1.0))], V, rank=1)
    with pytest.raises(ValueError, match="CFX_F_COEFFICIENT"):      # u_h without its dof values
        fem.form([fem.Integral(fem.M_FIELD, cells=cells, params=(fem.F_COEFFICIENT, 1.0))], V)
    with pytest.raises(ValueError, match="bs = 1"):
        fem.form([fem.Integral(fem.M_L2_DIFF, cells=cells, params=(fem.F_SINPROD, 1.0, 1.0), coefficient=np.zeros(2 * V.ndofs))],
                 cfx.FunctionSpace(mesh, 1, bs=2))
    with pytest.raises(ValueError, match="registered facet integrands"):
        fem.form([fem.Integral(fem.M_FIELD, facets=np.zeros((0, 4), np.int32), params=(fem.F_ONE, 1.0))], V)


# ---- 10. the C++ facade ----------------------------------------------------------------------------------------------
def test_cpp_facade_assembles_the_volume(tmp_path):
    import cutfemx_amd as cfx
    fem = cfx.fem
    exe = tmp_path / "functional_facade"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/functional_facade.cpp"),
                    "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd", f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe), "3", "8"], check=True, capture_output=True, text=True).stdout
    got, got_dev = (float(t) for t in out.split()[-2:])
    mesh = cfx.Mesh.create_box(3, 8)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, level_set_values(mesh.x, 3)))
    M = fem.form([fem.Integral(fem.M_FIELD, cells=cfx.locate_entities(cd, "phi<0"), rules=cfx.runtime_quadrature(cd, "phi<0", 4),
                               params=(fem.F_ONE, 1.0), qdegree=1)], V)
    want = fem.assemble_scalar(M)
    assert got == got_dev and abs(got - want) <= TOL * want and abs(want - 4.0 / 3.0 * np.pi * 0.31 ** 3) < 0.1 * want
