"""The exact rectangular blocks, coefficient-weighted forms, coefficient sources, Dirichlet lifting and two-space facet
terms of `exact_cut.py`: self-checks that need neither the oracle nor the engine, then oracle == exact for every family
that `test_gpu_exact_forms.py` holds the engine to, so that a failure on the GPU can be placed.  CPU only.

Every integrand is a polynomial and every comparison integrates it exactly: `qdegree` (uncut cells) and the order of
the runtime rules are at least the integrand's degree (the tables below, asserted), so no two sides can agree by
under-integrating alike.  Self-checks are equalities in longdouble (1e-15 relative where a square root or a different
summation order enters).  Oracle: abs(got - exact) <= 1e-12 x the largest entry of the same tensor on the WHOLE cell or
facet (times max abs(kappa_cell) / max abs(w_cell) where a coefficient enters); assembled arrays: rel_err <= 1e-12; the
two-space JUMP block cancels in the assembled matrix and is measured on the scale of its local tensors; lifting:
1e-12 x max(abs(b0) + abs(A_exact) @ abs(alpha (g - x0))).  The oracle has no rectangular lifting: that one is compared
on the GPU alone, `exact_lift` itself is checked here against a dense product.

The case tables and the exact-side helpers below are shared with `test_gpu_exact_forms.py`.
"""
from fractions import Fraction as F

import numpy as np
import pytest

import exact_cut as X
from helpers import rel_err

TOL = 1e-12
EPS = 1e-15
LD = X.LD
C2, H2, S3, G3, D2 = "2d-n8-sphere", "2d-n8-sphere-scrambled", "3d-n4-sphere-scrambled", "3d-n5-gyroid", "2d-n7-degenerate-scrambled"
ENTITY_CASES = [C2, H2, S3, D2]            # per entity: every kept cut cell / ghost facet, one in ten inside cells
ASSEMBLED_CASES = [C2, H2, S3, G3]         # assembled over [inside cells, phi<0 rules]; all regular level sets
DEG6_CASES = (C2, S3)                      # where degree-6 moments are taken (P2 mass times P2 kappa)

# ---- family 1: rectangular blocks.  name: (kind, (degree, bs) test, (degree, bs) trial, params, integrand degree);
# bs "d" = tdim
RECT = {"Bt": ("div_test", (2, "d"), (1, 1), (-1.0,), 2), "B": ("div_trial", (1, 1), (2, "d"), (-1.0,), 2),
        "M21": ("mass", (2, 1), (1, 1), (), 3), "K12": ("stiffness", (1, 1), (2, 1), (), 1)}
RECT_Q, RECT_ORDER = 3, 4                  # qdegree of the uncut cells, order of the runtime rules


# ---- family 2: kappa-weighted forms.  Spaces by tdim: (degree, bs)
WEIGHTED_SPACES = {2: [(1, 1), (2, 1), (2, 2)], 3: [(1, 1), (2, 1), (1, 3)]}
ELASTIC = (1.0e3, 0.3)


def weighted_degree(kind, degree):
    """Polynomial degree of kappa x the integrand, kappa in the form's element."""
    return 3 * degree if kind == "mass" else 3 * degree - 2


def weighted_terms(name, degree, bs):
    """(kind, params, integrand degree = qdegree = rule order) of one space on one case."""
    out = [("stiffness", (), weighted_degree("stiffness", degree))]
    if degree == 1 or name in DEG6_CASES:
        out.append(("mass", (), weighted_degree("mass", degree)))
    if bs > 1:
        out.append(("elasticity", ELASTIC, weighted_degree("elasticity", degree)))
    return out


def kappa_values(ndofs, which):
    """The two coefficients: 1 + U(0, 2), and one that changes sign, U(-1, 1)."""
    rng = np.random.default_rng(17 + which)
    return 1.0 + rng.uniform(0.0, 2.0, ndofs) if which == 0 else rng.uniform(-1.0, 1.0, ndofs)


# ---- family 3: coefficient sources: (tdim, degree, bs, scale); the integrand f . v has degree 2 degree
SOURCES = {3: [(1, 1, 1.0), (1, 3, 1.5)], 2: [(2, 1, 1.0), (2, 2, 1.5)]}

# ---- family 5: two-space facet terms: (kind, params, qdegree, integrand degree P2 x P1)
FACET2 = [("ghost", (0.3, 2.0), 2, 1), ("jump", (5.0,), 3, 3)]
PAIRS = {"P2xP1": (2, 1), "P1xP2": (1, 2)}


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def dofmaps(cs, degree):
    from cutfemx_amd.mesh import lagrange_dofmap
    return X.cached(("dofmap", cs["name"], degree),
                    lambda: lagrange_dofmap(cs["tdim"], cs["conn"], cs["x"].shape[0], degree))


def rect_spec(cs, block):
    kind, (d0, b0), (d1, b1), params, ideg = RECT[block]
    d = cs["tdim"]
    return kind, (d0, d if b0 == "d" else b0), (d1, d if b1 == "d" else b1), params, ideg


def inside_sample(cs):
    """One in ten inside cells, as positions in the located list."""
    return list(range(0, cs["inside"].size, 10))


def left_out(cs):
    """`build_case`'s `keep` is all that is left out: at most 5 % of the cut cells, none for a regular level set."""
    n_out = int((~cs["keep"]).sum())
    assert n_out <= 0.05 * cs["cut"].size and (cs["degenerate"] or n_out == 0), (cs["name"], n_out)


def coo(entries, shape):
    import scipy.sparse as sp
    r, c, v = entries
    return sp.coo_matrix((v, (r, c)), shape=shape).tocsr()


def exact_rect(name, cs, block):
    """The assembled block over [inside cells, phi<0 rules]: (entries, shape)."""
    kind, (d0, b0), (d1, b1), params, _ = rect_spec(cs, block)
    (dm0, n0), (dm1, n1) = dofmaps(cs, d0), dofmaps(cs, d1)
    e = X.exact_entries(name, cs, dm0, b0, kind, d0, params, cs["inside"], trial=(dm1, b1, d1))
    return e, (n0 * b0, n1 * b1)


def exact_weighted(name, cs, degree, bs, kind, params, kappa, ideg):
    dm, nd = dofmaps(cs, degree)
    e = X.exact_entries(name, cs, dm, bs, kind, degree, params, cs["inside"], coefficient=kappa, mom_degree=max(4, ideg))
    return coo(e, (nd * bs, nd * bs))


def exact_source(name, cs, degree, bs, scale, w):
    dm, nd = dofmaps(cs, degree)
    r, v = X.exact_entries(name, cs, dm, bs, "source_coeff", degree, (scale,), cs["inside"], coefficient=w)
    out = np.zeros(nd * bs, dtype=LD)
    np.add.at(out, r, v.astype(LD))
    return out.astype(np.float64)


def exact_poisson_entries(name, cs, fc):
    """P1 stiffness over [inside cells, rules] + ghost penalty (0.1 h_avg [dn u][dn v]): the entries of the existing
    cell and facet references, put one after the other."""
    a = X.exact_entries(name, cs, cs["conn"], 1, "stiffness", 1, (), cs["inside"])
    b = X.exact_facet_entries(name, cs, cs["conn"], 1, "ghost", 1, (0.1, 0.0), fc["ghost"])
    return tuple(np.concatenate([u, v]) for u, v in zip(a, b))


def lifting_data(entries, shape, seed):
    """Seeded 10 % markers on the trial side, random g, x0 (trial) and b0 (test).  b0 is drawn on the scale of the
    matrix (its largest exact entry), so that the lifted part is not lost below it."""
    rng = np.random.default_rng(seed)
    marks = (rng.random(shape[1]) < 0.1).astype(np.int8)
    g, x0 = rng.standard_normal(shape[1]), rng.standard_normal(shape[1])
    return marks, g, x0, rng.standard_normal(shape[0]) * float(np.abs(entries[2]).max())


LIFT_VARIANTS = [(1.0, False), (1.0, True), (0.7, False), (0.7, True)]       # (alpha, with x0)


def facet2_scale(name, cs, rows, kind, params, d0, d1):
    """Largest entry of the term's local tensors on the whole facets `rows`."""
    whole = X.Moments(cs["tdim"] - 1)
    return max(float(np.abs(X.facet_tensor2(kind, X.facet_basis(name, cs, r, d0), X.facet_basis(name, cs, r, d1), whole, params)).max())
               for r in rows)


# ---- self-checks ------------------------------------------------------------------------------------------------------
def _some_cells(cs, n=12):
    cut = cs["cut"][cs["keep"]]
    return cut[:: max(1, cut.size // n)]


@pytest.mark.parametrize("name", [H2, S3])
def test_rectangular_tensors_reduce_to_the_square_ones_and_the_divergence_blocks_are_transposes(oracle, name):
    cs = X.build_case(oracle, name)
    d = cs["tdim"]
    for c in _some_cells(cs):
        xc = cs["x"][cs["conn"][c], :d]
        for mom in (X.Moments(d), X.cut_moments(name, cs, c)):
            for degree in (1, 2):
                for kind in ("mass", "stiffness"):
                    assert np.array_equal(X.rect_tensor(kind, mom, xc, degree, 1, degree, 1), X.tensor(kind, mom, xc, degree))
                T = X.rect_tensor("mass", mom, xc, degree, d, degree, d)
                n = T.shape[0] // d
                assert np.array_equal(T.reshape(n, d, n, d), np.einsum("ij,ab->iajb", X.mass(mom, xc, degree), np.eye(d)))
            for d0, d1 in ((2, 1), (1, 2), (2, 2)):
                Bt, B = X.rect_tensor("div_test", mom, xc, d0, d, d1, 1, (-1.0,)), X.rect_tensor("div_trial", mom, xc, d1, 1, d0, d, (-1.0,))
                assert Bt.shape == (B.shape[1], B.shape[0]) and np.array_equal(Bt, B.T) and np.abs(Bt).max() > 0
                for kind in ("mass", "stiffness"):      # (another summation order: to rounding)
                    T, S = X.rect_tensor(kind, mom, xc, d0, 1, d1, 1), X.rect_tensor(kind, mom, xc, d1, 1, d0, 1)
                    assert np.abs(T - S.T).max() <= EPS * np.abs(T).max()


def test_the_divergence_block_of_a_known_field_on_a_known_cell():
    """On the unit right triangle, v = (x^2, 0) in P2 and p = y in P1: -int 2 x y = -1/12; the row of component 1 of
    the same dofs against any p is -int d_y(x^2) p = 0.  d_x and d_y are told apart, and so are test and trial."""
    xc = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    Bt = X.rect_tensor("div_test", X.Moments(2), xc, 2, 2, 1, 1, (-1.0,))
    pts = np.concatenate([xc, [(xc[a] + xc[b]) / 2 for a, b in X.EDGES[2]]])
    v = np.zeros((6, 2))
    v[:, 0] = pts[:, 0] ** 2
    p = xc[:, 1]
    assert abs(v.ravel() @ Bt @ p + 1.0 / 12.0) <= EPS
    assert abs(v[:, ::-1].ravel() @ Bt @ p) <= EPS        # v = (0, x^2): div v = 0
    v[:, 0] = pts[:, 0] * pts[:, 1]                       # v = (x y, 0): div v = y; p = y: -int y^2 = -1/12
    assert abs(v.ravel() @ Bt @ p + 1.0 / 12.0) <= EPS
    assert abs(v.ravel() @ Bt @ xc[:, 0] + 1.0 / 24.0) <= EPS   # p = x: -int x y = -1/24


@pytest.mark.parametrize("name", [C2, S3])
def test_weights_one_and_the_partition_of_unity_give_the_unweighted_tensor_and_the_two_sides_add_up(oracle, name):
    cs = X.build_case(oracle, name)
    d = cs["tdim"]
    rng = np.random.default_rng(1)
    worst = 0.0
    for c in _some_cells(cs, 6):
        xc = cs["x"][cs["conn"][c], :d]
        ph = X.cell_phi([cs["phi"]], cs["conn"][c])[0]
        whole, neg = X.Moments(d, degree=6), X.cut_moments(name, cs, c, degree=6)
        pos = X.Moments(d, [(ph, 1)], 6)
        for degree in (1, 2):
            nd = X.basis(d, degree)[1].shape[0]
            kap = rng.uniform(-1.0, 1.0, nd)
            for kind, params in (("mass", ()), ("stiffness", ()), ("elasticity", ELASTIC)):
                plain = X.tensor(kind, neg, xc, degree, params)
                top = np.abs(X.tensor(kind, whole, xc, degree, params)).max()
                worst = max(worst, np.abs(X.weighted(kind, neg, xc, degree, np.ones(nd), params) - plain).max() / top)
                hats = sum(X.weighted(kind, neg, xc, degree, np.eye(nd)[k], params) for k in range(nd))
                worst = max(worst, np.abs(hats - plain).max() / top)
                both = X.weighted(kind, neg, xc, degree, kap, params) + X.weighted(kind, pos, xc, degree, kap, params)
                worst = max(worst, np.abs(both - X.weighted(kind, whole, xc, degree, kap, params)).max() / top)
                # a weight that is not constant is seen (P1 gradients are constants: the mass tensor tells)
                assert kind != "mass" or np.abs(X.weighted(kind, whole, xc, degree, kap, params) - kap.mean() * X.tensor(kind, whole, xc, degree, params)).max() > 1e-3 * top
        for block in RECT:
            kind, (d0, b0), (d1, b1), params, _ = rect_spec(cs, block)
            parts = X.rect_tensor(kind, neg, xc, d0, b0, d1, b1, params) + X.rect_tensor(kind, pos, xc, d0, b0, d1, b1, params)
            full = X.rect_tensor(kind, whole, xc, d0, b0, d1, b1, params)
            worst = max(worst, np.abs(parts - full).max() / np.abs(full).max())
        # the coefficient source is the mass tensor times the dofs, component by component
        w = rng.standard_normal((nd, d))
        got = X.source_coeff(neg, xc, 2, w, d, 1.5).reshape(nd, d)
        worst = max(worst, np.abs(got - 1.5 * X.mass(neg, xc, 2) @ w).max() / np.abs(X.mass(whole, xc, 2)).max())
    _report("self", f"{name} weights / two sides", worst)
    assert worst <= 4 * EPS


def test_moments_of_degree_six_extend_those_of_degree_four(oracle):
    cs = X.build_case(oracle, C2)
    c = cs["cut"][cs["keep"]][3]
    m4, m6 = X.cut_moments(C2, cs, c), X.cut_moments(C2, cs, c, degree=6)
    assert m4 is X.cut_moments(C2, cs, c) and m6 is not m4 and len(m6.alphas) > len(m4.alphas)
    assert all(m6.m[a] == m4.m[a] for a in m4.alphas)
    w = X.Moments(2, degree=6)
    assert w.m[(6, 0, 0)] == X._ld(F(2 * 720, 40320)) and w.m[(2, 2, 2)] == X._ld(F(2 * 8, 40320))


@pytest.mark.parametrize("name", [H2, S3, D2])
def test_two_space_facet_tensors_are_blind_to_what_has_no_jump(oracle, name):
    """The P2 x P1 gradient-jump tensor annihilates the macro dofs of global affine functions on the trial side and of
    global quadratics on the test side; the two-space JUMP tensor annihilates functions that are continuous across the
    facet on either side; with equal degrees both are the square tensors; P1 x P2 is the transpose of P2 x P1."""
    cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
    d = cs["tdim"]
    whole = X.Moments(d - 1)
    rng = np.random.default_rng(5)
    worst = 0.0
    for row in fc["ghost"]:
        fb = {k: X.facet_basis(name, cs, row, k) for k in (1, 2)}
        co = [F(int(v), 7) for v in rng.integers(-9, 10, size=16)]
        x0 = X.frac_rows(cs["x"][fb[1].verts[:1], :d])[0]
        nv = [-g for g in X.gradients(X.frac_rows(cs["x"][cs["conn"][row[0]], :d]))[0][int(row[1])]]

        def poly(degree):
            def f(p):
                v = co[3] + sum(co[a] * q for a, q in zip(range(d), p))
                return v if degree == 1 else v + co[4] * p[0] * p[1] + co[5] * p[-1] * p[-1] + co[6] * p[0] * p[0]
            return f

        def kinked(degree):
            def f(p):
                L = sum(a * (b - c) for a, b, c in zip(nv, p, x0))
                q = F(5, 3) + co[8] if degree == 1 else F(5, 3) + co[8] + sum(co[9 + a] * p[a] for a in range(d))
                return poly(degree)(p) + q * L
            return f

        smooth = {k: X.facet_dofs(fb[k], [poly(k), poly(k)], cs["x"], cs["conn"], row, k) for k in (1, 2)}
        cont = {k: X.facet_dofs(fb[k], [poly(k), kinked(k)], cs["x"], cs["conn"], row, k) for k in (1, 2)}
        for mom in (whole, X.facet_moments(name, cs, fb[1])):
            for kind, params, _, _ in FACET2:
                T = X.facet_tensor2(kind, fb[2], fb[1], mom, params)
                top = max(float(np.abs(X.facet_tensor2(kind, fb[2], fb[1], whole, params)).max()), 1e-300)
                assert T.shape == (2 * fb[2].val[0].shape[0], 2 * fb[1].val[0].shape[0])
                assert np.abs(X.facet_tensor2(kind, fb[1], fb[2], mom, params) - T.T).max() <= EPS * top
                for k in (1, 2):
                    assert np.array_equal(X.facet_tensor2(kind, fb[k], fb[k], mom, params), X.facet_tensor(kind, fb[k], mom, params))
                blind = smooth if kind == "ghost" else cont
                worst = max(worst, float(np.abs(T @ blind[1]).max() / (top * np.abs(blind[1]).max())),
                            float(np.abs(blind[2] @ T).max() / (top * np.abs(blind[2]).max())))
                if kind == "ghost" and mom is whole:            # the kink is seen from either side
                    assert np.abs(T @ cont[1]).max() > 1e-6 * top * np.abs(cont[1]).max()
                    assert np.abs(cont[2] @ T).max() > 1e-6 * top * np.abs(cont[2]).max()
    _report("self", f"{name} two-space facet null spaces", worst)
    assert worst <= EPS


def test_exact_lift_is_the_dense_product(oracle):
    cs = X.build_case(oracle, C2)
    e, shape = exact_rect(C2, cs, "M21")
    A = np.zeros(shape, dtype=LD)
    np.add.at(A, (e[0], e[1]), e[2].astype(LD))
    marks, g, x0, b0 = lifting_data(e, shape, 3)
    assert 0 < marks.sum() < marks.size
    for alpha, with_x0 in LIFT_VARIANTS:
        got, scale = X.exact_lift(e, shape, marks, g, x0 if with_x0 else None, alpha, b0)
        y = np.where(marks != 0, LD(alpha) * (g.astype(LD) - (x0.astype(LD) if with_x0 else 0)), LD(0))
        want = b0.astype(LD) - A @ y
        assert np.abs(got - want).max() <= 2e-16 * scale and scale >= np.abs(b0).max()
        assert np.abs(got - b0).max() > 1e-3 * scale                 # something is lifted
        if with_x0 and alpha != 1.0:                                 # alpha multiplies x0 as well
            other, _ = X.exact_lift(e, shape, marks, alpha * g, x0, 1.0, b0)
            assert np.abs(other - got).max() > 1e-3 * scale
    with pytest.raises(ValueError):
        X.exact_lift(e, shape, marks[:-1], g[:-1], None, 1.0, b0)


def test_the_cases_have_what_the_comparisons_need(oracle):
    """From the inputs alone: at most 5 % of a case's cut cells are left out, none for the regular level sets; every
    case has inside cells and ghost facets; the orders used integrate exactly."""
    for name in set(ENTITY_CASES + ASSEMBLED_CASES):
        cs, fc = X.build_case(oracle, name), X.facet_case(oracle, name)
        left_out(cs)
        print(f"EXACT cases: {name}: cut {cs['cut'].size} inside {cs['inside'].size} ghost {len(fc['ghost'])}")
        assert cs["inside"].size >= 1 and len(fc["ghost"]) >= 10 and cs["cut"].size >= 10
        assert int((~fc["ghost_keep"]).sum()) <= 0.05 * len(fc["ghost"])
    for name in ASSEMBLED_CASES:
        assert not X.build_case(oracle, name)["degenerate"]
    assert all(RECT_Q >= v[4] and RECT_ORDER >= v[4] for v in RECT.values())


# ---- oracle == exact ----------------------------------------------------------------------------------------------------
def _oracle(O, cs):
    om, phi = cs["om"], cs["phi"]
    dom = O.classify(om.conn, phi)
    assert np.array_equal(O.locate_entities(dom, "phi<0"), cs["inside"])
    return om, phi, dom


def _ospace(O, cs, degree, bs=1):
    dm, nd = dofmaps(cs, degree)
    return O.Space(dm, nd, degree, bs)


def _per_entity(cs, name, R, tab, want, top, mom_degree=4):
    """Worst abs(got - exact) / scale over the rules of the kept cut cells and one in ten inside cells.
    tab(index, use_rule) -> array; want(c, mom) -> exact array; top(c) -> scale.  A kept cut cell without a rule has no
    negative part: its exact tensor is zero."""
    d = cs["tdim"]
    kept = set(cs["cut"][cs["keep"]].tolist())
    got = {}
    for idx, c in enumerate(R.parent_map):
        if int(c) in kept:
            t = np.asarray(tab(idx, True))
            got[int(c)] = got[int(c)] + t if int(c) in got else t
    worst, n = 0.0, 0
    for c in kept:
        mom = X.cut_moments(name, cs, c, degree=mom_degree)
        if c not in got:
            assert mom.m[tuple([0] * (d + 1))] == 0
            continue
        w = want(c, mom)
        worst = max(worst, np.abs(got[c].reshape(w.shape) - w).max() / top(c))
        n += 1
    whole = X.Moments(d, degree=mom_degree)
    for pos in inside_sample(cs):
        c = int(cs["inside"][pos])
        w = want(c, whole)
        worst = max(worst, np.abs(np.asarray(tab(pos, False)).reshape(w.shape) - w).max() / top(c))
        n += 1
    assert n > len(inside_sample(cs)) and (n == len(kept) + len(inside_sample(cs)) or cs["degenerate"])
    return worst, n


@pytest.mark.parametrize("name", ENTITY_CASES + [G3])
def test_oracle_rectangular_blocks_are_exact(oracle, name):
    """`tabulate_entity2` of every kept cut cell's rule and of one in ten inside cells (not on the gyroid), and the
    assembled block over [inside cells, rules] (not on the degenerate case), for B^T, B, M21 and K12."""
    import scipy.sparse as sp
    O = oracle
    cs = X.build_case(O, name)
    om, phi, dom = _oracle(O, cs)
    d = cs["tdim"]
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", RECT_ORDER)
    whole = X.Moments(d)
    for block in RECT:
        kind, (d0, b0), (d1, b1), params, ideg = rect_spec(cs, block)
        assert RECT_Q >= ideg and RECT_ORDER >= ideg
        V0, V1 = _ospace(O, cs, d0, b0), _ospace(O, cs, d1, b1)
        I = O.Integral(O.CELL, getattr(O, "K_" + kind.upper()), entities=cs["inside"], rules=R, params=params, qdegree=RECT_Q)
        if name in ENTITY_CASES:
            xc = lambda c: cs["x"][cs["conn"][c], :d]
            worst, n = _per_entity(cs, name, R, lambda i, u: O.tabulate_entity2(om, V0, V1, I, i, u),
                                   lambda c, mom: X.rect_tensor(kind, mom, xc(c), d0, b0, d1, b1, params),
                                   lambda c: np.abs(X.rect_tensor(kind, whole, xc(c), d0, b0, d1, b1, params)).max())
            _report("rect tensors", f"oracle {name} {block} ({n} tensors)", worst)
            assert 0.0 < worst <= TOL
        if name in ASSEMBLED_CASES:
            e, shape = exact_rect(name, cs, block)
            ip, ix = O.create_sparsity2(om, V0, V1, [I])
            A = sp.csr_matrix((O.assemble_matrix2(om, V0, V1, [I], ip, ix), ix, ip), shape=shape)
            M = coo(e, shape)
            err = abs(A - M).max() / abs(M).max()
            _report("rect assembled", f"oracle {name} {block}", err)
            assert 0.0 < err <= TOL


@pytest.mark.parametrize("which", [0, 1], ids=["kappa-positive", "kappa-changes-sign"])
@pytest.mark.parametrize("name", ENTITY_CASES + [G3])
def test_oracle_weighted_forms_are_exact(oracle, name, which):
    """kappa x (mass, stiffness, elasticity), kappa a Function of the form's scalar element, for the spaces of
    WEIGHTED_SPACES: `tabulate_entity` per entity and the assembled matrix, each at qdegree = rule order = the integrand's
    degree (P2 mass: 6, on the cases that take degree-6 moments)."""
    import scipy.sparse as sp
    O = oracle
    cs = X.build_case(O, name)
    om, phi, dom = _oracle(O, cs)
    d = cs["tdim"]
    xc = lambda c: cs["x"][cs["conn"][c], :d]
    for degree, bs in WEIGHTED_SPACES[d]:
        dm, nd = dofmaps(cs, degree)
        kappa = kappa_values(nd, which)
        V = O.Space(dm, nd, degree, bs)
        for kind, params, ideg in weighted_terms(name, degree, bs):
            q = order = ideg
            assert q >= weighted_degree(kind, degree) and order >= weighted_degree(kind, degree)
            md = max(4, ideg)
            R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", order)
            I = O.Integral(O.CELL, getattr(O, "K_" + kind.upper()), entities=cs["inside"], rules=R, params=params, qdegree=q,
                           coefficient=kappa)
            whole = X.Moments(d, degree=md)
            blocks = (lambda T: X._diag_blocks(T, bs)) if kind != "elasticity" else (lambda T: T)
            if name in ENTITY_CASES:
                worst, n = _per_entity(
                    cs, name, R, lambda i, u: O.tabulate_entity(om, V, I, i, u),
                    lambda c, mom: blocks(X.weighted(kind, mom, xc(c), degree, kappa[dm[c]], params)),
                    lambda c: np.abs(X.tensor(kind, whole, xc(c), degree, params)).max() * np.abs(kappa[dm[c]]).max(), md)
                _report("weighted tensors", f"oracle {name} P{degree} bs {bs} {kind} q {q} ({n} tensors)", worst)
                assert 0.0 < worst <= TOL
            if name in ASSEMBLED_CASES:
                M = exact_weighted(name, cs, degree, bs, kind, params, kappa, ideg)
                ip, ix = O.create_sparsity(om, V, [I])
                A = sp.csr_matrix((O.assemble_matrix(om, V, [I], ip, ix), ix, ip), shape=M.shape)
                err = abs(A - M).max() / abs(M).max()
                _report("weighted assembled", f"oracle {name} P{degree} bs {bs} {kind} q {q}", err)
                assert 0.0 < err <= TOL


@pytest.mark.parametrize("name", ENTITY_CASES + [G3])
def test_oracle_coefficient_sources_are_exact(oracle, name):
    """SOURCE with F_COEFFICIENT, scalar and vector-valued (scale 1.5), per entity and assembled."""
    O = oracle
    cs = X.build_case(O, name)
    om, phi, dom = _oracle(O, cs)
    d = cs["tdim"]
    xc = lambda c: cs["x"][cs["conn"][c], :d]
    whole = X.Moments(d)
    for degree, bs, scale in SOURCES[d]:
        dm, nd = dofmaps(cs, degree)
        w = np.random.default_rng(23 + bs).standard_normal(nd * bs)
        q = order = 2 * degree
        V = O.Space(dm, nd, degree, bs)
        R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", order)
        I = O.Integral(O.CELL, O.L_SOURCE, entities=cs["inside"], rules=R, params=(O.F_COEFFICIENT, scale), qdegree=q, coefficient=w)
        wc = lambda c: w.reshape(nd, bs)[dm[c]]
        if name in ENTITY_CASES:
            worst, n = _per_entity(cs, name, R, lambda i, u: O.tabulate_entity(om, V, I, i, u),
                                   lambda c, mom: X.source_coeff(mom, xc(c), degree, wc(c), bs, scale),
                                   lambda c: scale * np.abs(X.mass(whole, xc(c), degree)).max() * np.abs(wc(c)).max())
            _report("source tensors", f"oracle {name} P{degree} bs {bs} ({n} vectors)", worst)
            assert 0.0 < worst <= TOL
        if name in ASSEMBLED_CASES:
            err = rel_err(O.assemble_vector(om, V, [I]), exact_source(name, cs, degree, bs, scale, w))
            _report("source assembled", f"oracle {name} P{degree} bs {bs}", err)
            assert 0.0 < err <= TOL


@pytest.mark.parametrize("name", [H2, S3])
def test_oracle_square_lifting_is_exact(oracle, name):
    """apply_lifting of the P1 Poisson matrix (stiffness + ghost penalty) and of the P2 stiffness, alpha 1 and 0.7, with
    and without x0, against b0 - A_exact alpha (g - x0)."""
    O = oracle
    cs, fc = X.build_case(O, name), X.facet_case(O, name)
    om, phi, dom = _oracle(O, cs)
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 4)
    forms = {"P1 poisson": (1, [O.Integral(O.CELL, O.K_STIFFNESS, entities=cs["inside"], rules=R, qdegree=0),
                                O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=fc["ghost"], params=(0.1,), qdegree=0)],
                            exact_poisson_entries(name, cs, fc)),
             "P2 stiffness": (2, [O.Integral(O.CELL, O.K_STIFFNESS, entities=cs["inside"], rules=R, qdegree=2)],
                              X.exact_entries(name, cs, dofmaps(cs, 2)[0], 1, "stiffness", 2, (), cs["inside"]))}
    for what, (degree, a, entries) in forms.items():
        V = _ospace(O, cs, degree)
        n = V.ndofs
        marks, g, x0, b0 = lifting_data(entries, (n, n), 31)
        worst = 0.0
        for alpha, with_x0 in LIFT_VARIANTS:
            want, scale = X.exact_lift(entries, (n, n), marks, g, x0 if with_x0 else None, alpha, b0)
            got = O.apply_lifting(om, V, a, marks, g, b0.copy(), x0 if with_x0 else None, alpha)
            worst = max(worst, np.abs(got - want).max() / scale)
            assert np.abs(want - b0).max() > 1e-3 * scale
        _report("lifting", f"oracle {name} {what}", worst)
        assert 0.0 < worst <= TOL


@pytest.mark.parametrize("name", ENTITY_CASES + [G3])
def test_oracle_two_space_facet_terms_are_exact(oracle, name):
    """GHOST_GRADJUMP (0.3, 2.0) at qdegree 2 and JUMP (5.0,) at qdegree 3 between P2 and P1, both orders:
    `tabulate_entity2` of every kept ghost facet; the assembled block alone and next to the mass block over [inside
    cells, rules]."""
    import scipy.sparse as sp
    O = oracle
    cs, fc = X.build_case(O, name), X.facet_case(O, name)
    om, phi, dom = _oracle(O, cs)
    d = cs["tdim"]
    whole = X.Moments(d - 1)
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", RECT_ORDER)
    for pair, (d0, d1) in PAIRS.items():
        V0, V1 = _ospace(O, cs, d0), _ospace(O, cs, d1)
        (dm0, n0), (dm1, n1) = dofmaps(cs, d0), dofmaps(cs, d1)
        for kind, params, q, ideg in FACET2:
            assert q >= ideg
            I = O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP if kind == "ghost" else O.K_JUMP, entities=fc["ghost"],
                           params=params, qdegree=q)
            if name in ENTITY_CASES:
                worst, n = 0.0, 0
                for i, row in enumerate(fc["ghost"]):
                    if not fc["ghost_keep"][i]:
                        continue
                    want = X.facet_tensor2(kind, X.facet_basis(name, cs, row, d0), X.facet_basis(name, cs, row, d1), whole, params)
                    got = O.tabulate_entity2(om, V0, V1, I, i, False)
                    worst = max(worst, np.abs(got - want.astype(np.float64)).max() / float(np.abs(want).max()))
                    n += 1
                _report("facet2 tensors", f"oracle {name} {pair} {kind} ({n} tensors)", worst)
                assert n > 0 and 0.0 < worst <= TOL
            if name in ASSEMBLED_CASES:
                scale = facet2_scale(name, cs, fc["ghost"], kind, params, d0, d1)
                G = coo(X.exact_facet_entries2(name, cs, dm0, d0, dm1, d1, kind, params, fc["ghost"]), (n0, n1))
                ip, ix = O.create_sparsity2(om, V0, V1, [I])
                A = sp.csr_matrix((O.assemble_matrix2(om, V0, V1, [I], ip, ix), ix, ip), shape=(n0, n1))
                e1 = abs(A - G).max() / scale
                Im = O.Integral(O.CELL, O.K_MASS, entities=cs["inside"], rules=R, qdegree=RECT_Q)
                Mx = coo(X.exact_entries(name, cs, dm0, 1, "mass", d0, (), cs["inside"], trial=(dm1, 1, d1)), (n0, n1))
                ip, ix = O.create_sparsity2(om, V0, V1, [I, Im])
                A2 = sp.csr_matrix((O.assemble_matrix2(om, V0, V1, [I, Im], ip, ix), ix, ip), shape=(n0, n1))
                e2 = abs(A2 - (G + Mx)).max() / max(scale, abs(Mx).max())
                _report("facet2 assembled", f"oracle {name} {pair} {kind}: alone {e1:.3e} with mass", e2)
                assert e1 <= TOL and 0.0 < e2 <= TOL
