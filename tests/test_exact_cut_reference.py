"""The exact rational reference of `exact_cut.py`: its own self-checks (exact equality in Fraction, no tolerance), and
the CPU oracle against it -- every cut cell / rule / host of every case, all monomials up to the rule's order,
1e-12 relative to the same moment of the WHOLE cell (a sliver's own moment is arbitrarily small).

Cells a test may leave out are selected from the inputs alone (`exact_cut.build_case`): all vertex values exactly
zero; for phi = 0 rules and normals a whole face on the interface with the cell on the negative side.  Each test
asserts that they are at most 5 % of the case's cut cells, and 0 for regular level sets.
"""
import itertools
import math
import random
from fractions import Fraction as F

import numpy as np
import pytest

import exact_cut as X

TOL = 1e-12
SPHERES = ["2d-n8-sphere", "3d-n4-sphere"]
TENSOR_CASES = ["2d-n8-sphere", "3d-n4-sphere", "3d-n4-sphere-scrambled", "2d-n7-degenerate-scrambled"]


# ---- self-checks of the module ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_whole_simplex_moments_equal_the_closed_form(d):
    alphas = X.monomials(d + 1, 8 if d < 3 else 6)
    for degree in (8, 5):
        use = [a for a in alphas if sum(a) <= degree]
        assert X.mean_moments(X.unit_simplex(d), use, degree) == [X.whole_moment(d, a) for a in use]
    low = [a for a in alphas if sum(a) <= 2]
    assert X.region_moments(d, [], low, 2) == [X.whole_moment(d, a) for a in low]


def _vertex_values(d):
    rnd = random.Random(7 + d)
    vals = [[F(rnd.uniform(-1, 1)) for _ in range(d + 1)] for _ in range(12)]
    vals += [[F(rnd.choice([0.0, 0.0, -1e-300, 3e-13, 0.7, -0.2])) for _ in range(d + 1)] for _ in range(40)]
    return vals


@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_two_sides_add_up_to_the_whole(d):
    alphas = X.monomials(d + 1, 4)
    whole = [X.whole_moment(d, a) for a in alphas]
    for phi in _vertex_values(d):
        if all(v == 0 for v in phi):
            continue
        neg, pos = X.region_moments(d, [(phi, -1)], alphas, 4), X.region_moments(d, [(phi, 1)], alphas, 4)
        assert [a + b for a, b in zip(neg, pos)] == whole, phi


def test_level_set_through_a_vertex_along_an_edge_along_a_face():
    one = [(0, 0, 0, 0)]
    vol = lambda phi, side: X.region_moments(3, [([F(v) for v in phi], side)], one, 0)[0]
    # through vertex 0: the positive part is the tetrahedron of vertex 3, vertex 0 and the zeros on edges 1-3 and 2-3
    # at 1/2 and 1/2 (then 1/2 and 1/4) of the way from vertex 3
    assert vol([0, -1, -1, 1], -1) == F(3, 4) and vol([0, -1, -1, 1], 1) == F(1, 2) * F(1, 2)
    assert vol([0, -1, -3, 1], 1) == F(1, 2) * F(1, 4)
    # along edge 0-1: the plane through it and the point at t = 2/3 of edge 2-3
    assert vol([0, 0, -2, 1], -1) == F(2, 3) and vol([0, 0, -2, 1], 1) == F(1, 3)
    # along face 0-1-2: one side owns the cell
    assert vol([0, 0, 0, 1], 1) == 1 and vol([0, 0, 0, 1], -1) == 0
    assert vol([0, 0, 0, -1], -1) == 1 and vol([0, 0, 0, -1], 1) == 0
    assert len(X.interface_faces(3, [F(0), F(0), F(0), F(-1)])) == 1 and X.interface_faces(3, [F(0), F(0), F(0), F(1)]) == []
    faces = X.interface_faces(3, [F(0), F(0), F(-2), F(1)])
    assert len(faces) == 1 and sorted(faces[0]) == sorted([(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, F(1, 3), F(2, 3))])
    # 2-D: through a vertex; interface length of x = 1/4 in the unit right triangle is 3/4
    assert X.region_moments(2, [([F(0), F(-1), F(3)], -1)], [(0, 0, 0)], 0)[0] == F(1, 4)
    Xt = X.frac_rows([[0, 0], [1, 0], [0, 1]])
    (length,) = X.interface_moments(2, [F(-1), F(3), F(-1)], Xt, [(0, 0, 0)], 0)
    assert length == 0.75


def _kuhn_cube():
    """The six tetrahedra of the unit cube along the diagonal (0,0,0)-(1,1,1), built here from the permutations."""
    tets = []
    for perm in itertools.permutations(range(3)):
        v, pts = [0, 0, 0], [(0, 0, 0)]
        for k in perm:
            v[k] = 1
            pts.append(tuple(v))
        tets.append([[F(c) for c in p] for p in pts])
    return tets


@pytest.mark.parametrize("plane", ["x<a", "x+y+z<c", "x+2y<b"])
def test_plane_cuts_of_the_unit_box_have_their_closed_form_moments(plane):
    """Volume, centroid and second moments (all monomials x^i y^j z^k up to degree 2) of {plane} in the unit cube."""
    a, c, b = F(3, 10), F(7, 8), F(1, 2)
    alphas = X.monomials(3, 2)
    fac = math.factorial
    if plane == "x<a":
        coef, rhs = (1, 0, 0), a
        want = [a ** (i + 1) / ((i + 1) * (j + 1) * (k + 1)) for i, j, k in alphas]
    elif plane == "x+y+z<c":       # the corner simplex scaled by c
        coef, rhs = (1, 1, 1), c
        want = [c ** (3 + i + j + k) * F(fac(i) * fac(j) * fac(k), fac(3 + i + j + k)) for i, j, k in alphas]
    else:                          # the prism {x + 2 y < b} x [0, 1]: the triangle (0,0), (b,0), (0,b/2) in x, y
        coef, rhs = (1, 2, 0), b
        want = [b ** (i + 1) * (b / 2) ** (j + 1) * F(fac(i) * fac(j), fac(2 + i + j)) / (k + 1) for i, j, k in alphas]
    got = [F(0)] * len(alphas)
    for tet in _kuhn_cube():
        phi = [sum(cf * x for cf, x in zip(coef, p)) - rhs for p in tet]
        for leaf in X.region(3, [(phi, -1)]):
            vf = X.volfrac(leaf) * F(1, 6)
            for n, m in enumerate(X.mean_moments(X.physical(leaf, tet), alphas, 2)):
                got[n] += vf * m
    assert got == want


@pytest.mark.parametrize("d", [2, 3])
def test_two_level_sets_partition_the_first(d):
    alphas = X.monomials(d + 1, 3)
    vals = _vertex_values(d)
    for A, B in zip(vals[:20], vals[20:40]):
        if all(v == 0 for v in A) or all(v == 0 for v in B):
            continue
        for sa in (-1, 1):
            whole = X.region_moments(d, [(A, sa)], alphas, 3)
            parts = [X.region_moments(d, [(A, sa), (B, sb)], alphas, 3) for sb in (-1, 1)]
            assert [p + q for p, q in zip(*parts)] == whole
            assert X.region_moments(d, [(B, -1), (A, sa)], alphas, 3) == parts[0]     # the order of the clauses


def test_physical_measures_and_gradients():
    Xt = X.frac_rows([[0, 0, 0], [2, 0, 0], [0, 3, 0], [0, 0, 4]])
    assert X.measure(Xt) == 4.0 and X.measure(Xt[1:]) == math.sqrt(F(61)) and X.measure(Xt[:2]) == 2.0
    G, vol = X.gradients(Xt)
    assert vol == 4 and G[1] == [F(1, 2), 0, 0] and G[0] == [F(-1, 2), F(-1, 3), F(-1, 4)]
    tiny = X.frac_rows([[0, 0], [1e-200, 0], [0, 1e-200]])
    assert X.measure(tiny[1:]) == pytest.approx(math.sqrt(2.0) * 1e-200, rel=1e-15)


# ---- the oracle against the exact values ------------------------------------------------------------------------------
def _report(group, what, worst):
    print(f"EXACT oracle {group}: {what}: worst {worst:.3e}")       # (shown with -s; DESIGN 4 quotes these)


def _left_out(cs, keep):
    """At most 5 % of the cut cells are left out, none for a regular level set."""
    n_out = int((~keep).sum())
    assert n_out <= 0.05 * cs["cut"].size and (cs["degenerate"] or n_out == 0), (n_out, cs["cut"].size)


@pytest.mark.parametrize("sel", ["phi<0", "phi>0"])
@pytest.mark.parametrize("name", list(X.CASES))
def test_oracle_volume_rules_have_the_exact_moments(oracle, name, sel):
    O = oracle
    cs = X.build_case(O, name)
    om, tdim, phi, cut = cs["om"], cs["tdim"], cs["phi"], cs["cut"]
    dom = O.classify(om.conn, phi)
    assert np.array_equal(np.flatnonzero(dom == 0), cut)
    _left_out(cs, cs["keep"])
    ex, alphas = X.exact_volume_moments(name, om.x, om.conn, [phi], cut, sel, max(cs["orders"]))
    full, vol = X.whole_moments(tdim, alphas), X.cell_measures(om.x, om.conn, tdim)
    deg = np.array([sum(a) for a in alphas])
    side = -1.0 if sel == "phi<0" else 1.0
    worst = 0.0
    for order in cs["orders"]:
        R = O.runtime_quadrature(om, om.conn, phi, dom, sel, order)
        assert np.all(np.isin(R.parent_map, cut)) and np.unique(R.parent_map).size == R.parent_map.size
        got = X.rule_moments(R, alphas, om.ncells)[cut] / vol[cut, None]
        err = (np.abs(got - ex) / full)[cs["keep"]][:, deg <= order]
        worst = max(worst, err.max())
        assert err.max() <= TOL, (order, err.max())
        # every point lies in the reference simplex and on its side of phi_h (1e-14, as test_rule_array_contracts)
        lam = np.concatenate([1.0 - R.points.sum(axis=1, keepdims=True), R.points], axis=1)
        owner = np.repeat(R.parent_map, np.diff(R.offsets))
        pv = phi[om.conn[owner]]
        assert lam.min() > -1e-14 and lam.max() < 1 + 1e-14
        assert np.all(side * np.einsum("qk,qk->q", lam, pv) >= -1e-14 * np.abs(pv).max(axis=1))
    _report("rules", f"{name} {sel}", worst)


@pytest.mark.parametrize("name", list(X.CASES))
def test_oracle_interface_rules_have_the_exact_moments(oracle, name):
    """Rules of one parent summed: a 3-D cell cut in a quadrilateral has two phi=0 rules with the same parent."""
    O = oracle
    cs = X.build_case(O, name)
    om, tdim, phi, cut = cs["om"], cs["tdim"], cs["phi"], cs["cut"]
    dom = O.classify(om.conn, phi)
    _left_out(cs, cs["keep_itf"])
    scale = X.interface_scale(om.x, om.conn, cut, tdim)
    D = max(cs["orders"])
    ex, alphas = X.exact_interface_moments(name, om.x, om.conn, [phi], cut, "phi=0", D)
    full, deg = X.whole_moments(tdim, alphas), np.array([sum(a) for a in alphas])
    doubles, worst = 0, 0.0
    for order in cs["orders"]:
        R = O.runtime_quadrature(om, om.conn, phi, dom, "phi=0", order)
        doubles += R.parent_map.size - np.unique(R.parent_map).size
        got = X.rule_moments(R, alphas, om.ncells)[cut]
        err = (np.abs(got - ex) / (scale[:, None] * full))[cs["keep_itf"]][:, deg <= order]
        worst = max(worst, err.max())
        assert err.max() <= TOL, (order, err.max())
    _report("rules", f"{name} phi=0", worst)
    if tdim == 3:
        assert doubles > 0
    # the normal of the parent cell at every interface point
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi=0", cs["orders"][-1])
    nrm = O.evaluate_normals(om, om.conn, phi, R)
    owner = np.repeat(R.parent_map, np.diff(R.offsets))
    ok = np.zeros(om.ncells, dtype=bool)
    ok[cut[cs["keep_itf"]]] = True
    want = {c: X.normal(X.cell_phi([phi], om.conn[c])[0], X.frac_rows(om.x[om.conn[c], :tdim])) for c in np.unique(owner[ok[owner]])}
    assert len(want) > 0
    err = np.abs(nrm[ok[owner]] - np.array([want[c] for c in owner[ok[owner]]])).max()
    _report("normals", name, err)
    assert err <= TOL


@pytest.mark.parametrize("sel", ["phi<0 and phi1>0", "phi<0 and phi1<0", "phi=0 and phi1<0"])
@pytest.mark.parametrize("name", SPHERES + ["3d-n4-sphere-scrambled"])
def test_oracle_multi_level_set_rules_have_the_exact_moments(oracle, name, sel):
    O = oracle
    cs = X.multi_case(O, name)
    om, tdim, cut = cs["om"], cs["tdim"], cs["cut"]
    dom = O.classify_multi(om.conn, cs["phis"])
    vol = X.cell_measures(om.x, om.conn, tdim)
    for order in (2, 4):
        R = O.runtime_quadrature_multi(om, om.conn, cs["phis"], dom, sel, order)
        assert R.parent_map.size > 0 and np.all(np.isin(R.parent_map, cut))
        if "=" in sel:
            ex, alphas = X.exact_interface_moments("multi-" + name, om.x, om.conn, cs["phis"], cut, sel, 4)
            scale = X.interface_scale(om.x, om.conn, cut, tdim)[:, None]
        else:
            ex, alphas = X.exact_volume_moments("multi-" + name, om.x, om.conn, cs["phis"], cut, sel, 4)
            scale = vol[cut, None]
        full, deg = X.whole_moments(tdim, alphas), np.array([sum(a) for a in alphas])
        got = X.rule_moments(R, alphas, om.ncells)[cut] / scale
        want = ex / scale if "=" in sel else ex          # surface moments are physical, volume moments fractions
        err = (np.abs(got - want) / full)[:, deg <= order]
        _report("multi", f"{name} {sel} order {order}", err.max())
        assert err.max() <= TOL, (order, err.max())


# the spheres lie inside the box: only the gyroid and the degenerate level sets cut boundary facets
HOST_CASES = [(n, "interior") for n in SPHERES + ["3d-n4-degenerate", "2d-n7-degenerate-scrambled"]] + \
             [("3d-n5-gyroid", "exterior"), ("3d-n4-degenerate", "exterior")]


@pytest.mark.parametrize("name,which", HOST_CASES)
def test_oracle_facet_host_rules_have_the_exact_moments(oracle, name, which):
    O = oracle
    cs = X.build_case(O, name)
    hc = X.host_case(O, name, which)
    om, tdim, phi = cs["om"], cs["tdim"], cs["phi"]
    H = O.facet_hosts(om, hc["rows"], om.conn)
    assert np.array_equal(H.verts, hc["verts"])
    fdom = O.facet_classify(H, phi)
    assert np.array_equal(np.flatnonzero(fdom == 0), hc["cut"]) and hc["cut"].size > 0
    assert int((~hc["keep"]).sum()) <= 0.05 * hc["cut"].size
    for sel in ("phi<0", "phi>0"):
        ex, alphas = X.exact_volume_moments(f"{name}-{which}", om.x, hc["verts"], [phi], hc["cut"], sel, 4)
        full, deg = X.whole_moments(tdim - 1, alphas), np.array([sum(a) for a in alphas])
        for order in (1, 2, 3, 4):
            R = O.facet_runtime_quadrature(om, H, phi, fdom, sel, order)
            assert R.tdim == tdim - 1
            got = X.rule_moments(R, alphas, hc["rows"].shape[0])[hc["cut"]] / hc["measure"][:, None]
            err = (np.abs(got - ex) / full)[hc["keep"]][:, deg <= order]
            _report("facet hosts", f"{name} {which} {sel} order {order}", err.max())
            assert err.max() <= TOL, (sel, order, err.max())


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", TENSOR_CASES)
def test_oracle_cut_cell_tensors_are_the_exact_ones(oracle, name, degree):
    """tabulate_entity(use_rule=True) of EVERY cut cell: stiffness and mass, P1 and P2."""
    from cutfemx_amd.mesh import lagrange_dofmap
    O = oracle
    cs = X.build_case(O, name)
    om, tdim, phi = cs["om"], cs["tdim"], cs["phi"]
    dom = O.classify(om.conn, phi)
    dofmap, ndofs = lagrange_dofmap(tdim, om.conn, om.nnodes, degree)
    V = O.Space(dofmap, ndofs, degree)
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 4)
    whole = X.Moments(tdim)
    kept = set(cs["cut"][cs["keep"]].tolist())
    worst = 0.0
    for kind, kernel in (("stiffness", O.K_STIFFNESS), ("mass", O.K_MASS)):
        integral = O.Integral(O.CELL, kernel, rules=R, qdegree=2 * degree)
        for idx, c in enumerate(R.parent_map):
            if int(c) not in kept:
                continue
            xc = om.x[om.conn[c], :tdim]
            want = X.tensor(kind, X.cut_moments(name, cs, c), xc, degree)
            scale = np.abs(X.tensor(kind, whole, xc, degree)).max()
            got = O.tabulate_entity(om, V, integral, idx, True)
            worst = max(worst, np.abs(got - want).max() / scale)
    _report("tensors", f"{name} P{degree} stiffness + mass", worst)
    assert 0.0 < worst <= TOL, worst


def test_oracle_assembled_arrays_are_the_exact_ones(oracle):
    """Forms over [inside cells, rules] on the 5^3 gyroid: P2-vector elasticity, P1 stiffness + mass, the f = 1 source."""
    import scipy.sparse as sp
    from cutfemx_amd.mesh import lagrange_dofmap
    from helpers import rel_err
    O, name = oracle, "3d-n5-gyroid"
    cs = X.build_case(O, name)
    om, phi, inside = cs["om"], cs["phi"], cs["inside"]
    dom = O.classify(om.conn, phi)
    assert np.array_equal(O.locate_entities(dom, "phi<0"), inside)
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 2)
    for degree, bs, terms in ((2, 3, [("elasticity", O.K_ELASTICITY, (1.0e3, 0.3), 2)]),
                              (1, 1, [("stiffness", O.K_STIFFNESS, (), 0), ("mass", O.K_MASS, (), 2)])):
        dofmap, ndofs = lagrange_dofmap(3, om.conn, om.nnodes, degree)
        V = O.Space(dofmap, ndofs, degree, bs)
        oa = [O.Integral(O.CELL, k, entities=inside, rules=R, params=p, qdegree=q) for _, k, p, q in terms]
        ip, ix = O.create_sparsity(om, V, oa)
        A = sp.csr_matrix((O.assemble_matrix(om, V, oa, ip, ix), ix, ip), shape=(ndofs * bs, ndofs * bs))
        M = None
        for kind, _, p, _ in terms:
            r, c, v = X.exact_entries(name, cs, dofmap, bs, kind, degree, p, inside)
            m = sp.coo_matrix((v, (r, c)), shape=A.shape).tocsr()
            M = m if M is None else M + m
        err = abs(A - M).max() / abs(M).max()
        _report("assembled", f"{name} P{degree} bs {bs} {[t[0] for t in terms]}", err)
        assert err <= TOL
    b = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                          [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=R, params=(O.F_ONE, 1.0), qdegree=1)])
    r, v = X.exact_entries(name, cs, om.conn, 1, "source", 1, (1.0,), inside)
    want = np.zeros(om.nnodes)
    np.add.at(want, r, v)
    _report("assembled", f"{name} P1 source", rel_err(b, want))
    assert rel_err(b, want) <= TOL


def test_every_sign_pattern_and_degenerate_class_is_compared(oracle):
    """All 2^(d+1) - 2 mixed sign patterns of a triangle and of a tetrahedron occur among the compared cut cells
    (in the local vertex order the kernels see), all-negative and all-positive cells among the uncut ones, and a
    level set through exactly 1, ..., d vertices of a cut cell (vertex, edge, face on the interface)."""
    seen = {2: set(), 3: set()}
    zeros = {2: set(), 3: set()}
    uncut = set()
    for name in X.CASES:
        cs = X.build_case(oracle, name)
        v = cs["phi"][cs["conn"]]
        for row in v[cs["cut"][cs["keep"]]]:
            p = X.sign_pattern(row)
            zeros[cs["tdim"]].add(p.count(0))
            if 0 not in p:
                seen[cs["tdim"]].add(p)
        uncut |= {-1} if cs["inside"].size else set()
        uncut |= {1} if np.any(np.all(v > 0, axis=1)) else set()
    assert uncut == {-1, 1}
    for d in (2, 3):
        mixed = {p for p in itertools.product((-1, 1), repeat=d + 1) if len(set(p)) == 2}
        assert seen[d] == mixed, (d, sorted(mixed - seen[d]))
        assert set(range(1, d + 1)) <= zeros[d], (d, zeros[d])
