"""Exact rational reference for P1 cuts of simplices: moments of {phi_h < 0}, {phi_h > 0} and {phi_h = 0} inside a
simplex, for one or several level sets and for facet hosts, and the local tensors that follow from the moments.

For a P1 level set the cut part of a simplex is a convex polytope whose vertices are rational functions of the float64
inputs, and every built-in integrand is a polynomial in the barycentric coordinates, so `fractions.Fraction` gives
the true value of each moment.  Nothing here shares a table or a line with the engine or with the oracle: the
sub-division is a recursive edge split (no case tables), the integration rule is Grundmann-Moeller with rational
points and weights derived below, the P2 basis is written in barycentric monomials.

Imported by the test files like `helpers.py`; needs numpy only for array I/O.
"""
from __future__ import annotations

import itertools
import math
from fractions import Fraction as F
from functools import lru_cache

import numpy as np

EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}   # Basix P2 edge order


# ---------------------------------------------------------------------------------------------------------------------
# clipping without tables
# ---------------------------------------------------------------------------------------------------------------------
def unit_simplex(d):
    return [tuple(F(int(i == j)) for j in range(d + 1)) for i in range(d + 1)]


def values(simplex, phi):
    return [sum(l * p for l, p in zip(v, phi) if l) for v in simplex]


def split(simplex, phi):
    """Leaves of `simplex` (barycentric vertices w.r.t. the parent) none of which has an edge whose ends have
    strictly opposite signs of phi_h: [(leaf, vertex values)].  Each step puts the zero of phi_h on such an edge and
    replaces the simplex by the two that have that point in place of one end each, so the leaves tile the simplex."""
    val = values(simplex, phi)
    for i, j in itertools.combinations(range(len(simplex)), 2):
        if (val[i] < 0 < val[j]) or (val[j] < 0 < val[i]):
            t = val[i] / (val[i] - val[j])
            c = tuple(a + t * (b - a) for a, b in zip(simplex[i], simplex[j]))
            s1 = list(simplex); s1[j] = c
            s2 = list(simplex); s2[i] = c
            return split(s1, phi) + split(s2, phi)
    return [(list(simplex), val)]


def det(M):
    n = len(M)
    if n == 1:
        return M[0][0]
    if n == 2:
        return M[0][0] * M[1][1] - M[0][1] * M[1][0]
    return sum((-1) ** j * M[0][j] * det([r[:j] + r[j + 1:] for r in M[1:]]) for j in range(n) if M[0][j])


def volfrac(simplex):
    """Volume of a full-dimensional sub-simplex as a fraction of the parent's."""
    return abs(det([list(v) for v in simplex]))


def clip(simplices, phi, side):
    """The leaves of `simplices` that lie in {side * phi_h >= 0} and have a vertex strictly on that side."""
    out = []
    for S in simplices:
        for leaf, val in split(S, phi):
            if any(v * side > 0 for v in val) and volfrac(leaf) != 0:
                out.append(leaf)
    return out


def region(d, clauses):
    """Leaves of the unit simplex inside every clause; clauses = [(phi vertex values, side = -1 / +1)]."""
    leaves = [unit_simplex(d)]
    for phi, side in clauses:
        leaves = clip(leaves, phi, side)
    return leaves


def interface_faces(d, phi, clauses=()):
    """(d-1)-simplices of {phi_h = 0} inside the unit simplex and inside `clauses`: the faces of the negative
    leaves whose d vertices all have value 0."""
    faces = []
    for S in region(d, clauses):
        for leaf, val in split(S, phi):
            if not any(v < 0 for v in val) or volfrac(leaf) == 0:
                continue
            for sub in itertools.combinations(range(d + 1), d):
                if all(val[i] == 0 for i in sub):
                    faces.append([leaf[i] for i in sub])
    return faces


# ---------------------------------------------------------------------------------------------------------------------
# exact moments
# ---------------------------------------------------------------------------------------------------------------------
def whole_moment(d, alpha):
    """int lambda^alpha over a d-simplex / its measure."""
    return F(math.factorial(d) * math.prod(math.factorial(e) for e in alpha), math.factorial(sum(alpha) + d))


def monomials(nvar, degree, first_zero=False):
    """Exponent tuples of length nvar with total degree <= degree (first_zero: lambda_0 absent, i.e. the monomials
    in the reference coordinates)."""
    return [a for a in itertools.product(range(degree + 1), repeat=nvar)
            if sum(a) <= degree and not (first_zero and a[0])]


@lru_cache(maxsize=None)
def gm_rule(d, s):
    """Grundmann-Moeller rule of index s on the d-simplex, exact for degree 2 s + 1 (SIAM J. Numer. Anal. 15 (1978)):
    levels [(denominator, weight, [odd integer numerators of the barycentric points])], weights normalised to sum 1."""
    levels = []
    for i in range(s + 1):
        den = d + 2 * s + 1 - 2 * i
        w = F((-1) ** i * den ** (2 * s + 1), 2 ** (2 * s) * math.factorial(i) * math.factorial(d + 2 * s + 1 - i))
        pts = [tuple(2 * b + 1 for b in beta) for beta in itertools.product(range(s - i + 1), repeat=d + 1)
               if sum(beta) == s - i]
        levels.append((den, w, pts))
    tot = sum(w * len(p) for _, w, p in levels)
    return [(den, w / tot, pts) for den, w, pts in levels]


def mean_moments(S, alphas, degree):
    """(int_S lambda^alpha) / |S| for a k-simplex S given by k + 1 points in the parent's barycentric coordinates,
    exactly.  Integer arithmetic inside: the points are brought to one denominator, a Grundmann-Moeller point is
    (odd integers) / den, so every monomial is an integer over (den * denominator)^|alpha|."""
    k, nvar = len(S) - 1, len(S[0])
    Dn = 1
    for v in S:
        for x in v:
            Dn = Dn * x.denominator // math.gcd(Dn, x.denominator)
    N = [[int(x * Dn) for x in v] for v in S]
    out = [F(0)] * len(alphas)
    degs = [sum(a) for a in alphas]
    for den, w, pts in gm_rule(k, degree // 2):
        acc = [0] * len(alphas)
        for p in pts:
            pw = []
            for i in range(nvar):
                L = sum(p[j] * N[j][i] for j in range(k + 1))
                row = [1] * (degree + 1)
                for e in range(1, degree + 1):
                    row[e] = row[e - 1] * L
                pw.append(row)
            for a, al in enumerate(alphas):
                m = 1
                for i, e in enumerate(al):
                    if e:
                        m *= pw[i][e]
                acc[a] += m
        base = den * Dn
        powers = [base ** e for e in range(degree + 1)]
        for a in range(len(alphas)):
            if acc[a]:
                out[a] += w * F(acc[a], powers[degs[a]])
    return out


def region_moments(d, clauses, alphas, degree):
    """int lambda^alpha over the region, as a fraction of the parent's measure (alpha = 0: the volume fraction)."""
    out = [F(0)] * len(alphas)
    for leaf in region(d, clauses):
        vf = volfrac(leaf)
        for a, m in enumerate(mean_moments(leaf, alphas, degree)):
            out[a] += vf * m
    return out


# ---------------------------------------------------------------------------------------------------------------------
# physical geometry
# ---------------------------------------------------------------------------------------------------------------------
def frac_rows(x):
    return [[F(float(v)) for v in row] for row in np.asarray(x, dtype=np.float64)]


def measure(points):
    """Measure of the k-simplex with the given physical points (rows of Fractions): the Gram determinant of its edge
    vectors is taken exactly, one square root at the end."""
    k = len(points) - 1
    e = [[a - b for a, b in zip(p, points[0])] for p in points[1:]]
    G = [[sum(a * b for a, b in zip(u, v)) for v in e] for u in e]
    g = det(G) if k else F(1)
    return _sqrt(g) / math.factorial(k)


def _sqrt(q):
    if q <= 0:
        return 0.0
    # scale by an even power of two so that the conversion neither overflows nor underflows
    sh = (q.numerator.bit_length() - q.denominator.bit_length()) // 2 * 2
    q2 = q / F(2) ** sh
    return math.ldexp(math.sqrt(float(q2)), sh // 2) if abs(sh) < 2000 else 0.0


def physical(S, X):
    """Physical points of barycentric points S w.r.t. vertices X (rows of Fractions)."""
    return [[sum(l * X[k][j] for k, l in enumerate(v) if l) for j in range(len(X[0]))] for v in S]


def interface_moments(d, phi, X, alphas, degree, clauses=()):
    """int_{phi_h = 0, inside the clauses} lambda^alpha dS in physical measure (floats, summed with fsum)."""
    terms = [[] for _ in alphas]
    for face in interface_faces(d, phi, clauses):
        area = measure(physical(face, X))
        if area == 0.0:
            continue
        for a, m in enumerate(mean_moments(face, alphas, degree)):
            terms[a].append(area * float(m))
    return [math.fsum(t) for t in terms]


def gradients(X):
    """Physical gradients of the barycentric coordinates of the simplex with vertex rows X (Fractions), exactly:
    rows of the inverse of [[1, x_k]] without its first column; and |det J| / d!."""
    d = len(X) - 1
    A = [[F(1)] + list(X[k][:d]) for k in range(d + 1)]
    D = det(A)
    inv = [[F(0)] * (d + 1) for _ in range(d + 1)]
    for i in range(d + 1):
        for j in range(d + 1):
            minor = [r[:j] + r[j + 1:] for k, r in enumerate(A) if k != i]
            inv[j][i] = (-1) ** (i + j) * det(minor) / D        # inverse = adjugate / det
    # lambda_k(x) = inv[0][k] + sum_a inv[a + 1][k] x_a
    G = [[inv[a + 1][k] for a in range(d)] for k in range(d + 1)]
    return G, abs(D) / math.factorial(d)


NORMAL_FLOOR = 1.0e-14     # the reference divides by max(|grad phi_h|, 1e-14) (level_set/normal.h): a convention


def normal(phi, X):
    """grad phi_h / max(|grad phi_h|, NORMAL_FLOOR) of the cell from exact arithmetic.  Above the floor each
    component is sign * sqrt(g_a^2 / |g|^2), so nothing overflows or underflows on the way."""
    G, _ = gradients(X)
    d = len(X) - 1
    g = [sum(phi[k] * G[k][a] for k in range(d + 1)) for a in range(d)]
    n2 = sum(v * v for v in g)
    floor = F(NORMAL_FLOOR)
    if n2 < floor * floor:
        return [float(v / floor) for v in g]
    return [math.copysign(math.sqrt(float(v * v / n2)), 1.0 if v >= 0 else -1.0) for v in g]


# ---------------------------------------------------------------------------------------------------------------------
# local tensors from the moments (numpy.longdouble from the exact moments)
# ---------------------------------------------------------------------------------------------------------------------
LD = np.longdouble


def _ld(q):
    """Fraction -> longdouble, correctly to ~1e-19 relative."""
    hi = float(q)
    return LD(hi) + LD(float(q - F(hi)))


class Moments:
    """Moments of one region in all barycentric monomials up to degree 4, normalised by the parent's measure."""

    def __init__(self, d, clauses=None):
        self.d = d
        self.alphas = monomials(d + 1, 4)
        if clauses is None:
            vals = [whole_moment(d, a) for a in self.alphas]
        else:
            vals = region_moments(d, clauses, self.alphas, 4)
        self.m = {a: _ld(v) for a, v in zip(self.alphas, vals)}

    def table(self, A, B):
        return np.array([[self.m[tuple(x + y for x, y in zip(a, b))] for b in B] for a in A], dtype=LD)


def _unit(n, *idx):
    a = [0] * n
    for i in idx:
        a[i] += 1
    return tuple(a)


@lru_cache(maxsize=None)
def basis(d, degree):
    """(A, C, A1, D): N_i = sum_p C[i, p] lambda^A[p]; dN_i / dlambda_m = sum_p D[i, m, p] lambda^A1[p].  Degree 2:
    vertex i: lambda_i (2 lambda_i - 1); edge (a, b): 4 lambda_a lambda_b, edges in Basix order."""
    n = d + 1
    A = monomials(n, degree)
    A1 = monomials(n, degree - 1)
    ia, i1 = {a: k for k, a in enumerate(A)}, {a: k for k, a in enumerate(A1)}
    nd = n if degree == 1 else n + len(EDGES[d])
    C = np.zeros((nd, len(A)), dtype=LD)
    D = np.zeros((nd, n, len(A1)), dtype=LD)
    for i in range(n):
        if degree == 1:
            C[i, ia[_unit(n, i)]] = 1
            D[i, i, i1[_unit(n)]] = 1
        else:
            C[i, ia[_unit(n, i, i)]] = 2
            C[i, ia[_unit(n, i)]] = -1
            D[i, i, i1[_unit(n, i)]] = 4
            D[i, i, i1[_unit(n)]] = -1
    if degree == 2:
        for e, (a, b) in enumerate(EDGES[d]):
            C[n + e, ia[_unit(n, a, b)]] = 4
            D[n + e, a, i1[_unit(n, b)]] = 4
            D[n + e, b, i1[_unit(n, a)]] = 4
    return A, C, A1, D


def cell_geometry(xc):
    X = frac_rows(xc)
    G, vol = gradients(X)
    return np.array([[_ld(v) for v in row] for row in G], dtype=LD), _ld(vol)


def mass(mom, xc, degree):
    A, C, _, _ = basis(mom.d, degree)
    _, vol = cell_geometry(xc)
    return (vol * (C @ mom.table(A, A) @ C.T)).astype(np.float64)


def grad_moments(mom, xc, degree):
    """W[i, a, j, b] = int d_a N_i d_b N_j over the region (physical)."""
    _, _, A1, D = basis(mom.d, degree)
    G, vol = cell_geometry(xc)
    T = np.einsum("imp,pq,jnq->imjn", D, mom.table(A1, A1), D)
    return vol * np.einsum("imjn,ma,nb->iajb", T, G, G)


def stiffness(mom, xc, degree):
    return np.einsum("iaja->ij", grad_moments(mom, xc, degree)).astype(np.float64)


def elasticity(mom, xc, degree, E, nu):
    """sigma(u) : eps(v), Lame parameters mu = E / (2 (1 + nu)), lambda = E nu / ((1 + nu) (1 - 2 nu)); entry
    (dof i, component a) at i * bs + a (include/cutfemx_amd.h)."""
    d = mom.d
    mu, lam = LD(E) / (2 * (1 + LD(nu))), LD(E) * LD(nu) / ((1 + LD(nu)) * (1 - 2 * LD(nu)))
    W = grad_moments(mom, xc, degree)                       # [i, a, j, b]
    tr = np.einsum("icjc->ij", W)
    out = lam * W + mu * np.einsum("iajb->ibja", W) + mu * np.einsum("ij,ab->iajb", tr, np.eye(d, dtype=LD))
    nd = W.shape[0]
    return out.reshape(nd * d, nd * d).astype(np.float64)


def source_one(mom, xc, degree, scale=1.0):
    A, C, _, _ = basis(mom.d, degree)
    _, vol = cell_geometry(xc)
    one = [tuple([0] * (mom.d + 1))]
    return (LD(scale) * vol * (C @ mom.table(A, one))[:, 0]).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# selectors and whole cases
# ---------------------------------------------------------------------------------------------------------------------
def parse(selector):
    """'phi<0 and phi1>0' -> [(0, -1), (1, +1)]; '=0' clauses have side 0; <= and >= as < and >."""
    out = []
    for cl in selector.replace(" ", "").split("and"):
        name, op = (cl[:-2], cl[-2]) if cl[-3] not in "<>" else (cl[:-3], cl[-3])
        out.append((0 if name == "phi" else int(name[3:]), {"<": -1, ">": 1, "=": 0}[op]))
    return out


def cell_phi(phis, conn_row):
    return [[F(float(p[v])) for v in conn_row] for p in phis]


def reference_monomials(points, alphas):
    """lambda^alpha at rule points given in reference coordinates: (nq, nalpha)."""
    p = np.asarray(points, dtype=np.float64)
    lam = np.concatenate([1.0 - p.sum(axis=1, keepdims=True), p], axis=1)
    out = np.ones((p.shape[0], len(alphas)))
    for a, al in enumerate(alphas):
        for i, e in enumerate(al):
            if e:
                out[:, a] *= lam[:, i] ** e
    return out


def rule_moments(rules, alphas, nparents, parents=None):
    """sum over the rules of each parent of w * lambda^alpha: (nparents, nalpha)."""
    P = reference_monomials(rules.points, alphas) * np.asarray(rules.weights, dtype=np.float64)[:, None]
    owner = np.repeat(np.asarray(rules.parent_map if parents is None else parents), np.diff(rules.offsets))
    out = np.zeros((nparents, len(alphas)))
    np.add.at(out, owner, P)
    return out


def cell_measures(x, conn, tdim):
    e = x[conn[:, 1:], :tdim] - x[conn[:, :1], :tdim]
    return np.abs(np.linalg.det(e)) / math.factorial(tdim)


_CACHE: dict = {}


def cached(key, fn):
    """Exact values are the cost of these tests: computed once per process and key."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def exact_volume_moments(key, x, conn, phis, cells, selector, degree):
    """(len(cells), nalpha) exact moments of the selector's part of each cell in the monomials of the reference
    coordinates up to `degree`, as fractions of the cell; and the alphas."""
    tdim = conn.shape[1] - 1
    alphas = monomials(tdim + 1, degree, first_zero=True)

    def run():
        out = np.zeros((len(cells), len(alphas)))
        for r, c in enumerate(cells):
            ph = cell_phi(phis, conn[c])
            clauses = [(ph[k], s) for k, s in parse(selector)]
            out[r] = [float(v) for v in region_moments(tdim, clauses, alphas, degree)]
        return out
    return cached(("vol", key, selector, degree), run), alphas


def exact_interface_moments(key, x, conn, phis, cells, selector, degree):
    """The same for a selector with one '=0' clause: physical surface moments."""
    tdim = conn.shape[1] - 1
    alphas = monomials(tdim + 1, degree, first_zero=True)
    cl = parse(selector)
    (k0,) = [k for k, s in cl if s == 0]

    def run():
        out = np.zeros((len(cells), len(alphas)))
        for r, c in enumerate(cells):
            ph = cell_phi(phis, conn[c])
            out[r] = interface_moments(tdim, ph[k0], frac_rows(x[conn[c], :tdim]), alphas, degree,
                                       [(ph[k], s) for k, s in cl if s])
        return out
    return cached(("itf", key, selector, degree), run), alphas


def whole_moments(tdim, alphas):
    return np.array([float(whole_moment(tdim, a)) for a in alphas])


def sign_pattern(phi_row):
    return tuple(int(np.sign(v)) for v in phi_row)


# ---- the shared cases ------------------------------------------------------------------------------------------------
def nasty(phi, seed=3):
    """A quarter of the vertices exactly on the interface, a quarter nearly (1e-13), a quarter at 1e-300 .. 1e-200."""
    rng = np.random.default_rng(seed)
    phi = phi.copy()
    k = rng.integers(0, 4, size=phi.size)
    phi[k == 0] = 0.0
    phi[k == 1] *= 1e-13
    phi[k == 2] = np.sign(phi[k == 2]) * rng.uniform(1e-300, 1e-200, size=int((k == 2).sum()))
    return phi


def second_level_set(x, tdim):
    """The oblique plane of tests/test_gpu_multi_level_set.py."""
    return 0.9 * (x[:, 0] - 0.52) + 0.4 * (x[:, 1] - 0.41) + (0.3 * (x[:, 2] - 0.38) if tdim == 3 else 0.0)


# name: (tdim, n, level set, scrambled, seed of the degenerate values or None, orders compared).  The seeds are chosen
# so that the cells a test may leave out (see build_case) stay under 5 % of the cut cells while each kind occurs.
CASES = {
    "2d-n8-sphere": (2, 8, "sphere", False, None, (0, 1, 2, 3, 4, 5, 6, 7, 8)),
    "3d-n4-sphere": (3, 4, "sphere", False, None, (0, 1, 2, 3, 4, 5, 6, 7, 8)),
    "3d-n4-sphere-scrambled": (3, 4, "sphere", True, None, (2, 5)),
    "3d-n4-degenerate": (3, 4, "sphere", False, 0, (3,)),
    "2d-n7-degenerate-scrambled": (2, 7, "sphere", True, 8, (3, 6)),
    "3d-n5-gyroid": (3, 5, "gyroid", False, None, (4,)),
}


def build_case(O, name):
    """Inputs of a case: mesh arrays from the mesh generator handed in (its arrays are inputs, never expected
    values), level-set values, the cut cells by the definition of DESIGN 1 (not all values < 0, not all > 0).
    `keep`: not all vertex values exactly zero (which side owns a cell with phi_h = 0 is a convention).  `keep_itf`,
    for phi = 0 rules and normals: additionally no whole face on the interface with the cell on the negative side
    (tdim zero vertices and a negative one: whether that face belongs to this cell or to its neighbour is a
    convention; with a positive last vertex there is no interface inside the cell either way, which is compared)."""
    from helpers import level_set_values, scrambled_mesh

    def run():
        tdim, n, kind, scr, deg, orders = CASES[name]
        om = scrambled_mesh(O, tdim, n) if scr else O.mesh_box(tdim, n)
        phi = level_set_values(om.x, tdim, kind)
        if deg is not None:
            phi = nasty(phi, deg)
        v = phi[om.conn]
        cut = np.flatnonzero(~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))).astype(np.int32)
        allzero = np.all(v[cut] == 0, axis=1)
        nzero = (v[cut] == 0).sum(axis=1)
        face_on = (nzero >= tdim) & np.any(v[cut] < 0, axis=1)
        return dict(name=name, tdim=tdim, n=n, scrambled=scr, degenerate=deg is not None, orders=orders, om=om, x=om.x, conn=om.conn,
                    phi=phi, cut=cut, keep=~allzero, keep_itf=~allzero & ~face_on,
                    inside=np.flatnonzero(np.all(v < 0, axis=1)).astype(np.int32))
    return cached(("case", name), run)


def multi_case(O, name):
    """The case with the oblique plane of tests/test_gpu_multi_level_set.py as second level set; `cut` are the
    cells cut by either level set."""
    def run():
        cs = dict(build_case(O, name))
        phi1 = second_level_set(cs["x"], cs["tdim"])
        v = phi1[cs["conn"]]
        cut1 = ~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))
        both = np.zeros(cs["conn"].shape[0], dtype=bool)
        both[cs["cut"]] = True
        cs.update(phis=[cs["phi"], phi1], cut=np.flatnonzero(both | cut1).astype(np.int32))
        return cs
    return cached(("multi", name), run)


def host_vertices(conn, rows):
    """Vertices of the facets given as integration rows (cell, local facet, ...): those of the cell except the one
    opposite the facet, in ascending local index (cut(level_set, facets, tdim - 1) without entity_geometry)."""
    rows = np.asarray(rows)
    nv = conn.shape[1]
    return np.array([[conn[c, k] for k in range(nv) if k != lf] for c, lf in rows[:, :2]], dtype=np.int32)


def host_case(O, name, which):
    """Facet hosts of a case: all interior or all exterior facets as rows, their vertices, the cut ones, their exact
    measures."""
    def run():
        cs = build_case(O, name)
        om, tdim = cs["om"], cs["tdim"]
        rows = O.exterior_facets(om) if which == "exterior" else \
            O.interior_facets_for_cells(om, np.arange(om.ncells, dtype=np.int32))
        hv = host_vertices(cs["conn"], rows)
        v = cs["phi"][hv]
        cut = np.flatnonzero(~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))).astype(np.int32)
        keep = ~np.all(v[cut] == 0, axis=1)
        meas = np.array([measure(frac_rows(cs["x"][hv[h], :tdim])) for h in cut])
        return dict(rows=rows, verts=hv, cut=cut, keep=keep, measure=meas)
    return cached(("hosts", name, which), run)


def cut_moments(key, cs, c, selector="phi<0"):
    """Moments (all barycentric monomials up to degree 4) of the selector's part of cell c, cached."""
    phis = cs.get("phis", [cs["phi"]])
    ph = cell_phi(phis, cs["conn"][c])
    return cached(("mom", key, selector, int(c)), lambda: Moments(cs["tdim"], [(ph[k], s) for k, s in parse(selector)]))


def tensor(kind, mom, xc, degree, params=()):
    if kind == "stiffness":
        return stiffness(mom, xc, degree)
    if kind == "mass":
        return mass(mom, xc, degree)
    if kind == "elasticity":
        return elasticity(mom, xc, degree, *params)
    if kind == "source":
        return source_one(mom, xc, degree, *params)
    raise ValueError(kind)


def interface_scale(x, conn, cells, tdim):
    """h^(tdim - 1), h the longest edge of the cell: no section of a simplex is larger."""
    xc = x[conn[cells]][:, :, :tdim]
    h = np.max([np.linalg.norm(xc[:, i] - xc[:, j], axis=1)
                for i, j in itertools.combinations(range(tdim + 1), 2)], axis=0)
    return h ** (tdim - 1)


def moved_case(O, name, shift=0.013):
    """The case after its level set has moved by `shift` (CutData.update())."""
    def run():
        cs = dict(build_case(O, name))
        phi = cs["phi"] + shift
        v = phi[cs["conn"]]
        cut = np.flatnonzero(~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))).astype(np.int32)
        cs.update(name=name + "-moved", phi=phi, cut=cut, keep=~np.all(v[cut] == 0, axis=1))
        return cs
    return cached(("moved", name), run)


def f32_case(O, name):
    """The case with float32 coordinates and level-set values; `x`, `phi` are the widened float32 inputs, which is
    what the engine computes on."""
    def run():
        cs = dict(build_case(O, name))
        x32, phi32 = cs["x"].astype(np.float32), cs["phi"].astype(np.float32)
        phi = phi32.astype(np.float64)
        v = phi[cs["conn"]]
        cut = np.flatnonzero(~(np.all(v < 0, axis=1) | np.all(v > 0, axis=1))).astype(np.int32)
        cs.update(name=name + "-f32", x32=x32, phi32=phi32, x=x32.astype(np.float64), phi=phi, cut=cut,
                  keep=~np.all(v[cut] == 0, axis=1))
        return cs
    return cached(("f32", name), run)


def exact_entries(key, cs, dofmap, bs, kind, degree, params=(), inside=None):
    """COO entries (rows, cols, values) -- or (rows, values) for kind 'source' -- of the form whose entities are the
    phi<0 rules of every cut cell and, if given, the uncut cells `inside`: exact local tensors scattered with the
    blocked dofmap (dof i, component a at i * bs + a)."""
    tdim = cs["tdim"]
    whole = Moments(tdim)

    def run():
        R, Cc, Vv = [], [], []
        cells = [(c, cut_moments(key, cs, c)) for c in cs["cut"][cs["keep"]]]
        cells += [(c, whole) for c in ([] if inside is None else inside)]
        for c, mom in cells:
            T = tensor(kind, mom, cs["x"][cs["conn"][c], :tdim], degree, params)
            dofs = (np.asarray(dofmap[c], dtype=np.int64)[:, None] * bs + np.arange(bs)[None, :]).ravel()
            if T.ndim == 1:
                if bs != 1:
                    raise ValueError("scalar source only")
                R.append(dofs); Vv.append(T)
            else:
                R.append(np.repeat(dofs, dofs.size)); Cc.append(np.tile(dofs, dofs.size)); Vv.append(T.ravel())
        out = (np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv)) if Cc else (np.concatenate(R), np.concatenate(Vv))
        return out
    return cached(("entries", key, kind, degree, bs, tuple(params), inside is not None), run)
