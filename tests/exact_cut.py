"""Exact rational reference for P1 cuts of simplices: moments of {phi_h < 0}, {phi_h > 0} and {phi_h = 0} inside a
simplex, for one or several level sets and for facet hosts, and the local tensors that follow from the moments: square
and rectangular cell tensors, coefficient-weighted ones, coefficient sources, facet and interface terms, lifting.

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
    """Moments of one region in all barycentric monomials up to `degree` (4: every unweighted built-in; 6: P2 mass
    times a P2 coefficient), normalised by the parent's measure."""

    def __init__(self, d, clauses=None, degree=4):
        self.d, self.degree = d, degree
        self.alphas = monomials(d + 1, degree)
        if clauses is None:
            vals = [whole_moment(d, a) for a in self.alphas]
        else:
            vals = region_moments(d, clauses, self.alphas, degree)
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


# ---- two spaces, coefficient weights, coefficient sources -----------------------------------------------------------
def _diag_blocks(T, bs):
    """The scalar tensor on the diagonal of the bs x bs component blocks: (dof i, component a) at i * bs + a."""
    return T if bs == 1 else np.kron(T, np.eye(bs, dtype=T.dtype))


def rect_tensor(kind, mom, xc, deg0, bs0, deg1, bs1, params=()):
    """Cell tensor between a test space (degree deg0, block size bs0) and a trial space (deg1, bs1) over the region
    of `mom`: [(nd0 bs0) x (nd1 bs1)] row-major, dof-major, component-minor (include/cutfemx_amd.h).
    'mass': C0 M C1^T and 'stiffness' (bs0 == bs1, the scalar block on the component diagonal);
    'div_test': scale d_a N0_i N1_j at row i * tdim + a (bs0 = tdim, bs1 = 1);
    'div_trial': scale N0_i d_b N1_j at column j * tdim + b (bs0 = 1, bs1 = tdim); params = (scale,)."""
    d = mom.d
    A0, C0, B0, D0 = basis(d, deg0)
    A1, C1, B1, D1 = basis(d, deg1)
    G, vol = cell_geometry(xc)
    if kind in ("mass", "stiffness"):
        if bs0 != bs1:
            raise ValueError("mass and stiffness blocks need bs0 == bs1")
        if kind == "mass":
            T = vol * (C0 @ mom.table(A0, A1) @ C1.T)
        else:
            W = np.einsum("imp,pq,jnq->imjn", D0, mom.table(B0, B1), D1)            # the order of `grad_moments`
            T = np.einsum("iaja->ij", vol * np.einsum("imjn,ma,nb->iajb", W, G, G))
        return _diag_blocks(T, bs0).astype(np.float64)
    scale = LD(params[0]) if len(params) else LD(1)
    if kind == "div_test":
        if (bs0, bs1) != (d, 1):
            raise ValueError("div_test: vector test space, scalar trial space")
        T = scale * vol * np.einsum("imp,ma,pq,jq->iaj", D0, G, mom.table(B0, A1), C1)
        return T.reshape(D0.shape[0] * d, C1.shape[0]).astype(np.float64)
    if kind == "div_trial":
        if (bs0, bs1) != (1, d):
            raise ValueError("div_trial: scalar test space, vector trial space")
        T = scale * vol * np.einsum("ip,pq,jnq,nb->ijb", C0, mom.table(A0, B1), D1, G)
        return T.reshape(C0.shape[0], D1.shape[0] * d).astype(np.float64)
    raise ValueError(kind)


def weighted_moments(mom, degree, kappa_cell):
    """The moments of `mom` against kappa = sum_k N_k kappa_cell[k] (N the basis of `degree`): kappa is expanded in the
    barycentric monomials like every other factor, so m'(alpha) = sum_r k_r m(alpha + A[r]) for every alpha that
    leaves room for kappa's degree."""
    A, C, _, _ = basis(mom.d, degree)
    k = np.asarray(kappa_cell, dtype=LD) @ C
    if k.shape != (len(A),):
        raise ValueError("kappa_cell: one value per dof of the cell")
    room = mom.degree - degree
    if room < 0:
        raise ValueError("moments of too low a degree")
    out = {}
    for al in monomials(mom.d + 1, room):
        out[al] = sum((k[r] * mom.m[tuple(x + y for x, y in zip(al, a))] for r, a in enumerate(A) if k[r] != 0), LD(0))
    t = Table(out)
    t.d, t.degree = mom.d, room
    return t


def weighted(kind, mom, xc, degree, kappa_cell, params=()):
    """'mass', 'stiffness' or 'elasticity' with the integrand multiplied by kappa = sum_k N_k kappa_cell[k], kappa in the
    form's own (scalar) element.  `mom` needs degree 3 `degree` (mass) or 3 `degree` - 2."""
    return tensor(kind, weighted_moments(mom, degree, kappa_cell), xc, degree, params)


def source_coeff(mom, xc, degree, w_cell, bs=1, scale=1.0):
    """int f . v with f = sum_j N_j w_cell[j, :]: entry (i, a) at i * bs + a is scale * sum_j M_ij w[j, a], M the exact
    scalar mass tensor."""
    A, C, _, _ = basis(mom.d, degree)
    _, vol = cell_geometry(xc)
    M = vol * (C @ mom.table(A, A) @ C.T)
    w = np.asarray(w_cell, dtype=LD).reshape(C.shape[0], bs)
    return (LD(scale) * (M @ w)).reshape(-1).astype(np.float64)


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
    # the scrambled mesh on which the two cells of most ghost facets differ in diameter (H_CASE of the facet terms)
    "2d-n8-sphere-scrambled": (2, 8, "sphere", True, None, (2, 4)),
    # 1248 P1 extension pairs at threshold 1.0, 333 bad cells on one root (the pair forms)
    "3d-n6-gyroid": (3, 6, "gyroid", False, None, (2,)),
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


def cut_moments(key, cs, c, selector="phi<0", degree=4):
    """Moments (all barycentric monomials up to `degree`) of the selector's part of cell c, cached by the degree too."""
    phis = cs.get("phis", [cs["phi"]])
    ph = cell_phi(phis, cs["conn"][c])
    tag = ("mom", key, selector, int(c)) + (() if degree == 4 else (degree,))
    return cached(tag, lambda: Moments(cs["tdim"], [(ph[k], s) for k, s in parse(selector)], degree))


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


def exact_entries(key, cs, dofmap, bs, kind, degree, params=(), inside=None, trial=None, coefficient=None, mom_degree=4):
    """COO entries (rows, cols, values) -- or (rows, values) for the kinds 'source' and 'source_coeff' -- of the form
    whose entities are the phi<0 rules of every kept cut cell and, if given, the uncut cells `inside`: exact local
    tensors scattered with the blocked dofmap (dof i, component a at i * bs + a).
    trial = (dofmap1, bs1, degree1): a rectangular block (`rect_tensor`), rows by `dofmap` / `bs`, columns by the trial
    space's.  coefficient: the dof values of a Function of the form's space -- kappa (one value per dof) for 'mass',
    'stiffness' and 'elasticity' (`weighted`), the field (bs values per dof) for 'source_coeff' (params = (scale,)).
    mom_degree: the degree of the moments taken (the integrand's, if above 4)."""
    tdim = cs["tdim"]
    co = None if coefficient is None else np.ascontiguousarray(coefficient, dtype=np.float64)

    def local(c, mom):
        xc = cs["x"][cs["conn"][c], :tdim]
        if trial is not None:
            return rect_tensor(kind, mom, xc, degree, bs, trial[2], trial[1], params)
        if kind == "source_coeff":
            return source_coeff(mom, xc, degree, co.reshape(-1, bs)[np.asarray(dofmap[c], dtype=np.int64)], bs, *params)
        if co is not None:
            T = weighted(kind, mom, xc, degree, co[np.asarray(dofmap[c], dtype=np.int64)], params)
        else:
            T = tensor(kind, mom, xc, degree, params)
        return _diag_blocks(T, bs) if kind in ("mass", "stiffness") else T

    def run():
        whole = Moments(tdim, degree=mom_degree)
        R, Cc, Vv = [], [], []
        cells = [(c, cut_moments(key, cs, c, degree=mom_degree)) for c in cs["cut"][cs["keep"]]]
        cells += [(c, whole) for c in ([] if inside is None else inside)]
        for c, mom in cells:
            T = local(c, mom)
            dofs = _blocked(dofmap[c], bs)
            if T.ndim == 1:
                if T.size != dofs.size:
                    raise ValueError("scalar source only")
                R.append(dofs); Vv.append(T)
            else:
                cols = dofs if trial is None else _blocked(trial[0][c], trial[1])
                R.append(np.repeat(dofs, cols.size)); Cc.append(np.tile(cols, dofs.size)); Vv.append(T.ravel())
        out = (np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv)) if Cc else (np.concatenate(R), np.concatenate(Vv))
        return out
    tag = ("entries", key, kind, degree, bs, tuple(params), inside is not None,
           np.ascontiguousarray(dofmap, dtype=np.int64).tobytes())
    if trial is not None or co is not None or mom_degree != 4:
        tag += (None if trial is None else (np.ascontiguousarray(trial[0], dtype=np.int64).tobytes(), trial[1], trial[2]),
                None if co is None else co.tobytes(), mom_degree)
    if inside is not None:
        tag += (np.ascontiguousarray(inside, dtype=np.int64).tobytes(),)
    return cached(tag, run)


def exact_lift(entries, shape, markers1, g, x0, alpha, b0):
    """b0 - A_exact @ where(marked, alpha (g - x0), 0) for A_exact given as COO `entries` of `shape`, accumulated in
    longdouble and rounded once; and the scale of the comparison, max(abs(b0) + abs(A_exact) @ abs(alpha (g - x0)))."""
    r, c, v = entries
    g = np.asarray(g, dtype=LD)
    y = LD(alpha) * (g - (0 if x0 is None else np.asarray(x0, dtype=LD)))
    y = np.where(np.asarray(markers1) != 0, y, LD(0))
    if y.shape != (shape[1],) or np.shape(b0) != (shape[0],):
        raise ValueError("lifting takes trial-space data and a test-space vector")
    out, mag = np.asarray(b0, dtype=LD).copy(), np.abs(np.asarray(b0, dtype=LD))
    t = np.asarray(v, dtype=LD) * y[c]
    np.subtract.at(out, r, t)
    np.add.at(mag, r, np.abs(t))
    return out.astype(np.float64), float(mag.max())


# ---------------------------------------------------------------------------------------------------------------------
# facet and interface terms: Nitsche, ghost penalty, value jump, symmetric interior penalty
# ---------------------------------------------------------------------------------------------------------------------
# The one convention (include/cutfemx_amd.h): h of a cell is its largest vertex-to-vertex distance, h_avg of an interior
# facet the arithmetic mean of its two cells' h.  Everything else is a polynomial integral over a whole facet, the
# phi_h < 0 part of a facet, or the planar piece of {phi_h = 0} inside a cell.
def _sqrt_ld(q):
    """sqrt of a positive Fraction in longdouble."""
    return np.sqrt(_ld(q)) if q > 0 else LD(0)


def cell_diameter(X):
    """Largest vertex-to-vertex distance of the simplex with vertex rows X (Fractions): the largest squared distance
    exactly, one square root at the end."""
    return _sqrt_ld(max(sum((a - b) ** 2 for a, b in zip(p, q)) for p, q in itertools.combinations(X, 2)))


class Table:
    """Moments keyed by exponent tuples (what `Moments` holds, from any source)."""

    def __init__(self, m):
        self.m = m

    def table(self, A, B):
        return np.array([[self.m[tuple(x + y for x, y in zip(a, b))] for b in B] for a in A], dtype=LD)

    def scaled(self, s):
        return Table({a: LD(s) * v for a, v in self.m.items()})


def centroid_moments(d):
    """The functional of the one-point rule: a rule with one point that integrates degree 1 exactly is the centroid with
    the whole measure as weight, so its 'moment' of lambda^alpha is (1 / (d + 1))^abs(alpha)."""
    return Table({a: _ld(F(1, (d + 1) ** sum(a))) for a in monomials(d + 1, 4)})


def facet_match(conn, row):
    """Vertices of the facet of an interior-facet row (c0, lf0, c1, lf1) -- those of cell 0 without the one opposite,
    in ascending local index -- and, for either cell, the facet's index of each local vertex (None opposite the
    facet), matched through the two connectivity rows."""
    c0, lf0, c1, lf1 = (int(v) for v in row)
    nv = conn.shape[1]
    verts = [int(conn[c0, k]) for k in range(nv) if k != lf0]
    pos = {v: i for i, v in enumerate(verts)}
    if len(pos) != nv - 1 or int(conn[c1, lf1]) in pos or int(conn[c0, lf0]) in pos:
        raise ValueError("not an interior-facet row")
    maps = [tuple(None if k == lf else pos[int(conn[c, k])] for k in range(nv)) for c, lf in ((c0, lf0), (c1, lf1))]
    return verts, maps


@lru_cache(maxsize=None)
def _restriction(d, degree, vmap):
    """R[p, q] = 1 where the cell's barycentric monomial p, restricted to the facet, is the facet's monomial q: the
    coordinate opposite the facet is 0 (a monomial that holds it vanishes), the others are the facet's own."""
    A, Af = monomials(d + 1, degree), monomials(d, degree)
    idx = {a: k for k, a in enumerate(Af)}
    R = np.zeros((len(A), len(Af)), dtype=LD)
    for p, a in enumerate(A):
        b = [0] * d
        for k, e in enumerate(a):
            if e and vmap[k] is None:
                break
            if e:
                b[vmap[k]] += e
        else:
            R[p, idx[tuple(b)]] = 1
    return R


class FacetBasis:
    """The macro basis [cell 0 dofs, cell 1 dofs] on an interior facet as polynomials in the facet's barycentric
    coordinates: values `val[s]` (nd x monomials of `degree`) and derivatives along the unit normal of cell 0
    (-grad lambda_lf0 of cell 0, rational up to one square root) `dn[s]` (nd x monomials of degree - 1); the
    facet's measure and the two cell diameters."""

    def __init__(self, x, conn, row, degree):
        d = conn.shape[1] - 1
        self.d, self.degree = d, degree
        self.verts, maps = facet_match(conn, row)
        cells = (int(row[0]), int(row[2]))
        Xs = [frac_rows(x[conn[c], :d]) for c in cells]
        Gs = [gradients(X)[0] for X in Xs]
        nvec = [-g for g in Gs[0][int(row[1])]]
        nlen = _sqrt_ld(sum(g * g for g in nvec))
        self.normal = np.array([_ld(g) for g in nvec], dtype=LD) / nlen
        self.h = [cell_diameter(X) for X in Xs]
        self.havg = (self.h[0] + self.h[1]) / 2
        self.area = LD(measure(frac_rows(x[self.verts, :d])))
        self.Af, self.Af1 = monomials(d, degree), monomials(d, degree - 1)
        _, C, _, D = basis(d, degree)
        self.val, self.dn = [], []
        for s in range(2):
            g = np.array([_ld(sum(a * b for a, b in zip(Gs[s][m], nvec))) for m in range(d + 1)], dtype=LD) / nlen
            self.val.append(C @ _restriction(d, degree, maps[s]))
            self.dn.append(np.einsum("imp,m,pq->iq", D, g, _restriction(d, degree - 1, maps[s])))

    def jump(self):
        return np.concatenate([self.val[0], -self.val[1]])

    def dn_jump(self):
        return np.concatenate([self.dn[0], -self.dn[1]])

    def dn_avg(self):
        return np.concatenate([self.dn[0], self.dn[1]]) / 2


def facet_tensor(kind, fb, mom, params, bs=1):
    """Local tensor of an interior-facet term over the part of the facet whose moments (normalised by the facet's
    measure) are `mom`, in longdouble; macro dof i, component k at i * bs + k.
    'ghost': gamma h_avg^(1 + e) [dn u][dn v], params (gamma, e); 'jump': gamma / h_avg [u][v];
    'sip': -{dn u}[v] - {dn v}[u] + sigma / h_avg [u][v]; 'sip-penalty': the last term alone."""
    jv, jn, an = fb.jump(), fb.dn_jump(), fb.dn_avg()
    if kind == "ghost":
        gamma, e = (tuple(params) + (0.0,))[:2]
        T = LD(gamma) * fb.havg ** (1 + int(e)) * (jn @ mom.table(fb.Af1, fb.Af1) @ jn.T)
    elif kind in ("jump", "sip-penalty"):
        T = LD(params[0]) / fb.havg * (jv @ mom.table(fb.Af, fb.Af) @ jv.T)
    elif kind == "sip":
        B = jv @ mom.table(fb.Af, fb.Af1) @ an.T                  # B[i, j] = int [N_i] {dn N_j}
        T = -B - B.T + LD(params[0]) / fb.havg * (jv @ mom.table(fb.Af, fb.Af) @ jv.T)
    else:
        raise ValueError(kind)
    T = fb.area * T
    return T if bs == 1 else np.kron(T, np.eye(bs, dtype=LD))


def facet_tensor2(kind, fb0, fb1, mom, params):
    """Local tensor of an interior-facet term between two scalar spaces on one facet row: rows from the test basis
    `fb0`, columns from the trial basis `fb1` (`FacetBasis` objects of the two degrees), over the part of the facet
    whose normalised moments are `mom`, in longdouble.  'ghost': gamma h_avg^(1 + e) [dn u][dn v], 'jump':
    gamma / h_avg [u][v]; h_avg as in `facet_tensor`."""
    if fb0.verts != fb1.verts:
        raise ValueError("two bases of one facet row")
    if kind == "ghost":
        gamma, e = (tuple(params) + (0.0,))[:2]
        T = LD(gamma) * fb0.havg ** (1 + int(e)) * (fb0.dn_jump() @ mom.table(fb0.Af1, fb1.Af1) @ fb1.dn_jump().T)
    elif kind == "jump":
        T = LD(params[0]) / fb0.havg * (fb0.jump() @ mom.table(fb0.Af, fb1.Af) @ fb1.jump().T)
    else:
        raise ValueError(kind)
    return fb0.area * T


def facet_dofs(fb, poly, x, conn, row, degree):
    """Macro dof vector [cell 0, cell 1] of the functions poly[s](point) on the two cells (nodal values: vertices,
    then edge midpoints in Basix order)."""
    d = conn.shape[1] - 1
    out = []
    for s, c in enumerate((int(row[0]), int(row[2]))):
        X = frac_rows(x[conn[c], :d])
        pts = list(X)
        if degree == 2:
            pts += [[(p + q) / 2 for p, q in zip(X[a], X[b])] for a, b in EDGES[d]]
        out += [poly[s](p) for p in pts]
    return np.array([_ld(F(v)) for v in out], dtype=LD)


def interior_facet_rows(conn, cells=None):
    """All interior facets (both cells in `cells`, if given) as rows (c0, lf0, c1, lf1), c0 < c1, ascending."""
    nv = conn.shape[1]
    ok = None if cells is None else set(int(c) for c in cells)
    seen = {}
    for c in range(conn.shape[0]):
        if ok is not None and c not in ok:
            continue
        for lf in range(nv):
            seen.setdefault(tuple(sorted(int(conn[c, k]) for k in range(nv) if k != lf)), []).append((c, lf))
    rows = sorted(v[0] + v[1] for v in seen.values() if len(v) == 2)
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def ghost_facets(cs):
    """The ghost-penalty facets of `phi<0` from the inputs alone: interior facets with at least one intersected cell
    whose other cell is intersected or inside; rows ascending.  Intersected: not all values < 0 and not all > 0."""
    cut, inside = set(cs["cut"].tolist()), set(cs["inside"].tolist())
    rows = interior_facet_rows(cs["conn"])
    keep = [(r[0] in cut or r[2] in cut) and all(c in cut or c in inside for c in (r[0], r[2])) for r in rows.tolist()]
    return rows[np.array(keep, dtype=bool)]


def facet_phi(cs, verts):
    return [F(float(cs["phi"][v])) for v in verts]


def facet_moments(key, cs, fb, side=-1):
    """Moments of the side * phi_h > 0 part of the facet, normalised by the facet's measure (clipping one dimension
    down, as for facet hosts), cached by the facet's vertices."""
    return cached(("fmom", key, tuple(fb.verts), side),
                  lambda: Moments(cs["tdim"] - 1, [(facet_phi(cs, fb.verts), side)]))


def facet_basis(key, cs, row, degree):
    return cached(("fbasis", key, tuple(int(v) for v in row), degree), lambda: FacetBasis(cs["x"], cs["conn"], row, degree))


class Interface:
    """The planar piece of {phi_h = 0} inside cell c: physical surface moments of all barycentric monomials up to
    degree 4, the unit normal (with the recorded floor), the cell's diameter and lambda gradients."""

    def __init__(self, cs, c):
        d = cs["tdim"]
        X = frac_rows(cs["x"][cs["conn"][c], :d])
        phi = cell_phi(cs.get("phis", [cs["phi"]]), cs["conn"][c])[0]
        al = monomials(d + 1, 4)
        self.d = d
        self.mom = Table({a: LD(v) for a, v in zip(al, interface_moments(d, phi, X, al, 4))})
        self.normal = np.array(normal(phi, X), dtype=LD)
        self.h = cell_diameter(X)
        self.G, _ = cell_geometry(cs["x"][cs["conn"][c], :d])
        # the same term with the whole cell's normalised moments times h^(tdim - 1) in place of the surface's: its scale
        self.whole = Table({a: _ld(whole_moment(d, a)) for a in al}).scaled(self.h ** (d - 1))


def interface(key, cs, c):
    return cached(("itf-cell", key, int(c)), lambda: Interface(cs, c))


def nitsche(itf, degree, gamma, mom=None):
    """-dn(u) v - dn(v) u + gamma / h u v over the interface piece (longdouble)."""
    mom = itf.mom if mom is None else mom
    A, C, A1, D = basis(itf.d, degree)
    Dn = np.einsum("imp,m->ip", D, itf.G @ itf.normal)
    B = C @ mom.table(A, A1) @ Dn.T                               # B[i, j] = int N_i dn N_j
    return -B - B.T + LD(gamma) / itf.h * (C @ mom.table(A, A) @ C.T)


def nitsche_rhs(itf, degree, gamma, scale=1.0, mom=None):
    """-dn(v) g + gamma / h g v with the constant datum g = scale."""
    mom = itf.mom if mom is None else mom
    A, C, A1, D = basis(itf.d, degree)
    Dn = np.einsum("imp,m->ip", D, itf.G @ itf.normal)
    one = [tuple([0] * (itf.d + 1))]
    return LD(scale) * (-(Dn @ mom.table(A1, one))[:, 0] + LD(gamma) / itf.h * (C @ mom.table(A, one))[:, 0])


def _blocked(dofs, bs):
    return (np.asarray(dofs, dtype=np.int64)[:, None] * bs + np.arange(bs)[None, :]).ravel()


def exact_facet_entries(key, cs, dofmap, bs, kind, degree, params, rows, cut_rows=(), one_point=False):
    """COO entries of an interior-facet term over the whole facets `rows` and the phi<0 parts of `cut_rows`, scattered
    with the blocked dofmap of the two cells.  one_point: the value of the one-point rule instead of the integral."""
    d = cs["tdim"]
    whole = centroid_moments(d - 1) if one_point else Moments(d - 1)

    def run():
        R, Cc, Vv = [], [], []
        for part, rr in ((False, rows), (True, cut_rows)):
            for row in np.asarray(rr).reshape(-1, 4):
                fb = facet_basis(key, cs, row, degree)
                T = facet_tensor(kind, fb, facet_moments(key, cs, fb) if part else whole, params, bs).astype(np.float64)
                dofs = _blocked(np.concatenate([dofmap[row[0]], dofmap[row[2]]]), bs)
                R.append(np.repeat(dofs, dofs.size)); Cc.append(np.tile(dofs, dofs.size)); Vv.append(T.ravel())
        return np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv)
    tag = tuple(np.ascontiguousarray(a, dtype=np.int64).tobytes() for a in (rows, cut_rows, dofmap))
    return cached(("fentries", key, kind, degree, bs, tuple(params), one_point, tag), run)


def exact_facet_entries2(key, cs, dofmap0, degree0, dofmap1, degree1, kind, params, rows):
    """COO entries of an interior-facet term between two scalar spaces over the whole facets `rows`: rows by the test
    space's dofs of the two cells, columns by the trial space's."""
    whole = Moments(cs["tdim"] - 1)

    def run():
        R, Cc, Vv = [], [], []
        for row in np.asarray(rows).reshape(-1, 4):
            fb0, fb1 = facet_basis(key, cs, row, degree0), facet_basis(key, cs, row, degree1)
            T = facet_tensor2(kind, fb0, fb1, whole, params).astype(np.float64)
            d0 = np.concatenate([dofmap0[row[0]], dofmap0[row[2]]]).astype(np.int64)
            d1 = np.concatenate([dofmap1[row[0]], dofmap1[row[2]]]).astype(np.int64)
            R.append(np.repeat(d0, d1.size)); Cc.append(np.tile(d1, d0.size)); Vv.append(T.ravel())
        return np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv)
    tag = tuple(np.ascontiguousarray(a, dtype=np.int64).tobytes() for a in (rows, dofmap0, dofmap1))
    return cached(("fentries2", key, kind, degree0, degree1, tuple(params), tag), run)


def exact_nitsche_entries(key, cs, dofmap, degree, gamma, rhs_scale=None):
    """COO entries of the Nitsche matrix (rhs_scale None) or of the g = rhs_scale Nitsche vector over the kept cut
    cells (`keep_itf`)."""
    def run():
        R, Cc, Vv = [], [], []
        for c in cs["cut"][cs["keep_itf"]]:
            itf = interface(key, cs, c)
            dofs = np.asarray(dofmap[c], dtype=np.int64)
            if rhs_scale is None:
                T = nitsche(itf, degree, gamma).astype(np.float64)
                R.append(np.repeat(dofs, dofs.size)); Cc.append(np.tile(dofs, dofs.size)); Vv.append(T.ravel())
            else:
                R.append(dofs); Vv.append(nitsche_rhs(itf, degree, gamma, rhs_scale).astype(np.float64))
        return (np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv)) if Cc else (np.concatenate(R), np.concatenate(Vv))
    return cached(("nentries", key, degree, gamma, rhs_scale, np.ascontiguousarray(dofmap, dtype=np.int64).tobytes()), run)


# ---- the facet cases ---------------------------------------------------------------------------------------------------
# On the generated Kuhn boxes every cell has the same diameter, so h0, h1, (h0 + h1) / 2 and max(h0, h1) agree there;
# only a scrambled mesh tells them apart.  H_CASE is the one on which abs(h0 - h1) > 0.05 h_avg holds on more than half
# of the ghost facets (asserted from the inputs).  In 3-D the six tetrahedra of a Kuhn cube share its body diagonal, which
# stays their longest edge after the scramble, so at most the facets between two cubes -- half of all -- can differ and
# about a quarter do by more than 5 %: the 3-D scrambled case is compared as well, the assertion is made on H_CASE.
FACET_CASES = ["2d-n8-sphere", "3d-n4-sphere", "3d-n4-sphere-scrambled", "2d-n7-degenerate-scrambled", "2d-n8-sphere-scrambled"]
H_CASE = "2d-n8-sphere-scrambled"


def facet_case(O, name):
    """Facet entities of a case from its inputs alone.  ghost: rows; skeleton: all interior facets, the ones inside
    (every facet vertex < 0: whole facets), the cut ones (neither all < 0 nor all > 0: phi<0 parts); `*_keep`: what
    is compared -- not facets whose vertex values are all exactly zero (as `host_case`), nor facets both of whose
    cells are all-zero cells; h: (h0, h1) of every ghost facet."""
    def run():
        cs = build_case(O, name)
        conn, phi = cs["conn"], cs["phi"]
        allzero = np.all(phi[conn] == 0, axis=1)
        rows = interior_facet_rows(conn)
        v = phi[host_vertices(conn, rows)]
        neg, pos = np.all(v < 0, axis=1), np.all(v > 0, axis=1)
        both0 = allzero[rows[:, 0]] & allzero[rows[:, 2]]
        ghost = ghost_facets(cs)
        cutset = set(cs["cut"].tolist())
        kinds = np.array([(r[0] in cutset) + (r[2] in cutset) for r in ghost.tolist()])
        h = np.array([[float(cell_diameter(frac_rows(cs["x"][conn[c], :cs["tdim"]]))) for c in (r[0], r[2])] for r in ghost])
        return dict(rows=rows, inside=rows[neg], cut=rows[~neg & ~pos], cut_keep=(~np.all(v == 0, axis=1) & ~both0)[~neg & ~pos],
                    inside_keep=~both0[neg], ghost=ghost, ghost_keep=~(allzero[ghost[:, 0]] & allzero[ghost[:, 2]]),
                    n_cut_cut=int((kinds == 2).sum()), n_cut_inside=int((kinds == 1).sum()), h=h)
    return cached(("facets", name), run)


# ---------------------------------------------------------------------------------------------------------------------
# extension penalty: the (bad, root) pair block, and the volume fractions that decide which cells are roots
# ---------------------------------------------------------------------------------------------------------------------
# beta int_{K_bad} M_i M_j with M = [N_bad, -(N_root o F_root^-1)]: the root's basis functions are polynomials of the
# physical point and are taken on the bad cell, outside the root.  The root's barycentric coordinates are an affine,
# rational function of the bad cell's, so at the rational Grundmann-Moeller points of the bad cell every factor is a
# rational number and the rule of index s, 2 s + 1 >= 2 degree, gives the integral itself.
def root_coordinates(Xb, Xr):
    """(P, D): lambda_k of the simplex Xr at vertex v of the simplex Xb is P[v][k] / D (Cramer's rule on
    sum_k lambda_k (1, x_k) = (1, p)); rows of Fractions."""
    A = [[F(1)] + list(r) for r in Xr]
    P = [[det(A[:k] + [[F(1)] + list(p)] + A[k + 1:]) for k in range(len(Xr))] for p in Xb]
    return P, det(A)


def _basis_numerators(n, Q, d, degree):
    """Numerators of the nodal basis over Q^degree at the point with barycentric coordinates n / Q (integers)."""
    if degree == 1:
        return list(n)
    return [v * (2 * v - Q) for v in n] + [4 * n[a] * n[b] for a, b in EDGES[d]]


def pair_tensor_exact(x, conn, tdim, degree, bad, root, beta=1):
    """The scalar (2 ND)^2 pair block as Fractions (rows of a list), layout [[bad bad, bad root], [root bad, root root]].
    Integer arithmetic inside: float64 inputs are dyadic, so one power of two clears P and D of `root_coordinates`; at
    a Grundmann-Moeller point (odd integers) / den the bad cell's coordinates are integers over den and the root's are
    integers over den * D."""
    d = tdim
    Xb, Xr = frac_rows(x[conn[bad], :d]), frac_rows(x[conn[root], :d])
    P, D = root_coordinates(Xb, Xr)
    if D == 0:
        raise ValueError("degenerate root cell")
    two = max([D.denominator] + [v.denominator for row in P for v in row])
    Pi, Di = [[int(v * two) for v in row] for row in P], int(D * two)
    s = degree
    assert 2 * s + 1 >= 2 * degree
    nd = len(_basis_numerators([0] * (d + 1), 1, d, degree))
    T = [[F(0)] * (2 * nd) for _ in range(2 * nd)]
    for den, w, pts in gm_rule(d, s):
        Q = (den, den * Di)
        S = [[0] * (2 * nd) for _ in range(2 * nd)]
        for p in pts:
            nr = [sum(p[v] * Pi[v][k] for v in range(d + 1)) for k in range(d + 1)]
            M = _basis_numerators(list(p), Q[0], d, degree) + [-v for v in _basis_numerators(nr, Q[1], d, degree)]
            for i in range(2 * nd):
                if M[i]:
                    Si, Mi = S[i], M[i]
                    for j in range(i, 2 * nd):
                        Si[j] += Mi * M[j]
        for i in range(2 * nd):
            for j in range(i, 2 * nd):
                if S[i][j]:
                    T[i][j] += w * F(S[i][j], (Q[i >= nd] * Q[j >= nd]) ** degree)
    vol = abs(det([[F(1)] + list(r) for r in Xb])) / math.factorial(d)
    scale = vol * F(beta)
    for i in range(2 * nd):
        for j in range(i, 2 * nd):
            T[i][j] = T[j][i] = scale * T[i][j]
    return T


def pair_tensor(x, conn, tdim, degree, bad, root, beta, bs=1, dtype=np.float64):
    """beta int_{K_bad} M_i M_j, M = [N_bad, -(N_root o F_root^-1)], as the (2 ND bs)^2 macro tensor of an
    interior-facet-type entity (include/cutfemx_amd.h): [[00, 01], [10, 11]], (dof i, component a) at i * bs + a, equal
    components only.  Fractions of the float64 inputs (beta included) until the one rounding through `_ld`."""
    T = np.array([[_ld(v) for v in row] for row in pair_tensor_exact(x, conn, tdim, degree, bad, root, F(float(beta)))], dtype=LD)
    return (T if bs == 1 else np.kron(T, np.eye(bs, dtype=LD))).astype(dtype)


def unit_pair_tensor(key, cs, degree, bad, root):
    """The scalar pair block with beta = 1 in longdouble, cached per pair."""
    return cached(("pair", key, degree, int(bad), int(root)),
                  lambda: pair_tensor(cs["x"], cs["conn"], cs["tdim"], degree, int(bad), int(root), 1.0, dtype=LD))


def pair_block_scales(T, nd):
    """sqrt(max|T_aa| max|T_bb|) for the four blocks (a, b) of a macro tensor with nd rows per cell: the block-wise scale
    of a pair comparison (for a far pair the root x root block is 10^4 to 10^5 times the bad x bad one)."""
    A = np.abs(np.asarray(T, dtype=np.float64))
    top = [A[:nd, :nd].max(), A[nd:, nd:].max()]
    S = np.empty_like(A)
    for a in (0, 1):
        for b in (0, 1):
            S[a * nd:(a + 1) * nd, b * nd:(b + 1) * nd] = math.sqrt(top[a] * top[b])
    return S


def exact_pair_entries(key, cs, dofmap, bs, degree, pairs, beta, beta_cell=None):
    """(rows, cols, values, scales) of the assembled pair form, one entry per (row, column), rows then columns
    ascending: values = the sum of beta (x beta_cell[bad]) x the exact pair blocks scattered with the blocked dofmap of
    (bad, root), accumulated in longdouble and rounded once; scales = the sum of the absolute values of the same
    contributions.  An entry all of whose contributions are exactly zero (the P2 mass of a vertex and an adjacent edge
    function in the bad x bad block) has no such scale: there the scale is the sum of the block scales of
    `pair_block_scales`, which is what the comparison of the pair tensors themselves allows those entries."""
    pairs = np.asarray(pairs).reshape(-1, 4)
    bc = None if beta_cell is None else np.ascontiguousarray(beta_cell, dtype=np.float64)

    def run():
        nd = np.asarray(dofmap).shape[1]
        n = 2 * nd
        R, Cc, Vv, Zz = [], [], [], []
        for bad, _, root, _ in pairs.tolist():
            T = unit_pair_tensor(key, cs, degree, bad, root) * (LD(beta) * (LD(1) if bc is None else LD(bc[bad])))
            dofs = np.concatenate([dofmap[bad], dofmap[root]]).astype(np.int64)
            R.append(np.repeat(dofs, n)); Cc.append(np.tile(dofs, n)); Vv.append(T.ravel())
            Zz.append(np.where(T == 0, pair_block_scales(T, nd), 0.0).ravel())
        if not R:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
        r, c, v, z = np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv), np.concatenate(Zz)
        order = np.lexsort((c, r))
        r, c, v, z = r[order], c[order], v[order], z[order]
        first = np.flatnonzero(np.r_[True, (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
        s = np.add.reduceat(np.abs(v), first).astype(np.float64)
        r, c, v = r[first], c[first], np.add.reduceat(v, first).astype(np.float64)
        s = np.where(s > 0, s, np.add.reduceat(z, first))
        # (dof i, component a) at i * bs + a, equal components only; rows then columns ascending again
        r, c = (r[:, None] * bs + np.arange(bs)).ravel(), (c[:, None] * bs + np.arange(bs)).ravel()
        v, s = np.repeat(v, bs), np.repeat(s, bs)
        order = np.lexsort((c, r))
        return r[order], c[order], v[order], s[order]
    tag = ("pentries", key, degree, bs, float(beta), None if bc is None else bc.tobytes(), pairs.tobytes(),
           np.ascontiguousarray(dofmap, dtype=np.int64).tobytes())
    return cached(tag, run)


def exact_fraction(cs, c, selector):
    """Volume of the selector's part of cell c over the cell's volume, as a Fraction (0 <= . <= 1)."""
    ph = cell_phi(cs.get("phis", [cs["phi"]]), cs["conn"][c])
    return sum((volfrac(leaf) for leaf in region(cs["tdim"], [(ph[k], s) for k, s in parse(selector)])), F(0))


def exact_fractions(key, cs, selector):
    """`exact_fraction` of every cut cell of the case as float64 (each rounded once), cached."""
    sel = selector.replace(" ", "")
    return cached(("fractions", key, sel), lambda: np.array([float(exact_fraction(cs, c, sel)) for c in cs["cut"]]))


def shared_vertices(conn, pairs):
    """Number of vertices the two cells of each pair share."""
    pairs = np.asarray(pairs).reshape(-1, 4)
    return np.array([len(set(conn[b].tolist()) & set(conn[r].tolist())) for b, r in pairs[:, [0, 2]].tolist()], dtype=np.int64)


def longest_pair_row(dofmap, bs, pairs, ndofs):
    """Longest row (in scalar columns) of the pair form's sparsity with the all-rows diagonal, from pairs and dofmap."""
    import scipy.sparse as sp
    pairs = np.asarray(pairs).reshape(-1, 4)
    dm = np.asarray(dofmap, dtype=np.int64)
    macro = np.concatenate([dm[pairs[:, 0]], dm[pairs[:, 2]]], axis=1)
    n = macro.shape[1]
    r, c = np.repeat(macro, n, axis=1).ravel(), np.tile(macro, (1, n)).ravel()
    r, c = np.concatenate([r, np.arange(ndofs)]), np.concatenate([c, np.arange(ndofs)])
    A = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(ndofs, ndofs)).tocsr()
    return int(np.diff(A.indptr).max()) * bs
