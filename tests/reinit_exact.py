"""References for the cell-local arithmetic of the reinitialisation that share no formulation with the engine
(cutfemx_amd/csrc/cfx_reinit_cell.h) or with its numpy model (tests/reinit_ref.py):

brute_update  the update U(t, K) as what it is defined to be, the minimum of F(lambda) = sum lambda_s d_s + |sum lambda_s P_s|
              over the convex hull of the usable sources, found by a nested golden-section search in long double.  F is
              convex, so the search converges to the global minimum; no Gram matrix, no multipliers, no case split.
mp_update     the same search in mpmath, for pinning brute_update on a sample.
exact_seed    the near field of one cell: the crossing points as exact rationals of the float inputs, the distance of
              every vertex to their convex hull by Voronoi regions in exact arithmetic, the square root last.

tests/test_reinit_cell_reference.py pins all three to mathematics."""
from __future__ import annotations

from fractions import Fraction
from itertools import combinations

import numpy as np

LD = np.longdouble
INF = 1e30
_G = (np.sqrt(LD(5)) - 1) / 2
ITERATIONS = 64


# ---- the update ---------------------------------------------------------------------------------------------------------
def _golden(f, lo, hi, iterations=ITERATIONS):
    """min of the unimodal f over [lo, hi], elementwise; the end points are evaluated explicitly"""
    a, b = lo.copy(), hi.copy()
    c, d = b - _G * (b - a), a + _G * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iterations):
        left = fc < fd                                     # the minimum lies in [a, d], else in [c, b]
        a, b = np.where(left, a, c), np.where(left, d, b)
        x = np.where(left, b - _G * (b - a), a + _G * (b - a))
        fx = f(x)
        c, d, fc, fd = np.where(left, x, d), np.where(left, c, x), np.where(left, fx, fd), np.where(left, fc, fx)
    return np.minimum(np.minimum(fc, fd), np.minimum(f(lo), f(hi)))


def _norm(w):
    return np.sqrt(np.sum(w * w, axis=1))


def brute_update(P, dv, ok, inf=INF):
    """U of m (target, cell) pairs as long doubles: P[m, k, dim] = x_s - x_t, dv[m, k], ok[m, k]; k = 2 or 3.  Every
    vertex, every edge and (k = 3) the triangle of usable sources is searched on its own and the least value taken: the
    pieces overlap, which costs time and nothing else."""
    P, dv, ok = np.asarray(P).astype(LD), np.asarray(dv).astype(LD), np.asarray(ok, dtype=bool)
    m, k, _ = P.shape
    # the lambda sum to 1, so a constant added to every d_s is added to F: search with the values of the cell's own
    # size (the search cannot place the minimum better than the rounding of F allows) and add the constant at the end
    shift = np.where(ok.any(axis=1), dv[np.arange(m), np.argmax(ok, axis=1)], LD(0))
    dv = dv - shift[:, None]
    best = np.full(m, LD(inf))
    for i in range(k):
        rows = np.nonzero(ok[:, i])[0]
        best[rows] = np.minimum(best[rows], dv[rows, i] + _norm(P[rows, i]))
    for i, j in combinations(range(k), 2):
        rows = np.nonzero(ok[:, i] & ok[:, j])[0]
        if rows.size == 0:
            continue
        A, B, da, db = P[rows, i], P[rows, j], dv[rows, i], dv[rows, j]
        f = lambda u: (1 - u) * da + u * db + _norm((1 - u)[:, None] * A + u[:, None] * B)
        best[rows] = np.minimum(best[rows], _golden(f, np.zeros(rows.size, LD), np.ones(rows.size, LD)))
    if k == 3:
        rows = np.nonzero(ok.all(axis=1))[0]
        if rows.size:
            A, B, C, d = P[rows, 0], P[rows, 1], P[rows, 2], dv[rows]
            zero = np.zeros(rows.size, LD)

            def F(u, v):
                w = 1 - u - v
                return w * d[:, 0] + u * d[:, 1] + v * d[:, 2] + _norm(w[:, None] * A + u[:, None] * B + v[:, None] * C)

            inner = lambda u: _golden(lambda v: F(u, v), zero, 1 - u)
            best[rows] = np.minimum(best[rows], _golden(inner, zero, np.ones(rows.size, LD)))
    return np.where(ok.any(axis=1), best + shift, LD(inf))


def mp_update(P, dv, digits=40, iterations=70):
    """U of ONE pair with every source usable, by the same nested search in mpmath (slow: a sample only)"""
    import mpmath as mp
    with mp.workdps(digits):
        Pm = [[mp.mpf(float(x)) for x in row] for row in P]
        dm = [mp.mpf(float(x)) for x in dv]
        k, g = len(dm), (mp.sqrt(5) - 1) / 2

        def F(lam):
            y = [sum(lam[s] * Pm[s][c] for s in range(k)) for c in range(len(Pm[0]))]
            return sum(lam[s] * dm[s] for s in range(k)) + mp.sqrt(sum(c * c for c in y))

        def golden(f, lo, hi):
            a, b = lo, hi
            c, d = b - g * (b - a), a + g * (b - a)
            fc, fd = f(c), f(d)
            for _ in range(iterations):
                if fc < fd:
                    b, d, fd = d, c, fc
                    c = b - g * (b - a)
                    fc = f(c)
                else:
                    a, c, fc = c, d, fd
                    d = a + g * (b - a)
                    fd = f(d)
            return min(fc, fd, f(lo), f(hi))

        if k == 2:
            return golden(lambda u: F([1 - u, u]), mp.mpf(0), mp.mpf(1))
        return golden(lambda u: golden(lambda v: F([1 - u - v, u, v]), mp.mpf(0), 1 - u), mp.mpf(0), mp.mpf(1))


# ---- the near field -----------------------------------------------------------------------------------------------------
def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _segment_dist2(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    l2 = _dot(ab, ab)
    t = Fraction(0) if l2 == 0 else min(max(_dot(ab, ap) / l2, Fraction(0)), Fraction(1))
    w = [x - t * y for x, y in zip(ap, ab)]
    return _dot(w, w)


def _triangle_dist2(p, a, b, c):
    """squared distance of p to the triangle abc by the Voronoi region of p: a vertex, an edge or the face, decided by the
    signs of the barycentric numerators (exact, so no region is ever missed)"""
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    if _dot(ab, ab) * _dot(ac, ac) == _dot(ab, ac) ** 2:   # collinear or coincident: the hull is a segment
        return min(_segment_dist2(p, a, b), _segment_dist2(p, b, c), _segment_dist2(p, c, a))
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return _dot(ap, ap)                                # vertex a
    bp = _sub(p, b)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return _dot(bp, bp)                                # vertex b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        w = [x - d1 / (d1 - d3) * y for x, y in zip(ap, ab)]
        return _dot(w, w)                                  # edge ab
    cp = _sub(p, c)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return _dot(cp, cp)                                # vertex c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = [x - d2 / (d2 - d6) * y for x, y in zip(ap, ac)]
        return _dot(w, w)                                  # edge ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        w = [x - t * y for x, y in zip(bp, _sub(c, b))]
        return _dot(w, w)                                  # edge bc
    v, w_ = vb / (va + vb + vc), vc / (va + vb + vc)
    r = [x - v * y - w_ * z for x, y, z in zip(ap, ab, ac)]
    return _dot(r, r)                                      # the face


def _sqrt(q):
    """the double nearest to sqrt of the rational q >= 0"""
    import mpmath as mp
    if q == 0:
        return 0.0
    with mp.workdps(50):
        return float(mp.sqrt(mp.mpf(q.numerator) / mp.mpf(q.denominator)))


def exact_seed(X, f):
    """(is a seed cell, dist[NV]) of ONE cell with vertex coordinates X[NV][TDIM] and level-set values f[NV]: a vertex
    is negative when f < 0 (so -0.0 and 0.0 are not), an edge is crossed when its ends differ, its crossing point is
    x_i + f_i / (f_i - f_j) (x_j - x_i); dist is the distance to the convex hull of the crossing points."""
    nv = len(f)
    Xq = [[Fraction(float(c)) for c in row] for row in X]
    fq = [Fraction(float(v)) for v in f]
    neg = [v < 0 for v in fq]
    if all(neg) or not any(neg):
        return False, None
    edges = [(i, j) for i in range(nv) for j in range(nv) if neg[i] and not neg[j]]     # (negative end, other end)
    point = {}
    for i, j in edges:
        t = fq[i] / (fq[i] - fq[j])
        point[(i, j)] = [a + t * (b - a) for a, b in zip(Xq[i], Xq[j])]
    if nv == 3:
        (a, b) = [point[e] for e in edges]
        d2 = [_segment_dist2(p, a, b) for p in Xq]
    elif len(edges) == 3:
        a, b, c = [point[e] for e in edges]
        d2 = [_triangle_dist2(p, a, b, c) for p in Xq]
    else:
        # four points, planar: walk them so that neighbours share a vertex of the cell, split along the diagonal 1-3
        # (every crossed edge shares a vertex with two of the others and none with the third)
        cycle, rest = [edges[0]], edges[1:]
        while rest:
            nxt = next(e for e in rest if e[0] == cycle[-1][0] or e[1] == cycle[-1][1])
            cycle.append(nxt)
            rest.remove(nxt)
        p0, p1, p2, p3 = [point[e] for e in cycle]
        d2 = [min(_triangle_dist2(p, p0, p1, p3), _triangle_dist2(p, p1, p2, p3)) for p in Xq]
    return True, np.array([_sqrt(q) for q in d2])


def nearest_crossing(X, f):
    """per vertex of ONE seed cell: the exact distance to the nearest crossing point (an upper bound of dist: every
    crossing point belongs to the hull)"""
    nv = len(f)
    Xq = [[Fraction(float(c)) for c in row] for row in X]
    fq = [Fraction(float(v)) for v in f]
    pts = []
    for i in range(nv):
        for j in range(nv):
            if fq[i] < 0 and not fq[j] < 0:
                t = fq[i] / (fq[i] - fq[j])
                pts.append([a + t * (b - a) for a, b in zip(Xq[i], Xq[j])])
    return np.array([_sqrt(min(_dot(_sub(p, q), _sub(p, q)) for q in pts)) for p in Xq])
