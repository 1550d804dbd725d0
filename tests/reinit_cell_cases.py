"""The cell-level cases of the reinitialisation and what is asserted of them, shared by tests/test_reinit_cell_reference.py
(the header on the CPU, and the numpy model) and tests/test_gpu_reinit_cell.py (the header on the GPU): the same seeded
cases and the same assertions for every implementation.  The references are tests/reinit_exact.py; every set's reference
is computed once per process.

An update set is dict(P [m, k, dim], dv [m, k], ok [m, k] bool, tag [m] str); a seed set is dict(X [m, nv, dim], f [m, nv],
tag [m]).  L of a case is the longest |P_s| (update) or the longest edge (seed)."""
from __future__ import annotations

import itertools
import os
import re
import subprocess
from pathlib import Path

import numpy as np

import reinit_exact as E
import reinit_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "cutfemx_amd" / "csrc"
INF = 1e30
Q0 = R.DEGENERATE
PLANE_TOL = 1e-12     # the project's plane tolerance
FLAT_TOL = 1e-10      # the project's TOL

_CACHE: dict = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- measures -----------------------------------------------------------------------------------------------------------
def length(P):
    return np.sqrt(np.max(np.sum(np.asarray(P, dtype=np.float64) ** 2, axis=2), axis=1))


def cell_flatness(P):
    """q = det G / prod G_ii of the Gram matrix of the rows of P, in long double: the squared volume of the cell relative
    to its edges at the target"""
    P = np.asarray(P).astype(np.longdouble)
    G = np.einsum("mik,mjk->mij", P, P)
    if P.shape[1] == 2:
        det = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] ** 2
    else:
        det = (G[:, 0, 0] * (G[:, 1, 1] * G[:, 2, 2] - G[:, 1, 2] ** 2) - G[:, 0, 1] * (G[:, 0, 1] * G[:, 2, 2] - G[:, 1, 2] * G[:, 0, 2])
               + G[:, 0, 2] * (G[:, 0, 1] * G[:, 1, 2] - G[:, 1, 1] * G[:, 0, 2]))
    prod = np.prod(np.einsum("mii->mi", G), axis=1)
    return np.where(prod > 0, np.abs(det) / np.where(prod > 0, prod, 1), 0).astype(np.float64)


def face_flatness(P):
    """sin^2 of the angle of the face P0 P1 P2 at P0 (the engine's degeneracy measure), in long double; 0 for a face whose
    first edge has no length"""
    P = np.asarray(P).astype(np.longdouble)
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    a, c = np.sum(e1 * e1, axis=1), np.sum(e2 * e2, axis=1)
    n = np.cross(e1, e2)
    den = a * c
    return np.where(den > 0, np.sum(n * n, axis=1) / np.where(den > 0, den, 1), 0).astype(np.float64)


def ulp_of_values(dv):
    return np.spacing(np.max(np.abs(dv), axis=1))


# ---- update sets --------------------------------------------------------------------------------------------------------
def _unit(rng, m, dim):
    n = rng.normal(size=(m, dim))
    return n / np.linalg.norm(n, axis=1)[:, None]


def _well_shaped(rng, m, dim):
    """m cells with q >= 1e-3 and L of order 1"""
    out = np.zeros((0, dim, dim))
    while out.shape[0] < m:
        P = rng.normal(size=(2 * m, dim, dim))
        out = np.concatenate([out, P[cell_flatness(P) >= 1e-3]])
    return out[:m]


def _values(rng, P, kind):
    """eikonal: a plane wave of unit slope; sub: slope below 1; inconsistent: slope 1 .. 3 plus noise, no plane wave"""
    m, k, dim = P.shape
    n = _unit(rng, m, dim)
    slope = {"eikonal": np.ones(m), "sub": rng.uniform(0.0, 1.0, m), "inconsistent": rng.uniform(1.0, 3.0, m)}[kind]
    dv = np.einsum("mik,mk->mi", P, n) * slope[:, None]
    if kind == "inconsistent":
        dv = dv + 0.3 * rng.normal(size=(m, k)) * length(P)[:, None]
    return dv


def well_shaped_set(dim):
    """q >= 1e-3; every combination of coordinate scale 2^-20, 1, 2^20 and value offset 0, 5 L, 1e6 L has its own 72 cells:
    24 per kind of values; of each 24, 12 with every source usable, 8 with the 2^dim masks in turn (the empty one
    included), 4 with one source moved onto the target (the target's own copy, not usable)."""
    def make():
        rng = np.random.default_rng([41, dim])
        Ps, ds, oks, tags = [], [], [], []
        masks = list(itertools.product([True, False], repeat=dim))
        for scale in (2.0 ** -20, 1.0, 2.0 ** 20):
            for offset in (0.0, 5.0, 1e6):
                for kind in ("eikonal", "sub", "inconsistent"):
                    P = _well_shaped(rng, 24, dim)
                    dv = _values(rng, P, kind) + offset * length(P)[:, None]
                    ok = np.ones((24, dim), dtype=bool)
                    for i in range(12, 24):
                        ok[i] = masks[i % len(masks)]
                    for i in range(20, 24):
                        s = i % dim
                        P[i, s], ok[i] = 0.0, True
                        ok[i, s] = False
                    Ps.append(P * scale), ds.append(dv * scale), oks.append(ok)
                    tags += [f"{kind} scale {scale:g} offset {offset:g}"] * 24
        return dict(P=np.concatenate(Ps), dv=np.concatenate(ds), ok=np.concatenate(oks), tag=np.array(tags))
    return cached(("well", dim), make)


def boundary_set(dim):
    """The stationary point y of a plane wave d = n . x, constructed on the boundary of the face: on an edge (3-D), at a
    vertex, or 1e-9 L inside / outside of either; the target is y + s n.  Every source usable."""
    def make():
        rng = np.random.default_rng([43, dim])
        Ps, ds, tags = [], [], []
        spots = {"vertex": [1.0] + [0.0] * (dim - 1)}
        if dim == 3:
            spots["edge"] = [0.3, 0.7, 0.0]
        for spot, lam0 in spots.items():
            for shift in (0.0, 1e-9, -1e-9):
                for rot in range(dim):
                    m = 12
                    X = _well_shaped(rng, m, dim)                     # the sources (any origin)
                    lam = np.roll(np.array(lam0), rot)[None, :].repeat(m, axis=0)
                    # shift towards the face's centroid (inside) or away from it (outside), barycentrics still sum to 1
                    lam = lam + shift * (1.0 / dim - lam)
                    y = np.einsum("mi,mik->mk", lam, X)
                    # a unit n that is not in the face's plane: the face normal tilted by a random tangential part
                    if dim == 3:
                        nf = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
                    else:
                        e = X[:, 1] - X[:, 0]
                        nf = np.stack([-e[:, 1], e[:, 0]], axis=1)
                    nf /= np.linalg.norm(nf, axis=1)[:, None]
                    n = nf + 0.8 * rng.uniform(0.2, 1.0, m)[:, None] * _unit(rng, m, dim)
                    n /= np.linalg.norm(n, axis=1)[:, None]
                    t = y + rng.uniform(0.3, 1.5, m)[:, None] * n
                    Ps.append(X - t[:, None, :]), ds.append(np.einsum("mik,mk->mi", X, n) + 3.0)
                    tags += [f"{spot} shift {shift:g}"] * m
        P = np.concatenate(Ps)
        return dict(P=P, dv=np.concatenate(ds), ok=np.ones(P.shape[:2], dtype=bool), tag=np.array(tags))
    return cached(("boundary", dim), make)


def _kuhn_tets():
    tets = []
    for perm in itertools.permutations(range(3)):
        v = [np.zeros(3)]
        for k in perm:
            w = v[-1].copy()
            w[k] = 1.0
            v.append(w)
        tets.append(np.array(v))
    return tets


def flat_set():
    """Graded flatness in 3-D, every source usable:
    kuhn      the six Kuhn cells of a box squeezed 1e-1 .. 1e-7 along each axis, every (target, cell) pair, with an
              eikonal and a sub-eikonal plane wave
    flat      random faces with the target 1e-3 .. 1e-10 L above a point of the interior, of an edge, or outside the face
    sliver    faces whose sin^2 at the first source is Q0 x 10^-3 .. 10^6 (the threshold Q0 is straddled by factors 4 and 2)
              -- with arbitrary values, and with a plane wave whose ray passes through the face's interior
    needle    faces with one edge 1e-3 .. 1e-7 of the others, rays through the interior
    coplanar  the target exactly in the face's plane, inside and outside the face
    collinear three sources exactly on a line
    coincident two sources in the same place"""
    def make():
        rng = np.random.default_rng(47)
        Ps, ds, tags = [], [], []

        def add(P, dv, tag):
            Ps.append(P), ds.append(dv), tags.extend([tag] * P.shape[0])

        for axis in range(3):
            for squeeze in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
                scale = np.ones(3)
                scale[axis] = squeeze
                rows = []
                for T in _kuhn_tets():
                    X = T * scale
                    for t in range(4):
                        rows.append(X[[i for i in range(4) if i != t]] - X[t])
                P = np.array(rows)
                for kind in ("eikonal", "sub"):
                    add(P, _values(rng, P, kind) + 2.0, f"kuhn {squeeze:g}")
        for height in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10):
            for where in ("interior", "edge", "outside"):
                m = 8
                X = np.zeros((m, 3, 3))
                while True:
                    X[:, :, :2] = rng.normal(size=(m, 3, 2))
                    if np.all(face_flatness(X) > 0.05):
                        break
                lam = {"interior": rng.dirichlet([2, 2, 2], m), "edge": np.stack([rng.uniform(0.2, 0.8, m), np.zeros(m)], axis=1),
                       "outside": np.stack([rng.uniform(0.2, 0.8, m), -rng.uniform(0.05, 0.5, m)], axis=1)}[where]
                if where != "interior":
                    lam = np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)
                t = np.einsum("mi,mik->mk", lam, X)
                t[:, 2] = height * length(X - t[:, None, :])
                rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]            # (out of the coordinate planes)
                P = (X - t[:, None, :]) @ rot
                add(P, _values(rng, P, "sub" if where == "outside" else "eikonal") + 2.0, f"flat {height:g} {where}")
        for factor in (1e-3, 0.25, 0.5, 2.0, 4.0, 10.0, 1e2, 1e3, 1e4, 1e6):
            m = 10
            sin = np.sqrt(Q0 * factor)
            e1 = _unit(rng, m, 3) * rng.uniform(0.5, 1.5, m)[:, None]
            perp = np.cross(e1, _unit(rng, m, 3))
            perp /= np.linalg.norm(perp, axis=1)[:, None]
            stretch = rng.uniform(0.3, 1.2, m) * np.where(rng.uniform(size=m) < 0.3, -1.0, 1.0)
            e2 = stretch[:, None] * e1 + (np.abs(stretch) * np.linalg.norm(e1, axis=1) * sin / np.sqrt(1 - sin * sin))[:, None] * perp
            x0 = _unit(rng, m, 3)
            P = np.stack([x0, x0 + e1, x0 + e2], axis=1)
            q = face_flatness(P)
            assert np.all(np.abs(q / (Q0 * factor) - 1.0) < 0.1), q
            add(P, _values(rng, P, "sub") + 2.0, f"sliver {factor:g}")
            # the same faces with a plane wave whose ray to the target passes through the face's interior
            nf = np.cross(e1, perp)
            n = nf / np.linalg.norm(nf, axis=1)[:, None] + 0.6 * _unit(rng, m, 3)
            n /= np.linalg.norm(n, axis=1)[:, None]
            for _ in range(3):
                lam = rng.dirichlet([2, 2, 2], m)
                t = np.einsum("mi,mik->mk", lam, P) + rng.uniform(0.3, 1.0, m)[:, None] * n
                add(P - t[:, None, :], np.einsum("mik,mk->mi", P, n) + 2.0, f"sliver {factor:g} ray")
        # needles: one edge of the face 1e-3 .. 1e-7 of the others, opposite each source in turn; rays through the interior
        for short in (1e-3, 1e-5, 1e-7):
            for apex in range(3):
                m = 8
                X = _well_shaped(rng, m, 3)
                a, b = [i for i in range(3) if i != apex]
                X[:, b] = X[:, a] + short * (X[:, b] - X[:, a])
                nf = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
                n = nf / np.linalg.norm(nf, axis=1)[:, None] + 0.6 * _unit(rng, m, 3)
                n /= np.linalg.norm(n, axis=1)[:, None]
                t = np.einsum("mi,mik->mk", rng.dirichlet([2, 2, 2], m), X) + rng.uniform(0.3, 1.0, m)[:, None] * n
                P = X - t[:, None, :]
                assert np.all(np.abs(face_flatness(P) / Q0 - 1.0) > 0.5)
                add(P, np.einsum("mik,mk->mi", X, n) + 2.0, f"needle {short:g} apex {apex}")
        # exactly degenerate, in small binary fractions so that every product is exact
        m = 12
        X = np.zeros((m, 3, 3))
        X[:, :, :2] = rng.integers(-8, 9, size=(m, 3, 2)) / 8.0
        X = X[face_flatness(X) > 0.01]
        lam = np.array([[0.25, 0.25, 0.5], [0.5, 0.75, -0.25]])[rng.integers(0, 2, X.shape[0])]
        P = X - np.einsum("mi,mik->mk", lam, X)[:, None, :]
        add(P, _values(rng, P, "sub") + 2.0, "coplanar")
        base, step = rng.integers(-8, 9, size=(m, 3)) / 8.0, rng.integers(-4, 5, size=(m, 3)) / 4.0
        keep = (np.abs(step).sum(axis=1) > 0) & (np.linalg.norm(np.cross(base, step), axis=1) > 0)
        base, step = base[keep], step[keep]
        P = np.stack([base, base + step, base - 0.5 * step], axis=1)
        add(P, _values(rng, P, "sub") + 2.0, "collinear")
        P = _well_shaped(rng, m, 3)
        for i in range(m):
            a, b = [(0, 1), (0, 2), (1, 2)][i % 3]
            P[i, b] = P[i, a]
        dv = _values(rng, P, "sub") + 2.0
        add(P, dv, "coincident")
        P = np.concatenate(Ps)
        return dict(P=P, dv=np.concatenate(ds), ok=np.ones(P.shape[:2], dtype=bool), tag=np.array(tags))
    return cached("flat", make)


def flat_set_2d():
    """2-D: the target 1e-3 .. 1e-10 L above the interior of the edge of two sources and beyond its end, exactly on its
    line, and coincident sources"""
    def make():
        rng = np.random.default_rng(53)
        Ps, ds, tags = [], [], []
        for height in (1e-3, 1e-5, 1e-7, 1e-8, 1e-9, 1e-10, 0.0):
            for where in ("interior", "outside"):
                m = 10
                X = rng.normal(size=(m, 2, 2))
                e = X[:, 1] - X[:, 0]
                lam = rng.uniform(0.1, 0.9, m) if where == "interior" else 1.0 + rng.uniform(0.05, 0.5, m)
                foot = X[:, 0] + lam[:, None] * e
                if height == 0.0:                                         # exactly collinear: binary fractions
                    X = rng.integers(-8, 9, size=(m, 2, 2)) / 8.0
                    X[:, 1] += (np.abs(X[:, 1] - X[:, 0]).sum(axis=1) == 0)[:, None] * 0.5
                    e = X[:, 1] - X[:, 0]
                    foot = X[:, 0] + (0.25 if where == "interior" else 1.5) * e
                nrm = np.stack([-e[:, 1], e[:, 0]], axis=1) / np.linalg.norm(e, axis=1)[:, None]
                t = foot + height * np.linalg.norm(e, axis=1)[:, None] * nrm
                P = X - t[:, None, :]
                Ps.append(P), ds.append(_values(rng, P, "sub") + 2.0)
                tags += [f"flat {height:g} {where}"] * m
        P = _well_shaped(rng, 6, 2)
        P[:, 1] = P[:, 0]
        Ps.append(P), ds.append(_values(rng, P, "sub") + 2.0)
        tags += ["coincident"] * 6
        P = np.concatenate(Ps)
        return dict(P=P, dv=np.concatenate(ds), ok=np.ones(P.shape[:2], dtype=bool), tag=np.array(tags))
    return cached("flat2", make)


UPDATE_SETS = {"well3": lambda: well_shaped_set(3), "well2": lambda: well_shaped_set(2), "boundary3": lambda: boundary_set(3),
               "boundary2": lambda: boundary_set(2), "flat3": flat_set, "flat2": flat_set_2d}


def brute(name):
    """(minimum over the hull of the usable sources, minimum over the sub-faces of one and two sources) of a set"""
    def make():
        s = UPDATE_SETS[name]()
        full = E.brute_update(s["P"], s["dv"], s["ok"], INF)
        if s["P"].shape[1] == 2:
            one = E.brute_update(s["P"][:, :1], s["dv"][:, :1], s["ok"][:, :1], INF)
            two = E.brute_update(s["P"][:, 1:], s["dv"][:, 1:], s["ok"][:, 1:], INF)
            return full, np.minimum(one, two)
        sub = np.full(full.shape, np.longdouble(INF))
        for i, j in ((0, 1), (0, 2), (1, 2)):
            sub = np.minimum(sub, E.brute_update(s["P"][:, [i, j]], s["dv"][:, [i, j]], s["ok"][:, [i, j]], INF))
        return full, sub
    return cached(("brute", name), make)


def _worst(err, tags, what):
    lines = []
    for tag in dict.fromkeys(tags):
        e = err[tags == tag]
        lines.append(f"  {what} {tag}: U - reference in [{e.min():+.2e}, {e.max():+.2e}] L")
    return "\n".join(lines)


def check_tight(name, U, who):
    """well-shaped and boundary sets: |U - brute| <= 1e-12 L + 4 ulp(max |d|); no usable source gives inf"""
    s, (ref, _) = UPDATE_SETS[name](), brute(name)
    L = length(s["P"])
    none = ~s["ok"].any(axis=1)
    assert np.array_equal(U[none], np.full(int(none.sum()), INF)), f"{who}: an empty mask does not give inf"
    some = ~none
    # (a source on the target itself has no length: L is over the rows, it stays the cell's size)
    err = ((U[some].astype(np.longdouble) - ref[some]) / L[some]).astype(np.float64)
    bound = PLANE_TOL + 4.0 * ulp_of_values(s["dv"][some]) / L[some]
    print(f"{who} {name}: {int(some.sum())} cases, worst |U - brute| = {np.max(np.abs(err)):.2e} L, "
          f"worst against its bound {np.max(np.abs(err) / bound):.3f}")
    bad = np.abs(err) > bound
    assert not bad.any(), f"{who} {name}:\n" + _worst(err[bad], s["tag"][some][bad], "beyond the bound")
    return err


def kernel_degenerate(P):
    """the cells whose full face the engine leaves to its sub-faces (3-D): sin^2 at the first source <= Q0, or no first edge"""
    return ~(face_flatness(P) > Q0)


def check_flat(name, U, who):
    """graded flatness: one-sided for every cell, two-sided for every cell the engine treats as non-degenerate, and the
    sub-faces' value below the threshold"""
    s, (ref, sub) = UPDATE_SETS[name](), brute(name)
    L = length(s["P"])
    err = ((U.astype(np.longdouble) - ref) / L).astype(np.float64)
    over = ((U.astype(np.longdouble) - sub) / L).astype(np.float64)
    if s["P"].shape[1] == 3:
        degenerate = kernel_degenerate(s["P"])
    else:
        degenerate = np.all(s["P"][:, 0] == s["P"][:, 1], axis=1)
    print(f"{who} {name}: {U.size} cases, {int(degenerate.sum())} degenerate\n" + _worst(err, s["tag"], "all"))
    low = err < -FLAT_TOL
    assert not low.any(), f"{who} {name}: below the true minimum\n" + _worst(err[low], s["tag"][low], "low")
    high = over > PLANE_TOL
    assert not high.any(), f"{who} {name}: above the least sub-face value\n" + _worst(over[high], s["tag"][high], "high")
    off = ~degenerate & (np.abs(err) > FLAT_TOL)
    assert not off.any(), f"{who} {name}: a non-degenerate cell misses {FLAT_TOL:g} L\n" + _worst(err[off], s["tag"][off], "off")
    wrong = degenerate & (np.abs(over) > PLANE_TOL + 4.0 * ulp_of_values(s["dv"]) / L)
    assert not wrong.any(), f"{who} {name}: a degenerate cell is not decided by its sub-faces\n" + _worst(over[wrong], s["tag"][wrong], "wrong")
    return err


def error_table(name, results):
    """worst |U - brute| / L of the cells whose full face is not degenerate, one column per implementation (for
    DESIGN.md): by decade of the cell's flatness q for well-shaped faces (3-D: sin^2 >= 1e-3), and by decade of the
    face's sin^2 for the others"""
    s, (ref, _) = UPDATE_SETS[name](), brute(name)
    L, q = length(s["P"]), cell_flatness(s["P"])
    if s["P"].shape[1] == 3:
        sin2 = face_flatness(s["P"])
        keep, fine = ~kernel_degenerate(s["P"]), sin2 >= 1e-3
    else:
        keep = ~np.all(s["P"][:, 0] == s["P"][:, 1], axis=1)
        sin2, fine = np.ones(q.size), np.ones(q.size, dtype=bool)

    def rows_of(measure, select, label):
        decade = np.where(measure > 0, np.floor(np.log10(np.where(measure > 0, measure, 1.0))), -np.inf)
        out = []
        for dec in sorted(set(decade[select]), reverse=True):
            rows = select & (decade == dec)
            cols = [f"{np.max(np.abs((U[rows].astype(np.longdouble) - ref[rows]) / L[rows]).astype(np.float64)):.1e}" for U in results.values()]
            out.append(f"  {label} {'= 0' if dec == -np.inf else f'1e{int(dec)}':>6s} {int(rows.sum()):5d}  " + "  ".join(cols))
        return out

    lines = [f"error table {name}: measure, cases, " + ", ".join(results)]
    lines += rows_of(q, keep & fine, "q")
    lines += rows_of(sin2, keep & ~fine, "sin^2")
    return "\n".join(lines)


# ---- seed sets ----------------------------------------------------------------------------------------------------------
def _cells(rng, dim):
    """a Kuhn cell of the unit box and a random cell with q >= 1e-3 at every vertex"""
    if dim == 3:
        kuhn = _kuhn_tets()[3]
    else:
        kuhn = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])
    while True:
        X = rng.normal(size=(dim + 1, dim))
        if all(cell_flatness((np.delete(X, t, axis=0) - X[t])[None])[0] >= 1e-3 for t in range(dim + 1)):
            return [kuhn, X]


def edge_length(X):
    nv = X.shape[1]
    return np.max([np.linalg.norm(X[:, i] - X[:, j], axis=1) for i in range(nv) for j in range(i)], axis=0)


def seed_set(dim):
    """Near-field cells with q >= 1e-3:
    signs      every sign pattern under every permutation of the local vertices, random magnitudes
    zeros      every pattern of {0, -, +} with a zero in it; the same with -0.0 for every zero
    near       a crossing 1e-12 and 1e-16 (within an ulp) from the negative or the other end of its edge
    extreme    |phi| ratios of 1e-100 and 1e-300 (asserted one-sided only)"""
    def make():
        rng = np.random.default_rng([59, dim])
        nv = dim + 1
        Xs, fs, tags = [], [], []
        for X in _cells(rng, dim):
            for perm in itertools.permutations(range(nv)):
                for signs in itertools.product([-1.0, 1.0], repeat=nv):
                    Xs.append(X[list(perm)]), fs.append(np.array(signs) * rng.uniform(0.1, 1.0, nv)), tags.append("signs")
            for pattern in itertools.product([0.0, -1.0, 1.0], repeat=nv):
                if 0.0 in pattern:
                    f = np.array(pattern) * rng.uniform(0.1, 1.0, nv)
                    Xs.append(X), fs.append(f + 0.0), tags.append("zeros")
                    Xs.append(X), fs.append(np.where(f == 0.0, -0.0, f)), tags.append("zeros")
            for small, tag in ((1e-12, "near"), (1e-16, "near"), (1e-100, "extreme"), (1e-300, "extreme")):
                for who in range(nv):                                   # the vertex with the small value
                    for sign in (-1.0, 1.0):                            # ... negative, or not
                        for others in itertools.product([-1.0, 1.0], repeat=nv - 1):
                            f = np.insert(np.array(others) * rng.uniform(0.5, 1.0, nv - 1), who, sign * small)
                            Xs.append(X), fs.append(f), tags.append(tag)
        return dict(X=np.array(Xs), f=np.array(fs), tag=np.array(tags))
    return cached(("seed", dim), make)


def exact_seeds(dim):
    """(flag [m], dist [m, nv], distance to the nearest crossing point [m, nv]) of seed_set(dim), exact"""
    def make():
        s = seed_set(dim)
        m, nv = s["f"].shape
        flag, dist, near = np.zeros(m, dtype=bool), np.full((m, nv), -1.0), np.full((m, nv), -1.0)
        for i in range(m):
            flag[i], d = E.exact_seed(s["X"][i], s["f"][i])
            if flag[i]:
                dist[i], near[i] = d, E.nearest_crossing(s["X"][i], s["f"][i])
        return flag, dist, near
    return cached(("exact_seed", dim), make)


def check_seed(dim, flag, dist, who):
    s, (xflag, xdist, xnear) = seed_set(dim), exact_seeds(dim)
    assert np.array_equal(flag.astype(bool), xflag), f"{who}: seed cells differ: {np.nonzero(flag.astype(bool) != xflag)[0][:10]}"
    L = edge_length(s["X"])
    tight = xflag & (s["tag"] != "extreme")
    err = np.abs(dist[tight] - xdist[tight]) / L[tight, None]
    for tag in ("signs", "zeros", "near"):
        print(f"{who} seed{dim} {tag}: {int((s['tag'][tight] == tag).sum())} seed cells, worst |dist - exact| = "
              f"{err[s['tag'][tight] == tag].max():.2e} L")
    assert np.all(err <= PLANE_TOL), f"{who}: {np.nonzero(np.any(err > PLANE_TOL, axis=1))[0][:10]} of the toleranced cells"
    loose = xflag & (s["tag"] == "extreme")
    d = dist[loose]
    assert np.all(np.isfinite(d)) and np.all(d >= 0.0)
    slack = (d - xnear[loose]) / L[loose, None]
    print(f"{who} seed{dim} extreme: {int(loose.sum())} seed cells, dist - nearest crossing <= {slack.max():+.2e} L, "
          f"worst |dist - exact| = {np.max(np.abs(d - xdist[loose]) / L[loose, None]):.2e} L")
    assert np.all(slack <= PLANE_TOL)
    # zeros: a vertex that is zero (of either sign) on a seed cell lies on the piece
    zero = xflag[:, None] & (s["f"] == 0.0)
    assert np.all(dist[zero] <= PLANE_TOL * np.broadcast_to(L[:, None], zero.shape)[zero])


# ---- the programs -------------------------------------------------------------------------------------------------------
def makefile_variable(name):
    text = (CSRC / "Makefile").read_text()
    m = re.search(rf"^{name}\s*\?=\s*(.*)$", text, re.M)
    assert m, f"{name} is not set in {CSRC / 'Makefile'}"
    return os.environ.get(name, m[1].strip())


def compile_program(source, exe, offload):
    """with the compiler and the flags of the engine's Makefile; offload: for the architecture of the Makefile, else
    plain host C++"""
    arch = [f"--offload-arch={makefile_variable('ARCH')}"] if offload else []
    cmd = [makefile_variable("HIPCC"), *arch, *makefile_variable("CXXFLAGS").split(), str(ROOT / "tests" / "cpp" / source), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, f"{source} does not compile:\n" + " ".join(cmd) + "\n" + done.stderr[-4000:]
    return exe


def run_program(exe, directory, seconds=120.0):
    """ONE process for every set of this module: {set name: U} and {dim: (flag, dist)}.  Raises on a non-zero status or
    at the time limit; the caller does not start the program again."""
    directory = Path(directory)
    lines = []

    def put(name, tag, a, dtype):
        np.ascontiguousarray(a, dtype=np.dtype(dtype).newbyteorder("<")).tofile(directory / f"{name}.{tag}.bin")

    for name, make in UPDATE_SETS.items():
        s = make()
        put(name, "P", s["P"], np.float64), put(name, "dv", s["dv"], np.float64), put(name, "ok", s["ok"], np.uint8)
        lines.append(f"{name} update{s['P'].shape[1]} n={s['P'].shape[0]} inf={INF!r}")
    for dim in (2, 3):
        s = seed_set(dim)
        put(f"seed{dim}", "X", s["X"], np.float64), put(f"seed{dim}", "f", s["f"], np.float64)
        lines.append(f"seed{dim} seed{dim} n={s['f'].shape[0]}")
    (directory / "manifest.txt").write_text("\n".join(lines) + "\n")
    done = subprocess.run([str(exe), str(directory)], capture_output=True, text=True, timeout=seconds)
    assert done.returncode == 0, f"{exe.name} ended with status {done.returncode}: {done.stderr[-2000:]}"
    get = lambda name, tag, dtype: np.fromfile(directory / f"{name}.{tag}.out", dtype=np.dtype(dtype).newbyteorder("<")).astype(dtype)
    updates = {name: get(name, "U", np.float64) for name in UPDATE_SETS}
    seeds = {dim: (get(f"seed{dim}", "flag", np.uint8), get(f"seed{dim}", "dist", np.float64).reshape(-1, dim + 1)) for dim in (2, 3)}
    return updates, seeds


def model_update(name):
    s = UPDATE_SETS[name]()
    return R.update(s["P"], s["dv"], s["ok"], INF)


def model_seed(dim):
    """reinit_ref.nearfield on the cells as a mesh of disjoint cells: (flag, dist).  The model's d0 = 0 on phi == 0 is the
    whole call's rule, not the cell's; on a seed cell it agrees with the cell's own distance (the vertex is a crossing
    point), and for the flag the zero vertices are left out."""
    s = seed_set(dim)
    m, nv = s["f"].shape
    x = np.zeros((m * nv, 3))
    x[:, :dim] = s["X"].reshape(m * nv, dim)
    d0 = R.nearfield(x, np.arange(m * nv).reshape(m, nv), s["f"].reshape(-1), INF).reshape(m, nv)
    flag = np.any((d0 < INF) & (s["f"] != 0.0), axis=1)
    return flag, np.where(flag[:, None], d0, -1.0)
