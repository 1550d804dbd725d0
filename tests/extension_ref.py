"""numpy model of the normal extension's contract (include/cutfemx_amd.h, cfx_extend_normal_velocity), written from the
contract on top of the reinitialisation's model (tests/reinit_ref.py: nearfield, fim): the near payload from the closest
point of the lowest seed cell in the window, the transported payload from the first candidate in the window on the
final distance with the causal sources renormalised, Jacobi (or in-place) sweeps to the fixed point.  Shared by
tests/test_extension_reference.py (which pins it to mathematics) and the GPU tests (which compare the engine with it on
the same arrays); every case's model runs once.

It also counts the GREY ZONE of a case: the candidates whose relative gap to the minimum lies between 1e-13 and 1e-11.
Inside 1e-13 two implementations agree that a candidate is in the window of 1e-12, beyond 1e-11 that it is not; a case
with an empty grey zone has one answer whatever the last ulps of the arithmetic are."""
from __future__ import annotations

from itertools import combinations

import numpy as np

import reinit_ref as R

WINDOW = 1e-12
GREY = (1e-13, 1e-11)
NONE, ZERO, NEAR, TRANSPORTED = 0, 1, 2, 3


# ---- closest points -----------------------------------------------------------------------------------------------------
def _seg_closest(p, a, b):
    ab = b - a
    l2 = ab @ ab
    t = min(max((ab @ (p - a)) / l2, 0.0), 1.0) if l2 > 0.0 else 0.0
    r = (p - a) - t * ab
    return r @ r, t


def _tri_closest(p, a, b, c):
    """(squared distance, weights of a, b, c) of the point of the triangle closest to p: the edges, and the foot of the
    perpendicular where it falls inside"""
    best, w = None, None
    for (i, j), (u, v) in zip(((0, 1), (1, 2), (2, 0)), ((a, b), (b, c), (c, a))):
        r2, t = _seg_closest(p, u, v)
        if best is None or r2 < best:
            best, w = r2, np.zeros(3)
            w[i], w[j] = 1.0 - t, t
    n = np.cross(b - a, c - a)
    nn = n @ n
    if nn > R.FLAT_PIECE * ((b - a) @ (b - a)) * ((c - a) @ (c - a)):
        s = n @ (p - a)
        q = p - n * (s / nn)
        e = np.array([np.cross(c - b, q - b) @ n, np.cross(a - c, q - c) @ n, np.cross(b - a, q - a) @ n])   # opposite a, b, c
        if np.all(e >= 0.0) and s * s / nn < best:
            best, w = s * s / nn, e / e.sum()
    return best, w


def seed_closest(X, f, at):
    """The point of the piece of the seed cell (X [nv, dim], f [nv]) closest to its vertex `at`: (distance, weights of the
    cell's vertices), or None when no edge of the cell is crossed.  The pieces are the model's (reinit_ref.nearfield)."""
    nv = f.size
    neg = f < 0.0
    nneg = int(neg.sum())
    if nneg in (0, nv):
        return None

    def crossing(i, j):
        if not neg[i]:
            i, j = j, i
        t = f[i] / (f[i] - f[j])
        lam = np.zeros(nv)
        lam[i] += 1.0 - t
        lam[j] += t
        return X[i] + t * (X[j] - X[i]), lam

    if nv == 4 and nneg == 2:
        ng, ps = np.nonzero(neg)[0], np.nonzero(~neg)[0]
        pts = [crossing(ng[0], ps[0]), crossing(ng[0], ps[1]), crossing(ng[1], ps[1]), crossing(ng[1], ps[0])]
        pieces = [(0, 1, 2), (0, 2, 3)]
    else:
        l = int(np.nonzero(neg == (nneg == 1))[0][0])
        pts = [crossing(l, i) for i in range(nv) if i != l]
        pieces = [tuple(range(nv - 1))]
    best = None
    for piece in pieces:
        if nv == 3:
            r2, t = _seg_closest(X[at], pts[0][0], pts[1][0])
            w = np.array([1.0 - t, t])
        else:
            r2, w = _tri_closest(X[at], *(pts[k][0] for k in piece))
        if best is None or r2 < best[0]:
            best = (r2, sum(wk * pts[k][1] for wk, k in zip(w, piece)))
    return np.sqrt(best[0]), best[1]


def cell_normal(X, f, sign=1.0):
    """sign grad(f) / |grad(f)| of the P1 function f on the cell X; None for a cell without volume, 0 for a zero gradient"""
    E = X[1:] - X[0]
    if abs(np.linalg.det(E)) == 0.0:
        return None
    g = np.linalg.solve(E, f[1:] - f[0])
    length = np.linalg.norm(g)
    return sign * g / length if length > 0.0 else np.zeros_like(g)


# ---- the update with the place of its minimum ---------------------------------------------------------------------------
def _subface(Ps, ds, inf):
    """(value, weights [m, size]) of the minimum over the plane of a sub-face of two or three sources where it lies in the
    sub-face, else (inf, 0): reinit_ref._subface_value with the minimiser"""
    m, size, _ = Ps.shape
    val, lam_out = np.full(m, inf), np.zeros((m, size))
    E = Ps[:, 1:, :] - Ps[:, :1, :]
    delta = ds[:, 1:] - ds[:, :1]
    l1 = np.linalg.norm(E[:, 0], axis=1)
    good = l1 > 0.0
    if size == 3:
        with np.errstate(all="ignore"):
            u1 = E[:, 0] / l1[:, None]
            w = E[:, 1] - np.einsum("mk,mk->m", E[:, 1], u1)[:, None] * u1
            good &= np.einsum("mk,mk->m", w, w) > R.DEGENERATE * np.einsum("mk,mk->m", E[:, 1], E[:, 1])
    rows = np.nonzero(good)[0]
    if rows.size == 0:
        return val, lam_out
    E, delta, P0, d0 = E[rows], delta[rows], Ps[rows, 0], ds[rows, 0]
    U = np.zeros((rows.size, size - 1, E.shape[2]))
    U[:, 0] = E[:, 0] / np.linalg.norm(E[:, 0], axis=1)[:, None]
    if size == 3:
        w = E[:, 1] - np.einsum("mk,mk->m", E[:, 1], U[:, 0])[:, None] * U[:, 0]
        U[:, 1] = w / np.linalg.norm(w, axis=1)[:, None]
    Cm = np.einsum("mik,mjk->mij", E, U)
    g = np.linalg.solve(Cm, delta[:, :, None])[:, :, 0]
    gg = 1.0 - np.einsum("mi,mi->m", g, g)
    real = gg > 0.0
    root = np.sqrt(np.where(real, gg, 1.0))
    pt = np.einsum("mik,mk->mi", U, P0)
    h = np.linalg.norm(P0 - np.einsum("mi,mik->mk", pt, U), axis=1)
    y = -pt - (h / root)[:, None] * g
    lam = np.linalg.solve(np.swapaxes(Cm, 1, 2), y[:, :, None])[:, :, 0]
    valid = real & np.all(lam >= 0.0, axis=1) & (lam.sum(axis=1) <= 1.0)
    val[rows] = np.where(valid, d0 - np.einsum("mi,mi->m", g, pt) + h * root, inf)
    lam_out[rows] = np.where(valid[:, None], np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1), 0.0)
    return val, lam_out


def subface_values(P, dv, ok, inf=R.INF):
    """Every sub-face of m (target, cell) pairs in cell_update's order (single sources, pairs, the triple):
    (values [m, nsub], weights [m, nsub, k]); inf where the sub-face is not valid or has a source that is not usable."""
    m, k, _ = P.shape
    subs = [list(S) for size in range(1, k + 1) for S in combinations(range(k), size)]
    vals, lams = np.full((m, len(subs)), inf), np.zeros((m, len(subs), k))
    for q, S in enumerate(subs):
        rows = np.nonzero(np.all(ok[:, S], axis=1))[0]
        if rows.size == 0:
            continue
        Ps, ds = P[rows][:, S, :], dv[rows][:, S]
        if len(S) == 1:
            val, lam = ds[:, 0] + np.linalg.norm(Ps[:, 0], axis=1), np.ones((rows.size, 1))
        else:
            val, lam = _subface(Ps, ds, inf)
        vals[rows, q] = val
        full = np.zeros((rows.size, k))
        full[:, S] = lam
        lams[rows, q] = full
    return vals, lams


def update_argmin(P, dv, ok, inf=R.INF, limit=None):
    """(U, value, weights) per pair: U the least value; the reported sub-face is the first with value <= limit, else the
    first that attains U (limit None: always that one)"""
    vals, lams = subface_values(P, dv, ok, inf)
    U = vals.min(axis=1)
    pick = np.argmin(vals, axis=1)
    if limit is not None:
        within = vals <= np.asarray(limit)[:, None]
        pick = np.where(within.any(axis=1), np.argmax(within, axis=1), pick)
    rows = np.arange(vals.shape[0])
    return U, vals[rows, pick], lams[rows, pick]


def _grey(values, least):
    gap = (values - least) / least if least > 0.0 else values
    return int(np.count_nonzero((gap > GREY[0]) & (gap < GREY[1])))


# ---- the whole call -----------------------------------------------------------------------------------------------------
def plan(x, conn, phi, w, d, d0, band=None, inf=R.INF, normal_sign=1.0):
    """Steps 2 and 3 of the contract up to the transport: dict(kind [nv], F [nv], n [nv, dim] -- the payload of the near
    vertices, 0 elsewhere --, ids [nv, k] (-1: none), wt [nv, k], grey, dropped -- transported vertices that lost a source to
    the causality rule --, orphans -- that lost all of them)."""
    conn = np.asarray(conn, dtype=np.int64)
    nvc = conn.shape[1]
    k = nvc - 1
    X = np.asarray(x, dtype=np.float64)[:, :k]
    nv = phi.size
    reached = (d < inf) & ((d <= band) if band is not None else True)
    kind = np.where(~reached, NONE, np.where(phi == 0.0, ZERO, np.where(d == d0, NEAR, TRANSPORTED)))
    F, n = np.zeros(nv), np.zeros((nv, k))
    ids, wt = np.full((nv, k), -1, dtype=np.int64), np.zeros((nv, k))
    cells_of = [[] for _ in range(nv)]
    for c in range(conn.shape[0]):
        for v in conn[c]:
            cells_of[v].append(c)
    seed = np.array([0 < s < nvc for s in (phi[conn] < 0.0).sum(axis=1)])
    grey = 0
    for v in np.nonzero(kind == ZERO)[0]:
        F[v] = w[v]
        cells = sorted(set(cells_of[v]))
        for wanted in (True, False):
            done = False
            for c in cells:
                if seed[c] == wanted:
                    nrm = cell_normal(X[conn[c]], phi[conn[c]], normal_sign)
                    if nrm is not None and (wanted or np.any(nrm != 0.0)):
                        n[v], done = nrm, True
                        break
            if done:
                break
    for v in np.nonzero(kind == NEAR)[0]:
        cand = []
        for c in sorted(set(cells_of[v])):
            if seed[c]:
                at = int(np.nonzero(conn[c] == v)[0][0])
                dist, lam = seed_closest(X[conn[c]], phi[conn[c]], at)
                cand.append((dist, c, lam))
        dists = np.array([q[0] for q in cand])
        grey += _grey(dists, dists.min())
        inside = [q for q in cand if q[0] <= (1.0 + WINDOW) * d0[v]]
        dist, c, lam = inside[0] if inside else min(cand, key=lambda q: (q[0], q[1]))
        F[v] = lam @ w[conn[c]]
        n[v] = cell_normal(X[conn[c]], phi[conn[c]], normal_sign)
    # transported: every (target, cell) pair of a transported target, the cell's other vertices in its own order
    tr = kind == TRANSPORTED
    tg, cl, src = [], [], []
    for i in range(nvc):
        rows = np.nonzero(tr[conn[:, i]])[0]
        tg.append(conn[rows, i]), cl.append(rows), src.append(conn[rows][:, [j for j in range(nvc) if j != i]])
    tg, cl, src = np.concatenate(tg), np.concatenate(cl), np.concatenate(src)
    dropped = orphans = 0
    if tg.size:
        P, dv = X[src] - X[tg][:, None, :], d[src]
        ok = (dv < inf) & ((dv <= band) if band is not None else True) & (src != tg[:, None])
        limit = (1.0 + WINDOW) * d[tg]
        vals, _ = subface_values(P, dv, ok, inf)
        _, value, lam = update_argmin(P, dv, ok, inf, limit)
        order = np.lexsort((cl, tg))
        starts = np.nonzero(np.r_[True, tg[order][1:] != tg[order][:-1]])[0]
        for a, b in zip(starts, np.r_[starts[1:], order.size]):
            rows = order[a:b]                                   # the pairs of one target, cells ascending
            t = tg[rows[0]]
            finite = vals[rows][vals[rows] < inf]
            if finite.size == 0:
                kind[t] = NONE
                continue
            grey += _grey(finite, finite.min())
            inside = rows[value[rows] <= limit[rows]]
            r = inside[0] if inside.size else rows[np.lexsort((cl[rows], value[rows]))[0]]
            keep = (lam[r] > 0.0) & (d[src[r]] < d[t]) & ok[r]
            dropped += int(np.any((lam[r] > 0.0) & ~keep))
            if not keep.any():
                orphans += 1
                kind[t] = NONE
                continue
            q = np.nonzero(keep)[0]
            ids[t, :q.size] = src[r][q]
            wt[t, :q.size] = lam[r][q] / lam[r][q].sum()
    return dict(kind=kind, F=F, n=n, ids=ids, wt=wt, grey=grey, dropped=dropped, orphans=orphans)


def _combine(F, n, ids, wt):
    """the payload of the transported rows ids / wt from the payload arrays F, n"""
    has = ids >= 0
    safe = np.where(has, ids, 0)
    lam = np.where(has, wt, 0.0)
    Fn = np.zeros(ids.shape[0])
    m = np.zeros((ids.shape[0], n.shape[1]))
    for i in range(ids.shape[1]):                               # (the order of the sum is the kernel's)
        Fn = Fn + lam[:, i] * F[safe[:, i]]
        m = m + lam[:, i, None] * n[safe[:, i]]
    length = np.linalg.norm(m, axis=1)
    heavy = n[safe[np.arange(ids.shape[0]), np.argmax(lam, axis=1)]]
    return Fn, np.where(length[:, None] > 0.0, m / np.where(length > 0.0, length, 1.0)[:, None], heavy)


def transport(pl, order="jacobi", max_sweeps=100000, chunk=97):
    """The payload of every vertex from a plan: (F, n, sweeps that changed a payload).  "jacobi": a sweep reads the
    payload of the sweep before; "inplace": the transported vertices are walked in chunks that see what the chunks before
    them wrote."""
    F, n = pl["F"].copy(), pl["n"].copy()
    rows = np.nonzero(pl["kind"] == TRANSPORTED)[0]
    for sweep in range(max_sweeps):
        changed = False
        parts = [rows] if order == "jacobi" else [rows[lo:lo + chunk] for lo in range(0, rows.size, chunk)]
        Fo, no = (F.copy(), n.copy()) if order == "jacobi" else (F, n)
        for part in parts:
            Fn, nn = _combine(Fo, no, pl["ids"][part], pl["wt"][part])
            changed = changed or Fn.tobytes() != F[part].tobytes() or nn.tobytes() != n[part].tobytes()
            F[part], n[part] = Fn, nn
        if not changed:
            return F, n, sweep
    raise RuntimeError("the transport did not reach its fixed point")


def extend(x, conn, phi, w, band=None, inf=R.INF, normal_sign=1.0, order="jacobi"):
    """The whole call: dict(reason, d, d0, signed_distance, kind, F, n, velocity, sweeps, transport_sweeps, grey, dropped,
    orphans, plan)."""
    phi, w = np.asarray(phi, dtype=np.float64), np.asarray(w, dtype=np.float64)
    d0 = R.nearfield(x, conn, phi, inf)
    if not np.any(d0 < inf):
        return dict(reason=R.NO_INTERFACE)
    d, sweeps = R.fim(x, conn, d0, band=band, inf=inf)
    pl = plan(x, conn, phi, w, d, d0, band=band, inf=inf, normal_sign=normal_sign)
    F, n, tsweeps = transport(pl, order=order)
    sd = np.where(phi >= 0.0, 1.0, -1.0) * (np.minimum(d, band) if band is not None else d)
    return dict(reason=R.CONVERGED, d=d, d0=d0, signed_distance=sd, kind=pl["kind"], F=F, n=n, velocity=F[:, None] * n,
                sweeps=sweeps, transport_sweeps=tsweeps, grey=pl["grey"], dropped=pl["dropped"], orphans=pl["orphans"], plan=pl)


# ---- cases --------------------------------------------------------------------------------------------------------------
PLANES = {"plane2": (2, 12, (0.6, 0.8), 0.71), "plane3": (3, 6, (0.48, 0.64, 0.6), 0.83)}
PLANE_G, PLANE_W0 = (1.3, -0.7, 0.9), 0.4
ASYM = ((0.47, 0.52, 0.55), 0.31)
ZEROS = "plane-3-4-0-50-p"           # an axis plane through a layer of vertices: phi == 0 on 25 of them
GPU_CASES = ["circle2", "sphere3", "scrambled3", "twospheres3", "corner3", "valence3big", "plane2", "plane3", "asym3", ZEROS]


def build_case(O, name):
    """(mesh, phi, w, h) of a named case: the planes of the exact test, the asymmetric sphere, or a case of
    reinit_ref.build_case with w = 1 + x_0 - 0.5 x_1"""
    if name in PLANES:
        tdim, nbox, a, c = PLANES[name]
        om = O.mesh_box(tdim, nbox)
        X = om.x[:, :tdim]
        return om, 1.7 * (X @ np.array(a) - c), X @ np.array(PLANE_G[:tdim]) + PLANE_W0, 1.0 / nbox
    if name == "asym3":
        om = O.mesh_box(3, 8)
        phi = R.quad_sphere(om.x, 3, ASYM[0], ASYM[1])
    else:
        om, phi = R.build_case(O, name)
    h = {"circle2": 1 / 16, ZEROS: 1 / 4}.get(name, 1 / 8)
    return om, phi, 1.0 + om.x[:, 0] - 0.5 * om.x[:, 1], h


_CACHE: dict = {}


def case(O, name, band_layers=None):
    """The case with its model result, computed once: the dict of extend() plus mesh, phi, w, h, band.  Nothing in it may
    be modified."""
    key = (name, band_layers)
    if key not in _CACHE:
        om, phi, w, h = build_case(O, name)
        band = None if band_layers is None else band_layers * h
        out = extend(om.x, om.conn, phi, w, band=band)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = dict(out, mesh=om, phi=phi, w=w, h=h, band=band)
    return _CACHE[key]


def plane_exact(name, x):
    """(distance to the plane, w at the foot, the normal a) of a plane case at the points x"""
    tdim, _, a, c = PLANES[name]
    a, X = np.array(a), np.asarray(x)[:, :tdim]
    s = X @ a - c
    foot = X - s[:, None] * a
    return np.abs(s), foot @ np.array(PLANE_G[:tdim]) + PLANE_W0, a
