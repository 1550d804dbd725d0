"""numpy model of the reinitialisation contract (include/cutfemx_amd.h, cfx_reinitialize), written from the contract:
sign, near field from the crossing points of the seed cells, the update U(t, K) as the least valid value over the finite
sub-faces, each in an orthonormal frame of its own, Jacobi sweeps to the exact fixed point.  Shared by
tests/test_reinit_reference.py (which pins it to mathematics) and the GPU tests (which compare the engine with it on the
same arrays).  Every case's model runs once.  The cell-local parts (nearfield, update) are themselves checked against
the independent references of tests/reinit_exact.py in tests/test_reinit_cell_reference.py."""
from __future__ import annotations

from itertools import combinations

import numpy as np

INF = 1e30
CONVERGED, MAX_ITER, NO_INTERFACE = 1, 2, 3
DEGENERATE = 1e-9     # the update: kDegenerate of cutfemx_amd/csrc/cfx_reinit_cell.h
FLAT_PIECE = 1e-20    # the near field: kFlatPiece


# ---- near field ---------------------------------------------------------------------------------------------------------
def _seg_dist2(p, a, b):
    ab, ap = b - a, p - a
    l2 = np.einsum("ij,ij->i", ab, ab)
    t = np.einsum("ij,ij->i", ab, ap)
    t = np.where(l2 > 0.0, np.clip(t / np.where(l2 > 0.0, l2, 1.0), 0.0, 1.0), 0.0)
    w = ap - t[:, None] * ab
    return np.einsum("ij,ij->i", w, w)


def _tri_dist2(p, a, b, c):
    r2 = np.minimum(np.minimum(_seg_dist2(p, a, b), _seg_dist2(p, b, c)), _seg_dist2(p, c, a))
    ab, ac, bc = b - a, c - a, c - b
    n = np.cross(ab, ac)
    nn = np.einsum("ij,ij->i", n, n)
    good = nn > FLAT_PIECE * np.einsum("ij,ij->i", ab, ab) * np.einsum("ij,ij->i", ac, ac)
    nn1 = np.where(good, nn, 1.0)
    s = np.einsum("ij,ij->i", n, p - a)
    q = p - n * (s / nn1)[:, None]
    e0 = np.einsum("ij,ij->i", np.cross(ab, q - a), n)
    e1 = np.einsum("ij,ij->i", np.cross(bc, q - b), n)
    e2 = np.einsum("ij,ij->i", np.cross(-ac, q - c), n)
    inside = good & (e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)
    return np.where(inside, np.minimum(r2, s * s / nn1), r2)


def _crossing(X, phi, vi, vj):
    """p_ij = x_i + phi_i / (phi_i - phi_j) (x_j - x_i), taken from the negative end."""
    swap = ~(phi[vi] < 0.0)
    i, j = np.where(swap, vj, vi), np.where(swap, vi, vj)
    t = phi[i] / (phi[i] - phi[j])
    return X[i] + t[:, None] * (X[j] - X[i])


def nearfield(x, conn, phi, inf=INF):
    """d0 of the contract: distance of every vertex of a seed cell to the cell's interface piece, minimum over the seed
    cells around the vertex; 0 on exact zeros; `inf` elsewhere."""
    conn = np.asarray(conn, dtype=np.int64)
    nv = conn.shape[1]
    tdim = nv - 1
    X = np.asarray(x, dtype=np.float64)[:, :tdim]
    neg = phi[conn] < 0.0
    nneg = neg.sum(axis=1)
    d0 = np.full(phi.size, inf)

    def lower(cells, pieces):
        for i in range(nv):
            v = conn[cells, i]
            r2 = None
            for piece in pieces:
                d2 = _seg_dist2(X[v], *piece) if tdim == 2 else _tri_dist2(X[v], *piece)
                r2 = d2 if r2 is None else np.minimum(r2, d2)
            np.minimum.at(d0, v, np.sqrt(r2))

    for lone_neg in (True, False):                      # one vertex alone on its side
        cells = np.nonzero(nneg == (1 if lone_neg else tdim))[0]
        if cells.size:
            l = np.argmax(neg[cells] == lone_neg, axis=1)
            others = [(l + k) % nv for k in range(1, nv)]
            vl = conn[cells, l]
            pts = [_crossing(X, phi, vl, conn[cells, o]) for o in others]
            lower(cells, [tuple(pts)])
    if tdim == 3:                                       # two and two: the quadrilateral ac, ad, bd, bc
        cells = np.nonzero(nneg == 2)[0]
        if cells.size:
            order = np.argsort(~neg[cells], axis=1, kind="stable")      # negatives first, local order kept
            a, b, c, d = (conn[cells, order[:, k]] for k in range(4))
            P = [_crossing(X, phi, a, c), _crossing(X, phi, a, d), _crossing(X, phi, b, d), _crossing(X, phi, b, c)]
            lower(cells, [(P[0], P[1], P[2]), (P[0], P[2], P[3])])
    d0[phi == 0.0] = 0.0
    return d0


# ---- the update ---------------------------------------------------------------------------------------------------------
def _subface_value(Ps, ds, inf):
    """The minimum of d + |x_t - y| over the PLANE of a sub-face of two or three sources, where it lies in the sub-face,
    else inf.  In an orthonormal frame (u_1, ...) of the sub-face: g the gradient of d within it, z the foot of the
    perpendicular from the target, h its height; U = d(z) + h sqrt(1 - |g|^2) at y = z - h g / sqrt(1 - |g|^2)."""
    m, size, _ = Ps.shape
    val = np.full(m, inf)
    E = Ps[:, 1:, :] - Ps[:, :1, :]                           # edges from the first source
    delta = ds[:, 1:] - ds[:, :1]
    l1 = np.linalg.norm(E[:, 0], axis=1)
    good = l1 > 0.0
    if size == 3:
        e2e2 = np.einsum("mk,mk->m", E[:, 1], E[:, 1])
        with np.errstate(all="ignore"):
            u1 = E[:, 0] / l1[:, None]
            w = E[:, 1] - np.einsum("mk,mk->m", E[:, 1], u1)[:, None] * u1
            ww = np.einsum("mk,mk->m", w, w)
        good &= ww > DEGENERATE * e2e2                        # sin^2 of the angle at the first source
    rows = np.nonzero(good)[0]
    if rows.size == 0:
        return val
    E, delta, P0, d0 = E[rows], delta[rows], Ps[rows, 0], ds[rows, 0]
    # frame and the edges' coordinates in it: E = C U, C lower triangular
    U = np.zeros((rows.size, size - 1, E.shape[2]))
    U[:, 0] = E[:, 0] / np.linalg.norm(E[:, 0], axis=1)[:, None]
    if size == 3:
        w = E[:, 1] - np.einsum("mk,mk->m", E[:, 1], U[:, 0])[:, None] * U[:, 0]
        U[:, 1] = w / np.linalg.norm(w, axis=1)[:, None]
    Cm = np.einsum("mik,mjk->mij", E, U)
    g = np.linalg.solve(Cm, delta[:, :, None])[:, :, 0]       # gradient in the frame
    gg = 1.0 - np.einsum("mi,mi->m", g, g)
    real = gg > 0.0
    root = np.sqrt(np.where(real, gg, 1.0))
    pt = np.einsum("mik,mk->mi", U, P0)                       # the first source in the frame (the target is the origin)
    z = P0 - np.einsum("mi,mik->mk", pt, U)                   # foot of the perpendicular
    h = np.linalg.norm(z, axis=1)
    y = -pt - (h / root)[:, None] * g                         # y - P0 in the frame
    lam = np.linalg.solve(np.swapaxes(Cm, 1, 2), y[:, :, None])[:, :, 0]
    valid = real & np.all(lam >= 0.0, axis=1) & (lam.sum(axis=1) <= 1.0)
    val[rows] = np.where(valid, d0 - np.einsum("mi,mi->m", g, pt) + h * root, inf)
    return val


def update(P, dv, ok, inf=INF):
    """U for m (target, cell) pairs: P[m, k, dim] = x_s - x_t and dv[m, k] of the k other vertices, ok[m, k] usable.
    The least valid value over every non-empty sub-face (a single source is always valid; a face of three sources whose
    sin^2 at its first source is not above DEGENERATE is left to its sub-faces)."""
    m, k, _ = P.shape
    best = np.full(m, inf)
    for size in range(1, k + 1):
        for S in combinations(range(k), size):
            S = list(S)
            rows = np.nonzero(np.all(ok[:, S], axis=1))[0]
            if rows.size == 0:
                continue
            Ps, ds = P[rows][:, S, :], dv[rows][:, S]
            if size == 1:
                val = ds[:, 0] + np.linalg.norm(Ps[:, 0], axis=1)
            else:
                val = _subface_value(Ps, ds, inf)
            best[rows] = np.minimum(best[rows], val)
    return best


def _pairs(x, conn):
    """Every (target, cell) pair: targets[m], sources[m, k] and P[m, k, dim]."""
    conn = np.asarray(conn, dtype=np.int64)
    nv = conn.shape[1]
    tdim = nv - 1
    X = np.asarray(x, dtype=np.float64)[:, :tdim]
    tg = np.concatenate([conn[:, i] for i in range(nv)])
    src = np.concatenate([conn[:, [j for j in range(nv) if j != i]] for i in range(nv)])
    return tg, src, X[src] - X[tg][:, None, :]


def fim(x, conn, d0, band=None, inf=INF, order="jacobi", max_sweeps=100000, chunk=97):
    """The iteration d_t <- min(d_t, min_K U(t, K)) from d0 to its exact fixed point; returns (d, sweeps that changed a
    value or were needed to see that none does).  order "jacobi": every update of a sweep reads the values of the sweep
    before; "inplace": the (target, cell) pairs are walked in chunks and every chunk sees the values the chunks before
    it wrote.  band: a value is a source only while it is <= band (the result is NOT clamped here)."""
    tg, src, P = _pairs(x, conn)
    d = d0.copy()

    def usable(v):
        return (v < inf) & ((v <= band) if band is not None else True)

    for sweep in range(max_sweeps):
        if order == "jacobi":
            dv = d[src]
            U = update(P, dv, usable(dv), inf)
            new = d.copy()
            np.minimum.at(new, tg, U)
            changed = bool(np.any(new < d))
            d = new
        else:
            changed = False
            for lo in range(0, tg.size, chunk):
                sl = slice(lo, lo + chunk)
                dv = d[src[sl]]
                U = update(P[sl], dv, usable(dv), inf)
                before = d[tg[sl]].copy()
                np.minimum.at(d, tg[sl], U)
                changed = changed or bool(np.any(d[tg[sl]] < before))
        if not changed:
            return d, sweep
    raise RuntimeError("the model did not reach its fixed point")


def reinit(x, conn, phi, band=None, inf=INF, order="jacobi"):
    """The whole call: (new phi, sweeps, reason)."""
    phi = np.asarray(phi, dtype=np.float64)
    d0 = nearfield(x, conn, phi, inf)
    if not np.any(d0 < inf):
        return phi.copy(), 0, NO_INTERFACE
    d, sweeps = fim(x, conn, d0, band=band, inf=inf, order=order)
    if band is not None:
        d = np.minimum(d, band)
    return np.where(phi >= 0.0, 1.0, -1.0) * d, sweeps, CONVERGED


# ---- cases --------------------------------------------------------------------------------------------------------------
def quad_sphere(x, tdim, centre=0.5, radius=0.3):
    """|x - m|^2 - r^2: the level set of the reference's sphere test (python/tests/test_distance.py:30-54), not a distance."""
    m = np.full(tdim, centre) if np.isscalar(centre) else np.asarray(centre, dtype=np.float64)
    return np.sum((x[:, :tdim] - m) ** 2, axis=1) - radius ** 2


def exact_sphere(x, tdim, centre=0.5, radius=0.3):
    m = np.full(tdim, centre) if np.isscalar(centre) else np.asarray(centre, dtype=np.float64)
    return np.linalg.norm(x[:, :tdim] - m, axis=1) - radius


def build_case(O, name):
    """(mesh, phi) of a named case; mesh has tdim, x [nv, 3] and conn."""
    import helpers as H
    if name.startswith("plane"):                       # plane-<tdim>-<n>-<axis>-<c in percent>-<sign>
        _, tdim, n, k, c, sgn = name.split("-")
        om = O.mesh_box(int(tdim), int(n))
        a = 1.7 if sgn == "p" else -0.6
        return om, a * (om.x[:, int(k)] - int(c) / 100.0)
    if name in ("circle2", "sphere3"):
        tdim = int(name[-1])
        om = O.mesh_box(tdim, 16 if tdim == 2 else 8)
        return om, quad_sphere(om.x, tdim)
    if name == "scrambled3":
        om = H.scrambled_mesh(O, 3, 8)
        return om, quad_sphere(om.x, 3)
    if name == "valence2":
        om, phi, _ = H.high_valence_case(O, 2, 30)
        return om, phi
    if name == "valence3":
        om, phi, _ = H.high_valence_case(O, 3, (6, 6))
        return om, phi
    if name == "valence3big":                          # an apex with 82 neighbours: beyond the 62 a stencil list holds
        om, phi, _ = H.high_valence_case(O, 3, (8, 8))
        return om, phi
    if name == "twospheres3":                          # two fronts that meet
        om = O.mesh_box(3, 8)
        return om, np.minimum(quad_sphere(om.x, 3, (0.3, 0.3, 0.3), 0.2), quad_sphere(om.x, 3, (0.7, 0.7, 0.65), 0.2))
    if name == "corner3":                              # seeds on the boundary, vertices with few cells
        om = O.mesh_box(3, 8)
        return om, quad_sphere(om.x, 3, 0.0, 0.45)
    if name == "corner2":
        om = O.mesh_box(2, 16)
        return om, quad_sphere(om.x, 2, 0.0, 0.45)
    if name == "positive3":
        om = O.mesh_box(3, 4)
        return om, 1.0 + om.x[:, 0]
    raise KeyError(name)


_CACHE: dict = {}


def case(O, name, band_layers=None):
    """The case with its model result, computed once: dict(mesh, phi, out, sweeps, reason, h) -- `out` must not be
    modified.  band_layers: max_distance = band_layers * h, h = 1 / n of the case's box."""
    key = (name, band_layers)
    if key not in _CACHE:
        om, phi = build_case(O, name)
        h = {"circle2": 1 / 16, "corner2": 1 / 16}.get(name, 1 / 8)
        band = None if band_layers is None else band_layers * h
        out, sweeps, reason = reinit(om.x, om.conn, phi, band=band)
        out.setflags(write=False)
        _CACHE[key] = dict(mesh=om, phi=phi, out=out, sweeps=sweeps, reason=reason, h=h, band=band)
    return _CACHE[key]
