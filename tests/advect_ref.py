"""numpy model of cutfemx_amd.distance.advect (the contract in include/cutfemx_amd.h): the cell -> cell table from a
dictionary of facets, the visibility walk in the operand order of cutfemx_amd/csrc/cfx_advect_cell.h, a brute-force locator
that knows nothing of the walk, and the closed forms of affine fields.  Every function takes a dtype: the float64 model
against the same model in np.longdouble is the noise floor of the arithmetic (FLOOR below)."""
import numpy as np

import reinit_ref as R

INSIDE_TOL = 1e-12
GREY = (1e-14, 1e-10)          # a best min lambda in (-1e-10, -1e-14): "inside" would hang on the rounding
LOCATED, OUTSIDE, CAPPED, SKIPPED = 1, 2, 3, 4

# The largest |float64 model - long double model| / max|phi| over CASES x fields x orders, measured by
# tests/test_advect_reference.py::test_noise_floor (which asserts that no case exceeds the constant): per mesh box3 2.1e-15,
# scrambled3 2.84e-15 (CFL 12, sphere, order 2: departure points far outside the box, where the lambda of the extension
# are large), box2 1.7e-15, valence3 3.8e-16.  The constant is the largest rounded up; the tests allow 16 x it, relative to
# max|phi|: 4.8e-14, far below the 1e-11 at which something would have to be looked into.
FLOOR = 3e-15
TOL = 16 * FLOOR


# ---- the table ------------------------------------------------------------------------------------------------------------
def neighbours(conn):
    """int32 [ncells, nv]: the cell across the facet opposite local vertex i, -1 on the boundary"""
    conn = np.asarray(conn)
    nc, nv = conn.shape
    seen: dict = {}
    for c in range(nc):
        row = conn[c]
        for i in range(nv):
            seen.setdefault(tuple(sorted(int(row[j]) for j in range(nv) if j != i)), []).append((c, i))
    out = np.full((nc, nv), -1, dtype=np.int32)
    for pair in seen.values():
        assert len(pair) <= 2, "a facet of more than two cells"
        if len(pair) == 2:
            (a, i), (b, j) = pair
            out[a, i], out[b, j] = b, a
    return out


def first_cells(conn, nv):
    """the lowest-numbered cell incident to every vertex (-1: none)"""
    conn = np.asarray(conn)
    first = np.full(nv, conn.shape[0], dtype=np.int64)
    np.minimum.at(first, conn.ravel(), np.repeat(np.arange(conn.shape[0]), conn.shape[1]))
    first[first == conn.shape[0]] = -1
    return first


# ---- one cell -------------------------------------------------------------------------------------------------------------
def _det2(a, b):
    return a[0] * b[1] - a[1] * b[0]


def _det3(a, b, c):
    return a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0])


def barycentric(X, p):
    """lambda [..., nv] of p [..., dim] in the cells X [..., nv, dim], in the dtype of X: Cramer's rule on the edge matrix in
    the header's operand order, lambda_0 = 1 - the others"""
    dim = X.shape[-1]
    one = X.dtype.type(1)
    r = [p[..., k] - X[..., 0, k] for k in range(dim)]
    E = [[X[..., j + 1, k] - X[..., 0, k] for k in range(dim)] for j in range(dim)]
    with np.errstate(all="ignore"):
        if dim == 2:
            det = _det2(E[0], E[1])
            l1, l2 = _det2(r, E[1]) / det, _det2(E[0], r) / det
            return np.stack([one - (l1 + l2), l1, l2], axis=-1)
        det = _det3(E[0], E[1], E[2])
        l1, l2, l3 = _det3(r, E[1], E[2]) / det, _det3(E[0], r, E[2]) / det, _det3(E[0], E[1], r) / det
        return np.stack([one - ((l1 + l2) + l3), l1, l2, l3], axis=-1)


def visit(X, p, tol=INSIDE_TOL):
    """(lambda, -1 or the facet to cross) of one cell: the header's visit()"""
    lam = barycentric(X, p)
    inside, facet, least = True, 0, lam[0]
    for i in range(lam.size):
        inside = inside and bool(lam[i] >= -tol)
        if lam[i] < least:
            least, facet = lam[i], i
    return lam, (-1 if inside else facet)


def interpolate(lam, f):
    s = lam[0] * f[0]
    for i in range(1, lam.size):
        s = s + lam[i] * f[i]
    return s


# ---- the walk and the call --------------------------------------------------------------------------------------------------
def walk(x, conn, nbr, p, c, steps, max_steps, tol=INSIDE_TOL):
    """from cell c to the target p: (status, final cell, lambda there, crossings so far)"""
    dim = conn.shape[1] - 1
    while True:
        lam, facet = visit(x[conn[c], :dim], p, tol)
        if facet < 0:
            return LOCATED, c, lam, steps
        nxt = int(nbr[c, facet])
        if nxt < 0:
            return OUTSIDE, c, lam, steps
        if steps >= max_steps:
            return CAPPED, c, lam, steps
        steps += 1
        c = nxt


def advect(x, conn, phi, vel, dt, order=2, band=None, tol=INSIDE_TOL, max_steps=4096, dtype=np.float64, nbr=None):
    """The contract, vertex by vertex.  dict(out, cells, status, walk [nv] crossings per vertex, half / dep [nv, dim] the
    targets (NaN rows where none was formed), located, outside, capped, skipped, steps, max_walk)"""
    conn = np.asarray(conn)
    dim = conn.shape[1] - 1
    nv = x.shape[0]
    nbr = neighbours(conn) if nbr is None else nbr
    first = first_cells(conn, nv)
    xs, f, w_all = x.astype(dtype), np.asarray(phi).astype(dtype), np.asarray(vel).reshape(nv, dim).astype(dtype)
    dt_, half_dt = dtype(dt), dtype(0.5) * dtype(dt)
    out, cells = f.copy(), np.full(nv, -1, dtype=np.int32)
    status, crossings = np.zeros(nv, dtype=np.int32), np.zeros(nv, dtype=np.int64)
    half, dep = np.full((nv, dim), np.nan, dtype=dtype), np.full((nv, dim), np.nan, dtype=dtype)
    for v in range(nv):
        if band is not None and band > 0.0 and abs(f[v]) > band:
            status[v] = SKIPPED
            continue
        if first[v] < 0:
            status[v] = OUTSIDE
            continue
        xv, w, c, steps = xs[v, :dim], w_all[v], int(first[v]), 0
        st = LOCATED
        with np.errstate(all="ignore"):
            if order == 2:
                p = xv - half_dt * w
                half[v] = p
                if p.tobytes() != xv.tobytes():
                    if not np.all(np.isfinite(p)):
                        st = CAPPED
                    else:
                        st, c, lam, steps = walk(xs, conn, nbr, p, c, steps, max_steps, tol)
                        if st != CAPPED:
                            w = np.array([interpolate(lam, w_all[conn[c], k]) for k in range(dim)], dtype=dtype)
            if st != CAPPED:
                p = xv - dt_ * w
                dep[v] = p
                if p.tobytes() == xv.tobytes():
                    st, cells[v] = LOCATED, first[v]
                elif not np.all(np.isfinite(p)):
                    st = CAPPED
                else:
                    st, c, lam, steps = walk(xs, conn, nbr, p, c, steps, max_steps, tol)
                    if st != CAPPED:
                        out[v] = interpolate(lam, f[conn[c]])
                        cells[v] = c
        status[v], crossings[v] = st, steps
    count = lambda s: int(np.count_nonzero(status == s))
    return dict(out=out, cells=cells, status=status, walk=crossings, half=half, dep=dep, located=count(LOCATED), outside=count(OUTSIDE),
                capped=count(CAPPED), skipped=count(SKIPPED), steps=int(crossings.sum()), max_walk=int(crossings.max()))


# ---- independent of the walk ---------------------------------------------------------------------------------------------
def brute_locate(x, conn, points, dtype=np.longdouble):
    """over all cells the one with the largest min lambda: (cell [m], that min lambda [m], lambda there [m, nv]); rows of
    `points` with a NaN give cell -1"""
    conn = np.asarray(conn)
    dim = conn.shape[1] - 1
    X = x[conn][:, :, :dim].astype(dtype)
    m = points.shape[0]
    cell, best, lam_at = np.full(m, -1, dtype=np.int64), np.full(m, -np.inf), np.zeros((m, dim + 1), dtype=dtype)
    for k in range(m):
        if not np.all(np.isfinite(points[k])):
            continue
        lam = barycentric(X, points[k].astype(dtype)[None, :])
        least = lam.min(axis=1)
        c = int(np.argmax(least))
        cell[k], best[k], lam_at[k] = c, float(least[c]), lam[c]
    return cell, best, lam_at


def grey_count(best):
    """vertices whose best min lambda lies in (-1e-10, -1e-14)"""
    return int(np.count_nonzero((best < -GREY[0]) & (best > -GREY[1])))


# ---- fields and closed forms -------------------------------------------------------------------------------------------------
def skew(dim):
    return np.array([[0.0, -1.0], [1.0, 0.0]]) if dim == 2 else np.array([[0.0, -1.0, 0.6], [1.0, 0.0, -0.8], [-0.6, 0.8, 0.0]])


def affine_velocity(x, dim):
    """A (x - 0.5) + 0.1 with A skew: (values [nv, dim], A, b) with velocity = A x + b"""
    A = skew(dim)
    b = 0.1 - A @ np.full(dim, 0.5)
    return x[:, :dim] @ A.T + b, A, b


def affine_phi(x, dim):
    g = np.array([0.6, -0.8, 0.35])[:dim]
    return x[:, :dim] @ g - 0.13, g, -0.13


def affine_exact(x, dim, dt, order):
    """phi(x_dep) of the affine fields in long double: x_dep = x - dt (A (x - dt/2 (A x + b)) + b), or x - dt (A x + b)"""
    ld = np.longdouble
    _, A, b = affine_velocity(x, dim)
    _, g, c = affine_phi(x, dim)
    X, A, b, g = x[:, :dim].astype(ld), A.astype(ld), b.astype(ld), g.astype(ld)
    v = X @ A.T + b
    if order == 2:
        v = (X - ld(0.5) * ld(dt) * v) @ A.T + b
    return (X - ld(dt) * v) @ g + ld(c)


def rotating_velocity(x, dim):
    return (x[:, :dim] - 0.5) @ skew(dim).T


# ---- cases ----------------------------------------------------------------------------------------------------------------------
CASES = {"box3": (0.3, 2.5, 12.0), "scrambled3": (0.3, 2.5, 12.0), "box2": (0.3, 2.5, 12.0), "valence3": (0.3, 2.5)}
_MESH: dict = {}
_MODEL: dict = {}


def mesh(O, name):
    """(mesh, cell -> cell table, h) of a named case, built once"""
    import helpers as H
    if name not in _MESH:
        if name == "box3":
            om, h = O.mesh_box(3, 8), 1 / 8
        elif name == "scrambled3":
            om, h = H.scrambled_mesh(O, 3, 8), 1 / 8
        elif name == "box2":
            om, h = O.mesh_box(2, 16), 1 / 16
        elif name == "valence3":
            om, h = H.high_valence_case(O, 3, (8, 8))[0], 1 / 8
        else:
            raise KeyError(name)
        _MESH[name] = (om, neighbours(om.conn), h)
    return _MESH[name]


def fields(O, name, field):
    """(phi, velocity [nv, dim]): 'affine' -- both affine; 'sphere' -- the quadratic sphere in a rotation"""
    om = mesh(O, name)[0]
    if field == "affine":
        return affine_phi(om.x, om.tdim)[0], affine_velocity(om.x, om.tdim)[0]
    return R.quad_sphere(om.x, om.tdim), rotating_velocity(om.x, om.tdim)


def time_step(O, name, field, cfl):
    """dt with dt max|velocity| = cfl h"""
    _, vel = fields(O, name, field)
    return cfl * mesh(O, name)[2] / float(np.max(np.linalg.norm(vel, axis=1)))


def model(O, name, field, cfl, order, band=None, dtype=np.float64, max_steps=4096):
    """the model's result on a case, computed once (do not modify)"""
    key = (name, field, cfl, order, band, np.dtype(dtype).name, max_steps)
    if key not in _MODEL:
        om, nbr, _ = mesh(O, name)
        phi, vel = fields(O, name, field)
        _MODEL[key] = advect(om.x, om.conn, phi, vel, time_step(O, name, field, cfl), order=order, band=band, dtype=dtype, nbr=nbr,
                             max_steps=max_steps)
    return _MODEL[key]
