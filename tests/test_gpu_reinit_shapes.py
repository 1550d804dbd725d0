"""cutfemx_amd.distance.reinitialize as a whole call on the smallest meshes that show each effect, against references
that do not share its formulas (tests/reinit_exact.py):

Bellman residual  the engine's |phi| is the fixed point d_t = min(d0_t, min_K U(t, K)) of the contract, with U from the
                  long-double minimiser and d0 from the exact near field -- on plain and squeezed boxes.  Every value
                  derives from strictly smaller ones, so the fixed point is unique: one reference sweep characterises it.
scaling           coordinates and phi times 2^-20 and 2^20 give the scaled result
zeros             -0.0 and +0.0, and a mesh whose only seeds are exact zeros
band edge         max_distance exactly at a value the unbanded run produces, and one ulp below it"""
from types import SimpleNamespace

import numpy as np
import pytest

import reinit_exact as E
import reinit_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
_SPACES: dict = {}


def _space(om):
    import cutfemx_amd as cfx
    if id(om) not in _SPACES:
        mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
        _SPACES[id(om)] = (om, cfx.FunctionSpace(mesh, 1))
    return _SPACES[id(om)][1]


def _run(om, phi, **kw):
    import cutfemx_amd as cfx
    fn = cfx.Function(_space(om), values=np.array(phi, dtype=np.float64))
    info = cfx.distance.reinitialize(fn, **kw)
    return fn.values, info


def _scaled(om, scale):
    return SimpleNamespace(tdim=om.tdim, x=om.x * np.asarray(scale, dtype=np.float64), conn=om.conn)


def _longest_edge(om):
    X = om.x[:, :om.tdim][om.conn]
    nv = om.conn.shape[1]
    return max(float(np.max(np.linalg.norm(X[:, i] - X[:, j], axis=1))) for i in range(nv) for j in range(i))


# ---- Bellman residual ---------------------------------------------------------------------------------------------------
def _squeezes(tdim):
    out = [("plain", np.ones(3))]
    for ratio in ((1e-1, 1e-3) if tdim == 3 else (1e-3,)):
        for axis in range(tdim):
            s = np.ones(3)
            s[axis] = ratio
            out.append((f"{ratio:g} along {axis}", s))
    return out


BELLMAN = [(tdim, name) for tdim in (3, 2) for name, _ in _squeezes(tdim)]


def _level_set(unit_x, tdim, which):
    """on the coordinates of the box before it is squeezed: the values are an input like any other"""
    if which == "sphere":
        return R.quad_sphere(unit_x, tdim)
    n = np.array([0.6, 0.48, 0.64]) if tdim == 3 else np.array([0.6, 0.8])
    return 1.3 * (unit_x[:, :tdim] @ n - 0.47 * n.sum())


def _exact_nearfield(om, phi, inf):
    X = om.x[:, :om.tdim]
    d0 = np.full(phi.size, inf)
    for cell in om.conn:
        flag, dist = E.exact_seed(X[cell], phi[cell])
        if flag:
            np.minimum.at(d0, cell, dist)
    d0[phi == 0.0] = 0.0
    return d0


@pytest.mark.parametrize("which", ["sphere", "plane"])
@pytest.mark.parametrize("tdim,squeeze", BELLMAN)
def test_bellman_residual(oracle, tdim, squeeze, which):
    unit = oracle.mesh_box(tdim, 4 if tdim == 3 else 8)
    om = _scaled(unit, dict(_squeezes(tdim))[squeeze])
    phi = _level_set(unit.x, tdim, which)
    out, info = _run(om, phi)
    assert info.converged
    d = np.abs(out)
    assert np.all(d < 0.5 * R.INF)
    d0 = _exact_nearfield(om, phi, R.INF)
    assert info.seeds == int(np.count_nonzero(d0 < R.INF))
    tg, src, P = R._pairs(om.x, om.conn)
    U = E.brute_update(P, d[src], np.ones(src.shape, dtype=bool), R.INF)
    want = d0.astype(np.longdouble)
    np.minimum.at(want, tg, U)
    L = _longest_edge(om)
    res = ((d - want) / L).astype(np.float64)
    print(f"{tdim}-D {squeeze} {which}: {d.size} vertices, {tg.size} pairs, {info.seeds} seeds, {info.sweeps} sweeps, "
          f"d - min(d0, min U) in [{res.min():+.2e}, {res.max():+.2e}] L, L = {L:.3g}")
    assert np.all(np.abs(res) <= 1e-12)
    assert np.array_equal(out >= 0.0, phi >= 0.0)


# ---- scaling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere3", "circle2"])
def test_scaling_by_powers_of_two(oracle, name):
    om, phi = R.build_case(oracle, name)
    base, info = _run(om, phi)
    for k in (-20, 20):
        s = 2.0 ** k
        out, info_s = _run(_scaled(om, s), phi * s)
        rel = float(np.max(np.abs(out / s - base)) / np.max(np.abs(base)))
        same = out.tobytes() == (base * s).tobytes()
        print(f"{name} x 2^{k}: relative difference {rel:.2e}, bit-identical: {same}, sweeps {info_s.sweeps} ({info.sweeps})")
        assert rel <= 1e-12
        assert (info_s.reason, info_s.seeds) == (info.reason, info.seeds)


# ---- zeros --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdim,n", [(2, 8), (3, 4)])
def test_signed_zeros(oracle, tdim, n):
    """the plane x_0 = 1/2 lies on vertices: half of the zeros are given as -0.0; every one comes back as +0.0, counts as
    non-negative, and the result is the plane's distance with the input's signs"""
    import cutfemx_amd as cfx
    om, phi = R.build_case(oracle, f"plane-{tdim}-{n}-0-50-p")
    phi = phi.copy()
    zeros = np.nonzero(phi == 0.0)[0]
    assert zeros.size == (n + 1) ** (tdim - 1)
    phi[zeros[::2]] = -0.0
    assert np.signbit(phi[zeros[0]]) and not np.signbit(phi[zeros[1]])
    out, info = _run(om, phi)
    model, _, reason = R.reinit(om.x, om.conn, phi)
    assert info.reason == cfx.distance.REINIT_CONVERGED and reason == R.CONVERGED
    assert np.all(out[zeros] == 0.0) and not np.any(np.signbit(out[zeros]))
    assert np.max(np.abs(out - (om.x[:, 0] - 0.5))) <= 1e-12 and np.max(np.abs(out - model)) <= 1e-12
    assert np.array_equal(out >= 0.0, phi >= 0.0)
    d0 = R.nearfield(om.x, om.conn, phi)
    assert info.seeds == int(np.count_nonzero(d0 < R.INF))


@pytest.mark.parametrize("tdim,n", [(2, 8), (3, 4)])
def test_only_exact_zeros_seed(oracle, tdim, n):
    """phi = 1.7 |x_0 - 1/2| >= 0: no edge is crossed, the plane of zeros is the only seed, and the call converges to the
    distance from it, all non-negative"""
    import cutfemx_amd as cfx
    om, plane = R.build_case(oracle, f"plane-{tdim}-{n}-0-50-p")
    phi = np.abs(plane)
    phi[::3] = np.where(phi[::3] == 0.0, -0.0, phi[::3])
    out, info = _run(om, phi)
    assert info.reason == cfx.distance.REINIT_CONVERGED
    assert info.seeds == int(np.count_nonzero(phi == 0.0)) == (n + 1) ** (tdim - 1)
    err = float(np.max(np.abs(out - np.abs(om.x[:, 0] - 0.5))))
    print(f"{tdim}-D: only zeros seed: err {err:.2e}, sweeps {info.sweeps}")
    assert err <= 1e-12
    assert np.all(out >= 0.0) and not np.any(np.signbit(out))


# ---- band edge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner3", "corner2"])
def test_band_edge(oracle, name):
    """w: a vertex in the middle of the range; B: the least unbanded value among its neighbours, at the vertices v.  With
    max_distance = B the v are sources and put w on a list; with one ulp less no neighbour of w is a source (all are
    >= B), so w is never recomputed.  The values up to the band have the same history in all three runs: same bits."""
    c = R.case(oracle, name)
    om, phi = c["mesh"], c["phi"]
    full, info_full = _run(om, phi)
    d = np.abs(full)
    conn = np.asarray(om.conn)
    w = int(np.argsort(d)[d.size // 2])
    nbrs = np.setdiff1d(np.unique(conn[np.any(conn == w, axis=1)]), [w])
    B = float(d[nbrs].min())
    below = float(np.nextafter(B, 0.0))
    v = nbrs[d[nbrs] == B]
    assert 0.0 < below < B < d[w]
    at, info_at = _run(om, phi, max_distance=B)
    under, info_under = _run(om, phi, max_distance=below)
    sign = np.where(phi >= 0.0, 1.0, -1.0)
    assert at.tobytes() == (sign * np.minimum(d, B)).tobytes()
    assert under.tobytes() == (sign * np.minimum(d, below)).tobytes()
    assert np.all(np.abs(at[v]) == B) and np.all(np.abs(under[v]) == below)
    print(f"{name}: B = {B!r} at {v.size} neighbours of vertex {w}; updates {info_under.updates} (one ulp below), "
          f"{info_at.updates} (at B), {info_full.updates} (no band)")
    assert info_at.converged and info_under.converged
    assert info_under.updates < info_at.updates < info_full.updates
    assert info_under.seeds == info_at.seeds == info_full.seeds
    for band, out in ((B, at), (below, under)):
        model, _, _ = R.reinit(om.x, om.conn, phi, band=band)
        assert np.max(np.abs(out - model)) <= TOL
