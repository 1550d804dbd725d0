"""The numpy model of the reinitialisation contract (tests/reinit_ref.py) pinned to mathematics, so that the GPU tests
compare the engine with something independent: exact distances to axis planes, the reference's sphere property
(python/tests/test_distance.py:30-54), independence of the update order, the band, and the library's defaults."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import reinit_ref as R

PLANES = [(2, 8), (3, 4), (3, 8)]


@pytest.mark.parametrize("tdim,n", PLANES)
@pytest.mark.parametrize("c", [57, 50])
def test_axis_planes_are_exact(oracle, tdim, n, c):
    """phi = a (x_k - c), a = 1.7 and -0.6: the result is +-(x_k - c) to 1e-12 (the tolerance of the reference's own
    plane test, python/tests/test_distance.py:114); c = 0.5 lies on vertices (n even), which stay exactly 0."""
    for k in range(tdim):
        for sgn, s in (("p", 1.0), ("m", -1.0)):
            om, phi = R.build_case(oracle, f"plane-{tdim}-{n}-{k}-{c}-{sgn}")
            out, sweeps, reason = R.reinit(om.x, om.conn, phi)
            exact = s * (om.x[:, k] - c / 100.0)
            err = float(np.max(np.abs(out - exact)))
            print(f"plane tdim {tdim} n {n} axis {k} c {c} sign {sgn}: err {err:.2e} sweeps {sweeps}")
            assert reason == R.CONVERGED and err <= 1e-12
            on = phi == 0.0
            assert on.any() == (c == 50)
            assert np.all(out[on] == 0.0) and not np.any(np.signbit(out[on]))
            assert np.array_equal(out >= 0.0, phi >= 0.0)


@pytest.mark.parametrize("name", ["circle2", "sphere3"])
def test_sphere_property(oracle, name):
    c = R.case(oracle, name)
    tdim = c["mesh"].tdim
    exact = R.exact_sphere(c["mesh"].x, tdim)
    moved = float(np.max(np.abs(c["out"] - c["phi"])))
    after, before = float(np.max(np.abs(c["out"] - exact))), float(np.max(np.abs(c["phi"] - exact)))
    print(f"{name}: moved {moved:.3e} after {after:.3e} before {before:.3e} sweeps {c['sweeps']}")
    assert c["reason"] == R.CONVERGED
    assert moved > 1e-3 and after < 0.5 * before
    assert np.all(np.abs(c["out"]) < 0.5 * R.INF)          # no vertex unreached


@pytest.mark.parametrize("name", ["scrambled3", "twospheres3"])
def test_order_independence(oracle, name):
    c = R.case(oracle, name)
    om = c["mesh"]
    d0 = R.nearfield(om.x, om.conn, c["phi"])
    d, _ = R.fim(om.x, om.conn, d0, order="inplace")
    diff = float(np.max(np.abs(d - np.abs(c["out"]))))
    print(f"{name}: Jacobi against in-place order {diff:.2e}")
    assert diff <= 1e-12


@pytest.mark.parametrize("name", ["sphere3", "circle2", "valence3"])
def test_band_is_the_clamped_full_result(oracle, name):
    full, banded = R.case(oracle, name), R.case(oracle, name, band_layers=3)
    B = banded["band"]
    d = np.abs(full["out"])
    want = np.where(full["phi"] >= 0.0, 1.0, -1.0) * np.where(d <= B, d, B)
    diff = float(np.max(np.abs(banded["out"] - want)))
    print(f"{name}: band {B:.4f} diff {diff:.2e} sweeps {banded['sweeps']} against {full['sweeps']}")
    assert diff <= 1e-12
    assert banded["sweeps"] <= full["sweeps"]


def test_update_closed_form_against_a_plane_wave():
    """d = n . x on a regular tetrahedron's face: U at the fourth vertex is n . x_t when the ray enters through the face."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        X = rng.normal(size=(4, 3))
        n = (X[1] + X[2] + X[3]) / 3.0 - X[0]
        n = -n / np.linalg.norm(n)                          # from the face's centroid towards vertex 0
        dv = (X[1:] @ n)[None, :] + 5.0
        U = R.update((X[1:] - X[0])[None, :, :], dv, np.ones((1, 3), dtype=bool))
        assert abs(U[0] - (X[0] @ n + 5.0)) <= 1e-12


def test_defaults_without_a_gpu():
    from cutfemx_amd import _lib, distance
    o = distance.reinit_default_options()
    assert (o.tol, o.inf_value, o.max_distance, o.max_iter, o.check_every) == (1e-10, 1e30, 0.0, 1000, 8)
    assert C.sizeof(_lib.ReinitOptions) == 32 and C.sizeof(_lib.ReinitInfoStruct) == 24
    assert _lib.load().cfx_reinit_options_default(None) == _lib.ERR_INVALID_ARGUMENT
    import inspect
    sig = inspect.signature(distance.reinitialize)
    assert list(sig.parameters)[:3] == ["phi", "max_iter", "tol"]          # python/cutfemx/distance.py:154-160
    assert sig.parameters["max_iter"].default == 1000 and sig.parameters["tol"].default == 1e-10
