"""The numpy model of the normal extension (tests/extension_ref.py) pinned to mathematics, without a GPU: exact planes,
the invariants of the transport, and the empty grey zone of every case the GPU tests compare against.  Also the
argument errors of cutfemx_amd.distance.extend_normal_velocity that are raised before the engine is called."""
import types

import numpy as np
import pytest

import extension_ref as X
import reinit_ref as R

CLEAN = 1e-13      # a vertex is clean when its model distance is the plane's within this
PLANE_TOL = 1e-13  # three digits over the errors observed (1.6e-15), inside the closed-form update's conditioning table
CLEAN_SHARE = {"plane2": 0.45, "plane3": 0.60}


@pytest.mark.parametrize("name", ["plane2", "plane3"])
def test_exact_planes(oracle, name):
    """phi = 1.7 (a.x - c), w = g.x + w0: on every vertex whose distance is exact, F is w at the foot of the
    perpendicular and n is a.  The other vertices have a characteristic that meets the clipped interface at the box:
    their errors are real (up to 0.3) and they are left out, but they may not be more than the cap allows."""
    c = X.case(oracle, name)
    dist, Fx, a = X.plane_exact(name, c["mesh"].x)
    clean = np.abs(c["d"] - dist) <= CLEAN
    share = float(clean.mean())
    eF, en = float(np.abs(c["F"] - Fx)[clean].max()), float(np.abs(c["n"] - a)[clean].max())
    print(f"{name}: clean share {share:.3f}, |F - w(foot)| <= {eF:.1e}, |n - a| <= {en:.1e}, sweeps {c['sweeps']} / {c['transport_sweeps']}")
    assert share >= CLEAN_SHARE[name]
    assert eF <= PLANE_TOL and en <= PLANE_TOL
    assert c["orphans"] == 0


@pytest.mark.parametrize("name", ["plane2", "sphere3", "scrambled3"])
def test_transport_orders_give_the_same_bits(oracle, name):
    c = X.case(oracle, name)
    F, n, _ = X.transport(c["plan"], order="inplace")
    assert F.tobytes() == c["F"].tobytes() and n.tobytes() == c["n"].tobytes()
    F, n, _ = X.transport(c["plan"], order="inplace", chunk=13)
    assert F.tobytes() == c["F"].tobytes() and n.tobytes() == c["n"].tobytes()


@pytest.mark.parametrize("name", X.GPU_CASES)
@pytest.mark.parametrize("layers", [None, 2])
def test_bounds_and_grey_zone(oracle, name, layers):
    """F stays between the least and the largest near value (convex combinations), normals are unit vectors or 0, and no
    candidate lies in the grey zone: the case has one answer whatever the last ulps of an implementation are"""
    c = X.case(oracle, name, layers)
    near = (c["kind"] == X.NEAR) | (c["kind"] == X.ZERO)
    reached = c["kind"] != X.NONE
    lo, hi = c["F"][near].min(), c["F"][near].max()
    print(f"{name} band {layers}: kinds {np.bincount(c['kind'], minlength=4)}, grey {c['grey']}, dropped {c['dropped']}, "
          f"orphans {c['orphans']}, sweeps {c['sweeps']} / {c['transport_sweeps']}")
    assert np.all(c["F"][reached] >= lo - 1e-14) and np.all(c["F"][reached] <= hi + 1e-14)
    assert np.all(c["F"][~reached] == 0.0) and np.all(c["n"][~reached] == 0.0)
    length = np.linalg.norm(c["n"][reached], axis=1)
    assert np.all((np.abs(length - 1.0) <= 4e-16) | (length == 0.0))
    assert c["grey"] == 0
    assert c["transport_sweeps"] <= c["sweeps"] + 1


@pytest.mark.parametrize("name", ["circle2", "scrambled3"])
def test_constant_speed_stays_constant(oracle, name):
    om, phi, _, _ = X.build_case(oracle, name)
    out = X.extend(om.x, om.conn, phi, np.full(phi.size, 0.3))
    reached = out["kind"] != X.NONE
    assert np.max(np.abs(out["F"][reached] - 0.3)) <= 4 * np.spacing(0.3)


def test_band_agrees_with_the_unbanded_payload(oracle):
    """on the vertices with unbanded d <= B the banded payload is the unbanded one (bit for bit on these cases: the GPU
    test asserts the same)"""
    for name in ("circle2", "sphere3", "asym3"):
        full, banded = X.case(oracle, name), X.case(oracle, name, 2)
        inside = full["d"] <= banded["band"]
        assert np.array_equal(banded["d"][inside], full["d"][inside])
        assert banded["F"][inside].tobytes() == full["F"][inside].tobytes(), name
        assert banded["n"][inside].tobytes() == full["n"][inside].tobytes(), name
        assert np.all(banded["F"][~inside] == 0.0)


def test_no_interface(oracle):
    om, phi = R.build_case(oracle, "positive3")
    assert X.extend(om.x, om.conn, phi, np.ones(phi.size))["reason"] == R.NO_INTERFACE


# ---- argument errors raised before the engine is called ------------------------------------------------------------------
def _stub(degree=1, bs=1, nv=5):
    V = types.SimpleNamespace(degree=degree, bs=bs, ndofs=nv, mesh=types.SimpleNamespace(gdim=2, tdim=2), _h=None)
    return types.SimpleNamespace(function_space=V, values=np.zeros(nv * bs))


def test_argument_errors_without_a_gpu():
    from cutfemx_amd import distance
    with pytest.raises(ValueError, match="degree 1"):
        distance.extend_normal_velocity(_stub(degree=2), np.zeros(5))
    with pytest.raises(ValueError, match="scalar"):
        distance.extend_normal_velocity(_stub(bs=3), np.zeros(15))
    with pytest.raises(ValueError, match="interface_speed must hold 5"):
        distance.extend_normal_velocity(_stub(), np.zeros(4))
    short = _stub()
    short.values = np.zeros(3)
    with pytest.raises(ValueError, match="phi.values must hold 5"):
        distance.extend_normal_velocity(short, np.zeros(5))
    with pytest.raises(TypeError, match="info_out is a device buffer"):
        distance.extend_normal_velocity(_stub(), np.zeros(5), info_out=np.zeros(5))


def test_option_defaults_without_a_gpu():
    import ctypes as C
    from cutfemx_amd import _lib
    o, r = _lib.ExtendOptions(), _lib.ReinitOptions()
    _lib.check(_lib.load().cfx_extend_options_default(C.byref(o)))
    _lib.check(_lib.load().cfx_reinit_options_default(C.byref(r)))
    assert (o.tol, o.inf_value, o.max_distance, o.max_iter, o.check_every) == (r.tol, r.inf_value, r.max_distance, r.max_iter, r.check_every)
    assert o.normal_sign == 1.0
    assert C.sizeof(_lib.ExtendInfoStruct) == 40 and C.sizeof(_lib.ExtendOptions) == 40
