"""cutfemx_amd.distance.reinitialize against the numpy model of its contract (tests/reinit_ref.py) on the same arrays.
The tolerance is 1e-10 absolute on unit-size meshes: the reference's own convergence threshold `tol`, below which it
regards two states as the same (axis planes: 1e-12, the tolerance of the reference's plane test)."""
import numpy as np
import pytest

import reinit_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = ["circle2", "sphere3", "scrambled3", "valence2", "valence3", "valence3big", "twospheres3", "corner3", "corner2"]

_SPACES: dict = {}


def _space(om):
    """The engine's mesh and P1 space of an oracle mesh, made once per mesh object."""
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


@pytest.mark.parametrize("name", CASES)
def test_against_the_model(oracle, name):
    import cutfemx_amd as cfx
    c = R.case(oracle, name)
    out, info = _run(c["mesh"], c["phi"])
    err = float(np.max(np.abs(out - c["out"])))
    print(f"{name}: err {err:.2e} sweeps {info.sweeps} (model {c['sweeps']}) seeds {info.seeds} updates {info.updates}")
    assert info.reason == cfx.distance.REINIT_CONVERGED and info.converged
    assert err <= TOL
    assert np.array_equal(out >= 0.0, c["phi"] >= 0.0)
    d0 = R.nearfield(c["mesh"].x, c["mesh"].conn, c["phi"])
    assert info.seeds == int(np.count_nonzero(d0 < R.INF))
    assert 0 < info.sweeps and info.updates >= info.seeds
    # changed vertices find their neighbours in the space's stencil lists; a space without them (an apex with more than
    # 62 neighbours) walks the cells around the vertex instead
    has_lists = _space(c["mesh"]).static_table_bytes()["row_stencil"] > 0
    assert has_lists == (name != "valence3big")
    if name in ("circle2", "sphere3"):                     # the reference's sphere property, on the engine's result
        exact = R.exact_sphere(c["mesh"].x, c["mesh"].tdim)
        assert np.max(np.abs(out - c["phi"])) > 1e-3
        assert np.max(np.abs(out - exact)) < 0.5 * np.max(np.abs(c["phi"] - exact))


@pytest.mark.parametrize("tdim,n", [(2, 8), (3, 4), (3, 8)])
@pytest.mark.parametrize("c", [57, 50])
def test_axis_planes(oracle, tdim, n, c):
    for k in range(tdim):
        for sgn, s in (("p", 1.0), ("m", -1.0)):
            om, phi = R.build_case(oracle, f"plane-{tdim}-{n}-{k}-{c}-{sgn}")
            out, info = _run(om, phi)
            exact = s * (om.x[:, k] - c / 100.0)
            err = float(np.max(np.abs(out - exact)))
            print(f"plane tdim {tdim} n {n} axis {k} c {c} sign {sgn}: err {err:.2e} sweeps {info.sweeps}")
            assert info.converged and err <= 1e-12
            on = phi == 0.0
            assert np.all(out[on] == 0.0) and not np.any(np.signbit(out[on]))


def test_no_interface_leaves_phi_untouched(oracle):
    import cutfemx_amd as cfx
    c = R.case(oracle, "positive3")
    out, info = _run(c["mesh"], c["phi"])
    assert info.reason == cfx.distance.REINIT_NO_INTERFACE and c["reason"] == R.NO_INTERFACE
    assert (info.sweeps, info.seeds, info.updates) == (0, 0, 0)
    assert out.tobytes() == np.asarray(c["phi"], dtype=np.float64).tobytes()


@pytest.mark.parametrize("name", ["circle2", "sphere3", "valence3"])
def test_band(oracle, name):
    full, banded = R.case(oracle, name), R.case(oracle, name, band_layers=3)
    B = banded["band"]
    out_full, info_full = _run(full["mesh"], full["phi"])
    out, info = _run(full["mesh"], full["phi"], max_distance=B)
    want = np.where(np.abs(out_full) <= B, out_full, np.where(full["phi"] >= 0.0, 1.0, -1.0) * B)
    err, err_model = float(np.max(np.abs(out - want))), float(np.max(np.abs(out - banded["out"])))
    print(f"{name}: band {B:.4f} err {err:.2e} against the model {err_model:.2e} sweeps {info.sweeps} < {info_full.sweeps}")
    assert info.converged and err <= TOL and err_model <= TOL
    assert np.max(np.abs(out)) <= B
    assert info.sweeps < info_full.sweeps and info.updates < info_full.updates


def test_max_iter_gives_an_upper_bound(oracle):
    import cutfemx_amd as cfx
    c = R.case(oracle, "sphere3")
    out, info = _run(c["mesh"], c["phi"], max_iter=2)
    assert info.reason == cfx.distance.REINIT_MAX_ITER and info.sweeps == 2
    assert np.all(np.abs(out) >= np.abs(c["out"]) - TOL)
    assert np.array_equal(out >= 0.0, c["phi"] >= 0.0)
    assert np.any(np.abs(out) > np.abs(c["out"]) + 1e-6)   # and it has not converged yet


def test_reproducible_and_independent_of_the_host_cadence(oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    c = R.case(oracle, "scrambled3")
    om, phi = c["mesh"], c["phi"]
    a, ia = _run(om, phi)
    b, ib = _run(om, phi)
    assert a.tobytes() == b.tobytes() and ia == ib
    for every in (1, 8, 0):
        g, ig = _run(om, phi, max_iter=64, check_every=every)
        assert g.tobytes() == a.tobytes(), every
        assert (ig.reason, ig.sweeps, ig.seeds, ig.updates) == (ia.reason, ia.sweeps, ia.seeds, ia.updates), every
    # device values, device info, no look: no host round trip
    V = _space(om)
    t = torch.tensor(phi, dtype=torch.float64, device="cuda")
    fn = cfx.Function(V, values=t)
    buf = cfx.distance.reinit_info_buffer()
    torch.cuda.synchronize()
    before = _lib.sync_count()
    ret = cfx.distance.reinitialize(fn, max_iter=64, check_every=0, info_out=buf)
    assert _lib.sync_count() == before
    assert ret is buf and fn.values is t
    assert cfx.distance.read_reinit_info(buf) == ia
    assert t.cpu().numpy().tobytes() == a.tobytes()


@pytest.mark.parametrize("name", ["sphere3", "circle2"])
def test_moving_domain_use(oracle, name):
    """cut, reinitialise the level set in place, update the cut: signs and zeros are kept, so the classification is."""
    import cutfemx_amd as cfx
    c = R.case(oracle, name)
    fn = cfx.Function(_space(c["mesh"]), values=np.array(c["phi"], dtype=np.float64), name="phi")
    cut = cfx.cut(fn)
    dom0, itf0 = cut.domain(), cfx.locate_entities(cut, "phi=0")
    info = cfx.distance.reinitialize(fn)
    assert info.converged and np.max(np.abs(fn.values - c["phi"])) > 1e-3
    cut.update()
    assert np.array_equal(cut.domain(), dom0)
    assert np.array_equal(cfx.locate_entities(cut, "phi=0"), itf0)
    assert itf0.size > 0


def test_argument_errors(oracle):
    import cutfemx_amd as cfx
    om = R.case(oracle, "positive3")["mesh"]
    mesh = _space(om).mesh
    V2 = cfx.FunctionSpace(mesh, 2)
    with pytest.raises(ValueError, match="degree 1"):
        cfx.distance.reinitialize(cfx.Function(V2))
    V3 = cfx.FunctionSpace(mesh, 1, bs=3)
    with pytest.raises(ValueError, match="scalar"):
        cfx.distance.reinitialize(cfx.Function(V3))
    own = cfx.FunctionSpace(mesh, 1, dofmap=om.conn.copy(), ndofs=om.x.shape[0])
    with pytest.raises(ValueError, match="geometry dofmap"):
        cfx.distance.reinitialize(cfx.Function(own))
    with pytest.raises(ValueError, match="max_iter"):
        cfx.distance.reinitialize(cfx.Function(_space(om), values=np.ones(om.x.shape[0])), max_iter=-1)
