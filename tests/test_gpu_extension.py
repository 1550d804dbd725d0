"""cutfemx_amd.distance.extend_normal_velocity against the numpy model of its contract (tests/extension_ref.py) on the same
arrays, and against the properties the contract promises: the distance of `reinitialize` bit for bit, an untouched phi,
exact planes, the same bits from every way of calling, from scaled inputs and inside a band.

The engine returns F (speed) and F n (velocity), not n itself.  Where a test needs n it divides in long double on the
vertices with |F| >= 0.1 max|w|: velocity = F n rounded once per component, so v / F is n within 2^-53 relative."""
import ctypes as C

import numpy as np
import pytest

import extension_ref as X
import reinit_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-12                    # of the issue: F within TOL max|w| of the model, n within TOL
UNIT = 4e-16 + 2.0 ** -53      # | |n| - 1 | <= 4e-16 of the contract, seen through v / F (see above)
_SPACES: dict = {}


def _space(om):
    import cutfemx_amd as cfx
    if id(om) not in _SPACES:
        mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
        _SPACES[id(om)] = (om, cfx.FunctionSpace(mesh, 1))
    return _SPACES[id(om)][1]


def _run(om, phi, w, device=False, **kw):
    """(speed [nv], velocity [nv, dim], signed distance [nv], info, phi after the call) as numpy arrays"""
    import cutfemx_amd as cfx
    host = lambda a: a.cpu().numpy() if device else a
    if device:
        import torch
        phi_in, w_in = (torch.tensor(np.asarray(a, dtype=np.float64), device="cuda") for a in (phi, w))
    else:
        phi_in, w_in = np.array(phi, dtype=np.float64), np.array(w, dtype=np.float64)
    res = cfx.distance.extend_normal_velocity(cfx.Function(_space(om), values=phi_in), w_in, **kw)
    if device:
        assert all(a.values.is_cuda for a in (res.speed, res.velocity, res.signed_distance))
    else:
        assert all(isinstance(a.values, np.ndarray) for a in (res.speed, res.velocity, res.signed_distance))
    assert res.velocity.function_space.bs == om.tdim and res.speed.function_space is _space(om)
    return host(res.speed.values), host(res.velocity.values).reshape(-1, om.tdim), host(res.signed_distance.values), res.info, host(phi_in)


def _normals(F, v, wmax):
    """(rows with |F| >= 0.1 wmax, n = v / F there, in long double)"""
    rows = np.abs(F) >= 0.1 * wmax
    return rows, v[rows].astype(np.longdouble) / F[rows, None].astype(np.longdouble)


@pytest.mark.parametrize("layers", [None, 2])
@pytest.mark.parametrize("name", X.GPU_CASES)
def test_against_the_model(oracle, name, layers):
    import cutfemx_amd as cfx
    c = X.case(oracle, name, layers)
    om, phi, w, B = c["mesh"], c["phi"], c["w"], c["band"]
    F, v, sd, info, phi_after = _run(om, phi, w, max_distance=B)
    assert phi_after.tobytes() == np.asarray(phi, dtype=np.float64).tobytes()
    # the distance of reinitialize, bit for bit
    fn = cfx.Function(_space(om), values=np.array(phi, dtype=np.float64))
    rinfo = cfx.distance.reinitialize(fn, max_distance=B)
    assert sd.tobytes() == fn.values.tobytes()
    assert (info.reason, info.sweeps, info.seeds, info.updates) == (rinfo.reason, rinfo.sweeps, rinfo.seeds, rinfo.updates)
    assert info.reason == cfx.distance.REINIT_CONVERGED and c["grey"] == 0
    # near / transported as in the model
    assert info.transported == int(np.count_nonzero(c["kind"] == X.TRANSPORTED))
    assert info.transport_sweeps == c["transport_sweeps"]
    wmax = float(np.max(np.abs(w)))
    eF = float(np.max(np.abs(F - c["F"])))
    ev = float(np.max(np.abs(v - c["velocity"])))
    rows, n = _normals(F, v, wmax)
    en = float(np.max(np.abs(n - c["n"][rows]))) if rows.any() else 0.0
    length = np.sqrt(np.sum(n * n, axis=1))
    moving = length != 0.0
    unit = float(np.max(np.abs(length[moving] - 1.0))) if moving.any() else 0.0
    print(f"{name} band {layers}: |F - model| {eF:.1e} (max|w| {wmax:.2f}), |n - model| {en:.1e} on {int(rows.sum())} vertices, "
          f"|v - model| {ev:.1e}, | |n| - 1 | {unit:.1e}, transported {info.transported}, sweeps {info.sweeps} / {info.transport_sweeps}")
    assert eF <= TOL * wmax
    assert en <= TOL
    assert ev <= 2 * TOL * wmax                              # (F within TOL max|w| times |n| = 1, and |F| <= max|w| times TOL for n)
    assert unit <= UNIT
    none = c["kind"] == X.NONE
    assert np.all(F[none] == 0.0) and np.all(v[none] == 0.0)
    if layers is not None:
        assert np.max(np.abs(sd)) <= B


@pytest.mark.parametrize("name", ["plane2", "plane3"])
def test_exact_planes(oracle, name):
    """the assertion of tests/test_extension_reference.py on the engine's own result"""
    c = X.case(oracle, name)
    F, v, sd, info, _ = _run(c["mesh"], c["phi"], c["w"])
    dist, Fx, a = X.plane_exact(name, c["mesh"].x)
    clean = np.abs(np.abs(sd) - dist) <= 1e-13
    share = float(clean.mean())
    eF = float(np.max(np.abs(F - Fx)[clean]))
    rows, n = _normals(F, v, float(np.max(np.abs(c["w"]))))
    en = float(np.max(np.abs(n - a)[clean[rows]]))
    print(f"{name}: clean share {share:.3f}, |F - w(foot)| {eF:.1e}, |n - a| {en:.1e}")
    assert share >= {"plane2": 0.45, "plane3": 0.60}[name]
    assert eF <= 1e-13 and en <= 1e-13
    assert np.array_equal(sd >= 0.0, c["phi"] >= 0.0)


def test_reproducible_and_independent_of_the_way_of_calling(oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    c = X.case(oracle, "scrambled3")
    om, phi, w = c["mesh"], c["phi"], c["w"]
    a = _run(om, phi, w)
    same = lambda r: all(r[k].tobytes() == a[k].tobytes() for k in range(3))
    assert same(_run(om, phi, w)) and _run(om, phi, w)[3] == a[3]
    for every in (1, 8, 0):
        r = _run(om, phi, w, max_iter=64, check_every=every)
        assert same(r) and r[3] == a[3], every
    d = _run(om, phi, w, device=True)
    assert same(d) and d[3] == a[3]
    # device values, device info, no look: no host round trip
    V = _space(om)
    tp, tw = torch.tensor(phi, dtype=torch.float64, device="cuda"), torch.tensor(w, dtype=torch.float64, device="cuda")
    buf = cfx.distance.extend_info_buffer()
    fn = cfx.Function(V, values=tp)
    cfx.distance.extend_normal_velocity(fn, tw, max_iter=64, check_every=0, info_out=buf)      # (the vector space is made once)
    torch.cuda.synchronize()
    before = _lib.sync_count()
    res = cfx.distance.extend_normal_velocity(fn, tw, max_iter=64, check_every=0, info_out=buf)
    assert _lib.sync_count() == before
    assert res.info is buf and cfx.distance.read_extend_info(buf) == a[3]
    assert res.speed.values.cpu().numpy().tobytes() == a[0].tobytes()
    assert res.velocity.values.cpu().numpy().tobytes() == a[1].tobytes()
    assert tp.cpu().numpy().tobytes() == np.asarray(phi).tobytes()


@pytest.mark.parametrize("name", ["circle2", "scrambled3"])
def test_scaling(oracle, name):
    """coordinates and phi times 2^20 and 2^-20: the same F and velocity bits and the scaled distance (no threshold of the
    contract is absolute)"""
    import types
    c = X.case(oracle, name)
    om, phi, w = c["mesh"], c["phi"], c["w"]
    F, v, sd, info, _ = _run(om, phi, w)
    for s in (2.0 ** 20, 2.0 ** -20):
        scaled = types.SimpleNamespace(tdim=om.tdim, x=om.x * s, conn=om.conn)
        Fs, vs, sds, infos, _ = _run(scaled, phi * s, w)
        assert Fs.tobytes() == F.tobytes() and vs.tobytes() == v.tobytes(), s
        assert sds.tobytes() == (sd * s).tobytes(), s
        assert infos == info


@pytest.mark.parametrize("name", ["circle2", "sphere3", "asym3"])
def test_band(oracle, name):
    """inside the band the payload is the unbanded one -- bit for bit: the model agrees bitwise on these cases on the CPU
    (tests/test_extension_reference.py::test_band_agrees_with_the_unbanded_payload) -- and beyond it F = 0, velocity = 0"""
    full, banded = X.case(oracle, name), X.case(oracle, name, 2)
    B = banded["band"]
    F, v, sd, info, _ = _run(full["mesh"], full["phi"], full["w"])
    Fb, vb, sdb, infob, _ = _run(full["mesh"], full["phi"], full["w"], max_distance=B)
    inside = np.abs(sd) <= B
    assert inside.any() and (~inside).any()
    assert Fb[inside].tobytes() == F[inside].tobytes() and vb[inside].tobytes() == v[inside].tobytes()
    assert np.all(Fb[~inside] == 0.0) and np.all(vb[~inside] == 0.0)
    assert np.all(np.abs(sdb[~inside]) == B) and sdb[inside].tobytes() == sd[inside].tobytes()
    assert infob.sweeps < info.sweeps and infob.transported < info.transported


def _raw_call(om, phi, w, speed, velocity, dist, max_iter=1000):
    """the C entry point on numpy arrays as they stand (None: a NULL output)"""
    from cutfemx_amd import _lib
    o = _lib.ExtendOptions()
    _lib.check(_lib.load().cfx_extend_options_default(C.byref(o)))
    o.max_iter = max_iter
    st = _lib.ExtendInfoStruct()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.lib().cfx_extend_normal_velocity(_space(om)._h, ptr(phi), ptr(w), ptr(speed), ptr(velocity), ptr(dist), C.byref(o), C.byref(st)))
    return st


def test_no_interface_leaves_the_outputs_untouched(oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    om, phi = R.build_case(oracle, "positive3")
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    nv = phi.size
    w = np.ones(nv)
    outs = [np.full(nv, 7.0), np.full(3 * nv, 7.0), np.full(nv, 7.0)]
    st = _raw_call(om, phi, w, *outs)
    assert st.reason == cfx.distance.REINIT_NO_INTERFACE and (st.sweeps, st.seeds, st.updates, st.transport_sweeps, st.transported) == (0, 0, 0, 0, 0)
    assert all(np.all(a == 7.0) for a in outs)
    dev = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for n in (nv, 3 * nv, nv)]
    tp, tw = torch.tensor(phi, device="cuda"), torch.tensor(w, device="cuda")
    o = _lib.ExtendOptions()
    _lib.check(_lib.load().cfx_extend_options_default(C.byref(o)))
    st = _lib.ExtendInfoStruct()
    _lib.check(_lib.lib().cfx_extend_normal_velocity(_space(om)._h, C.c_void_p(tp.data_ptr()), C.c_void_p(tw.data_ptr()),
                                                     *(C.c_void_p(a.data_ptr()) for a in dev), C.byref(o), C.byref(st)))
    assert st.reason == cfx.distance.REINIT_NO_INTERFACE and all(bool(torch.all(a == 7.0)) for a in dev)
    res = cfx.distance.extend_normal_velocity(cfx.Function(_space(om), values=phi.copy()), w)
    assert res.info.reason_name == "no_interface" and not res.info.converged


def test_max_iter(oracle):
    import cutfemx_amd as cfx
    c = X.case(oracle, "sphere3")
    F, v, sd, info, _ = _run(c["mesh"], c["phi"], c["w"], max_iter=1)
    assert info.reason == cfx.distance.REINIT_MAX_ITER and info.sweeps == 1
    unreached = np.abs(sd) == R.INF
    assert unreached.any() and np.all(F[unreached] == 0.0) and np.all(v[unreached] == 0.0)
    near = (c["kind"] == X.NEAR) & (np.abs(sd) == c["d0"])     # a near vertex that the one sweep did not lower keeps its payload
    assert near.any() and np.max(np.abs(F[near] - c["F"][near])) <= TOL * np.max(np.abs(c["w"]))


def test_null_outputs_are_skipped(oracle):
    c = X.case(oracle, "circle2")
    om, phi, w = c["mesh"], np.ascontiguousarray(c["phi"], dtype=np.float64), np.ascontiguousarray(c["w"], dtype=np.float64)
    nv = phi.size
    speed, velocity, dist = np.zeros(nv), np.zeros(2 * nv), np.zeros(nv)
    st = _raw_call(om, phi, w, speed, velocity, dist)
    for keep in range(3):
        outs = [np.full(a.size, 7.0) if k == keep else None for k, a in enumerate((speed, velocity, dist))]
        st2 = _raw_call(om, phi, w, *outs)
        assert outs[keep].tobytes() == (speed, velocity, dist)[keep].tobytes()
        assert (st2.reason, st2.transported) == (st.reason, st.transported)
    st3 = _raw_call(om, phi, w, None, None, None)
    assert (st3.reason, st3.sweeps, st3.transport_sweeps) == (st.reason, st.sweeps, st.transport_sweeps)


def test_argument_errors(oracle):
    import cutfemx_amd as cfx
    om = R.case(oracle, "positive3")["mesh"]
    mesh = _space(om).mesh
    nv = om.x.shape[0]
    own = cfx.FunctionSpace(mesh, 1, dofmap=om.conn.copy(), ndofs=nv)
    with pytest.raises(ValueError, match="geometry dofmap"):
        cfx.distance.extend_normal_velocity(cfx.Function(own), np.ones(nv))
    with pytest.raises(ValueError, match="max_iter"):
        cfx.distance.extend_normal_velocity(cfx.Function(_space(om), values=np.ones(nv)), np.ones(nv), max_iter=-1)
    with pytest.raises(ValueError, match="degree 1"):
        cfx.distance.extend_normal_velocity(cfx.Function(cfx.FunctionSpace(mesh, 2)), np.ones(nv))
    with pytest.raises(TypeError, match="device buffer"):
        cfx.distance.extend_normal_velocity(cfx.Function(_space(om), values=np.ones(nv)), np.ones(nv), info_out=np.zeros(5))
