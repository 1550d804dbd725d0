"""cutfemx_amd.distance.advect against the closed forms of affine fields, against a brute-force locator that knows nothing
of the walk, against the numpy model of the contract (tests/advect_ref.py: its counts and its walks), and against the
properties the contract promises: fixed dofs, bands, the same bits from every way of calling and from scaled inputs,
capped walks and non-finite velocities that leave the other vertices alone.

Cases: the four meshes of tests/test_advect_reference.py (a 3-D Kuhn box, the same scrambled, a 2-D box, a double cone with
two apexes of 128 cells joined with a box), at CFL 0.3, 2.5 and 12 (the cone: 0.3 and 2.5), on which that module shows the
model alone to have no capped vertex and an empty grey zone.  'Equal' where it is not bit for bit: advect_ref.TOL,
16 x the model's float64-against-long-double floor, relative to max|phi|."""
import ctypes as C
import types

import numpy as np
import pytest

import advect_ref as A

pytestmark = pytest.mark.gpu

RUNS = [(name, cfl) for name, cfls in A.CASES.items() for cfl in cfls]
_SPACES: dict = {}
_BRUTE: dict = {}


def _space(om):
    import cutfemx_amd as cfx
    if id(om) not in _SPACES:
        mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
        _SPACES[id(om)] = (om, cfx.FunctionSpace(mesh, 1))
    return _SPACES[id(om)][1]


def _run(om, phi, vel, dt, device=False, **kw):
    """(out [nv], cells [nv], info) as numpy arrays / AdvectInfo"""
    import cutfemx_amd as cfx
    nv = om.x.shape[0]
    if device:
        import torch
        p = torch.tensor(np.asarray(phi, dtype=np.float64), device="cuda")
        w = torch.tensor(np.ascontiguousarray(vel, dtype=np.float64).ravel(), device="cuda")
        cells = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    else:
        p, w, cells = np.array(phi, dtype=np.float64), np.ascontiguousarray(vel, dtype=np.float64).ravel(), np.full(nv, -7, dtype=np.int32)
    fn = cfx.Function(_space(om), values=p)
    info = cfx.distance.advect(fn, w, dt, cells_out=cells, **kw)
    assert fn.values is p
    host = lambda a: a.cpu().numpy() if device else a
    return host(p), host(cells), info


def _brute(oracle, name, cfl, order, which):
    key = (name, cfl, order, which)
    if key not in _BRUTE:
        om = A.mesh(oracle, name)[0]
        _BRUTE[key] = A.brute_locate(om.x, om.conn, A.model(oracle, name, "sphere", cfl, order)[which])
    return _BRUTE[key]


def _counts(info):
    return (info.located, info.outside, info.capped, info.skipped, info.steps, info.max_walk)


def _model_counts(m):
    return tuple(m[k] for k in ("located", "outside", "capped", "skipped", "steps", "max_walk"))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name,cfl", RUNS)
def test_affine_fields_are_exact_at_every_vertex(oracle, name, cfl, order):
    """phi and velocity affine: the P1 extension reproduces both, so the closed form holds whether the departure point is
    inside, outside or far beyond the mesh"""
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "affine")
    dt = A.time_step(oracle, name, "affine", cfl)
    out, cells, info = _run(om, phi, vel, dt, order=order)
    m = A.model(oracle, name, "affine", cfl, order)
    scale = float(np.max(np.abs(phi)))
    err = float(np.max(np.abs(out - A.affine_exact(om.x, om.tdim, dt, order)))) / scale
    print(f"{name} CFL {cfl} order {order}: |out - closed form| / max|phi| = {err:.1e} (allowed {A.TOL:.1e}); {info}; "
          f"same bits as the float64 model: {out.tobytes() == m['out'].tobytes()}")
    assert err <= A.TOL
    assert _counts(info) == _model_counts(m) and info.capped == 0
    assert np.array_equal(cells, m["cells"])


@pytest.mark.parametrize("name,cfl", RUNS)
def test_against_the_brute_force_locator(oracle, name, cfl):
    """the quadratic sphere in a rotation, order 1: the departure points are x - dt v, and the locator is a maximum over
    all cells"""
    om, nbr, _ = A.mesh(oracle, name)
    phi, vel = A.fields(oracle, name, "sphere")
    dt = A.time_step(oracle, name, "sphere", cfl)
    out, cells, info = _run(om, phi, vel, dt, order=1)
    m = A.model(oracle, name, "sphere", cfl, 1)
    cell_b, best, lam_b = _brute(oracle, name, cfl, 1, "dep")
    inside = best >= -A.INSIDE_TOL
    scale = float(np.max(np.abs(phi)))
    ld = np.longdouble
    assert np.all(cells >= 0)
    lam = A.barycentric(om.x[om.conn[cells]][:, :, :om.tdim].astype(ld), m["dep"].astype(ld))
    here = np.einsum("mi,mi->m", lam, phi[om.conn[cells]].astype(ld))
    # inside: the value of the brute-force cell, and the engine's own cell holds the point
    value = np.einsum("mi,mi->m", lam_b, phi[om.conn[cell_b]].astype(ld))
    e_in = float(np.max(np.abs(out[inside] - value[inside]))) / scale
    assert float(lam[inside].min()) >= -(A.INSIDE_TOL + 1e-15)
    # outside: a cell with a boundary facet, its P1 extension at the departure point
    outside = ~inside
    assert np.all(np.any(nbr[cells[outside]] < 0, axis=1))
    e_out = float(np.max(np.abs(out[outside] - here[outside]))) / scale if outside.any() else 0.0
    print(f"{name} CFL {cfl}: {int(inside.sum())} inside |out - brute force| {e_in:.1e}, {int(outside.sum())} outside |out - extension| {e_out:.1e} "
          f"(allowed {A.TOL:.1e}); {info}")
    assert e_in <= A.TOL and e_out <= A.TOL
    assert (info.located, info.outside) == (int(inside.sum()), int(outside.sum()))
    assert _counts(info) == _model_counts(m) and info.capped == 0 and info.skipped == 0


@pytest.mark.parametrize("name,cfl", RUNS)
def test_order_two_against_the_brute_force_locator(oracle, name, cfl):
    """... order 2 on the vertices whose half point and departure point both lie inside the mesh"""
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "sphere")
    out, cells, info = _run(om, phi, vel, A.time_step(oracle, name, "sphere", cfl), order=2)
    m = A.model(oracle, name, "sphere", cfl, 2)
    cell_b, best, lam_b = _brute(oracle, name, cfl, 2, "dep")
    _, best_half, _ = _brute(oracle, name, cfl, 2, "half")
    both = (best >= -A.INSIDE_TOL) & (best_half >= -A.INSIDE_TOL)
    assert both.sum() >= 20
    value = np.einsum("mi,mi->m", lam_b, phi[om.conn[cell_b]].astype(np.longdouble))
    err = float(np.max(np.abs(out[both] - value[both]))) / float(np.max(np.abs(phi)))
    print(f"{name} CFL {cfl}: {int(both.sum())} vertices, |out - brute force| / max|phi| = {err:.1e} (allowed {A.TOL:.1e}); {info}")
    assert err <= A.TOL
    assert _counts(info) == _model_counts(m) and info.capped == 0


@pytest.mark.parametrize("name", list(A.CASES))
def test_fixed_dofs(oracle, name):
    """CFL 0: zero velocity gives phi back bit for bit, on the whole mesh and on a subset of the vertices"""
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "sphere")
    nv = phi.size
    dt = A.time_step(oracle, name, "sphere", 2.5)
    for order in (1, 2):
        out, cells, info = _run(om, phi, np.zeros_like(vel), dt, order=order)
        assert out.tobytes() == phi.tobytes()
        assert _counts(info) == (nv, 0, 0, 0, 0, 0)
        assert np.array_equal(cells, A.first_cells(om.conn, nv))
        full, _, _ = _run(om, phi, vel, dt, order=order)
        held = np.arange(nv) % 3 == 0
        part = vel.copy()
        part[held] = 0.0
        out, _, info = _run(om, phi, part, dt, order=order)
        assert out[held].tobytes() == phi[held].tobytes()
        if order == 1:                                   # (order 2 reads the neighbours' velocities, which changed)
            assert out[~held].tobytes() == full[~held].tobytes()
        assert info.located >= int(held.sum()) and info.capped == 0


@pytest.mark.parametrize("name", ["box3", "box2", "valence3"])
def test_band(oracle, name):
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "sphere")
    dt = A.time_step(oracle, name, "sphere", 2.5)
    B = 0.6 * float(np.max(np.abs(phi)))
    beyond = np.abs(phi) > B
    assert beyond.any() and (~beyond).any()
    full, cells_full, _ = _run(om, phi, vel, dt)
    out, cells, info = _run(om, phi, vel, dt, max_distance=B)
    assert out[beyond].tobytes() == phi[beyond].tobytes() and np.all(cells[beyond] == -1)
    assert out[~beyond].tobytes() == full[~beyond].tobytes() and np.array_equal(cells[~beyond], cells_full[~beyond])
    assert info.skipped == int(beyond.sum())
    assert _counts(info) == _model_counts(A.model(oracle, name, "sphere", 2.5, 2, band=B))


def _raw(V, phi, vel, out, cells, dt, info=None, **fields):
    """the C entry point on pointers as they stand"""
    from cutfemx_amd import _lib
    o = _lib.AdvectOptions()
    _lib.check(_lib.load().cfx_advect_options_default(C.byref(o)))
    o.dt = dt
    for k, v in fields.items():
        setattr(o, k, v)
    st = _lib.AdvectInfoStruct()
    _lib.check(_lib.lib().cfx_advect_level_set(V._h, phi, vel, out, cells, C.byref(o), C.byref(st) if info is None else info))
    return st


def test_defaults():
    from cutfemx_amd import _lib
    o = _lib.AdvectOptions()
    _lib.check(_lib.load().cfx_advect_options_default(C.byref(o)))
    assert (o.dt, o.max_distance, o.inside_tol, o.order, o.max_steps) == (0.0, 0.0, 1e-12, 2, 4096)


def test_every_way_of_calling_gives_the_same_bits(oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    name, cfl = "scrambled3", 2.5
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "sphere")
    dt = A.time_step(oracle, name, "sphere", cfl)
    nv = phi.size
    V = _space(om)
    out, cells, info = _run(om, phi, vel, dt)
    again = _run(om, phi, vel, dt)
    assert again[0].tobytes() == out.tobytes() and np.array_equal(again[1], cells) and again[2] == info
    dev = _run(om, phi, vel, dt, device=True)
    assert dev[0].tobytes() == out.tobytes() and np.array_equal(dev[1], cells) and dev[2] == info
    # the velocity as a Function on the vector space, as extend_normal_velocity returns it
    W = cfx.FunctionSpace(V.mesh, 1, bs=om.tdim)
    fn = cfx.Function(V, values=phi.copy())
    assert cfx.distance.advect(fn, cfx.Function(W, values=vel.ravel().copy()), dt) == info and fn.values.tobytes() == out.tobytes()
    # raw device buffers; out into a second array (phi untouched) and in place; no cells
    bp, bv, bo = _lib.DeviceBuffer(nv, np.float64), _lib.DeviceBuffer(nv * om.tdim, np.float64), _lib.DeviceBuffer(nv, np.float64)
    bp.fill_from(phi), bv.fill_from(vel.ravel()), bo.fill_from(np.full(nv, 7.0))
    ptr = lambda b: C.c_void_p(b.ptr)
    st = _raw(V, ptr(bp), ptr(bv), ptr(bo), None, dt)
    assert bo.numpy().tobytes() == out.tobytes() and bp.numpy().tobytes() == phi.tobytes()
    assert cfx.distance._advect_info(st) == info
    _raw(V, ptr(bp), ptr(bv), ptr(bp), None, dt)
    assert bp.numpy().tobytes() == out.tobytes()
    # host arrays, out into a second array
    hp, hv, ho = phi.copy(), np.ascontiguousarray(vel.ravel()), np.full(nv, 7.0)
    np_ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _raw(V, np_ptr(hp), np_ptr(hv), np_ptr(ho), None, dt)
    assert ho.tobytes() == out.tobytes() and hp.tobytes() == phi.tobytes()
    # device tensors and a device info: no host round trip
    tp = torch.tensor(phi, dtype=torch.float64, device="cuda")
    tv = torch.tensor(vel.ravel(), dtype=torch.float64, device="cuda")
    buf = cfx.distance.advect_info_buffer()
    torch.cuda.synchronize()
    before = _lib.sync_count()
    assert cfx.distance.advect(cfx.Function(V, values=tp), tv, dt, info_out=buf) is buf
    assert _lib.sync_count() == before
    assert tp.cpu().numpy().tobytes() == out.tobytes() and cfx.distance.read_advect_info(buf) == info


@pytest.mark.parametrize("name,cfl", [("scrambled3", 2.5), ("box2", 12.0)])
def test_scaling(oracle, name, cfl):
    """coordinates, phi and dt x velocity times 2^20 and 2^-20: the scaled bits, the same cells and counts (every operation is
    homogeneous; inside_tol compares ratios)"""
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "sphere")
    dt = A.time_step(oracle, name, "sphere", cfl)
    out, cells, info = _run(om, phi, vel, dt)
    for s in (2.0 ** 20, 2.0 ** -20):
        scaled = types.SimpleNamespace(tdim=om.tdim, x=om.x * s, conn=om.conn)
        outs, cellss, infos = _run(scaled, phi * s, vel * s, dt)
        assert outs.tobytes() == (out * s).tobytes(), s
        assert np.array_equal(cellss, cells) and infos == info


def test_cap_and_non_finite_velocity(oracle):
    om = A.mesh(oracle, "box3")[0]
    phi, vel = A.fields(oracle, "box3", "sphere")
    dt = A.time_step(oracle, "box3", "sphere", 12.0)
    full, cells_full, info_full = _run(om, phi, vel, dt, order=1)
    out, cells, info = _run(om, phi, vel, dt, order=1, max_steps=2)
    m = A.model(oracle, "box3", "sphere", 12.0, 1, max_steps=2)
    assert info.capped > 0 and _counts(info) == _model_counts(m)
    capped = m["status"] == A.CAPPED
    assert out[capped].tobytes() == phi[capped].tobytes() and np.all(cells[capped] == -1)
    assert out[~capped].tobytes() == full[~capped].tobytes() and np.array_equal(cells[~capped], cells_full[~capped])
    assert info.max_walk == 2
    # one NaN velocity, order 1: that vertex alone is capped
    bad = vel.copy()
    v = phi.size // 2
    bad[v, 1] = np.nan
    out, cells, info = _run(om, phi, bad, dt, order=1)
    others = np.arange(phi.size) != v
    assert info.capped == 1 and out[v] == phi[v] and cells[v] == -1
    assert out[others].tobytes() == full[others].tobytes()
    assert (info.located + info.outside, info.skipped) == (phi.size - 1, 0)
    # order 2 reads the NaN wherever a half point lies in a cell of that vertex: the call returns, the vertices whose
    # midpoint velocity is a NaN are capped and unchanged, the rest is as without it
    full2, _, _ = _run(om, phi, vel, dt, order=2)
    out, cells, info = _run(om, phi, bad, dt, order=2)
    hit = cells == -1
    assert 1 <= info.capped == int(hit.sum()) < 200 and hit[v]
    assert out[hit].tobytes() == phi[hit].tobytes() and np.all(np.isfinite(out))
    assert out[~hit].tobytes() == full2[~hit].tobytes()
    # an infinite one
    bad[v, 1] = np.inf
    assert _run(om, phi, bad, dt, order=1)[2].capped == 1


def test_argument_errors(oracle):
    import torch
    import cutfemx_amd as cfx
    om = A.mesh(oracle, "box2")[0]
    V = _space(om)
    nv = om.x.shape[0]
    phi, vel = np.ones(nv), np.zeros(2 * nv)
    with pytest.raises(ValueError, match="degree 1"):
        cfx.distance.advect(cfx.Function(cfx.FunctionSpace(V.mesh, 2)), vel, 0.1)
    with pytest.raises(ValueError, match="scalar"):
        cfx.distance.advect(cfx.Function(cfx.FunctionSpace(V.mesh, 1, bs=2)), vel, 0.1)
    with pytest.raises(ValueError, match="order is 1 or 2"):
        cfx.distance.advect(cfx.Function(V, values=phi.copy()), vel, 0.1, order=3)
    for dt in (np.nan, np.inf):
        with pytest.raises(ValueError, match="dt is finite"):
            cfx.distance.advect(cfx.Function(V, values=phi.copy()), vel, dt)
    with pytest.raises(ValueError, match="max_steps"):
        cfx.distance.advect(cfx.Function(V, values=phi.copy()), vel, 0.1, max_steps=0)
    with pytest.raises(TypeError, match="all be host or all be device"):
        cfx.distance.advect(cfx.Function(V, values=phi.copy()), torch.zeros(2 * nv, dtype=torch.float64, device="cuda"), 0.1)
    with pytest.raises(TypeError, match="all be host or all be device"):
        cfx.distance.advect(cfx.Function(V, values=torch.ones(nv, dtype=torch.float64, device="cuda")), vel, 0.1)
    with pytest.raises(ValueError, match="per vertex"):
        cfx.distance.advect(cfx.Function(V, values=phi.copy()), vel[:-1], 0.1)
    own = cfx.FunctionSpace(V.mesh, 1, dofmap=om.conn.copy(), ndofs=nv)
    with pytest.raises(ValueError, match="geometry dofmap"):
        cfx.distance.advect(cfx.Function(own, values=phi.copy()), vel, 0.1)
    with pytest.raises(TypeError, match="device buffer"):
        cfx.distance.advect(cfx.Function(V, values=phi.copy()), vel, 0.1, info_out=np.zeros(6))
