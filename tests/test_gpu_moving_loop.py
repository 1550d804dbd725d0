"""The moving-domain loop on device tensors: advect -> reinitialize(band) -> cut.update, five steps, on a plane in a constant
velocity, where every stage has a closed form.

The plane is x_k = c, aligned with the mesh, and the velocity is not.  phi = x_k - c is a distance and stays one under a
translation; advect reproduces an affine phi (up to rounding) wherever the cell of the departure point lies inside the band
of the step before -- every vertex within 2 h of the new contour, as the contour moves 0.35 h per step; the reinitialisation
then rebuilds the band from the cut cells alone, and on a mesh-aligned plane its update along the mesh edge is d + h, with
no error of the method.  What is left is rounding: the tolerance is 1e-12 absolute on values below 0.5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 5
TOL = 1e-12


@pytest.mark.parametrize("tdim,n,k,velocity", [(3, 8, 0, (0.31, 0.11, -0.17)), (2, 16, 1, (-0.23, 0.155))])
def test_plane_moves_with_the_velocity(oracle, tdim, n, k, velocity):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib
    om = oracle.mesh_box(tdim, n)
    h = 1.0 / n
    band = 4 * h
    u = np.array(velocity)
    dt = 0.35 * h / abs(u[k])
    c = [0.3303 + j * dt * u[k] for j in range(STEPS + 1)]
    exact = [om.x[:, k] - cj for cj in c]
    assert min(float(np.min(np.abs(e))) for e in exact) > 1e-6          # no vertex value near zero, at any step

    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    nv = om.x.shape[0]
    phi = cfx.Function(V, values=torch.tensor(np.clip(exact[0], -band, band), dtype=torch.float64, device="cuda"), name="phi")
    vel = torch.tensor(np.tile(u, (nv, 1)).ravel(), dtype=torch.float64, device="cuda")
    cut = cfx.cut(phi)
    ainfo, rinfo = cfx.distance.advect_info_buffer(), cfx.distance.reinit_info_buffer()
    for j in range(1, STEPS + 1):
        torch.cuda.synchronize()
        before = _lib.sync_count()
        cfx.distance.advect(phi, vel, dt, info_out=ainfo)
        cfx.distance.reinitialize(phi, max_iter=16, max_distance=band, check_every=0, info_out=rinfo)
        if j > 1:                                                        # (the first step builds the mesh's static tables)
            assert _lib.sync_count() == before
        cut.update()
        got = phi.values.cpu().numpy()
        inside = np.abs(exact[j]) <= band
        err = float(np.max(np.abs(got - exact[j])[inside]))
        a, r = cfx.distance.read_advect_info(ainfo), cfx.distance.read_reinit_info(rinfo)
        print(f"{tdim}-D step {j}: |phi - distance| in the band {err:.1e} on {int(inside.sum())} vertices; {a}; reinit sweeps {r.sweeps}")
        assert err <= TOL
        assert np.all(np.abs(got[~inside]) == band) and np.array_equal(got > 0, exact[j] > 0)
        assert r.converged and a.capped == 0 and a.skipped == 0 and a.located + a.outside == nv and a.outside > 0
        want = cfx.cut(cfx.Function(V, values=exact[j].copy(), name="phi"))
        for part in ("phi<0", "phi=0"):
            cells = cfx.locate_entities(cut, part)
            assert cells.size > 0 and np.array_equal(cells, cfx.locate_entities(want, part))
