"""The SUPG level-set step in HBM (cutfemx_amd/supg.py: two registered integrands with the coefficient list
(phi, speed), assembled over every cell, Dirichlet treatment with the old phi, BiCGStab) against the numpy model of
tests/supg_ref.py (pinned by tests/test_supg_reference.py: nonsymmetric, nonsingular, exact on a plane).

A and b within 1e-12 of the model, relative to the largest entry (A compared as matrices: stored zeros may differ);
supg.advect within supg_ref.DIRECT_BAR -- ten times the distance of the BiCGStab restatement from the direct solve on
the model's systems -- of phi - dt F on the plane and of the direct solve of the engine's OWN matrix on the sphere.
Two calls agree bit for bit (every sum of the row assembly and of the solver has a fixed order); with fixed dofs the
right-hand side passes through fem.apply_lifting, which adds with atomics, and the calls agree to rounding."""
import os

import numpy as np
import pytest

import supg_ref as R

pytestmark = pytest.mark.gpu
_id = lambda k: "-".join(str(v) for v in k)


def bits(a):
    return np.ascontiguousarray(host(a), dtype=np.float64).view(np.int64)


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def dev(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def engine(om):
    import cutfemx_amd as cfx
    mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
    return mesh, cfx.FunctionSpace(mesh, 1)


def max_rel(got, want):
    return float(abs(got - want).max() / abs(want).max())


@pytest.mark.parametrize("key", R.MESHES, ids=_id)
def test_supg_system_equals_the_model(oracle, key):
    from cutfemx_amd import supg
    om, phi, speed, dt = R.setting(oracle, key, "sphere")
    mesh, V = engine(om)
    for fixed in (None, R.face_dofs(om)):
        A_ref, b_ref, _ = R.assemble(oracle, om, phi, speed, dt, fixed_dofs=fixed)
        for up in (np.asarray, dev):                                  # host values, values in HBM
            system = supg.build_forms(V, up(phi), up(speed), dt, fixed_dofs=fixed)
            A, b = supg.assemble(system)
            As = A.to_scipy()
            ea, eb = max_rel(As, A_ref), max_rel(host(b), b_ref)
            print(f"{key} fixed={fixed is not None} {up.__name__}: A {ea:.2e}, b {eb:.2e}")
            assert ea <= 1e-12 and eb <= 1e-12
            assert hasattr(b, "is_cuda") == (up is dev)
            if fixed is not None:
                D = As.toarray()
                assert not D[fixed].any() and not D[:, fixed].any() and np.array_equal(host(b)[fixed], phi[fixed])
    # another rule, another tau_scale, another dt through with_dt: the same kernels, no new registration
    ids = supg.kernel_ids()
    system = supg.with_dt(supg.build_forms(V, phi, speed, dt, tau_scale=0.25, qdegree=3), 0.3 * dt)
    A, b = supg.assemble(system)
    A_ref, b_ref, _ = R.assemble(oracle, om, phi, speed, 0.3 * dt, tau_scale=0.25, qdegree=3)
    assert supg.kernel_ids() == ids and system.dt == 0.3 * dt
    assert max_rel(A.to_scipy(), A_ref) <= 1e-12 and max_rel(b, b_ref) <= 1e-12


@pytest.mark.parametrize("key", R.MESHES, ids=_id)
def test_supg_advect(oracle, key):
    from cutfemx_amd import fem, supg
    # the plane: phi - dt F, exactly
    om, phi, speed, dt = R.setting(oracle, key, "linear")
    mesh, V = engine(om)
    system = supg.build_forms(V, dev(phi), dev(speed), dt)
    phi_new, info = supg.advect(system, rtol=R.RTOL)
    want = phi - dt * speed
    err = np.max(np.abs(host(phi_new) - want)) / np.max(np.abs(want))
    print(f"{key} plane: {info.iterations} iterations, max|phi_new - (phi - dt F)| / max = {err:.2e}")
    assert info.converged and hasattr(phi_new, "is_cuda") and phi_new.is_cuda
    assert err <= R.DIRECT_BAR
    assert np.array_equal(bits(system.phi.values), bits(phi))                       # phi itself is not modified
    # the sphere, free and with the face fixed: the direct solve of the engine's own matrix
    om, phi, speed, dt = R.setting(oracle, key, "sphere")
    for fixed in (None, R.face_dofs(om)):
        system = supg.build_forms(V, dev(phi), dev(speed), dt, fixed_dofs=fixed)
        A, b = supg.assemble(system)
        direct = R.solve_direct(A.to_scipy(), host(b), fixed)
        phi_new, info = supg.advect(system, rtol=R.RTOL)
        err = np.max(np.abs(host(phi_new) - direct)) / np.max(np.abs(direct))
        print(f"{key} sphere fixed={fixed is not None}: {info.iterations} iterations, max|phi_new - direct| / max = {err:.2e}")
        assert info.reason == fem.CG_CONVERGED and info.residual_norm <= R.RTOL * info.rhs_norm
        assert err <= R.DIRECT_BAR
        if fixed is not None:
            assert np.array_equal(bits(phi_new)[fixed], bits(phi)[fixed])
        # two calls agree bit for bit; host values give the same bits as values in HBM.  (With fixed dofs b passes
        # through fem.apply_lifting, whose sums are atomic: the two calls then agree to rounding, both inside the bar.)
        again, info2 = supg.advect(system, rtol=R.RTOL)
        hosted, info3 = supg.advect(supg.build_forms(V, phi, speed, dt, fixed_dofs=fixed), rtol=R.RTOL)
        assert isinstance(hosted, np.ndarray) and info2.converged and info3.converged
        if fixed is None and os.environ.get("CFX_ASSEMBLY") != "atomic":
            assert np.array_equal(bits(again), bits(phi_new)) and info2 == info
            assert np.array_equal(bits(hosted), bits(phi_new)) and info3 == info
        else:
            for other in (again, hosted):
                assert np.max(np.abs(host(other) - direct)) <= R.DIRECT_BAR * np.max(np.abs(direct))
    # the caller assigns, and the next step uses the new values
    system.phi.values = phi_new
    A2, b2 = supg.assemble(system)
    A_ref, b_ref, _ = R.assemble(oracle, om, host(phi_new), speed, dt, fixed_dofs=fixed)
    assert max_rel(A2.to_scipy(), A_ref) <= 1e-12 and max_rel(host(b2), b_ref) <= 1e-12
