"""The SUPG level-set step without a GPU: the two integrand sources of cutfemx_amd/supg.py register and compile for
their variants (hipRTC targets gfx950; no device needed), and the numpy model of tests/supg_ref.py -- the reference of
tests/test_gpu_supg.py -- is pinned: nonsymmetric, nonsingular, and EXACT on a plane: for phi = n . x - c with |n| = 1
and a constant speed F, n_K = n in every cell, so phi - dt F satisfies u + dt a . grad u = phi pointwise and with it both
terms of the scheme, whatever tau and the rule are.

Measured (bicgstab_ref.bicgstab, Jacobi, rtol = 1e-10, x0 = phi, on the model's systems; max|x - direct| / max|direct|):
    mesh                  dofs   linear     sphere     linear, fixed face   sphere, fixed face     iterations
    ("box", 2, 4)           25   8.00e-11   3.04e-11   1.00e-10             8.43e-11               10 .. 14
    ("box", 3, 3)           64   2.08e-10   2.78e-10   4.56e-11             1.83e-10               11 .. 17
    ("scrambled", 3, 6)    343   5.57e-10   3.52e-10   1.59e-11             4.27e-10               12 .. 19
The worst, 5.57e-10, is supg_ref.DIRECT_WORST (5.6e-10); ten times that is supg_ref.DIRECT_BAR."""
import numpy as np
import pytest

import bicgstab_ref as B
import supg_ref as R

_id = lambda k: "-".join(str(v) for v in k)


def test_integrands_register_and_compile():
    from cutfemx_amd import fem, supg
    lhs, rhs = supg.kernel_ids()
    assert lhs != rhs and (lhs, rhs) == supg.kernel_ids()                      # registered once
    assert fem._user_integrand_rank[lhs] == 2 and fem._user_integrand_rank[rhs] == 1
    assert supg.VARIANTS == ((2, 3, 1), (3, 4, 1))
    for kid in (lhs, rhs):
        for tdim, nd, bs in supg.VARIANTS:
            fem.compile_integrand(kid, tdim, nd, bs, coefficients=[(nd, 1), (nd, 1)])   # (compiled already: returns at once)
    # a source that breaks the contract is refused with the compiler's message
    with pytest.raises(ValueError, match="does not compile"):
        fem.register_integrand("cfx_supg_broken", supg.LHS_SOURCE.replace("cfx_supg_lhs", "cfx_supg_broken").replace("nn;", "nn"),
                               rank=2, variant=(2, 3, 1), coefficients=[(3, 1), (3, 1)])


@pytest.mark.parametrize("key", R.MESHES, ids=_id)
def test_model_is_nonsymmetric_and_nonsingular(oracle, key):
    om, phi, speed, dt = R.setting(oracle, key, "sphere")
    A, b, _ = R.assemble(oracle, om, phi, speed, dt)
    D = A.toarray()
    assert np.abs(D - D.T).max() > 1e-3 * np.abs(D).max()
    sv = np.linalg.svd(D, compute_uv=False)
    assert sv[-1] > 1e-4 * sv[0], (sv[0], sv[-1])
    # with the face fixed: zero rows and columns there, nonsingular on the rest
    fixed = R.face_dofs(om)
    Af, bf, _ = R.assemble(oracle, om, phi, speed, dt, fixed_dofs=fixed)
    F = Af.toarray()
    free = np.setdiff1d(np.arange(om.nnodes), fixed)
    assert fixed.size > 0 and not F[fixed].any() and not F[:, fixed].any() and np.array_equal(bf[fixed], phi[fixed])
    assert np.array_equal(F[np.ix_(free, free)], D[np.ix_(free, free)])
    assert np.linalg.svd(F[np.ix_(free, free)], compute_uv=False)[-1] > 1e-4 * sv[0]


@pytest.mark.parametrize("key", R.MESHES, ids=_id)
def test_model_is_exact_on_a_plane(oracle, key):
    om = R.mesh_of(oracle, key)
    phi, speed, n, c = R.linear(om)
    dt = 0.5 / key[2]
    want = phi - dt * speed
    for qdegree, tau_scale, fixed in ((2, 1.0, None), (3, 0.25, None), (2, 1.0, R.face_dofs(om))):
        A, b, _ = R.assemble(oracle, om, phi, speed, dt, tau_scale=tau_scale, qdegree=qdegree, fixed_dofs=fixed)
        x = R.solve_direct(A, b, fixed)
        if fixed is not None:                     # the fixed dofs keep the OLD phi: the exact solution only where none is fixed
            assert np.array_equal(x[fixed], phi[fixed])
            continue
        assert np.max(np.abs(x - want)) <= 1e-12 * np.max(np.abs(phi)), np.max(np.abs(x - want))


@pytest.mark.parametrize("key", R.MESHES, ids=_id)
def test_restatement_on_the_model_systems(oracle, key):
    """The BiCGStab restatement on the systems the GPU test solves: converged, and its distance from the direct solve --
    the figures supg_ref.DIRECT_WORST is taken from."""
    for which in ("linear", "sphere"):
        om, phi, speed, dt = R.setting(oracle, key, which)
        for fixed in (None, R.face_dofs(om)):
            A, b, _ = R.assemble(oracle, om, phi, speed, dt, fixed_dofs=fixed)
            rows = None if fixed is None else np.setdiff1d(np.arange(om.nnodes), fixed)
            x, reason, its, rn, bn = B.bicgstab(A, b, phi, rtol=R.RTOL, rows=rows)
            direct = R.solve_direct(A, b, fixed)
            ratio = np.max(np.abs(x - direct)) / np.max(np.abs(direct))
            print(f"{key} {which} fixed={fixed is not None}: {its} iterations, max|x - direct| / max|direct| = {ratio:.2e}")
            assert reason == B.CONVERGED and rn <= R.RTOL * bn
            assert ratio <= R.DIRECT_WORST
