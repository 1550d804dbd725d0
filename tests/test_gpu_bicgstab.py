"""BiCGStab in HBM (cutfemx_amd/csrc/cfx_solve.hip, cfx_bicgstab_solve) through fem.bicgstab_solve and
fem.csr_from_arrays, on the nonsymmetric matrices of tests/bicgstab_ref.py (pinned as nonsymmetric, nonsingular and stable
in their iteration counts under permuted summation orders by tests/test_bicgstab_reference.py).

References.  The numpy restatement of the same recurrence (bicgstab_ref.bicgstab): the iteration count within
[k / 1.1 - 2, ceil(1.1 k) + 2] (every sum of the engine runs in another order), |b| to 1e-12, the recurrence residual
under the rule, the true residual within 10 x the restatement's own at its final iterate, and the solution within
bicgstab_ref.DIRECT_BAR (ten times the restatement's own worst distance from the direct solve) of the x* the right-hand
side was made from.  Every sum of the engine has a fixed order, so bits are compared wherever two calls must agree."""
import numpy as np
import pytest

import bicgstab_ref as R

pytestmark = pytest.mark.gpu
RTOL = R.RTOL
LANES = (1, 4, 8, 16, 64)
SMALL = ("convdiff", 12, 10, 8)


def _id(v):
    return "-".join(str(p).replace(" ", "") for p in v) if isinstance(v, tuple) else str(v)


def bits(a):
    return np.ascontiguousarray(host(a), dtype=np.float64).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def residual2(As, b, x, rows=None):
    r = b - As @ host(x)
    return float(np.linalg.norm(r if rows is None else r[rows]))


def in_count_band(k, k_ref):
    return k_ref / 1.1 - 2 <= k <= R.iteration_bound(k_ref)


_HBM = {}


def hbm(key):
    """The matrix of a case in HBM (fem.csr_from_arrays), once."""
    if key not in _HBM:
        from cutfemx_amd import fem
        A = R.case(key)["A"]
        _HBM[key] = fem.csr_from_arrays(A.indptr, A.indices, A.data)
    return _HBM[key]


def check_against_restatement(key, x, info, what=""):
    from cutfemx_amd import fem
    c = R.case(key)
    As, b, xstar = c["A"], c["b"], c["xstar"]
    x_ref, reason, k_ref, rn_ref, bn_ref = R.solved(key)
    true_ref, true = residual2(As, b, x_ref), residual2(As, b, x)
    err = np.max(np.abs(host(x) - xstar)) / np.max(np.abs(xstar))
    print(f"{key} {what}: engine {info.iterations} iterations, numpy {k_ref}; |r| / |b| = {info.residual_norm / info.rhs_norm:.2e}; "
          f"true |r|_2 engine {true:.3e}, numpy {true_ref:.3e}; max|x - x*| / max|x*| = {err:.2e}")
    assert reason == R.CONVERGED and k_ref == R.ITERATIONS[key]
    assert info.reason == fem.CG_CONVERGED and info.converged, (what, info)
    assert in_count_band(info.iterations, k_ref), (what, info.iterations, k_ref)
    assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref and info.residual_norm <= RTOL * info.rhs_norm, (what, info)
    assert true <= 10.0 * true_ref, f"{what} true residual: engine {true:.3e}, restatement {true_ref:.3e}"
    assert err <= R.DIRECT_BAR, (what, err)


# ---- 1. parity with the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(R.ITERATIONS), ids=_id)
def test_bicgstab_parity_with_the_restatement(key):
    from cutfemx_amd import fem
    x, info = fem.bicgstab_solve(hbm(key), dev(R.case(key)["b"]), rtol=RTOL)
    check_against_restatement(key, x, info)


# ---- 2. every lanes_per_row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key", [SMALL, ("long_rows", 300, 150)], ids=_id)
def test_bicgstab_lanes(key, lanes):
    from cutfemx_amd import fem
    x, info = fem.bicgstab_solve(hbm(key), dev(R.case(key)["b"]), rtol=RTOL, lanes_per_row=lanes)
    check_against_restatement(key, x, info, f"L = {lanes}")


# ---- 3. a row list and a start vector with entries off the list -------------------------------------------------------
def test_bicgstab_row_list():
    import scipy.sparse.linalg as spla
    import torch
    from cutfemx_amd import fem
    c = R.case(SMALL)
    As, b = c["A"], c["b"]
    n = As.shape[0]
    rng = np.random.default_rng(3)
    rows = np.sort(rng.choice(n, size=n // 2, replace=False)).astype(np.int32)
    others = np.setdiff1d(np.arange(n), rows)
    x0 = rng.standard_normal(n)
    assert abs(As[rows][:, others]).max() > 1.0 and np.all(x0[others] != 0.0)
    want = spla.spsolve(As[rows][:, rows].tocsc(), b[rows] - As[rows][:, others] @ x0[others])
    x_ref, reason, k_ref, rn_ref, bn_ref = R.bicgstab(As, b, x0, rtol=RTOL, rows=rows)
    assert reason == R.CONVERGED
    for lanes, rows_in in ((0, rows), (64, torch.tensor(rows, device="cuda"))):         # a host list, a device list
        x, info = fem.bicgstab_solve(hbm(SMALL), dev(b), x0=dev(x0), rows=rows_in, rtol=RTOL, lanes_per_row=lanes)
        assert info.converged and in_count_band(info.iterations, k_ref), (info, k_ref)
        assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref and info.residual_norm <= RTOL * info.rhs_norm
        assert residual2(As, b, x, rows) <= 10.0 * residual2(As, b, x_ref, rows)
        assert np.max(np.abs(host(x)[rows] - want)) <= R.DIRECT_BAR * np.max(np.abs(want))
        assert np.array_equal(bits(x)[others], bits(x0)[others])


# ---- 4. determinism and freezing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [SMALL, ("convdiff", 40, 37, 4)], ids=_id)
def test_bicgstab_is_deterministic_and_frozen(key):
    from cutfemx_amd import _lib, fem
    A, b = hbm(key), R.case(key)["b"]
    bd = dev(b)
    x, info = fem.bicgstab_solve(A, bd, rtol=RTOL)
    x2, info2 = fem.bicgstab_solve(A, bd, rtol=RTOL)
    assert info.converged and np.array_equal(bits(x), bits(x2)) and info2 == info
    k = info.iterations
    for more in (dict(check_every=1), dict(check_every=16), dict(check_every=0, max_iter=k + 5)):
        x3, info3 = fem.bicgstab_solve(A, bd, rtol=RTOL, **more)
        assert np.array_equal(bits(x3), bits(x)) and info3 == info, more
    buf = fem.cg_info_buffer()
    s0 = _lib.sync_count()
    x4, out = fem.bicgstab_solve(A, bd, rtol=RTOL, check_every=0, max_iter=k + 5, info_out=buf)
    assert _lib.sync_count() == s0 and out is buf
    assert np.array_equal(bits(x4), bits(x)) and fem.read_cg_info(buf) == info
    # numpy in, numpy out (the same kernels on staged copies); device tensor in, device tensor out
    xh, infoh = fem.bicgstab_solve(A, b, rtol=RTOL)
    assert isinstance(xh, np.ndarray) and np.array_equal(bits(xh), bits(x)) and infoh == info
    assert hasattr(x, "is_cuda") and x.is_cuda and x.data_ptr() != bd.data_ptr()


def test_bicgstab_launch_count():
    """Five launches per iteration and a constant number around them."""
    from helpers import profiled
    from cutfemx_amd import fem
    bd = dev(R.case(SMALL)["b"])
    (x, info), names = profiled(lambda: fem.bicgstab_solve(hbm(SMALL), bd, rtol=RTOL, check_every=16))
    launched = -(-info.iterations // 16) * 16
    for name in ("bicg_spmv_v", "bicg_half", "bicg_spmv_t", "bicg_update", "bicg_direction"):
        assert names[name] == launched, (names, info)
    assert names["bicg_init"] == names["bicg_start"] == 1
    assert sum(names.values()) <= 5 * launched + 8, names


# ---- 5. edges ------------------------------------------------------------------------------------------------------------
def test_bicgstab_edges():
    import scipy.sparse as sp
    from cutfemx_amd import fem
    c = R.case(SMALL)
    As, b, xstar = c["A"], c["b"], c["xstar"]
    A = hbm(SMALL)
    # b = 0 with x0 = 0
    x, info = fem.bicgstab_solve(A, dev(np.zeros_like(b)))
    assert (info.reason, info.iterations, info.residual_norm, info.rhs_norm) == (fem.CG_CONVERGED, 0, 0.0, 0.0) and not host(x).any()
    # x0 = x*
    x, info = fem.bicgstab_solve(A, dev(b), x0=dev(xstar), rtol=1e-6)
    assert (info.reason, info.iterations) == (fem.CG_CONVERGED, 0) and np.array_equal(bits(x), bits(xstar))
    # max_iter 3 and 0: the restatement's iterates
    for m in (3, 0):
        x_ref, reason, its, rn_ref, _ = R.bicgstab(As, b, max_iter=m)
        x, info = fem.bicgstab_solve(A, dev(b), max_iter=m)
        assert (info.reason, info.iterations) == (fem.CG_MAX_ITER, m) == (reason, its)
        assert np.max(np.abs(host(x) - x_ref)) <= 1e-12 * np.max(np.abs(xstar))
        assert abs(info.residual_norm - rn_ref) <= 1e-10 * rn_ref
    # the 2 x 2 rotation: rhat.v = 0 without a preconditioner, no diagonal with Jacobi; x = x0 bit for bit
    J = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    AJ = fem.csr_from_arrays(J.indptr, J.indices, J.data)
    x, info = fem.bicgstab_solve(AJ, dev([1.0, 0.0]), precond=None)
    assert (info.reason, info.iterations) == (fem.CG_BREAKDOWN, 0) and not host(x).any()
    x0 = np.array([0.25, -3.0])
    x, info = fem.bicgstab_solve(AJ, dev([1.0, 0.0]), x0=dev(x0), precond="jacobi")
    assert (info.reason, info.iterations) == (fem.CG_BAD_DIAGONAL, 0) and np.array_equal(bits(x), bits(x0))
    # a diagonal matrix with pivots of both signs: one iteration, ended by the half step
    d, bd = R.signed_diagonal()
    D = sp.diags(d, format="csr")
    x, info = fem.bicgstab_solve(fem.csr_from_arrays(D.indptr, D.indices, D.data), dev(bd))
    assert (info.reason, info.iterations) == (fem.CG_CONVERGED, 1)
    assert np.max(np.abs(host(x) - bd / d) / np.abs(bd / d)) <= 4 * np.finfo(float).eps
    # the ABS preconditioners are MINRES's
    with pytest.raises(ValueError, match="precond"):
        fem.bicgstab_solve(A, dev(b), precond="abs_rowsum")
