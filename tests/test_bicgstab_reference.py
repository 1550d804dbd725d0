"""BiCGStab without a GPU: the defaults of cfx_bicgstab_options_default, the argument checks that run on the host, the
C++ facade, and the numpy restatement of the engine's BiCGStab (tests/bicgstab_ref.py) on the small nonsymmetric matrices
of that file -- the inputs of tests/test_gpu_bicgstab.py, pinned here as valid: nonsymmetric, nonsingular, solved to the
stated tolerance in the tabulated number of iterations, whatever the order of the sums.

Measured on these cases (restatement at rtol = 1e-10, Jacobi, x0 = 0, b = A x*):
    case                        rows  iterations  max|x - x_direct| / max|x_direct|  true |r| / recurrence |r|  8 permuted orders
    ("convdiff", 8, 8, 2)         64      25          4.00e-10                           1.000                     25 .. 25
    ("convdiff", 12, 10, 8)      120      28          4.25e-10                           1.000                     28 .. 28
    ("convdiff", 6, 5, 20)        30      16          8.97e-11                           1.000                     16 .. 16
    ("convdiff", 40, 37, 4)     1480      79          3.02e-10                           1.000                     79 .. 79
    ("long_rows", 300, 150)      300       5          5.11e-11                           1.000                      5 .. 5
    ("tridiag", 524588)       524588      20          1.15e-10                           1.000                     20 .. 20
The worst ratio, 4.25e-10, is bicgstab_ref.DIRECT_WORST (4.3e-10); ten times that is DIRECT_BAR, the engine's bar."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bicgstab_ref as R

ROOT = Path(__file__).resolve().parent.parent
CASES = list(R.ITERATIONS)
_id = lambda k: "-".join(str(v) for v in k)
ORDERS = 8


def test_default_options():
    from cutfemx_amd import _lib, fem
    o = fem.bicgstab_default_options()
    assert (o.rtol, o.atol, o.max_iter, o.check_every, o.precond, o.lanes_per_row) == (1e-10, 0.0, 10000, 16, _lib.PC_JACOBI, 0)
    assert _lib.load().cfx_bicgstab_options_default(None) == _lib.ERR_INVALID_ARGUMENT
    # ... and through ctypes alone
    raw = (C.c_byte * 32)()
    assert _lib.load().cfx_bicgstab_options_default(C.byref(raw)) == 0
    got = _lib.CGOptions.from_buffer_copy(raw)
    assert (got.rtol, got.atol, got.max_iter, got.check_every, got.precond, got.lanes_per_row) == (1e-10, 0.0, 10000, 16, 1, 0)
    assert "cfx_bicgstab_solve" in _lib.SYMBOLS and "cfx_bicgstab_options_default" in _lib.SYMBOLS


def _call(lib, opt=None, null=None, nrows=2, n_rows=0, rows=None):
    ip = np.array([0, 1, 2], dtype=np.int64)
    ix = np.array([0, 1], dtype=np.int32)
    va, b, x = np.ones(2), np.ones(2), np.zeros(2)
    p = lambda a, name: None if null == name else a.ctypes.data_as(C.c_void_p)
    rp = None if rows is None else rows.ctypes.data_as(C.c_void_p)
    from cutfemx_amd import _lib
    info = _lib.CGInfoStruct()
    return lib.cfx_bicgstab_solve(C.c_int64(nrows), p(ip, "indptr"), p(ix, "indices"), p(va, "values"), rp, C.c_int64(n_rows),
                                  p(b, "b"), p(x, "x"), None if opt is None else C.byref(opt), C.byref(info))


def test_arguments_are_checked_on_the_host():
    from cutfemx_amd import _lib, fem
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert _call(lib, nrows=-1) == bad and _call(lib, null="indptr") == bad and _call(lib, null="b") == bad
    assert _call(lib, rows=np.zeros(3, dtype=np.int32), n_rows=3) == bad
    for field, value in (("rtol", -1.0), ("atol", -1.0), ("max_iter", -1), ("check_every", -1), ("max_iter", 0x1999999a),
                         ("precond", _lib.PC_ABS_JACOBI), ("precond", _lib.PC_ABS_ROWSUM), ("precond", 4), ("lanes_per_row", 3)):
        o = fem.bicgstab_default_options()
        setattr(o, field, value)
        assert _call(lib, opt=o) == bad, field
    A = fem.MergedCSR(None, None, None, 0, 3, 3, None, None)                 # (no HBM behind it: never dereferenced)
    with pytest.raises(ValueError, match="precond"):
        fem.bicgstab_solve(A, np.zeros(3), precond="abs_jacobi")
    with pytest.raises(ValueError, match="not both"):
        fem.bicgstab_solve(A, np.zeros(3), rows=np.zeros(1, dtype=np.int32), domain=object())
    with pytest.raises(ValueError, match="square"):
        fem.bicgstab_solve(fem.MergedCSR(None, None, None, 0, 4, 3, None, None), np.zeros(4))


def test_bicgstab_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from cutfemx_amd import _lib
    lib = _lib.load()
    assert _call(lib) == _lib.ERR_HIP and b"no HIP device" in lib.cfx_last_error()


def test_bicgstab_facade_compiles_without_gpu(tmp_path):
    exe = tmp_path / "bicgstab_facade"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/bicgstab_facade.cpp"),
                    "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
                    f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert exe.exists()


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_restatement_on_the_cases(key):
    """Nonsymmetric; the restatement against spsolve and against x*; the recurrence residual against the true one; the
    table; the counts under permuted summation orders inside solve_ref's band."""
    import scipy.sparse.linalg as spla
    c = R.case(key)
    A, b = c["A"], c["b"]
    assert abs(A - A.T).max() > 0.0
    x, reason, its, rnorm, bnorm = R.solved(key)
    assert reason == R.CONVERGED and its == R.ITERATIONS[key]
    assert rnorm <= R.RTOL * bnorm and bnorm == pytest.approx(np.linalg.norm(b), rel=1e-13)
    direct = spla.spsolve(A.tocsc(), b)
    ratio = np.max(np.abs(x - direct)) / np.max(np.abs(direct))
    true = float(np.linalg.norm(b - A @ x))
    k = R.ITERATIONS[key]
    counts = [R.bicgstab(A, b, rtol=R.RTOL, dot=R.permuted_dot(seed))[1:3] for seed in range(ORDERS)]
    print(f"{key}: {its} iterations, max|x - direct| / max|direct| = {ratio:.2e}, recurrence |r| = {rnorm:.3e}, true = {true:.3e}, "
          f"permuted orders: {min(n for _, n in counts)} .. {max(n for _, n in counts)}")
    assert ratio <= R.DIRECT_BAR
    assert np.max(np.abs(x - c["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(c["xstar"]))
    assert true <= 2.0 * rnorm and rnorm <= 2.0 * true
    for why, n in counts:
        assert why == R.CONVERGED and k / 1.1 - 2 <= n <= R.iteration_bound(k), (key, counts)


def test_restatement_variants():
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    key = ("convdiff", 12, 10, 8)
    c = R.case(key)
    A, b, xstar = c["A"], c["b"], c["xstar"]
    n = A.shape[0]
    # no preconditioner converges to the same solution
    x, reason, its, _, _ = R.bicgstab(A, b, rtol=R.RTOL, precond=None)
    assert reason == R.CONVERGED and np.max(np.abs(x - xstar)) <= R.DIRECT_BAR * np.max(np.abs(xstar))
    # a row list: x off the list is data
    rng = np.random.default_rng(3)
    rows = np.sort(rng.choice(n, size=n // 2, replace=False))
    others = np.setdiff1d(np.arange(n), rows)
    x0 = rng.standard_normal(n)
    x, reason, its, _, _ = R.bicgstab(A, b, x0, rtol=R.RTOL, rows=rows)
    y = spla.spsolve(A[rows][:, rows].tocsc(), b[rows] - A[rows][:, others] @ x0[others])
    assert reason == R.CONVERGED and np.array_equal(x[others], x0[others])
    assert np.max(np.abs(x[rows] - y)) <= R.DIRECT_BAR * np.max(np.abs(y))
    # edges
    assert R.bicgstab(A, b, max_iter=3)[1:3] == (R.MAX_ITER, 3)
    assert R.bicgstab(A, b, max_iter=0)[1:3] == (R.MAX_ITER, 0)
    x, reason, its, rn, bn = R.bicgstab(A, np.zeros_like(b))
    assert (reason, its, rn, bn) == (R.CONVERGED, 0, 0.0, 0.0) and not x.any()
    assert R.bicgstab(A, b, xstar, rtol=1e-6)[1:3] == (R.CONVERGED, 0)
    # the 2 x 2 rotation: rhat.v = 0 in the first iteration; with Jacobi there is no diagonal
    J = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    x, reason, its, _, _ = R.bicgstab(J, np.array([1.0, 0.0]), precond=None)
    assert (reason, its) == (R.BREAKDOWN, 0) and not x.any()
    x, reason, its, _, _ = R.bicgstab(J, np.array([1.0, 0.0]), precond="jacobi")
    assert (reason, its) == (R.BAD_DIAGONAL, 0) and not x.any()
    # a diagonal matrix with pivots of both signs: Jacobi makes A M^-1 = I, the half step ends it
    d, bd = R.signed_diagonal()
    x, reason, its, rn, _ = R.bicgstab(sp.diags(d, format="csr"), bd, precond="jacobi")
    assert (reason, its) == (R.CONVERGED, 1) and np.max(np.abs(x - bd / d) / np.abs(bd / d)) <= 4 * np.finfo(float).eps

