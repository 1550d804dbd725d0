"""MINRES without a GPU: the defaults of cfx_minres_options_default, the argument checks that run on the host, the C++
facade, and the numpy restatement of the engine's MINRES (tests/minres_ref.py) on the oracle's cut Stokes systems -- the
inputs of tests/test_gpu_minres.py, pinned here as valid: symmetric, one negative eigenvalue per active pressure dof,
nonsingular, solved to the stated tolerance in the tabulated number of iterations.

Measured on these cases (restatement at rtol = 1e-8, |diag| Jacobi, active rows):
    case                 rows  iterations  max|x - x_direct| / max|x_direct|   | |eta| - true | / true
    ("box", 2, 8)         117     199          3.8e-08                            9e-09
    ("box", 2, 16)        348     614          3.4e-06                            5e-09
    ("box", 3, 4)         196     476          8.4e-08                            1e-09
    ("scrambled", 3, 6)   404    1150          1.5e-06                            4e-09
All below the bar 1e3 rtol = 1e-5 of minres_ref.DIRECT_BAR."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import minres_ref as R

ROOT = Path(__file__).resolve().parent.parent
CASES = list(R.ITERATIONS)
_id = lambda k: "-".join(str(v) for v in k)


def test_default_options():
    from cutfemx_amd import _lib, fem
    o = fem.minres_default_options()
    assert (o.rtol, o.atol, o.max_iter, o.check_every, o.precond, o.lanes_per_row) == (1e-10, 0.0, 10000, 16, _lib.PC_ABS_JACOBI, 0)
    assert (_lib.PC_NONE, _lib.PC_JACOBI, _lib.PC_ABS_JACOBI, _lib.PC_ABS_ROWSUM) == (0, 1, 2, 3)
    assert _lib.load().cfx_minres_options_default(None) == _lib.ERR_INVALID_ARGUMENT
    # ... and through ctypes alone
    raw = (C.c_byte * 32)()
    assert _lib.load().cfx_minres_options_default(C.byref(raw)) == 0
    got = _lib.CGOptions.from_buffer_copy(raw)
    assert (got.rtol, got.atol, got.max_iter, got.check_every, got.precond, got.lanes_per_row) == (1e-10, 0.0, 10000, 16, 2, 0)


def _call(lib, opt=None, null=None, nrows=2, n_rows=0, rows=None):
    ip = np.array([0, 1, 2], dtype=np.int64)
    ix = np.array([0, 1], dtype=np.int32)
    va, b, x = np.ones(2), np.ones(2), np.zeros(2)
    p = lambda a, name: None if null == name else a.ctypes.data_as(C.c_void_p)
    rp = None if rows is None else rows.ctypes.data_as(C.c_void_p)
    from cutfemx_amd import _lib
    info = _lib.CGInfoStruct()
    return lib.cfx_minres_solve(C.c_int64(nrows), p(ip, "indptr"), p(ix, "indices"), p(va, "values"), rp, C.c_int64(n_rows),
                                p(b, "b"), p(x, "x"), None if opt is None else C.byref(opt), C.byref(info))


def test_arguments_are_checked_on_the_host():
    from cutfemx_amd import _lib, fem
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert _call(lib, nrows=-1) == bad and _call(lib, null="indptr") == bad and _call(lib, null="b") == bad
    assert _call(lib, rows=np.zeros(3, dtype=np.int32), n_rows=3) == bad
    for field, value in (("rtol", -1.0), ("atol", -1.0), ("max_iter", -1), ("check_every", -1), ("precond", 1), ("precond", 4),
                         ("lanes_per_row", 3)):
        o = fem.minres_default_options()
        setattr(o, field, value)
        assert _call(lib, opt=o) == bad, field
    # cfx_cg_solve keeps refusing the new ids
    for pc in (_lib.PC_ABS_JACOBI, _lib.PC_ABS_ROWSUM):
        o = fem.cg_default_options()
        o.precond = pc
        ip, ix = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
        va, b, x, info = np.ones(2), np.ones(2), np.zeros(2), _lib.CGInfoStruct()
        q = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.cfx_cg_solve(C.c_int64(2), q(ip), q(ix), q(va), None, C.c_int64(0), q(b), q(x), C.byref(o), C.byref(info)) == bad
    A = fem.MergedCSR(None, None, None, 0, 3, 3, None, None)                 # (no HBM behind it: never dereferenced)
    with pytest.raises(ValueError, match="precond"):
        fem.minres_solve(A, np.zeros(3), precond="jacobi")
    with pytest.raises(ValueError, match="not both"):
        fem.minres_solve(A, np.zeros(3), rows=np.zeros(1, dtype=np.int32), domain=object())
    with pytest.raises(ValueError, match="square"):
        fem.minres_solve(fem.MergedCSR(None, None, None, 0, 4, 3, None, None), np.zeros(4))


def test_minres_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from cutfemx_amd import _lib
    lib = _lib.load()
    assert _call(lib) == _lib.ERR_HIP and b"no HIP device" in lib.cfx_last_error()


def test_minres_facade_compiles_without_gpu(tmp_path):
    exe = tmp_path / "minres_facade"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/minres_facade.cpp"),
                    "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
                    f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert exe.exists()


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_stokes_cases_are_symmetric_indefinite_and_nonsingular(oracle, key):
    """What the cases rest on: symmetric to 1e-14, exactly one negative eigenvalue per active pressure dof, none within
    1e-6 of zero; inactive rows are identity rows."""
    c = R.stokes_case(oracle, *key)
    A, rows, nu = c["A"], c["rows"], c["nu"]
    assert abs(A - A.T).max() <= 1e-14
    ev = np.linalg.eigvalsh(A[rows][:, rows].toarray())
    n_pressure_active = int(np.count_nonzero(rows >= nu))
    assert 0 < n_pressure_active < rows.size
    assert int(np.count_nonzero(ev < 0.0)) == n_pressure_active and np.abs(ev).min() > 1e-6
    I = A[c["inactive"]]
    assert c["inactive"].size > 0 and I.nnz >= c["inactive"].size and np.array_equal(I @ np.ones(A.shape[0]), np.ones(c["inactive"].size))
    assert np.all(np.diff(rows) > 0) and not np.intersect1d(rows, c["inactive"]).size


@pytest.mark.parametrize("key", CASES, ids=_id)
def test_restatement_on_stokes_cases(oracle, key):
    """The restatement against spsolve and scipy's minres with the same M; |eta| against the true residual; the table."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    c = R.stokes_case(oracle, *key)
    A, b, rows = c["A"], c["b"], c["rows"]
    x, reason, its, rnorm, bnorm = R.minres(A, b, rtol=R.RTOL, rows=rows)
    assert reason == R.CONVERGED and its == R.ITERATIONS[key]
    assert rnorm <= R.RTOL * bnorm and np.all(x[c["inactive"]] == 0.0)
    direct = spla.spsolve(A.tocsc(), b)
    ratio = np.max(np.abs(x - direct)) / np.max(np.abs(direct))
    true = R.minv_norm(A, b - A @ x, rows, "abs_jacobi")
    print(f"{key}: {its} iterations, max|x - direct| / max|direct| = {ratio:.2e}, |eta| = {rnorm:.3e}, true = {true:.3e}")
    assert ratio <= R.DIRECT_BAR
    assert np.max(np.abs(x - c["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(c["xstar"]))
    assert abs(rnorm - true) <= 1e-3 * true
    # scipy's minres with the same M on the active block.  Its own rule is relative to |A| |x|, not to |b|: run it two
    # orders tighter and hold BOTH to the engine's rule on the true residual
    Aa = A[rows][:, rows].tocsr()
    m = np.abs(Aa.diagonal())
    xs, flag = spla.minres(Aa, b[rows], M=sp.diags(1.0 / m), rtol=1e-2 * R.RTOL, maxiter=20000)
    rs = b[rows] - Aa @ xs
    assert flag == 0 and np.sqrt(rs @ (rs / m)) <= R.RTOL * bnorm
    assert true <= (1.0 + 1e-3) * R.RTOL * bnorm
    assert np.max(np.abs(xs - x[rows])) <= 2.0 * R.DIRECT_BAR * np.max(np.abs(direct))


def test_restatement_variants(oracle):
    import scipy.sparse as sp
    key = ("box", 2, 8)
    c = R.stokes_case(oracle, *key)
    A, b, rows, nu = c["A"], c["b"], c["rows"], c["nu"]
    k = R.ITERATIONS[key]
    # the other preconditioners; none takes about twice as long
    k_sum = R.minres(A, b, rtol=R.RTOL, rows=rows, precond="abs_rowsum")
    k_none = R.minres(A, b, rtol=R.RTOL, rows=rows, precond=None)
    assert k_sum[1] == k_none[1] == R.CONVERGED and abs(k_sum[2] - k) <= 0.1 * k and k_none[2] > 1.5 * k
    # all rows: the identity rows hold x = 0
    xa, reason, its, _, _ = R.minres(A, b, rtol=R.RTOL)
    assert reason == R.CONVERGED and its <= R.iteration_bound(k) and np.max(np.abs(xa - c["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(c["xstar"]))
    # edges
    assert R.minres(A, b, rows=rows, max_iter=3)[1:3] == (R.MAX_ITER, 3)
    assert R.minres(A, b, rows=rows, max_iter=0)[1:3] == (R.MAX_ITER, 0)
    x, reason, its, rn, bn = R.minres(A, np.zeros_like(b), rows=rows)
    assert (reason, its, rn, bn) == (R.CONVERGED, 0, 0.0, 0.0) and not x.any()
    assert R.minres(A, b, c["xstar"], rows=rows, rtol=1e-6)[1:3] == (R.CONVERGED, 0)
    # the pressure diagonal removed from the pattern: |diag| refuses, the row sum works
    N = R.without_pressure_diagonal(A, rows, nu)
    bn_ = N @ c["xstar"]
    x, reason, its, _, _ = R.minres(N, bn_, rows=rows, precond="abs_jacobi")
    assert (reason, its) == (R.BAD_DIAGONAL, 0) and not x.any()
    x, reason, its, _, _ = R.minres(N, bn_, rtol=R.RTOL, rows=rows, precond="abs_rowsum")
    assert reason == R.CONVERGED and np.max(np.abs(x - c["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(c["xstar"]))
    # 1 x 1 and the 2 x 2 permutation: exact in at most 2 iterations
    x, reason, its, _, _ = R.minres(sp.csr_matrix(np.array([[-4.0]])), np.array([2.0]), precond=None, rtol=1e-12)
    assert reason == R.CONVERGED and its == 1 and x[0] == -0.5
    x, reason, its, _, _ = R.minres(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), np.array([1.0, 2.0]), precond=None, rtol=1e-12)
    assert reason == R.CONVERGED and its == 2 and np.max(np.abs(x - [2.0, 1.0])) <= 1e-14
