"""The solve without a GPU: the defaults of cfx_cg_options_default, the loud failure of the compute entry points, the
argument checks that run on the host, the C++ facade, and the numpy restatement of the engine's conjugate gradients
(tests/solve_ref.py) on the oracle's deactivated cut Poisson systems -- the inputs of tests/test_gpu_solve.py, pinned here
as valid: symmetric, solved to the stated residual in the stated number of iterations, and indefinite once negated."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solve_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_default_options():
    from cutfemx_amd import _lib, fem
    o = fem.cg_default_options()
    assert (o.rtol, o.atol, o.max_iter, o.check_every, o.precond, o.lanes_per_row) == (1e-10, 0.0, 10000, 16, _lib.PC_JACOBI, 0)
    assert _lib.load().cfx_cg_options_default(None) == _lib.ERR_INVALID_ARGUMENT
    assert C.sizeof(_lib.CGOptions) == 32 and C.sizeof(_lib.CGInfoStruct) == 24
    assert (fem.CG_CONVERGED, fem.CG_MAX_ITER, fem.CG_BREAKDOWN, fem.CG_BAD_DIAGONAL) == \
        (R.CONVERGED, R.MAX_ITER, R.BREAKDOWN, R.BAD_DIAGONAL)


def _call(lib, fn, nrows=2, lanes=0, opt=None, null=None, n_rows=0, rows=None):
    ip = np.array([0, 1, 2], dtype=np.int64)
    ix = np.array([0, 1], dtype=np.int32)
    va, b, x = np.ones(2), np.ones(2), np.zeros(2)
    p = lambda a, name: None if null == name else a.ctypes.data_as(C.c_void_p)
    rp = None if rows is None else rows.ctypes.data_as(C.c_void_p)
    if fn == "spmv":
        return lib.cfx_csr_spmv(C.c_int64(nrows), p(ip, "indptr"), p(ix, "indices"), p(va, "values"), rp, C.c_int64(n_rows),
                                lanes, p(b, "x"), p(x, "y"))
    info = _call.info
    return lib.cfx_cg_solve(C.c_int64(nrows), p(ip, "indptr"), p(ix, "indices"), p(va, "values"), rp, C.c_int64(n_rows),
                            p(b, "b"), p(x, "x"), None if opt is None else C.byref(opt), C.byref(info))


def test_arguments_are_checked_on_the_host():
    from cutfemx_amd import _lib, fem
    lib = _lib.load()
    _call.info = _lib.CGInfoStruct()
    bad = _lib.ERR_INVALID_ARGUMENT
    for fn in ("spmv", "cg"):
        assert _call(lib, fn, nrows=-1) == bad
        assert _call(lib, fn, null="indptr") == bad and _call(lib, fn, null="values") == bad
        assert _call(lib, fn, rows=np.zeros(3, dtype=np.int32), n_rows=3) == bad          # more listed rows than rows
    assert _call(lib, "spmv", lanes=2) == bad and b"lanes_per_row" in lib.cfx_last_error()
    assert _call(lib, "spmv", null="x") == bad
    assert _call(lib, "cg", null="b") == bad
    for field, value in (("rtol", -1.0), ("atol", -1.0), ("max_iter", -1), ("check_every", -1), ("precond", 7),
                         ("lanes_per_row", 3)):
        o = fem.cg_default_options()
        setattr(o, field, value)
        assert _call(lib, "cg", opt=o) == bad, field


def test_python_argument_checks():
    """Checks of fem.cg_solve / fem.spmv that run before the library is entered."""
    from cutfemx_amd import fem
    A = fem.MergedCSR(None, None, None, 0, 3, 3, None, None)                 # (no HBM behind it: never dereferenced)
    with pytest.raises(ValueError, match="precond"):
        fem.cg_solve(A, np.zeros(3), precond="ilu")
    with pytest.raises(ValueError, match="not both"):
        fem.cg_solve(A, np.zeros(3), rows=np.zeros(1, dtype=np.int32), domain=object())
    R43 = fem.MergedCSR(None, None, None, 0, 4, 3, None, None)
    with pytest.raises(ValueError, match="square"):
        fem.cg_solve(R43, np.zeros(4))
    A.dtype = np.dtype(np.float32)
    with pytest.raises(TypeError, match="float64"):
        fem.spmv(A, np.zeros(3))
    info = fem.CGInfo(fem.CG_BREAKDOWN, 3, 1.0, 2.0)
    assert not info.converged and info.reason_name == "breakdown" and fem.CGInfo(0, 0, 0.0, 0.0).reason_name == "running"


def test_solve_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from cutfemx_amd import _lib
    lib = _lib.load()
    _call.info = _lib.CGInfoStruct()
    for fn in ("spmv", "cg"):
        assert _call(lib, fn) == _lib.ERR_HIP
        assert b"no HIP device" in lib.cfx_last_error()


def test_solve_facade_compiles_without_gpu(tmp_path):
    exe = tmp_path / "solve_facade"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/solve_facade.cpp"),
                    "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
                    f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert exe.exists()


@pytest.mark.parametrize("key", list(R.ITERATIONS), ids=lambda k: "-".join(str(v).replace(" ", "") for v in k))
def test_reference_pcg_on_oracle_systems(oracle, key):
    """Symmetric to rounding, solved to rtol in the tabulated number of iterations, true residual below rtol, agreement
    with the direct solve."""
    import scipy.sparse.linalg as spla
    c = R.case(oracle, *key)
    A, b = c["A"], c["b"]
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
    x, reason, its, rnorm, bnorm = R.pcg(A, b)
    assert reason == R.CONVERGED and its == R.ITERATIONS[key]
    assert rnorm <= 1e-10 * bnorm and np.linalg.norm(b - A @ x) <= 1e-10 * bnorm
    direct = spla.spsolve(A.tocsc(), b)
    assert np.max(np.abs(x - direct)) <= 3e-9 * np.max(np.abs(direct))
    inactive = c["ref"]["inactive"]
    assert np.all(x[inactive] == 0.0)                                   # identity rows, b = 0 there


def test_reference_pcg_variants(oracle):
    c = R.case(oracle, "box", 2, 8)
    A, b = c["A"], c["b"]
    k = R.ITERATIONS[("box", 2, 8)]
    # the negated matrix is negative definite: p.Ap <= 0 in the first iteration, x untouched
    x, reason, its, _, _ = R.pcg(-A, b)
    assert reason == R.BREAKDOWN and its == 0 and not x.any()
    # no preconditioner: more iterations
    _, reason, its_none, _, _ = R.pcg(A, b, precond="none")
    assert reason == R.CONVERGED and its_none > k
    # the active rows alone: the same solution (the identity rows hold x = 0)
    active = np.setdiff1d(np.arange(A.shape[0]), c["ref"]["inactive"])
    xa, reason, its_a, _, _ = R.pcg(A, b, rows=active)
    x, _, _, _, _ = R.pcg(A, b)
    assert reason == R.CONVERGED and its_a == k and np.max(np.abs(xa - x)) <= 1e-8 * np.max(np.abs(x))
    # max_iter, a zero right-hand side, a zero diagonal
    assert R.pcg(A, b, max_iter=5)[1:3] == (R.MAX_ITER, 5)
    assert R.pcg(A, np.zeros_like(b))[1:3] == (R.CONVERGED, 0)
    Z = A.copy().tolil()
    Z[int(active[0]), int(active[0])] = 0.0
    assert R.pcg(Z.tocsr(), b)[1] == R.BAD_DIAGONAL
    assert R.iteration_bound(53) == 61
