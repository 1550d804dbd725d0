"""fem::bicgstab_solve of the C++ facade (include/cutfemx_amd.hpp): tests/cpp/bicgstab_facade.cpp compiled with the host
compiler against libcutfemx_amd.so, run on a small convection-diffusion system written to a file, and compared with the
Python call on the same arrays -- every sum of the engine has a fixed order, so both give the same bits."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bicgstab_ref as R

ROOT = Path(__file__).resolve().parent.parent
KEY = ("convdiff", 12, 10, 8)


def _build(tmp_path):
    exe = tmp_path / "bicgstab_facade"
    cmd = ["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/bicgstab_facade.cpp"),
           "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
           f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.gpu
def test_cpp_bicgstab_facade(tmp_path):
    from cutfemx_amd import fem
    c = R.case(KEY)
    A, b = c["A"], c["b"]
    rows = np.arange(A.shape[0], dtype=np.int32)
    path = tmp_path / "system.bin"
    with open(path, "wb") as f:
        f.write(np.array([A.shape[0], A.nnz, rows.size], dtype=np.int64).tobytes())
        for a, dt in ((A.indptr, np.int64), (A.indices, np.int32), (A.data, np.float64), (b, np.float64), (rows, np.int32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([str(_build(tmp_path)), str(path), repr(R.RTOL)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"reason (\d+) iterations (\d+) xnorm (\S+) residual (\S+) rhs (\S+)", out)
    assert m, out
    reason, its, xnorm, rnorm, bnorm = int(m[1]), int(m[2]), float(m[3]), float(m[4]), float(m[5])
    x, info = fem.bicgstab_solve(fem.csr_from_arrays(A.indptr, A.indices, A.data), b, rtol=R.RTOL, rows=rows)
    assert (reason, its, rnorm, bnorm) == (info.reason, info.iterations, info.residual_norm, info.rhs_norm)
    assert reason == R.CONVERGED and its <= R.iteration_bound(R.ITERATIONS[KEY])
    assert abs(xnorm - np.linalg.norm(x)) <= 1e-14 * xnorm
    assert np.max(np.abs(x - c["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(c["xstar"]))
