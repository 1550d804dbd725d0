"""distance::reinitialize of the C++ facade (include/cutfemx_amd.hpp): tests/cpp/reinit_facade.cpp compiled with the host
compiler against libcutfemx_amd.so, run on a mesh and a level set written to a file, and compared with the Python call on
the same arrays -- the engine's result does not depend on the order of its lists, so both give the same bits."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import reinit_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path):
    exe = tmp_path / "reinit_facade"
    cmd = ["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/reinit_facade.cpp"),
           "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
           f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.gpu
def test_cpp_reinit_facade(oracle, tmp_path):
    import cutfemx_amd as cfx
    c = R.case(oracle, "scrambled3")
    om, phi = c["mesh"], c["phi"]
    path, out_path = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(np.array([om.tdim, om.x.shape[0], om.conn.shape[0]], dtype=np.int64).tobytes())
        for a, dt in ((om.x, np.float64), (om.conn, np.int32), (phi, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([str(_build(tmp_path)), str(path), str(out_path)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"reason (\d+) sweeps (\d+) seeds (\d+) updates (\d+)", out)
    assert m, out
    mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
    fn = cfx.Function(cfx.FunctionSpace(mesh, 1), values=phi.copy())
    info = cfx.distance.reinitialize(fn)
    assert tuple(int(g) for g in m.groups()) == (info.reason, info.sweeps, info.seeds, info.updates)
    assert info.reason == cfx.distance.REINIT_CONVERGED
    got = np.fromfile(out_path, dtype=np.float64)
    assert np.array_equal(got, fn.values)
    assert np.max(np.abs(got - c["out"])) <= 1e-10
