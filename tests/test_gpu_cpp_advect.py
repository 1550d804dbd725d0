"""distance::advect of the C++ facade (include/cutfemx_amd.hpp): tests/cpp/advect_facade.cpp compiled with the host
compiler against libcutfemx_amd.so, run on the 2-D box case written to a file, and compared with the Python call on the
same arrays (the same bits) and with the closed form of the affine fields."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import advect_ref as A

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path):
    exe = tmp_path / "advect_facade"
    cmd = ["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/advect_facade.cpp"),
           "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
           f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.gpu
def test_cpp_advect_facade(oracle, tmp_path):
    import cutfemx_amd as cfx
    name, cfl = "box2", 2.5
    om = A.mesh(oracle, name)[0]
    phi, vel = A.fields(oracle, name, "affine")
    dt = A.time_step(oracle, name, "affine", cfl)
    path, out_path = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(np.array([om.tdim, om.x.shape[0], om.conn.shape[0]], dtype=np.int64).tobytes())
        f.write(np.array([dt], dtype=np.float64).tobytes())
        for a, dtype in ((om.x, np.float64), (om.conn, np.int32), (phi, np.float64), (vel, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dtype).tobytes())
    out = subprocess.run([str(_build(tmp_path)), str(path), str(out_path)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"located (\d+) outside (\d+) capped (\d+) skipped (\d+) steps (\d+) max_walk (\d+) boundary (\d+)", out)
    assert m, out
    mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
    fn = cfx.Function(cfx.FunctionSpace(mesh, 1), values=phi.copy())
    info = cfx.distance.advect(fn, vel.ravel().copy(), dt)
    assert tuple(int(g) for g in m.groups()[:6]) == (info.located, info.outside, info.capped, info.skipped, info.steps, info.max_walk)
    assert int(m.group(7)) == 4 * 16 and info.capped == 0 and info.outside > 0
    got = np.fromfile(out_path, dtype=np.float64)
    assert got.tobytes() == fn.values.tobytes()
    assert np.max(np.abs(got - A.affine_exact(om.x, om.tdim, dt, 2))) <= A.TOL * np.max(np.abs(phi))
