"""distance::extend_normal_velocity of the C++ facade (include/cutfemx_amd.hpp): tests/cpp/extension_facade.cpp compiled
with the host compiler against libcutfemx_amd.so, run on the 2-D plane case written to a file, and compared with the
Python call on the same arrays (the same bits) and with the plane's exact answer."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import extension_ref as X

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path):
    exe = tmp_path / "extension_facade"
    cmd = ["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/extension_facade.cpp"),
           "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
           f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.gpu
def test_cpp_extension_facade(oracle, tmp_path):
    import cutfemx_amd as cfx
    c = X.case(oracle, "plane2")
    om, phi, w = c["mesh"], c["phi"], c["w"]
    nv = phi.size
    path, out_path = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(np.array([om.tdim, om.x.shape[0], om.conn.shape[0]], dtype=np.int64).tobytes())
        for a, dt in ((om.x, np.float64), (om.conn, np.int32), (phi, np.float64), (w, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([str(_build(tmp_path)), str(path), str(out_path)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"reason (\d+) sweeps (\d+) seeds (\d+) updates (\d+) transport_sweeps (\d+) transported (\d+)", out)
    assert m, out
    mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
    res = cfx.distance.extend_normal_velocity(cfx.Function(cfx.FunctionSpace(mesh, 1), values=phi.copy()), w.copy())
    info = res.info
    assert tuple(int(g) for g in m.groups()) == (info.reason, info.sweeps, info.seeds, info.updates, info.transport_sweeps, info.transported)
    assert info.reason == cfx.distance.REINIT_CONVERGED
    got = np.fromfile(out_path, dtype=np.float64)
    speed, velocity, dist = got[:nv], got[nv:3 * nv].reshape(nv, 2), got[3 * nv:]
    assert np.array_equal(speed, res.speed.values) and np.array_equal(velocity.ravel(), res.velocity.values)
    assert np.array_equal(dist, res.signed_distance.values)
    exact, Fx, a = X.plane_exact("plane2", om.x)
    clean = np.abs(np.abs(dist) - exact) <= 1e-13
    assert clean.mean() >= 0.45
    assert np.max(np.abs(speed - Fx)[clean]) <= 1e-13
    assert np.max(np.abs(velocity - Fx[:, None] * a)[clean]) <= 4e-13      # (|F| <= 2.4 times 1e-13 for n, and 1e-13 for F)
