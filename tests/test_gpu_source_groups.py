"""The P1 series source term by hex (cfx_mesh_s::hex_groups, vec_source_groups_kernel): b against the oracle on the
meshes where the group path is taken, against the per-cell path (CFX_SOURCE_GROUPS=0), bit for bit between two runs,
and the per-cell path on a mesh that is not made of Kuhn hexes in order."""
import os

import numpy as np
import pytest

from helpers import groups_expected, level_set_values, oracle_poisson, profiled, rel_err, scrambled_mesh

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _system(mesh, phi):
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    return poisson.build_forms(V, cd, order=4)


def _b(sysm):
    import cutfemx_amd as cfx
    return profiled(lambda: cfx.fem.assemble_vector(sysm.L))


def _check(O, om, mesh, phi, grouped):
    ref = oracle_poisson(O, om, phi, order=4)
    sysm = _system(mesh, phi)
    b, names = _b(sysm)
    assert rel_err(b, ref["b"]) < RTOL
    grouped = grouped and groups_expected()          # (the diagnostic modes take the cell path: same values)
    assert ("source_groups" in names) == grouped, " ".join(sorted(names))
    if grouped:
        assert "vec_tensors_std" in names and "assemble_vec_plain" in names, " ".join(sorted(names))
    return sysm, b


@pytest.mark.parametrize("n", [16, 23, 32])
def test_groups_box(oracle, n):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, n)
    _check(oracle, om, cfx.Mesh.create_box(3, n), level_set_values(om.x, 3, "sphere"), True)


def test_groups_from_arrays(oracle):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 18)
    _check(oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), level_set_values(om.x, 3, "sphere"), True)


def test_groups_inside_touches_boundary(oracle):
    # the inside reaches the box faces: rows there lack corner slots
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 20)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.0, 0.1, 0.0]), axis=1) - 0.7
    _check(oracle, om, cfx.Mesh.create_box(3, 20), phi, True)


def test_scrambled_takes_cell_path(oracle):
    import cutfemx_amd as cfx
    om = scrambled_mesh(oracle, 3, 16)
    _check(oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), level_set_values(om.x, 3, "sphere"), False)


def test_groups_match_cell_path_and_repeat(oracle, monkeypatch):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 20)
    phi = level_set_values(om.x, 3, "sphere")
    sysm = _system(cfx.Mesh.create_box(3, 20), phi)
    b1, n1 = _b(sysm)
    b2, _ = _b(sysm)
    want = groups_expected()                           # (the mode of the run, before the switch below)
    assert ("source_groups" in n1) == want
    if os.environ.get("CFX_ASSEMBLY") == "atomic":      # (FP64 atomics: the order of the sums is the schedule's)
        assert rel_err(b1, b2) < 1e-13
    else:
        assert np.array_equal(b1, b2)                  # fixed summation order: bit for bit
    monkeypatch.setenv("CFX_SOURCE_GROUPS", "0")
    b0, n0 = _b(sysm)
    assert "source_groups" not in n0 and ("vec_tensors_std" in n0 or not want)
    assert rel_err(b1, b0) < 1e-13
