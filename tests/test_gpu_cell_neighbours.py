"""Mesh.cell_neighbours() -- the mesh-static cell -> cell table the characteristic walk of distance.advect crosses facets
with -- against the dictionary of facets of tests/advect_ref.py, entry for entry: the table is unique."""
import numpy as np
import pytest

import advect_ref as A
import helpers as H

pytestmark = pytest.mark.gpu


def _mesh(oracle, name):
    if name == "box2":
        return oracle.mesh_box(2, 4)
    if name == "box3":
        return oracle.mesh_box(3, 4)
    if name == "scrambled3":
        return H.scrambled_mesh(oracle, 3, 8)
    if name == "cone3":
        return H.cone_mesh(3, (8, 8))                       # each apex in 128 cells
    return H.high_valence_case(oracle, 3, (8, 8))[0]        # the cone and a box, disjoint


@pytest.mark.parametrize("name", ["box2", "box3", "scrambled3", "cone3", "union3"])
def test_table_equals_the_model(oracle, name):
    import cutfemx_amd as cfx
    om = _mesh(oracle, name)
    mesh = cfx.Mesh.from_arrays(om.tdim, om.x, om.conn)
    got = mesh.cell_neighbours()
    want = A.neighbours(om.conn)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(mesh.cell_neighbours(), want)      # the second call returns the table built by the first
    boundary = int(np.count_nonzero(got < 0))
    if name == "box2":
        assert boundary == 4 * 4
    if name == "box3":
        assert boundary == 12 * 4 * 4
    if name == "cone3":
        apex = om.nnodes - 2
        assert int(np.count_nonzero(np.any(om.conn == apex, axis=1))) == 128


def test_generated_box_and_static_bytes():
    """the box generated in HBM has the table of the same arrays given by the caller, and a space lists its bytes"""
    import cutfemx_amd as cfx
    mesh = cfx.Mesh.create_box(3, 4)
    V = cfx.FunctionSpace(mesh, 1)
    before = V.static_table_bytes()["cell_neighbours"]
    got = mesh.cell_neighbours()
    assert np.array_equal(got, A.neighbours(mesh.conn))
    assert int(np.count_nonzero(got < 0)) == 12 * 4 * 4
    assert before == 0 and V.static_table_bytes()["cell_neighbours"] >= 16 * mesh.num_cells
