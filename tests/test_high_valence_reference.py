"""The high-valence meshes of test_gpu_high_valence.py, pinned with the CPU oracle alone: the builders (helpers.cone_mesh,
mesh_union, high_valence_case) must keep producing the stencil and row lengths that the GPU cases are chosen for -- a
builder that drifted would leave the GPU file green while it tests other kernel classes than it says."""
import numpy as np
import pytest

from helpers import (HIGH_VALENCE_P1, HIGH_VALENCE_P2, cone_mesh, high_valence_case, mesh_union, oracle_poisson,
                     oracle_stiffness_source)


def _stencil(conn, v):
    return np.unique(conn[np.any(conn == v, axis=1)])


def _row(ref, r):
    return ref["indices"][ref["indptr"][r]:ref["indptr"][r + 1]]


def test_cone_and_union_builders(oracle):
    for tdim, shape, ncells, nb in ((2, 5, 10, 6), (3, (2, 3), 24, 12), (3, 3, 36, 16)):
        c = cone_mesh(tdim, shape)
        assert c.ncells == ncells and c.nnodes == nb + 2 and c.conn.shape[1] == tdim + 1
        assert np.all(c.x[:nb, tdim - 1] == 0.5) and c.x[:nb, :tdim - 1].min() == 0.0 and c.x[:nb, :tdim - 1].max() == 1.0
        assert np.array_equal(c.x[nb, :tdim], [0.5] * (tdim - 1) + [0.0]) and np.array_equal(c.x[nb + 1, :tdim], [0.45] * (tdim - 1) + [1.0])
        assert np.all(c.conn[:ncells // 2, tdim] == nb) and np.all(c.conn[ncells // 2:, tdim] == nb + 1)
        assert np.array_equal(c.conn[:ncells // 2, :tdim], c.conn[ncells // 2:, :tdim])      # every base cell, to each apex
        assert len(np.unique(np.sort(c.conn[:ncells // 2, :tdim], axis=1), axis=0)) == ncells // 2
        vol = oracle.cell_volumes(c)
        assert np.all(vol > 0) and abs(vol.sum() - (0.5 if tdim == 2 else 1.0 / 3.0)) < 1e-14   # two cones of height 0.5
        box = oracle.mesh_box(tdim, 2)
        u = mesh_union(c, box, 2.0)
        assert u.ncells == c.ncells + box.ncells and u.nnodes == c.nnodes + box.nnodes
        assert np.array_equal(u.conn[:c.ncells], c.conn) and np.array_equal(u.conn[c.ncells:], box.conn + c.nnodes)
        assert np.array_equal(u.x[:c.nnodes], c.x) and np.array_equal(u.x[c.nnodes:], box.x + np.array([2.0, 0.0, 0.0]))
        assert np.array_equal(mesh_union(c, box, [2.0, 0.0, 0.0]).x, u.x)


@pytest.mark.parametrize("tdim,shape", list(HIGH_VALENCE_P1), ids=lambda v: str(v).replace(" ", ""))
def test_p1_shapes(oracle, tdim, shape):
    O = oracle
    apex_len, poisson_len, stiffness_len = HIGH_VALENCE_P1[(tdim, shape)]
    om, phi, info = high_valence_case(O, tdim, shape)
    nb = info["nbase"]
    assert nb == (shape + 1 if tdim == 2 else (shape[0] + 1) * (shape[1] + 1)) and apex_len == nb + 1
    for apex in (info["lower_apex"], info["upper_apex"]):
        st = _stencil(om.conn, apex)
        assert len(st) == apex_len and np.array_equal(st, np.r_[np.arange(nb), apex])
    assert max(len(_stencil(om.conn, v)) for v in range(nb)) <= 9                  # base vertices keep short rows
    a, b = oracle_poisson(O, om, phi), oracle_stiffness_source(O, om, phi)
    assert int(np.diff(a["indptr"]).max()) == poisson_len
    assert int(np.diff(b["indptr"]).max()) == stiffness_len
    dom = a["domain"]
    assert np.all(dom[info["lower_cells"]] == -1) and np.all(dom[info["upper_cells"]] == 0)
    assert set(dom[info["box_cells"]].tolist()) == {-1, 0, 1}
    assert phi[info["upper_apex"]] > 0 and np.all(phi[:nb + 1] < 0) and np.all(phi != 0.0)
    # with the ghost penalty both apex rows hold the base and each other; without it the lower apex is a vertex of no cut
    # cell -- every cell around it is inside -- and its row is its complete static stencil: a plain long row
    both = np.r_[np.arange(nb + 2)]
    assert np.array_equal(_row(a, info["lower_apex"]), both) and np.array_equal(_row(a, info["upper_apex"]), both)
    cut_vertices = np.unique(om.conn[dom == 0])
    assert info["lower_apex"] not in cut_vertices
    assert np.all(dom[np.any(om.conn == info["lower_apex"], axis=1)] == -1)
    assert np.array_equal(_row(b, info["lower_apex"]), _stencil(om.conn, info["lower_apex"]))
    assert np.array_equal(_row(b, info["upper_apex"]), [info["upper_apex"]])       # outside the form: its diagonal alone
    assert np.all(np.isfinite(a["values"])) and np.all(np.isfinite(b["values"])) and np.all(np.isfinite(a["b"]))


@pytest.mark.parametrize("m", list(HIGH_VALENCE_P2))
def test_p2_shapes(oracle, m):
    import cutfemx_amd as cfx
    O = oracle
    om, phi, info = high_valence_case(O, 3, (m, m))
    dofmap, ndofs = cfx.lagrange_dofmap(3, om.conn, om.nnodes, 2)
    a = oracle_poisson(O, om, phi, degree=2, dofmap=dofmap, ndofs=ndofs)
    b = oracle_stiffness_source(O, om, phi, degree=2, dofmap=dofmap, ndofs=ndofs)
    assert (int(np.diff(a["indptr"]).max()), int(np.diff(b["indptr"]).max())) == HIGH_VALENCE_P2[m]
    # the static degree-2 list of an apex: itself, the base vertices, its edges to them, the base's edges
    apex_list = np.unique(dofmap[np.any(om.conn == info["lower_apex"], axis=1)])
    nb = info["nbase"]
    base_edges = 2 * m * (m + 1) + m * m
    assert len(apex_list) == 1 + 2 * nb + base_edges
    assert np.array_equal(_row(b, info["lower_apex"]), apex_list)
    if m >= 3:
        assert len(apex_list) == HIGH_VALENCE_P2[m][1]
    assert np.all(np.isfinite(a["values"])) and np.all(np.isfinite(b["values"]))
