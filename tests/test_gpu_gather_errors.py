"""The error word of the row gathers: 1 = an entry of the form is not in the sparsity pattern it is assembled into.
The kernels skip the absent slot (nothing is written out of bounds) and the call raises; the engine stays usable."""
import numpy as np
import pytest

from helpers import level_set_values, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("deterministic", [False, True])
def test_an_entry_outside_the_pattern_is_reported_and_the_next_assembly_is_right(oracle, deterministic, monkeypatch):
    """3-D P1 on the 4^3 Kuhn box cut by the sphere.  a_small: the stiffness on the inside and cut cells; a_big: the
    same plus the gradient jump on the cut band's facets, whose macro rows couple the opposite vertices of two
    facet-sharing tets -- vertices that share no cell, so a_small's pattern has no entry for them."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    if deterministic:
        monkeypatch.setenv("CFX_DETERMINISTIC", "1")
    O, tdim, n = oracle, 3, 4
    om = O.mesh_box(tdim, n)
    phi = level_set_values(om.x, tdim)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    inside = cfx.locate_entities_device(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 2)
    ghost = cfx.ghost_penalty_facets(cd, "phi<0")
    assert ghost.size > 0
    stiffness = lambda: fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=0)
    a_small = fem.form([stiffness()], V)
    a_big = fem.form([stiffness(), fem.Integral(fem.GHOST_GRADJUMP, facets=ghost, params=(0.1,), qdegree=0)], V)

    A_small = fem.create_matrix(a_small)
    assert fem.create_matrix(a_big).nnz > A_small.nnz
    with pytest.raises(RuntimeError, match="not in the sparsity pattern"):
        fem.assemble_matrix(a_big, A=A_small)

    d = O.classify(om.conn, phi)
    oV = O.Space(om.conn, om.nnodes, 1)
    oi = [O.Integral(O.CELL, O.K_STIFFNESS, entities=O.locate_entities(d, "phi<0"),
                     rules=O.runtime_quadrature(om, om.conn, phi, d, "phi<0", 2), qdegree=0),
          O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=O.ghost_penalty_facets(om, d, "phi<0"),
                     params=(0.1,), qdegree=0)]
    ip, ix = O.create_sparsity(om, oV, oi)
    A = fem.assemble_matrix(a_big)
    assert np.array_equal(A.indptr, ip) and np.array_equal(A.indices, ix)
    assert rel_err(A.data, O.assemble_matrix(om, oV, oi, ip, ix)) < 1e-12
