"""The numpy model of the advection (tests/advect_ref.py) against what does not depend on it: the closed forms of affine
fields, a brute-force locator, and its own long-double run.  The GPU tests (tests/test_gpu_advect.py) compare the engine
with this model on the same cases; here the model alone is shown to hold the conditions those tests rest on: no capped
vertex, an empty grey zone, and every branch of the walk reached."""
import numpy as np
import pytest

import advect_ref as A

RUNS = [(name, cfl) for name, cfls in A.CASES.items() for cfl in cfls]


def test_neighbours_of_two_triangles_and_boundary_counts(oracle):
    conn = oracle.mesh_box(2, 1).conn
    assert conn.tolist() == [[0, 1, 3], [0, 3, 2]]
    assert A.neighbours(conn).tolist() == [[-1, 1, -1], [-1, -1, 0]]
    for tdim, n, boundary in ((2, 4, 4 * 4), (3, 4, 12 * 4 * 4)):
        om = oracle.mesh_box(tdim, n)
        nbr = A.neighbours(om.conn)
        assert int(np.count_nonzero(nbr < 0)) == boundary
        c, i = np.nonzero(nbr >= 0)
        back = nbr[nbr[c, i]]
        assert np.all(np.any(back == c[:, None], axis=1))              # the neighbour names the cell back
        shared = [len(set(om.conn[a]) & set(om.conn[b])) for a, b in zip(c[:50], nbr[c, i][:50])]
        assert set(shared) == {tdim}
        assert all(om.conn[a, j] not in om.conn[b] for a, j, b in zip(c[:50], i[:50], nbr[c, i][:50]))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name,cfl", RUNS)
def test_affine_fields_are_exact(oracle, name, cfl, order):
    """the P1 extension reproduces affine fields: the closed form holds inside, outside and far beyond the mesh"""
    om = A.mesh(oracle, name)[0]
    m = A.model(oracle, name, "affine", cfl, order)
    exact = A.affine_exact(om.x, om.tdim, A.time_step(oracle, name, "affine", cfl), order)
    scale = float(np.max(np.abs(A.fields(oracle, name, "affine")[0])))
    err = float(np.max(np.abs(m["out"] - exact))) / scale
    print(f"{name} CFL {cfl} order {order}: |model - closed form| / max|phi| = {err:.1e}; located {m['located']} outside {m['outside']} "
          f"steps {m['steps']} max_walk {m['max_walk']}")
    assert m["capped"] == 0 and m["skipped"] == 0 and m["located"] + m["outside"] == om.x.shape[0]
    assert err <= A.TOL


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name,cfl", RUNS)
def test_walk_agrees_with_the_brute_force_locator(oracle, name, cfl, order):
    om, nbr, _ = A.mesh(oracle, name)
    phi, _ = A.fields(oracle, name, "sphere")
    m = A.model(oracle, name, "sphere", cfl, order)
    assert m["capped"] == 0
    cell, best, lam = A.brute_locate(om.x, om.conn, m["dep"])
    moved = cell >= 0                                                 # (every vertex here: the rotation has no fixed vertex)
    assert moved.all() and A.grey_count(best) == 0
    inside = best >= -A.INSIDE_TOL
    assert np.array_equal(inside, m["status"] == A.LOCATED) and np.array_equal(~inside, m["status"] == A.OUTSIDE)
    if order == 2:
        _, best_half, _ = A.brute_locate(om.x, om.conn, m["half"])
        assert A.grey_count(best_half) == 0
    value = np.einsum("mi,mi->m", lam, phi[om.conn[cell]].astype(np.longdouble))
    scale = float(np.max(np.abs(phi)))
    err = float(np.max(np.abs(m["out"][inside] - value[inside]))) / scale
    print(f"{name} CFL {cfl} order {order}: {int(inside.sum())} inside, |walk - brute force| / max|phi| = {err:.1e}")
    assert err <= A.TOL
    # an outside vertex ended in a cell with a boundary facet, and carries that cell's P1 extension
    out = np.nonzero(~inside)[0]
    assert np.all(np.any(nbr[m["cells"][out]] < 0, axis=1))
    X = om.x[om.conn[m["cells"][out]]][:, :, :om.tdim].astype(np.longdouble)
    ext = np.einsum("mi,mi->m", A.barycentric(X, m["dep"][out].astype(np.longdouble)), phi[om.conn[m["cells"][out]]].astype(np.longdouble))
    assert out.size == 0 or float(np.max(np.abs(m["out"][out] - ext))) / scale <= A.TOL


def test_every_branch_is_reached(oracle):
    """the figures of the issue: walks of 4 to 34 crossings at the largest CFL, hundreds of vertices leave the 3-D boxes"""
    longest, left = {}, {}
    for name, cfls in A.CASES.items():
        m = A.model(oracle, name, "affine", cfls[-1], 2)
        longest[name], left[name] = m["max_walk"], m["outside"]
    print(f"longest walks {longest}, outside {left}")
    assert all(4 <= w <= 40 for w in longest.values())
    assert left["box3"] >= 200 and left["scrambled3"] >= 200 and all(v > 0 for v in left.values())
    small = A.model(oracle, "box3", "affine", 0.3, 2)
    assert small["located"] > small["outside"] > 0


def test_noise_floor(oracle):
    """float64 against long double on every case: what 'equal' means for a result that is not compared bit for bit"""
    worst = {}
    for name, cfl in RUNS:
        for field in ("affine", "sphere"):
            for order in (1, 2):
                a = A.model(oracle, name, field, cfl, order)
                b = A.model(oracle, name, field, cfl, order, dtype=np.longdouble)
                assert np.array_equal(a["status"], b["status"])
                scale = float(np.max(np.abs(A.fields(oracle, name, field)[0])))
                # (an outside vertex of a curved phi carries the extension of ITS boundary cell: compared where the two
                # runs left through the same one)
                rows = (a["status"] == A.LOCATED) | (a["cells"] == b["cells"])
                assert rows.mean() > 0.9
                worst[(name, cfl, field, order)] = float(np.max(np.abs(a["out"].astype(np.longdouble) - b["out"])[rows])) / scale
    top = max(worst, key=worst.get)
    per_mesh = {n: max(v for k, v in worst.items() if k[0] == n) for n in A.CASES}
    print(f"noise floors per mesh {({k: f'{v:.1e}' for k, v in per_mesh.items()})}; largest at {top}: {worst[top]:.2e}")
    assert worst[top] <= A.FLOOR
    assert A.TOL <= 1e-11
