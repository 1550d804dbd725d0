"""The cell-local arithmetic of the reinitialisation (cutfemx_amd/csrc/cfx_reinit_cell.h) without a GPU.

First the independent references of tests/reinit_exact.py are pinned to mathematics: the long-double minimiser against
an mpmath minimiser and against plane waves whose ray meets the face in its interior, on an edge and at a vertex; the
exact near field against planes and hand-made cells with rational answers.  Then the header, compiled as plain host C++
(tests/cpp/reinit_cell_host.cpp, one process for the module), and the numpy model (tests/reinit_ref.py) meet the cases
and assertions of tests/reinit_cell_cases.py -- the same ones tests/test_gpu_reinit_cell.py applies to the GPU."""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import reinit_cell_cases as C
import reinit_exact as E


# ---- the references -----------------------------------------------------------------------------------------------------
def test_brute_update_against_mpmath():
    """a sample of every kind of set, flat cells included: 2e-15 L, and the rounding of a long double at the size of the
    values, is what the search may leave"""
    worst = 0.0
    for name, count in (("well3", 3), ("boundary3", 1), ("flat3", 4), ("well2", 2), ("flat2", 2)):
        s, (ref, _) = C.UPDATE_SETS[name](), C.brute(name)
        rows = np.nonzero(s["ok"].all(axis=1))[0]
        rows = rows[np.random.default_rng(5).choice(rows.size, count, replace=False)]
        for i in rows:
            want = E.mp_update(s["P"][i], s["dv"][i])
            with mp.workdps(40):                            # (a long double is the sum of two doubles)
                got = mp.mpf(float(ref[i])) + mp.mpf(float(ref[i] - np.longdouble(float(ref[i]))))
                err = float(abs(got - want)) / C.length(s["P"][i:i + 1])[0]
            worst = max(worst, err)
            assert err <= 2e-15 + 2.0 ** -62 * np.max(np.abs(s["dv"][i])) / C.length(s["P"][i:i + 1])[0], (name, i, s["tag"][i], err)
    print(f"brute_update against mpmath: worst {worst:.2e} L")


@pytest.mark.parametrize("dim", [2, 3])
def test_brute_update_against_plane_waves(dim):
    """d = n . x + c on the sources, the target on the ray y + s n from a point y of the face: U = n . x_t + c exactly,
    with y in the interior, on an edge (3-D) and at a vertex"""
    rng = np.random.default_rng([7, dim])
    spots = {"interior": np.full(dim, 1.0 / dim), "vertex": np.eye(dim)[0]}
    if dim == 3:
        spots["edge"] = np.array([0.0, 0.4, 0.6])
    for spot, lam in spots.items():
        m = 40
        X = C._well_shaped(rng, m, dim)
        y = np.einsum("i,mik->mk", lam, X)
        if dim == 3:
            nf = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        else:
            e = X[:, 1] - X[:, 0]
            nf = np.stack([-e[:, 1], e[:, 0]], axis=1)
        nf /= np.linalg.norm(nf, axis=1)[:, None]
        n = nf + 0.7 * C._unit(rng, m, dim)
        n /= np.linalg.norm(n, axis=1)[:, None]
        t = y + rng.uniform(0.2, 2.0, m)[:, None] * n
        c = 3.0
        U = E.brute_update(X - t[:, None, :], np.einsum("mik,mk->mi", X, n) + c, np.ones((m, dim), dtype=bool))
        err = np.abs((U - (np.einsum("mk,mk->m", t, n) + c)).astype(np.float64))
        print(f"plane wave through the {spot} of the face, {dim}-D: worst {err.max():.2e}")
        assert np.all(err <= 1e-14)                         # (the inputs are rounded: d, P and n . x_t to 1 ulp each)


def test_brute_update_masks():
    """a source that is not usable plays no part; none usable: inf"""
    s = C.well_shaped_set(3)
    P, dv = s["P"][:8], s["dv"][:8]
    ok = np.array([[True, False, True]] * 8)
    full = E.brute_update(P, dv, ok)
    assert np.array_equal(full, E.brute_update(P[:, [0, 2]], dv[:, [0, 2]], np.ones((8, 2), dtype=bool)))
    assert np.all(E.brute_update(P, dv, np.zeros((8, 3), dtype=bool)) == E.INF)


def test_exact_seed_against_planes():
    """phi = a (n . x - c) with an integer n: every vertex's distance is |n . x - c| / |n| when the foot of its
    perpendicular falls into the cell's piece, and never less"""
    rng = np.random.default_rng(11)
    hit = 0
    for dim in (2, 3):
        for _ in range(100):
            X = rng.integers(-8, 9, size=(dim + 1, dim)) / 4.0
            if abs(np.linalg.det(X[1:] - X[0])) < 0.1:
                continue
            n = rng.integers(-3, 4, size=dim).astype(float)
            if not n.any():
                continue
            c = float(rng.integers(-8, 9)) / 8.0
            f = -1.75 * (X @ n - c)
            flag, dist = E.exact_seed(X, f)
            if not flag:
                assert np.all(f >= 0) or np.all(f < 0)
                continue
            plane = np.abs(X @ n - c) / np.linalg.norm(n)
            assert np.all(dist >= plane - 1e-15)
            # the foot of the perpendicular of vertex i lies in the cell iff its barycentric coordinates are >= 0
            for i in range(dim + 1):
                foot = X[i] - (X[i] @ n - c) / (n @ n) * n
                lam = np.linalg.solve(np.vstack([X.T, np.ones(dim + 1)]), np.append(foot, 1.0))
                if np.all(lam >= 1e-9):
                    hit += 1
                    assert abs(dist[i] - plane[i]) <= 1e-15
    assert hit >= 30


def test_exact_seed_hand_made_cells():
    ULP2 = 2.3e-16                                          # (the expected values are rounded doubles themselves)
    unit = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    # one vertex cut off at half of every edge: the piece is the triangle (1/2,0,0), (0,1/2,0), (0,0,1/2), in the plane
    # x + y + z = 1/2; the origin's foot is its centroid, the other vertices' feet fall outside: their nearest points
    # are the piece's corners, at distance 1/2
    flag, d = E.exact_seed(unit, [-1.0, 1.0, 1.0, 1.0])
    assert flag and np.allclose(d, [0.5 / np.sqrt(3.0), 0.5, 0.5, 0.5], rtol=0, atol=ULP2)
    # two and two, cut at half: the rectangle 0 <= z <= 1/2 of the plane x + y = 1/2 between x = 0 and y = 0
    flag, d = E.exact_seed(unit, [-1.0, 1.0, 1.0, -1.0])
    pts = np.array([[0.5, 0, 0], [0, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])    # crossings of 0-1, 0-2, 3-1, 3-2
    assert flag
    # the origin's foot (1/4,1/4,0) lies on the piece's edge: distance sqrt(1/8); the foot of (0,0,1) is 1/2 above the
    # piece: sqrt(1/8 + 1/4)
    assert abs(d[0] - np.sqrt(0.125)) <= ULP2 and abs(d[3] - np.sqrt(0.375)) <= ULP2
    # vertex 1 = (1,0,0): foot (3/4,-1/4,0) is outside, the nearest point is the corner (1/2,0,0)
    assert abs(d[1] - 0.5) <= ULP2 and abs(d[2] - 0.5) <= ULP2
    assert np.all(d <= np.min(np.linalg.norm(np.array(unit, dtype=float)[:, None, :] - pts[None], axis=2), axis=1) + ULP2)
    # zeros: (-, 0, 0, 0) is a seed cell whose piece is the face of the zeros; (0, 0, 0, +) and (-0.0, ...) are none
    flag, d = E.exact_seed(unit, [-1.0, 0.0, 0.0, -0.0])
    assert flag and abs(d[0] - 1 / np.sqrt(3.0)) <= ULP2 and np.all(d[1:] == 0.0)
    assert not E.exact_seed(unit, [0.0, -0.0, 0.0, 2.0])[0]
    # 2-D: the segment from (1/4, 0) to (0, 3/4)
    flag, d = E.exact_seed([[0, 0], [1, 0], [0, 1]], [-1.0, 3.0, 1.0 / 3.0])
    assert flag
    a, b = np.array([0.25, 0.0]), np.array([0.0, 1.0 / (1.0 + 1.0 / 3.0)])
    line = abs(a[0] * b[1]) / np.linalg.norm(b - a)
    assert abs(d[0] - line) <= 1e-15 and abs(d[1] - 0.75) <= 1e-15
    # the distance of a point to a triangle, region by region, on the 3-4-5 grid
    tri = [[Fraction(0), Fraction(0), Fraction(0)], [Fraction(4), Fraction(0), Fraction(0)], [Fraction(0), Fraction(3), Fraction(0)]]
    for p, want2 in (((1, 1, 2), 4), ((-1, -1, 0), 2), ((5, -1, 1), 3), ((2, -3, 0), 9), ((-2, 1, 0), 4), ((-1, 5, 0), 5),
                     ((4, 3, 0), Fraction(144, 25)), ((4, 3, 1), Fraction(169, 25))):
        assert E._triangle_dist2([Fraction(v) for v in p], *tri) == want2, p


# ---- the header on the CPU, and the model -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{"host": (updates, seeds), "model": ...}; the host program is compiled and started once"""
    work = tmp_path_factory.mktemp("reinit_cell_host")
    exe = C.compile_program("reinit_cell_host.cpp", work / "reinit_cell_host", offload=False)
    host = C.run_program(exe, work)
    model = ({name: C.model_update(name) for name in C.UPDATE_SETS}, {dim: C.model_seed(dim) for dim in (2, 3)})
    return {"host": host, "model": model}


@pytest.mark.parametrize("who", ["host", "model"])
@pytest.mark.parametrize("name", ["well3", "well2", "boundary3", "boundary2"])
def test_update_well_shaped_and_boundary(results, who, name):
    C.check_tight(name, results[who][0][name], who)


@pytest.mark.parametrize("who", ["host", "model"])
@pytest.mark.parametrize("name", ["flat3", "flat2"])
def test_update_graded_flatness(results, who, name):
    C.check_flat(name, results[who][0][name], who)


@pytest.mark.parametrize("who", ["host", "model"])
@pytest.mark.parametrize("dim", [2, 3])
def test_near_field(results, who, dim):
    C.check_seed(dim, *results[who][1][dim], who)


def test_error_table(results):
    for name in ("flat3", "flat2"):
        print(C.error_table(name, {who: results[who][0][name] for who in ("host", "model")}))


def test_the_thresholds_are_in_step():
    import re
    import reinit_ref as R
    header = (C.CSRC / "cfx_reinit_cell.h").read_text()
    assert float(re.search(r"kDegenerate = ([0-9.e+-]+);", header)[1]) == R.DEGENERATE
    assert float(re.search(r"kFlatPiece = ([0-9.e+-]+);", header)[1]) == R.FLAT_PIECE
    assert R.DEGENERATE <= 2.5e-9
