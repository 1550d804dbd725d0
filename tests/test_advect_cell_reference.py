"""One cell visit of the characteristic walk (cutfemx_amd/csrc/cfx_advect_cell.h) without a GPU: the header compiled as
plain host C++ with its own main (tests/cpp/advect_cell_host.cpp), under the address and undefined-behaviour sanitizers,
one process for the module, against the numpy model of tests/advect_ref.py in long double.

Cells: the Kuhn simplices of a cube, jittered ones, and ones squeezed to 1 : 1e3 (along an axis, and turned), in both
orientations.  Targets, given by their barycentric weights: the vertices, the midpoints of the edges, the centres of the
faces, the centre of the cell, points 1e-13 and 1e-9 outside every face, and points a few cell widths away."""
import itertools
import subprocess

import numpy as np
import pytest

import advect_ref as A
import reinit_cell_cases as C

ULP = 2.0 ** -52
TOL = A.INSIDE_TOL
KUHN = {2: [[0, 1, 3], [0, 3, 2]], 3: [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]}


def _turn(dim):
    if dim == 2:
        return np.array([[0.8, -0.6], [0.6, 0.8]])
    return np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])


def _weights(dim, rng):
    """(mu [m, nv], tag [m]) of the targets of one cell"""
    nv = dim + 1
    rows, tags = [], []
    eye = np.eye(nv)
    for i in range(nv):
        rows.append(eye[i]), tags.append("vertex")
    for i, j in itertools.combinations(range(nv), 2):
        rows.append(0.5 * (eye[i] + eye[j])), tags.append("edge")
    for i in range(nv):
        face = (1.0 - eye[i]) / dim
        if dim == 3:
            rows.append(face), tags.append("face")
        for delta, tag in ((1e-13, "out13"), (1e-9, "out9")):
            rows.append(face * (1.0 + delta) - delta * eye[i]), tags.append(tag)
    rows.append(np.full(nv, 1.0 / nv)), tags.append("centre")
    for _ in range(4):
        mu = rng.uniform(-3.0, 4.0, nv)
        mu[-1] = 1.0 - mu[:-1].sum()
        rows.append(mu), tags.append("far")
    return np.array(rows), np.array(tags)


def case_set(dim):
    """dict(X [n, nv, dim], P [n, dim], F [n, nv], kind [n], tag [n]): float64 arrays, made once"""
    def make():
        rng = np.random.default_rng(20 + dim)
        corners = np.array([[(i >> k) & 1 for k in range(dim)] for i in range(2 ** dim)], dtype=np.float64)
        kuhn = [corners[row] for row in KUHN[dim]]
        cells, kinds = [], []
        for X in kuhn:
            cells.append(0.125 * X + 0.25), kinds.append("kuhn")
            J = 0.125 * (X + rng.uniform(-0.2, 0.2, X.shape)) + 0.25
            cells.append(J), kinds.append("jittered")
            cells.append(J[rng.permutation(dim + 1)]), kinds.append("jittered")       # (the other orientation occurs too)
            S = J.copy()
            S[:, 1] *= 1e-3
            cells.append(S), kinds.append("squeezed")
            cells.append(S @ _turn(dim).T), kinds.append("squeezed-turned")
        Xs, Ps, kind, tag = [], [], [], []
        for X, k in zip(cells, kinds):
            mu, t = _weights(dim, rng)
            P = (mu.astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
            Xs.append(np.broadcast_to(X, (mu.shape[0],) + X.shape)), Ps.append(P)
            kind += [k] * mu.shape[0]
            tag += list(t)
        X = np.ascontiguousarray(np.concatenate(Xs))
        return dict(X=X, P=np.concatenate(Ps), F=rng.uniform(-1.0, 1.0, X.shape[:2]), kind=np.array(kind), tag=np.array(tag))
    return C.cached(("advect-cell", dim), make)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """{dim: (lam, value, D, facet)}: the program is compiled once, with the sanitizers, and run once per dimension"""
    work = tmp_path_factory.mktemp("advect_cell_host")
    exe = work / "advect_cell_host"
    cmd = [C.makefile_variable("HIPCC"), *C.makefile_variable("CXXFLAGS").split(), "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all",        # (the host side alone: nothing here is built for a GPU)
           str(C.ROOT / "tests" / "cpp" / "advect_cell_host.cpp"), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, "advect_cell_host.cpp does not compile:\n" + " ".join(cmd) + "\n" + done.stderr[-4000:]
    out = {}
    for dim in (2, 3):
        s = case_set(dim)
        n, nv = s["X"].shape[:2]
        with open(work / f"in{dim}.bin", "wb") as f:
            f.write(np.array([dim, n], dtype="<i8").tobytes() + np.array([TOL], dtype="<f8").tobytes())
            for a in (s["X"], s["P"], s["F"]):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
        run = subprocess.run([str(exe), str(work / f"in{dim}.bin"), str(work / f"out{dim}.bin")], capture_output=True, text=True, timeout=120.0)
        assert run.returncode == 0, f"advect_cell_host ended with status {run.returncode}: {run.stderr[-3000:]}"
        raw = (work / f"out{dim}.bin").read_bytes()
        sizes = [n * nv * 8, n * 8, n * dim * 8, n * 4]
        assert len(raw) == sum(sizes)
        cut = np.cumsum([0] + sizes)
        part = lambda k, dt: np.frombuffer(raw[cut[k]:cut[k + 1]], dtype=dt)
        out[dim] = (part(0, "<f8").reshape(n, nv), part(1, "<f8"), part(2, "<f8").reshape(n, dim), part(3, "<i4"))
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_lambda_against_long_double(host, dim):
    """lambda within 64 ulp of the long-double model times the cell's conditioning (1 for Kuhn and jittered cells, 1e3 for
    the squeezed ones), relative to max(1, |lambda|); the sum is 1 within 4 ulp of max(1, max |lambda|)"""
    s = case_set(dim)
    lam = host[dim][0]
    ld = np.longdouble
    ref = A.barycentric(s["X"].astype(ld), s["P"].astype(ld))
    size = np.maximum(1.0, np.max(np.abs(ref), axis=1).astype(np.float64))
    err = np.max(np.abs(lam.astype(ld) - ref), axis=1).astype(np.float64) / size
    cond = np.where(np.char.startswith(s["kind"], "squeezed"), 1e3, 1.0)
    for kind in np.unique(s["kind"]):
        print(f"dim {dim} {kind}: worst |lambda - long double| = {np.max(err[s['kind'] == kind]) / ULP:.1f} ulp of max(1, |lambda|)")
    assert np.all(err <= 64 * ULP * cond)
    total = np.abs(lam.astype(ld).sum(axis=1) - 1).astype(np.float64)
    print(f"dim {dim}: worst |sum lambda - 1| = {np.max(total / size) / ULP:.2f} ulp")
    assert np.all(total <= 4 * ULP * size)


@pytest.mark.parametrize("dim", [2, 3])
def test_inside_and_facet_are_the_models(host, dim):
    """'inside' is the long-double model's wherever its least lambda is not within 2e-13 of -inside_tol, and the facet is
    the model's wherever its two most negative lambda differ by more than 1e-10"""
    s = case_set(dim)
    facet = host[dim][3]
    ld = np.longdouble
    ref = A.barycentric(s["X"].astype(ld), s["P"].astype(ld))
    least = ref.min(axis=1).astype(np.float64)
    clear = np.abs(least + TOL) > 2e-13
    inside = least >= -TOL
    assert clear.mean() > 0.95
    assert np.array_equal(facet[clear] < 0, inside[clear])
    by_tag = {t: (facet[s["tag"] == t] < 0) for t in np.unique(s["tag"])}
    assert all(by_tag[t].all() for t in ("vertex", "edge", "centre", "out13") if t in by_tag)      # on the cell, or 1e-13 outside it
    assert not by_tag["out9"].any()                                                               # 1e-9 outside a face
    if dim == 3:
        assert by_tag["face"].all()
    order = np.sort(ref, axis=1)
    decided = ~inside & (facet >= 0) & ((order[:, 1] - order[:, 0]).astype(np.float64) > 1e-10)
    assert decided.sum() > 50
    assert np.array_equal(facet[decided], np.argmin(ref, axis=1)[decided])


@pytest.mark.parametrize("dim", [2, 3])
def test_the_float64_model_gives_the_same_bits(host, dim):
    """no contraction in the header: the numpy model in float64, which has the same operand order, agrees bit for bit --
    lambda, the facet, the interpolated value and the departure point.  The GPU tests' equal walks rest on this."""
    s = case_set(dim)
    lam, value, D, facet = host[dim]
    ref = A.barycentric(s["X"], s["P"])
    assert lam.tobytes() == ref.tobytes()
    model = [A.visit(s["X"][i], s["P"][i], TOL)[1] for i in range(ref.shape[0])]
    assert facet.tolist() == model
    assert value.tobytes() == np.array([A.interpolate(ref[i], s["F"][i]) for i in range(ref.shape[0])]).tobytes()
    assert D.tobytes() == (s["P"] - 0.375 * s["X"][:, 1, :]).tobytes()
