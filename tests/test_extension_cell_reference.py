"""The cell-local arithmetic of the normal extension (cell_update_argmin and seed_closest of
cutfemx_amd/csrc/cfx_reinit_cell.h) without a GPU: the header compiled as plain host C++
(tests/cpp/extension_cell_host.cpp, one process for the module) on the case sets of tests/reinit_cell_cases.py, against
the long-double references of tests/reinit_exact.py.  "Where" must agree with "how far": the place reported for a minimum,
put back into the function that is minimised, gives the minimum."""
import numpy as np
import pytest

import reinit_cell_cases as C

ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """(updates, seeds, directory): the program is compiled and started once"""
    work = tmp_path_factory.mktemp("extension_cell_host")
    exe = C.compile_program("extension_cell_host.cpp", work / "extension_cell_host", offload=False)
    updates, seeds = C.run_program(exe, work)
    return updates, seeds, work


def _out(work, name, tag, shape=(-1,)):
    return np.fromfile(work / f"{name}.{tag}.out", dtype="<f8").reshape(shape)


@pytest.mark.parametrize("name", list(C.UPDATE_SETS))
def test_argmin_value_is_the_update(host, name):
    """the same U bits as cell_update, and the reported sub-face's own value is U (limit -infinity: the one that attains it)"""
    updates, _, work = host
    U, Uref, value = updates[name], _out(work, name, "Uref"), _out(work, name, "value")
    assert U.tobytes() == Uref.tobytes()
    assert value.tobytes() == U.tobytes()


@pytest.mark.parametrize("name", list(C.UPDATE_SETS))
def test_argmin_weights(host, name):
    """weights >= 0 that sum to 1 within 4 ulp; sum lambda d + |sum lambda P| in long double gives the minimum back.

    The bound is 1e-14 L beside 4 ulp of the largest |d|: weights that sum to 1 within 4 ulp move sum lambda d by that
    much, whatever the minimiser (the sets carry offsets of up to 1e6 L).  The reference is the minimum over the hull of
    the usable sources where the engine takes the face of three sources as it is, and the least over the sub-faces of one
    and two sources where it declares the face degenerate -- as in reinit_cell_cases.check_flat."""
    updates, _, work = host
    s, (full, sub) = C.UPDATE_SETS[name](), C.brute(name)
    k = s["P"].shape[1]
    U, lam = updates[name], _out(work, name, "lam", (-1, k))
    some = U < C.INF
    assert np.array_equal(some, s["ok"].any(axis=1))
    assert np.all(lam[~some] == 0.0)
    lam, P, dv, ok = lam[some], s["P"][some], s["dv"][some], s["ok"][some]
    assert np.all(lam >= 0.0) and np.all(lam[~ok] == 0.0)
    assert np.max(np.abs(lam.sum(axis=1) - 1.0)) <= 4 * ULP
    L = C.length(s["P"])[some]
    ld = np.longdouble
    again = np.einsum("mi,mi->m", lam.astype(ld), dv.astype(ld)) + np.sqrt(np.sum(np.einsum("mi,mik->mk", lam.astype(ld), P.astype(ld)) ** 2, axis=1))
    degenerate = C.kernel_degenerate(s["P"])[some] if k == 3 else np.all(s["P"][some][:, 0] == s["P"][some][:, 1], axis=1)
    ref = np.where(degenerate, sub[some], full[some])
    err = ((again - ref) / L).astype(np.float64)
    bound = 1e-14 + 4.0 * C.ulp_of_values(dv) / L
    print(f"{name}: {int(some.sum())} cases, value at the reported minimiser - reference in [{err.min():+.2e}, {err.max():+.2e}] L, "
          f"worst against its bound {np.max(np.abs(err) / bound):.3f}")
    bad = np.abs(err) > bound
    assert not bad.any(), C._worst(err[bad], s["tag"][some][bad], "beyond the bound")


@pytest.mark.parametrize("dim", [2, 3])
def test_closest_point_weights(host, dim):
    """seed_closest's distance is seed_cell's within 4 ulp of L, its weights are >= 0 and sum to 1 within 4 ulp, and the
    point they name lies at that distance from the vertex (in long double) within 4 ulp of L"""
    _, seeds, work = host
    nv = dim + 1
    s = C.seed_set(dim)
    flag, dist = seeds[dim]
    dref, lam = _out(work, f"seed{dim}", "dref", (-1, nv)), _out(work, f"seed{dim}", "clam", (-1, nv, nv))
    on = flag.astype(bool) & (s["tag"] != "extreme")
    assert np.array_equal(dist >= 0.0, np.broadcast_to(flag.astype(bool)[:, None], dist.shape))
    L = C.edge_length(s["X"])[on]
    tol = 4 * ULP * L[:, None]
    assert np.max(np.abs(dist[on] - dref[on]) / L[:, None]) <= 4 * ULP
    lam, X = lam[on], s["X"][on]
    assert np.all(lam >= 0.0) and np.max(np.abs(lam.sum(axis=2) - 1.0)) <= 4 * ULP
    ld = np.longdouble
    c = np.einsum("mai,mik->mak", lam.astype(ld), X.astype(ld))
    far = np.sqrt(np.sum((c - X.astype(ld)) ** 2, axis=2)).astype(np.float64)
    err = np.abs(far - dref[on])
    print(f"seed{dim}: {int(on.sum())} seed cells, worst | |c - x| - dist | = {np.max(err / L[:, None]) / ULP:.2f} ulp of L")
    assert np.all(err <= tol)
