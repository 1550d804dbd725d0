"""The solve in HBM (cutfemx_amd/csrc/cfx_solve.hip): y = A x with L lanes per row and Jacobi-preconditioned conjugate
gradients, through fem.spmv / fem.cg_solve / poisson.solve and the C++ facade.

References.  SpMV: scipy's A @ x on the same (downloaded) matrix, componentwise within the summation bound
4 len(row) eps (|A| @ |x|).  CG: the true residual formed by scipy, |b - A x| <= 2 rtol |b| (the recurrence residual
drifts from the true one by eps cond, far below rtol), and the iteration count of the numpy restatement
(tests/solve_ref.py, pinned to the issue's table by tests/test_solve_reference.py) within ceil(1.1 k) + 2.  Every sum of
the engine has a fixed order, so bits are compared wherever two calls must agree.

Measured iteration counts (engine / numpy): see DESIGN.md, "Solve"."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import solve_ref as R
from helpers import profiled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
EPS = np.finfo(np.float64).eps
LANES = (0, 1, 4, 8, 16, 64)
SENTINEL = np.float64(-7.25e300)
CG_CASES = [("box", 2, 16), ("box", 3, 8), ("scrambled", 3, 8), ("high_valence", 2, 30), ("high_valence", 3, (6, 6))]


def _id(v):
    return "-".join(str(p).replace(" ", "") for p in v) if isinstance(v, tuple) else str(v)


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def check_spmv(As, y, x, rows=None):
    """|y - A x| <= 4 len(row) eps (|A| @ |x|), componentwise, on the listed rows."""
    import scipy.sparse as sp
    want = As @ x
    # (|A| from the raw arrays: abs() of a scipy matrix first merges repeated columns IN PLACE)
    absA = sp.csr_matrix((np.abs(As.data), As.indices, As.indptr), shape=As.shape)
    bound = 4.0 * np.diff(As.indptr) * EPS * (absA @ np.abs(x))
    sel = np.arange(As.shape[0]) if rows is None else np.asarray(rows)
    err = np.abs(host(y) - want)[sel]
    assert np.all(err <= bound[sel]), (float(np.max(err - bound[sel])), int(sel[np.argmax(err - bound[sel])]))


# ---- SpMV on seeded random matrices ---------------------------------------------------------------------------------
_RANDOM = {}


def random_csr(nrows, rect):
    """Seeded random CSR: row lengths 0, 1, L and L + 1 for every L, and one row of 700; columns drawn with repetition
    and unsorted (a raw CSR array may hold both); ncols != nrows when `rect`."""
    import scipy.sparse as sp
    key = (nrows, rect)
    if key not in _RANDOM:
        rng = np.random.default_rng(1000 * nrows + rect)
        ncols = nrows + 37 if rect else nrows
        pool = np.array([0, 1, 2, 4, 5, 8, 9, 16, 17, 64, 65, 3, 30])
        lens = pool[rng.permutation(nrows) % pool.size]
        lens[nrows // 2] = 700
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        indices = rng.integers(0, ncols, size=int(indptr[-1])).astype(np.int32)
        values = rng.standard_normal(int(indptr[-1]))
        As = sp.csr_matrix((values, indices, indptr), shape=(nrows, ncols))
        _RANDOM[key] = (As, rng.standard_normal(ncols), rng.permutation(nrows)[: max(1, nrows // 3)].astype(np.int32))
    return _RANDOM[key]


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("rect", [False, True], ids=["square", "rect"])
@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 257, 1000])
def test_spmv_random(nrows, rect, lanes):
    from cutfemx_amd import fem
    As, x, rows = random_csr(nrows, rect)
    A = fem.csr_from_arrays(As.indptr, As.indices, As.data, ncols=As.shape[1])
    xd = dev(x)
    y = fem.spmv(A, xd, lanes_per_row=lanes)
    check_spmv(As, y, x)
    assert np.array_equal(bits(y), bits(fem.spmv(A, xd, lanes_per_row=lanes)))        # two calls: the same bits
    # a row list: the listed entries as before, every other entry untouched
    out = dev(np.full(nrows, SENTINEL))
    assert fem.spmv(A, xd, out=out, rows=rows, lanes_per_row=lanes) is out
    check_spmv(As, out, x, rows)
    assert np.array_equal(bits(out)[rows], bits(y)[rows])
    others = np.setdiff1d(np.arange(nrows), rows)
    assert np.all(bits(out)[others] == bits(np.array([SENTINEL]))[0])
    # host vectors go through the same kernel
    yh = fem.spmv(A, x, lanes_per_row=lanes)
    assert isinstance(yh, np.ndarray) and np.array_equal(bits(yh), bits(y))


# ---- assembled systems ------------------------------------------------------------------------------------------------
_ENGINE = {}


def engine_poisson(O, key, degree=1):
    """The cut Poisson system of a case assembled and deactivated by the engine: dict(A, b (numpy), domain, system, V, As
    (scipy, downloaded)).  Built once; nothing modifies it."""
    k = (key, degree)
    if k not in _ENGINE:
        import cutfemx_amd as cfx
        from cutfemx_amd import fem, poisson
        c = R.case(O, *key)
        om = c["om"]
        mesh = cfx.Mesh.from_arrays(key[1], om.x, om.conn)
        V1 = cfx.FunctionSpace(mesh, 1)
        V = V1 if degree == 1 else cfx.FunctionSpace(mesh, 2)
        cd = cfx.cut(cfx.Function(V1, c["phi"]))
        system = poisson.build_forms(V, cd)
        A = fem.assemble_matrix(system.a)
        b = fem.assemble_vector(system.L)
        domain = fem.active_domain(system.a)
        fem.deactivate_outside(A, b, domain)
        _ENGINE[k] = dict(A=A, b=b, domain=domain, system=system, V=V, As=A.to_scipy(), mesh=mesh, cd=cd)
    return _ENGINE[k]


@pytest.mark.parametrize("key,degree", [(("box", 2, 16), 1), (("box", 3, 8), 1), (("box", 3, 4), 2),
                                        (("high_valence", 3, (6, 6)), 1)], ids=_id)
def test_spmv_assembled(oracle, key, degree):
    from cutfemx_amd import fem
    E = engine_poisson(oracle, key, degree)
    As = E["As"]
    x = np.random.default_rng(5).standard_normal(As.shape[1])
    xd = dev(x)
    for lanes in LANES:
        y = fem.spmv(E["A"], xd, lanes_per_row=lanes)
        check_spmv(As, y, x)
        assert np.array_equal(bits(y), bits(fem.spmv(E["A"], xd, lanes_per_row=lanes)))


def true_residual(As, b, x):
    return float(np.linalg.norm(b - As @ host(x)))


@pytest.mark.parametrize("key", CG_CASES, ids=_id)
def test_cg_oracle_systems(oracle, key):
    """Converged, true residual, iteration count against the numpy restatement on the downloaded matrix; the bits of x
    and the iteration count do not depend on how often the host looks -- nor on whether it looks at all."""
    from cutfemx_amd import _lib, fem
    E = engine_poisson(oracle, key)
    A, As, b = E["A"], E["As"], E["b"]
    rtol = 1e-10
    _, reason, k_ref, _, _ = R.pcg(As, b, rtol=rtol)
    assert reason == R.CONVERGED and abs(k_ref - R.ITERATIONS[key]) <= 1   # (the engine's matrix is the oracle's to 1e-12)
    bd = dev(b)
    x, info = fem.cg_solve(A, bd, rtol=rtol)
    print(f"{key}: engine {info.iterations} iterations, numpy {k_ref}; |r| / |b| = {info.residual_norm / info.rhs_norm:.2e}, "
          f"true {true_residual(As, b, x) / np.linalg.norm(b):.2e}")
    assert info.reason == fem.CG_CONVERGED and info.converged
    assert abs(info.rhs_norm - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
    assert info.residual_norm <= rtol * info.rhs_norm
    assert true_residual(As, b, x) <= 2.0 * rtol * np.linalg.norm(b)
    assert info.iterations <= R.iteration_bound(k_ref)
    for kw in (dict(), dict(check_every=1), dict(check_every=7)):
        x2, info2 = fem.cg_solve(A, bd, rtol=rtol, **kw)
        assert np.array_equal(bits(x2), bits(x)) and info2 == info, kw
    # the host never looks: exactly max_iter iterations are launched, the info stays in HBM, no read-back
    buf = fem.cg_info_buffer()
    s0 = _lib.sync_count()
    x3, out = fem.cg_solve(A, bd, rtol=rtol, check_every=0, max_iter=200, info_out=buf)
    assert _lib.sync_count() == s0 and out is buf
    assert np.array_equal(bits(x3), bits(x)) and fem.read_cg_info(buf) == info
    # host vectors: the same kernels on staged copies
    xh, infoh = fem.cg_solve(A, b, rtol=rtol)
    assert isinstance(xh, np.ndarray) and np.array_equal(bits(xh), bits(x)) and infoh == info


def test_cg_active_rows_only(oracle):
    """The active rows alone give the solution of the full solve (the identity rows hold x = 0): from the ActiveDomain
    (listed on the device) and from a host list."""
    from cutfemx_amd import fem
    key = ("box", 3, 8)
    E = engine_poisson(oracle, key)
    A, As, b = E["A"], E["As"], E["b"]
    bd = dev(b)
    x, info = fem.cg_solve(A, bd)
    active = np.setdiff1d(np.arange(As.shape[0]), E["domain"].inactive_dofs).astype(np.int32)
    assert np.array_equal(host(fem.active_rows(E["domain"])), active) and 0 < active.size < As.shape[0]
    for kw in (dict(domain=E["domain"]), dict(rows=active)):
        xa, ia = fem.cg_solve(A, bd, **kw)
        assert ia.converged and ia.iterations <= R.iteration_bound(R.ITERATIONS[key])
        assert np.max(np.abs(host(xa) - host(x))) <= 1e-8 * np.max(np.abs(host(x)))
        assert true_residual(As, b, xa) <= 2e-10 * np.linalg.norm(b)
    with pytest.raises(ValueError):
        fem.cg_solve(A, bd, rows=active, domain=E["domain"])


def spd_matrix(n=300, seed=3):
    """A small sparse SPD matrix that is not an M-matrix: B B^T + I with B random sparse."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=0.02, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    return (B @ B.T + sp.identity(n)).tocsr()


def test_cg_rows_solve_the_reduced_system():
    """Nonzero x outside the list: A[rows, rows] y = b[rows] - A[rows, others] x[others]; unlisted entries untouched."""
    import scipy.sparse.linalg as spla
    from cutfemx_amd import fem
    As = spd_matrix()
    n = As.shape[0]
    rng = np.random.default_rng(8)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    rows = np.sort(rng.permutation(n)[: n // 2]).astype(np.int32)
    others = np.setdiff1d(np.arange(n), rows)
    want = spla.spsolve(As[rows][:, rows].tocsc(), b[rows] - As[rows][:, others] @ x0[others])
    A = fem.csr_from_arrays(As.indptr, As.indices, As.data)
    for lanes in (0, 64):
        x, info = fem.cg_solve(A, dev(b), x0=dev(x0), rows=rows, rtol=1e-12, lanes_per_row=lanes)
        assert info.converged
        assert np.max(np.abs(host(x)[rows] - want)) <= 1e-8 * np.max(np.abs(want))
        assert np.array_equal(bits(x)[others], bits(x0)[others])
        k_ref = R.pcg(As, b, x0, rtol=1e-12, rows=rows)[2]
        assert info.iterations <= R.iteration_bound(k_ref)


def test_cg_without_preconditioner_takes_longer(oracle):
    from cutfemx_amd import fem
    E = engine_poisson(oracle, ("box", 2, 16))
    bd = dev(E["b"])
    _, jac = fem.cg_solve(E["A"], bd)
    x, none = fem.cg_solve(E["A"], bd, precond="none")
    k_ref = R.pcg(E["As"], E["b"], precond="none")[2]
    assert none.converged and none.iterations > jac.iterations and none.iterations <= R.iteration_bound(k_ref)
    assert true_residual(E["As"], E["b"], x) <= 2e-10 * np.linalg.norm(E["b"])


def test_cg_start_vector_and_zero_rhs(oracle):
    import scipy.sparse.linalg as spla
    from cutfemx_amd import fem
    E = engine_poisson(oracle, ("box", 2, 16))
    A, As, b = E["A"], E["As"], E["b"]
    direct = spla.spsolve(As.tocsc(), b)
    assert np.linalg.norm(direct) > 0.0
    x, info = fem.cg_solve(A, dev(b), x0=dev(direct))                     # the solution as start vector: nothing to do
    assert info.converged and info.iterations == 0 and np.array_equal(bits(x), bits(direct))
    x, info = fem.cg_solve(A, dev(np.zeros_like(b)))                      # b = 0
    assert info.converged and info.iterations == 0 and info.rhs_norm == 0.0 and not host(x).any()


def test_cg_max_iter(oracle):
    from cutfemx_amd import fem
    E = engine_poisson(oracle, ("box", 3, 8))
    bd = dev(E["b"])
    x, info = fem.cg_solve(E["A"], bd, max_iter=5)
    assert info.reason == fem.CG_MAX_ITER and info.iterations == 5 and np.all(np.isfinite(host(x))) and host(x).any()
    xr = R.pcg(E["As"], E["b"], max_iter=5)[0]
    assert np.max(np.abs(host(x) - xr)) <= 1e-10 * np.max(np.abs(xr))
    x2, info2 = fem.cg_solve(E["A"], bd, max_iter=5, check_every=0)
    assert info2 == info and np.array_equal(bits(x2), bits(x))
    x0, info0 = fem.cg_solve(E["A"], bd, max_iter=0)
    assert info0.reason == fem.CG_MAX_ITER and info0.iterations == 0 and not host(x0).any()


def test_cg_breakdown_and_bad_diagonal(oracle):
    from cutfemx_amd import fem
    E = engine_poisson(oracle, ("box", 2, 16))
    As, b = E["As"], E["b"]
    N = fem.csr_from_arrays(As.indptr, As.indices, -As.data)
    for pc in ("jacobi", "none"):
        x, info = fem.cg_solve(N, dev(b), precond=pc)
        assert info.reason == fem.CG_BREAKDOWN and info.iterations == 0 and not host(x).any(), pc
    active = np.setdiff1d(np.arange(As.shape[0]), E["domain"].inactive_dofs).astype(np.int32)
    row = int(active[len(active) // 2])
    # the stored diagonal of a listed row set to 0 ...
    Z = As.copy()
    j = As.indptr[row] + int(np.flatnonzero(As.indices[As.indptr[row]:As.indptr[row + 1]] == row)[0])
    Z.data[j] = 0.0
    # ... and the entry removed from the pattern
    keep = np.ones(As.nnz, dtype=bool)
    keep[j] = False
    lens = np.diff(As.indptr)
    lens[row] -= 1
    ip = np.concatenate([[0], np.cumsum(lens)])
    for M in (fem.csr_from_arrays(Z.indptr, Z.indices, Z.data), fem.csr_from_arrays(ip, As.indices[keep], As.data[keep])):
        x, info = fem.cg_solve(M, dev(b), rows=active)
        assert info.reason == fem.CG_BAD_DIAGONAL and info.iterations == 0 and not host(x).any()
        x, info = fem.cg_solve(M, dev(b), rows=np.setdiff1d(active, [row]).astype(np.int32))   # the row not listed: fine
        assert info.converged
        assert fem.cg_solve(M, dev(b), rows=active, precond="none", max_iter=20)[1].reason != fem.CG_BAD_DIAGONAL


# ---- degree 2, vector spaces, merged blocks: SPD by construction ------------------------------------------------------
_SPD = {}


def spd_form_system(kind):
    """MASS + STIFFNESS (P2) or MASS + ELASTICITY (P1, bs = 3) over ALL cells of the 4^3 box: dict(A, As, b)."""
    if kind not in _SPD:
        import cutfemx_amd as cfx
        from cutfemx_amd import fem
        mesh = cfx.Mesh.create_box(3, 4)
        cells = np.arange(mesh.num_cells, dtype=np.int32)
        if kind == "p2":
            V = cfx.FunctionSpace(mesh, 2)
            ints = [fem.Integral(fem.MASS, cells=cells, qdegree=4), fem.Integral(fem.STIFFNESS, cells=cells, qdegree=2)]
        else:
            V = cfx.FunctionSpace(mesh, 1, bs=3)
            ints = [fem.Integral(fem.MASS, cells=cells, qdegree=2),
                    fem.Integral(fem.ELASTICITY, cells=cells, params=(1.0, 0.3), qdegree=0)]
        A = fem.assemble_matrix(fem.form(ints, V))
        As = A.to_scipy()
        b = np.random.default_rng(21).standard_normal(As.shape[0])
        _SPD[kind] = dict(A=A, As=As, b=b, V=V, mesh=mesh)
    return _SPD[kind]


@pytest.mark.parametrize("kind", ["p2", "elasticity"])
def test_cg_spd_forms(kind):
    """Degree-2 row lengths and a vector space (bs = 3) in CG."""
    from cutfemx_amd import fem
    S = spd_form_system(kind)
    As, b = S["As"], S["b"]
    assert abs(As - As.T).max() <= 1e-13 * abs(As).max() and np.diff(As.indptr).max() > (60 if kind == "p2" else 40)
    k_ref = R.pcg(As, b)[2]
    x, info = fem.cg_solve(S["A"], dev(b))
    print(f"{kind}: engine {info.iterations} iterations, numpy {k_ref}")
    assert info.converged and info.iterations <= R.iteration_bound(k_ref)
    assert true_residual(As, b, x) <= 2e-10 * np.linalg.norm(b)


def test_cg_merged_blocks():
    """A MergedCSR of two blocks on the diagonal: both systems in one solve."""
    import scipy.sparse as sp
    from cutfemx_amd import fem
    P, E = spd_form_system("p2"), spd_form_system("elasticity")
    M = fem.merge_blocks([[P["A"], None], [None, E["A"]]])
    Ms = M.to_scipy()
    assert abs(Ms - sp.block_diag([P["As"], E["As"]])).max() == 0.0
    b = np.concatenate([P["b"], E["b"]])
    k_ref = R.pcg(Ms, b)[2]
    x, info = fem.cg_solve(M, dev(b))
    assert info.converged and info.iterations <= R.iteration_bound(k_ref)
    assert true_residual(Ms, b, x) <= 2e-10 * np.linalg.norm(b)
    y = fem.spmv(M, x)
    check_spmv(Ms, y, host(x))


def test_cg_launch_count(oracle):
    """Three launches per iteration and a constant number around them; the host's look every check_every iterations
    decides only how many iterations are launched."""
    from cutfemx_amd import fem
    E = engine_poisson(oracle, ("box", 3, 8))
    bd = dev(E["b"])
    active = fem.active_rows(E["domain"])               # (ahead of the profile: the first request compacts the lists)
    for check_every, rows in ((1, None), (16, None), (16, active)):
        (x, info), names = profiled(lambda: fem.cg_solve(E["A"], bd, check_every=check_every, rows=rows))
        launched = -(-info.iterations // check_every) * check_every
        assert names["cg_spmv"] == names["cg_update"] == names["cg_direction"] == launched, (names, info)
        assert sum(names.values()) <= 3 * launched + 8, names
    (x, info), names = profiled(lambda: fem.cg_solve(E["A"], bd, check_every=0, max_iter=90))
    assert names["cg_spmv"] == 90 and info.converged and info.iterations < 90


def test_poisson_solve_end_to_end():
    """poisson.solve, then the L2 error functional of the solution in HBM, on 2-D n = 8, 16, 32: the error of the direct
    solve of the same system, and its convergence rate.

    rtol: the two discrete solutions differ by about rtol cond |u| (3e-9 |u| at the default 1e-10, tests/solve_ref.py's
    table), which is 1e-6 of a discretisation error of 5e-4 or more; two orders tighter keeps that difference two orders
    below the 1e-6 the comparison allows."""
    import scipy.sparse.linalg as spla
    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson
    from helpers import level_set_values
    err_cg, err_direct = [], []
    for n in (8, 16, 32):
        x, conn = cfx.box_mesh_arrays(2, n)
        mesh = cfx.Mesh.from_arrays(2, x, conn)
        V = cfx.FunctionSpace(mesh, 1)
        cd = cfx.cut(cfx.Function(V, level_set_values(x, 2)))
        system = poisson.build_forms(V, cd)
        uh, info = poisson.solve(system, V, rtol=1e-12)
        assert info.converged and uh.is_cuda
        err_cg.append(float(np.sqrt(fem.assemble_scalar(poisson.l2_error_form(system, V, uh)))))
        A = fem.assemble_matrix(system.a)
        b = fem.assemble_vector(system.L)
        fem.deactivate_outside(A, b, fem.active_domain(system.a))
        ud = spla.spsolve(A.to_scipy().tocsc(), b)
        err_direct.append(float(np.sqrt(fem.assemble_scalar(poisson.l2_error_form(system, V, ud)))))
    err_cg, err_direct = np.array(err_cg), np.array(err_direct)
    rate_cg, rate_direct = np.log2(err_cg[:-1] / err_cg[1:]), np.log2(err_direct[:-1] / err_direct[1:])
    print(f"L2 errors: cg {err_cg}, direct {err_direct}; rates {rate_cg} / {rate_direct}")
    assert np.all(np.abs(err_cg - err_direct) <= 1e-6 * err_direct)
    assert np.all(np.abs(rate_cg - rate_direct) <= 1e-5)
    if np.all(rate_direct > 1.7):
        assert np.all(rate_cg > 1.7)


def _read(path, dtypes):
    out, buf, o = [], path.read_bytes(), 0
    for dt in dtypes:
        n = int(np.frombuffer(buf, dtype=np.int64, count=1, offset=o)[0]); o += 8
        out.append(np.frombuffer(buf, dtype=dt, count=n, offset=o).copy()); o += n * np.dtype(dt).itemsize
    return out


@pytest.mark.parametrize("tdim,n", [(2, 16), (3, 8)])
def test_cpp_solve_facade(tmp_path, tdim, n):
    """tests/cpp/solve_facade.cpp: cg_solve and spmv of include/cutfemx_amd.hpp against scipy on the system it wrote."""
    import scipy.sparse as sp
    exe, out = tmp_path / "solve_facade", tmp_path / "solve.bin"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/solve_facade.cpp"),
                    "-o", str(exe), "-L", str(ROOT / "cutfemx_amd"), "-lcutfemx_amd",
                    f"-Wl,-rpath,{ROOT / 'cutfemx_amd'}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([str(exe), str(tdim), str(n), str(out)], check=True)
    ip, ix, va, b, u, y, info = _read(out, [np.int64, np.int32, np.float64, np.float64, np.float64, np.float64, np.float64])
    As = sp.csr_matrix((va, ix, ip), shape=(b.size, b.size))
    k_ref = R.pcg(As, b)[2]
    assert abs(k_ref - R.ITERATIONS[("box", tdim, n)]) <= 1
    assert int(info[0]) == R.CONVERGED and int(info[1]) <= R.iteration_bound(k_ref)
    assert abs(info[3] - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b) and info[2] <= 1e-10 * info[3]
    assert np.linalg.norm(b - As @ u) <= 2e-10 * np.linalg.norm(b)
    check_spmv(As, y, u)
