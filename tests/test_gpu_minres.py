"""MINRES in HBM (cutfemx_amd/csrc/cfx_solve.hip, cfx_minres_solve) through fem.minres_solve and stokes.solve, on the cut
Stokes systems of tests/minres_ref.py (pinned as symmetric, indefinite and nonsingular by tests/test_minres_reference.py).

References.  The numpy restatement of the same recurrence (minres_ref.minres) on the engine's OWN downloaded matrix: the
iteration count within [k / 1.1 - 2, ceil(1.1 k) + 2] (every sum of the engine runs in another order; four renumberings
of the rows moved the restatement's own counts by at most 1.5 %), the true residual within 10 x the restatement's own true
residual at its final iterate, and the solution within minres_ref.DIRECT_BAR = 1e3 rtol of the x* the right-hand side was
made from (the CPU test's bar against the direct solve).  Every sum of the engine has a fixed order, so bits are compared
wherever two calls must agree."""
import numpy as np
import pytest

import minres_ref as R
import solve_ref as S

pytestmark = pytest.mark.gpu
RTOL = R.RTOL
LANES = (1, 4, 8, 16, 64)


def _id(v):
    return "-".join(str(p).replace(" ", "") for p in v) if isinstance(v, tuple) else str(v)


def bits(a):
    return np.ascontiguousarray(host(a), dtype=np.float64).view(np.int64)


def dev(a):
    import torch
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def residual2(As, b, x, rows=None):
    r = b - As @ host(x)
    return float(np.linalg.norm(r if rows is None else r[rows]))


def in_count_band(k, k_ref):
    return k_ref / 1.1 - 2 <= k <= R.iteration_bound(k_ref)


_ENGINE = {}


def engine_stokes(O, key):
    """The system of a case built by stokes.build_blocks and assembled, deactivated and merged by the engine:
    dict(M, Ms (scipy, downloaded), rows (numpy), rows_dev, b (numpy, = Ms x*), xstar, system, nu, c (the oracle's case)).
    Built once; nothing modifies it."""
    if key not in _ENGINE:
        import cutfemx_amd as cfx
        from cutfemx_amd import stokes
        c = R.stokes_case(O, *key)
        om, tdim = c["om"], key[1]
        mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
        VU, VP = cfx.FunctionSpace(mesh, 1, bs=tdim), cfx.FunctionSpace(mesh, 1)
        cd = cfx.cut(cfx.Function(VP, c["phi"]))
        system = stokes.build_blocks(VU, VP, cd)
        M, rows_dev, domains = stokes.assemble(system)
        Ms = M.to_scipy()
        _ENGINE[key] = dict(M=M, Ms=Ms, rows=host(rows_dev).astype(np.int32), rows_dev=rows_dev, b=Ms @ c["xstar"], xstar=c["xstar"],
                            system=system, nu=c["nu"], c=c, domains=domains, mesh=mesh, VU=VU, VP=VP, cd=cd)
    return _ENGINE[key]


_REF = {}


def reference(E, key, **kw):
    """minres_ref.minres on the engine's matrix, with its own true 2-norm residual over the iterated rows; computed once
    per (case, arguments)."""
    k = (key, tuple(sorted((a, None if v is None else (v if np.isscalar(v) else id(v))) for a, v in kw.items())))
    if k not in _REF:
        out = R.minres(E["Ms"], E["b"], **kw)
        _REF[k] = out + (residual2(E["Ms"], E["b"], out[0], kw.get("rows")),)
    return _REF[k]


# ---- 1. parity with the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("box", 2, 8), ("box", 3, 4), ("scrambled", 3, 6)], ids=_id)
def test_minres_parity_with_the_restatement(oracle, key):
    from cutfemx_amd import fem
    E = engine_stokes(oracle, key)
    Ms, b, rows = E["Ms"], E["b"], E["rows"]
    assert np.array_equal(rows, E["c"]["rows"])                       # velocity rows, then nu + pressure rows, ascending
    x_ref, reason, k_ref, rn_ref, bn_ref, true_ref = reference(E, key, rtol=RTOL, rows=rows)
    assert reason == R.CONVERGED and in_count_band(k_ref, R.ITERATIONS[key])   # (the engine's matrix is the oracle's to 1e-12)
    x, info = fem.minres_solve(E["M"], dev(b), rtol=RTOL, rows=E["rows_dev"])
    true = residual2(Ms, b, x, rows)
    err = np.max(np.abs(host(x) - E["xstar"])) / np.max(np.abs(E["xstar"]))
    print(f"{key}: engine {info.iterations} iterations, numpy {k_ref}; |eta| / |b| = {info.residual_norm / info.rhs_norm:.2e}; "
          f"true |r|_2 engine {true:.3e}, numpy {true_ref:.3e}; max|x - x*| / max|x*| = {err:.2e}")
    assert info.reason == fem.CG_CONVERGED and info.converged
    assert in_count_band(info.iterations, k_ref), (info.iterations, k_ref)
    assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref and info.residual_norm <= RTOL * info.rhs_norm
    assert true <= 10.0 * true_ref, f"true residual: engine {true:.3e}, restatement {true_ref:.3e}"
    assert err <= R.DIRECT_BAR
    others = np.setdiff1d(np.arange(Ms.shape[0]), rows)
    assert others.size > 0 and np.array_equal(bits(x)[others], bits(np.zeros(others.size)))   # x0 = 0 there, bit for bit


# ---- 2. the blocks of stokes.py against the oracle's -------------------------------------------------------------------
def test_stokes_blocks_equal_the_oracles(oracle):
    from helpers import rel_err
    E = engine_stokes(oracle, ("box", 2, 8))
    got, ref = E["Ms"], E["c"]["A"]
    assert got.shape == ref.shape
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert rel_err(got.data, ref.data) < 1e-12
    for d, want in zip(E["domains"], (E["c"]["inactive_u"], E["c"]["inactive_p"])):
        assert np.array_equal(np.asarray(d.inactive_dofs), want)


# ---- 3. all rows; a start vector with entries off the list -----------------------------------------------------------
def test_minres_all_rows_and_start_vector(oracle):
    import scipy.sparse.linalg as spla
    from cutfemx_amd import fem
    key = ("box", 2, 8)
    E = engine_stokes(oracle, key)
    Ms, b = E["Ms"], E["b"]
    _, reason, k_ref, _, _, true_ref = reference(E, key, rtol=RTOL)
    x, info = fem.minres_solve(E["M"], dev(b), rtol=RTOL)
    assert reason == R.CONVERGED and info.converged and in_count_band(info.iterations, k_ref)
    assert residual2(Ms, b, x) <= 10.0 * true_ref, (residual2(Ms, b, x), true_ref)
    assert np.max(np.abs(host(x) - E["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(E["xstar"]))
    # non-zero x0 off the list acts as data: A[rows, rows] y = b[rows] - A[rows, others] x0[others]
    As = R.quasi_definite()
    n = As.shape[0]
    rng = np.random.default_rng(8)
    bq, x0 = rng.standard_normal(n), rng.standard_normal(n)
    rows = np.sort(rng.permutation(n)[: n // 2]).astype(np.int32)
    others = np.setdiff1d(np.arange(n), rows)
    assert abs(As[rows][:, others]).max() > 1.0
    want = spla.spsolve(As[rows][:, rows].tocsc(), bq[rows] - As[rows][:, others] @ x0[others])
    A = fem.csr_from_arrays(As.indptr, As.indices, As.data)
    x_ref, reason, k_ref, rn_ref, bn_ref = R.minres(As, bq, x0, rtol=1e-10, rows=rows)
    for lanes in (0, 64):
        x, info = fem.minres_solve(A, dev(bq), x0=dev(x0), rows=rows, rtol=1e-10, lanes_per_row=lanes)
        assert reason == R.CONVERGED and info.converged and in_count_band(info.iterations, k_ref)
        assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref
        assert np.max(np.abs(host(x)[rows] - want)) <= 1e-8 * np.max(np.abs(want))     # (|eigenvalues| in [1, 30])
        assert np.max(np.abs(host(x) - x_ref)) <= 1e-8 * np.max(np.abs(want))
        assert np.array_equal(bits(x)[others], bits(x0)[others])


# ---- 4. the preconditioners --------------------------------------------------------------------------------------------
def test_minres_preconditioners(oracle):
    from cutfemx_amd import fem
    key = ("box", 2, 8)
    E = engine_stokes(oracle, key)
    Ms, b, rows = E["Ms"], E["b"], E["rows"]
    bd = dev(b)
    counts = {}
    for pc in ("abs_jacobi", "abs_rowsum", None):
        x_ref, reason, k_ref, rn_ref, bn_ref, true_ref = reference(E, key, rtol=RTOL, rows=rows, precond=pc)
        x, info = fem.minres_solve(E["M"], bd, rtol=RTOL, rows=E["rows_dev"], precond=pc)
        counts[pc] = info.iterations
        assert reason == R.CONVERGED and info.converged and in_count_band(info.iterations, k_ref), (pc, info, k_ref)
        assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref and info.residual_norm <= RTOL * info.rhs_norm, pc
        assert residual2(Ms, b, x, rows) <= 10.0 * true_ref, (pc, residual2(Ms, b, x, rows), true_ref)
    assert counts[None] > 1.5 * counts["abs_jacobi"]
    bnorm2 = np.linalg.norm(b[rows])                                  # no preconditioner: the 2-norm, "none" is None
    assert abs(fem.minres_solve(E["M"], bd, rtol=RTOL, rows=rows, precond="none")[1].rhs_norm - bnorm2) <= 1e-12 * bnorm2
    # the stored diagonal of the pressure rows removed from the pattern: the row sum works, |diag| refuses
    N = R.without_pressure_diagonal(Ms, rows, E["nu"])
    bn = N @ E["xstar"]
    A = fem.csr_from_arrays(N.indptr, N.indices, N.data)
    x_ref, reason, k_ref, _, _ = R.minres(N, bn, rtol=RTOL, rows=rows, precond="abs_rowsum")
    x, info = fem.minres_solve(A, dev(bn), rtol=RTOL, rows=rows, precond="abs_rowsum")
    assert reason == R.CONVERGED and info.converged and in_count_band(info.iterations, k_ref)
    assert residual2(N, bn, x, rows) <= 10.0 * residual2(N, bn, x_ref, rows)
    assert np.max(np.abs(host(x) - E["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(E["xstar"]))
    x0 = np.random.default_rng(4).standard_normal(bn.size)
    x, info = fem.minres_solve(A, dev(bn), x0=dev(x0), rows=rows, precond="abs_jacobi")
    assert info.reason == fem.CG_BAD_DIAGONAL and info.iterations == 0 and np.array_equal(bits(x), bits(x0))
    # ... the velocity rows alone have their diagonal: fine
    assert fem.minres_solve(A, dev(bn), rows=rows[rows < E["nu"]], precond="abs_jacobi", max_iter=20)[1].reason != fem.CG_BAD_DIAGONAL
    # a listed row with no stored entry at all: the row sum refuses as well
    Z = N.tolil()
    Z[int(rows[-1]), :] = 0.0
    Z = Z.tocsr()
    Z.eliminate_zeros()
    Az = fem.csr_from_arrays(Z.indptr, Z.indices, Z.data)
    x, info = fem.minres_solve(Az, dev(bn), rows=rows, precond="abs_rowsum")
    assert info.reason == fem.CG_BAD_DIAGONAL and not host(x).any()
    # cg_solve keeps its own two names, and breaks down on the indefinite matrix
    with pytest.raises(ValueError, match="precond"):
        fem.cg_solve(E["M"], bd, precond="abs_jacobi")
    assert fem.cg_solve(E["M"], bd, rows=E["rows_dev"])[1].reason == fem.CG_BREAKDOWN


# ---- 5. determinism and freezing ---------------------------------------------------------------------------------------
def test_minres_is_deterministic_and_frozen(oracle):
    from cutfemx_amd import _lib, fem
    key = ("box", 2, 8)
    E = engine_stokes(oracle, key)
    bd = dev(E["b"])
    kw = dict(rtol=RTOL, rows=E["rows_dev"])
    x, info = fem.minres_solve(E["M"], bd, **kw)
    x2, info2 = fem.minres_solve(E["M"], bd, **kw)
    assert info.converged and np.array_equal(bits(x), bits(x2)) and info2 == info
    k = info.iterations
    for more in (dict(check_every=1), dict(check_every=7), dict(check_every=16), dict(check_every=0, max_iter=k + 40)):
        x3, info3 = fem.minres_solve(E["M"], bd, **kw, **more)
        assert np.array_equal(bits(x3), bits(x)) and info3 == info, more
    buf = fem.cg_info_buffer()
    s0 = _lib.sync_count()
    x4, out = fem.minres_solve(E["M"], bd, **kw, check_every=0, max_iter=k + 40, info_out=buf)
    assert _lib.sync_count() == s0 and out is buf
    assert np.array_equal(bits(x4), bits(x)) and fem.read_cg_info(buf) == info
    # host vectors: the same kernels on staged copies
    xh, infoh = fem.minres_solve(E["M"], E["b"], **kw)
    assert isinstance(xh, np.ndarray) and np.array_equal(bits(xh), bits(x)) and infoh == info


def test_minres_launch_count(oracle):
    """Three launches per iteration and a constant number around them."""
    from helpers import profiled
    from cutfemx_amd import fem
    E = engine_stokes(oracle, ("box", 2, 8))
    bd = dev(E["b"])
    (x, info), names = profiled(lambda: fem.minres_solve(E["M"], bd, rtol=RTOL, rows=E["rows_dev"], check_every=16))
    launched = -(-info.iterations // 16) * 16
    assert names["minres_spmv"] == names["minres_lanczos"] == names["minres_update"] == launched, (names, info)
    assert names["minres_init"] == names["minres_start"] == names["minres_normalise"] == 1
    assert sum(names.values()) <= 3 * launched + 8, names


# ---- 6. every lanes_per_row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_minres_lanes(oracle, lanes):
    from cutfemx_amd import fem
    key = ("box", 3, 4)                                              # mean row length 52
    E = engine_stokes(oracle, key)
    Ms, b, rows = E["Ms"], E["b"], E["rows"]
    _, reason, k_ref, _, _, true_ref = reference(E, key, rtol=RTOL, rows=rows)
    x, info = fem.minres_solve(E["M"], dev(b), rtol=RTOL, rows=E["rows_dev"], lanes_per_row=lanes)
    assert reason == R.CONVERGED and info.converged and in_count_band(info.iterations, k_ref), (info, k_ref)
    assert residual2(Ms, b, x, rows) <= 10.0 * true_ref, (residual2(Ms, b, x, rows), true_ref)
    assert np.max(np.abs(host(x) - E["xstar"])) <= R.DIRECT_BAR * np.max(np.abs(E["xstar"]))


@pytest.mark.parametrize("shape", [30, 70])
def test_minres_rowsum_on_long_rows(oracle, shape):
    """The P1 cut Poisson matrix of the high-valence mesh (rows of 33 entries on shape 30, of 73 -- longer than a wave --
    on shape 70): SPD, hence fine for MINRES.  The set-up sum of abs_rowsum with every L, a wave per row included, against
    the restatement; on shape 30 the count stays within 1.1 x + 2 of CG's count in solve_ref.ITERATIONS."""
    from cutfemx_amd import fem
    c = S.case(oracle, "high_valence", 2, shape)
    As, b = c["A"], c["b"]
    assert np.diff(As.indptr).max() == {30: 33, 70: 73}[shape]
    A = fem.csr_from_arrays(As.indptr, As.indices, As.data)
    x_ref, reason, k_ref, rn_ref, bn_ref = R.minres(As, b, precond="abs_rowsum")
    true_ref = residual2(As, b, x_ref)
    assert reason == R.CONVERGED
    for lanes in (0,) + LANES:
        x, info = fem.minres_solve(A, dev(b), precond="abs_rowsum", lanes_per_row=lanes)
        assert info.converged and in_count_band(info.iterations, k_ref), (lanes, info, k_ref)
        assert abs(info.rhs_norm - bn_ref) <= 1e-12 * bn_ref, lanes             # (the row sums enter |b|_{M^-1})
        assert residual2(As, b, x) <= 10.0 * true_ref, (lanes, residual2(As, b, x), true_ref)
        if shape == 30:
            assert info.iterations <= 1.1 * S.ITERATIONS[("high_valence", 2, 30)] + 2


# ---- 7. edges ------------------------------------------------------------------------------------------------------------
def test_minres_edges(oracle):
    import scipy.sparse as sp
    from cutfemx_amd import fem
    key = ("box", 2, 8)
    E = engine_stokes(oracle, key)
    M, Ms, b, rows = E["M"], E["Ms"], E["b"], E["rows"]
    bd = dev(b)
    x, info = fem.minres_solve(M, dev(np.zeros_like(b)), rows=rows)                     # b = 0
    assert info.converged and info.iterations == 0 and info.rhs_norm == 0.0 and not host(x).any()
    x, info = fem.minres_solve(M, bd, x0=dev(E["xstar"]), rows=rows, rtol=1e-6)          # x0 meets the rule
    assert info.converged and info.iterations == 0 and np.array_equal(bits(x), bits(E["xstar"]))
    x, info = fem.minres_solve(M, bd, rows=rows, max_iter=0)
    assert info.reason == fem.CG_MAX_ITER and info.iterations == 0 and not host(x).any()
    x, info = fem.minres_solve(M, bd, rows=rows, max_iter=3)
    x_ref, reason, its, rn_ref, _ = R.minres(Ms, b, rows=rows, max_iter=3)
    assert (info.reason, info.iterations) == (fem.CG_MAX_ITER, 3) == (reason, its)
    assert np.max(np.abs(host(x) - x_ref)) <= 1e-12 * np.max(np.abs(x_ref)) and abs(info.residual_norm - rn_ref) <= 1e-12 * rn_ref
    x2, info2 = fem.minres_solve(M, bd, rows=rows, max_iter=3, check_every=0)
    assert info2 == info and np.array_equal(bits(x2), bits(x))
    x, info = fem.minres_solve(M, bd, x0=dev(E["xstar"]), rows=np.zeros(0, dtype=np.int32))   # n_rows = 0
    assert info.converged and info.iterations == 0 and np.array_equal(bits(x), bits(E["xstar"]))
    # 1 x 1, and the 2 x 2 permutation (zero diagonal, indefinite): exact in at most 2 iterations
    A1 = fem.csr_from_arrays([0, 1], [0], [-4.0])
    x, info = fem.minres_solve(A1, dev([2.0]), precond=None, rtol=1e-12)
    assert info.converged and info.iterations == 1 and host(x)[0] == -0.5
    A2 = fem.csr_from_arrays([0, 1, 2], [1, 0], [1.0, 1.0])
    x, info = fem.minres_solve(A2, dev([1.0, 2.0]), precond=None, rtol=1e-12)
    assert info.converged and info.iterations == 2 and np.max(np.abs(host(x) - [2.0, 1.0])) <= 1e-14
    assert fem.minres_solve(A2, dev([1.0, 2.0]))[1].reason == fem.CG_BAD_DIAGONAL       # (|diag| = 0)
    # an SPD system: CG and MINRES agree to the tolerance
    c = S.case(oracle, "box", 2, 16)
    A = fem.csr_from_arrays(c["A"].indptr, c["A"].indices, c["A"].data)
    xc, ic = fem.cg_solve(A, dev(c["b"]))
    xm, im = fem.minres_solve(A, dev(c["b"]))
    assert ic.converged and im.converged and im.iterations <= R.iteration_bound(S.ITERATIONS[("box", 2, 16)])
    assert np.max(np.abs(host(xc) - host(xm))) <= 3e-9 * np.max(np.abs(host(xc)))      # (test_solve_reference's bar to the direct solve)
    # bad arguments are refused
    with pytest.raises(ValueError, match="precond"):
        fem.minres_solve(M, bd, precond="ilu")
    with pytest.raises(ValueError, match="lanes_per_row"):
        fem.minres_solve(M, bd, lanes_per_row=2)
    import ctypes as C
    from cutfemx_amd import _lib
    ip, ix, va = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32), np.ones(2)
    xh, info = np.zeros(2), _lib.CGInfoStruct()
    q = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().cfx_minres_solve(C.c_int64(2), q(ip), q(ix), q(va), None, C.c_int64(0), q(va), q(xh), None, C.byref(info))
    assert rc == _lib.ERR_INVALID_ARGUMENT and b"device pointer" in _lib.lib().cfx_last_error()    # host CSR arrays


# ---- 8. stokes.solve end to end ------------------------------------------------------------------------------------------
def test_stokes_solve_end_to_end(oracle):
    import scipy.sparse.linalg as spla
    from cutfemx_amd import fem, stokes
    key = ("box", 2, 16)
    E = engine_stokes(oracle, key)
    Ms, b, nu = E["Ms"], E["b"], E["nu"]
    u, p, info = stokes.solve(E["system"], dev(b[:nu]), b[nu:], rtol=RTOL)
    assert info.converged and u.is_cuda and p.is_cuda and in_count_band(info.iterations, R.ITERATIONS[key])
    x = np.concatenate([host(u), host(p)])
    direct = spla.spsolve(Ms.tocsc(), b)
    print(f"{key}: {info.iterations} iterations, max|x - direct| / max|direct| = {np.max(np.abs(x - direct)) / np.max(np.abs(direct)):.2e}")
    assert np.max(np.abs(x - direct)) <= R.DIRECT_BAR * np.max(np.abs(direct))
    inactive = E["c"]["inactive"]
    assert inactive.size > 0 and not x[inactive].any()
