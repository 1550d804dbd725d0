"""A numpy restatement of the engine's MINRES (cutfemx_amd/csrc/cfx_solve.hip, cfx_minres_solve), shared by
tests/test_minres_reference.py (no GPU) and tests/test_gpu_minres.py, and the cut Stokes systems both files solve.

Paige-Saunders MINRES in the Lanczos form with an SPD diagonal preconditioner M: "abs_jacobi" m_i = |a_ii|, "abs_rowsum"
m_i = sum_j |a_ij| over the stored entries, or none.  Stopping rule |r|_{M^-1} <= max(rtol |b|_{M^-1}, atol) with
|y|_{M^-1} = sqrt(y . M^-1 y) over the iterated rows; |r|_{M^-1} is |eta| of the recurrence.  With a row list the entries of
x outside the list are held fixed: they enter r0 = b - A x0 and nothing else (z stays 0 there), so the call solves
A[rows, rows] x[rows] = b[rows] - A[rows, others] x[others].  `iterations` counts the updates of x that were made.
Reasons: a listed row with m_i = 0 gives BAD_DIAGONAL and x = x0; a non-finite delta or gamma^2 gives BREAKDOWN with x the
iterate before; gamma = 0 (the Krylov space is exhausted) finishes the update and is CONVERGED if the rule is met,
BREAKDOWN otherwise."""
from __future__ import annotations

import math

import numpy as np

from solve_ref import BAD_DIAGONAL, BREAKDOWN, CONVERGED, MAX_ITER, iteration_bound  # noqa: F401  (shared with the CG tests)

# iterations of |diag|-Jacobi MINRES to rtol = 1e-8 from x0 = 0 over the active rows of stokes_case(...): counts of
# minres() below, computed on the CPU (tests/test_minres_reference.py holds them to this table)
ITERATIONS = {("box", 2, 8): 199, ("box", 2, 16): 614, ("box", 3, 4): 476, ("scrambled", 3, 6): 1150}
RTOL = 1e-8
# max |x - x_direct| / max |x_direct| of minres() at RTOL stays below 1e3 RTOL on every case (smallest |eigenvalue| about
# 1e-4 against entries of order 1): measured ratios are recorded in tests/test_minres_reference.py
DIRECT_BAR = 1e3 * RTOL


def preconditioner(A, rows, precond):
    """m_i of the iterated rows (None: no preconditioner)."""
    A = A.tocsr()
    if precond in (None, "none"):
        return None
    if precond == "abs_jacobi":
        return np.abs(A.diagonal()[rows])
    if precond == "abs_rowsum":
        Ar = A[rows]
        return np.add.reduceat(np.concatenate([np.abs(Ar.data), [0.0]]), Ar.indptr[:-1]) * (np.diff(Ar.indptr) > 0)
    raise ValueError(precond)


def minres(A, b, x0=None, *, rtol=1e-10, atol=0.0, max_iter=10000, precond="abs_jacobi", rows=None):
    """(x, reason, iterations, residual_norm, rhs_norm); A a scipy CSR matrix, symmetric on the iterated rows."""
    n = A.shape[0]
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    Ar = A.tocsr()[rows]                       # the iterated rows, all columns
    m = preconditioner(A, rows, precond)
    minv = np.ones(rows.size) if m is None else 1.0 / np.where(m > 0.0, m, 1.0)
    v = b[rows] - Ar @ x                       # r0
    gamma1 = math.sqrt(float(v @ (minv * v)))
    bnorm = math.sqrt(float(b[rows] @ (minv * b[rows])))
    threshold = max(rtol * bnorm, atol)
    if m is not None and np.any(~(m > 0.0)):
        return x, BAD_DIAGONAL, 0, gamma1, bnorm
    if gamma1 <= threshold:
        return x, CONVERGED, 0, gamma1, bnorm
    if max_iter == 0:
        return x, MAX_ITER, 0, gamma1, bnorm
    z = np.zeros(n)
    z[rows] = minv * v / gamma1
    v_old, w, w_old = np.zeros(rows.size), np.zeros(rows.size), np.zeros(rows.size)
    gamma0, c0, s0, c1, s1, eta = 1.0, 1.0, 0.0, 1.0, 0.0, gamma1
    rnorm = gamma1
    for it in range(max_iter):
        q = Ar @ z
        delta = float(z[rows] @ q)
        if not math.isfinite(delta):
            return x, BREAKDOWN, it, rnorm, bnorm
        v_new = q - (delta / gamma1) * v - (gamma1 / gamma0) * v_old
        g2sq = float(v_new @ (minv * v_new))
        a0 = c1 * delta - c0 * s1 * gamma1
        a1 = math.sqrt(a0 * a0 + g2sq) if math.isfinite(g2sq) else math.nan
        a2 = s1 * delta + c0 * c1 * gamma1
        a3 = s0 * gamma1
        if not (math.isfinite(g2sq) and a1 > 0.0 and math.isfinite(a1)):
            return x, BREAKDOWN, it, rnorm, bnorm
        gamma2 = math.sqrt(g2sq)
        c2, s2 = a0 / a1, gamma2 / a1
        w_new = (z[rows] - a3 * w_old - a2 * w) / a1
        x[rows] += (c2 * eta) * w_new
        eta = -s2 * eta
        rnorm = abs(eta)
        if rnorm <= threshold:
            return x, CONVERGED, it + 1, rnorm, bnorm
        if not gamma2 > 0.0:
            return x, BREAKDOWN, it + 1, rnorm, bnorm
        z[rows] = minv * v_new / gamma2
        v_old, v = v, v_new
        w_old, w = w, w_new
        gamma0, gamma1 = gamma1, gamma2
        c0, s0, c1, s1 = c1, s1, c2, s2
    return x, MAX_ITER, max_iter, rnorm, bnorm


def minv_norm(A, y, rows, precond):
    """sqrt(y[rows] . M^-1 y[rows])."""
    m = preconditioner(A, rows, precond)
    yr = np.asarray(y)[rows]
    return math.sqrt(float(yr @ (yr if m is None else yr / m)))


_CASES = {}


def case_mesh(O, kind: str, tdim: int, n: int):
    from helpers import level_set_values, scrambled_mesh
    om = O.mesh_box(tdim, n) if kind == "box" else scrambled_mesh(O, tdim, n)
    if kind not in ("box", "scrambled"):
        raise ValueError(kind)
    return om, level_set_values(om.x, tdim)


def stokes_blocks(O, om, phi, *, order=4, sigma=1.0, gamma_u=0.1, gamma_p=0.1):
    """The oracle's four blocks of the P1 vector x P1 cut Brinkman / Stokes system [[K + sigma M + g_u, B^T], [B, -g_p]]
    (scipy CSR, diagonal blocks NOT yet deactivated) and the inactive dofs of the velocity and the pressure block."""
    import scipy.sparse as sp
    tdim = om.tdim
    VU, VP = O.Space(om.conn, om.nnodes, 1, tdim), O.Space(om.conn, om.nnodes, 1, 1)
    dom = O.classify(om.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    active = O.locate_entities(dom, "phi<=0")
    vol = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", order)
    ghost = O.ghost_penalty_facets(om, dom, "phi<0")
    skeleton = O.interior_facets_for_cells(om, active)
    aU = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=vol, qdegree=0),
          O.Integral(O.CELL, O.K_MASS, entities=inside, rules=vol, qdegree=2, coefficient=np.full(om.nnodes, float(sigma))),
          O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=ghost, params=(gamma_u,), qdegree=0)]
    aP = [O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=skeleton, params=(-gamma_p, 2.0), qdegree=0)]
    aBt = [O.Integral(O.CELL, O.K_DIV_TEST, entities=inside, rules=vol, params=(-1.0,), qdegree=1)]
    aB = [O.Integral(O.CELL, O.K_DIV_TRIAL, entities=inside, rules=vol, params=(-1.0,), qdegree=1)]
    aPd = [O.Integral(O.CELL, O.K_MASS, entities=inside, rules=vol, qdegree=2)]      # (the pressure's support)
    nu, npr = om.nnodes * tdim, om.nnodes

    def square(V, a, nn):
        ip, ix = O.create_sparsity(om, V, a)
        return sp.csr_matrix((O.assemble_matrix(om, V, a, ip, ix), ix, ip), shape=(nn, nn))

    def rect(V0, V1, a, shape):
        ip, ix = O.create_sparsity2(om, V0, V1, a)
        return sp.csr_matrix((O.assemble_matrix2(om, V0, V1, a, ip, ix), ix, ip), shape=shape)
    blocks = [[square(VU, aU, nu), rect(VU, VP, aBt, (nu, npr))], [rect(VP, VU, aB, (npr, nu)), square(VP, aP, npr)]]
    inactive_u = O.inactive_dofs(VU, O.active_cells(aU, om.ncells))
    inactive_p = O.inactive_dofs(VP, O.active_cells(aPd, om.ncells))
    return blocks, inactive_u, inactive_p


def merge(O, blocks, inactive_u, inactive_p):
    """The blocks put together (scipy.sparse.bmat; explicit zeros kept) after the deactivation of the two diagonal
    blocks: inactive rows / columns of a diagonal block zeroed, 1 on the diagonal."""
    import scipy.sparse as sp
    out = [[blocks[0][0].copy(), blocks[0][1]], [blocks[1][0], blocks[1][1].copy()]]
    for D, inactive in ((out[0][0], inactive_u), (out[1][1], inactive_p)):
        O.deactivate(inactive, D.indptr.astype(np.int64), D.indices.astype(np.int32), D.data)
    A = sp.bmat(out, format="csr")
    A.sort_indices()
    return A


def stokes_case(O, kind: str, tdim: int, n: int):
    """dict(om, phi, A, b, xstar, rows, nu, npr, inactive): the merged, deactivated system of a named case (A a scipy
    CSR matrix whose inactive rows are identity rows), b = A x* for a seeded x* that is zero on the inactive rows, and
    `rows`: the active rows -- velocity rows, then nu + pressure rows, ascending.  Computed once and never modified."""
    key = (kind, tdim, n)
    if key not in _CASES:
        om, phi = case_mesh(O, kind, tdim, n)
        blocks, iu, ip = stokes_blocks(O, om, phi)
        A = merge(O, blocks, iu, ip)
        nu, npr = om.nnodes * tdim, om.nnodes
        inactive = np.concatenate([iu, nu + ip]).astype(np.int64)
        rows = np.setdiff1d(np.arange(nu + npr), inactive).astype(np.int32)
        xstar = np.random.default_rng(17).standard_normal(nu + npr)
        xstar[inactive] = 0.0
        _CASES[key] = dict(om=om, phi=phi, A=A, b=A @ xstar, xstar=xstar, rows=rows, nu=nu, npr=npr, inactive=inactive,
                           blocks=blocks, inactive_u=iu, inactive_p=ip)
    return _CASES[key]


def without_pressure_diagonal(A, rows, nu):
    """A with the stored diagonal entries of the active pressure rows removed from the pattern (still symmetric)."""
    import scipy.sparse as sp
    coo = A.tocoo()
    drop = (coo.row == coo.col) & np.isin(coo.row, rows[rows >= nu])
    N = sp.csr_matrix((coo.data[~drop], (coo.row[~drop], coo.col[~drop])), shape=A.shape)
    N.sort_indices()
    return N


def quasi_definite(n=150, seed=3):
    """A small symmetric quasi-definite matrix [[S1, E], [E^T, -S2]] (S = B B^T + I, B and E random sparse): indefinite,
    and every principal submatrix is nonsingular -- any row list gives a solvable reduced system."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)

    def spd(s):
        B = sp.random(n, n, density=0.03, random_state=np.random.default_rng(s), data_rvs=np.random.default_rng(s + 1).standard_normal,
                      format="csr")
        return (B @ B.T + sp.identity(n)).tocsr()
    E = sp.random(n, n, density=0.03, random_state=rng, data_rvs=rng.standard_normal, format="csr")
    A = sp.bmat([[spd(seed), E], [E.T, -spd(seed + 7)]], format="csr")
    A.sort_indices()
    return A
