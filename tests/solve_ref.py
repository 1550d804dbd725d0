"""A numpy restatement of the engine's conjugate gradients (cutfemx_amd/csrc/cfx_solve.hip), shared by
tests/test_solve_reference.py (no GPU) and tests/test_gpu_solve.py, and the oracle systems both files solve.

Classic PCG, Jacobi or no preconditioner, stopping rule |r|_2 <= max(rtol |b|_2, atol) on the recurrence residual, norms
over the iterated rows.  With a row list the entries of x outside the list are held fixed: they enter r0 = b - A x0 and
nothing else (p stays 0 there), so the call solves A[rows, rows] x[rows] = b[rows] - A[rows, others] x[others].
`iterations` counts the updates of x that were made: a breakdown (p.Ap <= 0) in the first iteration reports 0."""
from __future__ import annotations

import math

import numpy as np

CONVERGED, MAX_ITER, BREAKDOWN, BAD_DIAGONAL = 1, 2, 3, 4

# iterations of Jacobi-PCG to rtol = 1e-10 from x0 = 0 on the deactivated P1 cut Poisson systems of
# helpers.oracle_poisson (inactive rows: identity rows, b = 0 there)
ITERATIONS = {
    ("box", 2, 8): 29, ("box", 2, 16): 43, ("box", 2, 32): 66, ("box", 3, 4): 34, ("box", 3, 8): 53, ("box", 3, 12): 57,
    ("box", 3, 16): 63, ("scrambled", 3, 8): 57, ("scrambled", 2, 16): 46, ("high_valence", 2, 30): 66,
    ("high_valence", 3, (6, 6)): 70,
}


def pcg(A, b, x0=None, *, rtol=1e-10, atol=0.0, max_iter=10000, precond="jacobi", rows=None):
    """(x, reason, iterations, residual_norm, rhs_norm); A a scipy CSR matrix."""
    n = A.shape[0]
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    Ar = A.tocsr()[rows]                       # the iterated rows, all columns
    r = b[rows] - Ar @ x
    bnorm, rnorm = float(np.linalg.norm(b[rows])), float(np.linalg.norm(r))
    threshold = max(rtol * bnorm, atol)
    if precond == "jacobi":
        d = A.diagonal()[rows]
        if np.any(d == 0.0):
            return x, BAD_DIAGONAL, 0, rnorm, bnorm
        dinv = 1.0 / d
    else:
        dinv = np.ones(rows.size)
    if rnorm <= threshold:
        return x, CONVERGED, 0, rnorm, bnorm
    z = r * dinv
    p = np.zeros(n)
    p[rows] = z
    rho = float(r @ z)
    for it in range(max_iter):
        q = Ar @ p
        pq = float(p[rows] @ q)
        if not pq > 0.0:
            return x, BREAKDOWN, it, rnorm, bnorm
        alpha = rho / pq
        x[rows] += alpha * p[rows]
        r -= alpha * q
        z = r * dinv
        rho_new, rnorm = float(r @ z), float(np.linalg.norm(r))
        if rnorm <= threshold:
            return x, CONVERGED, it + 1, rnorm, bnorm
        p[rows] = z + (rho_new / rho) * p[rows]
        rho = rho_new
    return x, MAX_ITER, max_iter, rnorm, bnorm


def iteration_bound(k_ref: int) -> int:
    """Iterations the engine may take where this file takes k_ref: the sums run in another order, so the crossing of
    the threshold can move by an iteration or two."""
    return math.ceil(1.1 * k_ref) + 2


_CASES = {}


def case(O, kind: str, tdim: int, shape):
    """Mesh, level set and the oracle's P1 cut Poisson system of a named case, deactivated: dict(om, phi, ref, A, b)
    with A a scipy CSR matrix.  Computed once per session and never modified."""
    import scipy.sparse as sp

    from helpers import high_valence_case, level_set_values, oracle_poisson, scrambled_mesh
    key = (kind, tdim, shape)
    if key not in _CASES:
        if kind == "box":
            om = O.mesh_box(tdim, shape)
            phi = level_set_values(om.x, tdim)
        elif kind == "scrambled":
            om = scrambled_mesh(O, tdim, shape)
            phi = level_set_values(om.x, tdim)
        elif kind == "high_valence":
            om, phi, _ = high_valence_case(O, tdim, shape)
        else:
            raise ValueError(kind)
        ref = oracle_poisson(O, om, phi)
        vals, b = ref["values"].copy(), ref["b"].copy()
        O.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, b)
        n = ref["indptr"].size - 1
        A = sp.csr_matrix((vals, ref["indices"], ref["indptr"]), shape=(n, n))
        _CASES[key] = dict(om=om, phi=phi, ref=ref, A=A, b=b)
    return _CASES[key]
