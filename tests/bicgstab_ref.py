"""A numpy restatement of the engine's BiCGStab (cutfemx_amd/csrc/cfx_solve.hip, cfx_bicgstab_solve), shared by
tests/test_bicgstab_reference.py (no GPU), tests/test_gpu_bicgstab.py and tests/test_gpu_cpp_bicgstab.py, and the small
nonsymmetric matrices these files solve.

van der Vorst's BiCGStab, preconditioned from the RIGHT with M = diag(a_ii) (the sign kept; "jacobi") or M = I, so the
recurrence residual is the residual of the original system; stopping rule |r|_2 <= threshold = max(rtol |b|_2, atol),
norms over the iterated rows.

    r = b - A x0 (iterated rows);  rhat = r;  rho = rhat.r;  p = r
    0 iterations: BAD_DIAGONAL, else CONVERGED if |r| <= threshold, else MAX_ITER if max_iter == 0
    iteration it:
      phat = M^-1 p;  v = A phat;  sigma = rhat.v
          sigma == 0 or not finite            -> BREAKDOWN, iterations = it, x unchanged
      alpha = rho / sigma;  s = r - alpha v
          |s| <= threshold                    -> x += alpha phat; CONVERGED, iterations = it + 1, residual_norm = |s|
      shat = M^-1 s;  t = A shat;  tt = t.t;  ts = t.s
          tt not finite or not > 0, or ts not finite -> BREAKDOWN, iterations = it, x unchanged
      omega = ts / tt;  x += alpha phat + omega shat;  r = s - omega t;  rho' = rhat.r
          |r| <= threshold                    -> CONVERGED, it + 1
          it + 1 == max_iter                  -> MAX_ITER, it + 1
          omega or rho' zero or not finite    -> BREAKDOWN, it + 1 (x is this iterate)
      beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v);  rho = rho'

With a row list the entries of x outside the list are held fixed: they enter r0 = b - A x0 and nothing else (phat and shat
stay 0 there), so the call solves A[rows, rows] x[rows] = b[rows] - A[rows, others] x[others].  `iterations` counts the
updates of x that were made."""
from __future__ import annotations

import math

import numpy as np

from solve_ref import BAD_DIAGONAL, BREAKDOWN, CONVERGED, MAX_ITER, iteration_bound  # noqa: F401  (shared with the CG tests)

RTOL = 1e-10
# iterations of Jacobi BiCGStab to RTOL from x0 = 0 with b = A x* (case() below): counts of bicgstab() below, computed on the
# CPU (tests/test_bicgstab_reference.py holds them to this table, and holds the counts under eight permuted summation
# orders of every dot product inside solve_ref's band around them)
ITERATIONS = {("convdiff", 8, 8, 2): 25, ("convdiff", 12, 10, 8): 28, ("convdiff", 6, 5, 20): 16,
              ("convdiff", 40, 37, 4): 79, ("long_rows", 300, 150): 5, ("tridiag", 2048 * 256 + 300): 20}
# max |x - x_direct| / max |x_direct| of bicgstab() at RTOL: the worst over the cases above is DIRECT_WORST (the table of
# tests/test_bicgstab_reference.py lists every case); the engine sums in another order, so its bar is ten times that
DIRECT_WORST = 4.3e-10        # (measured 4.25e-10, on ("convdiff", 12, 10, 8))
DIRECT_BAR = 10.0 * DIRECT_WORST


def _dot(a, b):
    return float(a @ b)


def bicgstab(A, b, x0=None, *, rtol=1e-10, atol=0.0, max_iter=10000, precond="jacobi", rows=None, dot=_dot):
    """(x, reason, iterations, residual_norm, rhs_norm); A a scipy CSR matrix.  `dot`: the sum every dot product and norm
    goes through (the tests permute its order)."""
    n = A.shape[0]
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    Ar = A.tocsr()[rows]                       # the iterated rows, all columns
    r = b[rows] - Ar @ x
    bnorm, rnorm = math.sqrt(dot(b[rows], b[rows])), math.sqrt(dot(r, r))
    threshold = max(rtol * bnorm, atol)
    if precond == "jacobi":
        d = A.diagonal()[rows]
        if np.any(d == 0.0):
            return x, BAD_DIAGONAL, 0, rnorm, bnorm
        dinv = 1.0 / d
    elif precond in (None, "none"):
        dinv = np.ones(rows.size)
    else:
        raise ValueError(precond)
    if rnorm <= threshold:
        return x, CONVERGED, 0, rnorm, bnorm
    if max_iter == 0:
        return x, MAX_ITER, 0, rnorm, bnorm
    rhat, p = r.copy(), r.copy()
    rho = dot(rhat, r)
    phat, shat = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            phat[rows] = dinv * p
            v = Ar @ phat
            sigma = dot(rhat, v)
            if sigma == 0.0 or not math.isfinite(sigma):
                return x, BREAKDOWN, it, rnorm, bnorm
            alpha = rho / sigma
            s = r - alpha * v
            snorm = math.sqrt(dot(s, s))
            if snorm <= threshold:
                x[rows] += alpha * phat[rows]
                return x, CONVERGED, it + 1, snorm, bnorm
            shat[rows] = dinv * s
            t = Ar @ shat
            tt, ts = dot(t, t), dot(t, s)
            if not (math.isfinite(tt) and tt > 0.0 and math.isfinite(ts)):
                return x, BREAKDOWN, it, rnorm, bnorm
            omega = ts / tt
            x[rows] += alpha * phat[rows] + omega * shat[rows]
            r = s - omega * t
            rho_new, rnorm = dot(rhat, r), math.sqrt(dot(r, r))
            if rnorm <= threshold:
                return x, CONVERGED, it + 1, rnorm, bnorm
            if it + 1 == max_iter:
                break
            if omega == 0.0 or not math.isfinite(omega) or rho_new == 0.0 or not math.isfinite(rho_new):
                return x, BREAKDOWN, it + 1, rnorm, bnorm
            beta = (rho_new / rho) * (alpha / omega)
            p = r + beta * (p - omega * v)
            rho = rho_new
    return x, MAX_ITER, max_iter, rnorm, bnorm


def permuted_dot(seed: int):
    """A dot product that adds its terms in a seeded random order, one after the other (another rounding of every sum
    of the recurrence, as another tiling of the rows gives)."""
    perms = {}

    def dot(a, b):
        n = a.size
        if n not in perms:
            perms[n] = np.random.default_rng(seed + n).permutation(n)
        return float(np.sum((a * b)[perms[n]]))      # (pairwise over the permuted terms: not the order of a @ b)
    return dot


# ---- the matrices: small, nonsymmetric, nonsingular -----------------------------------------------------------------
def convdiff(nx: int, ny: int, pe: float):
    """-lap u + beta . grad u on an nx x ny grid of unknowns (unit spacing, Dirichlet rows eliminated), 5-point Laplacian
    and first-order upwinding; beta = pe (cos t, sin t) with t = 2 pi (i / nx + j / (2 ny)) turning with the position,
    so the asymmetry varies over the rows.  An irreducibly diagonally dominant M-matrix: nonsingular."""
    import scipy.sparse as sp
    A = sp.lil_matrix((nx * ny, nx * ny))
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            t = 2.0 * math.pi * (i / nx + 0.5 * j / ny)
            bx, by = pe * math.cos(t), pe * math.sin(t)
            A[k, k] = 4.0 + abs(bx) + abs(by)
            for di, dj, bd in ((-1, 0, bx), (1, 0, -bx), (0, -1, by), (0, 1, -by)):
                # the neighbour at (-1, 0) is upwind when bx > 0, the one at (+1, 0) when bx < 0: the upwind one takes -|bx|
                w = -1.0 - max(bd, 0.0)
                ii, jj = i + di, j + dj
                if 0 <= ii < nx and 0 <= jj < ny:
                    A[k, jj * nx + ii] = w
    A = A.tocsr()
    A.sort_indices()
    return A


def long_rows(n: int = 300, per_row: int = 150, seed: int = 5):
    """per_row random off-diagonal entries in (-1, 1) per row and a diagonal of alternating sign with
    |a_ii| = 1.5 sum_j |a_ij|: rows longer than a wave, pivots of both signs, strictly diagonally dominant."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    ip, ix, va = [0], [], []
    for i in range(n):
        cols = np.sort(rng.choice(np.delete(np.arange(n), i), size=per_row, replace=False))
        vals = rng.uniform(-1.0, 1.0, size=per_row)
        d = 1.5 * np.abs(vals).sum() * (1.0 if i % 2 == 0 else -1.0)
        pos = int(np.searchsorted(cols, i))
        ix.extend(np.insert(cols, pos, i))
        va.extend(np.insert(vals, pos, d))
        ip.append(len(ix))
    return sp.csr_matrix((np.array(va), np.array(ix, dtype=np.int32), np.array(ip, dtype=np.int64)), shape=(n, n))


def tridiag(n: int, c: float = 0.5):
    """(-1 - c, 3, -1 + c) on the three diagonals: more 256-row tiles than the solve kernels have blocks."""
    import scipy.sparse as sp
    A = sp.diags([np.full(n - 1, -1.0 - c), np.full(n, 3.0), np.full(n - 1, -1.0 + c)], [-1, 0, 1], format="csr")
    A.sort_indices()
    return A


def signed_diagonal(n: int = 37):
    """(d, b): a diagonal of both signs and magnitudes over three decades, and a right-hand side."""
    rng = np.random.default_rng(11)
    d = rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(-1, 2, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    return d, rng.standard_normal(n)


_CASES = {}


def case(key):
    """dict(A, b, xstar) of a key of ITERATIONS: b = A x* for a seeded x*.  Computed once and never modified."""
    if key not in _CASES:
        A = {"convdiff": convdiff, "long_rows": long_rows, "tridiag": tridiag}[key[0]](*key[1:])
        xstar = np.random.default_rng(23).standard_normal(A.shape[0])
        _CASES[key] = dict(A=A, b=A @ xstar, xstar=xstar)
    return _CASES[key]


_SOLVED = {}


def solved(key):
    """The restatement's (x, reason, iterations, residual_norm, rhs_norm) on case(key) at RTOL from x0 = 0, once."""
    if key not in _SOLVED:
        c = case(key)
        _SOLVED[key] = bicgstab(c["A"], c["b"], rtol=RTOL)
    return _SOLVED[key]
