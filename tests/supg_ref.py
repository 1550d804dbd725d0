"""A numpy model of the SUPG level-set step of cutfemx_amd/supg.py, shared by tests/test_supg_reference.py (no GPU) and
tests/test_gpu_supg.py: A and b assembled cell by cell from the formulas of the module's docstring,

    n_K = grad(phi) / sqrt(|grad phi|^2 + 1e-14),  a = speed n_K,  h = largest vertex distance of the cell,
    tau = tau_scale / sqrt((2 / dt)^2 + (2 sqrt(|a|^2 + 1e-14) / h)^2 + 1e-30)
    A(u, w) = int u w + dt (a . grad u) w + tau (u + dt a . grad u)(a . grad w) dx
    b(w)    = int phi w + tau phi (a . grad w) dx

at the points of the standard rule the oracle serves (pyoracle.full_cell_rules: reference points, weights x |det J|),
then the Dirichlet treatment of the demo: rows and columns of the fixed dofs zeroed, b lifted by the old phi and set to
it on the fixed dofs."""
from __future__ import annotations

import numpy as np

RTOL = 1e-10
# max |x - x_direct| / max |x_direct| of bicgstab_ref.bicgstab (Jacobi, RTOL, x0 = phi) on the MODEL's systems of the
# cases of tests/test_gpu_supg.py (linear and sphere level set on each mesh, with and without fixed dofs): the worst is
# DIRECT_WORST (tests/test_supg_reference.py prints and holds every figure); the engine sums in another order, so its bar
# is ten times that
DIRECT_WORST = 5.6e-10        # (measured 5.57e-10, on ("scrambled", 3, 6), linear, no fixed dofs)
DIRECT_BAR = 10.0 * DIRECT_WORST

MESHES = (("box", 2, 4), ("box", 3, 3), ("scrambled", 3, 6))


def mesh_of(O, key):
    from helpers import scrambled_mesh
    kind, tdim, n = key
    return O.mesh_box(tdim, n) if kind == "box" else scrambled_mesh(O, tdim, n)


def cell_geometry(om):
    """(g [nc, nv, tdim]: the P1 gradients, h [nc]: the cell diameters)."""
    tdim = om.tdim
    X = om.x[om.conn][:, :, :tdim]                                     # (nc, nv, tdim)
    J = np.transpose(X[:, 1:, :] - X[:, :1, :], (0, 2, 1))             # J[c, d, t] = d x_d / d X_t
    Jinv = np.linalg.inv(J)
    dN = np.vstack([-np.ones((1, tdim)), np.eye(tdim)])                # (nv, tdim)
    g = np.einsum("it,ctd->cid", dN, Jinv)
    d = X[:, :, None, :] - X[:, None, :, :]
    return g, np.sqrt((d * d).sum(axis=3)).max(axis=(1, 2))


def assemble(O, om, phi, speed, dt, *, tau_scale=1.0, qdegree=2, fixed_dofs=None):
    """(A, b, A_full): scipy CSR matrix and vector of the step after the Dirichlet treatment (fixed rows and columns of A
    are zero, b lifted and set), and the matrix before it."""
    import scipy.sparse as sp
    tdim, nc, nv, n = om.tdim, om.ncells, om.tdim + 1, om.nnodes
    conn = om.conn
    r = O.full_cell_rules(om, np.arange(nc, dtype=np.int32), qdegree)
    off = np.asarray(r.offsets)
    nq = int(off[1] - off[0])
    assert np.all(np.diff(off) == nq) and np.array_equal(np.asarray(r.parent_map), np.arange(nc))
    P = np.asarray(r.points, dtype=np.float64).reshape(nc, nq, tdim)
    W = np.asarray(r.weights, dtype=np.float64).reshape(nc, nq)
    N = np.concatenate([1.0 - P.sum(axis=2, keepdims=True), P], axis=2)            # (nc, nq, nv)
    g, h = cell_geometry(om)
    pc, sc = phi[conn], speed[conn]
    gphi = np.einsum("ci,cid->cd", pc, g)
    g2 = (gphi * gphi).sum(axis=1)
    inv = 1.0 / np.sqrt(g2 + 1.0e-14)
    nn = g2 * inv * inv
    ng = np.einsum("cd,cid->ci", gphi, g) * inv[:, None]                            # n_K . grad N_i
    s, f = np.einsum("cqi,ci->cq", N, sc), np.einsum("cqi,ci->cq", N, pc)
    adv = np.sqrt(s * s * nn[:, None] + 1.0e-14)
    tau = tau_scale / np.sqrt((2.0 / dt) ** 2 + (2.0 * adv / h[:, None]) ** 2 + 1.0e-30)
    au = s[:, :, None] * ng[:, None, :]                                             # a . grad N_j at the points
    trial = N + dt * au                                                             # u + dt a . grad u
    Ae = np.einsum("cq,cqi,cqj->cij", W, N, trial) + np.einsum("cq,cq,cqi,cqj->cij", W, tau, au, trial)
    be = np.einsum("cq,cq,cqi->ci", W, f, N) + np.einsum("cq,cq,cq,cqi->ci", W, tau, f, au)
    rows = np.repeat(conn, nv, axis=1).ravel()
    cols = np.tile(conn, (1, nv)).ravel()
    A_full = sp.csr_matrix((Ae.ravel(), (rows, cols)), shape=(n, n))
    A_full.sum_duplicates()
    A_full.sort_indices()
    b = np.zeros(n)
    np.add.at(b, conn.ravel(), be.ravel())
    if fixed_dofs is None or len(fixed_dofs) == 0:
        return A_full, b, A_full
    fixed = np.asarray(fixed_dofs, dtype=np.int64)
    keep = np.ones(n)
    keep[fixed] = 0.0
    b = b - A_full[:, fixed] @ phi[fixed]
    b[fixed] = phi[fixed]
    A = (sp.diags(keep) @ A_full @ sp.diags(keep)).tocsr()
    A.sort_indices()
    return A, b, A_full


def solve_direct(A, b, fixed_dofs=None):
    """spsolve of the step: the zeroed rows of the fixed dofs get a unit diagonal."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    m = np.zeros(A.shape[0])
    if fixed_dofs is not None and len(fixed_dofs) > 0:
        m[np.asarray(fixed_dofs)] = 1.0
    return spla.spsolve((A + sp.diags(m)).tocsc(), b)


def sphere(om):
    from helpers import level_set_values
    return level_set_values(om.x, om.tdim)


def linear(om, F=0.7):
    """(phi, speed, n, c): phi = n . x - c with |n| = 1 and the constant speed F."""
    n = np.array([2.0, -1.0, 0.5][: om.tdim])
    n /= np.linalg.norm(n)
    return om.x[:, : om.tdim] @ n - 0.3, np.full(om.nnodes, F), n, 0.3


def face_dofs(om):
    """The dofs of the box face x_0 = 0."""
    return np.flatnonzero(np.abs(om.x[:, 0]) < 1e-12).astype(np.int32)


def setting(O, key, which: str):
    """(om, phi, speed, dt) of a test case: `which` = "sphere" (an off-centre sphere, speed = 1 + x_0) or "linear";
    dt = 0.5 h with h = 1 / n the mesh size."""
    om = mesh_of(O, key)
    if which == "sphere":
        phi, speed = sphere(om), 1.0 + om.x[:, 0]
    else:
        phi, speed = linear(om)[:2]
    return om, phi, speed, 0.5 / key[2]
