"""Registered integrands with a coefficient LIST: several Functions per integral, each packed through the dofmap of its
own space into `w` at the reference's offsets (Form::coefficients() / coefficient_offsets(), pack_form.h:69-158).
Compilation targets gfx950 and needs no GPU; layout and values are checked on the GPU.  In every GPU test one
coefficient space has a caller-given degree-2 dofmap that is a renumbering of the standard one, so a gather through the
wrong dofmap shows."""
import numpy as np
import pytest

from helpers import level_set_values, rel_err

# scalar coefficient with ND dofs per cell (degree 1 or 2) at the reference point X
COEF_HELPERS = r"""
template <int ND>
__device__ inline double coef_value(const double* X, const double* wk)
{
  double N[10], dN[10][CFX_TDIM];
  if constexpr (ND == CFX_TDIM + 1) cfx_tabulate_p1(X, N, dN); else cfx_tabulate_p2(X, N, dN);
  double v = 0.0;
  for (int j = 0; j < ND; ++j) v += N[j] * wk[j];
  return v;
}
"""

# A[k] = w[k]: the packed array as the integrand sees it
DUMP_SRC = r"""
__device__ void user_wdump(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                           const double* points, const double* weights, const double* point_data)
{
  static_assert(CFX_CSTRIDE == CFX_W_OFF2 + CFX_W_ND2 * CFX_W_BS2 && CFX_NCOEF == 3, "offsets");
  for (int k = 0; k < CFX_CSTRIDE; ++k) A[k] = w[k];
}
"""
DUMP_FACET_SRC = r"""
__device__ void user_wdump_facet(double* A, const double* w, const double* c, const double* coordinate_dofs,
                                 const int* entity_local_index, int nq, const double* points0, const double* points1,
                                 const double* weights)
{
  for (int k = 0; k < 2 * CFX_CSTRIDE; ++k) A[k] = w[k];
}
"""

# kappa grad u . grad v, kappa = coefficient 0 of the list: CFX_K_STIFFNESS with `coefficient` (kappa = 1 where the form
# has no coefficient: w = NULL)
KAPPA_STIFFNESS_SRC = COEF_HELPERS + r"""
__device__ void user_kappa_stiffness(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                                     const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], g[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    const double kappa = w ? coef_value<CFX_W_ND0>(points + q * CFX_TDIM, w + CFX_W_OFF0) : 1.0;
    for (int i = 0; i < CFX_ND; ++i)
      for (int d = 0; d < CFX_TDIM; ++d)
      {
        double v = 0.0;
        for (int t = 0; t < CFX_TDIM; ++t) v += dN[i][t] * K[t][d];
        g[i][d] = v;
      }
    for (int i = 0; i < CFX_ND; ++i)
      for (int j = 0; j < CFX_ND; ++j)
      {
        double v = 0.0;
        for (int d = 0; d < CFX_TDIM; ++d) v += g[i][d] * g[j][d];
        A[i * CFX_ND + j] += weights[q] * kappa * v;
      }
  }
}
"""

# c1 (f, v), f = coefficient 0: CFX_L_SOURCE with the field id CFX_F_COEFFICIENT
F_SOURCE_SRC = COEF_HELPERS + r"""
__device__ void user_f_source(double* b, const double* w, const double* c, const double* coordinate_dofs, int nq,
                              const double* points, const double* weights, const double* point_data)
{
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    const double f = c[1] * coef_value<CFX_W_ND0>(points + q * CFX_TDIM, w + CFX_W_OFF0);
    for (int i = 0; i < CFX_ND; ++i) b[i] += weights[q] * f * N[i];
  }
}
"""

# c1 (kappa f, v): kappa and f are coefficients KF_K and KF_F of the list, each of its own shape
KF_SOURCE_SRC = COEF_HELPERS + r"""
#ifdef KF_SWAP
#define KF_K_ND CFX_W_ND1
#define KF_K_OFF CFX_W_OFF1
#define KF_F_ND CFX_W_ND0
#define KF_F_OFF CFX_W_OFF0
#else
#define KF_K_ND CFX_W_ND0
#define KF_K_OFF CFX_W_OFF0
#define KF_F_ND CFX_W_ND1
#define KF_F_OFF CFX_W_OFF1
#endif
__device__ void user_kf_source(double* b, const double* w, const double* c, const double* coordinate_dofs, int nq,
                               const double* points, const double* weights, const double* point_data)
{
  static_assert(CFX_W_BS0 == 1 && CFX_W_BS1 == 1 && CFX_CSTRIDE == CFX_W_ND0 + CFX_W_ND1, "two scalar coefficients");
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    const double kappa = coef_value<KF_K_ND>(points + q * CFX_TDIM, w + KF_K_OFF);
    const double f = c[1] * coef_value<KF_F_ND>(points + q * CFX_TDIM, w + KF_F_OFF);
    for (int i = 0; i < CFX_ND; ++i) b[i] += weights[q] * kappa * f * N[i];
  }
}
"""

# (beta . grad u) v: beta from a degree-2 vector Function (coefficient 0, CFX_W_BS0 components per dof) when the source is
# compiled for a list, from the constants c[0..2] otherwise
ADVECTION_SRC = r"""
__device__ void user_advection(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                               const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], beta[CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
#ifdef CFX_NCOEF
    double M[CFX_W_ND0], dM[CFX_W_ND0][CFX_TDIM];
    cfx_tabulate_p2(points + q * CFX_TDIM, M, dM);
    for (int d = 0; d < CFX_TDIM; ++d)
    {
      beta[d] = 0.0;
      for (int j = 0; j < CFX_W_ND0; ++j) beta[d] += M[j] * w[CFX_W_OFF0 + j * CFX_W_BS0 + d];
    }
#else
    for (int d = 0; d < CFX_TDIM; ++d) beta[d] = c[d];
#endif
    for (int j = 0; j < CFX_ND; ++j)
    {
      double bg = 0.0;
      for (int d = 0; d < CFX_TDIM; ++d)
        for (int t = 0; t < CFX_TDIM; ++t) bg += beta[d] * dN[j][t] * K[t][d];
      for (int i = 0; i < CFX_ND; ++i) A[i * CFX_ND + j] += weights[q] * bg * N[i];
    }
  }
}
"""

# two-space mass weighted by coefficient 1 of the list
MASS2_SRC = COEF_HELPERS + r"""
__device__ void user_wmass2(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                            const double* points, const double* weights, const double* point_data)
{
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND0], dN0[CFX_ND0][CFX_TDIM], N1[CFX_ND1], dN1[CFX_ND1][CFX_TDIM];
    cfx_tabulate0(points + q * CFX_TDIM, N0, dN0);
    cfx_tabulate1(points + q * CFX_TDIM, N1, dN1);
    const double rho = coef_value<CFX_W_ND1>(points + q * CFX_TDIM, w + CFX_W_OFF1);
    for (int i = 0; i < CFX_ND0; ++i)
      for (int j = 0; j < CFX_ND1; ++j) A[i * CFX_NDB1 + j] += weights[q] * rho * N0[i] * N1[j];
  }
}
"""


def test_sources_with_coefficient_lists_compile_for_gfx950_without_a_gpu():
    from cutfemx_amd import fem
    # reads w + CFX_W_OFF1, CFX_W_ND1, CFX_W_BS1 and CFX_CSTRIDE
    src = COEF_HELPERS + r"""
__device__ void user_two(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                         const double* points, const double* weights, const double* point_data)
{
  const double* w1 = w + CFX_W_OFF1;
  for (int q = 0; q < nq; ++q)
    for (int k = 0; k < CFX_W_ND1 * CFX_W_BS1; ++k) A[k % (CFX_NDB * CFX_NDB)] += weights[q] * w1[k] * w[CFX_CSTRIDE - 1];
}
"""
    k = fem.register_integrand("user_two", src, variant=(3, 4, 1), coefficients=[(4, 1), (10, 3)])
    assert k >= 1000
    fem.compile_integrand(k, 2, 6, 1, coefficients=[(3, 1), (6, 1), (3, 2)])
    kf = fem.register_integrand("user_wdump_facet", DUMP_FACET_SRC, facet=True, variant=(3, 4, 1),
                                coefficients=[(4, 1), (10, 1), (4, 3)])
    k2 = fem.register_integrand("user_wmass2", MASS2_SRC, variant=(2, 3, 1, 6, 1), coefficients=[(3, 1), (6, 1)])
    fem.compile_integrand2(k2, 3, 4, 1, 10, 1, coefficients=[(4, 1), (4, 1)])
    assert len({k, kf, k2}) == 3
    # without the signature the source names macros that do not exist
    with pytest.raises(ValueError, match="does not compile"):
        fem.register_integrand("user_two", src, variant=(3, 4, 1))
    # a source written for other shapes is refused with the compiler's log
    with pytest.raises(ValueError, match="two scalar coefficients"):
        fem.register_integrand("user_kf_source", KF_SOURCE_SRC, rank=1, variant=(3, 10, 1), coefficients=[(4, 1), (10, 3)])
    # `w` holds at most 64 doubles: 4 + 30 + 30 + 4 = 68 for a cell integral, 2 * (10 + 30) for a facet
    with pytest.raises(ValueError, match="64 doubles"):
        fem.compile_integrand(k, 3, 4, 1, coefficients=[(4, 1), (10, 3), (10, 3), (4, 1)])
    with pytest.raises(ValueError, match="32 per cell"):
        fem.compile_integrand(kf, 3, 4, 1, coefficients=[(10, 1), (10, 3)])
    with pytest.raises(ValueError, match="at most 8"):
        fem.compile_integrand(k, 3, 4, 1, coefficients=[(4, 1)] * 9)
    # exactly 64 is accepted
    fem.compile_integrand(k, 3, 4, 1, coefficients=[(4, 1), (10, 3), (10, 3)])
    # one integral takes `coefficient` or `coefficients`
    with pytest.raises(ValueError, match="not both"):
        fem.Integral(k, coefficient=np.zeros(4), coefficients=(object(),))


class _Problem:
    """mesh_box(2, 4) / mesh_box(3, 3) cut by the circle / sphere of helpers.level_set_values with P1 / P2 spaces; `P2p`
    is the degree-2 space under a random renumbering of its dofs, given as a caller dofmap.  The integrals run over
    {phi < 0} in 2-D (3 uncut cells, 16 cut ones).  In 3-D no cell of the 3^3 box (h = 1/3) fits into the sphere of
    radius 0.31 -- `phi<0` locates nothing -- so they run over the complement {phi > 0}: 84 uncut cells and the rules of
    the 78 cut ones, which keeps the standard entities and the cut rules non-empty on the same mesh and level set."""

    def __init__(self, oracle, tdim):
        import cutfemx_amd as cfx
        n = 3 if tdim == 3 else 4
        om = oracle.mesh_box(tdim, n)
        self.tdim, self.om = tdim, om
        self.conn = np.ascontiguousarray(om.conn, dtype=np.int32)
        self.mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
        self.dm2, self.nd2 = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
        rng = np.random.default_rng(17)
        self.perm = rng.permutation(self.nd2).astype(np.int32)       # new id of standard dof d: perm[d]
        self.dm2p = np.ascontiguousarray(self.perm[self.dm2], dtype=np.int32)
        assert not np.array_equal(self.dm2p, self.dm2)
        mesh = self.mesh
        self.P1 = cfx.FunctionSpace(mesh, 1)
        self.P1b = cfx.FunctionSpace(mesh, 1, dofmap=self.conn, ndofs=om.nnodes)   # another space object
        self.P2 = cfx.FunctionSpace(mesh, 2, dofmap=self.dm2, ndofs=self.nd2)
        self.P2p = cfx.FunctionSpace(mesh, 2, dofmap=self.dm2p, ndofs=self.nd2)
        self.cd = cfx.cut(cfx.Function(self.P1, level_set_values(om.x, tdim)))
        self.side = "phi<0" if tdim == 2 else "phi>0"
        self.inside = cfx.locate_entities(self.cd, self.side)
        self.vol = cfx.runtime_quadrature(self.cd, self.side, 3)
        assert len(self.inside) > 0 and self.vol.num_rules > 0
        # coordinates of the degree-2 dofs (standard numbering): vertices, then edge midpoints in the engine's order
        edges = [(1, 2), (0, 2), (0, 1)] if tdim == 2 else [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]
        self.x2 = np.zeros((self.nd2, 3))
        xc = om.x[self.conn]
        for i in range(tdim + 1):
            self.x2[self.dm2[:, i]] = xc[:, i]
        for e, (a, b) in enumerate(edges):
            self.x2[self.dm2[:, tdim + 1 + e]] = 0.5 * (xc[:, a] + xc[:, b])
        self.x1 = om.x
        self.p1, self.p2 = tdim + 1, self.dm2.shape[1]

    def permuted(self, v2, bs=1):
        """dof values of a degree-2 Function in the numbering of P2p"""
        v2 = np.asarray(v2).reshape(self.nd2, bs)
        out = np.empty_like(v2)
        out[self.perm] = v2
        return np.ascontiguousarray(out.ravel())


@pytest.fixture(scope="module", params=[2, 3], ids=["2d", "3d"])
def problem(request, oracle):
    return _Problem(oracle, request.param)


@pytest.fixture(scope="module")
def problem3(oracle):
    return _Problem(oracle, 3)


def _smooth(x):
    return 1.5 + np.sin(2.0 * x[:, 0] + 0.3) * np.cos(1.5 * x[:, 1]) + 0.25 * x[:, 2] * x[:, 0]


@pytest.mark.gpu
def test_cell_integrand_sees_the_reference_layout_of_w(problem3):
    """P1 scalar + P2 vector (bs 3, renumbered dofmap) + P2 scalar on a scalar P2 form: cstride 44 of the 100 entries."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem3
    rng = np.random.default_rng(1)
    U2p = cfx.FunctionSpace(pb.mesh, 2, dofmap=pb.dm2p, ndofs=pb.nd2, bs=3)
    v0, v1, v2 = rng.standard_normal(pb.om.nnodes), rng.standard_normal(3 * pb.nd2), rng.standard_normal(pb.nd2)
    fs = (cfx.Function(pb.P1b, v0), cfx.Function(U2p, v1), cfx.Function(pb.P2, v2))
    k = fem.register_integrand("user_wdump", DUMP_SRC, variant=(3, 10, 1), coefficients=[(4, 1), (10, 3), (10, 1)])
    a = fem.form([fem.Integral(k, cells=pb.inside, rules=pb.vol, qdegree=2, coefficients=fs)], pb.P2, rank=2)

    def expected(cell):
        w = np.concatenate([v0[pb.conn[cell]], v1.reshape(-1, 3)[pb.dm2p[cell]].ravel(), v2[pb.dm2[cell]]])
        assert w.size == 44
        return np.concatenate([w, np.zeros(100 - 44)])
    parents = pb.vol.parent_map
    for idx in (1, len(pb.inside) - 1):
        assert np.array_equal(fem.tabulate_entity(a, 0, idx, False).ravel(), expected(pb.inside[idx]))
    for idx in (2, pb.vol.num_rules - 1):
        assert np.array_equal(fem.tabulate_entity(a, 0, idx, True).ravel(), expected(parents[idx]))


@pytest.mark.gpu
def test_facet_integrand_sees_both_cells_of_every_coefficient(problem3):
    """P1 scalar + P2 scalar (renumbered dofmap) + P1 vector (bs 3) on a scalar P1 form in 3-D: cstride 26, w = 52 of the
    64 macro entries; coefficient k: cell 0 at 2 off_k, cell 1 directly after it.  Ghost-penalty facets, and the DG
    skeleton's [facets, facet-hosted rules]."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem3
    rng = np.random.default_rng(2)
    U1 = cfx.FunctionSpace(pb.mesh, 1, bs=3)
    v0, v1, v2 = rng.standard_normal(pb.om.nnodes), rng.standard_normal(pb.nd2), rng.standard_normal(3 * pb.om.nnodes)
    fs = (cfx.Function(pb.P1b, v0), cfx.Function(pb.P2p, v1), cfx.Function(U1, v2))
    k = fem.register_integrand("user_wdump_facet", DUMP_FACET_SRC, facet=True, variant=(3, 4, 1),
                               coefficients=[(4, 1), (10, 1), (4, 3)])

    def expected(row):
        c0, c1 = int(row[0]), int(row[2])
        blocks = []
        for c in (c0, c1):
            blocks.append([v0[pb.conn[c]], v1[pb.dm2p[c]], v2.reshape(-1, 3)[pb.conn[c]].ravel()])
        w = np.concatenate([blocks[s][j] for j in range(3) for s in range(2)])
        assert w.size == 52
        return np.concatenate([w, np.zeros(64 - 52)])
    ghost = cfx.ghost_penalty_facets(pb.cd, "phi<0")
    rows = ghost.rows
    assert len(rows) > 2
    a = fem.form([fem.Integral(k, facets=ghost, qdegree=2, coefficients=fs)], pb.P1, rank=2)
    for f in (0, len(rows) // 2, len(rows) - 1):
        want = expected(rows[f])
        assert not np.array_equal(want[0:4], want[4:8]) and not np.array_equal(want[8:18], want[18:28])  # the cells differ
        assert np.array_equal(fem.tabulate_entity(a, 0, f, False).ravel(), want)
    # facet-hosted rules: entities past the standard facets
    # (the cut DG skeleton as poisson.build_dg_forms makes it: the skeleton of the active cells cut with the facets as hosts)
    from cutfemx_amd.cut import cut, interior_facets_for_cells, locate_entities, runtime_quadrature
    nc = pb.mesh.num_cells
    DG = cfx.FunctionSpace(pb.mesh, 1, dofmap=np.arange(4 * nc, dtype=np.int32).reshape(nc, 4), ndofs=4 * nc)
    skeleton = interior_facets_for_cells(pb.mesh, locate_entities(pb.cd, "phi<=0"))
    skeleton_cut = cut(cfx.Function(pb.P1, level_set_values(pb.om.x, 3)), skeleton, 2)
    std_rows = np.ascontiguousarray(skeleton.rows[locate_entities(skeleton_cut, "phi<0")], dtype=np.int32).reshape(-1, 4)
    facet_rules = runtime_quadrature(skeleton_cut, "phi<0", 3)
    n_std, nr = len(std_rows), facet_rules.num_rules
    assert nr > 0
    a = fem.form([fem.Integral(k, facets=std_rows, rules=facet_rules, qdegree=2, coefficients=fs)], DG, rank=2)
    hosts = facet_rules.host_rows.reshape(-1, 4)
    if n_std > 0:   # (no skeleton facet lies inside the sphere on this mesh when no cell does)
        assert np.array_equal(fem.tabulate_entity(a, 0, n_std - 1, False).ravel(), expected(std_rows[n_std - 1]))
    for r in (0, nr - 1):
        assert np.array_equal(fem.tabulate_entity(a, 0, n_std + r, False).ravel(), expected(hosts[r]))


def _space_and_twin(pb, degree):
    """(form space, Function of a smooth field on it, the same Function on a space with another dofmap object)"""
    import cutfemx_amd as cfx
    if degree == 1:
        v = _smooth(pb.x1)
        return pb.P1, cfx.Function(pb.P1, v), cfx.Function(pb.P1b, v)
    v = _smooth(pb.x2)
    return pb.P2, cfx.Function(pb.P2, v), cfx.Function(pb.P2p, pb.permuted(v))


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 2])
def test_one_coefficient_equals_the_builtin_coefficient(problem, degree, monkeypatch):
    """n = 1: kappa-weighted stiffness = CFX_K_STIFFNESS with `coefficient`, (f, v) = CFX_L_SOURCE with F_COEFFICIENT --
    the Function on the form's own space, and the same Function on a renumbered twin of that space."""
    from cutfemx_amd import fem
    pb = problem
    V, kappa, twin = _space_and_twin(pb, degree)
    nd = V.ndofs_cell
    ks = fem.register_integrand("user_kappa_stiffness", KAPPA_STIFFNESS_SRC, variant=(pb.tdim, nd, 1), coefficients=[(nd, 1)])
    kf = fem.register_integrand("user_f_source", F_SOURCE_SRC, rank=1, variant=(pb.tdim, nd, 1), coefficients=[(nd, 1)])
    qd = 2 * degree

    def builtin():
        a = fem.form([fem.Integral(fem.STIFFNESS, cells=pb.inside, rules=pb.vol, qdegree=qd, coefficient=kappa)], V)
        L = fem.form([fem.Integral(fem.SOURCE, cells=pb.inside, rules=pb.vol, qdegree=qd, params=(fem.F_COEFFICIENT, 2.5),
                                   coefficient=kappa)], V)
        return a, L

    def registered(fn):
        a = fem.form([fem.Integral(ks, cells=pb.inside, rules=pb.vol, qdegree=qd, coefficients=(fn,))], V)
        L = fem.form([fem.Integral(kf, cells=pb.inside, rules=pb.vol, qdegree=qd, params=(0.0, 2.5), coefficients=(fn,))], V)
        return a, L
    a_ref, L_ref = builtin()
    A_ref, b_ref = fem.assemble_matrix(a_ref), fem.assemble_vector(L_ref)
    assert np.abs(A_ref.data).max() > 1e-3 and np.abs(b_ref).max() > 1e-6
    for fn in (kappa, twin):
        a, L = registered(fn)
        A = fem.assemble_matrix(a)
        assert np.array_equal(A.indptr, A_ref.indptr) and np.array_equal(A.indices, A_ref.indices)
        assert rel_err(A.data, A_ref.data) < 1e-13
        assert rel_err(fem.assemble_vector(L), b_ref) < 1e-13
        for idx, use_rule in ((0, False), (len(pb.inside) - 1, False), (1, True)):
            assert rel_err(fem.tabulate_entity(a, 0, idx, use_rule), fem.tabulate_entity(a_ref, 0, idx, use_rule)) < 1e-13
    monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    a_ref, L_ref = builtin()
    a, L = registered(twin)
    assert rel_err(fem.assemble_matrix(a).data, fem.assemble_matrix(a_ref).data) < 1e-13
    assert rel_err(fem.assemble_vector(L), fem.assemble_vector(L_ref)) < 1e-13


def _kf_forms(pb, fem, cfx):
    """The two-coefficient source (kappa f, v), kappa in P1 (its own space object), f in P2 (renumbered dofmap)."""
    sig = [(pb.p1, 1), (pb.p2, 1)]
    k_p2 = fem.register_integrand("user_kf_source", KF_SOURCE_SRC, rank=1, variant=(pb.tdim, pb.p2, 1), coefficients=sig)
    k_p1 = fem.register_integrand("user_kf_source", KF_SOURCE_SRC, rank=1, variant=(pb.tdim, pb.p1, 1), coefficients=sig)
    k_swap = fem.register_integrand("user_kf_source", "#define KF_SWAP 1\n" + KF_SOURCE_SRC, rank=1,
                                    variant=(pb.tdim, pb.p2, 1), coefficients=sig[::-1])

    def form_of(k, V, fs):
        return fem.form([fem.Integral(k, cells=pb.inside, rules=pb.vol, qdegree=4, params=(0.0, 1.5), coefficients=fs)], V)
    return k_p2, k_p1, k_swap, form_of


@pytest.mark.gpu
def test_two_coefficients_on_two_spaces(problem):
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem
    k_p2, k_p1, k_swap, form_of = _kf_forms(pb, fem, cfx)
    kap, f2 = _smooth(pb.x1), _smooth(pb.x2[:, [1, 2, 0]])

    def builtin(V, fn):
        return fem.assemble_vector(fem.form([fem.Integral(fem.SOURCE, cells=pb.inside, rules=pb.vol, qdegree=4,
                                                          params=(fem.F_COEFFICIENT, 1.5), coefficient=fn)], V))
    one1, one2 = cfx.Function(pb.P1b, np.ones(pb.om.nnodes)), cfx.Function(pb.P2p, np.ones(pb.nd2))
    K, F = cfx.Function(pb.P1b, kap), cfx.Function(pb.P2p, pb.permuted(f2))
    # kappa = 1: the source term of f on the P2 space
    want = builtin(pb.P2, cfx.Function(pb.P2, f2))
    assert np.abs(want).max() > 1e-6
    assert rel_err(fem.assemble_vector(form_of(k_p2, pb.P2, (one1, F))), want) < 1e-13
    # f = 1, form space P1: the source term of kappa
    assert rel_err(fem.assemble_vector(form_of(k_p1, pb.P1, (K, one2))), builtin(pb.P1, cfx.Function(pb.P1, kap))) < 1e-13
    # the list in the other order, read by a source with the offsets swapped
    b = fem.assemble_vector(form_of(k_p2, pb.P2, (K, F)))
    assert rel_err(b, want) > 1e-3
    assert rel_err(fem.assemble_vector(form_of(k_swap, pb.P2, (F, K))), b) < 1e-13


@pytest.mark.gpu
def test_vector_coefficient_advects_like_the_constant(problem):
    """(beta . grad u, v) on P1 with beta a constant degree-2 vector Function (bs = gdim, renumbered dofmap) equals the
    integrand that takes beta from `params`."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem
    td = pb.tdim
    beta = (0.7, -1.3, 0.4)[:td]
    U2p = cfx.FunctionSpace(pb.mesh, 2, dofmap=pb.dm2p, ndofs=pb.nd2, bs=td)
    B = cfx.Function(U2p, np.tile(np.array(beta), pb.nd2))
    k_w = fem.register_integrand("user_advection", ADVECTION_SRC, variant=(td, pb.p1, 1), coefficients=[(pb.p2, td)])
    k_c = fem.register_integrand("user_advection", ADVECTION_SRC, variant=(td, pb.p1, 1))
    a_w = fem.form([fem.Integral(k_w, cells=pb.inside, rules=pb.vol, qdegree=2, coefficients=(B,))], pb.P1)
    a_c = fem.form([fem.Integral(k_c, cells=pb.inside, rules=pb.vol, qdegree=2, params=beta)], pb.P1)
    A_w, A_c = fem.assemble_matrix(a_w), fem.assemble_matrix(a_c)
    assert np.array_equal(A_w.indptr, A_c.indptr) and np.array_equal(A_w.indices, A_c.indices)
    assert np.abs(A_c.data).max() > 1e-3 and rel_err(A_w.data, A_c.data) < 1e-13


@pytest.mark.gpu
def test_lifting_through_a_coefficient_list_equals_b_minus_A_g(problem):
    """b - alpha A (g - x0) on the Dirichlet columns, from the form's own assembled matrix.  Bound: every entry sums at
    most the row's products in another order and from local tensors summed in another order -- 64 eps times the
    largest sum of |A_ij| |alpha (g - x0)_j| over the rows, relative to the result."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem
    kappa = cfx.Function(pb.P2p, pb.permuted(_smooth(pb.x2)))
    ks = fem.register_integrand("user_kappa_stiffness", KAPPA_STIFFNESS_SRC, variant=(pb.tdim, pb.p1, 1),
                                coefficients=[(pb.p2, 1)])
    a = fem.form([fem.Integral(ks, cells=pb.inside, rules=pb.vol, qdegree=2, coefficients=(kappa,))], pb.P1)
    A = fem.assemble_matrix(a).to_scipy()
    rng = np.random.default_rng(4)
    N = pb.P1.ndofs
    bc = (rng.random(N) < 0.3).astype(np.int8)
    g, x0, b0 = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)
    d = np.where(bc != 0, 0.7 * (g - x0), 0.0)
    want = b0 - A @ d
    got = fem.apply_lifting(b0.copy(), a, bc, g, x0=x0, alpha=0.7)
    bound = 64 * np.finfo(np.float64).eps * (abs(A) @ np.abs(d)).max() / np.abs(want).max()
    assert rel_err(got, b0) > 1e-6 and bound < 1e-12
    assert rel_err(got, want) < bound


@pytest.mark.gpu
def test_a_live_form_takes_new_values_without_a_read_back(problem):
    import cutfemx_amd as cfx
    from cutfemx_amd import _lib, fem
    pb = problem
    k_p2, _, _, form_of = _kf_forms(pb, fem, cfx)
    kap, f2 = _smooth(pb.x1), pb.permuted(_smooth(pb.x2))
    K, F = cfx.Function(pb.P1b, kap), cfx.Function(pb.P2p, f2)
    L = form_of(k_p2, pb.P2, (K, F))
    b1 = fem.assemble_vector(L)
    s0 = _lib.sync_count()
    b1b = fem.assemble_vector(L)
    without = _lib.sync_count() - s0
    s0 = _lib.sync_count()
    L.set_coefficients(0, (cfx.Function(pb.P1b, 2.0 * kap), F))
    b2 = fem.assemble_vector(L)
    with_setter = _lib.sync_count() - s0
    assert with_setter == without
    assert np.abs(b1).max() > 1e-6 and rel_err(b1b, b1) < 1e-13 and rel_err(b2, 2.0 * b1) < 1e-13
    # a bilinear form created without a list (w = NULL: kappa = 1) takes one, then another, and n = 0 restores it
    V, kappa, twin = _space_and_twin(pb, 2)
    ks = fem.register_integrand("user_kappa_stiffness", KAPPA_STIFFNESS_SRC, variant=(pb.tdim, pb.p2, 1), coefficients=[(pb.p2, 1)])

    def builtin(fn):
        return fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=pb.inside, rules=pb.vol, qdegree=2,
                                                          coefficient=fn)], V)).data
    a = fem.form([fem.Integral(ks, cells=pb.inside, rules=pb.vol, qdegree=2)], V)
    A0 = fem.assemble_matrix(a).data.copy()
    assert rel_err(A0, builtin(None)) < 1e-13
    a.set_coefficients(0, (twin,))
    A1 = fem.assemble_matrix(a).data.copy()
    assert rel_err(A1, builtin(kappa)) < 1e-13 and rel_err(A1, A0) > 1e-3
    a.set_coefficients(0, (cfx.Function(pb.P2p, 2.0 * twin.values),))
    assert rel_err(fem.assemble_matrix(a).data, 2.0 * A1) < 1e-13
    a.set_coefficients(0, ())
    assert rel_err(fem.assemble_matrix(a).data, A0) < 1e-13


@pytest.mark.gpu
def test_float32_and_complex_containers_carry_the_list(problem):
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem
    k_p2, _, _, form_of = _kf_forms(pb, fem, cfx)
    kap, f2 = _smooth(pb.x1), pb.permuted(_smooth(pb.x2))
    K, F = cfx.Function(pb.P1b, kap), cfx.Function(pb.P2p, f2)
    L = form_of(k_p2, pb.P2, (K, F))
    b = fem.assemble_vector(L)
    b32 = fem.assemble_vector(L, dtype=np.float32)
    assert np.asarray(b32).dtype == np.float32 and rel_err(b32, b) < 1e-6
    # complex128: one real list under two complex constants (the integrals are assembled as two real sub-forms)
    par = (0.0, 1.5)
    Lc = fem.form([fem.Integral(k_p2, cells=pb.inside, qdegree=4, params=par, coefficients=(K, F)),
                   fem.Integral(k_p2, rules=pb.vol, params=par, coefficients=(K, F), scale=2.0j)], pb.P2, dtype=np.complex128)
    parts = [fem.assemble_vector(fem.form([fem.Integral(k_p2, cells=pb.inside, qdegree=4, params=par, coefficients=(K, F))], pb.P2)),
             fem.assemble_vector(fem.form([fem.Integral(k_p2, rules=pb.vol, params=par, coefficients=(K, F))], pb.P2))]
    bc = np.asarray(fem.assemble_vector(Lc))
    assert np.iscomplexobj(bc) and np.abs(parts[1]).max() > 1e-8
    assert rel_err(bc.real, parts[0]) < 1e-13 and rel_err(bc.imag, 2.0 * parts[1]) < 1e-13
    # ... and the sub-forms follow an update of the live form
    Lc.set_coefficients(1, (cfx.Function(pb.P1b, 3.0 * kap), F))
    bc = np.asarray(fem.assemble_vector(Lc))
    assert rel_err(bc.real, parts[0]) < 1e-13 and rel_err(bc.imag, 6.0 * parts[1]) < 1e-13


@pytest.mark.gpu
def test_refused_lists_leave_the_device_clean(problem3, oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    pb = problem3
    ks = fem.register_integrand("user_kappa_stiffness", KAPPA_STIFFNESS_SRC, variant=(3, 4, 1), coefficients=[(4, 1)])
    k1, k2 = cfx.Function(pb.P1b, _smooth(pb.x1)), cfx.Function(pb.P2p, pb.permuted(_smooth(pb.x2)))

    def form_of(k, fs):
        return fem.form([fem.Integral(k, cells=pb.inside, rules=pb.vol, qdegree=2, coefficients=fs)], pb.P1)
    with pytest.raises(ValueError, match="registered integrand"):      # a built-in id keeps its single coefficient
        form_of(fem.STIFFNESS, (k1,))
    om2 = oracle.mesh_box(3, 2)
    other = cfx.FunctionSpace(cfx.Mesh.from_arrays(3, om2.x, om2.conn), 1)
    with pytest.raises(ValueError, match="another mesh"):
        form_of(ks, (cfx.Function(other, np.ones(om2.nnodes)),))
    with pytest.raises(ValueError, match="at most 8"):
        form_of(ks, (k1,) * 9)
    with pytest.raises(ValueError, match="differ from the signatures"):   # compiled for [(4, 1)], given a P2 Function
        form_of(ks, (k2,))
    with pytest.raises(ValueError, match="complex"):
        form_of(ks, (cfx.Function(pb.P1b, _smooth(pb.x1) * (1.0 + 1.0j)),))
    a = form_of(ks, (k1,))
    with pytest.raises(ValueError, match="differ from the signatures"):   # ... and on the live form, which keeps its list
        a.set_coefficients(0, (k1, k2))
    with pytest.raises(ValueError, match="out of range"):
        a.set_coefficients(3, (k1,))
    A = fem.assemble_matrix(a)
    ref = fem.assemble_matrix(fem.form([fem.Integral(fem.STIFFNESS, cells=pb.inside, rules=pb.vol, qdegree=2,
                                                     coefficient=cfx.Function(pb.P1, _smooth(pb.x1)))], pb.P1))
    assert rel_err(A.data, ref.data) < 1e-13
    torch.cuda.synchronize()
