"""Registered integrands between two spaces (cfx_integrand_register2), registered interior-facet integrals over
facet-hosted rules, and lifting through registered integrands: the hipRTC counterpart of the reference's generated
kernels for every integral of every form (Form.h:59-75, python/cutfemx/_runintgen_adapter.py:181-217).  Compilation
targets gfx950 and needs no GPU; the parity tests against the built-in ids run on the GPU."""
import numpy as np
import pytest

from helpers import level_set_values, rel_err

# -c0 (div v, p): vector test space (CFX_BS0 = tdim), scalar trial space -- the built-in CFX_K_DIV_TEST
DIV_TEST_SRC = r"""
__device__ void user_div_test(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                              const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND0], dN0[CFX_ND0][CFX_TDIM], N1[CFX_ND1], dN1[CFX_ND1][CFX_TDIM];
    cfx_tabulate0(points + q * CFX_TDIM, N0, dN0);
    cfx_tabulate1(points + q * CFX_TDIM, N1, dN1);
    for (int i = 0; i < CFX_ND0; ++i)
      for (int a = 0; a < CFX_BS0; ++a)
      {
        double g = 0.0;
        for (int t = 0; t < CFX_TDIM; ++t) g += dN0[i][t] * K[t][a];
        for (int j = 0; j < CFX_ND1; ++j) A[(i * CFX_BS0 + a) * CFX_NDB1 + j] += weights[q] * c[0] * g * N1[j];
      }
  }
}
"""

# c0 (q, div u): scalar test space, vector trial space -- the built-in CFX_K_DIV_TRIAL
DIV_TRIAL_SRC = r"""
__device__ void user_div_trial(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                               const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND0], dN0[CFX_ND0][CFX_TDIM], N1[CFX_ND1], dN1[CFX_ND1][CFX_TDIM];
    cfx_tabulate0(points + q * CFX_TDIM, N0, dN0);
    cfx_tabulate1(points + q * CFX_TDIM, N1, dN1);
    for (int j = 0; j < CFX_ND1; ++j)
      for (int b = 0; b < CFX_BS1; ++b)
      {
        double g = 0.0;
        for (int t = 0; t < CFX_TDIM; ++t) g += dN1[j][t] * K[t][b];
        for (int i = 0; i < CFX_ND0; ++i) A[i * CFX_NDB1 + j * CFX_BS1 + b] += weights[q] * c[0] * N0[i] * g;
      }
  }
}
"""

# (u, v) + (grad u, grad v) selected by c[0] (0: mass, 1: stiffness) between two scalar spaces
MASS_STIFF2_SRC = r"""
__device__ void user_ms2(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                         const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND0], dN0[CFX_ND0][CFX_TDIM], N1[CFX_ND1], dN1[CFX_ND1][CFX_TDIM];
    cfx_tabulate0(points + q * CFX_TDIM, N0, dN0);
    cfx_tabulate1(points + q * CFX_TDIM, N1, dN1);
    for (int i = 0; i < CFX_ND0; ++i)
      for (int j = 0; j < CFX_ND1; ++j)
      {
        double v = N0[i] * N1[j];
        if (c[0] != 0.0)
        {
          v = 0.0;
          for (int d = 0; d < CFX_TDIM; ++d)
          {
            double gi = 0.0, gj = 0.0;
            for (int t = 0; t < CFX_TDIM; ++t) { gi += dN0[i][t] * K[t][d]; gj += dN1[j][t] * K[t][d]; }
            v += gi * gj;
          }
        }
        A[i * CFX_NDB1 + j] += weights[q] * v;
      }
  }
}
"""

# gamma / h_avg [v][u] between two scalar spaces: the built-in CFX_K_JUMP on cfx_form_create2 forms
JUMP2_SRC = r"""
__device__ void user_jump2(double* A, const double* w, const double* c, const double* coordinate_dofs,
                           const int* entity_local_index, int nq, const double* points0, const double* points1,
                           const double* weights)
{
  const double* x0 = coordinate_dofs;
  const double* x1 = coordinate_dofs + (CFX_TDIM + 1) * 3;
  const double h = 0.5 * (cfx_cell_diameter(x0) + cfx_cell_diameter(x1));
  for (int q = 0; q < nq; ++q)
  {
    double Na[CFX_ND0], Nb[CFX_ND0], Ma[CFX_ND1], Mb[CFX_ND1], dN0[CFX_ND0][CFX_TDIM], dN1[CFX_ND1][CFX_TDIM];
    double jt[2 * CFX_ND0], ju[2 * CFX_ND1];
    cfx_tabulate0(points0 + q * CFX_TDIM, Na, dN0);
    cfx_tabulate0(points1 + q * CFX_TDIM, Nb, dN0);
    cfx_tabulate1(points0 + q * CFX_TDIM, Ma, dN1);
    cfx_tabulate1(points1 + q * CFX_TDIM, Mb, dN1);
    for (int i = 0; i < CFX_ND0; ++i) { jt[i] = Na[i]; jt[CFX_ND0 + i] = -Nb[i]; }
    for (int j = 0; j < CFX_ND1; ++j) { ju[j] = Ma[j]; ju[CFX_ND1 + j] = -Mb[j]; }
    for (int i = 0; i < 2 * CFX_ND0; ++i)
      for (int j = 0; j < 2 * CFX_ND1; ++j) A[i * (2 * CFX_NDB1) + j] += weights[q] * c[0] / h * jt[i] * ju[j];
  }
}
"""

# symmetric interior penalty -{dn u}[v] - {dn v}[u] + c0 / h_avg [u][v] (the built-in CFX_K_SIP, scalar space)
SIP_SRC = r"""
__device__ void user_sip(double* A, const double* w, const double* c, const double* coordinate_dofs,
                         const int* entity_local_index, int nq, const double* points0, const double* points1,
                         const double* weights)
{
  const double* x0 = coordinate_dofs;
  const double* x1 = coordinate_dofs + (CFX_TDIM + 1) * 3;
  double K0[CFX_TDIM][CFX_TDIM], K1[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(x0, K0);
  (void)cfx_inverse_jacobian(x1, K1);
  const double h = 0.5 * (cfx_cell_diameter(x0) + cfx_cell_diameter(x1));
  const int lf0 = entity_local_index[0];
  double nrm[CFX_TDIM], nn = 0.0;
  for (int d = 0; d < CFX_TDIM; ++d)
  {
    double v = 0.0;
    for (int t = 0; t < CFX_TDIM; ++t) v -= K0[t][d] * (lf0 == 0 ? -1.0 : (lf0 - 1 == t ? 1.0 : 0.0));
    nrm[d] = v; nn += v * v;
  }
  nn = sqrt(nn);
  for (int d = 0; d < CFX_TDIM; ++d) nrm[d] /= nn;
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND], dN0[CFX_ND][CFX_TDIM], N1[CFX_ND], dN1[CFX_ND][CFX_TDIM], v[2 * CFX_ND], av[2 * CFX_ND];
    cfx_tabulate(points0 + q * CFX_TDIM, N0, dN0);
    cfx_tabulate(points1 + q * CFX_TDIM, N1, dN1);
    for (int j = 0; j < CFX_ND; ++j)
    {
      double a = 0.0, b = 0.0;
      for (int d = 0; d < CFX_TDIM; ++d)
        for (int t = 0; t < CFX_TDIM; ++t) { a += K0[t][d] * dN0[j][t] * nrm[d]; b += K1[t][d] * dN1[j][t] * nrm[d]; }
      v[j] = N0[j]; v[CFX_ND + j] = -N1[j];
      av[j] = 0.5 * a; av[CFX_ND + j] = 0.5 * b;
    }
    for (int i = 0; i < 2 * CFX_ND; ++i)
      for (int j = 0; j < 2 * CFX_ND; ++j)
        A[i * 2 * CFX_ND + j] += weights[q] * (-av[j] * v[i] - av[i] * v[j] + c[0] / h * v[i] * v[j]);
  }
}
"""


def test_two_space_sources_compile_for_gfx950_without_a_gpu():
    from cutfemx_amd import fem
    kdt = fem.register_integrand("user_div_test", DIV_TEST_SRC, variant=(2, 6, 2, 3, 1))      # P2 vector x P1
    kdr = fem.register_integrand("user_div_trial", DIV_TRIAL_SRC, variant=(3, 4), trial=(10, 3))
    kms = fem.register_integrand("user_ms2", MASS_STIFF2_SRC, variant=(2, 3, 1, 6, 1))       # P1 x P2
    kj = fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(2, 3, 1, 6, 1))
    assert len({kdt, kdr, kms, kj}) == 4 and min(kdt, kdr, kms, kj) >= 1000
    for tdim in (2, 3):
        p1, p2 = tdim + 1, (tdim + 1) * (tdim + 2) // 2
        fem.compile_integrand2(kdt, tdim, p2, tdim, p1, 1)
        fem.compile_integrand2(kdr, tdim, p1, 1, p2, tdim)
        fem.compile_integrand2(kms, tdim, p2, 1, p1, 1)
        fem.compile_integrand2(kj, tdim, p1, 1, p2, 1)
    # a square source (CFX_ND, cfx_tabulate) names one space: not defined in a two-space variant
    with pytest.raises(ValueError, match="does not compile"):
        fem.register_integrand("user_sip", SIP_SRC, facet=True, variant=(2, 3, 1, 3, 1))
    # a source written for another shape is refused with the compiler's log
    bad = DIV_TEST_SRC.replace("double K[CFX_TDIM][CFX_TDIM];", "static_assert(CFX_NDB1 == 4, \"trial shape\");\n  double K[CFX_TDIM][CFX_TDIM];")
    with pytest.raises(ValueError, match="trial shape"):
        fem.register_integrand("user_div_test", bad, variant=(2, 6, 2, 3, 1))
    # the variant must name two Lagrange spaces; more than 24 macro dofs on a facet is refused
    with pytest.raises(ValueError, match="variant"):
        fem.register_integrand("user_ms2", MASS_STIFF2_SRC, variant=(2, 5, 1, 3, 1))
    with pytest.raises(ValueError, match="24 macro dofs"):
        fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(3, 10, 3, 4, 1))
    with pytest.raises(ValueError, match="bilinear"):
        fem.register_integrand("user_ms2", MASS_STIFF2_SRC, rank=1, variant=(2, 3, 1, 6, 1))
    with pytest.raises(ValueError, match="compile2"):
        fem.compile_integrand(kms, 2, 3)
    k_sq = fem.register_integrand("user_sip", SIP_SRC, facet=True, variant=(2, 3, 1))
    with pytest.raises(ValueError, match="square forms"):
        fem.compile_integrand2(k_sq, 2, 3, 1, 6, 1)


def _setup(oracle, tdim, n):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(tdim, n)
    phi = level_set_values(om.x, tdim)
    dm2, nd2 = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    sp = {"U": cfx.FunctionSpace(mesh, 2, dofmap=dm2, ndofs=nd2, bs=tdim),
          "S": cfx.FunctionSpace(mesh, 2, dofmap=dm2, ndofs=nd2),
          "P": cfx.FunctionSpace(mesh, 1)}
    cd = cfx.cut(cfx.Function(sp["P"], phi))
    return mesh, sp, cd


def _same(A, B):
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert rel_err(A.data, B.data) < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n", [(2, 10), (3, 5)])
def test_registered_two_space_cell_sources_equal_the_builtin_blocks(oracle, tdim, n, monkeypatch):
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    mesh, sp, cd = _setup(oracle, tdim, n)
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 4)
    p1, p2 = tdim + 1, (tdim + 1) * (tdim + 2) // 2
    kdt = fem.register_integrand("user_div_test", DIV_TEST_SRC, variant=(tdim, p2, tdim, p1, 1))
    kdr = fem.register_integrand("user_div_trial", DIV_TRIAL_SRC, variant=(tdim, p1, 1, p2, tdim))
    kms = fem.register_integrand("user_ms2", MASS_STIFF2_SRC, variant=(tdim, p1, 1, p2, 1))
    cases = [("U", "P", fem.DIV_TEST, kdt, (-1.0,), (-1.0,)), ("P", "U", fem.DIV_TRIAL, kdr, (-1.0,), (-1.0,)),
             ("P", "S", fem.MASS, kms, (), (0.0,)), ("P", "S", fem.STIFFNESS, kms, (), (1.0,))]

    def forms(t, s, k, par):
        return fem.form([fem.Integral(k, cells=inside, rules=vol, params=par, qdegree=3)], sp[t], trial_space=sp[s])
    for t, s, kb, ku, pb, pu in cases:
        a_ref, a_usr = forms(t, s, kb, pb), forms(t, s, ku, pu)
        A_ref = fem.assemble_matrix(a_ref)
        _same(fem.assemble_matrix(a_usr), A_ref)
        for idx, use_rule in ((0, False), (len(inside) // 2, False), (3, True)):
            ref = fem.tabulate_entity(a_ref, 0, idx, use_rule)
            got = fem.tabulate_entity(a_usr, 0, idx, use_rule)
            assert got.shape == ref.shape and rel_err(got, ref) < 1e-13
        # Dirichlet rows / columns of either space
        rng = np.random.default_rng(3)
        bc0 = (rng.random(sp[t].ndofs * sp[t].bs) < 0.1).astype(np.int8)
        bc1 = (rng.random(sp[s].ndofs * sp[s].bs) < 0.1).astype(np.int8)
        _same(fem.assemble_matrix(a_usr, bcs=(bc0, bc1)), fem.assemble_matrix(a_ref, bcs=(bc0, bc1)))
    monkeypatch.setenv("CFX_RECT_GATHER", "0")
    for t, s, kb, ku, pb, pu in cases:
        _same(fem.assemble_matrix(forms(t, s, ku, pu)), fem.assemble_matrix(forms(t, s, kb, pb)))


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n", [(2, 10), (3, 5)])
def test_registered_two_space_value_jump_equals_the_builtin(oracle, tdim, n):
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    mesh, _, cd = _setup(oracle, tdim, n)
    ghost = cfx.ghost_penalty_facets(cd, "phi<0")
    p1, p2 = tdim + 1, (tdim + 1) * (tdim + 2) // 2
    # discontinuous spaces (every cell owns its dofs): the jumps of continuous spaces cancel in the assembled matrix
    nc = mesh.num_cells
    sp = {"P": cfx.FunctionSpace(mesh, 1, dofmap=np.arange(nc * p1, dtype=np.int32).reshape(nc, p1), ndofs=nc * p1),
          "S": cfx.FunctionSpace(mesh, 2, dofmap=np.arange(nc * p2, dtype=np.int32).reshape(nc, p2), ndofs=nc * p2)}
    kj = fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(tdim, p1, 1, p2, 1))
    for t, s in (("P", "S"), ("S", "P")):
        if t == "S":
            kj = fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(tdim, p2, 1, p1, 1))

        def form_of(k):
            return fem.form([fem.Integral(k, facets=ghost, params=(5.0,), qdegree=3)], sp[t], trial_space=sp[s])
        a_ref, a_usr = form_of(fem.JUMP), form_of(kj)
        A_ref = fem.assemble_matrix(a_ref)
        assert np.abs(A_ref.data).max() > 1e-3
        _same(fem.assemble_matrix(a_usr), A_ref)
        for f in (0, ghost.size // 2, ghost.size - 1):
            assert rel_err(fem.tabulate_entity(a_usr, 0, f, False), fem.tabulate_entity(a_ref, 0, f, False)) < 1e-13


def _dg_sip_forms(tdim, n, degree):
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    mesh = cfx.Mesh.create_box(tdim, n)
    P1 = cfx.FunctionSpace(mesh, 1)
    phi = np.sqrt(((mesh.x[:, :tdim] - 0.5) ** 2).sum(axis=1)) - 0.37
    return poisson.build_dg_forms(cfx.Function(P1, phi), degree)


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n,degree", [(2, 12, 1), (2, 8, 2), (3, 5, 1), (3, 4, 2)])
def test_registered_sip_over_facet_hosted_rules_equals_fem_sip(tdim, n, degree, monkeypatch):
    """The cut DG skeleton of build_dg_forms -- [skeleton facets inside, rules of the cut skeleton facets] -- with a
    registered SIP source: equal to fem.SIP on the matrix and on single entities past the standard facets; and the
    lifting through it equals the built-in lifting."""
    from cutfemx_amd import fem
    system = _dg_sip_forms(tdim, n, degree)
    V = system.function_space
    nd = V.ndofs_cell
    k = fem.register_integrand("user_sip", SIP_SRC, facet=True, variant=(tdim, nd, 1))
    sigma = 10.0 * degree * degree

    def form_of(kern):
        return fem.form([fem.Integral(fem.STIFFNESS, rules=system.volume_rules, qdegree=2 * (degree - 1)),
                         fem.Integral(kern, facets=system.omega_facets, rules=system.facet_rules, params=(sigma,),
                                      qdegree=2 * degree)], V)
    a_ref, a_usr = form_of(fem.SIP), form_of(k)
    _same(fem.assemble_matrix(a_usr), fem.assemble_matrix(a_ref))
    n_std = len(system.omega_facets)
    n_all = n_std + system.facet_rules.num_rules
    assert n_all > n_std
    for f in (0, n_std - 1, n_std, (n_std + n_all) // 2, n_all - 1):
        assert rel_err(fem.tabulate_entity(a_usr, 1, f, False), fem.tabulate_entity(a_ref, 1, f, False)) < 1e-13
    rng = np.random.default_rng(7)
    N = V.ndofs
    bc = (rng.random(N) < 0.15).astype(np.int8)
    g, x0, b0 = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)
    want = fem.apply_lifting(b0.copy(), a_ref, bc, g, x0=x0, alpha=0.7)
    got = fem.apply_lifting(b0.copy(), a_usr, bc, g, x0=x0, alpha=0.7)
    assert rel_err(got, want) < 1e-13
    monkeypatch.setenv("CFX_ASSEMBLY", "atomic")
    _same(fem.assemble_matrix(form_of(k)), fem.assemble_matrix(form_of(fem.SIP)))


STIFFNESS_SRC = r"""
__device__ void user_stiffness(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                               const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], g[CFX_ND][CFX_TDIM];
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
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
        A[i * CFX_ND + j] += weights[q] * v;
      }
  }
}
"""


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n", [(2, 12), (3, 5)])
def test_lifting_through_registered_integrands_equals_the_builtin(oracle, tdim, n):
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    mesh, sp, cd = _setup(oracle, tdim, n)
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 4)
    p1, p2 = tdim + 1, (tdim + 1) * (tdim + 2) // 2
    ks = fem.register_integrand("user_stiffness", STIFFNESS_SRC, variant=(tdim, p1, 1))
    kdr = fem.register_integrand("user_div_trial", DIV_TRIAL_SRC, variant=(tdim, p1, 1, p2, tdim))
    rng = np.random.default_rng(11)
    for t, s, kb, ku, par in (("P", "P", fem.STIFFNESS, ks, ()), ("P", "U", fem.DIV_TRIAL, kdr, (-1.0,))):
        def form_of(k):
            return fem.form([fem.Integral(k, cells=inside, rules=vol, params=par, qdegree=3)], sp[t],
                            trial_space=None if s == t else sp[s])
        n0, n1 = sp[t].ndofs * sp[t].bs, sp[s].ndofs * sp[s].bs
        bc = (rng.random(n1) < 0.1).astype(np.int8)
        g, x0, b0 = rng.standard_normal(n1), rng.standard_normal(n1), rng.standard_normal(n0)
        want = fem.apply_lifting(b0.copy(), form_of(kb), bc, g, x0=x0, alpha=1.3)
        got = fem.apply_lifting(b0.copy(), form_of(ku), bc, g, x0=x0, alpha=1.3)
        assert rel_err(got, want) < 1e-13
        assert rel_err(got, b0) > 1e-6      # (the lifting did something)


@pytest.mark.gpu
def test_two_space_refusals_leave_no_hip_error(oracle):
    import torch
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    tdim = 3
    mesh, sp, cd = _setup(oracle, tdim, 3)
    inside = cfx.locate_entities(cd, "phi<0")
    ghost = cfx.ghost_penalty_facets(cd, "phi<0")
    ks = fem.register_integrand("user_stiffness", STIFFNESS_SRC, variant=(3, 4, 1))
    kms = fem.register_integrand("user_ms2", MASS_STIFF2_SRC, variant=(3, 4, 1, 10, 1))
    kj = fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(3, 4, 1, 10, 1))
    # a square id on a two-space form, and the reverse
    with pytest.raises(ValueError, match="registered for a square form"):
        fem.form([fem.Integral(ks, cells=inside, qdegree=2)], sp["P"], trial_space=sp["S"])
    with pytest.raises(ValueError, match="cfx_integrand_register2"):
        fem.form([fem.Integral(kms, cells=inside, qdegree=2)], sp["P"])
    # a coefficient on the trial space
    with pytest.raises(ValueError, match="test space"):
        fem.form([fem.Integral(kms, cells=inside, qdegree=2, coefficient=cfx.Function(sp["S"]))], sp["P"], trial_space=sp["S"])
    # a wrong variant
    with pytest.raises(ValueError, match="variant"):
        fem.register_integrand("user_ms2", MASS_STIFF2_SRC, variant=(3, 4, 1, 7, 1))
    # more than 24 macro dofs: the P2 vector space in 3-D has 2 x 30
    with pytest.raises(ValueError, match="24 macro dofs"):
        fem.form([fem.Integral(kj, facets=ghost, qdegree=2)], sp["P"], trial_space=sp["U"])
    # a coefficient packed with the test space is accepted; the device is clean after the refusals
    a = fem.form([fem.Integral(kms, cells=inside, qdegree=2, params=(0.0,), coefficient=cfx.Function(sp["P"]))], sp["P"],
                 trial_space=sp["S"])
    A = fem.assemble_matrix(a)
    assert np.isfinite(A.data).all()
    torch.cuda.synchronize()


# interface coupling of block (a, b) of the two-field interface problem on phi = 0, normals in point_data:
# -0.5 kb dn(u_b) s_a v_a - 0.5 ka dn(v_a) s_b u_b + eta / h s_a s_b u_b v_a, c = (ka, kb, s_a, s_b, eta).  One text for
# the square blocks (CFX_ND) and the two-space ones (CFX_ND0 / CFX_ND1)
COUPLING_SRC = r"""
#ifdef CFX_ND0
#define CPL_NA CFX_ND0
#define CPL_NB CFX_ND1
#define CPL_TAB_A cfx_tabulate0
#define CPL_TAB_B cfx_tabulate1
#else
#define CPL_NA CFX_ND
#define CPL_NB CFX_ND
#define CPL_TAB_A cfx_tabulate
#define CPL_TAB_B cfx_tabulate
#endif
__device__ void user_coupling(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                              const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  const double h = cfx_cell_diameter(coordinate_dofs);
  for (int q = 0; q < nq; ++q)
  {
    double Na[CPL_NA], dNa[CPL_NA][CFX_TDIM], Nb[CPL_NB], dNb[CPL_NB][CFX_TDIM], ga[CPL_NA], gb[CPL_NB];
    CPL_TAB_A(points + q * CFX_TDIM, Na, dNa);
    CPL_TAB_B(points + q * CFX_TDIM, Nb, dNb);
    const double* n = point_data + q * CFX_TDIM;
    for (int i = 0; i < CPL_NA; ++i)
    {
      ga[i] = 0.0;
      for (int d = 0; d < CFX_TDIM; ++d)
        for (int t = 0; t < CFX_TDIM; ++t) ga[i] += dNa[i][t] * K[t][d] * n[d];
    }
    for (int j = 0; j < CPL_NB; ++j)
    {
      gb[j] = 0.0;
      for (int d = 0; d < CFX_TDIM; ++d)
        for (int t = 0; t < CFX_TDIM; ++t) gb[j] += dNb[j][t] * K[t][d] * n[d];
    }
    for (int i = 0; i < CPL_NA; ++i)
      for (int j = 0; j < CPL_NB; ++j)
        A[i * CPL_NB + j] += weights[q] * (-0.5 * c[1] * gb[j] * c[2] * Na[i] - 0.5 * c[0] * ga[i] * c[3] * Nb[j]
                                           + c[4] / h * c[2] * c[3] * Na[i] * Nb[j]);
  }
}
"""


def test_interface_coupling_source_compiles_for_both_shapes_without_a_gpu():
    from cutfemx_amd import fem
    k2 = fem.register_integrand("user_coupling", COUPLING_SRC, variant=(2, 3, 1, 3, 1))
    k1 = fem.register_integrand("user_coupling", COUPLING_SRC, variant=(2, 3, 1))
    fem.compile_integrand2(k2, 3, 4, 1, 4, 1)
    fem.compile_integrand(k1, 3, 4)
    with pytest.raises(ValueError, match="24 macro dofs"):
        fem.compile_integrand2(fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(2, 3, 1, 3, 1)),
                               3, 10, 3, 4, 1)


def _p1_pair(mesh):
    """Two P1 space objects over the same dofmap (the sub-spaces of MixedSpace([P1, P1])): their forms are two-space."""
    import cutfemx_amd as cfx
    nc, nd = mesh.num_cells, mesh.tdim + 1
    conn = np.ascontiguousarray(mesh.conn, dtype=np.int32)
    return cfx.FunctionSpace(mesh, 1), cfx.FunctionSpace(mesh, 1, dofmap=conn, ndofs=mesh.num_nodes), nc, nd


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n", [(2, 12), (3, 5)])
def test_interface_coupling_with_point_data_on_two_space_blocks(oracle, tdim, n, monkeypatch):
    """The interface normal reaches a two-space integrand through point_data on cut-cell rules: the (0, 1) / (1, 0)
    blocks between two P1 space objects equal the same source on one space, block (0, 1) = block (1, 0)^T, on the row
    gather, the scatter and per entity; bitwise repeatable with CFX_DETERMINISTIC=1."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    om = oracle.mesh_box(tdim, n)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V0, V1, _, nd = _p1_pair(mesh)
    cd = cfx.cut(cfx.Function(V0, level_set_values(om.x, tdim)))
    inside = cfx.locate_entities(cd, "phi<0")
    vol = cfx.runtime_quadrature(cd, "phi<0", 2)
    itf = cfx.runtime_quadrature(cd, "phi=0", 3)
    nrm = cfx.normal(cd, itf)
    k2 = fem.register_integrand("user_coupling", COUPLING_SRC, variant=(tdim, nd, 1, nd, 1))
    k1 = fem.register_integrand("user_coupling", COUPLING_SRC, variant=(tdim, nd, 1))
    ka, kb, eta = 1.0, 7.0, 20.0

    def block(k, a, b, W0, W1):
        par = ((ka, kb)[a], (ka, kb)[b], (1.0, -1.0)[a], (1.0, -1.0)[b], eta * kb)
        return fem.form([fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=0),
                         fem.Integral(k, rules=itf, point_data=nrm, params=par)], W0, trial_space=W1)
    for a, b in ((0, 1), (1, 0)):
        A2 = fem.assemble_matrix(block(k2, a, b, V0, V1)).to_scipy()
        A1 = fem.assemble_matrix(block(k1, a, b, V0, None)).to_scipy()
        assert abs(A2 - A1).max() < 1e-13 * abs(A1).max()
        for idx in (0, itf.num_rules // 2):
            got = fem.tabulate_entity(block(k2, a, b, V0, V1), 1, idx, True)
            ref = fem.tabulate_entity(block(k1, a, b, V0, None), 1, idx, True)
            assert rel_err(got, ref) < 1e-13
    B01 = fem.assemble_matrix(block(k2, 0, 1, V0, V1)).to_scipy()
    B10 = fem.assemble_matrix(block(k2, 1, 0, V1, V0)).to_scipy()
    assert abs(B01 - B10.T).max() < 1e-14 * abs(B01).max()
    # scatter path
    monkeypatch.setenv("CFX_RECT_GATHER", "0")
    S01 = fem.assemble_matrix(block(k2, 0, 1, V0, V1)).to_scipy()
    assert abs(S01 - B01).max() < 1e-13 * abs(B01).max()
    monkeypatch.delenv("CFX_RECT_GATHER")
    # one writer per row: bitwise repeatable
    monkeypatch.setenv("CFX_DETERMINISTIC", "1")
    f = block(k2, 0, 1, V0, V1)
    r1, r2 = fem.assemble_matrix(f).data, fem.assemble_matrix(f).data
    assert np.array_equal(r1, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("tdim,n,degree", [(2, 12, 1), (3, 4, 1), (2, 8, 2)])
def test_two_space_facet_integral_over_facet_hosted_rules(tdim, n, degree, monkeypatch):
    """A registered two-space value jump over the DG skeleton's [facets, facet-hosted rules] between two DG space objects
    with one dofmap equals the built-in CFX_K_JUMP on one space (square form over the same entities), per entity too,
    and its lifting equals the built-in lifting."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    system = _dg_sip_forms(tdim, n, degree)
    V = system.function_space
    nd = V.ndofs_cell
    mesh = V.mesh
    dm = np.arange(mesh.num_cells * nd, dtype=np.int32).reshape(mesh.num_cells, nd)
    W = cfx.FunctionSpace(mesh, degree, dofmap=dm, ndofs=V.ndofs)
    kj = fem.register_integrand("user_jump2", JUMP2_SRC, facet=True, variant=(tdim, nd, 1, nd, 1))

    def form_of(k, trial):
        return fem.form([fem.Integral(k, facets=system.omega_facets, rules=system.facet_rules, params=(5.0,),
                                      qdegree=2 * degree)], V, trial_space=trial)
    a_ref, a_usr = form_of(fem.JUMP, None), form_of(kj, W)
    R, U = fem.assemble_matrix(a_ref).to_scipy(), fem.assemble_matrix(a_usr).to_scipy()
    assert abs(R).max() > 1e-3 and abs(U - R).max() < 1e-13 * abs(R).max()
    n_std = len(system.omega_facets)
    n_all = n_std + system.facet_rules.num_rules
    for f in (0, n_std, n_all - 1):
        assert rel_err(fem.tabulate_entity(a_usr, 0, f, False), fem.tabulate_entity(a_ref, 0, f, False)) < 1e-13
    rng = np.random.default_rng(5)
    bc = (rng.random(V.ndofs) < 0.15).astype(np.int8)
    g, x0, b0 = rng.standard_normal(V.ndofs), rng.standard_normal(V.ndofs), rng.standard_normal(V.ndofs)
    want = fem.apply_lifting(b0.copy(), a_ref, bc, g, x0=x0, alpha=0.7)
    assert rel_err(fem.apply_lifting(b0.copy(), a_usr, bc, g, x0=x0, alpha=0.7), want) < 1e-13
