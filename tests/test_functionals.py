"""Functionals (rank-0 forms, cfx_assemble_scalar) as far as they go without a GPU: rank-0 sources compile for gfx950
with the block-sum ending of their wrapper, the ABI lists the new entry point, `fem.form` infers rank 0 and
`fem.assemble_scalar` names what it accepts.  The sources are shared with tests/test_gpu_functionals.py."""
import types

import pytest

# c[1] f: f = u_h (the packed coefficient) or 1 -- CFX_M_FIELD with CFX_F_COEFFICIENT / CFX_F_ONE
FIELD_SRC = r"""
__device__ void user_m_field(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                             const double* points, const double* weights, const double* point_data)
{
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], f = 1.0;
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    if (w)
    {
      f = 0.0;
      for (int j = 0; j < CFX_ND; ++j) f += N[j] * w[j * CFX_BS];
    }
    A[0] += c[1] * weights[q] * f;
  }
}
"""

# c[1] |u_h - c[2] prod sin(pi x_d)|^2, summed over the components (the analytic field acts on component 0) -- CFX_M_L2_DIFF
L2_SRC = r"""
__device__ void user_m_l2(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                          const double* points, const double* weights, const double* point_data)
{
  for (int q = 0; q < nq; ++q)
  {
    const double* X = points + q * CFX_TDIM;
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], g = 0.0;
    cfx_tabulate(X, N, dN);
    if (c[2] != 0.0)
    {
      double l0 = 1.0;
      for (int t = 0; t < CFX_TDIM; ++t) l0 -= X[t];
      g = c[2];
      for (int d = 0; d < CFX_TDIM; ++d)
      {
        double x = l0 * coordinate_dofs[d];
        for (int t = 0; t < CFX_TDIM; ++t) x += X[t] * coordinate_dofs[3 * (t + 1) + d];
        g *= sinpi(x);
      }
    }
    double s = 0.0;
    for (int b = 0; b < CFX_BS; ++b)
    {
      double u = 0.0;
      for (int j = 0; j < CFX_ND; ++j) u += N[j] * w[j * CFX_BS + b];
      if (b == 0) u -= g;
      s += u * u;
    }
    A[0] += c[1] * weights[q] * s;
  }
}
"""

# c[1] |grad u_h|^2, summed over the components -- CFX_M_H1_SEMI
H1_SRC = r"""
__device__ void user_m_h1(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                          const double* points, const double* weights, const double* point_data)
{
  double K[CFX_TDIM][CFX_TDIM];
  (void)cfx_inverse_jacobian(coordinate_dofs, K);
  for (int q = 0; q < nq; ++q)
  {
    double N[CFX_ND], dN[CFX_ND][CFX_TDIM], s = 0.0;
    cfx_tabulate(points + q * CFX_TDIM, N, dN);
    for (int b = 0; b < CFX_BS; ++b)
    {
      double gr[CFX_TDIM];
      for (int t = 0; t < CFX_TDIM; ++t)
      {
        gr[t] = 0.0;
        for (int j = 0; j < CFX_ND; ++j) gr[t] += dN[j][t] * w[j * CFX_BS + b];
      }
      for (int d = 0; d < CFX_TDIM; ++d)
      {
        double v = 0.0;
        for (int t = 0; t < CFX_TDIM; ++t) v += K[t][d] * gr[t];
        s += v * v;
      }
    }
    A[0] += c[1] * weights[q] * s;
  }
}
"""

# c[0] / h_avg [u_h]^2 over an interior facet: u^T J u with J from CFX_K_JUMP; w = [2][ND]
FACET_JUMP_SRC = r"""
__device__ void user_m_jump(double* A, const double* w, const double* c, const double* coordinate_dofs,
                            const int* entity_local_index, int nq, const double* points0, const double* points1,
                            const double* weights)
{
  const double h = 0.5 * (cfx_cell_diameter(coordinate_dofs) + cfx_cell_diameter(coordinate_dofs + (CFX_TDIM + 1) * 3));
  for (int q = 0; q < nq; ++q)
  {
    double N0[CFX_ND], N1[CFX_ND], dN[CFX_ND][CFX_TDIM], jump = 0.0;
    cfx_tabulate(points0 + q * CFX_TDIM, N0, dN);
    cfx_tabulate(points1 + q * CFX_TDIM, N1, dN);
    for (int j = 0; j < CFX_ND; ++j) jump += N0[j] * w[j] - N1[j] * w[CFX_ND + j];
    A[0] += c[0] / h * weights[q] * jump * jump;
  }
}
"""

# c[1] (u1_h - u2_h)^2: two Functions on two spaces, coefficients 0 and 1 of the integral's list
TWO_SPACE_SRC = r"""
template <int ND>
__device__ inline double two_space_value(const double* X, const double* wk)
{
  double N[10], dN[10][CFX_TDIM];
  if constexpr (ND == CFX_TDIM + 1) cfx_tabulate_p1(X, N, dN); else cfx_tabulate_p2(X, N, dN);
  double v = 0.0;
  for (int j = 0; j < ND; ++j) v += N[j] * wk[j];
  return v;
}
__device__ void user_m_two(double* A, const double* w, const double* c, const double* coordinate_dofs, int nq,
                           const double* points, const double* weights, const double* point_data)
{
  static_assert(CFX_NCOEF == 2 && CFX_W_BS0 == 1 && CFX_W_BS1 == 1, "two scalar Functions");
  for (int q = 0; q < nq; ++q)
  {
    const double* X = points + q * CFX_TDIM;
    const double d = two_space_value<CFX_W_ND0>(X, w + CFX_W_OFF0) - two_space_value<CFX_W_ND1>(X, w + CFX_W_OFF1);
    A[0] += c[1] * weights[q] * d * d;
  }
}
"""

VARIANTS = [(2, 3), (2, 6), (3, 4), (3, 10)]


def test_rank0_sources_compile_for_gfx950_without_a_gpu():
    """Cell and interior-facet rank-0 integrands and one with a two-Function list, in every (tdim, dofs per cell)
    variant: each compilation goes through the predicate, the block sum and the partial store of the rank-0 wrapper."""
    from cutfemx_amd import fem
    ids = []
    for name, src in (("user_m_field", FIELD_SRC), ("user_m_l2", L2_SRC), ("user_m_h1", H1_SRC)):
        k = fem.register_integrand(name, src, rank=0)
        assert k >= 1000 and fem._user_integrand_rank[k] == 0
        for tdim, nd in VARIANTS:
            fem.compile_integrand(k, tdim, nd, 1)
        fem.compile_integrand(k, 2, 3, 2)        # vector-valued u_h
        ids.append(k)
    kf = fem.register_integrand("user_m_jump", FACET_JUMP_SRC, rank=0, facet=True)
    assert fem._user_integrand_rank[kf] == 0 and kf in fem._user_integrand_facet
    for tdim, nd in VARIANTS:
        fem.compile_integrand(kf, tdim, nd, 1)
    k2 = fem.register_integrand("user_m_two", TWO_SPACE_SRC, rank=0, variant=(2, 3, 1), coefficients=[(3, 1), (6, 1)])
    fem.compile_integrand(k2, 2, 6, 1, coefficients=[(3, 1), (6, 1)])
    fem.compile_integrand(k2, 3, 4, 1, coefficients=[(4, 1), (10, 1)])
    fem.compile_integrand(k2, 3, 10, 1, coefficients=[(4, 1), (10, 1)])
    kf2 = fem.register_integrand("user_m_jump", FACET_JUMP_SRC, rank=0, facet=True, variant=(2, 6, 1),
                                 coefficients=[(6, 1)])
    assert len(set(ids + [kf, k2, kf2])) == 6


def test_a_rank0_source_that_does_not_compile_is_refused_with_the_log():
    from cutfemx_amd import fem
    bad = FIELD_SRC.replace("A[0] +=", "A[0] += undeclared_scale *")
    with pytest.raises(ValueError, match="does not compile(.|\n)*undeclared_scale"):
        fem.register_integrand("user_m_field", bad, rank=0)
    # a linear interior-facet integrand still does not exist
    with pytest.raises(ValueError, match="bilinear"):
        fem.register_integrand("user_m_jump", FACET_JUMP_SRC, rank=1, facet=True, variant=(3, 4, 1))
    with pytest.raises(ValueError, match="rank must be 0, 1 or 2"):
        fem.register_integrand("user_m_field", FIELD_SRC, rank=3)


def test_abi_lists_assemble_scalar():
    from cutfemx_amd import _lib
    assert "cfx_assemble_scalar" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "cfx_assemble_scalar")
    assert (_lib.M_FIELD, _lib.M_L2_DIFF, _lib.M_H1_SEMI) == (201, 202, 203)


def test_form_infers_rank_0(monkeypatch):
    from cutfemx_amd import fem
    monkeypatch.setattr(fem, "CutForm", lambda V, integrals, rank, trial_space=None, dtype=None: rank)
    k0 = fem.register_integrand("user_m_field", FIELD_SRC, rank=0)
    assert fem.form([fem.Integral(fem.M_FIELD, params=(fem.F_ONE, 1.0))], None) == 0
    assert fem.form([fem.Integral(fem.M_L2_DIFF), fem.Integral(fem.M_H1_SEMI), fem.Integral(k0)], None) == 0
    assert fem.form([fem.Integral(fem.SOURCE)], None) == 1 and fem.form([fem.Integral(fem.MASS)], None) == 2
    with pytest.raises(ValueError, match="same rank"):
        fem.form([fem.Integral(fem.M_FIELD), fem.Integral(fem.SOURCE)], None)


def test_assemble_scalar_names_what_it_accepts():
    from cutfemx_amd import fem
    import numpy as np
    f64 = np.dtype(np.float64)
    bilinear = types.SimpleNamespace(rank=2, dtype=f64, integrals=[fem.Integral(fem.MASS)])
    linear = types.SimpleNamespace(rank=1, dtype=f64, integrals=[fem.Integral(fem.SOURCE), fem.Integral(fem.NITSCHE_RHS)])
    for M in (bilinear, linear):
        with pytest.raises(ValueError, match="rank-0 form(.|\n)*SOURCE"):
            fem.assemble_scalar(M)
