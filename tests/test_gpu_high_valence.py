"""Assembly on meshes with vertices of high valence.  Every other mesh of the suite is a Kuhn box mesh (or one renumbered
and jittered): a P1 vertex there has at most 7 (2-D) or 15 (3-D) stencil entries and the degree-2 lists come in one narrow
band of lengths, while the engine picks kernels, template instantiations and whole code paths from exactly those lengths
(cfx_rowasm.hip: space_stencil, the tile build, build_pattern; cfx_gather.hip: run_matrix, run_matrix_block,
assemble_matrix_rows).  The meshes here -- helpers.high_valence_case: a double cone whose two apexes see every base vertex,
joined with a small Kuhn box so that short and long rows go through the same launches -- put one shape on each side of
each of those edges.  tests/test_high_valence_reference.py pins the stencil and row lengths of every shape with the oracle
alone.  Each case compares with the oracle as the parity tests do: indptr / indices bit for bit, values and vectors to
1e-12 relative.

The edge of the P1 row stencil.  pattern_rows_kernel<4, 64> collects a vertex's list in a 64-slot hash set and reports
an overflow when the set comes out FULL (`cnt >= T`: a full table cannot be told from one that dropped a candidate), so
a list of 63 entries -- the vertex itself and 62 neighbours -- is the last one the stencil holds, and a list of 64 makes
space_stencil give up for the whole space (the hashed row sets, the searching kernels).  STENCIL_MAX below is that 63,
read from the kernel and not from a run; the shapes with apex stencils 63, 64 and 65 pin it."""
import os

import numpy as np
import pytest

from helpers import (HIGH_VALENCE_P1, HIGH_VALENCE_P2, high_valence_case, level_set_values, oracle_poisson,
                     oracle_stiffness_source, profiled, rel_err)

pytestmark = pytest.mark.gpu
RTOL = 1e-12
STENCIL_MAX = 63          # longest static P1 list (the vertex included) that space_stencil keeps

P1_SHAPES = [(2, 14), (2, 15), (2, 30), (2, 31), (2, 61), (2, 62), (2, 70),
             (3, (2, 4)), (3, (3, 3)), (3, (4, 4)), (3, (3, 7)), (3, (1, 30)), (3, (6, 8)), (3, (7, 7))]
MODE_SHAPES = [(3, (4, 4)), (3, (6, 6)), (2, 31)]                      # apex stencils 26, 50, 33
MODES = ["default", "CFX_DETERMINISTIC=1", "CFX_ROWS_SPLIT=1", "CFX_TILES=0", "CFX_PLAIN_STAGE=0", "CFX_STENCIL_STAGED=0",
         "CFX_STENCIL=0", "CFX_BULK_ROWS=0", "CFX_ASSEMBLY=atomic",
         # without the tiles the plain rows take assemble_rows_plain: its unstaged form on every stencil length, and its
         # ordered variants
         "CFX_TILES=0 CFX_PLAIN_STAGE=0", "CFX_TILES=0 CFX_DETERMINISTIC=1", "CFX_TILES=0 CFX_PLAIN_STAGE=0 CFX_DETERMINISTIC=1"]


def _id(v):
    return str(v).replace(", ", ",").replace(" ", "+").replace("CFX_", "")


def _setenv(monkeypatch, mode):
    for pair in ([] if mode == "default" else mode.split()):
        k, v = pair.split("=")
        monkeypatch.setenv(k, v)


def _foreign_switches():
    """Switches of the whole run (tools/test_modes.sh): the results hold under all of them, the kernel names of the
    default configuration do not."""
    return [k for k in os.environ if k.startswith("CFX_") and k not in ("CFX_STEP_DEBUG", "CFX_COUNT_SYNC", "CFX_DEVICE")]


_REFS = {}


def refs(O, tdim, shape, degree=1):
    """Mesh, level set and the two oracle systems of a shape: (a) the Poisson system (stiffness + Nitsche + ghost penalty,
    L), (b) the stiffness over the inside cells alone + the SOURCE / F_SINPROD form.  Computed once, never modified."""
    key = (tdim, shape, degree)
    if key not in _REFS:
        import cutfemx_amd as cfx
        om, phi, info = high_valence_case(O, tdim, shape)
        kw = {}
        if degree == 2:
            dofmap, ndofs = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, 2)
            kw = dict(degree=2, dofmap=dofmap, ndofs=ndofs)
        _REFS[key] = dict(om=om, phi=phi, info=info, tdim=tdim, degree=degree, kw=kw,
                          a=oracle_poisson(O, om, phi, **kw), b=oracle_stiffness_source(O, om, phi, **kw))
    return _REFS[key]


def engine(R):
    """A fresh mesh, space and cut (several switches are read when a space's tables are built)."""
    import cutfemx_amd as cfx
    om = R["om"]
    mesh = cfx.Mesh.from_arrays(R["tdim"], om.x, om.conn)
    V1 = cfx.FunctionSpace(mesh, 1)
    V = V1 if R["degree"] == 1 else cfx.FunctionSpace(mesh, 2, dofmap=R["kw"]["dofmap"], ndofs=R["kw"]["ndofs"])
    cd = cfx.cut(cfx.Function(V1, R["phi"]))
    return V, cd


def forms(V, cd, which):
    from cutfemx_amd import fem, poisson
    if which == "a":
        s = poisson.build_forms(V, cd, order=4)
        return s.a, s.L, s
    inside = cfx_inside(cd)
    a = fem.form([fem.Integral(fem.STIFFNESS, cells=inside, qdegree=2 * (V.degree - 1))], V)
    L = fem.form([fem.Integral(fem.SOURCE, cells=inside, params=(fem.F_SINPROD, 1.0), qdegree=4)], V, rank=1)
    return a, L, inside


def cfx_inside(cd):
    import cutfemx_amd as cfx
    return cfx.locate_entities_device(cd, "phi<0")


def check_system(O, R, which, a, L, tag, deterministic=False):
    """Everything the issue of a form pair is checked for, against the oracle system R[which]."""
    from cutfemx_amd import fem
    om, ref, info = R["om"], R[which], R["info"]
    oV, ip, ix = ref["V"], ref["indptr"], ref["indices"]
    A = fem.create_matrix(a)
    assert np.array_equal(A.indptr, ip) and A.indptr.dtype == np.int64, tag
    assert np.array_equal(A.indices, ix) and A.indices.dtype == np.int32, tag
    fem.assemble_matrix(a, A=A)
    e1 = rel_err(A.data, ref["values"])
    print(f"{tag}: A {e1:.2e}", end="")
    assert e1 < RTOL, tag
    fem.assemble_matrix(a, A=A)                       # a second assembly accumulates: twice the values
    assert rel_err(A.data, 2.0 * ref["values"]) < RTOL, tag
    b = fem.assemble_vector(L)
    eb = rel_err(b, ref["b"])
    print(f", b {eb:.2e}", end="")
    assert eb < RTOL, tag
    if deterministic:                                 # fixed summation orders: bit for bit between two assemblies
        assert np.array_equal(fem.assemble_matrix(a).data, fem.assemble_matrix(a).data), tag
        assert np.array_equal(fem.assemble_vector(L), b), tag
    # Dirichlet markers on random dofs and on both apexes
    rng = np.random.default_rng(7)
    n = oV.ndofs
    bc = (rng.random(n) < 0.1).astype(np.int8)
    bc[[info["lower_apex"], info["upper_apex"]]] = 1
    want = O.assemble_matrix(om, oV, ref["a"], ip, ix, bc0=bc, bc1=bc)
    B = fem.assemble_matrix(a, bcs=bc)
    ebc = rel_err(B.data, want)
    print(f", bcs {ebc:.2e}", end="")
    assert np.array_equal(B.indices, ix) and ebc < RTOL, tag
    g, x0, b0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    for alpha, x in ((1.0, None), (0.6, x0)):
        want = O.apply_lifting(om, oV, ref["a"], bc, g, b0.copy(), x0=x, alpha=alpha)
        got = fem.apply_lifting(b0.copy(), a, bc, g, x0=x, alpha=alpha)
        el = rel_err(got, want)
        print(f", lift {el:.2e}", end="")
        assert el < RTOL, tag
    # the active domain and the deactivation of the dofs outside it
    A1, b1 = fem.assemble_matrix(a), fem.assemble_vector(L)
    dom = fem.active_domain(a)
    assert np.array_equal(dom.active_cells, ref["active"]) and np.array_equal(dom.inactive_dofs, ref["inactive"]), tag
    fem.deactivate_outside(A1, b1, dom)
    vals, bb = ref["values"].copy(), ref["b"].copy()
    O.deactivate(ref["inactive"], ip, ix, vals, bb)
    assert rel_err(A1.data, vals) < RTOL and rel_err(b1, bb) < RTOL, tag
    print()
    return A


def stencil_expected(apex_len):
    return apex_len <= STENCIL_MAX and os.environ.get("CFX_STENCIL", "1")[:1] != "0"


@pytest.mark.parametrize("tdim,shape", P1_SHAPES, ids=_id)
def test_p1_every_stencil_class(oracle, tdim, shape):
    """Apex stencils 16 | 17 .. 32 | 33 .. 63 | 64, 65, 72: both sides of plain_cap 16 / 32 / 64, of the LDS staging of
    the plain rows (<= 32), of the 32- and 64-column forms of assemble_rows_p1 / assemble_rows_cut / assemble_rows, of the
    stencil's own capacity, and (2-D 62, 70; 3-D (6, 8), (7, 7)) of the 64 columns beyond which a P1 form leaves the split
    for assemble_rows_wide."""
    R = refs(oracle, tdim, shape)
    apex_len = HIGH_VALENCE_P1[(tdim, shape)][0]
    for which in ("a", "b"):
        V, cd = engine(R)
        assert V.static_table_bytes()["row_stencil"] == 0
        a, L, _keep = forms(V, cd, which)
        check_system(oracle, R, which, a, L, f"{tdim}d {shape} ({which})")
        built = V.static_table_bytes()["row_stencil"] > 0
        assert built == stencil_expected(apex_len), (apex_len, V.static_table_bytes())


@pytest.mark.parametrize("tdim,shape,cls", [(3, (2, 4), "<=16"), (3, (4, 4), "17-32"), (3, (6, 6), "33-63"), (3, (6, 8), "overflow"),
                                            (2, 31, "33-63"), (2, 62, "overflow")], ids=_id)
def test_p1_long_row_kernels_run(oracle, tdim, shape, cls, monkeypatch):
    """The long rows must be assembled by the kernels made for them, not by a fall back that happens to be right.  Form
    (b): every active row is a plain row (a subset of its stencil), the lower apex's a complete one.  Form (a) with
    CFX_ROWS_SPLIT=1 (on these meshes the interface rows are no minority, which the split otherwise waits for): lean kernel
    + cut kernel.  Beyond the stencil's capacity no plain-row kernel may run."""
    from cutfemx_amd import fem
    named = not _foreign_switches()                   # (a switch of the whole run: the results alone)
    R = refs(oracle, tdim, shape)
    _apex, longest_a, longest_b = HIGH_VALENCE_P1[(tdim, shape)]

    def run(which):
        V, cd = engine(R)
        a, L, _keep = forms(V, cd, which)
        A, names = profiled(lambda: fem.assemble_matrix(a))
        assert np.array_equal(A.indices, R[which]["indices"]) and rel_err(A.data, R[which]["values"]) < RTOL
        print(which, " ".join(sorted(names)))
        return names
    plain = ("assemble_rows_plain", "assemble_tiles_plain")
    names = run("b")
    if named and cls == "overflow":
        assert not any(k in names for k in plain), sorted(names)
        # the longest row holds 64 columns (the split's lean kernel in its 64-column form) or more (one wavefront per row)
        assert ("assemble_rows_p1" if longest_b <= 64 else "assemble_rows_wide") in names, sorted(names)
    elif named:
        # every tile of these meshes fits an LDS class of the tile kernel (the two apexes share a tile: 2 x 63 + 14 x 15
        # neighbour entries at the most): no silent drop from the tiles to the row-wise kernel
        assert "assemble_tiles_plain" in names and "assemble_rows_plain" not in names, sorted(names)
    names = run("a")                                  # the default configuration on the Poisson system
    if named and longest_a <= 64:
        # the whole cone (ghost penalty) and the box's band are interface rows, more than half of the active ones: the
        # split waits for them to be a minority (run_matrix: split_p1), so one searching kernel takes every row, in its
        # 32- or 64-column form by the longest row
        assert "assemble_rows" in names and "assemble_rows_p1" not in names and "assemble_rows_cut" not in names, sorted(names)
    elif named:
        assert "assemble_rows_wide" in names and "assemble_rows_p1" not in names, sorted(names)
    monkeypatch.setenv("CFX_TILES", "0")
    names = run("b")
    if named:
        assert ("assemble_rows_plain" in names) == (cls != "overflow") and "assemble_tiles_plain" not in names, sorted(names)
    monkeypatch.delenv("CFX_TILES")
    monkeypatch.setenv("CFX_ROWS_SPLIT", "1")
    names = run("a")
    if named and longest_a <= 64:
        assert "assemble_rows_p1" in names and "assemble_rows_cut" in names and "assemble_rows" not in names, sorted(names)
        assert any(k in names for k in plain) == (cls != "overflow"), sorted(names)
    elif named:                                       # a P1 row beyond 64 columns: no split, one wavefront per row
        assert "assemble_rows_wide" in names and "assemble_rows_p1" not in names, sorted(names)


@pytest.mark.parametrize("mode", MODES, ids=_id)
@pytest.mark.parametrize("tdim,shape", MODE_SHAPES, ids=_id)
def test_p1_modes(oracle, tdim, shape, mode, monkeypatch):
    _setenv(monkeypatch, mode)
    R = refs(oracle, tdim, shape)
    for which in ("a", "b"):
        V, cd = engine(R)
        a, L, _keep = forms(V, cd, which)
        check_system(oracle, R, which, a, L, f"{tdim}d {shape} ({which}) {mode}",
                     deterministic="CFX_DETERMINISTIC=1" in mode and os.environ.get("CFX_ASSEMBLY") != "atomic")


P2_CASES = [(m, mode) for m in (3, 4, 6, 7, 10) for mode in ("default", "CFX_ROWS_SPLIT=1")]
P2_CASES += [(m, mode) for m in (4, 6) for mode in ("CFX_P2_CLOSED=0", "CFX_P2_PLAIN=0", "CFX_P2_INTERFACE=0", "CFX_STENCIL_LISTS=0")]


@pytest.mark.parametrize("m,mode", P2_CASES, ids=_id)
def test_p2_scalar(oracle, m, mode, monkeypatch):
    """Degree 2 on the 3-D cone over an m x m base: apex lists of 66, 107, 219, 290, 563 dofs, one on each side of the 72
    and 128 columns of assemble_rows_p2_plain, the 255 of the slot records, and the 512 of the widest row set (stencil
    lists, pattern_rows_wide, the row gather); the Poisson rows (102 .. 685) cross the 64 / 128 / 256 classes of the hashed
    rows.  Beyond 511 columns the sparsity takes the 2048-slot set (pattern_rows_huge) and the entity-parallel kernels
    assemble: no row gather."""
    from cutfemx_amd import fem
    _setenv(monkeypatch, mode)
    R = refs(oracle, 3, (m, m), degree=2)
    assert (int(np.diff(R["a"]["indptr"]).max()), int(np.diff(R["b"]["indptr"]).max())) == HIGH_VALENCE_P2[m]
    for which in ("a", "b"):
        V, cd = engine(R)
        a, L, _keep = forms(V, cd, which)
        check_system(oracle, R, which, a, L, f"P2 m={m} ({which}) {mode}")
        if _foreign_switches() != ([] if mode == "default" else [mode.split("=")[0]]):
            continue
        V, cd = engine(R)
        a, L, _keep = forms(V, cd, which)
        A, names = profiled(lambda: fem.assemble_matrix(a))
        assert rel_err(A.data, R[which]["values"]) < RTOL
        gathered = any(k.startswith("assemble_rows") for k in names)
        longest = HIGH_VALENCE_P2[m][0 if which == "a" else 1]
        assert gathered == (longest <= 512), (longest, sorted(names))
        assert ("pattern_rows_huge" in names) == (longest > 511), (longest, sorted(names))


def _vector_refs(O, degree, m):
    key = ("vector", degree, m)
    if key not in _REFS:
        om, phi, info = high_valence_case(O, 3, (m, m))
        _REFS[key] = (om, phi, info)
    return _REFS[key]


VECTOR_MODES = ["default", "CFX_BLOCK_PLAIN=0", "CFX_BLOCK_GATHER=0", "CFX_MFMA=0", "CFX_P2_CLOSED=0"]


@pytest.mark.parametrize("mode", VECTOR_MODES, ids=_id)
@pytest.mark.parametrize("degree,m", [(1, 4), (1, 6), (1, 8), (2, 2), (2, 3), (2, 4)], ids=_id)
def test_vector_elasticity_with_ghost_penalty(oracle, degree, m, mode, monkeypatch):
    """bs = 3.  P1: 27, 51, 83 scalar columns per apex row (the 32 / 128 / 256 classes of assemble_rows_block).  P2: the
    longest static list is 65 (m = 2: a Kuhn-box vertex), 66 (m = 3) and 107 (m = 4) -- the closed-form and the staged
    plain block rows stop at lists of 72 -- and the scalar rows reach 102, 102 and 133."""
    import cutfemx_amd as cfx
    from test_gpu_spaces import elasticity_problem, setup
    _setenv(monkeypatch, mode)
    O = oracle
    om, phi, info = _vector_refs(O, degree, m)
    s = setup(O, 3, None, degree, 3, mesh_phi=(om, phi))
    oV = s["oV"]
    key = ("vector-system", degree, m)
    if key not in _REFS:
        inside, oa, ga = elasticity_problem(s, degree)
        ip, ix = O.create_sparsity(om, oV, oa)
        _REFS[key] = (oa, ip, ix, O.assemble_matrix(om, oV, oa, ip, ix))
    else:
        inside, _oa, ga = elasticity_problem(s, degree)
    oa, ip, ix, want = _REFS[key]
    a = cfx.fem.form(ga, s["V"])
    A = cfx.fem.create_matrix(a)
    assert np.array_equal(A.indptr, ip) and np.array_equal(A.indices, ix)
    cfx.fem.assemble_matrix(a, A=A)
    e = rel_err(A.data, want)
    print(f"vector P{degree} m={m} {mode}: A {e:.2e}, longest row {int(np.diff(ip).max())}")
    assert e < RTOL
    cfx.fem.assemble_matrix(a, A=A)
    assert rel_err(A.data, 2.0 * want) < RTOL
    rng = np.random.default_rng(5)
    ndofs = oV.ndofs * 3
    bc = (rng.random(ndofs) < 0.1).astype(np.int8)
    for apex in (info["lower_apex"], info["upper_apex"]):
        bc[3 * apex:3 * apex + 3] = 1
    wbc = O.assemble_matrix(om, oV, oa, ip, ix, bc, bc)
    assert rel_err(cfx.fem.assemble_matrix(a, bcs=bc).data, wbc) < RTOL
    g, b0 = rng.standard_normal(ndofs), rng.standard_normal(ndofs)
    wl = O.apply_lifting(om, oV, oa, bc, g, b0.copy())
    assert rel_err(cfx.fem.apply_lifting(b0.copy(), a, bc, g), wl) < RTOL


VEC_MODES = ["default", "CFX_VEC_BLOCKS=0", "CFX_VEC_BLOCKS=2", "CFX_VEC_ROWORDER=0", "CFX_SOURCE_SERIES=0", "CFX_SOURCE_GROUPS=0"]


@pytest.mark.parametrize("mode", VEC_MODES, ids=_id)
@pytest.mark.parametrize("shape", [(4, 4), (6, 6)], ids=_id)
def test_linear_forms(oracle, shape, mode, monkeypatch):
    """The series SOURCE term (with and without cut-cell rules) and NITSCHE_RHS on rows of 26 and 50 cells.  The hex-grouped
    source kernel needs a mesh made of Kuhn hexes, six cells each, all through (cfx_mesh.hip: hex_groups_check marks the
    whole mesh or nothing): a cone's cells are none, so neither the cone alone nor its union with a box may take it -- on
    (4, 4) the cell count is no multiple of six, on (6, 6) it is (528) and the check itself has to refuse."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    from helpers import cone_mesh
    _setenv(monkeypatch, mode)
    O = oracle
    R = refs(O, 3, shape)
    assert (R["om"].ncells % 6 == 0) == (shape == (6, 6))
    for which in ("a", "b"):
        V, cd = engine(R)
        a, L, _keep = forms(V, cd, which)
        b, names = profiled(lambda: fem.assemble_vector(L))
        e = rel_err(b, R[which]["b"])
        print(f"3d {shape} L({which}) {mode}: {e:.2e} {' '.join(sorted(names))}")
        assert e < RTOL
        assert "source_groups" not in names, sorted(names)
        b2 = fem.assemble_vector(L, b.copy())          # accumulates into the caller's vector
        assert rel_err(b2, 2.0 * R[which]["b"]) < RTOL
    # the cone alone (every cell inside below the level set's plane)
    cone = cone_mesh(3, (6, 6))                        # 144 cells = 24 x 6
    phi = cone.x[:, 2] - 0.75
    dom = O.classify(cone.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    assert len(inside) == 72
    oL = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, params=(O.F_SINPROD, 1.0), qdegree=4)]
    want = O.assemble_vector(cone, O.Space(cone.conn, cone.nnodes, 1), oL)
    V = cfx.FunctionSpace(cfx.Mesh.from_arrays(3, cone.x, cone.conn), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    L = fem.form([fem.Integral(fem.SOURCE, cells=cfx.locate_entities_device(cd, "phi<0"), params=(fem.F_SINPROD, 1.0), qdegree=4)], V, rank=1)
    b, names = profiled(lambda: fem.assemble_vector(L))
    assert rel_err(b, want) < RTOL and "source_groups" not in names, sorted(names)


def test_sync_free_step(oracle):
    """One recorded and two speculated steps (cutfemx_amd.run_step) on the 3-D shape with apex stencil 50, the interface
    moving a little: each equals the oracle and the plain sequence of the same calls."""
    import torch

    import cutfemx_amd as cfx
    from test_gpu_step import check_against_oracle, one_step
    R = refs(oracle, 3, (6, 6))
    om = R["om"]
    mesh = cfx.Mesh.from_arrays(3, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, 1)
    base = torch.tensor(R["phi"], device="cuda")
    phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
    f = cfx.Function(V, phi)
    state = {"cd": None, "b": torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)}
    key = "test-high-valence-step"
    cfx.forget_step_history(key)
    for k in range(3):
        phi.copy_(base - 0.004 * k)                    # in place: the engine aliases this array
        state["b"].zero_()
        info = {}
        system, A, b, dom = cfx.run_step(lambda: one_step(V, state["cd"], f, state), key=key, info=info)
        assert info["passes"] <= 2, info
        check_against_oracle(oracle, om, phi, state["cd"], system, A, b, dom)
        plain = {"cd": None, "b": torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)}
        _s2, A2, b2, dom2 = one_step(V, None, f, plain)
        assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices)
        assert rel_err(A.data, A2.data) < 1e-13 and rel_err(b.cpu().numpy(), b2.cpu().numpy()) < 1e-13
        assert np.array_equal(dom.inactive_dofs, dom2.inactive_dofs)


SWITCHES = ["CFX_STENCIL_STAGED=0", "CFX_PLAIN_STAGE=0", "CFX_MFMA=0", "CFX_VEC_ROWORDER=0", "CFX_SOURCE_SERIES=0",
            "CFX_STENCIL_STAGED=0 CFX_TILES=0", "CFX_PLAIN_STAGE=0 CFX_TILES=0"]    # (with the tiles on, the tile kernel has the plain rows)
_BOX = {}


@pytest.mark.parametrize("mode", SWITCHES, ids=_id)
@pytest.mark.parametrize("tdim,n", [(3, 8), (2, 16)])
def test_never_set_switches_on_box_meshes(oracle, tdim, n, mode, monkeypatch):
    """The per-call and table-build switches that no other test sets, on ordinary Kuhn meshes: the forms behind them (the
    two-pass stencil build, plain rows without LDS staging, ...) give the oracle's Poisson system."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson
    _setenv(monkeypatch, mode)
    if (tdim, n) not in _BOX:
        om = oracle.mesh_box(tdim, n)
        phi = level_set_values(om.x, tdim)
        _BOX[(tdim, n)] = (om, phi, oracle_poisson(oracle, om, phi))
    om, phi, ref = _BOX[(tdim, n)]
    V = cfx.FunctionSpace(cfx.Mesh.from_arrays(tdim, om.x, om.conn), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    s = poisson.build_forms(V, cd, order=4)
    A = fem.create_matrix(s.a)
    assert np.array_equal(A.indptr, ref["indptr"]) and np.array_equal(A.indices, ref["indices"])
    fem.assemble_matrix(s.a, A=A)
    b = fem.assemble_vector(s.L)
    assert rel_err(A.data, ref["values"]) < RTOL and rel_err(b, ref["b"]) < RTOL
    dom = fem.active_domain(s.a)
    fem.deactivate_outside(A, b, dom)
    vals, bb = ref["values"].copy(), ref["b"].copy()
    oracle.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb)
    assert rel_err(A.data, vals) < RTOL and rel_err(b, bb) < RTOL and np.array_equal(dom.inactive_dofs, ref["inactive"])
