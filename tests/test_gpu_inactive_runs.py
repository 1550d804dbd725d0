"""The inactive rows of a step as runs (round 11): the CSR build (indptr and the diagonal column indices of
indptr_tile), the fused set_value(0) (zero_inactive_tiles_kernel) and the deactivation (deactivate_marks_kernel) write
the rows of whole 16-row groups without an active row as contiguous runs, 16 B per lane, and only the inactive rows of
groups with active rows one by one.

Every case: the value buffer starts as NaN and is handed to create_matrix longer than nnz; b starts as NaN on the rows
the oracle calls inactive and as 0 on the others (assemble_vector accumulates: a NaN under an active row would swallow
that row's comparison); create_matrix -> set_value(0) -> assemble_matrix -> assemble_vector ->
deactivate_outside(diagonal=3.5, rhs_value=-2.25).  indptr / indices array-equal to the oracle's create_sparsity, the
inactive rows' entries exactly 0.0 after assemble_matrix and exactly 3.5 / -2.25 after the deactivation, the active rows
within 1e-12 of the oracle, the buffer beyond nnz still NaN.  CFX_ROWS_SPLIT=1 sends these small systems through the
split the 512^3 benchmark takes (the fused zero fill), CFX_STAGING_NAN=1 starts every column index as -1.

Each case asserts from the oracle's arrays that its path occurs: wholly inactive and mixed tiles of 2048 rows (the CSR
build) and of 4096 rows (zero fill, deactivation), and 16-row groups with rows of both kinds."""
import numpy as np
import pytest

from helpers import level_set_values, oracle_poisson, rel_err, scrambled_mesh

pytestmark = pytest.mark.gpu
RTOL = 1e-12
DIAG, RHS = 3.5, -2.25
PAD = 37
ENV = {"CFX_ROWS_SPLIT": "1", "CFX_STAGING_NAN": "1"}


def _sphere(c, r):
    return lambda x, tdim: np.linalg.norm(x[:, :tdim] - np.asarray(c)[:tdim], axis=1) - r


# name: (tdim, n, level set, scrambled numbering)
CASES = {
    "sphere16": (3, 16, lambda x, tdim: level_set_values(x, 3), False),
    "sphere32": (3, 32, lambda x, tdim: level_set_values(x, 3), False),
    "small32": (3, 32, _sphere((0.5, 0.5, 0.5), 0.12), False),
    "complement32": (3, 32, lambda x, tdim: 0.35 - np.linalg.norm(x[:, :3] - 0.5, axis=1), False),
    "plane_x32": (3, 32, lambda x, tdim: x[:, 0] - 0.37, False),
    "plane_z32": (3, 32, lambda x, tdim: x[:, 2] - 0.37, False),
    "plane_mz32": (3, 32, lambda x, tdim: 0.37 - x[:, 2], False),
    "whole16": (3, 16, _sphere((0.5, 0.5, 0.5), 2.0), False),
    "scrambled16": (3, 16, lambda x, tdim: level_set_values(x, 3), True),
    "circle64": (2, 64, lambda x, tdim: level_set_values(x, 2), False),
    "circle128": (2, 128, _sphere((0.5, 0.5), 0.1), False),
}
_REF = {}


def reference(O, name):
    """Mesh, level set and the oracle's deactivated system of a case: computed once, left unchanged."""
    if name not in _REF:
        tdim, n, ls, scrambled = CASES[name]
        om = scrambled_mesh(O, tdim, n) if scrambled else O.mesh_box(tdim, n)
        phi = ls(om.x, tdim)
        _REF[name] = (om, phi, finish_reference(O, oracle_poisson(O, om, phi)))
    return _REF[name]


def finish_reference(O, ref):
    vals, bb = ref["values"].copy(), ref["b"].copy()
    O.deactivate(ref["inactive"], ref["indptr"], ref["indices"], vals, bb, DIAG, RHS)
    off = np.zeros(ref["indptr"].size - 1, dtype=bool)
    off[ref["inactive"]] = True
    return dict(indptr=ref["indptr"], indices=ref["indices"], values=vals, b=bb, inactive=off)


def shape_of(ref):
    """What the marks offer the kernels: whole tiles of 2048 / 4096 rows without an active row, tiles and whole 16-row
    groups with rows of both kinds, and the first entries of the whole groups without an active row."""
    off = ref["inactive"]
    out = {}
    for t in (2048, 4096, 16):
        nfull = off.size // t
        per = off[:nfull * t].reshape(nfull, t).sum(axis=1)
        out[f"inactive{t}"] = int(np.count_nonzero(per == t))
        out[f"mixed{t}"] = int(np.count_nonzero((per > 0) & (per < t)))
        out[f"active{t}"] = int(np.count_nonzero(per == 0))
        if t == 16:
            out["first_entries"] = ref["indptr"][:nfull * t:t][per == t]
    return out


def run_system(cfx, V, a, L, ref, monkeypatch, A_none=False, b_none=False):
    """The sequence of the docstring on the forms a, L of V, every check against `ref` included."""
    import torch
    off = ref["inactive"]
    nnz, nrows = int(ref["indptr"][-1]), off.size
    with monkeypatch.context() as mp:
        for k, v in ENV.items():
            mp.setenv(k, v)
        values = torch.full((nnz + PAD,), float("nan"), device="cuda", dtype=torch.float64)
        A = cfx.fem.create_matrix(a, values=values)
        assert A.nnz == nnz
        indptr, indices = A.indptr.copy(), A.indices.copy()
        assert np.array_equal(indptr, ref["indptr"]) and np.array_equal(indices, ref["indices"])
        A.set_value(0.0)
        cfx.fem.assemble_matrix(a, A=A)
        zeroed = values.cpu().numpy().copy()
        b = torch.zeros(nrows, device="cuda", dtype=torch.float64)
        b[torch.as_tensor(off, device="cuda")] = float("nan")
        cfx.fem.assemble_vector(L, b)
        cfx.fem.deactivate_outside(None if A_none else A, None if b_none else b, cfx.fem.active_domain(a),
                                   diagonal=DIAG, rhs_value=RHS)
        torch.cuda.synchronize()
        got, gb = values.cpu().numpy().copy(), b.cpu().numpy().copy()
    entry_off = np.repeat(off, np.diff(indptr))            # entries of inactive rows: their bs x bs diagonal block
    bs = V.bs
    assert int(entry_off.sum()) == bs * int(off.sum())
    assert np.all(zeroed[:nnz][entry_off] == 0.0) and not np.any(np.signbit(zeroed[:nnz][entry_off]))
    assert np.all(np.isnan(zeroed[nnz:])) and np.all(np.isnan(got[nnz:]))
    if A_none:
        assert np.array_equal(got[:nnz], zeroed[:nnz])
    else:
        # exactly 3.5 on the diagonal (and 0.0 beside it in a vector space), as the oracle leaves them
        assert np.array_equal(got[:nnz][entry_off], ref["values"][entry_off])
        assert int(np.count_nonzero(got[:nnz][entry_off] == DIAG)) == int(off.sum())
        assert bs > 1 or np.all(got[:nnz][entry_off] == DIAG)
    assert rel_err(got[:nnz][~entry_off], ref["values"][~entry_off]) < RTOL
    if b_none:
        assert np.all(np.isnan(gb[off]))
    else:
        assert np.all(gb[off] == RHS)
    assert rel_err(gb[~off], ref["b"][~off]) < RTOL
    return dict(indptr=indptr, indices=indices, values=got[:nnz], b=gb)


def run_case(O, name, monkeypatch, **kw):
    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    tdim, n, _, scrambled = CASES[name]
    om, phi, ref = reference(O, name)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn) if scrambled else cfx.Mesh.create_box(tdim, n)
    V = cfx.FunctionSpace(mesh, 1)
    with monkeypatch.context() as mp:
        for k, v in ENV.items():
            mp.setenv(k, v)
        s = poisson.build_forms(V, cfx.cut(cfx.Function(V, phi)), order=4)
        run_system(cfx, V, s.a, s.L, ref, monkeypatch, **kw)
    return shape_of(ref)


@pytest.mark.parametrize("n", [16, 32])
def test_the_benchmark_sphere(oracle, monkeypatch, n):
    """16^3: 4913 rows, two mixed tiles of 2048 rows and one of 4096, the last tile partial; 32^3: wholly inactive tiles
    of both sizes and several hundred mixed groups."""
    sh = run_case(oracle, f"sphere{n}", monkeypatch)
    print(sh)
    assert sh["mixed16"] > 0 and sh["mixed2048"] > 0 and sh["mixed4096"] > 0
    if n == 32:
        assert sh["inactive2048"] > 0 and sh["inactive4096"] > 0 and sh["mixed16"] > 100


def test_a_small_sphere(oracle, monkeypatch):
    """Centre 0.5, R 0.12 on 32^3: most tiles wholly inactive, the first and the last full one among them."""
    sh = run_case(oracle, "small32", monkeypatch)
    print(sh)
    off = reference(oracle, "small32")[2]["inactive"]
    assert sh["inactive2048"] > 4 and sh["inactive4096"] > 2 and sh["mixed2048"] > 0 and sh["mixed4096"] > 0
    for t in (2048, 4096):
        assert off[:t].all() and off[(off.size // t - 1) * t:(off.size // t) * t].all()


def test_the_complement_of_a_sphere(oracle, monkeypatch):
    """phi = 0.35 - |x - c|: rows 0 and N - 1 are active, there are wholly ACTIVE tiles."""
    sh = run_case(oracle, "complement32", monkeypatch)
    print(sh)
    off = reference(oracle, "complement32")[2]["inactive"]
    assert not off[0] and not off[-1]
    assert sh["active2048"] > 0 and sh["active4096"] > 0 and sh["mixed16"] > 100


def test_a_plane_across_the_fastest_index(oracle, monkeypatch):
    """phi = x - 0.37: every x-line of 33 rows changes sides, every tile is mixed, runs start at every residue mod 16."""
    sh = run_case(oracle, "plane_x32", monkeypatch)
    print(sh)
    off = reference(oracle, "plane_x32")[2]["inactive"]
    assert sh["inactive2048"] == 0 and sh["active2048"] == 0 and sh["mixed16"] > 1000
    starts = np.flatnonzero(off & ~np.concatenate([[False], off[:-1]]))
    assert set(starts % 16) == set(range(16))


@pytest.mark.parametrize("name", ["plane_z32", "plane_mz32"])
def test_a_plane_across_the_slowest_index(oracle, monkeypatch, name):
    """phi = z - 0.37 and 0.37 - z: one long run of each kind; the inactive tiles begin behind the active rows' entries
    in the first case and at entry 0 in the second."""
    sh = run_case(oracle, name, monkeypatch)
    print(sh)
    ref = reference(oracle, name)[2]
    assert sh["inactive2048"] > 2 and sh["inactive4096"] > 1
    first_off = int(np.flatnonzero(ref["inactive"])[0])
    if name == "plane_z32":
        assert first_off > 0 and ref["indptr"][first_off] > first_off
    else:
        assert first_off == 0 and ref["inactive"][:4096].all()


def test_a_sphere_that_holds_the_whole_box(oracle, monkeypatch):
    """No row is inactive: nothing to zero, nothing to deactivate."""
    sh = run_case(oracle, "whole16", monkeypatch)
    assert not reference(oracle, "whole16")[2]["inactive"].any() and sh["inactive16"] == 0


def test_a_scrambled_numbering(oracle, monkeypatch):
    """Marks without structure: mixed groups throughout."""
    sh = run_case(oracle, "scrambled16", monkeypatch)
    print(sh)
    assert sh["mixed16"] > 100


@pytest.mark.parametrize("name", ["circle64", "circle128"])
def test_squares(oracle, monkeypatch, name):
    sh = run_case(oracle, name, monkeypatch)
    print(sh)
    assert sh["mixed16"] > 0
    if name == "circle128":
        assert sh["inactive2048"] > 0 and sh["inactive4096"] > 0


@pytest.mark.parametrize("degree,bs", [(2, 1), (1, 3)])
def test_general_spaces_keep_the_general_paths(oracle, monkeypatch, degree, bs):
    """A degree-2 space and a vector space at 8^3 (hashed patterns, block size 3: the per-row code of all three
    kernels' callers) against the oracle."""
    import cutfemx_amd as cfx
    fem, O = cfx.fem, oracle
    tdim, n = 3, 8
    om = O.mesh_box(tdim, n)
    phi = level_set_values(om.x, tdim)
    dofmap, ndofs = cfx.lagrange_dofmap(tdim, om.conn, om.nnodes, degree)
    oV = O.Space(dofmap, ndofs, degree, bs)
    mesh = cfx.Mesh.from_arrays(tdim, om.x, om.conn)
    V = cfx.FunctionSpace(mesh, degree, dofmap=None if degree == 1 else dofmap, ndofs=ndofs, bs=bs)
    cd = cfx.cut(cfx.Function(cfx.FunctionSpace(mesh, 1), phi))
    dom = O.classify(om.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    ovol = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 2)
    vol = cfx.runtime_quadrature(cd, "phi<0", 2)
    if bs == 1:
        oa = [O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, rules=ovol, qdegree=2)]
        ga = [fem.Integral(fem.STIFFNESS, cells=inside, rules=vol, qdegree=2)]
        oL = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=ovol, params=(O.F_SINPROD, 1.0), qdegree=4)]
        gL = [fem.Integral(fem.SOURCE, cells=inside, rules=vol, params=(fem.F_SINPROD, 1.0), qdegree=4)]
    else:
        w = np.random.default_rng(5).standard_normal(ndofs * bs)
        oa = [O.Integral(O.CELL, O.K_ELASTICITY, entities=inside, rules=ovol, params=(10.0, 0.3), qdegree=0)]
        ga = [fem.Integral(fem.ELASTICITY, cells=inside, rules=vol, params=(10.0, 0.3), qdegree=0)]
        oL = [O.Integral(O.CELL, O.L_SOURCE, entities=inside, rules=ovol, params=(O.F_COEFFICIENT, 1.0), qdegree=4,
                         coefficient=w)]
        gL = [fem.Integral(fem.SOURCE, cells=inside, rules=vol, params=(fem.F_COEFFICIENT, 1.0), qdegree=4, coefficient=w)]
    ip, ix = O.create_sparsity(om, oV, oa)
    ref = finish_reference(O, dict(indptr=ip, indices=ix, values=O.assemble_matrix(om, oV, oa, ip, ix),
                                   b=O.assemble_vector(om, oV, oL),
                                   inactive=O.inactive_dofs(oV, O.active_cells(oa, om.conn.shape[0]))))
    assert ref["inactive"].any() and not ref["inactive"].all()
    run_system(cfx, V, fem.form(ga, V), fem.form(gL, V, rank=1), ref, monkeypatch)


@pytest.mark.parametrize("which", ["A", "b"])
def test_deactivation_without_the_matrix_or_the_vector(oracle, monkeypatch, which):
    """deactivate_outside(None, b, ...) leaves the matrix as assembled; deactivate_outside(A, None, ...) leaves b."""
    run_case(oracle, "small32", monkeypatch, A_none=which == "A", b_none=which == "b")


def test_deactivation_of_a_pattern_built_from_another_plan(oracle, monkeypatch):
    """The matrix of the Poisson system deactivated with the active domain of its stiffness integral alone: the
    pattern was not built from that plan (the entries of a run are read back, not taken on trust), and the inactive
    rows next to the interface are full rows of the matrix -- runs that fail the check and go row by row through
    csr_find.  Every inactive row's diagonal becomes 3.5 and nothing else changes."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem, poisson
    O, n = oracle, 32
    om, phi, ref = reference(O, "sphere32")
    dom = O.classify(om.conn, phi)
    inside = O.locate_entities(dom, "phi<0")
    oV = O.Space(om.conn, om.nnodes, 1)
    off = np.zeros(om.nnodes, dtype=bool)
    off[O.inactive_dofs(oV, O.active_cells([O.Integral(O.CELL, O.K_STIFFNESS, entities=inside, qdegree=0)],
                                           om.conn.shape[0]))] = True
    assert np.count_nonzero(off & ~ref["inactive"]) > 100 and not np.any(ref["inactive"] & ~off)
    with monkeypatch.context() as mp:
        for k, v in ENV.items():
            mp.setenv(k, v)
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        cd = cfx.cut(cfx.Function(V, phi))
        s = poisson.build_forms(V, cd, order=4)
        a2 = fem.form([fem.Integral(fem.STIFFNESS, cells=cfx.locate_entities_device(cd, "phi<0"), qdegree=0)], V)
        A = fem.assemble_matrix(s.a)
        before = A.data.copy()
        b = torch.full((om.nnodes,), 7.0, device="cuda", dtype=torch.float64)
        fem.deactivate_outside(A, b, fem.active_domain(a2), diagonal=DIAG, rhs_value=RHS)
        got, gb, ip, ix = A.data.copy(), b.cpu().numpy(), A.indptr, A.indices
    assert np.array_equal(ip, ref["indptr"]) and np.array_equal(ix, ref["indices"])
    rows = np.repeat(np.arange(om.nnodes), np.diff(ip))
    diag_off = (ix == rows) & off[rows]
    assert int(diag_off.sum()) == int(off.sum())
    assert np.all(got[diag_off] == DIAG) and np.array_equal(got[~diag_off], before[~diag_off])
    assert np.all(gb[off] == RHS) and np.all(gb[~off] == 7.0)


def test_the_first_entries_of_inactive_groups_cover_every_alignment(oracle):
    """Over the cases of this file the first entry of a 16-row group without an active row falls on both parities (the
    8 B runs of the fills) and on all four residues modulo 4 (the 4 B runs of the column indices)."""
    seen = set()
    for name in CASES:
        seen |= set((shape_of(reference(oracle, name)[2])["first_entries"] % 4).tolist())
    assert seen == {0, 1, 2, 3}, seen


@pytest.mark.parametrize("n", [16, 32])
def test_in_steps_with_and_without_forced_overflow(oracle, monkeypatch, n):
    """Eight steps of a sphere moving by 0.3 h, as a plain sequence (indptr_reduce + indptr_write), as sync-free steps
    (indptr_chained at these sizes) and with capacities forced below the previous counts (void passes, repeated): every
    accepted step has the four arrays of the plain sequence, the buffer beyond nnz stays NaN, and a void pass leaves no
    HIP error behind."""
    import ctypes as C
    import os

    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib, poisson
    steps = 8
    om = oracle.mesh_box(3, n)
    xt = torch.tensor(om.x.copy(), device="cuda")
    nrows = om.nnodes

    def phi_of(k):
        c = torch.tensor([0.40 + 0.3 / n * k, 0.45, 0.5], device="cuda", dtype=torch.float64)
        return torch.linalg.norm(xt - c, dim=1) - 0.27

    refs = {k: finish_reference(oracle, oracle_poisson(oracle, om, phi_of(k).cpu().numpy())) for k in (0, steps - 1)}
    cap = max(int(r["indptr"][-1]) for r in refs.values()) + 4096

    def loop(tag, margin, in_steps):
        with monkeypatch.context() as mp:
            for name, v in dict(ENV, CFX_DETERMINISTIC="1").items():   # (ordered sums: "equal" means the same bits)
                mp.setenv(name, v)
            V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
            phi = torch.empty(nrows, device="cuda", dtype=torch.float64)
            f = cfx.Function(V, phi)
            values = torch.empty(cap, device="cuda", dtype=torch.float64)
            b = torch.empty(nrows, device="cuda", dtype=torch.float64)
            state = {"cd": None}

            def body():
                if state["cd"] is None:
                    state["cd"] = cfx.cut(f)
                else:
                    cfx.update(state["cd"])
                s = poisson.build_forms(V, state["cd"], order=4)
                _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(b.data_ptr()), 0, C.c_size_t(8 * b.numel())))
                A = cfx.fem.create_matrix(s.a, values=values)
                A.set_value(0.0)
                cfx.fem.assemble_matrix(s.a, A=A)
                cfx.fem.assemble_vector(s.L, b)
                cfx.fem.deactivate_outside(A, b, cfx.fem.active_domain(s.a), diagonal=DIAG, rhs_value=RHS)
                return A

            key = f"test-inactive-runs-{n}-{tag}"
            cfx.forget_step_history(key)
            out, passes = [], []
            try:
                if margin is not None:
                    cfx.set_step_margin(margin, 0)
                for k in range(steps):
                    phi.copy_(phi_of(k))
                    values.fill_(float("nan"))
                    info = {"passes": 1}
                    A = cfx.run_step(body, key=key, info=info) if in_steps else body()
                    torch.cuda.synchronize()          # (a fault of a void pass would surface here)
                    passes.append(info["passes"])
                    nnz = A.nnz
                    v = values.cpu().numpy()
                    assert np.all(np.isnan(v[nnz:])), (tag, k)
                    out.append((A.indptr.copy(), A.indices.copy(), v[:nnz].copy(), b.cpu().numpy().copy()))
            finally:
                cfx.set_step_margin()
            return out, passes

    want, _ = loop("plain", None, False)
    for k, ref in refs.items():
        ip, ix, va, bb = want[k]
        off = ref["inactive"]
        entry_off = np.repeat(off, np.diff(ip))
        assert np.array_equal(ip, ref["indptr"]) and np.array_equal(ix, ref["indices"])
        assert np.all(va[entry_off] == DIAG) and np.all(bb[off] == RHS)
        assert rel_err(va, ref["values"]) < RTOL and rel_err(bb, ref["b"]) < RTOL
    speculative = os.environ.get("CFX_STEP_SPECULATE") != "0"
    bitwise = os.environ.get("CFX_ASSEMBLY") != "atomic"      # (FP64 atomics: the active rows' sums are not ordered)
    for tag, margin in (("steps", None), ("forced", 0.97)):
        got, passes = loop(tag, margin, True)
        print(tag, "passes", passes)
        for k in range(steps):
            assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), (tag, k)
            if bitwise:
                assert np.array_equal(got[k][2], want[k][2]) and np.array_equal(got[k][3], want[k][3]), (tag, k)
            else:
                assert rel_err(got[k][2], want[k][2]) < RTOL and rel_err(got[k][3], want[k][3]) < RTOL, (tag, k)
        if tag == "forced" and speculative:
            assert max(passes) == 2, passes
