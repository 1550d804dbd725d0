"""The exact extension-penalty pair block, the exact volume fractions and a statement of what a valid cell aggregation is
(`exact_cut.py`: `pair_tensor`, `exact_pair_entries`, `exact_fraction`): self-checks that need neither the oracle nor the
engine, then oracle == exact for everything that `test_gpu_exact_extensions.py` holds the engine to, so that a failure
on the GPU can be placed.  CPU only.

The pair integrand beta M_i M_j, M = [N_bad, -(N_root o F_root^-1)], is a polynomial of degree 2 degree on the whole bad
cell: `qdegree = 2 degree` integrates it exactly (asserted), so no two sides can agree by under-integrating alike.
Self-checks are equalities in Fractions (1e-15 where longdouble enters).  Tolerances: a pair tensor block by block,
abs(got - exact) <= 1e-12 x sqrt(max|T_aa| max|T_bb|) for block (a, b), a, b in {bad, root}, the maxima taken over the
exact diagonal blocks of the same pair (for a far pair the root x root block is 10^4 to 10^5 times the bad x bad one: one
scale for the whole tensor would let an error of 100 % in the bad cell's own block pass); assembled arrays entry by entry,
abs(got - exact) <= 1e-12 x the sum of the absolute exact contributions to that entry, and rel_err <= 1e-12 on the whole
array; volume fractions absolute 1e-12.  Nothing is left out: pairs are whole cells and every level set here is regular.

The case tables and the exact-side helpers below are shared with `test_gpu_exact_extensions.py`.
"""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import exact_cut as X
from test_exact_forms_reference import dofmaps

TOL = 1e-12
EPS = 1e-15
LD = X.LD
BETA = 2.5
GHOST = (0.1, 0.0)              # the ghost penalty of form (c): 0.1 h_avg [dn u][dn v]
C2, H2, S3, G3, G6 = "2d-n8-sphere", "2d-n8-sphere-scrambled", "3d-n4-sphere-scrambled", "3d-n5-gyroid", "3d-n6-gyroid"
# (case, threshold, degrees): the pair forms.  The last one has 1248 pairs and is taken at P1 only.
PAIR_CASES = [(C2, 1.0, (1, 2)), (H2, 0.6, (1, 2)), (S3, 1.0, (1, 2)), (G3, 1.0, (1, 2)), (G3, 0.6, (1, 2)), (G6, 1.0, (1,))]
PAIR_IDS = [f"{n}-thr{t}" for n, t, _ in PAIR_CASES]
# longest CSR row of the scalar pair form (with the all-rows diagonal) where a case is meant to reach a column class:
# (case, threshold, degree) -> columns; computed from pairs and dofmap, asserted in both files
LONGEST_ROW = {(C2, 1.0, 2): 43, (S3, 1.0, 2): 262, (G3, 1.0, 2): 412, (G6, 1.0, 1): 127}
AGG_CASES = [C2, H2, S3, G3, G6]
AGG_THRESHOLDS = (0.3, 0.6, 1.0)
SELECTORS = ("phi<0", "phi>0")
POLICIES = ("interior_or_well_cut", "interior_only")


def _report(group, what, worst):
    print(f"EXACT {group}: {what}: worst {worst:.3e}")


def block_spaces(tdim, degree):
    """(bs,) of the spaces a degree is compared on: scalar everywhere, P1 bs = 3 in 3-D, P2 bs = 2 in 2-D."""
    return (1, 3) if (tdim, degree) == (3, 1) else (1, 2) if (tdim, degree) == (2, 2) else (1,)


def beta_cells(ncells):
    """Cellwise beta in [0.5, 2], one random value per cell: not monotone in the cell index, so a read at the root or at
    the pair's position in another order gives other numbers."""
    return np.random.default_rng(97).uniform(0.5, 2.0, ncells)


def interior_of(cs, selector):
    v = cs["phi"][cs["conn"]]
    return np.flatnonzero(np.all(v < 0, axis=1) if "<" in selector else np.all(v > 0, axis=1)).astype(np.int32)


def pair_figures(cs, pairs, degree):
    """From the inputs alone: pairs by the number of shared vertices, the most bad cells of one root, the longest row."""
    dm, nd = dofmaps(cs, degree)
    shared = np.bincount(X.shared_vertices(cs["conn"], pairs), minlength=cs["tdim"] + 1)[:cs["tdim"] + 1]
    most = int(np.unique(pairs[:, 2], return_counts=True)[1].max()) if len(pairs) else 0
    return shared.tolist(), most, X.longest_pair_row(dm, 1, pairs, nd)


def check_pair_case(cs, thr, degree, pairs):
    """What a pair case must hold, from the inputs alone: every 3-D case has pairs that share 0, 1, 2 and 3 vertices; the
    longest-row figure of the cases that are meant to reach one."""
    shared, most, longest = pair_figures(cs, pairs, degree)
    print(f"EXACT pairs: {cs['name']} thr {thr} P{degree}: pairs {len(pairs)} most bad cells of one root {most} longest row {longest} "
          f"shared vertices {shared}")
    assert len(pairs) > 0 and np.all(pairs[:, 0] != pairs[:, 2]) and np.all(pairs[:, [1, 3]] == 0)
    if cs["tdim"] == 3:
        assert all(v > 0 for v in shared), shared
    if (cs["name"], thr, degree) in LONGEST_ROW:
        assert longest == LONGEST_ROW[(cs["name"], thr, degree)], longest
    return shared, most, longest


def pair_errors(got, T, ndc):
    """Worst abs(got - T) / scale of the four blocks (00, 01, 10, 11) of one pair, each on its own scale."""
    e = np.abs(np.asarray(got, dtype=np.float64).reshape(T.shape) - T) / X.pair_block_scales(T, ndc)
    return np.array([e[:ndc, :ndc].max(), e[:ndc, ndc:].max(), e[ndc:, :ndc].max(), e[ndc:, ndc:].max()])


def exact_pair(name, cs, degree, bs, row, beta=BETA):
    T = X.unit_pair_tensor(name, cs, degree, row[0], row[2]) * LD(beta)
    return (T if bs == 1 else np.kron(T, np.eye(bs, dtype=LD))).astype(np.float64)


def summed(parts):
    """Exact assembled entries from several terms: `parts` are COO triplets of contributions (rows, cols, values) or
    summed quadruplets (rows, cols, values, scales).  -> (rows, cols, values, scales), one entry per (row, column), rows
    then columns ascending; scales = the sum of the absolute contributions."""
    r = np.concatenate([np.asarray(p[0], dtype=np.int64) for p in parts])
    c = np.concatenate([np.asarray(p[1], dtype=np.int64) for p in parts])
    v = np.concatenate([np.asarray(p[2], dtype=LD) for p in parts])
    s = np.concatenate([np.abs(np.asarray(p[2], dtype=LD)) if len(p) == 3 else np.asarray(p[3], dtype=LD) for p in parts])
    order = np.lexsort((c, r))
    r, c, v, s = r[order], c[order], v[order], s[order]
    first = np.flatnonzero(np.r_[True, (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
    return r[first], c[first], np.add.reduceat(v, first).astype(np.float64), np.add.reduceat(s, first).astype(np.float64)


def entry_errors(indptr, indices, data, exact, ncols):
    """(worst abs(got - exact) / scale over the entries, rel_err of the whole array) of a CSR matrix against summed exact
    entries.  An entry of the pattern that no exact contribution reaches must be exactly zero (it counts as inf
    otherwise); every exact entry with a scale must be in the pattern.  An entry whose exact contributions are all exactly
    zero and that brings no scale of its own (a P1 stiffness entry of two orthogonal gradients) has no per-entry bound: the
    bound of the whole array holds it."""
    r, c, v, s = exact
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    key, ekey = rows * ncols + np.asarray(indices, dtype=np.int64), r * ncols + c
    order = np.argsort(key, kind="stable")
    key, got = key[order], np.asarray(data, dtype=np.float64)[order]
    assert np.all(np.diff(key) > 0), "a column twice in one row"
    pos = np.searchsorted(key, ekey)
    found = (pos < key.size) & (key[np.minimum(pos, key.size - 1)] == ekey)
    assert np.all(found | (s == 0)), "an exact entry is missing from the pattern"
    want, scale, reached = np.zeros(key.size), np.zeros(key.size), np.zeros(key.size, dtype=bool)
    want[pos[found]], scale[pos[found]], reached[pos[found]] = v[found], s[found], True
    diff = np.abs(got - want)
    ratio = np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(reached | (diff == 0), 0.0, np.inf))
    return float(ratio.max()), float(diff.max() / np.abs(v).max())


def exact_form_c(name, cs, fc, thr, degree, bs, pairs):
    """Stiffness over [inside cells, phi<0 rules] + ghost penalty + pair form: the three exact terms, summed per entry."""
    dm, _ = dofmaps(cs, degree)
    return X.cached(("form-c", name, thr, degree, bs, pairs.tobytes()), lambda: summed([
        X.exact_entries(name, cs, dm, bs, "stiffness", degree, (), cs["inside"]),
        X.exact_facet_entries(name, cs, dm, bs, "ghost", degree, GHOST, fc["ghost"]),
        X.exact_pair_entries(name, cs, dm, bs, degree, pairs, BETA)]))


# ---- what a valid aggregation is, without an oracle ---------------------------------------------------------------------
def _field(a, name):
    return np.asarray(a[name] if isinstance(a, dict) else getattr(a, name))


def facet_neighbours(name, cs):
    """CSR adjacency of the cells over interior facets (`interior_facet_rows`), cached."""
    import scipy.sparse as sp

    def run():
        rows = X.interior_facet_rows(cs["conn"])
        n = cs["conn"].shape[0]
        a, b = rows[:, 0].astype(np.int64), rows[:, 2].astype(np.int64)
        return sp.coo_matrix((np.ones(2 * a.size), (np.r_[a, b], np.r_[b, a])), shape=(n, n)).tocsr()
    return X.cached(("neighbours", name), run)


def thresholds_are_decidable(name, cs):
    """No exact fraction of the case lies within 1e-9 of a threshold: the classes are then a condition, not a measurement."""
    for sel in SELECTORS:
        f = X.exact_fractions(name, cs, sel)
        for thr in AGG_THRESHOLDS:
            assert np.abs(f - thr).min() > 1e-9, (name, sel, thr)


def check_fractions(name, cs, selector, frac):
    """`cut_volume_fraction`: the exact fraction on every cut cell (absolute 1e-12; a fraction lives in [0, 1]), exactly 0
    off the cut cells (include/cutfemx_amd.h: "0 off the cut cells")."""
    frac = np.asarray(frac)
    assert frac.shape == (cs["conn"].shape[0],)
    off = np.ones(frac.size, dtype=bool)
    off[cs["cut"]] = False
    assert np.all(frac[off] == 0.0)
    ex = X.exact_fractions(name, cs, selector)
    assert np.all((ex > 0) & (ex < 1))
    return float(np.abs(frac[cs["cut"]] - ex).max())


def check_aggregation(name, cs, selector, threshold, policy, agg):
    """The classes from mathematics, the structure from the definition alone, and the pairs (unlimited iterations)."""
    from scipy.sparse.csgraph import connected_components
    ncells = cs["conn"].shape[0]
    cut, interior = cs["cut"], interior_of(cs, selector)
    active = np.union1d(cut, interior)
    ex = X.exact_fractions(name, cs, selector)
    assert np.abs(ex - threshold).min() > 1e-9
    good = cut[ex >= threshold] if policy == "interior_or_well_cut" else cut[:0]
    well, ill = np.union1d(interior, good), np.setdiff1d(cut, good)
    for field, want in (("active_cells", active), ("cut_cells", cut), ("interior_cells", interior), ("well_posed_cells", well),
                        ("ill_posed_cells", ill)):
        assert np.array_equal(_field(agg, field), want), field
    root, aid, depth = (_field(agg, k) for k in ("root_cell", "aggregate_id", "propagation_depth"))
    assert root.shape == aid.shape == depth.shape == (ncells,)
    # roots: depth 0, their own root, aggregate ids 0 .. n_well - 1 in ascending cell order
    assert np.array_equal(root[well], well) and np.all(depth[well] == 0) and np.array_equal(aid[well], np.arange(well.size))
    # a rooted ill-posed cell at depth k has an active facet neighbour with its root, its aggregate id and depth k - 1
    N = facet_neighbours(name, cs)
    is_active = np.zeros(ncells, dtype=bool)
    is_active[active] = True
    rooted = ill[root[ill] >= 0]
    assert np.all(depth[rooted] >= 1) and np.all(np.isin(root[rooted], well)) and np.array_equal(aid[rooted], aid[root[rooted]])
    for c in rooted.tolist():
        nb = N.indices[N.indptr[c]:N.indptr[c + 1]]
        nb = nb[is_active[nb]]
        assert np.any((root[nb] == root[c]) & (aid[nb] == aid[c]) & (depth[nb] == depth[c] - 1)), c
    # rootless: exactly the ill-posed cells whose component of the active facet graph holds no well-posed cell
    sub = N[active][:, active]
    ncomp, label = connected_components(sub, directed=False)
    has_root = np.zeros(ncomp, dtype=bool)
    has_root[label[np.searchsorted(active, well)]] = True
    lonely = ill[~has_root[label[np.searchsorted(active, ill)]]]
    assert np.array_equal(_field(agg, "rootless_cells"), lonely)
    assert np.array_equal(ill[root[ill] < 0], lonely)
    inactive = np.setdiff1d(np.arange(ncells), active)
    assert np.all(root[inactive] == -1) and np.all(root[lonely] == -1)
    pairs = np.zeros((rooted.size, 4), dtype=np.int32)
    pairs[:, 0], pairs[:, 2] = rooted, root[rooted]
    return pairs, int(depth[rooted].max()) if rooted.size else 0, lonely.size


# ---- self-checks of the exact pair block ----------------------------------------------------------------------------------
def _oracle_setup(O, cs):
    om, phi = cs["om"], cs["phi"]
    return om, phi, O.classify(om.conn, phi)


def oracle_pairs(O, name, thr):
    """The oracle's pairs of `phi<0` (the sequential sweeps; inputs of the CPU comparisons)."""
    def run():
        cs = X.build_case(O, name)
        om, phi, dom = _oracle_setup(O, cs)
        return O.extension_pairs(O.cell_aggregation(om, om.conn, phi, dom, "phi<0", thr))
    return X.cached(("opairs", name, thr), run)


def _some_pairs(cs, pairs, n=6):
    """A few pairs that share each number of vertices, far ones first."""
    sh = X.shared_vertices(cs["conn"], pairs)
    out = []
    for k in range(cs["tdim"] + 1):
        out += np.flatnonzero(sh == k)[: max(1, n // (cs["tdim"] + 1))].tolist()
    return pairs[sorted(out)]


def pair_dofs(poly, x, conn, cells, degree):
    """[poly at the dofs of cells[0], poly at the dofs of cells[1]] as Fractions (vertices, then edge midpoints in Basix
    order)."""
    d = conn.shape[1] - 1
    out = []
    for c in cells:
        Xc = X.frac_rows(x[conn[c], :d])
        pts = list(Xc)
        if degree == 2:
            pts += [[(p + q) / 2 for p, q in zip(Xc[a], Xc[b])] for a, b in X.EDGES[d]]
        out += [F(poly(p)) for p in pts]
    return out


def _apply(T, v):
    return [sum(t * w for t, w in zip(row, v) if t and w) for row in T]


def _dof_permutation(d, degree, perm):
    """Old local dof of each new local dof when the new local vertex i is the old local vertex perm[i]."""
    out = list(perm)
    if degree == 2:
        old = {frozenset(e): k for k, e in enumerate(X.EDGES[d])}
        out += [d + 1 + old[frozenset((perm[a], perm[b]))] for a, b in X.EDGES[d]]
    return out


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name,thr", [(H2, 0.6), (S3, 1.0)])
def test_the_exact_pair_block_has_the_properties_of_the_integral(oracle, name, thr, degree):
    """In Fractions: symmetric; bad x bad = beta x the whole-cell mass; the pair (c, c) is beta [[M, -M], [-M, M]]; every
    global polynomial of degree <= `degree` (all monomials) is annihilated, x_0^(degree + 1) is not; a permutation of either
    cell's vertices permutes the tensor; a mesh twice as large has 2^tdim times the tensor."""
    cs = X.build_case(oracle, name)
    x, conn, d = cs["x"], cs["conn"], cs["tdim"]
    beta = F(5, 2)
    rng = np.random.default_rng(4)
    for row in _some_pairs(cs, oracle_pairs(oracle, name, thr)):
        bad, root = int(row[0]), int(row[2])
        T = X.pair_tensor_exact(x, conn, d, degree, bad, root, beta)
        n = len(T)
        nd = n // 2
        assert all(T[i][j] == T[j][i] for i in range(n) for j in range(n))
        M = X.mass(X.Moments(d), x[conn[bad], :d], degree)
        B = np.array([[float(T[i][j]) for j in range(nd)] for i in range(nd)])
        assert np.abs(B - 2.5 * M).max() <= EPS * np.abs(M).max()
        S = X.pair_tensor_exact(x, conn, d, degree, bad, bad, beta)
        assert all(S[i][j] == T[i][j] == -S[i][nd + j] == -S[nd + i][j] == S[nd + i][nd + j] for i in range(nd) for j in range(nd))
        for al in X.monomials(d, degree):
            v = pair_dofs(lambda p: math.prod(p[a] ** e for a, e in enumerate(al)), x, conn, (bad, root), degree)
            assert any(v) and not any(_apply(T, v)), al
        v = pair_dofs(lambda p: p[0] ** (degree + 1), x, conn, (bad, root), degree)
        assert any(_apply(T, v))
        for side, cell in ((0, bad), (1, root)):
            perm = rng.permutation(d + 1).tolist()
            conn2 = conn.copy()
            conn2[cell] = conn[cell][perm]
            P = X.pair_tensor_exact(x, conn2, d, degree, bad, root, beta)
            p = _dof_permutation(d, degree, perm)
            m = [list(range(nd)), list(range(nd))]
            m[side] = p
            m = m[0] + [nd + k for k in m[1]]
            assert all(P[i][j] == T[m[i]][m[j]] for i in range(n) for j in range(n)), (side, perm)
        D = X.pair_tensor_exact(2.0 * x, conn, d, degree, bad, root, beta)
        assert all(D[i][j] == 2 ** d * T[i][j] for i in range(n) for j in range(n))
        # the float64 tensor is the rounded exact one, and bs > 1 repeats it on equal components only
        T64 = X.pair_tensor(x, conn, d, degree, bad, root, 2.5)
        assert np.array_equal(T64, np.array([[float(v) for v in r] for r in T]))
        Tb = X.pair_tensor(x, conn, d, degree, bad, root, 2.5, bs=d)
        assert np.array_equal(Tb.reshape(n, d, n, d), np.einsum("ij,ab->iajb", T64, np.eye(d)))
        assert np.abs(exact_pair(name, cs, degree, 1, row) - T64).max() <= EPS * np.abs(T64).max()


def test_exact_fractions_add_up_and_thresholds_are_decidable(oracle):
    """The two sides of every cut cell add up to the cell, exactly; no fraction lies within 1e-9 of 0.3, 0.6 or 1.0."""
    for name in AGG_CASES:
        cs = X.build_case(oracle, name)
        assert not cs["degenerate"] and np.all(cs["keep"])
        for c in cs["cut"][:: max(1, cs["cut"].size // 40)]:
            a, b = X.exact_fraction(cs, c, "phi<0"), X.exact_fraction(cs, c, "phi>0")
            assert a + b == 1 and 0 < a < 1
        thresholds_are_decidable(name, cs)


def test_summed_entries_and_entry_errors_see_what_they_should():
    """`summed` adds contributions and their absolute values; `entry_errors` measures each entry on its own scale, wants
    pattern entries without a contribution to be exactly zero, and refuses a pattern that lacks an entry."""
    ex = summed([(np.array([0, 0, 1]), np.array([0, 0, 1]), np.array([1.0, -1.0 + 1e-3, 1e-6]))])
    assert ex[0].tolist() == [0, 1] and ex[1].tolist() == [0, 1] and np.allclose(ex[2], [1e-3, 1e-6], rtol=1e-12, atol=0)
    assert np.allclose(ex[3], [2.0 - 1e-3, 1e-6])
    ip, ix = np.array([0, 2, 3]), np.array([0, 1, 1])
    w, r = entry_errors(ip, ix, np.array([1e-3, 0.0, 2e-6]), ex, 2)
    assert abs(w - 1.0) < 1e-9 and abs(r - 1e-3) < 1e-9               # 100 % of a small entry: seen per entry
    assert entry_errors(ip, ix, np.array([1e-3, 1e-30, 1e-6]), ex, 2)[0] == np.inf
    with pytest.raises(AssertionError):
        entry_errors(np.array([0, 1, 1]), np.array([0]), np.array([1e-3]), ex, 2)


def test_the_exact_cellwise_form_tells_the_reads_of_beta_apart(oracle):
    """With beta taken at the root, or at the pair's position in the list, the exact numbers differ by far more than the
    bound: the cellwise forms of both files cannot pass with either read."""
    cs = X.build_case(oracle, S3)
    pairs, dm = oracle_pairs(oracle, S3, 1.0), dofmaps(cs, 1)[0]
    bcell = beta_cells(cs["conn"].shape[0])
    right = X.exact_pair_entries(S3, cs, dm, 1, 1, pairs, 1.0, bcell)
    at_root, at_position = bcell.copy(), bcell.copy()
    at_root[pairs[:, 0]] = bcell[pairs[:, 2]]
    at_position[pairs[:, 0]] = bcell[:len(pairs)]
    for other in (at_root, at_position):
        wrong = X.exact_pair_entries(S3, cs, dm, 1, 1, pairs, 1.0, other)
        assert np.array_equal(wrong[0], right[0]) and np.abs(wrong[2] - right[2]).max() > 1e-2 * np.abs(right[2]).max()


# ---- oracle == exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,thr,degrees", PAIR_CASES, ids=PAIR_IDS)
def test_oracle_pair_tensors_are_the_exact_ones(oracle, name, thr, degrees):
    """`tabulate_entity` of every pair at qdegree = 2 degree, scalar and on the block spaces, block by block."""
    O = oracle
    cs = X.build_case(O, name)
    om = cs["om"]
    pairs = oracle_pairs(O, name, thr)
    for degree in degrees:
        check_pair_case(cs, thr, degree, pairs)
        q = 2 * degree
        assert q >= 2 * degree                                    # never below the integrand's degree
        dm, nd = dofmaps(cs, degree)
        for bs in block_spaces(cs["tdim"], degree):
            V = O.Space(dm, nd, degree, bs)
            I = O.Integral(O.INTERIOR_FACET, O.K_EXTENSION_L2, entities=pairs, params=(BETA,), qdegree=q)
            worst, whole = np.zeros(4), 0.0
            for i, row in enumerate(pairs):
                T = exact_pair(name, cs, degree, bs, row)
                got = O.tabulate_entity(om, V, I, i, False)
                worst = np.maximum(worst, pair_errors(got, T, dm.shape[1] * bs))
                whole = max(whole, np.abs(got - T).max() / np.abs(T).max())
            _report("pair tensors", f"oracle {name} thr {thr} P{degree} bs {bs} ({len(pairs)} pairs): whole tensor {whole:.3e} "
                    f"blocks {' '.join(f'{v:.1e}' for v in worst)}", worst.max())
            assert 0.0 < worst.max() <= TOL, (degree, bs)


@pytest.mark.parametrize("name,thr,degrees", PAIR_CASES, ids=PAIR_IDS)
def test_oracle_assembled_pair_forms_are_exact(oracle, name, thr, degrees):
    """The pair form alone, with scalar beta and with cellwise beta, entry by entry."""
    O = oracle
    cs = X.build_case(O, name)
    om = cs["om"]
    pairs = oracle_pairs(O, name, thr)
    bcell = beta_cells(om.ncells)
    for degree in degrees:
        q = 2 * degree
        assert q >= 2 * degree
        dm, nd = dofmaps(cs, degree)
        V = O.Space(dm, nd, degree, 1)
        for what, params, pdata, ex in (("beta", (BETA,), None, X.exact_pair_entries(name, cs, dm, 1, degree, pairs, BETA)),
                                        ("cellwise beta", (1.0,), bcell[pairs[:, 0]],
                                         X.exact_pair_entries(name, cs, dm, 1, degree, pairs, 1.0, bcell))):
            I = [O.Integral(O.INTERIOR_FACET, O.K_EXTENSION_L2, entities=pairs, params=params, qdegree=q, point_data=pdata)]
            ip, ix = O.create_sparsity(om, V, I)
            assert int(np.diff(ip).max()) == X.longest_pair_row(dm, 1, pairs, nd)
            worst, rel = entry_errors(ip, ix, O.assemble_matrix(om, V, I, ip, ix), ex, nd)
            _report("pair forms assembled", f"oracle {name} thr {thr} P{degree} {what}: whole array {rel:.3e} per entry", worst)
            assert 0.0 < worst <= TOL and rel <= TOL, (degree, what)


@pytest.mark.parametrize("name,thr", [(C2, 1.0), (S3, 1.0)])
def test_oracle_pair_form_next_to_stiffness_and_ghost_penalty_is_exact(oracle, name, thr):
    """Form (c) of the GPU file -- stiffness over [inside cells, phi<0 rules] + ghost penalty + pair form -- for the
    oracle, scalar P1 and P2, entry by entry.  The P2 stiffness entries that are small by cancellation inside the local
    tensor (nearly orthogonal gradients) set the worst per-entry figure, a few 1e-13 on the 3-D case for either side."""
    O = oracle
    cs, fc = X.build_case(O, name), X.facet_case(O, name)
    om, phi, dom = _oracle_setup(O, cs)
    pairs = oracle_pairs(O, name, thr)
    R = O.runtime_quadrature(om, om.conn, phi, dom, "phi<0", 4)
    for degree in (1, 2):
        dm, nd = dofmaps(cs, degree)
        V = O.Space(dm, nd, degree, 1)
        qs, q = 2 * (degree - 1), 2 * degree
        assert q >= 2 * degree and 4 >= qs
        I = [O.Integral(O.CELL, O.K_STIFFNESS, entities=cs["inside"], rules=R, qdegree=qs),
             O.Integral(O.INTERIOR_FACET, O.K_GHOST_GRADJUMP, entities=fc["ghost"], params=GHOST[:1], qdegree=qs),
             O.Integral(O.INTERIOR_FACET, O.K_EXTENSION_L2, entities=pairs, params=(BETA,), qdegree=q)]
        ip, ix = O.create_sparsity(om, V, I)
        worst, rel = entry_errors(ip, ix, O.assemble_matrix(om, V, I, ip, ix), exact_form_c(name, cs, fc, thr, degree, 1, pairs), nd)
        _report("pair forms assembled", f"oracle {name} thr {thr} P{degree} (c): whole array {rel:.3e} per entry", worst)
        assert 0.0 < worst <= TOL and rel <= TOL, degree


@pytest.mark.parametrize("name", AGG_CASES)
def test_oracle_volume_fractions_are_exact(oracle, name):
    """`volume_fractions` of every cut cell and both selectors against `exact_fraction`; the two sides add up to 1."""
    O = oracle
    cs = X.build_case(O, name)
    om, phi, dom = _oracle_setup(O, cs)
    assert np.array_equal(np.flatnonzero(dom == 0), cs["cut"])
    got = {}
    for sel in SELECTORS:
        got[sel] = np.where(dom == 0, O.volume_fractions(om, om.conn, phi, dom, sel), 0.0)
        worst = check_fractions(name, cs, sel, got[sel])
        _report("fractions", f"oracle {name} {sel} ({cs['cut'].size} cut cells)", worst)
        assert 0.0 < worst <= TOL
    assert np.abs(got["phi<0"] + got["phi>0"] - 1.0)[cs["cut"]].max() <= TOL


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", AGG_CASES)
def test_the_oracle_aggregation_is_a_valid_one(oracle, name, policy):
    """The reference itself satisfies the oracle-free statement: fractions, classes from the exact fractions, structure,
    rootless cells, pairs; both selectors, thresholds 0.3, 0.6 and 1.0."""
    O = oracle
    cs = X.build_case(O, name)
    om, phi, dom = _oracle_setup(O, cs)
    thresholds_are_decidable(name, cs)
    for sel in SELECTORS:
        for thr in AGG_THRESHOLDS:
            agg = O.cell_aggregation(om, om.conn, phi, dom, sel, thr, root_policy=policy, allow_rootless=True)
            assert check_fractions(name, cs, sel, agg["cut_volume_fraction"]) <= TOL
            pairs, deepest, lonely = check_aggregation(name, cs, sel, thr, policy, agg)
            assert np.array_equal(O.extension_pairs(agg), pairs)
            print(f"EXACT aggregation: oracle {name} {sel} thr {thr} {policy}: pairs {len(pairs)} deepest {deepest} rootless {lonely}")
