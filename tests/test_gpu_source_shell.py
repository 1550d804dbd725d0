"""Shell hexes of the closed-form P1 source term (round 9).  With the closed form on the complete lattice rows
(tests/test_gpu_lattice_source.py) a hex of six Kuhn tets writes something that somebody reads only if it has a tet
that is an entity of the integral and has a corner row off the closed form.  The engine finds those hexes from the
rows that read them -- the special rows and the plain rows without the closed form mark the hexes of their marked
cells in a bit set, the set bits are compacted into a list, the hex kernel takes one list entry per lane -- instead of
sifting every hex of the entity list (CFX_SOURCE_SHELL=0, round 8).

Every case assembles b under CFX_STAGING_NAN=1 and compares it with the same call under CFX_SOURCE_SHELL=0 bit for
bit (a hex writes only its own slots and the fold's order is fixed: equality is the derived tolerance), with the oracle
to 1e-12, and the counter FunctionSpace.source_shell_hexes() with the definition above evaluated in numpy from the
oracle's entity list and the closed-form rows (test_gpu_lattice_source.eligible_rows).

Which rows mark: a form of the entity integral alone has no special rows -- the rows at the edge of the list are plain
rows whose cells do not all carry the mark ("odd" plain rows, no segment), and they are the readers of the per-cell
records in every case below that has no rule integral.  Special rows exist where the form has runtime rules (the
integral in cell slot 1, the Poisson system's linear form of the step loops).  A restricted list (a caller's array)
does not take the hex-group path at all (tests/test_gpu_source_groups_edges.py: no provenance), so the case below
asserts that the shell path is refused with it: counter 0, b equal to the switched-off call."""
import os

import numpy as np
import pytest

from helpers import groups_expected, level_set_values, oracle_poisson, profiled, rel_err
from test_gpu_lattice_source import NAN, bitwise, closed_expected, eligible_rows, gpu_b

pytestmark = pytest.mark.gpu
RTOL = 1e-12
# the engine takes the shell path from 4 M entities on (at 128^3 the sift is as fast); =2 takes it at any length
ON = dict(NAN, CFX_SOURCE_SHELL="2")
SIFT = dict(NAN, CFX_SOURCE_SHELL="0")


def shell_expected() -> bool:
    """Under CFX_SOURCE_SHELL=2 (every `on` call here sets it), wherever the closed form is on."""
    return closed_expected()


def shell_hexes(om, entities, closed):
    """The definition: hexes with a tet in `entities` that has a corner row off the closed form."""
    entities = np.asarray(entities)
    off = ~np.all(closed[om.conn[entities]], axis=1)
    return np.unique(entities[off] // 6)


def same(a, b):
    return np.array_equal(a, b) if bitwise() else rel_err(a, b) < 1e-13


def check_shell(cfx, O, om, mesh, phi, monkeypatch, *, selector="phi<0", field="poisson", scale=1.25, q=4, closed=None,
                lattice=True, with_rules=False):
    """One source integral over the located list of `selector`: shell list, sift, oracle, counter."""
    fg, fo = {"poisson": (cfx.fem.F_POISSON_RHS, O.F_POISSON_RHS), "sinprod": (cfx.fem.F_SINPROD, O.F_SINPROD)}[field]
    dom = O.classify(om.conn, phi)
    ents = O.locate_entities(dom, selector)
    oints = [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(fo, scale), qdegree=q)]
    V = cfx.FunctionSpace(mesh, 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, selector)
    rules = None
    if with_rules:   # a rules-only cell integral first: the uncut entities sit in cell slot 1 (mark bit 2)
        oints.insert(0, O.Integral(O.CELL, O.L_SOURCE, rules=O.runtime_quadrature(om, om.conn, phi, dom, selector, q),
                                   params=(fo, scale), qdegree=q))
        rules = cfx.runtime_quadrature(cd, selector, q)
    ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1), oints)
    if closed is None:
        closed = eligible_rows(om, ents)
    want = shell_hexes(om, ents, closed).size if lattice and shell_expected() else 0
    on, names, rows = gpu_b(cfx, V, cells, fg, scale, q, ON, monkeypatch, rules=rules)
    ran = V.source_shell_hexes()
    off, names0, rows0 = gpu_b(cfx, V, cells, fg, scale, q, SIFT, monkeypatch, rules=rules)
    ran0 = V.source_shell_hexes()
    print(f"shell hexes {ran} (definition {want}, hexes with an entity {np.unique(np.asarray(ents) // 6).size}), "
          f"closed-form rows {rows}, oracle {rel_err(on, ref):.2e}, shell/sift {rel_err(on, off):.2e}")
    assert ("source_groups" in names) == groups_expected() and ("source_groups" in names0) == groups_expected()
    assert ("source_shell" in names) == (lattice and shell_expected()) and "source_shell" not in names0, sorted(names)
    assert rows == rows0
    assert np.all(np.isfinite(on)) and np.all(np.isfinite(off))
    assert same(on, off), rel_err(on, off)
    assert rel_err(on, ref) < RTOL and rel_err(off, ref) < RTOL, (rel_err(on, ref), rel_err(off, ref))
    assert (ran, ran0) == (want, 0), (ran, ran0, want)
    return on, ran, ents, closed


# --------------------------------------------------------------------------- cases
@pytest.mark.parametrize("n", [8, 16, 32])
def test_generated_boxes(oracle, monkeypatch, n):
    """8^3: almost no bulk.  16^3: the smallest box with hexes whose six entity bits straddle two 64-bit words (6 h mod
    64 > 58 first at h = 10) inside the sphere.  32^3: a bulk several blocks of the sift deep."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, n)
    phi = level_set_values(om.x, 3)
    _, ran, ents, closed = check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, n), phi, monkeypatch)
    hexes = shell_hexes(om, ents, closed)
    with_entity = np.unique(np.asarray(ents) // 6)
    if n >= 16:
        assert np.any((6 * hexes) % 64 > 58)                 # straddling hexes are in the list
        assert hexes.size < with_entity.size                 # ... and there is a bulk that is left out
    if n == 32:
        assert with_entity.size - hexes.size > 2 * 256


def test_inside_reaches_the_box_faces(oracle, monkeypatch):
    """Rows on the box faces are no lattice rows: the shell includes the hexes along the faces."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.0, 0.1, 0.0]), axis=1) - 0.7
    _, ran, ents, closed = check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch)
    hexes = shell_hexes(om, ents, closed)
    assert 0 in hexes and hexes.size < np.unique(np.asarray(ents) // 6).size


def test_one_moved_vertex(oracle, monkeypatch):
    """One interior vertex moved by 0.2 h: 15 rows in the middle of the bulk lose the closed form; their hexes must be in
    the list (under CFX_STAGING_NAN a missing one turns b into NaN)."""
    import cutfemx_amd as cfx
    n = 16
    om0 = oracle.mesh_box(3, n)
    x = om0.x.copy()
    v = 6 + (n + 1) * (7 + (n + 1) * 7)
    x[v, 1] += 0.2 / n
    om = oracle.Mesh(3, x, om0.conn)
    phi = level_set_values(om.x, 3)
    touched = np.zeros(om.nnodes, dtype=bool)
    touched[om.conn[np.any(om.conn == v, axis=1)].ravel()] = True
    ents = oracle.locate_entities(oracle.classify(om.conn, phi), "phi<0")
    closed = eligible_rows(om, ents) & ~touched
    before = shell_hexes(om, ents, eligible_rows(om, ents)).size
    _, ran, _, _ = check_shell(cfx, oracle, om, cfx.Mesh.from_arrays(3, om.x, om.conn), phi, monkeypatch, closed=closed)
    assert shell_hexes(om, ents, closed).size > before


def test_a_box_that_is_no_exact_lattice(oracle, monkeypatch):
    """n = 20: no lattice flags, no closed form: the path is not taken, the counter reads 0."""
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 20)
    phi = level_set_values(om.x, 3)
    check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, 20), phi, monkeypatch, lattice=False)


def test_a_restricted_list_is_refused(oracle, monkeypatch):
    """The inside list without a contiguous range of cells (a device array of the caller's): plain rows at the edge of the
    gap have unmarked cells around them.  Such a list does not take the hex-group path at all (no provenance), so the
    shell path must not be taken either: counter 0, b as switched off and as the oracle's.

    The hazard this case was meant to carry -- "odd" plain rows, whose hexes only the mark pass of the plain rows
    finds -- is carried by the other cases instead: every form here without a rule integral has no special rows, so
    the rows at the edge of its located list are odd plain rows (boxes, box faces, moved vertex, phi>0, degrees, slab,
    twice, fresh space: the 13 tests that fail when the mark pass skips the rows with vec_t2off == 0)."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    om = O.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    inside = O.locate_entities(O.classify(om.conn, phi), "phi<0")
    k = inside.size // 2
    ents = np.concatenate([inside[:k - 40], inside[k + 41:]])
    ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                            [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(O.F_POISSON_RHS, 1.25), qdegree=4)])
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
    cells = torch.tensor(ents, device="cuda")
    out = {}
    for tag, env in (("on", ON), ("off", SIFT)):
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_POISSON_RHS, 1.25), qdegree=4)], V, rank=1)
            b, names = profiled(lambda: fem.assemble_vector(L))
        assert "source_groups" not in names and "source_shell" not in names, sorted(names)
        assert V.source_shell_hexes() == 0
        out[tag] = np.asarray(b.cpu() if hasattr(b, "cpu") else b).copy()
    assert same(out["on"], out["off"]) and rel_err(out["on"], ref) < RTOL


def test_the_outside_list(oracle, monkeypatch):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, selector="phi>0")


def test_source_integral_in_cell_slot_one(oracle, monkeypatch):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, with_rules=True)


@pytest.mark.parametrize("q", [1, 2, 4, 8])
def test_degrees(oracle, monkeypatch, q):
    import cutfemx_amd as cfx
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    check_shell(cfx, oracle, om, cfx.Mesh.create_box(3, 16), phi, monkeypatch, field="sinprod", scale=-0.75, q=q)


def test_slab_where_every_hex_is_shell(oracle, monkeypatch):
    """128 x 128 x 2: every vertex but the middle plane's lies on a box face, every hex has a corner there."""
    import cutfemx_amd as cfx
    slab = cfx.Mesh.create_slab(128, 60, 2)
    om = oracle.Mesh(3, slab.x, slab.conn)
    phi = np.linalg.norm(om.x[:, :3] - np.array([0.47, 0.43, 61.0 / 128]), axis=1) - 0.31
    _, ran, ents, closed = check_shell(cfx, oracle, om, slab, phi, monkeypatch)
    assert shell_hexes(om, ents, closed).size == np.unique(np.asarray(ents) // 6).size


def test_assembling_twice_with_one_plan(oracle, monkeypatch):
    """One form, two assemblies into one unzeroed b: the bit set must be clear the second time (a leftover bit of the
    first assembly is harmless, a count that doubled or a list out of order is not), the counter speaks of the last."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    om = O.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    ents = O.locate_entities(O.classify(om.conn, phi), "phi<0")
    ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                            [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(O.F_POISSON_RHS, 1.25), qdegree=4)])
    want = shell_hexes(om, ents, eligible_rows(om, ents)).size if shell_expected() else 0

    def twice(env):
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
            cd = cfx.cut(cfx.Function(V, phi))
            cells = cfx.locate_entities_device(cd, "phi<0")
            L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_POISSON_RHS, 1.25), qdegree=4)], V, rank=1)
            b = torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)
            fem.assemble_vector(L, b)
            once, r1 = b.cpu().numpy().copy(), V.source_shell_hexes()
            fem.assemble_vector(L, b)
            return once, b.cpu().numpy().copy(), r1, V.source_shell_hexes()
    once, both, r1, r2 = twice(ON)
    once0, both0, z1, z2 = twice(SIFT)
    assert (r1, r2, z1, z2) == (want, want, 0, 0)
    assert same(once, once0) and same(both, both0)
    assert rel_err(once, ref) < RTOL and rel_err(both, 2.0 * ref) < RTOL


def test_linear_form_first_on_a_fresh_space(oracle, monkeypatch):
    """Nobody asked the space for its lattice table: the linear form builds it, and the counter with it."""
    import cutfemx_amd as cfx
    from cutfemx_amd import fem
    O = oracle
    om = O.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    ents = O.locate_entities(O.classify(om.conn, phi), "phi<0")
    ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                            [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(O.F_POISSON_RHS, 1.0), qdegree=4)])
    monkeypatch.setenv("CFX_STAGING_NAN", "1")
    monkeypatch.setenv("CFX_SOURCE_SHELL", "2")
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, "phi<0")
    L = fem.form([fem.Integral(fem.SOURCE, cells=cells, params=(fem.F_POISSON_RHS, 1.0), qdegree=4)], V)
    b = fem.assemble_vector(L)                           # (first call on the space)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    assert rel_err(b, ref) < RTOL
    assert V.source_shell_hexes() == (shell_hexes(om, ents, eligible_rows(om, ents)).size if shell_expected() else 0)


def test_in_steps_with_and_without_forced_overflow(oracle, monkeypatch):
    """Eight steps of a moving sphere at 16^3, the Poisson system's linear form: the plain call sequence, sync-free
    steps and steps with forced overflow margins, each against the oracle and the three against each other bit for
    bit; the same three with the sift, bit for bit again.  A step that fits takes one pass and one host round trip
    (the read-back at its end)."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import _lib, poisson
    n, steps = 16, 8
    om = oracle.mesh_box(3, n)
    xt = torch.tensor(om.x.copy(), device="cuda")

    def phi_of(k):
        c = torch.tensor([0.40 + 0.3 / n * k, 0.45, 0.5], device="cuda", dtype=torch.float64)
        return torch.linalg.norm(xt - c, dim=1) - 0.27

    def body(V, f, state):
        if state.get("cd") is None:
            state["cd"] = cfx.cut(f)
        else:
            cfx.update(state["cd"])
        s = poisson.build_forms(V, state["cd"], order=4)
        return cfx.fem.assemble_vector(s.L, state["b"])

    def loop(tag, margin, in_steps):
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        phi = torch.empty(om.nnodes, device="cuda", dtype=torch.float64)
        f = cfx.Function(V, phi)
        state = {"cd": None, "b": torch.zeros(om.nnodes, device="cuda", dtype=torch.float64)}
        key = f"test-source-shell-{tag}"
        cfx.forget_step_history(key)
        out, passes, syncs, ran = [], [], [], []
        try:
            if margin is not None:
                cfx.set_step_margin(margin, 0)
            for k in range(steps):
                phi.copy_(phi_of(k))
                state["b"].zero_()
                info = {"passes": 1}
                s0 = _lib.sync_count()
                b = cfx.run_step(lambda: body(V, f, state), key=key, info=info) if in_steps else body(V, f, state)
                syncs.append(_lib.sync_count() - s0)
                passes.append(info["passes"])
                out.append(b.cpu().numpy().copy())
                ran.append(V.source_shell_hexes())
        finally:
            cfx.set_step_margin()
        return out, passes, syncs, ran

    monkeypatch.setenv("CFX_STAGING_NAN", "1")
    monkeypatch.setenv("CFX_SOURCE_SHELL", "2")
    plain, _, _, ran = loop("plain", None, False)
    want = []
    for k in range(steps):
        phik = phi_of(k).cpu().numpy()
        ref = oracle_poisson(oracle, om, phik)
        assert rel_err(plain[k], ref["b"]) < RTOL, (k, rel_err(plain[k], ref["b"]))
        ents = oracle.locate_entities(oracle.classify(om.conn, phik), "phi<0")
        want.append(shell_hexes(om, ents, eligible_rows(om, ents)).size if shell_expected() else 0)
    assert ran == want, (ran, want)
    assert len(set(want)) > 1 or not shell_expected()        # the shell really changes from step to step
    switches = [k for k in os.environ if k.startswith("CFX_") and k not in ("CFX_STAGING_NAN", "CFX_SOURCE_SHELL", "CFX_STEP_DEBUG", "CFX_COUNT_SYNC", "CFX_DEVICE")]
    for tag, margin in (("steps", None), ("forced", 0.97)):
        got, passes, syncs, ran = loop(tag, margin, True)
        print(tag, "passes", passes, "host round trips", syncs)
        assert ran == want, (tag, ran, want)
        if margin is not None and os.environ.get("CFX_STEP_SPECULATE") != "0":
            assert max(passes) == 2, passes
        if margin is None and not switches:
            assert passes[1:] == [1] * (steps - 1), passes
            assert syncs[1:] == [1] * (steps - 1), syncs
        for k in range(steps):
            assert same(got[k], plain[k]), (tag, k)
    with monkeypatch.context() as mp:
        mp.setenv("CFX_SOURCE_SHELL", "0")
        for tag, margin, in_steps in (("sift-plain", None, False), ("sift-steps", None, True)):
            got, _, _, ran = loop(tag, margin, in_steps)
            assert ran == [0] * steps
            for k in range(steps):
                assert same(got[k], plain[k]), (tag, k)


def test_a_second_level_set_on_the_same_space(oracle, monkeypatch):
    """The bit set after an assembly, directly: a small sphere first, then a larger one around it on the SAME space.  The
    first shell lies in the bulk of the second, where its hexes have marked tets: a bit that survived the first
    assembly would run the body there, and the counter (hexes with a marked tet that the body ran) would exceed the
    definition for the second level set.  (The other order cannot show it: stale hexes outside the new domain have no
    marked tet and are not counted.)"""
    import cutfemx_amd as cfx
    O = oracle
    om = O.mesh_box(3, 32)
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 32), 1)
    centre = np.array([0.47, 0.43, 0.41])
    for radius in (0.18, 0.36):
        phi = np.linalg.norm(om.x[:, :3] - centre, axis=1) - radius
        ents = O.locate_entities(O.classify(om.conn, phi), "phi<0")
        ref = O.assemble_vector(om, O.Space(om.conn, om.nnodes, 1),
                                [O.Integral(O.CELL, O.L_SOURCE, entities=ents, params=(O.F_POISSON_RHS, 1.25), qdegree=4)])
        want = shell_hexes(om, ents, eligible_rows(om, ents)).size if shell_expected() else 0
        cd = cfx.cut(cfx.Function(V, phi))
        cells = cfx.locate_entities_device(cd, "phi<0")
        b, names, _ = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, ON, monkeypatch)
        assert V.source_shell_hexes() == want, (radius, V.source_shell_hexes(), want)
        assert rel_err(b, ref) < RTOL
    assert want > 0 or not shell_expected()


def test_short_lists_keep_the_sift_by_default(oracle, monkeypatch):
    """Without the switch the path is chosen by the length of the entity list (4 M entities): 16^3 keeps the sift."""
    import cutfemx_amd as cfx
    if os.environ.get("CFX_SOURCE_SHELL"):
        return       # (a mode of tools/test_modes.sh sets the switch: the default choice is not what runs)
    om = oracle.mesh_box(3, 16)
    phi = level_set_values(om.x, 3)
    V = cfx.FunctionSpace(cfx.Mesh.create_box(3, 16), 1)
    cd = cfx.cut(cfx.Function(V, phi))
    cells = cfx.locate_entities_device(cd, "phi<0")
    b, names, rows = gpu_b(cfx, V, cells, cfx.fem.F_POISSON_RHS, 1.25, 4, NAN, monkeypatch)
    assert "source_shell" not in names and V.source_shell_hexes() == 0
    assert ("source_groups" in names) == groups_expected() and rows == (223 if closed_expected() else 0)


# --------------------------------------------------------------------------- the tile lists of the bilinear form
def tile_rule(rows, templ):
    """The rule in numpy: a tile (rows // 16) with a plain row that is no template row is listed once, at the position of
    the first such row."""
    tiles = rows // 16
    first, ids = [], []
    for t in np.unique(tiles):
        pos = np.flatnonzero((tiles == t) & (templ == 0))
        if pos.size:
            first.append(pos[0])
            ids.append(t)
    return np.array(first, dtype=np.int32), np.array(ids, dtype=np.int32)


@pytest.mark.parametrize("n", [16, 32])
def test_tile_lists_against_the_rule(oracle, n):
    """lat_tile_first / lat_tile_id of the Poisson system's bilinear form (the write pass decides them from wavefront
    ballots): array-equal to the numpy statement of the rule, from a plain call sequence (count, scan, write) and from
    sync-free steps (one chained launch), whose lists must also equal each other."""
    import torch

    import cutfemx_amd as cfx
    from cutfemx_amd import poisson
    om = oracle.mesh_box(3, n)
    # (a sphere that reaches the box faces: the rows on the faces are plain and no lattice rows, so tiles with template
    # rows only, tiles that start with a listed row and tiles that start with template rows all occur)
    phi = torch.tensor(np.linalg.norm(om.x[:, :3] - np.array([0.0, 0.1, 0.0]), axis=1) - 0.7, device="cuda")
    got = {}
    for tag in ("plain", "steps"):
        V = cfx.FunctionSpace(cfx.Mesh.create_box(3, n), 1)
        f = cfx.Function(V, phi)
        state = {}

        def body():
            if "cd" not in state:
                state["cd"] = cfx.cut(f)
            else:
                cfx.update(state["cd"])
            state["s"] = poisson.build_forms(V, state["cd"], order=4)
            return cfx.fem.assemble_matrix(state["s"].a)
        key = f"test-tile-lists-{n}"
        cfx.forget_step_history(key)
        for k in range(3):
            A = cfx.run_step(body, key=key) if tag == "steps" else body()
        lists = state["s"].a.lattice_tile_lists()
        if lists is None:
            assert any(k.startswith("CFX_") and k not in ("CFX_DEVICE", "CFX_COUNT_SYNC", "CFX_STEP_DEBUG") for k in os.environ), \
                "no filtered tile list on an exact lattice in the default mode"
            return
        rows, templ = lists["plain_rows"], lists["templ"]
        assert np.all(np.diff(rows) > 0)
        first, ids = tile_rule(rows, templ)
        print(f"{tag}: {rows.size} plain rows, {int(templ.sum())} template rows, {first.size} listed tiles of {np.unique(rows // 16).size}")
        assert np.array_equal(lists["tile_first"], first) and np.array_equal(lists["tile_id"], ids)
        if n == 32:
            assert 0 < first.size < np.unique(rows // 16).size     # some tiles are all template rows, some are not
            assert np.any(first != np.searchsorted(rows // 16, ids))  # ... and some listed tiles start with template rows
        got[tag] = lists
    for name in ("plain_rows", "templ", "tile_first", "tile_id"):
        assert np.array_equal(got["plain"][name], got["steps"][name]), name
