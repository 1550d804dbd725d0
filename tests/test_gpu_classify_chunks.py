"""The block decision of the culled classification from mesh-static chunk descriptors (the aligned 16 B words of the
sign-code array that a block's vertex runs touch, with byte masks; the quarters of a mixed block from the words their
spans lie in) against the run decoder (CFX_CLASSIFY_CHUNKS=0), the cell loop (CFX_CLASSIFY_CULL=0) and the oracle: same
domain array and located lists bit for bit, on the first cut and on a second one that reuses the table, and the same
number of blocks decided whole (`CutData.uniform_blocks`) as a numpy model of the runs counts
(tests/classify_chunks_model.py, itself checked by tests/test_classify_chunks_reference.py).  Every case first asserts,
from that model, the properties it is there for."""
import numpy as np
import pytest

import classify_chunks_model as M

pytestmark = pytest.mark.gpu

# (CFX_CLASSIFY_CULL, CFX_CLASSIFY_CHUNKS): the cell loop; the chunk descriptors, named and by default; the run decoder
SETTINGS = [("0", None), ("1", "1"), ("1", None), ("1", "0")]


def residues(model):
    heads = {int(r[0]) % 16 for m in model for r in m.runs}
    tails = {int(r[0] + r[1] - 1) % 16 for m in model for r in m.runs}
    return heads, tails


def span(model, what):
    v = [len(getattr(m, what)) for m in model if m.summary]
    return min(v), max(v)


def box(oracle, tdim, n):
    om = oracle.mesh_box(tdim, n)
    return tdim, om.x, om.conn


def permuted(oracle, n, group, holds):
    """the n^3 box with its vertex ids permuted in groups: the first seed for which `holds(model)`."""
    tdim, x, conn = box(oracle, 3, n)
    for seed in range(20):
        new = M.permute_in_groups(x.shape[0], group, np.random.default_rng(seed))
        conn2 = np.ascontiguousarray(new[conn].astype(np.int32))
        if holds(M.blocks(conn2)):
            x2 = np.empty_like(x)
            x2[new] = x
            return tdim, x2, conn2
    raise AssertionError("no seed gives the case its properties")


def case_box14(oracle):
    tdim, x, conn = box(oracle, 3, 14)
    model = M.blocks(conn)
    heads, tails = residues(model)
    assert len(model) == 17 and conn.shape[0] - 16 * M.BLOCK == 80        # odd: the last wavefront has one block
    assert span(model, "runs") == (2, 4) and span(model, "words") == (4, 29) and all(m.chunked for m in model)
    assert len(heads) == 16 and len(tails) == 15
    assert any(sum(1 for r in m.runs if r[0] // 16 <= w <= (r[0] + r[1] - 1) // 16) > 1 for m in model for w in m.words)
    return tdim, x, conn, model


def case_box21(oracle):
    tdim, x, conn = box(oracle, 3, 21)
    model = M.blocks(conn)
    heads, tails = residues(model)
    assert len(model) == 55 and conn.shape[0] - 54 * M.BLOCK == 270 and len(heads) == 16 and len(tails) == 16
    assert all(m.chunked for m in model)
    return tdim, x, conn, model


def case_box16(oracle):
    tdim, x, conn = box(oracle, 3, 16)
    model = M.blocks(conn)
    assert len(model) == 24 and conn.shape[0] == 24 * M.BLOCK and x.shape[0] % 16 == 1     # the last word is partial
    assert (x.shape[0] - 1) // 16 in model[-1].words and all(m.chunked for m in model)
    return tdim, x, conn, model


def case_square100(oracle):
    tdim, x, conn = box(oracle, 2, 100)
    model = M.blocks(conn)
    assert len(model) == 20 and span(model, "runs") == (1, 1) and span(model, "words") == (24, 40)   # a lane's second word
    assert all(m.chunked for m in model)
    return tdim, x, conn, model


def case_slab(oracle):
    x, conn = M.kuhn_slab(200, 2, 2)
    model = M.blocks(conn)
    assert len(model) == 5 and span(model, "runs") == (4, 6) and span(model, "words") == (33, 49)
    assert max(int(r[1]) for m in model for r in m.runs) >= 170 and all(m.chunked for m in model)   # the benchmark's block shape
    return 3, x, conn, model


def case_groups24(n):
    def case(oracle):
        def holds(model):
            short = sum(int((m.runs[:, 1] < 16).sum()) for m in model)
            return all(m.chunked for m in model) and span(model, "runs")[1] >= 16 and short >= 24
        tdim, x, conn = permuted(oracle, n, 24, holds)
        model = M.blocks(conn)
        assert holds(model) and span(model, "runs")[0] >= 5 and span(model, "words")[1] > 32
        return tdim, x, conn, model
    return case


def case_groups100(n):
    def case(oracle):
        def holds(model):
            return all(m.chunked for m in model) and 3 <= span(model, "runs")[0] and span(model, "runs")[1] <= 10
        tdim, x, conn = permuted(oracle, n, 100, holds)
        return tdim, x, conn, M.blocks(conn)
    return case


def case_groups5(n):
    def case(oracle):
        def holds(model):   # all blocks but one have no summary and take the cell loop
            return sum(1 for m in model if m.summary) == 1 and min(len(m.runs) for m in model if not m.summary) > M.MAX_RUNS
        tdim, x, conn = permuted(oracle, n, 5, holds)
        return tdim, x, conn, M.blocks(conn)
    return case


def case_gaps(n):
    """One-id gaps: in every 12th word the ids at bytes 1, 3, 5, 7, 9 belong to vertices of a distant block, so a block
    reads bytes 0, 2, 4, 6, 8, 10.. of such a word: six runs in one word, four of them a single id.  In the table's build
    the single-id runs open no word of their own (several lanes in a row) and OR their byte into the slot of the word
    that an earlier run opened."""
    def case(oracle):
        tdim, x, conn = box(oracle, 3, n)
        far = ((x.shape[0] + 15) // 16) // 2
        new = M.swap_odd_bytes(x.shape[0], 12, far)
        assert np.array_equal(np.sort(new), np.arange(x.shape[0]))
        conn = np.ascontiguousarray(new[conn].astype(np.int32))
        model = M.blocks(conn)
        crowded = [m for m in model if m.chunked and max(M.runs_in_word(m, w) for w in m.words) >= 5]
        assert len(crowded) >= 10 and sum(1 for m in model if m.summary) >= len(model) - 2
        # ... a run wholly inside the word the run before ended in, followed by a further run in that same word
        m = crowded[0]
        w = next(w for w in sorted(m.words) if M.runs_in_word(m, w) >= 5)
        inside = [r for r in m.runs if r[0] // 16 == w and (r[0] + r[1] - 1) // 16 == w]
        assert len(inside) >= 4 and all(r[1] == 1 for r in inside[:4])
        assert span(model, "runs")[1] >= 30
        x2 = np.empty_like(x)
        x2[new] = x
        return tdim, x2, conn, model
    return case


def case_over_the_table(oracle):
    """Blocks with a summary and more words than the table holds: the run decoder, in two rounds (771 ids, 768 a
    round).  A strip of 1024 x 2 squares, vertices numbered across the strip and permuted in groups of 33: a group on
    its own is 33 bytes, three words.  (Disjoint tetrahedra do not serve: 4096 distinct ids per block are more than a
    summary is built from, so those blocks go cell by cell.)"""
    x, conn0 = M.strip_2d(1024, 2)
    for seed in range(20):
        new = M.permute_in_groups(x.shape[0], 33, np.random.default_rng(seed))
        conn = np.ascontiguousarray(new[conn0].astype(np.int32))
        model = M.blocks(conn)
        if any(m.summary and not m.chunked for m in model) and any(m.chunked for m in model):
            break
    else:
        raise AssertionError("no seed gives the case its properties")
    assert len(model) == 4 and all(m.summary and m.ids.size == 771 for m in model)
    assert any(len(m.words) == M.MAX_WORDS for m in model)                       # ... and one block that fills it exactly
    assert max(len(m.words) for m in model) > M.MAX_WORDS and span(model, "runs")[1] <= M.MAX_RUNS
    x2 = np.empty_like(x)
    x2[new] = x
    return 2, x2, conn, model


CASES = {
    "box14": case_box14, "box21": case_box21, "box16": case_box16, "square100": case_square100, "slab200x2x2": case_slab,
    "box14-groups24": case_groups24(14), "box21-groups24": case_groups24(21),
    "box14-groups100": case_groups100(14), "box21-groups100": case_groups100(21),
    "box14-groups5": case_groups5(14), "box21-groups5": case_groups5(21),
    "strip-over-the-table": case_over_the_table,
    "box14-gaps": case_gaps(14), "box21-gaps": case_gaps(21),
}


def one_vertex_differs(model, nnodes):
    """Three level sets, all negative but for one positive vertex: at the first id of a run, at the last id of a run,
    and at an id just outside a run but inside one of its 16 B words.  The block and the run: the first block with a
    summary (one decided from the chunk table if there is any) that has a run starting inside a word / ending inside
    a word."""
    order = sorted((m for m in model if m.summary), key=lambda m: not m.chunked)
    out = {}
    head = next((m, r) for m in order for r in m.runs if r[0] % 16 != 0)
    tail = next((m, r) for m in order for r in m.runs if (r[0] + r[1] - 1) % 16 != 15 and r[0] + r[1] < nnodes)
    for name, (m, r), v in (("first-of-run", head, int(head[1][0])), ("last-of-run", tail, int(tail[1][0] + tail[1][1] - 1)),
                            ("before-run", head, int(head[1][0]) - 1), ("after-run", tail, int(tail[1][0] + tail[1][1]))):
        phi = -np.ones(nnodes)
        phi[v] = 1.0
        inside = v in m.ids
        assert inside == (name in ("first-of-run", "last-of-run")) and v // 16 in m.words, name
        # the model's count: the neighbour of a run leaves its block uniform (the byte masks, from the superset side)
        assert bool(np.all(phi[m.ids] < 0)) == (not inside), name
        out["one-" + name] = phi
    # ... and one positive vertex in the second and in the last word of the block with the most words among those
    # decided from the table: whichever way the words are dealt to the lanes, one of the two is no lane's first word
    chunked = [m for m in order if m.chunked and len(m.words) >= 2]
    if chunked:
        m = max(chunked, key=lambda m: len(m.words))
        for name, w in (("second-word", sorted(m.words)[1]), ("last-word", sorted(m.words)[-1])):
            v = int(m.ids[m.ids // 16 == w][0])
            phi = -np.ones(nnodes)
            phi[v] = 1.0
            out["one-in-" + name] = phi
    # ... and, where a block decided from the table has five or more runs in one word: one positive vertex at each of two
    # single-id runs inside that word (the second and the last of them) and at the one-id gap behind the second, which is
    # no vertex of the block (its uniform count must not drop)
    crowded = [(m, w) for m in order if m.chunked for w in sorted(m.words) if M.runs_in_word(m, w) >= 5]
    if crowded:
        m, w = crowded[0]
        singles = [int(r[0]) for r in m.runs if r[1] == 1 and r[0] // 16 == w]
        assert len(singles) >= 3
        for name, v, inside in (("second-single-of-word", singles[1], True), ("last-single-of-word", singles[-1], True),
                                ("gap-in-word", singles[1] + 1, False)):
            phi = -np.ones(nnodes)
            phi[v] = 1.0
            assert (v in m.ids) == inside and v // 16 == w and bool(np.all(phi[m.ids] < 0)) == (not inside), name
            out["one-" + name] = phi
    return out


def level_sets(tdim, x, model):
    nnodes = x.shape[0]
    rng = np.random.default_rng(12)
    centre = np.array([0.47, 0.43, 0.41])[:tdim]
    unit = x[:, :tdim] / np.ptp(x[:, :tdim], axis=0)                                  # (slab and strip: stretched to the unit box)
    levels = {
        "sphere": np.linalg.norm(unit - centre, axis=1) - 0.31,                       # the benchmark's
        "zeros": np.round(8.0 * (x[:, 0] - 0.5)) / 8.0,                               # exact zeros on a vertex plane
        "random": rng.standard_normal(nnodes),
        "negative": -np.ones(nnodes), "positive": np.ones(nnodes),
    }
    assert (levels["zeros"] == 0).any() and (levels["zeros"] < 0).any() and (levels["zeros"] > 0).any()
    levels.update(one_vertex_differs(model, nnodes))
    return levels


@pytest.mark.parametrize("name", list(CASES))
def test_chunked_block_decision_equals_the_run_decoder_the_cell_loop_and_the_oracle(oracle, name, monkeypatch):
    import cutfemx_amd as cfx
    O = oracle
    tdim, x, conn, model = CASES[name](oracle)
    levels = level_sets(tdim, x, model)
    want = {}
    for lname, phi in levels.items():
        for shift in (0.0, 0.03):
            dom = O.classify(conn, phi + shift)
            want[lname, shift] = (dom, O.locate_entities(dom, "phi<0"), O.locate_entities(dom, "phi=0"),
                                  M.uniform_blocks(model, phi + shift))
    nsummary = sum(1 for m in model if m.summary)
    assert want["negative", 0.0][3] == (nsummary, 0) and want["positive", 0.0][3] == (0, nsummary)
    for cull, chunks in SETTINGS:
        monkeypatch.setenv("CFX_CLASSIFY_CULL", cull)
        if chunks is None:
            monkeypatch.delenv("CFX_CLASSIFY_CHUNKS", raising=False)
        else:
            monkeypatch.setenv("CFX_CLASSIFY_CHUNKS", chunks)
        mesh = cfx.Mesh.from_arrays(tdim, x, conn)         # (its tables are built by the first cut and kept)
        V = cfx.FunctionSpace(mesh, 1)
        for lname, phi in levels.items():
            for shift in (0.0, 0.03):                      # the second cut reuses the table
                cd = cfx.cut(cfx.Function(V, phi + shift))
                dom, inside, cutc, uniform = want[lname, shift]
                tag = (name, lname, shift, cull, chunks)
                assert np.array_equal(cd.domain(), dom), tag
                assert np.array_equal(cfx.locate_entities(cd, "phi<0"), inside), tag
                assert np.array_equal(cfx.locate_entities(cd, "phi=0"), cutc), tag
                assert cd.uniform_blocks() == (None if cull == "0" else uniform), tag
