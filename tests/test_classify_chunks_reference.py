"""The numpy model of runs and 16 B words per block (tests/classify_chunks_model.py) checked against first principles
on the CPU: the words cover exactly the bytes of the runs, the runs are exactly the distinct ids.  No GPU, no engine."""
import numpy as np
import pytest

import classify_chunks_model as M


def bytes_of(words):
    return sorted(16 * w + i for w, mask in words.items() for i in range(16) if (mask >> i) & 1)


def random_id_sets(rng):
    yield np.array([5]), "one id"
    yield np.arange(16, 32), "one whole word"
    yield np.arange(15, 33), "a word and a byte either side"
    yield np.array([0, 2, 4, 6, 8, 10, 12, 14, 15, 16]), "many runs in one word"
    for k in range(40):
        n = int(rng.integers(1, 700))
        lo = int(rng.integers(0, 5000))
        ids = np.unique(rng.integers(lo, lo + int(rng.integers(n, 4 * n + 2)), size=n))
        yield ids, f"random {k}"
    for head in range(16):
        for tail in range(16):
            yield np.arange(32 + head, 64 + tail + 1), f"head {head} tail {tail}"


def test_runs_are_the_ids_and_words_cover_exactly_the_run_bytes():
    rng = np.random.default_rng(3)
    for ids, name in random_id_sets(rng):
        runs = M.runs_of(ids)
        back = np.concatenate([np.arange(s, s + n) for s, n in runs])
        assert np.array_equal(back, ids), name
        assert np.all(runs[:, 1] >= 1) and np.all(runs[1:, 0] > runs[:-1, 0] + runs[:-1, 1]), name   # maximal, ascending
        words = M.words_of(runs)
        assert bytes_of(words) == [int(i) for i in ids], name                       # exact set, no superset
        assert sorted(words) == sorted({int(i) // 16 for i in ids}), name           # every word touched, no other
        assert all(0 < m < (1 << 16) for m in words.values()), name


def test_block_model_on_a_mesh_and_under_a_group_permutation():
    x, conn = M.kuhn_slab(200, 2, 2)
    model = M.blocks(conn)
    assert len(model) == 5 and all(m.summary and m.chunked for m in model)
    for b, m in enumerate(model):
        assert np.array_equal(m.ids, np.unique(conn[b * M.BLOCK:(b + 1) * M.BLOCK]))
        assert bytes_of(m.words) == [int(i) for i in m.ids]
    new = M.permute_in_groups(x.shape[0], 24, np.random.default_rng(0))
    assert np.array_equal(np.sort(new), np.arange(x.shape[0]))                      # a permutation
    moved = M.blocks(new[conn])
    assert max(len(m.runs) for m in moved) > max(len(m.runs) for m in model)
    for m0, m1 in zip(model, moved):
        assert np.array_equal(np.sort(new[m0.ids]), m1.ids)


def test_uniform_count_of_the_model():
    x, conn = M.kuhn_slab(200, 2, 2)
    model = M.blocks(conn)
    assert M.uniform_blocks(model, -np.ones(x.shape[0])) == (5, 0)
    assert M.uniform_blocks(model, np.ones(x.shape[0])) == (0, 5)
    phi = -np.ones(x.shape[0])
    phi[model[2].ids[0]] = 1.0          # one vertex of block 2 (and of whoever shares it)
    n_in, n_out = M.uniform_blocks(model, phi)
    sharing = sum(1 for m in model if model[2].ids[0] in m.ids)
    assert (n_in, n_out) == (5 - sharing, 0) and sharing >= 1
    phi[:] = 0.0                        # zeros are neither side
    assert M.uniform_blocks(model, phi) == (0, 0)


@pytest.mark.parametrize("gen,shape,cells", [(M.kuhn_slab, (200, 2, 2), 4800), (M.strip_2d, (1024, 2), 4096)])
def test_generated_meshes_are_consistent(gen, shape, cells):
    x, conn = gen(*shape)
    assert conn.shape[0] == cells and conn.min() == 0 and conn.max() == x.shape[0] - 1
    assert np.unique(conn).size == x.shape[0]
    # no degenerate cell: positive volume / area up to orientation
    p = x[conn]
    e = p[:, 1:] - p[:, :1]
    vol = np.linalg.det(e)
    assert np.all(np.abs(vol) > 1e-12)
    assert abs(np.abs(vol).sum() / (6 if x.shape[1] == 3 else 2) - np.prod(np.ptp(x, axis=0))) < 1e-12


def test_swapped_odd_bytes_put_six_runs_into_one_word():
    x, conn = M.kuhn_slab(200, 2, 2)
    n = x.shape[0]
    far = ((n + 15) // 16) // 2
    new = M.swap_odd_bytes(n, 12, far)
    assert np.array_equal(new[new], np.arange(n)) and (new != np.arange(n)).sum() == 10 * len(range(0, far, 12))
    ids = np.setdiff1d(np.arange(16 * 12, 16 * 14), 16 * 12 + np.array([1, 3, 5, 7, 9]))   # a block that held words 12, 13
    runs = M.runs_of(ids)
    assert [tuple(r) for r in runs] == [(192, 1), (194, 1), (196, 1), (198, 1), (200, 1), (202, 22)]
    words = M.words_of(runs)
    assert words == {12: 0b1111110101010101, 13: 0xffff}
    b = M.Block.__new__(M.Block)
    b.runs = runs
    assert M.runs_in_word(b, 12) == 6 and M.runs_in_word(b, 13) == 1
