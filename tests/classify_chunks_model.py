"""numpy model of the mesh-static tables behind the culled classification: per block of 1024 consecutive cells the
distinct vertex ids as runs of consecutive ids, and the aligned 16 B words of a one-byte-per-vertex array that those runs
touch, each with the mask of its bytes that belong to a run.  Shared by tests/test_classify_chunks_reference.py (which
checks the model) and tests/test_gpu_classify_chunks.py (which asserts each case's properties from it and compares the
engine's uniform-block count with its)."""
import numpy as np

BLOCK = 1024      # cells per block
MAX_RUNS = 32     # runs a summary holds
MAX_IDS = 1024    # distinct vertex ids a summary is built from
MAX_WORDS = 64    # 16 B words a block's chunk table holds
WORD = 16


def block_ids(conn, b):
    """Distinct vertex ids of block b, ascending."""
    return np.unique(np.asarray(conn)[b * BLOCK:(b + 1) * BLOCK])


def runs_of(ids):
    """(start, length) of the maximal runs of consecutive ids in an ascending array of distinct ids."""
    ids = np.asarray(ids, dtype=np.int64)
    if ids.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    first = np.flatnonzero(np.r_[True, np.diff(ids) != 1])
    length = np.diff(np.r_[first, ids.size])
    return np.stack([ids[first], length], axis=1)


def words_of(runs):
    """{word index: 16-bit mask} of the aligned 16 B words the runs touch; bit i: byte i of the word lies in a run.
    Written run by run and byte range by byte range, not from the id list: the reference test compares the two."""
    out = {}
    for start, length in runs:
        start, end = int(start), int(start + length)          # [start, end)
        for w in range(start // WORD, (end - 1) // WORD + 1):
            lo, hi = max(start, w * WORD) - w * WORD, min(end, (w + 1) * WORD) - w * WORD
            out[w] = out.get(w, 0) | (((1 << hi) - 1) & ~((1 << lo) - 1))
    return out


class Block:
    def __init__(self, conn, b):
        self.ids = block_ids(conn, b)
        self.runs = runs_of(self.ids)
        self.summary = len(self.runs) <= MAX_RUNS and self.ids.size <= MAX_IDS
        self.words = words_of(self.runs)
        self.chunked = self.summary and len(self.words) <= MAX_WORDS   # decided from the chunk table, else from the runs


def blocks(conn):
    ncells = np.asarray(conn).shape[0]
    return [Block(conn, b) for b in range((ncells + BLOCK - 1) // BLOCK)]


def uniform_blocks(model, phi):
    """(all inside, all outside): blocks with a summary whose distinct vertices are all negative / all positive."""
    phi = np.asarray(phi)
    n_in = sum(1 for m in model if m.summary and np.all(phi[m.ids] < 0))
    n_out = sum(1 for m in model if m.summary and np.all(phi[m.ids] > 0))
    return n_in, n_out


def permute_in_groups(nnodes, group, rng):
    """new id of every vertex: the groups of `group` consecutive ids in random order (the last, short group stays last
    so that every group keeps its length and its place is a multiple of `group`)."""
    ngroups = nnodes // group
    order = rng.permutation(ngroups)                      # group g moves to place order[g]
    new = np.arange(nnodes, dtype=np.int64)
    g = new[:ngroups * group] // group
    new[:ngroups * group] = order[g] * group + new[:ngroups * group] % group
    return new


def runs_in_word(block, w):
    """Number of the block's runs that have a byte in 16 B word w."""
    return sum(1 for s, n in block.runs if s // WORD <= w <= (s + n - 1) // WORD)


def swap_odd_bytes(nnodes, every, far):
    """new id of every vertex (an involution): in every `every`-th 16 B word of the first `far` words the ids at bytes
    1, 3, 5, 7, 9 change places with the same bytes of the word `far` words on.  A block that held such a word whole
    now holds its bytes 0, 2, 4, 6, 8, 10..15: six runs in one word, four of them a single id, with one-id gaps that
    belong to vertices of a distant block."""
    new = np.arange(nnodes, dtype=np.int64)
    for w in range(0, far, every):
        for byte in (1, 3, 5, 7, 9):
            a, b = WORD * w + byte, WORD * (w + far) + byte
            if b < nnodes:
                new[a], new[b] = b, a
    return new


def strip_2d(nx, ny):
    """nx x ny squares of two triangles each, vertices and squares numbered y fastest: with ny = 2 a block of 1024
    triangles is 256 columns and refers to 257 x 3 = 771 consecutive vertex ids."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    h = 1.0 / nx
    x = np.stack([i.ravel() * h, j.ravel() * h], axis=1).astype(np.float64)
    ci, cj = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"))
    corner = np.stack([(cj + ((c >> 1) & 1)) + (ny + 1) * (ci + (c & 1)) for c in range(4)], axis=1)
    conn = corner[:, np.array([[0, 1, 3], [0, 3, 2]])].reshape(-1, 3)
    return x, np.ascontiguousarray(conn.astype(np.int32))


def kuhn_slab(nx, ny, nz):
    """nx x ny x nz cubes of six tetrahedra each (Kuhn split), vertices and cubes numbered x fastest."""
    tet = np.array([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    h = 1.0 / max(nx, ny, nz)
    x = np.stack([i.ravel() * h, j.ravel() * h, k.ravel() * h], axis=1).astype(np.float64)
    ck, cj, ci = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ci, cj, ck = ci.ravel(), cj.ravel(), ck.ravel()
    corner = np.stack([(ci + (c & 1)) + (nx + 1) * ((cj + ((c >> 1) & 1)) + (ny + 1) * (ck + ((c >> 2) & 1)))
                       for c in range(8)], axis=1)          # [ncubes, 8]
    conn = corner[:, tet].reshape(-1, 4)
    return x, np.ascontiguousarray(conn.astype(np.int32))
