"""Exact references and comparison helpers for the engine's index primitives (scans, compactions, incidence
inversion, fills): what tests/test_gpu_primitives.py holds the probe's raw output against.  Every answer is an integer
array with one right value: numpy.cumsum in int64, numpy.flatnonzero, a stable argsort.  A helper returns None when the
output is right and raises AssertionError naming the first wrong element otherwise; tests/test_primitives_reference.py
feeds each of them a right answer and copies with one defect."""
import numpy as np

T = 2048                     # kTile of cfx_device.h: 256 threads x 8 items
BYTE_TILE = 4096             # kByteTile: 256 threads x 16 bytes
POISON_BYTE = 0xA5           # what the probe fills its output buffers with before a case runs


def poison_word(dtype):
    return np.frombuffer(bytes([POISON_BYTE]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


def _first_difference(got, want, what):
    if got.shape != want.shape:
        raise AssertionError(f"{what}: {got.shape[0]} elements, expected {want.shape[0]}")
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} wrong elements, the first at [{i}] (tile {i // T}): "
                             f"got {got[i]}, expected {want[i]}")


# ---- scans -------------------------------------------------------------------------------------------------------------
def scan_reference(values, out_dtype):
    """out[0..n] of an exclusive scan with the total in out[n], summed in int64 and cast last."""
    out = np.zeros(values.size + 1, dtype=np.int64)
    np.cumsum(values.astype(np.int64), out=out[1:])
    assert out[-1] <= np.iinfo(out_dtype).max, "the test's own input overflows the output type"
    return out.astype(out_dtype)


def check_scan(got, values, out_dtype, what="scan"):
    """`got`: the n + 2 words of the probe's buffer -- the scan, the total, one poisoned word that must survive."""
    n = values.size
    if got.shape != (n + 2,) or got.dtype != np.dtype(out_dtype):
        raise AssertionError(f"{what}: output of {got.shape} {got.dtype}, expected {n + 2} x {np.dtype(out_dtype)}")
    _first_difference(got[:n + 1], scan_reference(values, out_dtype), what)
    if got[n + 1] != poison_word(out_dtype):
        raise AssertionError(f"{what}: the word behind out[n] was overwritten with {got[n + 1]}")


# ---- compactions -------------------------------------------------------------------------------------------------------
def check_list(got, count, flags, what="list"):
    """`got`: the list as written (its first `count` entries), `flags`: the predicate per index."""
    want = np.flatnonzero(flags).astype(np.int32)
    if count != want.size:
        raise AssertionError(f"{what}: count {count}, expected {want.size}")
    _first_difference(got, want, what)


def domain_mask_flags(codes, mask):
    """DomainMask of cfx_device.h: bit 0 selects code -1, bit 1 code 0, bit 2 code 1."""
    return ((mask >> (codes.astype(np.int64) + 1)) & 1).astype(bool)


# ---- capacities of a speculative step ----------------------------------------------------------------------------------
MARGIN, SLACK = 1.03125, 256  # g_margin, g_slack of cfx_runtime.hip (cutfemx_amd.step.set_margin's defaults)


def capacity(prev, before):
    """CountPlan's capacity of a kCountUpTo site (cfx_runtime.hip): the previous count, moved on by its growth over the
    valid step before it (at most doubled), x margin + slack; a list that was empty must stay empty."""
    if prev == 0:
        return 0
    expect = prev
    if before is not None and before > 0 and prev > before:
        expect = prev + min(prev - before, prev)
    return int(expect * MARGIN) + SLACK


def step_model(counts_per_step):
    """What a loop of steps does with these counts (one tuple of site counts per step): per step the list of passes,
    each (speculative, redo).  The first step of a loop and the repeat of a void one size everything by read-back."""
    values = before = None  # the history of the loop (cfx_step_end): the last record, the valid record before it
    valid = False
    out = []
    for counts in counts_per_step:
        passes = []
        while True:
            speculative = valid
            redo = speculative and any(c > capacity(values[k], None if before is None else before[k])
                                       for k, c in enumerate(counts))
            passes.append((speculative, redo))
            if valid:
                before = values
            values, valid = tuple(counts), not redo  # (a void step's record is kept but sizes nothing)
            if not redo:
                break
        out.append(passes)
    return out


# ---- incidence inversion -----------------------------------------------------------------------------------------------
def adjacency_reference(item_map, width, nitems):
    flat = item_map.ravel()
    offsets = np.zeros(nitems + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=nitems), out=offsets[1:])
    cells = (np.argsort(flat, kind="stable") // width).astype(np.int32)
    return offsets, cells


def check_adjacency(offsets, cells, item_map, width, nitems, what="adjacency"):
    want_offsets, want_cells = adjacency_reference(item_map, width, nitems)
    _first_difference(offsets, want_offsets, what + " offsets")
    if cells.shape != want_cells.shape:
        raise AssertionError(f"{what} cells: {cells.shape[0]} entries, expected {want_cells.shape[0]}")
    bad = np.flatnonzero(cells != want_cells)
    if bad.size:
        i = int(bad[0])
        item = int(np.searchsorted(want_offsets, i, side="right") - 1)
        lo, hi = int(want_offsets[item]), int(want_offsets[item + 1])
        kind = "unsorted" if np.array_equal(np.sort(cells[lo:hi]), want_cells[lo:hi]) else "wrong cells"
        raise AssertionError(f"{what} cells: {bad.size} wrong entries, the first at [{i}] in the list of item {item} "
                             f"({kind}): got {cells[i]}, expected {want_cells[i]}")


# ---- fills -------------------------------------------------------------------------------------------------------------
def check_fill(block, start, size, byte, untouched, what="fill"):
    """`block`: a whole allocation that held `untouched` everywhere before block[start : start + size] was filled."""
    want = np.full(block.shape, untouched, dtype=np.uint8)
    want[start:start + size] = byte
    bad = np.flatnonzero(block != want)
    if bad.size:
        i = int(bad[0])
        where = "before the range" if i < start else ("behind the range" if i >= start + size else "inside the range")
        raise AssertionError(f"{what}: {bad.size} wrong bytes, the first at [{i}] ({where}, range [{start}, {start + size})): "
                             f"got {block[i]:#x}, expected {want[i]:#x}")
