"""The comparison helpers of tests/primitives_ref.py on the CPU: each passes the numpy answer and rejects a copy of it
with one defect of the kind a wrong kernel would leave -- which is what shows that tests/test_gpu_primitives.py can
fail.  (Kernels are not broken on purpose to show it: a wrong look-back spins.)"""
import numpy as np
import pytest

import primitives_ref as R
from primitives_ref import T


def _rejects(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def _scan_buffer(values, dtype):
    return np.concatenate([R.scan_reference(values, dtype), [R.poison_word(dtype)]]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_check_scan(dtype):
    values = np.random.default_rng(1).integers(0, 10, size=5 * T + 3).astype(np.int32)
    good = _scan_buffer(values, dtype)
    n = values.size
    assert good[n] == values.sum() and good[0] == 0 and good[1] == values[0]
    R.check_scan(good, values, dtype)
    one_off = good.copy()
    one_off[3 * T + 17] += 1
    _rejects(R.check_scan, one_off, values, dtype)
    # a tile whose prefix counts its predecessor twice (a stale or doubled look-back word)
    shifted = good.copy()
    shifted[2 * T:3 * T] += values[T:2 * T].sum()
    _rejects(R.check_scan, shifted, values, dtype)
    no_total = good.copy()
    no_total[n] = good[n - 1]
    _rejects(R.check_scan, no_total, values, dtype)
    overrun = good.copy()
    overrun[n + 1] = good[n]
    _rejects(R.check_scan, overrun, values, dtype)
    _rejects(R.check_scan, good[:-1], values, dtype)
    _rejects(R.check_scan, good.astype(np.int64 if dtype == np.int32 else np.int32), values, dtype)


def test_check_scan_past_32_bits_and_empty():
    values = np.full(600 * T + 1, 1 << 20, dtype=np.int32)
    good = _scan_buffer(values, np.int64)
    assert good[values.size] > 1 << 32
    R.check_scan(good, values, np.int64)
    wrapped = good.copy()
    wrapped[:-1] &= 0xFFFFFFFF  # what a 32-bit accumulator leaves
    _rejects(R.check_scan, wrapped, values, np.int64)
    empty = np.zeros(0, dtype=np.int32)
    R.check_scan(_scan_buffer(empty, np.int64), empty, np.int64)
    _rejects(R.check_scan, np.array([1, R.poison_word(np.int64)]), empty, np.int64)
    with pytest.raises(AssertionError):  # an input of the test's own that does not fit the output type
        R.scan_reference(np.full(3000, 1 << 20, dtype=np.int32), np.int32)


def test_check_list():
    flags = np.random.default_rng(2).random(3 * T + 5) < 0.3
    flags[-1] = True
    good = np.flatnonzero(flags).astype(np.int32)
    R.check_list(good, good.size, flags)
    _rejects(R.check_list, good[:-1], good.size - 1, flags)      # the last hit is missing
    _rejects(R.check_list, good, good.size + 1, flags)           # the count alone is wrong
    swapped = good.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    _rejects(R.check_list, swapped, good.size, flags)            # not ascending
    one_off = good.copy()
    one_off[100] += 1 if good[101] > good[100] + 1 else -1
    _rejects(R.check_list, one_off, good.size, flags)
    none = np.zeros(7, dtype=bool)
    R.check_list(np.zeros(0, dtype=np.int32), 0, none)
    _rejects(R.check_list, np.zeros(1, dtype=np.int32), 1, none)


def test_domain_mask_flags():
    codes = np.array([-1, 0, 1, 1, 0, -1], dtype=np.int8)
    assert np.array_equal(R.domain_mask_flags(codes, 1), codes == -1)
    assert np.array_equal(R.domain_mask_flags(codes, 2), codes == 0)
    assert np.array_equal(R.domain_mask_flags(codes, 4), codes == 1)
    assert np.array_equal(R.domain_mask_flags(codes, 5), codes != 0)
    assert R.domain_mask_flags(codes, 7).all()


def test_capacity_and_step_model():
    assert R.capacity(0, None) == 0 and R.capacity(0, 50) == 0
    assert R.capacity(1000, None) == 1031 + 256 and R.capacity(1000, 1200) == 1031 + 256
    assert R.capacity(1000, 900) == int(1100 * 1.03125) + 256        # the growth of the last step once more
    assert R.capacity(1000, 100) == int(1900 * 1.03125) + 256
    assert R.capacity(1000, 0) == 1031 + 256                         # no trend from an empty list
    n = 300 * T
    exact = [(int(0.30 * n),), (int(0.30 * n),), (int(0.31 * n),), (int(0.60 * n),)]
    # at exactly 30 % -> 31 % the third step misses its capacity by 128 entries
    assert R.capacity(exact[1][0], exact[0][0]) == exact[2][0] - 128
    assert R.step_model(exact)[2] == [(True, True), (False, False)]
    fits = [exact[0], exact[1], (exact[2][0] - 128,), exact[3]]
    assert R.step_model(fits) == [[(False, False)], [(True, False)], [(True, False)], [(True, True), (False, False)]]
    # a void step sizes nothing: the step behind its repeat is speculative again, its trend from the last valid records
    assert R.step_model([(100, 100), (100, 100), (0, 5000), (0, 5000), (100, 100)]) == \
        [[(False, False)], [(True, False)], [(True, True), (False, False)], [(True, False)], [(True, True), (False, False)]]


def test_check_adjacency():
    rng = np.random.default_rng(3)
    width, nitems = 4, 203
    item_map = rng.integers(0, nitems - 3, size=(517, width)).astype(np.int32)  # the last three items have no cells
    offsets, cells = R.adjacency_reference(item_map, width, nitems)
    assert offsets[-1] == item_map.size and offsets[-4] == offsets[-1]
    for item in (0, 100):
        assert np.array_equal(cells[offsets[item]:offsets[item + 1]], np.sort(np.nonzero(item_map == item)[0]))
    R.check_adjacency(offsets, cells, item_map, width, nitems)
    item = int(np.argmax(np.diff(offsets) >= 3))
    lo, hi = int(offsets[item]), int(offsets[item + 1])
    assert cells[lo] != cells[hi - 1]
    unsorted = cells.copy()
    unsorted[lo:hi] = unsorted[lo:hi][::-1]
    with pytest.raises(AssertionError, match="unsorted"):
        R.check_adjacency(offsets, unsorted, item_map, width, nitems)
    wrong = cells.copy()
    wrong[lo] = wrong[lo] + 1 if wrong[lo] + 1 not in cells[lo:hi] else wrong[lo] - 1
    with pytest.raises(AssertionError, match="wrong cells"):
        R.check_adjacency(offsets, wrong, item_map, width, nitems)
    late = offsets.copy()
    late[item + 1] += 1
    _rejects(R.check_adjacency, late, cells, item_map, width, nitems)
    _rejects(R.check_adjacency, offsets[:-1], cells, item_map, width, nitems)
    _rejects(R.check_adjacency, offsets, cells[:-1], item_map, width, nitems)


def test_check_fill():
    block = np.full(64 + 8 + 1000 + 64, R.POISON_BYTE, dtype=np.uint8)
    block[72:1072] = 0x7F
    R.check_fill(block, 72, 1000, 0x7F, R.POISON_BYTE)
    for i, where in ((71, "before"), (1072, "behind"), (1071, "inside"), (72, "inside")):
        bad = block.copy()
        bad[i] = 0x7F if where != "inside" else R.POISON_BYTE
        with pytest.raises(AssertionError, match=where):
            R.check_fill(bad, 72, 1000, 0x7F, R.POISON_BYTE)
    R.check_fill(np.full(128, R.POISON_BYTE, dtype=np.uint8), 64, 0, 0x00, R.POISON_BYTE)
