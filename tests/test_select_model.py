"""The numpy model of the selection vectors (tests/select_model.py) against plain numpy formulations, on random and
adversarial inputs.  No device."""
import numpy as np
import pytest

from tests import select_model as sm

EDGES = np.array([0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def _columns():
    rng = np.random.default_rng(7)
    yield "edges", np.tile(EDGES, 5)
    yield "random", rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    yield "narrow", rng.integers(100, 120, 3000, dtype=np.uint64).astype(np.uint32)
    yield "empty", np.zeros(0, dtype=np.uint32)
    yield "one", np.array([0x80000000], dtype=np.uint32)


BOUNDS = [(0, 0xFFFFFFFF), (5, 5), (0x80000000, 0x80000000), (110, 115), (0x7FFFFFFF, 0x80000001), (0xFFFFFFFF, 0),
          (116, 109), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (1, 0xFFFFFFFF)]


@pytest.mark.parametrize("name,col", list(_columns()), ids=[n for n, _ in _columns()])
def test_dense_unsigned_and_signed(name, col):
    for lo, hi in BOUNDS:
        c = col.astype(np.int64)
        want = np.flatnonzero((c >= lo) & (c <= hi))
        got, st = sm.select_range(col, lo, hi)
        assert st == 0 and got.dtype == np.uint32 and np.array_equal(got, want)
        got, st = sm.select_range(col, lo, hi, sm.NEGATE)
        assert st == 0 and np.array_equal(got, np.flatnonzero(~((c >= lo) & (c <= hi))))
        s = col.view(np.int32).astype(np.int64)
        slo, shi = np.int64(np.uint32(lo).view(np.int32)), np.int64(np.uint32(hi).view(np.int32))
        got, st = sm.select_range(col, lo, hi, sm.SIGNED)
        assert st == 0 and np.array_equal(got, np.flatnonzero((s >= slo) & (s <= shi)))
        got, st = sm.select_range(col, lo, hi, sm.SIGNED | sm.NEGATE)
        assert st == 0 and np.array_equal(got, np.flatnonzero((s < slo) | (s > shi)))


def test_signed_bounds_as_python_ints():
    col = np.array([-5, -1, 0, 1, 5], dtype=np.int32).view(np.uint32)
    got, _ = sm.select_range(col, sm.pattern(-1), sm.pattern(1), sm.SIGNED)
    assert got.tolist() == [1, 2, 3]
    got, _ = sm.select_range(col, sm.pattern(-1), sm.pattern(1))  # unsigned: 0xFFFFFFFF > 1, the empty interval
    assert got.tolist() == []
    got, _ = sm.select_range(col, sm.pattern(-1), sm.pattern(1), sm.NEGATE)
    assert got.tolist() == [0, 1, 2, 3, 4]


def test_lists_keep_order_and_duplicates():
    rng = np.random.default_rng(11)
    col = rng.integers(0, 1000, 4000, dtype=np.uint64).astype(np.uint32)
    sorted_rows = np.sort(rng.choice(4000, 900, replace=False)).astype(np.uint32)
    shuffled = rng.permutation(4000).astype(np.uint32)
    repeated = rng.integers(0, 50, 2000, dtype=np.uint64).astype(np.uint32)
    for rows in (sorted_rows, shuffled, repeated, np.zeros(0, dtype=np.uint32)):
        for flags in (0, sm.NEGATE):
            keep = (col[rows] >= 200) & (col[rows] <= 700)
            got, st = sm.select_range(col, 200, 700, flags, in_rows=rows)
            assert st == 0 and np.array_equal(got, rows[keep != bool(flags)])


def test_count_is_clamped_to_the_capacity():
    col = np.arange(100, dtype=np.uint32)
    rows = np.arange(99, -1, -1, dtype=np.uint32)
    for count, m in ((0, 0), (1, 1), (40, 40), (100, 100), (101, 100), (1 << 40, 100), (None, 100)):
        got, st = sm.select_range(col, 10, 95, in_rows=rows, in_count=count)
        head = rows[:m]
        assert st == 0 and np.array_equal(got, head[(head >= 10) & (head <= 95)])


def test_row_ids_outside_the_column():
    col = np.arange(10, dtype=np.uint32)
    rows = np.array([3, 10, 0xFFFFFFFF, 4, 0x80000000, 9, 11], dtype=np.uint32)
    for flags in (0, sm.SIGNED):
        got, st = sm.select_range(col, 0, 0x7FFFFFFF, flags, in_rows=rows)
        assert got.tolist() == [3, 4, 9] and st == sm.KEY_RANGE
        got, st = sm.select_range(col, 4, 4, flags | sm.NEGATE, in_rows=rows)
        assert got.tolist() == [3, 9] and st == sm.KEY_RANGE  # never kept, not even under negate
    got, st = sm.select_range(col, 0, 5, in_rows=rows, in_count=1)
    assert got.tolist() == [3] and st == 0  # behind the count nothing is looked at
    got, st = sm.select_range(np.zeros(0, dtype=np.uint32), 0, 0xFFFFFFFF, sm.NEGATE, in_rows=rows[:1])
    assert got.size == 0 and st == sm.KEY_RANGE


def test_chain_is_the_conjunction():
    rng = np.random.default_rng(3)
    a, b, c = (rng.integers(0, 100, 5000, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    got = sm.chain([a, b, c], [(10, 80), (0, 50), (30, 99)])
    assert np.array_equal(got, np.flatnonzero((a >= 10) & (a <= 80) & (b <= 50) & (c >= 30)))
