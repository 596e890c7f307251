"""tests/take_model.py against plain Python loops on hand-written cases: the model is what the GPU tests compare the
kernels of dwarf_bench_amd/host/take_rows.cpp with, so it is checked here against the header's sentences one by one."""
import numpy as np
import pytest

from dwarf_bench_amd import take_native as tn
from tests import take_model as tm

U = np.uint32
COL_A = np.array([10, 11, 12, 13, 14, 0xFFFFFFFF, 0x80000000, 7], U)
COL_B = np.array([100, 101, 102, 103, 104, 105, 106, 107], U)
LISTS = {
    "ascending": [0, 2, 3, 7],
    "shuffled with repeats": [7, 0, 0, 5, 6, 5, 1],
    "one row throughout": [4, 4, 4, 4, 4],
    "the last row": [7],
    "past the end": [0, 8, 1],
    "far past the end": [9, 0x80000000, 3],
    "the no-row id": [1, 0xFFFFFFFF, 2, 0xFFFFFFFF],
    "no-row and past the end": [0xFFFFFFFF, 8],
    "empty": [],
}
COUNTS = (None, 0, 1, 2, 3, 4, 7, 8, 100, (1 << 32) + 1, (1 << 64) - 1)


def loop_take(cols, rows, count, flags, fill, before):
    capacity = len(rows)
    m = capacity if count is None else min(count, capacity)
    outs, status = [list(b) for b in before], 0
    for i in range(m):
        r = rows[i]
        for c, col in enumerate(cols):
            outs[c][i] = int(col[r]) if r < len(col) else fill
        if r >= len(col) and not (flags & tm.OUTER and r == 0xFFFFFFFF):
            status |= 2
    return outs, status


def loop_aggregate(col, rows, count, flags):
    signed = bool(flags & tm.SIGNED)
    if rows is None:
        cand, m = list(range(len(col))), len(col)
    else:
        m = len(rows) if count is None else min(count, len(rows))
        cand = rows[:m]
    n, total, status = 0, 0, 0
    least, most = ((1 << 31) - 1, -(1 << 31)) if signed else (0xFFFFFFFF, 0)
    for r in cand:
        if r >= len(col):
            if not (flags & tm.OUTER and r == 0xFFFFFFFF):
                status |= 2
            continue
        v = int(col[r])
        if signed and v >> 31:
            v -= 1 << 32
        n, total = n + 1, total + v
        least, most = min(least, v), max(most, v)
    return (n, total % (1 << 64), least % (1 << 64), most % (1 << 64)), status


def test_constants_are_the_bindings():
    assert (tm.OUTER, tm.SIGNED, tm.NO_ROW) == (tn.OUTER, tn.SIGNED, tn.NO_ROW)
    from dwarf_bench_amd import ops
    assert tm.KEY_RANGE == ops.DEV_KEY_RANGE


def test_length_clamps_any_64_bit_count():
    assert tm.length(None, 5) == 5 and tm.length(0, 5) == 0 and tm.length(5, 5) == 5 and tm.length(6, 5) == 5
    assert tm.length((1 << 32) + 1, 5) == 5 and tm.length((1 << 64) - 1, 5) == 5 and tm.length(3, 0) == 0
    assert tm.length(-1, 5) == 5  # an int64 view of a count above 2^63


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("flags", (0, tm.OUTER))
def test_take_against_the_loop(name, flags):
    rows = LISTS[name]
    for count in COUNTS:
        for cols in ([COL_A], [COL_A, COL_B]):
            before = [np.full(len(rows), 0xDEAD0000 + c, U) for c in range(len(cols))]
            got, status = tm.take(cols, np.array(rows, U), count, flags, fill=0xABCD, before=before)
            want, want_status = loop_take(cols, rows, count, flags, 0xABCD, before)
            assert status == want_status, (name, count)
            assert [g.tolist() for g in got] == want, (name, count)


def test_take_hand_written():
    outs, status = tm.take([COL_A, COL_B], np.array([7, 8, 0xFFFFFFFF, 0], U), count=3, flags=tm.OUTER, fill=5,
                           before=[np.full(4, 1, U), np.full(4, 2, U)])
    assert [o.tolist() for o in outs] == [[7, 5, 5, 1], [107, 5, 5, 2]] and status == 2  # row 8 raises, the tail stays
    outs, status = tm.take([COL_A], np.array([0xFFFFFFFF, 1], U), flags=tm.OUTER, fill=9)
    assert outs[0].tolist() == [9, 11] and status == 0
    outs, status = tm.take([COL_A], np.array([0xFFFFFFFF, 1], U), fill=9)
    assert outs[0].tolist() == [9, 11] and status == 2  # without OUTER the same id is an error
    outs, status = tm.take([np.zeros(0, U)], np.array([0, 0xFFFFFFFF], U), flags=tm.OUTER, fill=3)
    assert outs[0].tolist() == [3, 3] and status == 2  # n_rows == 0: every entry is filled, row 0 does not exist
    outs, status = tm.take([np.zeros(0, U)], np.array([0xFFFFFFFF], U), flags=tm.OUTER, fill=3)
    assert outs[0].tolist() == [3] and status == 0


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("flags", (0, tm.OUTER, tm.SIGNED, tm.OUTER | tm.SIGNED))
def test_aggregate_against_the_loop(name, flags):
    rows = LISTS[name]
    for count in COUNTS:
        assert tm.aggregate(COL_A, np.array(rows, U), count, flags) == loop_aggregate(COL_A, rows, count, flags), (name, count)
    assert tm.aggregate(COL_A, None, None, flags) == loop_aggregate(COL_A, None, None, flags)


def test_aggregate_hand_written():
    M = 1 << 64
    assert tm.aggregate(COL_A) == ((8, 10 + 11 + 12 + 13 + 14 + 0xFFFFFFFF + 0x80000000 + 7, 7, 0xFFFFFFFF), 0)
    assert tm.aggregate(COL_A, flags=tm.SIGNED) == ((8, (67 - 1 - (1 << 31)) % M, (-(1 << 31)) % M, 14), 0)
    # the empty aggregate, by an empty list, a zero count, and candidates that are all skipped
    for kw in (dict(rows=np.zeros(0, U)), dict(rows=np.array([1, 2], U), count=0), dict(rows=np.array([8, 9], U))):
        words, status = tm.aggregate(COL_A, **kw)
        assert words == (0, 0, 0xFFFFFFFF, 0) and status == (2 if "count" not in kw and kw["rows"].size else 0)
        words, _ = tm.aggregate(COL_A, flags=tm.SIGNED, **kw)
        assert words == (0, 0, (1 << 31) - 1, (-(1 << 31)) % M)
        assert tm.as_ints(words, True) == (0, 0, None, None)
    assert tm.aggregate(COL_A, np.array([0xFFFFFFFF] * 3, U), flags=tm.OUTER) == ((0, 0, 0xFFFFFFFF, 0), 0)
    # the 64-bit sum: a few thousand 0xFFFFFFFF exceed 2^32; as int32 they are -1 each
    big = np.full(5000, 0xFFFFFFFF, U)
    assert tm.aggregate(big)[0] == (5000, 5000 * 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert tm.as_ints(tm.aggregate(big, flags=tm.SIGNED)[0], True) == (5000, -5000, -1, -1)
    assert tm.as_ints(tm.aggregate(big)[0], False) == (5000, 5000 * 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    # a repeated row counts each time
    assert tm.aggregate(COL_B, np.array([3, 3, 3], U))[0] == (3, 309, 103, 103)
