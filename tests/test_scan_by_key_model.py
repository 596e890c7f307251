"""tests/scan_by_key_model.py against a plain Python loop over include/dbhip_scan_by_key.h's definitions, on small random and
adversarial columns, and the validator model on every kind of wrong table."""
import numpy as np
import pytest

from tests import scan_by_key_model as sm

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF


def _signed(v):
    return v - (1 << 32) if v >> 31 else v


def loop_scan(keys, vals, signed):
    out = {name: [] for name in sm.NAMES}
    run = -1
    for i, (k, v) in enumerate(zip(map(int, keys), map(int, vals))):
        value = _signed(v) if signed else v
        if i == 0 or k != int(keys[i - 1]):
            run, number, total, lo, hi = run + 1, 0, 0, value, value
        number, total, lo, hi = number + 1, total + value, min(lo, value), max(hi, value)
        for name, word in zip(sm.NAMES, (run, number, total & M64, lo & M32, hi & M32)):
            out[name].append(word)
    return tuple(np.array(out[name], dtype=np.uint64 if name == "sums" else np.uint32) for name in sm.NAMES)


def loop_check(keys, vals, cols, signed):
    """the header's recurrence, row by row, mod 2^32 / 2^64, on whatever the columns hold"""
    run_ids, row_numbers, sums, mins, maxs = ([int(x) for x in c] if c is not None else None for c in cols)
    key = (lambda v: _signed(v)) if signed else (lambda v: v)
    faults, lowest, heads = 0, M64, 0
    for i in range(len(keys)):
        v = int(vals[i]) if vals is not None else 0
        e = (_signed(v) if signed else v) & M64
        head = i == 0 or int(keys[i]) != int(keys[i - 1])
        heads += head
        bad = 0
        if head:
            bad += run_ids is not None and run_ids[i] != ((run_ids[i - 1] + 1) & M32 if i else 0)
            bad += row_numbers is not None and row_numbers[i] != 1
            bad += sums is not None and sums[i] != e
            bad += mins is not None and mins[i] != v
            bad += maxs is not None and maxs[i] != v
        else:
            bad += run_ids is not None and run_ids[i] != run_ids[i - 1]
            bad += row_numbers is not None and row_numbers[i] != (row_numbers[i - 1] + 1) & M32
            bad += sums is not None and sums[i] != (sums[i - 1] + e) & M64
            bad += mins is not None and mins[i] != min(mins[i - 1], v, key=key)
            bad += maxs is not None and maxs[i] != max(maxs[i - 1], v, key=key)
        faults += bad
        if bad and lowest == M64:
            lowest = i
    return faults, lowest, heads, 0


def columns():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 64, 300):
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        yield "all distinct", np.arange(n, dtype=np.uint32) * np.uint32(2654435761), vals
        yield "one run", np.full(n, 7, dtype=np.uint32), vals
        yield "short runs", np.cumsum(rng.random(n) < 0.5).astype(np.uint32), vals
        yield "a key that returns", (np.cumsum(rng.random(n) < 0.3) % 2).astype(np.uint32), vals
    n = 200
    keys = np.cumsum(rng.random(n) < 0.05).astype(np.uint32)
    yield "all ones: the sum passes 2^32", keys, np.full(n, M32, dtype=np.uint32)
    yield "the ends of the signed range", keys, np.array([INT_MIN, INT_MAX, M32, 0, 1], dtype=np.uint32)[rng.integers(0, 5, n)]
    yield "sums that go negative and come back", keys, np.tile(np.array([5, M32 - 9, M32 - 2, 40], dtype=np.uint32), n // 4)


@pytest.mark.parametrize("signed", [False, True])
def test_the_model_is_the_loop(signed):
    for what, keys, vals in columns():
        got, want = sm.scan_by_key(keys, vals, signed), loop_scan(keys, vals, signed)
        for name, g, w in zip(sm.NAMES, got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, keys.size, name)
        words = sm.check_words(keys, vals, *got, signed=signed)
        assert words == loop_check(keys, vals, got, signed) and sm.verdict(words, keys), (what, words)
    empty = sm.scan_by_key(np.zeros(0, np.uint32), np.zeros(0, np.uint32), signed)
    assert all(c.size == 0 for c in empty) and empty[2].dtype == np.uint64
    assert sm.check_words(np.zeros(0, np.uint32), np.zeros(0, np.uint32), *empty, signed=signed) == (0, M64, 0, 0)


@pytest.mark.parametrize("signed", [False, True])
def test_the_validator_model_on_every_kind_of_wrong_table(signed):
    rng = np.random.default_rng(9)
    n = 120
    keys = np.cumsum(rng.random(n) < 0.2).astype(np.uint32)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    right = sm.scan_by_key(keys, vals, signed)
    heads = np.flatnonzero(sm.head_flags(keys))
    inside = np.flatnonzero(~sm.head_flags(keys))
    seen = set()
    for col in range(5):
        for row in (0, int(heads[2]), int(inside[3]), int(inside[-1]), n - 1):
            for delta in (1, 1 << 31, M32):
                table = [c.copy() for c in right]
                table[col][row] ^= table[col].dtype.type(delta)
                words = sm.check_words(keys, vals, *table, signed=signed)
                assert words == loop_check(keys, vals, table, signed), (col, row, delta)
                assert words[0] >= 1 and words[1] == row and not sm.verdict(words, keys), (col, row, words)
                seen.add(words[0])
                alone = [t if j == col else None for j, t in enumerate(table)]  # the other columns skipped
                assert sm.check_words(keys, vals, *alone, signed=signed) == loop_check(keys, vals, alone, signed)
                others = [None if j == col else t for j, t in enumerate(table)]
                assert sm.check_words(keys, vals, *others, signed=signed)[:2] == (0, M64)
    assert seen == {1, 2}  # a poked word breaks its own rule and, unless the next row is a head, the next row's
    # garbage, a shifted table, a table of another input, another signedness
    junk = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(5)]
    junk[2] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    other = sm.scan_by_key(np.roll(keys, 1), vals, signed)
    flipped = sm.scan_by_key(keys, vals | np.uint32(0x80000000), not signed)
    for table in (junk, [np.roll(c, 1) for c in right], other, flipped):
        words = sm.check_words(keys, vals, *table, signed=signed)
        assert words == loop_check(keys, vals, table, signed) and words[0] > 0 and not sm.verdict(words, keys)
    # run_ids and row_numbers without values
    words = sm.check_words(keys, None, right[0], right[1])
    assert words == loop_check(keys, None, (right[0], right[1], None, None, None), False) and sm.verdict(words, keys)
