"""tests/reduce_by_key_model.py against brute force: the contract's answer, and the verdict drawn from the validator's four
words, on every column of up to 6 rows over a small alphabet of keys and values and on every kind of wrong table.  The
verdict must be true for the right table only."""
import itertools

import numpy as np

from tests import reduce_by_key_model as rm

KEYS = (7, 0xFFFFFFFF)
VALUES = (0x00000005, 0x80000000, 0xFFFFFFFE)  # either side of the sign bit: signed and unsigned order differ
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


def brute(keys, vals, signed):
    """one row per run, by the contract's words -> five lists (sums mod 2^64, mins and maxs as 32-bit patterns)"""
    runs = []
    for i, (k, v) in enumerate(zip(keys, vals)):
        sv = v - (1 << 32) if signed and v >> 31 else v
        if i == 0 or k != keys[i - 1]:
            runs.append([k, 0, 0, sv, sv])
        r = runs[-1]
        r[1] += 1
        r[2] += sv
        r[3], r[4] = min(r[3], sv), max(r[4], sv)
    return ([r[0] for r in runs], [r[1] for r in runs], [r[2] & M64 for r in runs], [r[3] & M32 for r in runs],
            [r[4] & M32 for r in runs])


def wrong_tables(keys, vals, signed, table):
    """(what, table) of every kind of damage to the right table"""
    n, runs = len(keys), len(table[0])

    def copy():
        return [list(c) for c in table]

    for i in range(runs - 1):
        for a, b in ((i, i + 1), (i + 1, i)):
            t = copy()
            t[1][a] -= 1
            t[1][b] += 1
            yield "count moved", t
        starts = np.cumsum([0] + table[1])
        merged = brute([keys[starts[i]]] * int(starts[i + 2] - starts[i]), vals[starts[i]:starts[i + 2]], signed)
        t = copy()
        for c, m in zip(t, merged):
            c[i:i + 2] = m
        yield "merged", t
    at = 0
    for i in range(runs):
        for other in set(KEYS + (11,)) - {table[0][i]}:
            t = copy()
            t[0][i] = other
            yield "key changed", t
        for col, step, what in ((3, -1, "min lowered"), (4, 1, "max raised"), (2, 1, "sum + 1"), (2, -1, "sum - 1")):
            t = copy()
            t[col][i] = (t[col][i] + step) & (M64 if col == 2 else M32)
            yield what, t
        for cut in range(1, table[1][i]):
            a = brute(keys[at:at + cut], vals[at:at + cut], signed)
            b = brute(keys[at + cut:at + table[1][i]], vals[at + cut:at + table[1][i]], signed)
            t = copy()
            for c, x, y in zip(t, a, b):
                c[i:i + 1] = x + y
            yield "split", t
        at += table[1][i]
    if runs:
        t = copy()
        t[1][-1] += 1
        yield "count total", t
        yield "count total", [c[:-1] for c in table]
    yield "count total", [c + [x] for c, x in zip(table, (11, 1, 0, 0, 0))]


def columns(t):
    return (np.array(t[0], dtype=np.uint32), np.array(t[1], dtype=np.uint32), np.array(t[2], dtype=np.uint64),
            np.array(t[3], dtype=np.uint32), np.array(t[4], dtype=np.uint32))


def test_the_model_answers_as_the_contract_words_it():
    case = 0
    for n in range(0, 7):
        values = VALUES if n <= 4 else VALUES[1:]  # the longer columns: two values, the two orders in turn
        for keys in itertools.product(KEYS, repeat=n):
            for vals in itertools.product(values, repeat=n):
                case += 1
                for signed in ((False, True) if n <= 4 else (bool(case % 2),)):
                    want = brute(keys, vals, signed)
                    got = rm.reduce_by_key(np.array(keys, dtype=np.uint32), np.array(vals, dtype=np.uint32), signed)
                    assert [g.tolist() for g in got] == [list(w) for w in want], (keys, vals, signed)


def test_the_verdict_is_true_for_the_right_table_only():
    seen = set()
    case = 0
    for n in range(0, 7):
        values = VALUES if n <= 4 else VALUES[1:]  # the longer columns: two values, the two orders in turn
        for keys in itertools.product(KEYS, repeat=n):
            for vals in itertools.product(values, repeat=n):
                case += 1
                kcol, vcol = np.array(keys, dtype=np.uint32), np.array(vals, dtype=np.uint32)
                for signed in ((False, True) if n <= 4 else (bool(case % 2),)):
                    right = brute(keys, vals, signed)
                    assert rm.verdict(rm.check_words(kcol, vcol, *columns(right), signed)), (keys, vals, signed)
                    if n > 4 and case % 8:  # the longer columns: every eighth is damaged in every way
                        continue
                    for what, t in wrong_tables(keys, vals, signed, right):
                        assert [list(c) for c in t] != [list(c) for c in right]
                        words = rm.check_words(kcol, vcol, *columns(t), signed)
                        assert not rm.verdict(words), (what, keys, vals, signed, t, words)
                        seen.add(what)
    assert seen == {"count moved", "merged", "key changed", "min lowered", "max raised", "sum + 1", "sum - 1", "split",
                    "count total"}


def test_a_table_whose_counts_wrap_is_read_inside_its_arrays():
    keys, vals = np.array([1, 1, 2], dtype=np.uint32), np.array([5, 6, 7], dtype=np.uint32)
    t = ([1, 2, 2], [2, 0xFFFFFFFF, 2], [11, 7, 0], [5, 7, 0], [6, 7, 0])
    words = rm.check_words(keys, vals, *columns(t))
    assert words[0] >= 1 and not rm.verdict(words)
    assert rm.check_words(np.zeros(0, np.uint32), np.zeros(0, np.uint32), *columns(([], [], [], [], []))) == (0, 0, 0, 0)
