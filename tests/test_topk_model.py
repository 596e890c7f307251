"""tests/topk_model.py against brute force: the contract's answer, and the verdict drawn from the validator's two words, on
every column of up to 6 rows over 3 key values, every k, and every kind of wrong table.  The verdict must be true for the
right table only (include/dbhip_topk.h says why the two words are complete)."""
import itertools

import numpy as np

from tests import topk_model as tm

VALUES = (0x00000005, 0x80000000, 0xFFFFFFFE)  # either side of the sign bit: signed and unsigned order differ
MODES = [(False, False), (False, True), (True, False), (True, True)]  # (largest, signed)


def brute(keys, k, largest, signed):
    """the first min(k, n) rows by the contract's words: better key first, equal keys by ascending row"""
    def rank(row):
        v = keys[row]
        if signed and v >= 1 << 31:
            v -= 1 << 32
        return (-v if largest else v, row)
    rows = sorted(range(len(keys)), key=rank)[:min(k, len(keys))]
    return [keys[r] for r in rows], rows


def wrong_tables(keys, ok, orow):
    """(what, keys, rows) of every kind of damage to the right table (ok, orow)"""
    n, m = len(keys), len(orow)
    for i, j in {(i, i + 1) for i in range(m - 1)} | ({(0, m - 1)} if m > 1 else set()):
        k2, r2 = list(ok), list(orow)
        k2[i], k2[j], r2[i], r2[j] = k2[j], k2[i], r2[j], r2[i]
        yield "swapped", k2, r2
    for i in range(m):
        for other in range(n):  # the other rows of the same key, lower and higher
            if other != orow[i] and keys[other] == ok[i]:
                r2 = list(orow)
                r2[i] = other
                yield "tie replaced", ok, r2
        for j in range(m):
            if j != i:
                k2, r2 = list(ok), list(orow)
                k2[i], r2[i] = ok[j], orow[j]
                yield "duplicated", k2, r2
        for row in (n, 0xFFFFFFFF):
            r2 = list(orow)
            r2[i] = row
            yield "row id out of range", ok, r2
        for v in VALUES:
            if v != ok[i]:
                k2 = list(ok)
                k2[i] = v
                yield "wrong key", k2, orow
    if m:
        for outside in set(range(n)) - set(orow):
            k2, r2 = list(ok), list(orow)
            k2[-1], r2[-1] = keys[outside], outside
            yield "last entry from outside the answer", k2, r2


def test_the_model_answers_as_the_contract_words_it():
    for n in range(0, 6):
        for keys in itertools.product(VALUES, repeat=n):
            col = np.array(keys, dtype=np.uint32)
            for largest, signed in MODES:
                for k in range(0, n + 2):
                    ok, orow = brute(keys, k, largest, signed)
                    gk, gr = tm.topk(col, k, largest, signed)
                    assert gk.tolist() == ok and gr.tolist() == orow, (keys, k, largest, signed)
                    uk, ur = tm.topk(col, k, largest, signed, sorted=False)
                    assert ur.tolist() == sorted(orow) and uk.tolist() == [keys[r] for r in sorted(orow)]
    # k >= n, smallest first: the stable argsort; largest first is not its reverse where keys tie
    col = np.array([7, 3, 7, 3], dtype=np.uint32)
    assert tm.topk(col, 9)[1].tolist() == np.argsort(col, kind="stable").tolist() == [1, 3, 0, 2]
    assert tm.topk(col, 4, largest=True)[1].tolist() == [0, 2, 1, 3]


def test_the_verdict_is_true_for_the_right_table_only():
    seen = set()
    case = 0
    for n in range(0, 7):
        for keys in itertools.product(VALUES, repeat=n):
            case += 1
            col = np.array(keys, dtype=np.uint32)
            modes = MODES if n <= 4 else [MODES[case % 4]]  # the larger columns take the four orders in turn
            for largest, signed in modes:
                for k in range(0, n + 1):
                    ok, orow = brute(keys, k, largest, signed)

                    def judged(tk, tr):
                        words = tm.check_words(col, np.array(tk, dtype=np.uint32), np.array(tr, dtype=np.uint32), largest, signed)
                        return tm.verdict(words, k, n)

                    assert judged(ok, orow), (keys, k, largest, signed)
                    for what, tk, tr in wrong_tables(keys, ok, orow):
                        assert (list(tk), list(tr)) != (list(ok), list(orow))
                        assert not judged(tk, tr), (what, keys, k, largest, signed, tk, tr)
                        seen.add(what)
    assert seen == {"swapped", "tie replaced", "duplicated", "row id out of range", "wrong key",
                    "last entry from outside the answer"}
    # a table longer than the column is judged on its first n entries
    col = np.array([4, 2, 9], dtype=np.uint32)
    assert tm.check_words(col, np.array([2, 4, 9, 1, 1], np.uint32), np.array([1, 0, 2, 5, 5], np.uint32)) == (0, 2)
    assert tm.check_words(col, np.zeros(0, np.uint32), np.zeros(0, np.uint32)) == (0, 0)
