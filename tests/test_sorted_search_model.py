"""tests/sorted_search_model.py against plain Python loops, its validator against every kind of wrong answer, and the fence
ladder's geometry at its boundaries (include/dbhip_sorted_search.h).  No GPU."""
import numpy as np
import pytest

from tests import sorted_search_model as sm

BOUNDARIES = (0, 1, 63, 64, 65, 16384, 16385, 1 << 20, (1 << 20) + 1, 1 << 26, (1 << 26) + 1, 1 << 31)


def _order(v, signed):
    v = int(v)
    return v - (1 << 32) if signed and v >> 31 else v


def _loop_search(s, lo, hi, signed):
    s = [_order(v, signed) for v in s]
    n = len(lo if lo is not None else hi)
    pos, cnt = [], []
    for i in range(n):
        h = _order((hi if hi is not None else lo)[i], signed)
        p = sum(1 for v in s if v < _order(lo[i], signed)) if lo is not None else 0
        e = sum(1 for v in s if v <= h)
        pos.append(p)
        cnt.append(e - p if e > p else 0)
    return np.array(pos, dtype=np.uint32), np.array(cnt, dtype=np.uint32)


def _columns(seed, m, n, signed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    s[rng.integers(0, m, m // 2)] = s[0]  # duplicates
    s[:4] = (0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000)
    s = s[np.argsort(sm.flip(s, signed), kind="stable")]
    lo = rng.choice(np.concatenate([s, s + np.uint32(1), s - np.uint32(1)]), n)
    hi = lo + rng.integers(0, 1 << 30, n).astype(np.uint32) * rng.integers(0, 2, n).astype(np.uint32)
    hi[:8] = lo[:8] - np.uint32(5)  # mostly empty intervals
    return s, lo, hi


@pytest.mark.parametrize("signed", (False, True))
def test_search_model_matches_a_plain_loop(signed):
    s, lo, hi = _columns(1, 300, 200, signed)
    for a, b in ((lo, hi), (lo, None), (None, hi)):
        got, want = sm.search(s, a, b, signed), _loop_search(s, a, b, signed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    empty = np.zeros(0, dtype=np.uint32)
    pos, cnt = sm.search(empty, lo, hi, signed)
    assert not pos.any() and not cnt.any()


@pytest.mark.parametrize("signed", (False, True))
def test_validator_model_sees_every_kind_of_wrong_answer(signed):
    s, lo, hi = _columns(2, 400, 300, signed)
    m = s.size
    pos, cnt = sm.search(s, lo, hi, signed)
    total = int(cnt.sum())
    assert sm.check(s, lo, hi, pos, cnt, signed) == (0, sm.NONE, total, 0)
    assert sm.check(s, lo, None, *sm.search(s, lo, None, signed), signed)[:2] == (0, sm.NONE)
    assert sm.check(s, None, hi, *sm.search(s, None, hi, signed), signed)[:2] == (0, sm.NONE)
    assert sm.check(s, lo, None, pos, None, signed) == (0, sm.NONE, 0, 0)
    hit = int(np.nonzero((cnt > 1) & (pos > 0) & (pos + cnt < m))[0][0])
    empty = int(np.nonzero(sm.flip(hi, signed) < sm.flip(lo, signed))[0][0])

    def poked(row, dpos, dcnt):
        p, c = pos.copy(), cnt.copy()
        p[row:row + 1] += np.uint32(dpos & 0xFFFFFFFF)  # (an array add wraps silently)
        c[row:row + 1] += np.uint32(dcnt & 0xFFFFFFFF)
        return sm.check(s, lo, hi, p, c, signed)

    # pos one too far or one short, the end kept: the pos column alone
    assert poked(hit, 1, -1)[:2] == (1, hit) and poked(hit, -1, 1)[:2] == (1, hit)
    # cnt too long or too short
    assert poked(hit, 0, 1) == (1, hit, total + 1, 0) and poked(hit, 0, -1) == (1, hit, total - 1, 0)
    # pos + cnt behind the column, pos inside it; pos behind the column: both columns
    assert poked(hit, 0, m)[:2] == (1, hit) and poked(hit, m + 1, 0)[:2] == (2, hit)
    # a count on an empty interval
    assert poked(empty, 0, 1)[:2] == (1, empty)
    # the lowest row of several
    assert poked(hit, 1, 0)[0] >= 1 and sm.check(s, lo, hi, pos + np.uint32(1), cnt, signed)[1] == 0
    # lo == NULL wants pos == 0
    p0, c0 = sm.search(s, None, hi, signed)
    p0[7] = 1
    bad, row = sm.check(s, None, hi, p0, c0, signed)[:2]
    assert bad in (1, 2) and row == 7  # the pos column, and the cnt column unless the shifted end happens to fit


def test_validator_model_on_an_empty_column():
    lo = np.arange(10, dtype=np.uint32)
    zero = np.zeros(10, dtype=np.uint32)
    assert sm.check(zero[:0], lo, None, zero, zero) == (0, sm.NONE, 0, 0)
    assert sm.check(zero[:0], lo, None, zero + np.uint32(1), zero) == (20, 0, 0, 0)


@pytest.mark.parametrize("top", (0, 64))
def test_geometry_at_the_boundaries(top):
    t = top or sm.TOP
    for m in BOUNDARIES:
        counts, offsets, total = sm.geometry(m, top)
        assert counts[0] == m and counts[-1] <= t and all(c > t for c in counts[:-1])
        for below, above in zip(counts, counts[1:]):
            assert above == -(-below // 64)
        assert all(o % 256 == 0 for o in offsets) and total % 256 == 0
        for l in range(1, len(counts)):
            end = offsets[l + 1] if l + 1 < len(counts) else total
            assert offsets[l] + 4 * counts[l] <= end and offsets[l] >= 256
        assert total <= 1536 + m // 15 and total == sm.workspace_bytes(m, top)
    levels = {m: len(sm.geometry(m, top)[0]) - 1 for m in BOUNDARIES}
    if top == 0:
        assert [levels[m] for m in BOUNDARIES] == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    else:
        assert [levels[m] for m in BOUNDARIES] == [0, 0, 0, 0, 1, 2, 2, 3, 3, 4, 4, 5]
    assert sm.workspace_bytes((1 << 31) + 1, top) == 0
    for bad in (1, 63, 65, 96, 32768, 1 << 20):
        assert sm.workspace_bytes(1000, bad) == 0


def test_the_workspace_bound_holds_for_every_top():
    rng = np.random.default_rng(3)
    sizes = list(BOUNDARIES) + [int(v) for v in rng.integers(0, 1 << 31, 2000)] + [64 ** k + d for k in range(1, 6)
                                                                                   for d in (-1, 0, 1)]
    for top in sm.TOPS:
        for m in sizes:
            assert sm.workspace_bytes(m, top) <= 1536 + m // 15, (m, top)


def test_levels_hold_the_maximum_of_every_block():
    rng = np.random.default_rng(4)
    for signed in (False, True):
        s = np.sort(rng.integers(0, 1 << 32, 4097 + 64 * 5 + 3, dtype=np.uint64).astype(np.uint32))
        s = s[np.argsort(sm.flip(s, signed), kind="stable")]
        ladder = sm.levels(s, signed, top=64)
        assert [lv.size for lv in ladder] == sm.geometry(s.size, 64)[0]
        for below, above in zip(ladder, ladder[1:]):
            for j in range(above.size):
                assert above[j] == below[64 * j: 64 * j + 64].max()


def test_range_join_model_matches_a_plain_loop():
    rng = np.random.default_rng(5)
    for signed in (False, True):
        keys = rng.integers(0, 40, 150).astype(np.uint32) - np.uint32(20)
        lo = rng.integers(0, 50, 90).astype(np.uint32) - np.uint32(25)
        hi = lo + rng.integers(0, 4, 90).astype(np.uint32) - np.uint32(1)
        for left_outer in (False, True):
            want_b, want_p = [], []
            for i in range(lo.size):
                rows = [(_order(keys[b], signed), b) for b in range(keys.size)
                        if _order(lo[i], signed) <= _order(keys[b], signed) <= _order(hi[i], signed)]
                rows.sort()
                if not rows and left_outer:
                    rows = [(0, 0xFFFFFFFF)]
                want_b += [b for _, b in rows]
                want_p += [i] * len(rows)
            got_b, got_p = sm.range_join(keys, lo, hi, signed, left_outer)
            assert got_b.tolist() == want_b and got_p.tolist() == want_p
