"""Test-only numpy model of the quantile select (dwarf_bench_amd/host/quantile_select.hpp, quantile_layout.hpp): the candidates
of a call (the clamped count, the row-id list, the ids that do not count and raise the status), np.sort, the rank a
(q_num, q_den) pair names among m candidates in Python integers, and below / equal by searchsorted.  Never imported by the
product."""
import numpy as np

SIGNED = 1
MAX_RANKS = 16
KEY_RANGE = 2  # DBHIP_DEV_KEY_RANGE
U, W = np.uint32, np.uint64
SHIFTS, WIDTHS = (21, 10, 0), (11, 11, 10)  # the three levels' digits


def as_u32(col):
    k = np.atleast_1d(np.asarray(col))
    return k.view(U) if k.dtype.itemsize == 4 else (k.astype(W) & W(0xFFFFFFFF)).astype(U)


def length(count, capacity):
    """min(*count, capacity); None: no count pointer"""
    return capacity if count is None else min(int(count), capacity)


def candidates(col, rows=None, count=None):
    """-> (the candidates' keys in candidate order, the status word)"""
    col = as_u32(col)
    if rows is None:
        return col[: length(count, col.size)], 0
    rows = as_u32(rows)[: length(count, np.asarray(rows).size)]
    inside = rows.astype(W) < W(col.size)
    return col[rows[inside]], 0 if inside.all() else KEY_RANGE


def rank(num, den, m):
    """the 0-based rank (num, den) names among m candidates, or None: no such row"""
    num, den, m = int(num), int(den), int(m)
    if den == 0:
        r = num
    else:
        assert 0 <= num <= den
        r = 0 if num == 0 else -((-num * m) // den) - 1  # ceil(num * m / den) - 1
    return r if 0 <= r < m else None


def select(col, q_num, q_den, flags=0, rows=None, count=None):
    """-> (values, below, equal, status): three uint32 arrays of one entry per rank"""
    keys, st = candidates(col, rows, count)
    flip = U(0x80000000 if flags & SIGNED else 0)
    x = np.sort(keys ^ flip)
    m = x.size
    values, below, equal = (np.zeros(len(q_num), U) for _ in range(3))
    for j, (num, den) in enumerate(zip(q_num, q_den)):
        r = rank(num, den, m)
        if r is None:
            values[j], below[j], equal[j] = 0, m, 0
            continue
        v = x[r]
        lo, hi = np.searchsorted(x, v, "left"), np.searchsorted(x, v, "right")
        values[j], below[j], equal[j] = v ^ flip, lo, hi - lo
        assert lo <= r < hi
    return values, below, equal, st
