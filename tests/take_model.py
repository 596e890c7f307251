"""Test-only numpy model of dbench_take_u32 and dbench_aggregate_rows_u32 (dwarf_bench_amd/host/take_rows.hpp): the
clamped length, the fill, the "no row" id of DBENCH_TAKE_OUTER, the skipped candidates, the status word that results and
the empty aggregate.  Never imported by the product."""
import numpy as np

OUTER, SIGNED = 1, 2
NO_ROW = 0xFFFFFFFF
KEY_RANGE = 2  # DBHIP_DEV_KEY_RANGE
M64 = (1 << 64) - 1


def length(count, capacity):
    """m = min(*count, capacity); count None: the capacity.  count is any uint64"""
    return int(capacity) if count is None else min(int(count) & M64, int(capacity))


def _split(rows, m, n_rows, flags):
    """the first m entries as uint32 -> (entries, those that name a row, the status word)"""
    e = np.asarray(rows).view(np.uint32)[:m]
    inside = e.astype(np.uint64) < np.uint64(n_rows)
    excused = (e == np.uint32(NO_ROW)) if flags & OUTER else np.zeros(e.size, bool)
    return e, inside, (KEY_RANGE if bool((~inside & ~excused).any()) else 0)


def take(cols, rows, count=None, flags=0, fill=0, before=None):
    """cols: uint32 arrays of one length; rows: the list (its size is the capacity); before: what the outputs held (one
    array per column, or None: zeros) -> (the outputs, all `capacity` entries each, the status word)"""
    cols = [np.asarray(c).view(np.uint32) for c in cols]
    n_rows, capacity = cols[0].size, np.asarray(rows).size
    assert all(c.size == n_rows for c in cols) and not flags & ~OUTER
    m = length(count, capacity)
    e, inside, status = _split(rows, m, n_rows, flags)
    outs = []
    for c, col in enumerate(cols):
        out = np.zeros(capacity, np.uint32) if before is None else np.asarray(before[c]).view(np.uint32).copy()
        got = np.full(m, fill & 0xFFFFFFFF, np.uint32)
        got[inside] = col[e[inside]]
        out[:m] = got
        outs.append(out)
    return outs, status


def aggregate(col, rows=None, count=None, flags=0):
    """-> ((count, sum mod 2^64, min, max) as the four uint64 words out[] holds, the status word)"""
    col = np.asarray(col).view(np.uint32)
    assert not flags & ~(OUTER | SIGNED)
    if rows is None:
        assert count is None
        vals, status = col, 0
    else:
        e, inside, status = _split(rows, length(count, np.asarray(rows).size), col.size, flags)
        vals = col[e[inside]]
    if flags & SIGNED:
        wide = [int(v) for v in vals.view(np.int32)]
        least, most = (1 << 31) - 1, -(1 << 31)
    else:
        wide = [int(v) for v in vals]
        least, most = 0xFFFFFFFF, 0
    if wide:
        least, most = min(wide), max(wide)
    return (len(wide), sum(wide) & M64, least & M64, most & M64), status


def as_ints(words, signed):
    """the four uint64 words -> what ops.AggregateRows.result() returns"""
    n, total, least, most = (int(w) & M64 for w in words)
    if signed:
        total, least, most = (w - (1 << 64) if w >> 63 else w for w in (total, least, most))
    return n, total, (least if n else None), (most if n else None)
