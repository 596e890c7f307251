"""Test-only numpy model of dbench_select_range_u32 (dwarf_bench_amd/host/select_rows.hpp): the candidates, the clamped
device count, row ids outside the column, signed and negated predicates, the empty interval and the status bit, stated
candidate by candidate.  Never imported by the product."""
import numpy as np

SIGNED, NEGATE = 1, 2  # DBENCH_SELECT_SIGNED, DBENCH_SELECT_NEGATE
KEY_RANGE = 2          # DBHIP_DEV_KEY_RANGE


def pattern(v):
    """a bound given as a Python int of either signedness -> its 32-bit pattern"""
    return int(v) & 0xFFFFFFFF


def select_range(col, lo, hi, flags=0, in_rows=None, in_count=None):
    """col: uint32 column; lo, hi: 32-bit patterns; in_rows: uint32 row-id list of `in_capacity` entries or None;
    in_count: the device count (None: the whole list).  -> (kept row ids as uint32, in candidate order; status word)"""
    col = np.asarray(col, dtype=np.uint32)
    n_col = col.size
    if in_rows is None:
        cand = np.arange(n_col, dtype=np.uint32)
    else:
        in_rows = np.asarray(in_rows, dtype=np.uint32)
        m = in_rows.size if in_count is None else min(int(in_count), in_rows.size)
        cand = in_rows[:m]
    inside = cand.astype(np.int64) < n_col
    status = 0 if inside.all() else KEY_RANGE
    value = np.zeros(cand.size, dtype=np.uint32)
    value[inside] = col[cand[inside]]
    if flags & SIGNED:
        value, lo, hi = value.view(np.int32).astype(np.int64), _as_i32(lo), _as_i32(hi)
    else:
        value, lo, hi = value.astype(np.int64), pattern(lo), pattern(hi)
    in_interval = (value >= lo) & (value <= hi)  # lo > hi: never
    keep = inside & (in_interval != bool(flags & NEGATE))
    return cand[keep], status


def _as_i32(p):
    p = pattern(p)
    return p - (1 << 32) if p >> 31 else p


def chain(cols, bounds, flags=None):
    """select_range(cols[0]) refined on cols[1:], each with its (lo, hi): -> row ids"""
    rows = None
    for i, (c, (lo, hi)) in enumerate(zip(cols, bounds)):
        rows, _ = select_range(c, lo, hi, 0 if flags is None else flags[i], in_rows=rows)
    return rows
