"""Test-only numpy model of dbench_merge_u32 and dbench_setop_u32 (dwarf_bench_amd/host/merge_sorted.hpp): the clamped
device counts, the order under both signednesses with A first on ties, the three value modes with the row-id offset,
the three set operations and the status word.  Never imported by the product."""
import numpy as np

SIGNED, ROW_IDS = 1, 2                  # DBENCH_MERGE_SIGNED, DBENCH_MERGE_ROW_IDS
UNION, INTERSECT, DIFFERENCE = 0, 1, 2  # DBENCH_SETOP_*
STATUS = 0                              # no kernel of this family raises the status word


def clamp(col, count):
    """the entries of a capacity-sized column that count: min(count, capacity) of them (count None: all)"""
    col = np.asarray(col, dtype=np.uint32)
    return col if count is None else col[:min(int(count), col.size)]


def order(keys, signed):
    """keys as the integers they compare as"""
    return keys.view(np.int32).astype(np.int64) if signed else keys.astype(np.int64)


def merge(a_keys, b_keys, flags=0, a_vals=None, b_vals=None, a_count=None, b_count=None):
    """-> (out_keys, out_vals or None, out_count, status).  ROW_IDS: out_vals are r for A's row r and a_capacity + r for
    B's row r; otherwise a_vals and b_vals (both or neither) are carried."""
    a_capacity = np.asarray(a_keys).size
    a, b = clamp(a_keys, a_count), clamp(b_keys, b_count)
    both = np.concatenate([a, b])
    perm = np.argsort(order(both, bool(flags & SIGNED)), kind="stable")  # stable: A before B among equal keys
    vals = None
    if flags & ROW_IDS:
        assert a_vals is None and b_vals is None
        vals = np.concatenate([np.arange(a.size, dtype=np.uint32), a_capacity + np.arange(b.size, dtype=np.uint32)])[perm]
    elif a_vals is not None or b_vals is not None:
        vals = np.concatenate([clamp(a_vals, a_count), clamp(b_vals, b_count)])[perm]
    return both[perm], vals, both.size, STATUS


def setop(op, a, b, a_count=None, b_count=None):
    """strictly ascending uint32 lists -> (out, out_count, status), stated by membership: an element has a partner iff
    the other list holds its value; the union drops B's partnered elements, the intersection keeps A's partnered
    elements, the difference A's unpartnered ones"""
    a, b = clamp(a, a_count), clamp(b, b_count)
    in_b, in_a = np.isin(a, b), np.isin(b, a)
    if op == UNION:
        out = np.sort(np.concatenate([a, b[~in_a]]))
    elif op == INTERSECT:
        out = a[in_b]
    elif op == DIFFERENCE:
        out = a[~in_b]
    else:
        raise ValueError(op)
    return out.astype(np.uint32), out.size, STATUS
