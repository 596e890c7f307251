"""numpy restatement of include/dbhip_scan_by_key.h: the contract's answer (one row per input row over runs of equal adjacent
keys) and the validator's four result words.  Test-only; never imported by the product.

The segmented running extremes are plain accumulates over composite 64-bit words: with R runs, the running minimum of
((R - 1 - run) << 32) | x never looks back over a head (an earlier run has a larger high half), and neither does the running
maximum of (run << 32) | x.  x = value ^ sign orders int32 values as unsigned.  The running sums are the column's cumulative
sum minus the cumulative sum in front of the run's head, mod 2^64."""
import numpy as np

NAMES = ("run_ids", "row_numbers", "sums", "mins", "maxs")
M64 = (1 << 64) - 1


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype.itemsize == 4 else np.asarray(a, dtype=np.uint32)


def head_flags(keys):
    keys = u32(keys)
    if keys.size == 0:
        return np.zeros(0, dtype=bool)
    return np.r_[True, keys[1:] != keys[:-1]]


def ext(vals, signed):
    """the values zero- or sign-extended to 64 bits, as uint64 bit patterns"""
    vals = u32(vals)
    return vals.view(np.int32).astype(np.int64).view(np.uint64) if signed else vals.astype(np.uint64)


def scan_by_key(keys, vals, signed=False):
    """-> (run_ids, row_numbers, sums, mins, maxs) as uint32 / uint32 / uint64 bit patterns / uint32 / uint32"""
    keys, vals = u32(keys), u32(vals)
    n = keys.size
    if n == 0:
        e = np.zeros(0, dtype=np.uint32)
        return e, e, np.zeros(0, dtype=np.uint64), e, e
    head = head_flags(keys)
    run = np.cumsum(head, dtype=np.uint64) - np.uint64(1)
    rows = np.arange(n, dtype=np.uint64)
    head_row = np.maximum.accumulate(np.where(head, rows, np.uint64(0)))
    row_numbers = rows - head_row + np.uint64(1)
    with np.errstate(over="ignore"):
        total = np.cumsum(ext(vals, signed), dtype=np.uint64)
        in_front = total - ext(vals, signed)  # the cumulative sum in front of every row
        sums = total - in_front[head_row.astype(np.int64)]
    x = (vals ^ np.uint32(0x80000000 if signed else 0)).astype(np.uint64)
    runs = run[-1] + np.uint64(1)
    mins = np.minimum.accumulate(((runs - np.uint64(1) - run) << np.uint64(32)) | x)
    maxs = np.maximum.accumulate((run << np.uint64(32)) | x)
    sign = np.uint32(0x80000000 if signed else 0)
    low = np.uint64(0xFFFFFFFF)
    return (run.astype(np.uint32), row_numbers.astype(np.uint32), sums, (mins & low).astype(np.uint32) ^ sign,
            (maxs & low).astype(np.uint32) ^ sign)


def check_words(keys, vals, run_ids=None, row_numbers=None, sums=None, mins=None, maxs=None, signed=False):
    """the four words of dbhip_check_scan_by_key_u32, as Python ints; a column that is None is skipped"""
    keys = u32(keys)
    n = keys.size
    if n == 0:
        return 0, M64, 0, 0
    v = u32(vals) if vals is not None else np.zeros(n, dtype=np.uint32)
    head = head_flags(keys)
    sign = np.uint32(0x80000000 if signed else 0)
    bad = np.zeros(n, dtype=np.int64)

    def prev(col):  # the column one row up (row 0 is a head: its entry is never used)
        return np.r_[col[:1], col[:-1]]
    with np.errstate(over="ignore"):
        if run_ids is not None:
            c = u32(run_ids)
            want = np.where(head, prev(c) + np.uint32(1), prev(c))
            want[0] = 0
            bad += c != want
        if row_numbers is not None:
            c = u32(row_numbers)
            bad += c != np.where(head, np.uint32(1), prev(c) + np.uint32(1))
        if sums is not None:
            c = np.ascontiguousarray(sums).view(np.uint64)
            e = ext(v, signed)
            bad += c != np.where(head, e, prev(c) + e)
        if mins is not None:
            c = u32(mins)
            bad += c != np.where(head, v, np.minimum(prev(c) ^ sign, v ^ sign) ^ sign)
        if maxs is not None:
            c = u32(maxs)
            bad += c != np.where(head, v, np.maximum(prev(c) ^ sign, v ^ sign) ^ sign)
    rows = np.flatnonzero(bad)
    return int(bad.sum()), int(rows[0]) if rows.size else M64, int(head.sum()), 0


def verdict(words, keys):
    """the table is right iff no (row, column) violates its rule; the heads are those of the input"""
    return words[0] == 0 and words[1] == M64 and words[2] == int(head_flags(keys).sum()) and words[3] == 0
