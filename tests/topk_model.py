"""The top-k contract of include/dbhip_topk.h and its validator's two words, in numpy.  Test infrastructure: never imported
by the product.  Columns are uint32 arrays (the bits of an int32 column where the order is signed)."""
import numpy as np


def mask(largest=False, signed=False):
    """keys XOR this: better means smaller as unsigned"""
    return np.uint32((0x80000000 if signed else 0) ^ (0xFFFFFFFF if largest else 0))


def topk(keys, k, largest=False, signed=False, sorted=True):
    """-> (keys, rows), uint32: the first m = min(k, n) rows by (key, row), in that order or (sorted=False) by row"""
    keys = np.ascontiguousarray(keys).view(np.uint32)
    m = min(int(k), keys.size)
    rows = np.argsort(keys ^ mask(largest, signed), kind="stable")[:m]
    if not sorted:
        rows = np.sort(rows)
    return keys[rows], rows.astype(np.uint32)


def check_words(keys, out_keys, out_rows, largest=False, signed=False):
    """the two words of dbhip_check_topk_u32 for a table of k = len(out_keys) entries"""
    keys = np.ascontiguousarray(keys).view(np.uint32)
    n = keys.size
    m = min(len(out_keys), n)
    if m == 0:
        return (0, 0)
    msk = mask(largest, signed)
    ok = np.ascontiguousarray(out_keys).view(np.uint32)[:m]
    orow = np.ascontiguousarray(out_rows).view(np.uint32)[:m].astype(np.int64)
    ox = (ok ^ msk).astype(np.uint64)
    in_range = orow < n
    bad = ~in_range
    bad[in_range] |= keys[orow[in_range]] != ok[in_range]
    pair = (ox << np.uint64(32)) | orow.astype(np.uint64)  # a (key, row) pair as one number: precedes <=> smaller
    bad[1:] |= ~(pair[:-1] < pair[1:])
    all_pairs = ((keys ^ msk).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return (int(bad.sum()), int((all_pairs < pair[-1]).sum()))


def verdict(words, k, n):
    m = min(k, n)
    return tuple(words) == (0, m - 1 if m else 0)
