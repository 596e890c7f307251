"""numpy restatement of include/dbhip_reduce_by_key.h: the contract's answer (one row per run of equal adjacent keys) and
the validator's four result words.  Test-only; never imported by the product."""
import numpy as np

from tests.validator_model import mix64

M64 = (1 << 64) - 1
WEIGHT_SEED = 0x72626B


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype.itemsize == 4 else np.asarray(a, dtype=np.uint32)


def heads(keys):
    keys = np.asarray(keys)
    if keys.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])


def reduce_by_key(keys, vals, signed=False):
    """-> (keys, counts, sums, mins, maxs) as uint32 / uint32 / uint64 bit patterns / uint32 / uint32"""
    keys, vals = u32(keys), u32(vals)
    h = heads(keys)
    if keys.size == 0:
        e = np.zeros(0, dtype=np.uint32)
        return e, e, np.zeros(0, dtype=np.uint64), e, e
    counts = np.diff(np.r_[h, keys.size]).astype(np.uint32)
    if signed:
        v = vals.view(np.int32)
        sums = np.add.reduceat(v.astype(np.int64), h).view(np.uint64)
    else:
        v = vals
        sums = np.add.reduceat(v.astype(np.uint64), h)
    mins = np.minimum.reduceat(v, h).view(np.uint32)
    maxs = np.maximum.reduceat(v, h).view(np.uint32)
    return keys[h], counts, sums, mins, maxs


def weight(run):
    return mix64(WEIGHT_SEED, run) | np.uint64(1)


def _bisect(starts, rows):
    """per row the last r of the validator's bisection with starts[r] <= row (starts need not ascend in a wrong table)"""
    lo = np.zeros(rows.size, dtype=np.int64)
    hi = np.full(rows.size, starts.size, dtype=np.int64)
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            return lo
        mid = lo + (hi - lo) // 2
        left = open_ & (starts[np.minimum(mid, starts.size - 1)].astype(np.int64) <= rows)
        lo = np.where(left, mid, lo)
        hi = np.where(open_ & ~left, mid, hi)


def check_words(keys, vals, out_keys, out_counts, out_sums, out_mins, out_maxs, signed=False):
    """the four words of dbhip_check_reduce_by_key_u32, as Python ints"""
    keys, vals = u32(keys), u32(vals)
    ok, oc, omn, omx = u32(out_keys), u32(out_counts), u32(out_mins), u32(out_maxs)
    osum = np.ascontiguousarray(out_sums).view(np.uint64)
    n, runs = keys.size, ok.size
    sign = np.uint32(0x80000000 if signed else 0)
    with np.errstate(over="ignore"):
        starts = (np.cumsum(oc, dtype=np.uint64) - oc.astype(np.uint64)).astype(np.uint32)  # 32-bit, as the device scan
    total = int(oc.astype(np.uint64).sum()) if runs else 0
    faults = int(total != n)
    faults += int((oc == 0).sum())
    r = np.arange(1, runs)
    s = starts[1:].astype(np.int64)
    inside = (s >= 1) & (s <= n)
    faults += int((keys[s[inside] - 1] == ok[r[inside]]).sum()) if runs > 1 else 0
    with np.errstate(over="ignore"):
        word3 = int((osum * weight(np.arange(runs, dtype=np.uint64))).sum(dtype=np.uint64)) if runs else 0
    covered = min(total, n) if runs else 0
    faults += n - covered  # rows behind the table
    word2, unseen = 0, 2 * runs
    if covered:
        rows = np.arange(covered, dtype=np.int64)
        run = _bisect(starts, rows)
        k, v = keys[:covered], vals[:covered]
        x, mn, mx = v ^ sign, omn[run] ^ sign, omx[run] ^ sign
        faults += int((k != ok[run]).sum()) + int(((x < mn) | (x > mx)).sum())
        unseen -= np.unique(run[x == mn]).size + np.unique(run[x == mx]).size
        ext = v.view(np.int32).astype(np.int64).view(np.uint64) if signed else v.astype(np.uint64)
        with np.errstate(over="ignore"):
            word2 = int((ext * weight(run.astype(np.uint64))).sum(dtype=np.uint64))
    return faults, unseen, word2 & M64, word3 & M64


def verdict(words):
    return words[0] == 0 and words[1] == 0 and words[2] == words[3]
