"""numpy restatement of include/dbhip_sorted_search.h: the search itself (np.searchsorted on the sign-flipped domain), the
fence ladder's geometry and workspace size as a function of (m, top), the ladder's levels, the validator's four words and the
range join's pair table.  Test infrastructure only; never imported by the product."""
import numpy as np

FANOUT = 64
TOP = 16384
MAX_M = 1 << 31
TOPS = tuple(1 << b for b in range(6, 15))  # the allowed top_entries (0 = TOP)
NONE = (1 << 64) - 1
U32 = np.uint32


def flip(a, signed):
    """the x domain: uint32 whose unsigned order is the column's order"""
    a = np.ascontiguousarray(a).view(U32)
    return a ^ U32(0x80000000) if signed else a


def geometry(m, top=0):
    """-> (counts, offsets, total): counts[l] entries of level l = 0..T, offsets[l] the byte offset of level l >= 1 in the
    workspace (offsets[0] = 0: level 0 is the column), total the workspace bytes"""
    top = top or TOP
    assert top in TOPS and 0 <= m <= MAX_M
    counts, offsets, total = [m], [0], 256
    while counts[-1] > top:
        nxt = (counts[-1] + FANOUT - 1) // FANOUT
        counts.append(nxt)
        offsets.append(total)
        total += (4 * nxt + 255) // 256 * 256
    return counts, offsets, total


def workspace_bytes(m, top=0):
    if m > MAX_M or (top or TOP) not in TOPS:
        return 0
    return geometry(m, top)[2]


def levels(sorted_keys, signed=False, top=0):
    """the ladder in the x domain: [level 0, level 1, ..., level T]"""
    out = [flip(sorted_keys, signed)]
    counts, _, _ = geometry(out[0].size, top)
    for count in counts[1:]:
        below = out[-1]
        last = np.minimum(np.arange(count, dtype=np.int64) * FANOUT + FANOUT - 1, below.size - 1)
        out.append(below[last])
    return out


def search(sorted_keys, lo, hi=None, signed=False):
    """-> (pos, cnt) as uint32; lo=None: minus infinity; hi=None: hi = lo"""
    s = flip(sorted_keys, signed)
    assert lo is not None or hi is not None
    n = (lo if lo is not None else hi).size
    pos = np.searchsorted(s, flip(lo, signed), side="left") if lo is not None else np.zeros(n, dtype=np.int64)
    end = np.searchsorted(s, flip(hi if hi is not None else lo, signed), side="right")
    return pos.astype(U32), np.where(end > pos, end - pos, 0).astype(U32)


def check(sorted_keys, lo, hi, pos, cnt, signed=False):
    """the four words of dbhip_check_sorted_search_u32, by its local rules, whatever the columns hold"""
    s = flip(sorted_keys, signed).astype(np.int64)
    m = s.size
    n = next(c for c in (lo, hi, pos, cnt) if c is not None).size
    xl = flip(lo, signed).astype(np.int64) if lo is not None else np.zeros(n, dtype=np.int64)
    xh = flip(hi, signed).astype(np.int64) if hi is not None else xl
    p = np.ascontiguousarray(pos).view(U32).astype(np.int64) if pos is not None else np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=np.int64)

    def at(idx, ok):  # s[idx] where ok, anything elsewhere
        return s[np.where(ok, idx, 0)] if m else np.zeros(n, dtype=np.int64)

    if pos is not None:
        ok = p <= m
        if lo is None:
            ok &= p == 0
        else:
            ok &= (p == 0) | (at(p - 1, ok & (p > 0)) < xl)
            ok &= (p == m) | (at(p, ok & (p < m)) >= xl)
        bad += ~ok
    pairs = 0
    if cnt is not None:
        c = np.ascontiguousarray(cnt).view(U32).astype(np.int64)
        pairs = int(c.sum())
        e = p + c
        ok = e <= m
        empty = (xh < xl) if lo is not None else np.zeros(n, dtype=bool)
        inner = ok & ~empty
        fine = ((e == 0) | (at(e - 1, inner & (e > 0)) <= xh)) & ((e == m) | (at(e, inner & (e < m)) > xh))
        ok &= np.where(empty, c == 0, fine)
        bad += ~ok
    rows = np.nonzero(bad)[0]
    return int(bad.sum()), int(rows[0]) if rows.size else NONE, pairs, 0


def range_join(build_keys, lo, hi=None, signed=False, left_outer=False):
    """-> (build_rows, probe_rows) as uint32: grouped by probe row ascending, inside a row by ascending build key, equal
    keys by ascending build row (a stable argsort); left_outer: (0xFFFFFFFF, row) for a probe row without a match"""
    x = flip(build_keys, signed)
    ids = np.argsort(x, kind="stable").astype(U32)
    pos, cnt = search(x[ids], flip(lo, signed) if lo is not None else None, flip(hi, signed) if hi is not None else None)
    pos, cnt = pos.astype(np.int64), cnt.astype(np.int64)
    each = np.maximum(cnt, 1) if left_outer else cnt
    probe_rows = np.repeat(np.arange(cnt.size, dtype=np.int64), each)
    first = np.cumsum(each) - each
    k = np.arange(probe_rows.size, dtype=np.int64) - first[probe_rows]
    hit = cnt[probe_rows] > 0
    at = np.where(hit, pos[probe_rows] + k, 0)
    build_rows = np.where(hit, ids[at] if ids.size else 0, 0xFFFFFFFF)
    return build_rows.astype(U32), probe_rows.astype(U32)
