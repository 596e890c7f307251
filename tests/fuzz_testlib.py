"""Test-only seeded draws for the randomised sweeps of the eleven newer operators (tests/test_gpu_fuzz.py on the GPU,
tests/test_fuzz_draws_host.py on the CPU, tools/fuzz_gpu.py): per operator draws(rng) yields cases, model(case) is what
a correct call leaves behind, check(case, result) compares a result with it exactly.

A case is a dict of host numpy inputs and parameters; nothing here touches torch or the GPU.  Every dimension of a case
(size, the placement of every buffer, each device count, each flag, the distributions) is drawn on its own.  A result is
a dict of what one call leaves behind: every output buffer IN FULL (so the entries behind the count, which must still
hold the fill word the buffer started with), the device count and the status word.  Never imported by the product."""
import numpy as np

from dwarf_bench_amd import bitpack_native as bn
from dwarf_bench_amd import dict_native as dn
from dwarf_bench_amd import merge_native as mn
from dwarf_bench_amd import select_native as sn
from dwarf_bench_amd import take_native as tn
from tests import bitpack_model as bm
from tests import dict_model as dm
from tests import merge_model as mm
from tests import reduce_by_key_model as rbm
from tests import scan_by_key_model as sbm
from tests import select_model as sm
from tests import sorted_search_model as ssm
from tests import take_model as tm
from tests import topk_model as tkm

U = np.uint32
FILLS = (0x5A5A5A5A, 0xA5A5A5A5)  # guard_testlib.FILLS (which imports torch); the GPU sweep holds the two together
SCAN_ROUND = 1024                 # segments or tiles rowlist_scan_kernel counts in one round
MAX_ROWS = 1 << 18                # every draw but the one second-round draw stays at or below this
COUNT_KINDS = ("none", "zero", "one", "below", "capacity", "above", "huge")
EDGES = np.array([0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], U)
KEY_KINDS = 9


# ---- the dimensions every operator draws from ------------------------------------------------------------------------
def u32(x):
    return np.asarray(x, dtype=np.uint64).astype(U)


def sizes(rng, count, seams, hi_log2=18):
    """0, 1, every seam with both neighbours, and `count` log-uniform sizes up to 2^hi_log2, shuffled"""
    out = [0, 1] + [s + d for s in seams for d in (-1, 0, 1)] + [int(2 ** rng.uniform(0, hi_log2)) for _ in range(count)]
    assert max(out) <= MAX_ROWS
    return [int(s) for s in rng.permutation(np.array(out))]


def offset(rng):
    """4-byte words past a 16-byte boundary"""
    return int(rng.integers(0, 4))


def device_count(rng, capacity):
    """a device count of one of COUNT_KINDS (None: the call gets no count pointer); the one draw above MAX_ROWS keeps
    all its entries, so that its scan does run a second round"""
    kinds = COUNT_KINDS if capacity <= MAX_ROWS else ("none", "capacity", "above", "huge")
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind == "below":
        return int(rng.integers(2, capacity)) if capacity > 2 else 0
    return {"none": None, "zero": 0, "one": 1, "capacity": capacity, "above": capacity + 1, "huge": 1 << 40}[kind]


def count_kind(count, capacity):
    """the kind a drawn count is at its capacity, or None where small capacities make kinds coincide"""
    if count is None:
        return "none"
    if capacity < 3:
        return None
    if count in (0, 1):
        return ("zero", "one")[count]
    return "below" if count < capacity else {capacity: "capacity", capacity + 1: "above"}.get(count, "huge")


def counted(count, capacity):
    return capacity if count is None else min(count, capacity)


def keys(rng, n, kind):
    """the kinds of _keys in tests/test_gpu_fuzz.py (0 .. 7), and 8: values at both ends of both number lines"""
    if kind == 0:
        return u32(rng.integers(1, 10001, n))
    if kind == 1:
        return u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))
    if kind == 2:
        return np.full(n, int(rng.integers(0, 1 << 32)), dtype=U)
    if kind == 3:
        return u32(rng.integers(0, 4, n)) * U(0x01000000)
    if kind == 5:
        k = u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))
        k[rng.random(n) < 0.9] = U(rng.integers(0, 1 << 32))
        return k
    if kind == 6:
        return np.where(rng.integers(0, 2, size=n) == 1, U(0xFFFFFFFF), U(0))
    if kind == 8:
        k = u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))
        at = rng.random(n) < 0.5
        k[at] = EDGES[rng.integers(0, EDGES.size, int(at.sum()))]
        return k
    return np.sort(u32(rng.integers(0, max(n, 1) + 1, n)))


def row_list(rng, m, n_rows, bad_ids):
    """m row ids into a column of n_rows: sorted, shuffled or repeated; with bad_ids about one in fifty lies outside the
    column (n_rows itself, 2^31 and 2^32 - 1 among them)"""
    kind = int(rng.integers(0, 3))
    inside = u32(rng.integers(0, max(n_rows, 1), m)) if kind < 2 else u32(rng.integers(0, max(n_rows // 100, 1), m))
    if kind == 0:
        inside = np.sort(inside)
    if n_rows == 0:
        bad_ids = True  # (no id names a row of an empty column)
    if bad_ids and m:
        at = np.flatnonzero(rng.random(m) < 0.02) if n_rows else np.arange(m)
        at = at if at.size else rng.integers(0, m, 1)
        special = np.array([n_rows, n_rows + 1, 0x80000000, 0xFFFFFFFF], np.uint64)
        inside[at] = np.where(rng.random(at.size) < 0.5, special[rng.integers(0, 4, at.size)],
                              rng.integers(n_rows, 1 << 32, at.size, dtype=np.uint64)).astype(U)
    return inside


def spoil_tail(rng, rows, count, n_rows):
    """behind its count a list holds row ids outside the column"""
    if count is not None and count < rows.size:
        rows[count:] = u32(rng.integers(n_rows, 1 << 32, rows.size - count, dtype=np.uint64))
        rows[count] = n_rows
    return rows


def interval(rng, values, signed):
    """[lo, hi] as 32-bit patterns -> (kind, lo, hi): between two of the values, the same reversed (empty), the full
    range, an interval on both sides of 2^31, one value"""
    kind = ("between", "reversed", "full", "straddle", "point")[int(rng.integers(0, 5))]
    v = [int(x) for x in values[rng.integers(0, values.size, 2)]] if values.size else [5, 500]
    as_cmp = (lambda p: p - (1 << 32) if p >> 31 else p) if signed else (lambda p: p)
    lo, hi = sorted(v, key=as_cmp)
    if kind == "reversed":
        lo, hi = (hi, lo) if lo != hi else (1, 0)
    elif kind == "full":
        lo, hi = (0x80000000, 0x7FFFFFFF) if signed else (0, 0xFFFFFFFF)
    elif kind == "straddle":
        lo, hi = 0x7FFFFF00, 0x800000FF
    elif kind == "point":
        hi = lo
    return kind, lo, hi


def _full(n, fill, head=None):
    """a buffer of n entries that started as the fill word and whose first entries were written"""
    out = np.full(n, fill, U)
    if head is not None:
        out[: head.size] = head
    return out


def same(case, result, want):
    """result and want hold the same fields with the same values, bit for bit"""
    assert set(result) == set(want), (sorted(result), sorted(want))
    for name, w in want.items():
        g = result[name]
        if isinstance(w, (list, tuple)) and len(w) and isinstance(w[0], np.ndarray):
            assert len(g) == len(w), (case["what"], name)
            pairs = list(zip(g, w))
        else:
            pairs = [(g, w)]
        for c, (gi, wi) in enumerate(pairs):
            if isinstance(wi, np.ndarray):
                gi = np.ascontiguousarray(gi).view(wi.dtype)
                assert gi.size == wi.size, (case["what"], name, c, gi.size, wi.size)
                bad = np.flatnonzero(gi != wi)
                assert bad.size == 0, (f"{case['what']}: {name}[{c}] differs at {bad.size} of {wi.size} entries, the first "
                                       f"at {int(bad[0])}: {int(gi[bad[0]]):#x}, the model has {int(wi[bad[0]]):#x}")
            else:
                assert gi == wi, (case["what"], name, gi, wi)


# ---- selection vectors ---------------------------------------------------------------------------------------------------
SELECT_SEAMS = (64, sn.SEGMENT_ROWS, 2 * sn.SEGMENT_ROWS)


def select_draws(rng, log_uniform=30):
    todo = sizes(rng, log_uniform, SELECT_SEAMS) + [SCAN_ROUND * sn.SEGMENT_ROWS + int(rng.integers(1, 2 * sn.SEGMENT_ROWS))]
    for cand in todo:
        listed = bool(rng.integers(0, 3))
        signed, negate, count_only = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), rng.integers(0, 5) == 0
        n_col = cand if not listed else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 17)))
        col = keys(rng, n_col, int(rng.integers(0, KEY_KINDS)))
        rows = count = None
        if listed:
            rows = row_list(rng, cand, n_col, bool(rng.integers(0, 2)))
            count = device_count(rng, cand)
            spoil_tail(rng, rows, count, n_col)
        kind, lo, hi = interval(rng, col, signed)
        yield dict(what="select", col=col, rows=rows, count=count, lo=lo, hi=hi, interval=kind, signed=signed, negate=negate,
                   flags=(sm.SIGNED if signed else 0) | (sm.NEGATE if negate else 0), count_only=bool(count_only),
                   offs=dict(col=offset(rng), rows=offset(rng), out=offset(rng)), size=cand)


def select_model(case):
    want, st = sm.select_range(case["col"], case["lo"], case["hi"], case["flags"], case["rows"], case["count"])
    return dict(out=_full(case["size"], case["fill"], None if case["count_only"] else want), count=int(want.size), status=st)


# ---- merge and set operations --------------------------------------------------------------------------------------------
T = mn.TILE_ROWS
MERGE_SEAMS = (T, 2 * T)
MODES = ("keys", "carried", "ids")


def _split(rng, total):
    """the merged size split over A and B: all on one side, halves, anything"""
    how = int(rng.integers(0, 4))
    na = (0, total, total // 2, int(rng.integers(0, total + 1)))[how]
    return na, total - na


def ascending_pair(rng, na, nb):
    """two STRICTLY ascending lists that share a drawn part of their values, reaching the ends of the range at times"""
    m = na + nb
    gaps = rng.integers(1, 4, m, dtype=np.uint64)
    universe = np.cumsum(gaps) - gaps[:1] if m else np.zeros(0, np.uint64)  # starts at 0
    if m and rng.integers(0, 3) == 0:  # over the whole range, the last value 2^32 - 1
        universe = universe * np.uint64(0xFFFFFFFF // max(int(universe[-1]), 1))
        universe[-1] = 0xFFFFFFFF
    share = float(rng.choice([0.0, 0.01, 0.5, 0.99, 1.0]))
    perm = rng.permutation(m)
    in_a, rest = perm[:na], perm[na:]
    common = int(round(share * min(na, nb)))
    in_b = np.concatenate([in_a[:common], rest[: nb - common]])
    return universe[np.sort(in_a)].astype(U), universe[np.sort(in_b)].astype(U), share


def merge_draws(rng, log_uniform=24):
    """set operations and merges in turn over the same sizes: na + nb is the size (the tiles cut the merged order)"""
    setops = sizes(rng, log_uniform, MERGE_SEAMS) + [(SCAN_ROUND + 1) * T + int(rng.integers(1, T))]
    for total in setops:
        na, nb = _split(rng, total) if total <= MAX_ROWS else (total // 2 + 1, total - total // 2 - 1)
        a, b, share = ascending_pair(rng, na, nb)
        ca, cb = device_count(rng, na), device_count(rng, nb)
        for lst, cnt in ((a, ca), (b, cb)):  # behind its count a list holds anything, unsorted
            if cnt is not None and cnt < lst.size:
                lst[cnt:] = u32(rng.integers(0, 1 << 32, lst.size - cnt, dtype=np.uint64))
                lst[cnt] = 0
        yield dict(what="setop", op=int(rng.integers(0, 3)), a=a, b=b, a_count=ca, b_count=cb, share=share,
                   count_only=bool(rng.integers(0, 5) == 0), offs=dict(a=offset(rng), b=offset(rng), out=offset(rng)), size=total)
    for total in sizes(rng, log_uniform, MERGE_SEAMS):
        na, nb = _split(rng, total)
        signed = bool(rng.integers(0, 2))
        kind = int(rng.choice([1, 2, 7, 7, 8]))  # full range, all equal, duplicates across the tile edges, the edges
        a, b = keys(rng, na, kind), keys(rng, nb, kind)
        if kind == 2 and nb:
            b[:] = a[0] if na else b[0]
        ca, cb = device_count(rng, na), device_count(rng, nb)
        a, b = (k[np.argsort(mm.order(k, signed), kind="stable")] for k in (a, b))
        for lst, cnt in ((a, ca), (b, cb)):
            if cnt is not None and cnt < lst.size:
                lst[cnt:] = u32(rng.integers(0, 1 << 32, lst.size - cnt, dtype=np.uint64))
        yield dict(what="merge", a=a, b=b, a_vals=keys(rng, na, 1), b_vals=keys(rng, nb, 1), a_count=ca, b_count=cb,
                   signed=signed, mode=MODES[int(rng.integers(0, 3))], size=total,
                   offs={name: offset(rng) for name in ("a", "b", "a_vals", "b_vals", "out_keys", "out_vals")})


def merge_model(case):
    a, b, fill = case["a"], case["b"], case["fill"]
    if case["what"] == "setop":
        want, k, st = mm.setop(case["op"], a, b, case["a_count"], case["b_count"])
        room = mn.set_bound(case["op"], a.size, b.size)
        return dict(out=_full(room, fill, None if case["count_only"] else want), count=k, status=st)
    mode = case["mode"]
    flags = (mm.SIGNED if case["signed"] else 0) | (mm.ROW_IDS if mode == "ids" else 0)
    carried = mode == "carried"
    keys_, vals, k, st = mm.merge(a, b, flags, case["a_vals"] if carried else None, case["b_vals"] if carried else None,
                                  case["a_count"], case["b_count"])
    res = dict(out_keys=_full(a.size + b.size, fill, keys_), count=k, status=st)
    if mode != "keys":
        res["out_vals"] = _full(a.size + b.size, fill, vals)
    return res


# ---- take and aggregate --------------------------------------------------------------------------------------------------
TAKE_SEAMS = (4, tn.SEGMENT_ROWS, 2 * tn.SEGMENT_ROWS)


def take_draws(rng, log_uniform=24):
    for what in ("take", "aggregate"):
        for capacity in sizes(rng, log_uniform, TAKE_SEAMS, hi_log2=17):
            outer, signed = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
            n_rows = 0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 17))
            dense = what == "aggregate" and rng.integers(0, 4) == 0  # all rows of the column, no list
            if dense:
                n_rows = capacity
            n_cols = int(rng.choice([1, 2, 3, 4, 4, 4])) if what == "take" else 1  # (half of them with a fourth column to place)
            kind = int(rng.choice([1, 2, 6, 8, 8]))  # sums that pass 2^32, both ends of the signed range
            cols = [keys(rng, n_rows, kind) for _ in range(n_cols)]
            rows = count = None
            if not dense:
                rows = row_list(rng, capacity, n_rows, bool(rng.integers(0, 2)))
                if outer and capacity and rng.integers(0, 2):  # the "no row" id alone: filled or skipped without raising
                    rows[rows >= n_rows] = tn.NO_ROW
                count = device_count(rng, capacity)
                spoil_tail(rng, rows, count, n_rows)
            case = dict(what=what, cols=cols, rows=rows, count=count, outer=outer, size=capacity,
                        offs=dict(rows=offset(rng), **{f"col{c}": offset(rng) for c in range(n_cols)}))
            if what == "take":
                case.update(fill_word=int(rng.integers(0, 1 << 32)), flags=tn.OUTER if outer else 0)
                case["offs"].update({f"out{c}": offset(rng) for c in range(n_cols)})
            else:
                case.update(signed=signed, flags=(tn.OUTER if outer else 0) | (tn.SIGNED if signed else 0),
                            ws_capacity=0 if dense and rng.integers(0, 2) else capacity)
            yield case


def take_model(case):
    if case["what"] == "aggregate":
        words, st = tm.aggregate(case["cols"][0], case["rows"], case["count"], case["flags"])
        return dict(words=tuple(words), status=st)
    before = [np.full(case["size"], case["fill"], U) for _ in case["cols"]]
    outs, st = tm.take(case["cols"], case["rows"], case["count"], case["flags"], case["fill_word"], before=before)
    return dict(outs=outs, status=st)


# ---- bit-packed columns --------------------------------------------------------------------------------------------------
BITPACK_SEAMS = (32, 128, bn.TILE_ROWS, bn.SEGMENT_ROWS, 2 * bn.SEGMENT_ROWS)
SPARE_WORDS = 8  # out_packed has this many words more than the capacity's packed form
BIG_WIDTHS = 3   # the second-round draw: the model holds a byte per bit of the column


def _packed_column(rng, n_rows, width):
    """-> (base, the decoded values, the packed words): base 0, an ordinary one, or one whose sums wrap past 2^32"""
    base = int(rng.choice([0, int(rng.integers(1, 1 << 20)), 0xFFFFFFF0, int(rng.integers(0, 1 << 32))]))
    kind = int(rng.integers(0, 4))
    codes = (u32(rng.integers(0, 1 << width, n_rows, dtype=np.uint64)) if kind < 2 else
             np.zeros(n_rows, U) if kind == 2 else np.full(n_rows, bm.mask(width), U))
    return base, codes + U(base), bm.pack_codes(codes, width)


def bitpack_draws(rng, log_uniform=24):
    big = SCAN_ROUND * bn.SEGMENT_ROWS + int(rng.integers(1, 2 * bn.SEGMENT_ROWS))
    for what in ("pack", "unpack", "select"):
        for size in sizes(rng, log_uniform, BITPACK_SEAMS, hi_log2=17) + ([big] if what == "select" else []):
            width = int(rng.integers(1, 33)) if size <= MAX_ROWS else int(rng.integers(1, BIG_WIDTHS + 1))
            listed = what != "pack" and bool(rng.integers(0, 2))
            n_rows = size if not listed else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 16)))
            base, values, packed = _packed_column(rng, n_rows, width)
            case = dict(what=what, width=width, base=base, size=size, offs={})
            if what == "pack":
                if width < 32 and size and rng.integers(0, 4) == 0:  # rows that do not fit: they keep their low bits
                    at = rng.integers(0, size, max(size // 50, 1))
                    values[at] = u32((rng.integers(0, 1 << 32, at.size, dtype=np.uint64) | np.uint64(1 << width)) + np.uint64(base))
                yield dict(case, col=values, count=device_count(rng, size), offs=dict(col=offset(rng)))
                continue
            rows = count = None
            outer = bool(rng.integers(0, 2))
            if listed:
                rows = row_list(rng, size, n_rows, bool(rng.integers(0, 2)))
                if what == "unpack" and outer and size and rng.integers(0, 2):
                    rows[rows >= n_rows] = bn.NO_ROW
                count = device_count(rng, size)
                spoil_tail(rng, rows, count, n_rows)
                case["offs"]["rows"] = offset(rng)
            case["offs"]["out"] = offset(rng)
            case.update(packed=packed, n_rows=n_rows, rows=rows, count=count)
            if what == "unpack":
                yield dict(case, outer=outer, flags=bn.OUTER if outer else 0, fill_word=int(rng.integers(0, 1 << 32)))
            else:
                signed, negate = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                kind, lo, hi = interval(rng, values, signed)
                yield dict(case, lo=lo, hi=hi, interval=kind, signed=signed, negate=negate, count_only=bool(rng.integers(0, 5) == 0),
                           flags=(bn.SIGNED if signed else 0) | (bn.NEGATE if negate else 0))


def bitpack_model(case):
    what, width, base, fill = case["what"], case["width"], case["base"], case["fill"]
    if what == "pack":
        col = case["col"]
        out, st = bm.pack(col, width, base, case["count"], before=np.full(bm.words(col.size, width) + SPARE_WORDS, fill, U))
        return dict(out=out, status=st)
    if what == "unpack":
        out, st = bm.unpack(case["packed"], case["n_rows"], width, base, case["rows"], case["count"], case["flags"],
                            case["fill_word"], before=np.full(case["size"], fill, U))
        return dict(out=out, status=st)
    want, st = bm.select_range(case["packed"], case["n_rows"], width, base, case["lo"], case["hi"], case["rows"], case["count"],
                               case["flags"])
    return dict(out=_full(case["size"], fill, None if case["count_only"] else want), count=int(want.size), status=st)


# ---- dictionary encoding -------------------------------------------------------------------------------------------------
BUILD_TILE, ENCODE_TILE = 1024, 4096  # tests/test_gpu_dict.py: rows of a workgroup at a time in the insert and the encode kernels
LDS_CAPACITY = dn.LDS_SLOTS // 2      # the largest capacity whose table the encode kernel keeps in LDS
DICT_SEAMS = (64, 256, BUILD_TILE, ENCODE_TILE)
CAPACITY_KINDS = ("below", "at", "above", "far above")


def dict_draws(rng, log_uniform=24):
    """a build, then the encode of another column through the dictionary it left in the workspace"""
    for n in sizes(rng, log_uniform, DICT_SEAMS, hi_log2=17):
        signed = bool(rng.integers(0, 2))
        pool = int(rng.choice([1, 2, 37, 300, LDS_CAPACITY - 1, LDS_CAPACITY, LDS_CAPACITY + 1, 20000]))
        values = np.unique(np.r_[EDGES[::2], u32(rng.integers(0, 1 << 32, pool, dtype=np.uint64))])
        values = rng.permutation(values)[:pool]
        col = values[rng.integers(0, values.size, n)] if n else np.zeros(0, U)
        count = device_count(rng, n)
        if count is not None and count < n:  # behind the count: values of their own, which must not enter the dictionary
            col[count:] = u32(rng.integers(0, 1 << 32, n - count, dtype=np.uint64))
        d = dm.ordered(col[: counted(count, n)], dm.SIGNED if signed else 0).size
        kind = CAPACITY_KINDS[int(rng.integers(0, 4))]
        capacity = {"below": d - 1, "at": d, "above": d + 1, "far above": d + int(rng.integers(2, 5000))}[kind]
        if capacity < 1:
            kind, capacity = ("at", 1) if d == 1 else ("above", 1)
        n_probe = sizes(rng, 0, DICT_SEAMS)[int(rng.integers(0, 2 + 3 * len(DICT_SEAMS)))] if rng.integers(0, 2) else int(2 ** rng.uniform(0, 16))
        absent = u32(rng.integers(0, 1 << 32, n_probe, dtype=np.uint64))
        probe = np.where(rng.random(n_probe) < 0.7, col[rng.integers(0, n, n_probe)] if n else absent, absent)
        yield dict(what="dict", col=col, count=count, capacity=int(capacity), capacity_kind=kind, distinct=int(d), signed=signed,
                   flags=dm.SIGNED if signed else 0, probe=probe, probe_count=device_count(rng, n_probe),
                   want_misses=bool(rng.integers(0, 2)), size=n,
                   offs=dict(col=offset(rng), keys=offset(rng), probe=offset(rng), codes=offset(rng)))


def dict_model(case):
    keys_, st = dm.build(case["col"], case["capacity"], case["count"], case["flags"])
    codes, misses = dm.encode(keys_, case["probe"], case["probe_count"], case["flags"])
    return dict(keys=_full(case["capacity"], case["fill"], keys_), distinct=int(keys_.size), status=st,
                codes=_full(case["probe"].size, case["fill"], codes), misses=misses if case["want_misses"] else None)


def dict_check(case, result):
    """out_keys[d .. capacity) is unspecified after a build that fits (dict_encode.hpp); a full table writes none of it"""
    want = dict_model(case)
    d = want["distinct"]
    if want["status"] == 0 and result["distinct"] == d:
        result = dict(result, keys=np.r_[np.asarray(result["keys"]).view(U)[:d], want["keys"][d:]])
    same(case, result, want)


# ---- top-k, reduce-by-key, scan-by-key: every column on a 16-byte boundary, as their headers demand ------------------
S, C = 4096, 32768  # the segment and chunk rows tests/test_gpu_topk.py and the by-key files name
BY_KEY_SEAMS = (64, 256, S, C)
TOPK_SEAMS = (64, S, 2 * S, C)
K_KINDS = ("zero", "one", "inside", "n - 1", "n", "above n")


def topk_draws(rng, log_uniform=24):
    for n in sizes(rng, log_uniform, TOPK_SEAMS):
        kind = K_KINDS[int(rng.integers(0, len(K_KINDS)))]
        k = {"zero": 0, "one": 1, "inside": int(rng.integers(0, n + 1)), "n - 1": max(n - 1, 0), "n": n,
             "above n": n + int(rng.integers(1, 6))}[kind]
        yield dict(what="topk", keys=keys(rng, n, int(rng.integers(0, KEY_KINDS))), k=k, k_kind=kind, size=n, offs={},
                   largest=bool(rng.integers(0, 2)), signed=bool(rng.integers(0, 2)), sorted=bool(rng.integers(0, 2)))


def topk_model(case):
    out_keys, out_rows = tkm.topk(case["keys"], case["k"], case["largest"], case["signed"], case["sorted"])
    return dict(out_keys=_full(case["k"], case["fill"], out_keys), out_rows=_full(case["k"], case["fill"], out_rows), status=0)


RUN_KINDS = ("all distinct", "about 40", "one run", "about 1.5", "a key that returns")


def run_keys(rng, n, kind):
    """keys by the lengths of their runs of equal neighbours"""
    if kind == "all distinct":
        return u32(rng.permutation(n)) + U(17)
    if kind == "one run":
        return np.full(n, 0xDEADBEEF, U)
    mean = {"about 40": 40, "about 1.5": 1.5, "a key that returns": 3}[kind]
    run = np.cumsum(rng.random(n) < 1.0 / mean, dtype=np.uint64)
    if kind == "a key that returns":
        return (run % np.uint64(2)).astype(U)
    return ((run * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(U)


def _by_key_columns(rng, names):
    """each output column given or NULL, at least one given; vals may be NULL only without sums, mins and maxs"""
    cols = tuple(name for name in names if rng.integers(0, 4))
    cols = cols or (names[int(rng.integers(0, len(names)))],)
    with_vals = bool(set(cols) & {"sums", "mins", "maxs"}) or bool(rng.integers(0, 2))
    return cols, with_vals


RBK_NAMES = ("keys", "counts", "sums", "mins", "maxs")
RBK_CAPACITIES = ("count only", "below", "at", "above")


def reduce_by_key_draws(rng, log_uniform=24):
    for n in sizes(rng, log_uniform, BY_KEY_SEAMS):
        kind = RUN_KINDS[int(rng.integers(0, len(RUN_KINDS)))]
        k = run_keys(rng, n, kind)
        runs = int(rbm.heads(k).size)
        cap_kind = RBK_CAPACITIES[int(rng.integers(0, 4))]
        capacity = {"count only": 0, "below": runs - 1, "at": runs, "above": runs + int(rng.integers(1, 100))}[cap_kind]
        if capacity < 1:
            cap_kind, capacity = "count only", 0
        cols, with_vals = _by_key_columns(rng, RBK_NAMES)
        yield dict(what="reduce_by_key", keys=k, vals=keys(rng, n, int(rng.choice([1, 2, 6, 8, 8]))), run_kind=kind, size=n,
                   signed=bool(rng.integers(0, 2)), capacity=int(capacity), capacity_kind=cap_kind, offs={},
                   cols=cols if capacity else (), with_vals=with_vals or not capacity)


def _by_key_full(case, names, answer, entries, written):
    out = {}
    for name, col in zip(names, answer):
        if name in case["cols"]:
            fill = np.uint64(case["fill"] * 0x100000001) if col.dtype == np.uint64 else U(case["fill"])
            out[name] = np.r_[col[:written], np.full(entries - written, fill, col.dtype)]
    return out


def reduce_by_key_model(case):
    answer = rbm.reduce_by_key(case["keys"], case["vals"], case["signed"])
    runs, cap = int(answer[0].size), case["capacity"]
    res = _by_key_full(case, RBK_NAMES, answer, cap, min(runs, cap))
    return dict(res, runs=runs, status=4 if 0 < cap < runs else 0)  # DBHIP_DEV_TABLE_FULL


SBK_NAMES = sbm.NAMES


def scan_by_key_draws(rng, log_uniform=24):
    for n in sizes(rng, log_uniform, BY_KEY_SEAMS):
        kind = RUN_KINDS[int(rng.integers(0, len(RUN_KINDS)))]
        cols, with_vals = _by_key_columns(rng, SBK_NAMES)
        yield dict(what="scan_by_key", keys=run_keys(rng, n, kind), vals=keys(rng, n, int(rng.choice([1, 2, 6, 8, 8]))),
                   run_kind=kind, size=n, signed=bool(rng.integers(0, 2)), cols=cols, with_vals=with_vals, offs={})


def scan_by_key_model(case):
    answer = sbm.scan_by_key(case["keys"], case["vals"], case["signed"])
    return dict(_by_key_full(case, SBK_NAMES, answer, case["size"], case["size"]), status=0)


# ---- key-value sort and argsort (all four buffers on 16-byte boundaries, as dbhip.h demands) -----------------------------
SORT_SEAMS = (64, 4096, 8192)  # the sizes tests/test_gpu_sort_pairs.py runs every path at


def sort_pairs_draws(rng, log_uniform=24):
    for n in sizes(rng, log_uniform, SORT_SEAMS):
        yield dict(what="sort_pairs", keys=keys(rng, n, int(rng.integers(0, KEY_KINDS))), vals=keys(rng, n, 1), size=n, offs={},
                   signed=bool(rng.integers(0, 2)), argsort=bool(rng.integers(0, 2)), bits=int(rng.choice([4, 8])))


def sort_pairs_model(case):
    k = case["keys"]
    order = np.argsort(k.view(np.int32) if case["signed"] else k, kind="stable")
    return dict(keys=k[order], vals=order.astype(U) if case["argsort"] else case["vals"][order], status=0)


# ---- sorted search (and, through the front door, the range join) ------------------------------------------------------------
SEARCH_SEAMS = tuple(ssm.TOPS)  # fan-out 64 and every allowed top_entries
BOUNDS = ("lo", "lo and hi", "hi")
SEARCH_OUTPUTS = ("pos and cnt", "pos", "cnt")


def sorted_search_draws(rng, log_uniform=14):
    for m in sizes(rng, log_uniform, SEARCH_SEAMS):
        signed = bool(rng.integers(0, 2))
        col = keys(rng, m, int(rng.choice([0, 1, 2, 3, 7, 8])))
        col = col[np.argsort(ssm.flip(col, signed), kind="stable")]
        n = int(rng.choice([0, 1, 3, 4, 5, 63, 64, 65])) if rng.integers(0, 3) == 0 else int(2 ** rng.uniform(0, 14))
        near = col[rng.integers(0, m, n)] if m else u32(rng.integers(0, 1 << 32, n, dtype=np.uint64))
        lo = np.where(rng.random(n) < 0.6, near + u32(rng.integers(0, 3, n)) - U(1), u32(rng.integers(0, 1 << 32, n, dtype=np.uint64)))
        lo[rng.random(n) < 0.05] = EDGES[int(rng.integers(0, EDGES.size))]
        band = rng.choice(np.array([0, 0, 1, 5, 1 << 12, 1 << 28], np.uint64), n)
        xl = ssm.flip(lo, signed).astype(np.uint64)
        xh = np.minimum(xl + band, 0xFFFFFFFF)
        below = rng.random(n) < 0.125  # hi below lo: cnt = 0
        xh[below] = np.maximum(xl[below], 3) - 3
        hi = ssm.flip(xh.astype(U), signed)
        bounds = BOUNDS[int(rng.integers(0, 3))]
        outputs = SEARCH_OUTPUTS[int(rng.integers(0, 3))] if bounds == "lo" else ("pos and cnt", "cnt")[int(rng.integers(0, 2))]
        yield dict(what="sorted_search", sorted=col, lo=None if bounds == "hi" else lo, hi=None if bounds == "lo" else hi,
                   bounds=bounds, outputs=outputs, signed=signed, top=int(rng.choice((0,) + ssm.TOPS)), size=m,
                   offs=dict(sorted=offset(rng)))


def sorted_search_model(case):
    n = (case["lo"] if case["lo"] is not None else case["hi"]).size
    pos, cnt = ssm.search(case["sorted"], case["lo"], case["hi"], case["signed"]) if n else (np.zeros(0, U), np.zeros(0, U))
    res = dict(status=0)
    if "pos" in case["outputs"]:
        res["pos"] = pos
    if "cnt" in case["outputs"]:
        res["cnt"] = cnt
    return res


# ---- join pairs: the answer of a one-to-many join expanded into rows --------------------------------------------------------
PAIR_SEAMS = (64, 2048, 4096)  # the expansion's chunks of 2048 items (dbhip.h); items are probe rows or pairs
PAIR_CAPACITIES = ("count only", "below", "at", "above")
NO_BUILD_ROW = 0xFFFFFFFF


def join_pairs_draws(rng, log_uniform=24):
    """(ids, pos, cnt) as a join of two key columns gives them - ids the stable argsort of the build keys, pos and cnt each
    probe key's range in it - or, once in eight, every probe row matching every build row: a total beyond 2^32"""
    for n_probe in sizes(rng, log_uniform, PAIR_SEAMS, hi_log2=17):
        heavy = n_probe > 1 << 15 and rng.integers(0, 2) == 0 or rng.integers(0, 8) == 0
        n_build = 1 << 17 if heavy else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 16)))
        hi = int(rng.choice([4, 1000, max(n_build, 1), (1 << 32) - 1]))  # (0xFFFFFFFF is the joins' empty key)
        build = u32(rng.integers(0, hi, n_build, dtype=np.uint64))
        probe = u32(rng.integers(0, hi + hi // 2 + 1, n_probe, dtype=np.uint64) % np.uint64((1 << 32) - 1))
        ids = np.argsort(build, kind="stable").astype(U)
        sb = build[ids]
        pos = np.searchsorted(sb, probe, "left").astype(U)
        cnt = (np.searchsorted(sb, probe, "right") - pos).astype(U)
        if heavy:
            pos[:], cnt[:] = 0, n_build
        elif hi == 4 and n_build > 2000:
            cnt = np.minimum(cnt, U(50))  # (a part of each range: still an answer the header defines)
        forged = bool(rng.integers(0, 4) == 0) and n_probe > 0
        if forged:  # ranges that leave the id buffer: they count as empty and raise KEY_RANGE
            at = rng.integers(0, n_probe, 3)
            pos[at], cnt[at] = [max(n_build, 1) - 1, n_build, 0xFFFFFFF0], [2, 1, 0xFFFFFFF0]
        left_outer = bool(rng.integers(0, 2))
        inside = pos.astype(np.uint64) + cnt <= n_build
        e = np.where(inside, cnt, 0).astype(np.uint64)
        total = int(np.maximum(e, 1).sum() if left_outer else e.sum())
        kind = PAIR_CAPACITIES[int(rng.integers(0, 4))]
        room = min(total, 1 << 18)
        capacity = {"count only": 0, "below": int(rng.integers(1, room)) if room > 1 else 0, "at": total,
                    "above": total + int(rng.integers(1, 100))}[kind]
        if total > 1 << 18 and kind in ("at", "above"):
            kind, capacity = "below", int(rng.integers(1, 1 << 16))
        if capacity == 0:
            kind = "count only"
        exact = not heavy and not forged and not (hi == 4 and n_build > 2000)
        yield dict(what="join_pairs", build=build if exact else None, probe=probe, ids=ids, pos=pos, cnt=cnt, rid=u32(rng.permutation(n_probe)) if rng.integers(0, 2) else None,
                   left_outer=left_outer, capacity=int(capacity), capacity_kind=kind, total=total, heavy=bool(total >> 32),
                   forged=forged, size=n_probe,
                   offs={name: offset(rng) for name in ("ids", "pos", "cnt", "rid", "out_build", "out_probe")})


def join_pairs_model(case, total_mask=(1 << 64) - 1, row_zero=False):
    ids, pos, cnt, cap = case["ids"], case["pos"].astype(np.int64), case["cnt"].astype(np.int64), case["capacity"]
    inside = pos + cnt <= ids.size
    e = np.where(inside, cnt, 0)
    per_row = np.maximum(e, 1) if case["left_outer"] else e
    off = np.cumsum(per_row) - per_row
    total = int(per_row.sum())
    rows = np.searchsorted(off + per_row, np.arange(min(cap, total), dtype=np.int64), "right")  # the row of pair number j
    k = np.arange(rows.size, dtype=np.int64) - off[rows]
    hit = e[rows] > 0
    b = np.full(rows.size, NO_BUILD_ROW, U)
    b[hit] = ids[pos[rows[hit]] + k[hit]]
    p = (case["rid"][rows] if case["rid"] is not None else rows).astype(U)
    status = (2 if not inside.all() else 0) | (4 if 0 < cap < total else 0)  # KEY_RANGE, TABLE_FULL
    return dict(out_build=_full(cap, case["fill"], b), out_probe=_full(cap, case["fill"], p), total=total & total_mask,
                status=status)


# ---- the table -----------------------------------------------------------------------------------------------------------
class Operator:
    def __init__(self, name, seed, draws, model, check=None):
        self.name, self.seed, self._draws, self.model, self._check = name, seed, draws, model, check

    def draws(self, rng):
        """the cases, each with the fill word its buffers start as: the two FILLS in turn"""
        for i, case in enumerate(self._draws(rng)):
            case["fill"] = FILLS[i % 2]
            case["draw"] = i
            yield case

    def cases(self, seed=None):
        return self.draws(np.random.default_rng(self.seed if seed is None else seed))

    def check(self, case, result):
        """what the call left behind is what the model leaves behind: outputs, count, status, the entries behind the count"""
        if self._check is not None:
            return self._check(case, result)
        same(case, result, self.model(case))


# the seeds the GPU sweeps use: tests/test_fuzz_draws_host.py asserts that these draw sets hold every category
OPERATORS = {op.name: op for op in (
    Operator("select", 202, select_draws, select_model),
    Operator("merge", 206, merge_draws, merge_model),
    Operator("take", 202, take_draws, take_model),
    Operator("bitpack", 204, bitpack_draws, bitpack_model),
    Operator("sort_pairs", 200, sort_pairs_draws, sort_pairs_model),
    Operator("sorted_search", 200, sorted_search_draws, sorted_search_model),
    Operator("join_pairs", 200, join_pairs_draws, join_pairs_model),
    Operator("topk", 200, topk_draws, topk_model),
    Operator("reduce_by_key", 202, reduce_by_key_draws, reduce_by_key_model),
    Operator("scan_by_key", 200, scan_by_key_draws, scan_by_key_model),
    Operator("dict", 200, dict_draws, dict_model, dict_check),
)}


def draws(name, rng):
    return OPERATORS[name].draws(rng)


def check(name, case, result):
    OPERATORS[name].check(case, result)


# ---- random query plans over the row-id operators ---------------------------------------------------------------------------
PLAN_STEPS = ("select", "refine", "setop", "take", "aggregate", "packed", "dictionary")


def plan_draws(rng, plans=20, max_log2=17):
    """plans of 3 to 6 steps over 2 to 4 columns: the first step selects over all rows, every later one is any of
    PLAN_STEPS on earlier lists.  A step: dict(step, col, list or lists by index, its parameters)"""
    for p in range(plans):
        n = int(2 ** rng.uniform(8, max_log2))
        cols = [keys(rng, n, int(rng.choice([0, 0, 1, 7, 8]))) for _ in range(int(rng.integers(2, 5)))]
        steps, lists = [], 0
        for i in range(int(rng.integers(3, 7))):
            kind = "select" if i == 0 else PLAN_STEPS[int(rng.integers(0, len(PLAN_STEPS)))]
            c = int(rng.integers(0, len(cols)))
            signed, negate = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
            _, lo, hi = interval(rng, cols[c], signed)
            step = dict(step=kind, col=c, signed=signed, negate=negate, lo=lo, hi=hi,
                        list=int(rng.integers(0, max(lists, 1))), other=int(rng.integers(0, max(lists, 1))),
                        op=int(rng.integers(0, 3)), dense=bool(rng.integers(0, 3) == 0))
            steps.append(step)
            lists += kind in ("select", "refine", "setop", "packed")
        yield dict(what="plan", draw=p, n=n, cols=cols, steps=steps)


def plan_model(plan):
    """the plan in numpy -> one answer per step: a row-id list, the taken values, the aggregate's four words, or the
    (codes, decoded values) of the dictionary step"""
    cols, lists, answers = plan["cols"], [], []
    for s in plan["steps"]:
        col, kind = cols[s["col"]], s["step"]
        flags = (sm.SIGNED if s["signed"] else 0) | (sm.NEGATE if s["negate"] else 0)
        if kind == "select" or (kind == "packed" and s["dense"]):
            out = sm.select_range(col, s["lo"], s["hi"], flags)[0]
        elif kind in ("refine", "packed"):
            out = sm.select_range(col, s["lo"], s["hi"], flags, in_rows=lists[s["list"]])[0]
        elif kind == "setop":
            out = mm.setop(s["op"], lists[s["list"]], lists[s["other"]])[0]
        elif kind == "take":
            out = col[lists[s["list"]]]
        elif kind == "aggregate":
            out = tm.aggregate(col, lists[s["list"]], None, tm.SIGNED if s["signed"] else 0)[0]
        else:
            values = col[lists[s["list"]]]
            uniques = dm.ordered(values, dm.SIGNED if s["signed"] else 0)
            out = (dm.encode(uniques, values, None, dm.SIGNED if s["signed"] else 0)[0], values)
        if kind in ("select", "refine", "setop", "packed"):
            lists.append(out)
        answers.append(out)
    return answers


def check_plan(plan, got):
    want = plan_model(plan)
    assert len(got) == len(want)
    for i, (s, g, w) in enumerate(zip(plan["steps"], got, want)):
        what = (plan["draw"], i, s["step"])
        if s["step"] == "aggregate":
            assert tuple(g) == tuple(w), what
        elif s["step"] == "dictionary":
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), what
        else:
            assert g.size == w.size and np.array_equal(g, w), what
