"""The seeded draws of tests/fuzz_testlib.py, checked without a GPU: for the seeds the GPU sweeps use, every operator's
draw set holds every category of every dimension (coverage), the intact model passes check on every draw, and every one
of a list of deliberately defective backends - the model with one defect - is rejected by check on at least one draw
(teeth).  A sweep that passes on the GPU has therefore looked where those defects would show."""
import numpy as np
import pytest

from tests import bitpack_model as bm
from tests import dict_model as dm
from tests import fuzz_testlib as ft
from tests import select_model as sm
from tests import take_model as tm

U = np.uint32
KEY_RANGE = 2
_cache = {}


def cases_of(name):
    if name not in _cache:
        _cache[name] = list(ft.OPERATORS[name].cases())
    return _cache[name]


# ---- coverage --------------------------------------------------------------------------------------------------------
# per kind of call: the seams of its size, the flags drawn both ways, the device counts (field, the capacity's field or
# function), other fields with the values each must take, and whether one draw runs the scan's second round
SEG, TILE, T = ft.sn.SEGMENT_ROWS, ft.bn.TILE_ROWS, ft.T
INTERVALS = ("between", "reversed", "full", "straddle", "point")
SCHEMA = {
    "select": dict(op="select", seams=ft.SELECT_SEAMS, flags=("signed", "negate", "count_only"), second_round=SEG,
                   counts=[("count", lambda c: c["size"])], values=dict(interval=INTERVALS), listed="rows"),
    "setop": dict(op="merge", seams=ft.MERGE_SEAMS, flags=("count_only",), second_round=T,
                  counts=[("a_count", lambda c: c["a"].size), ("b_count", lambda c: c["b"].size)],
                  values=dict(op=(0, 1, 2), share=(0.0, 0.01, 0.5, 0.99, 1.0))),
    "merge": dict(op="merge", seams=ft.MERGE_SEAMS, flags=("signed",),
                  counts=[("a_count", lambda c: c["a"].size), ("b_count", lambda c: c["b"].size)], values=dict(mode=ft.MODES)),
    "take": dict(op="take", seams=ft.TAKE_SEAMS, flags=("outer",), counts=[("count", lambda c: c["size"])],
                 values=dict(n_cols=(1, 2, 3, 4))),
    "aggregate": dict(op="take", seams=ft.TAKE_SEAMS, flags=("outer", "signed"), counts=[("count", lambda c: c["size"])],
                      listed="rows"),
    "pack": dict(op="bitpack", seams=ft.BITPACK_SEAMS, flags=(), counts=[("count", lambda c: c["size"])],
                 values=dict(width=(1, 32))),
    "unpack": dict(op="bitpack", seams=ft.BITPACK_SEAMS, flags=("outer",), counts=[("count", lambda c: c["size"])],
                   values=dict(width=(1, 32)), listed="rows"),
    "sort_pairs": dict(op="sort_pairs", seams=ft.SORT_SEAMS, flags=("signed", "argsort"), counts=[], aligned=True,
                       values=dict(bits=(4, 8))),
    "sorted_search": dict(op="sorted_search", seams=ft.SEARCH_SEAMS, flags=("signed",), counts=[],
                          values=dict(bounds=ft.BOUNDS, outputs=ft.SEARCH_OUTPUTS, top=(0,) + ft.ssm.TOPS)),
    "join_pairs": dict(op="join_pairs", seams=ft.PAIR_SEAMS, flags=("left_outer", "heavy", "forged"), counts=[],
                       values=dict(capacity_kind=ft.PAIR_CAPACITIES), listed="rid"),
    "topk": dict(op="topk", seams=ft.TOPK_SEAMS, flags=("largest", "signed", "sorted"), counts=[], aligned=True,
                 values=dict(k_kind=ft.K_KINDS)),
    "reduce_by_key": dict(op="reduce_by_key", seams=ft.BY_KEY_SEAMS, flags=("signed", "with_vals"), counts=[], aligned=True,
                          values=dict(run_kind=ft.RUN_KINDS, capacity_kind=ft.RBK_CAPACITIES)),
    "scan_by_key": dict(op="scan_by_key", seams=ft.BY_KEY_SEAMS, flags=("signed", "with_vals"), counts=[], aligned=True,
                        values=dict(run_kind=ft.RUN_KINDS)),
    "dict": dict(op="dict", seams=ft.DICT_SEAMS, flags=("signed", "want_misses"),
                 counts=[("count", lambda c: c["size"]), ("probe_count", lambda c: c["probe"].size)],
                 values=dict(capacity_kind=ft.CAPACITY_KINDS)),
    "bitpack select": dict(op="bitpack", what="select", seams=ft.BITPACK_SEAMS, flags=("signed", "negate", "count_only"),
                           second_round=SEG, counts=[("count", lambda c: c["size"])],
                           values=dict(width=(1, 32), interval=INTERVALS), listed="rows"),
}


@pytest.mark.parametrize("kind", sorted(SCHEMA))
def test_the_draws_hold_every_category(kind):
    spec = SCHEMA[kind]
    what = spec.get("what", kind)
    cases = [c for c in cases_of(spec["op"]) if c["what"] == what]
    for c in cases:
        c.setdefault("n_cols", len(c.get("cols", ())))
    sizes = [c["size"] for c in cases]
    for want in [0, 1] + [s + d for s in spec["seams"] for d in (-1, 0, 1)]:
        assert want in sizes, f"no draw of size {want}"
    big = [s for s in sizes if s > ft.MAX_ROWS]
    if "second_round" in spec:  # exactly one draw whose scan runs a second round, on the entries that count
        assert len(big) == 1
        c = cases[sizes.index(big[0])]
        counting = sum(ft.counted(c[field], capacity(c)) for field, capacity in spec["counts"]) if c.get("rows", 1) is not None else big[0]
        assert -(-counting // spec["second_round"]) > ft.SCAN_ROUND
    else:
        assert not big
    buffers = set().union(*(c["offs"] for c in cases))
    assert buffers or spec.get("aligned")  # (the dbhip headers of top-k and the by-key kernels demand 16-byte alignment)
    for name in sorted(buffers):  # every placeable buffer at every offset
        assert {c["offs"][name] for c in cases if name in c["offs"]} == {0, 1, 2, 3}, name
    assert {c["fill"] for c in cases} == set(ft.FILLS)
    for flag in spec["flags"]:
        assert {c[flag] for c in cases} == {False, True}, flag
    for field, capacity in spec["counts"]:
        seen = {ft.count_kind(c[field], capacity(c)) for c in cases if spec.get("listed") is None or c[spec["listed"]] is not None}
        assert seen >= set(ft.COUNT_KINDS), (field, set(ft.COUNT_KINDS) - seen)
    for field, wanted in spec.get("values", {}).items():
        assert {c[field] for c in cases} >= set(wanted), field
    if "listed" in spec:  # over all rows and through a list, with and without row ids outside the column
        assert {c[spec["listed"]] is None for c in cases} == {False, True}


def test_every_draw_is_made_of_independent_dimensions():
    """no placement offset is a function of another (which would leave a pair of them 4 of its 16 values): every pair of
    a call's offsets that 16 draws or more share takes at least 8"""
    for name in ft.OPERATORS:
        by_what = {}
        for c in cases_of(name):
            by_what.setdefault(c["what"], []).append(c)
        for what, cases in by_what.items():
            names = sorted(set().union(*(c["offs"] for c in cases)))
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    pairs = [(c["offs"][a], c["offs"][b]) for c in cases if a in c["offs"] and b in c["offs"]]
                    assert len(pairs) < 16 or len(set(pairs)) >= 8, (what, a, b, len(set(pairs)))


# ---- the intact model passes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ft.OPERATORS))
def test_the_intact_model_passes_every_draw(name):
    op = ft.OPERATORS[name]
    n = 0
    for case in cases_of(name):
        op.check(case, op.model(case))
        n += 1
    assert n == DRAWS[name], n  # the draw counts the summary states


DRAWS = {"sort_pairs": 35, "sorted_search": 43, "join_pairs": 35, "topk": 38, "reduce_by_key": 38, "scan_by_key": 38, "dict": 38, "select": 42, "merge": 65, "take": 70, "bitpack": 124}


# ---- teeth -------------------------------------------------------------------------------------------------------------
def clamp(case, field="count", capacity=None):
    return ft.counted(case[field], case["size"] if capacity is None else capacity)


def cmp32(p, signed):
    return p - (1 << 32) if signed and p >> 31 else p


def widen_interval(case):
    """lo > hi treated as the full range"""
    if cmp32(case["lo"], case["signed"]) > cmp32(case["hi"], case["signed"]):
        return dict(lo=0x80000000 if case["signed"] else 0, hi=0x7FFFFFFF if case["signed"] else 0xFFFFFFFF)
    return {}


def one_more(rows, case, field="count"):
    """the device count is not clamped: the entry behind the list - the guard's fill word - counts too"""
    if rows is not None and case[field] is not None and case[field] > rows.size:
        return np.r_[rows, U(case["fill"])], rows.size + 1
    return rows, case[field]


def candidates(case, n_all):
    return np.arange(n_all, dtype=U) if case["rows"] is None else case["rows"][: clamp(case)]


def behind(result, name, at, room=None):
    """one entry behind the count is written"""
    buf = result[name]
    if at < buf.size:
        buf[at] = 0
    return result


# -- select: a backend is the numpy model on an altered call, its answer laid into the buffers of the real call
def select_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        want, st = sm.select_range(c["col"], c["lo"], c["hi"], c["flags"], c["rows"], c["count"])
        want = want[: case["size"]]
        res = dict(out=ft._full(case["size"], case["fill"], None if case["count_only"] else want), count=int(want.size), status=st)
        return after(case, res) if after else res
    return run


def ragged_last(seg):
    def change(case):
        n_all = case["col"].size if "col" in case else case["n_rows"]
        cand = candidates(case, n_all)
        return dict(rows=cand[:-1] if cand.size % seg else cand, count=None)
    return change


def first_of_unaligned(buffer, n_all=lambda case: case["col"].size):
    def change(case):
        cand = candidates(case, n_all(case))
        return dict(rows=cand[cand != 0] if case["offs"].get(buffer) else cand, count=None)
    return change


def as_row_zero(n_all=lambda case: case["col"].size):
    """a row id outside the column is read as row 0; the status word is still raised"""
    def change(case):
        rows = case["rows"]
        return dict(rows=None if rows is None or not n_all(case) else np.where(rows >= n_all(case), U(0), rows))
    return change


def keep_status(model):
    def after(case, res):
        res["status"] = model(case)["status"]
        return res
    return after


SELECT_DEFECTS = {
    "the device count is ignored": select_backend(lambda c: dict(count=None)),
    "the device count is not clamped": select_backend(lambda c: dict(zip(("rows", "count"), one_more(c["rows"], c)))),
    "signed compared as unsigned": select_backend(lambda c: dict(flags=c["flags"] & ~sm.SIGNED)),
    "negate is ignored": select_backend(lambda c: dict(flags=c["flags"] & ~sm.NEGATE)),
    "lo > hi is the full range": select_backend(widen_interval),
    "the last candidate of a ragged final segment is dropped": select_backend(ragged_last(SEG)),
    "the first element of an unaligned column is dropped": select_backend(first_of_unaligned("col")),
    "a row id outside the column is read as row 0": select_backend(as_row_zero(), keep_status(ft.select_model)),
    "the status word is not raised": select_backend(after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": select_backend(after=lambda c, r: dict(r, status=KEY_RANGE)),
    "one entry behind the count is written": select_backend(after=lambda c, r: behind(r, "out", 0 if c["count_only"] else r["count"])),
}


# -- merge and set operations
def merge_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = ft.merge_model(c)
        real = ft.merge_model(case)
        for name in ("out", "out_keys", "out_vals"):  # laid into the real call's buffers
            if name in res:
                k = min(res["count"], real[name].size) if not case.get("count_only") else 0
                res[name] = ft._full(real[name].size, case["fill"], res[name][:k])
        res["count"] = min(res["count"], real.get("out", real.get("out_keys")).size)
        return after(case, res) if after else res
    return run


def merge_unclamped(case):
    a, ca = one_more(case["a"], case, "a_count")
    b, cb = one_more(case["b"], case, "b_count")
    ch = dict(a=a, b=b, a_count=ca, b_count=cb)
    if case["what"] == "merge":
        ch.update(a_vals=np.r_[case["a_vals"], U(case["fill"])][: a.size], b_vals=np.r_[case["b_vals"], U(case["fill"])][: b.size])
    return ch


def merge_first_of_unaligned(case):
    if not case["offs"]["a"] or not ft.counted(case["a_count"], case["a"].size):
        return {}
    ch = dict(a=case["a"][1:], a_count=None if case["a_count"] is None else max(case["a_count"] - 1, 0))
    if case["what"] == "merge":
        ch["a_vals"] = case["a_vals"][1:]
    return ch


def merge_ragged_last(case, res):
    k = res["count"]
    if k % T:
        res["count"] = k - 1
        for name in ("out", "out_keys", "out_vals"):
            if name in res and not case.get("count_only"):
                res[name][k - 1] = case["fill"]
    return res


def merge_unstable(case, res):
    """the first two neighbours with one key and different values change places"""
    if "out_vals" in res:
        k, keys, vals = res["count"], res["out_keys"], res["out_vals"]
        at = np.flatnonzero((keys[1:k] == keys[: max(k - 1, 0)]) & (vals[1:k] != vals[: max(k - 1, 0)]))
        if at.size:
            vals[[at[0], at[0] + 1]] = vals[[at[0] + 1, at[0]]]
    return res


def merge_behind(case, res):
    for name in ("out", "out_keys", "out_vals"):
        if name in res:
            behind(res, name, 0 if case.get("count_only") else res["count"])
    return res


MERGE_DEFECTS = {
    "the device count is ignored": merge_backend(lambda c: dict(a_count=None, b_count=None)),
    "the device count is not clamped": merge_backend(merge_unclamped),
    "signed compared as unsigned": merge_backend(lambda c: dict(signed=False) if c["what"] == "merge" else {}),
    "the last element of a ragged final tile is dropped": merge_backend(after=merge_ragged_last),
    "the first element of an unaligned column is dropped": merge_backend(merge_first_of_unaligned),
    "the status word is not cleared": merge_backend(after=lambda c, r: dict(r, status=KEY_RANGE)),
    "one entry behind the count is written": merge_backend(after=merge_behind),
    "order among equal keys is unstable": merge_backend(after=merge_unstable),
}
# not listed: "the status word is not raised" - no kernel of this family raises it (merge_model.STATUS)


# -- take and aggregate
def take_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = ft.take_model(dict(c, size=(c["rows"].size if c["rows"] is not None else case["size"])))
        if "outs" in res:  # laid into the real call's buffers
            res["outs"] = [o[: case["size"]].copy() for o in res["outs"]]
        return after(case, res) if after else res
    return run


def take_unclamped(case):
    rows, count = one_more(case["rows"], case)
    return dict(rows=rows, count=count)


def take_ragged_last(case):
    m = clamp(case)
    if case["rows"] is None or not m % ft.tn.SEGMENT_ROWS:
        return {}
    if case["what"] == "take":
        return dict(count=m - 1)  # the entry keeps what the buffer held
    return dict(rows=case["rows"][: m - 1], count=None)


def take_first_of_unaligned(case):
    """column 0 off its boundary: its row 0 reads as another value"""
    if not case["offs"]["col0"] or not case["cols"][0].size:
        return {}
    col = case["cols"][0].copy()
    col[0] ^= U(0x80000001)
    return dict(cols=[col] + list(case["cols"][1:]))


def take_as_row_zero(case):
    rows, n_rows = case["rows"], case["cols"][0].size
    if rows is None or not n_rows:
        return {}
    bad = rows >= n_rows
    if case["outer"]:
        bad &= rows != tm.NO_ROW
    return dict(rows=np.where(bad, U(0), rows))


def take_behind(case, res):
    if "outs" in res:
        res["outs"][-1] = res["outs"][-1].copy()
        m = clamp(case)
        if m < case["size"]:
            res["outs"][-1][m] = 0
    return res


def agg_words(fn):
    def after(case, res):
        if "words" in res:
            res["words"] = tuple(fn(case, list(res["words"])))
        return res
    return after


def unsigned_min_max(case, words):
    if case["signed"] and words[0]:
        plain = tm.aggregate(case["cols"][0], case["rows"], case["count"], case["flags"] & ~tm.SIGNED)[0]
        words[2], words[3] = plain[2], plain[3]
    return words


TAKE_DEFECTS = {
    "the device count is ignored": take_backend(lambda c: dict(count=None)),
    "the device count is not clamped": take_backend(take_unclamped),
    "outer is ignored": take_backend(lambda c: dict(flags=c["flags"] & ~tm.OUTER)),
    "the last entry of a ragged final segment is dropped": take_backend(take_ragged_last),
    "the first element of an unaligned column is dropped": take_backend(take_first_of_unaligned),
    "a row id outside the column is gathered as row 0": take_backend(take_as_row_zero, keep_status(ft.take_model)),
    "the status word is not raised": take_backend(after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": take_backend(after=lambda c, r: dict(r, status=KEY_RANGE)),
    "one entry behind the count is written": take_backend(after=take_behind),
    "sums are truncated to 32 bits": take_backend(after=agg_words(lambda c, w: [w[0], w[1] & 0xFFFFFFFF, w[2], w[3]])),
    "MIN and MAX of signed values are taken unsigned": take_backend(after=agg_words(unsigned_min_max)),
    "signed sums are taken unsigned": take_backend(lambda c: dict(flags=c["flags"] & ~tm.SIGNED) if c["what"] == "aggregate" else {}),
}


# -- bit-packed columns
def straddlers_lose_their_high_part(packed, n_rows, width):
    """every code that lies in two words keeps only the bits in its first word"""
    codes = bm.unpack_codes(packed, n_rows, width)
    first = (np.arange(n_rows, dtype=np.uint64) * np.uint64(width)) % np.uint64(32)
    room = np.minimum(np.uint64(32) - first, np.uint64(width))
    return bm.pack_codes((codes.astype(np.uint64) & ((np.uint64(1) << room) - np.uint64(1))).astype(U), width)


def bitpack_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        if case["what"] != "pack" and c["rows"] is not None:
            c["size"] = c["rows"].size
        res = ft.bitpack_model(c)
        real_size = ft.bitpack_model(case)["out"].size
        out = res["out"][:real_size]
        res["out"] = np.r_[out, np.full(real_size - out.size, case["fill"], U)]
        if "count" in res:
            res["count"] = min(res["count"], case["size"])
        return after(case, res) if after else res
    return run


def bitpack_unclamped(case):
    if case["what"] == "pack":
        col, count = one_more(case["col"], case)
        return dict(col=col, count=count)
    rows, count = one_more(case["rows"], case)
    return dict(rows=rows, count=count)


def bitpack_ragged_last(case):
    m = clamp(case)
    if case["what"] == "pack":
        if not m % TILE:
            return {}
        col = case["col"].copy()
        col[m - 1] = case["base"]  # its code is not stored
        return dict(col=col)
    if case["what"] == "unpack":
        if case["rows"] is None or not m % SEG:
            return {}
        return dict(count=m - 1)
    return ragged_last(SEG)(case)


def bitpack_first_of_unaligned(case):
    if case["what"] == "pack":
        if not case["offs"]["col"] or not case["col"].size:
            return {}
        col = case["col"].copy()
        col[0] = case["base"]
        return dict(col=col)
    if case["what"] == "select" and case["rows"] is not None and case["offs"]["rows"]:
        return dict(rows=case["rows"][: clamp(case)][1:], count=None)
    return {}


def bitpack_as_row_zero(case):
    if case["what"] == "pack" or case["rows"] is None or not case["n_rows"]:
        return {}
    rows = case["rows"]
    bad = rows >= case["n_rows"]
    if case.get("outer"):
        bad &= rows != bm.NO_ROW
    return dict(rows=np.where(bad, U(0), rows))


def bitpack_lossy(case):
    if 32 % case["width"] == 0:
        return {}
    if case["what"] == "pack":
        return {}
    return dict(packed=straddlers_lose_their_high_part(case["packed"], case["n_rows"], case["width"]))


def bitpack_lossy_pack(case, res):
    if case["what"] == "pack" and 32 % case["width"]:
        m = clamp(case)
        w = bm.words(m, case["width"])
        res["out"][:w] = straddlers_lose_their_high_part(res["out"][:w], m, case["width"])
    return res


def bitpack_behind(case, res):
    if case["what"] == "pack":
        return behind(res, "out", bm.words(clamp(case), case["width"]))
    if case["what"] == "unpack":
        return behind(res, "out", clamp(case) if case["rows"] is not None else case["size"])
    return behind(res, "out", 0 if case["count_only"] else res["count"])


def only(what, change):
    return lambda case: change(case) if case["what"] == what else {}


BITPACK_DEFECTS = {
    "the device count is ignored": bitpack_backend(lambda c: dict(count=None)),
    "the device count is not clamped": bitpack_backend(bitpack_unclamped),
    "signed compared as unsigned": bitpack_backend(only("select", lambda c: dict(flags=c["flags"] & ~bm.SIGNED))),
    "negate is ignored": bitpack_backend(only("select", lambda c: dict(flags=c["flags"] & ~bm.NEGATE))),
    "lo > hi is the full range": bitpack_backend(only("select", widen_interval)),
    "outer is ignored": bitpack_backend(only("unpack", lambda c: dict(flags=0))),
    "the last row of a ragged final tile or segment is dropped": bitpack_backend(bitpack_ragged_last),
    "the first element of an unaligned column or list is dropped": bitpack_backend(bitpack_first_of_unaligned),
    "a row id outside the column is read as row 0": bitpack_backend(bitpack_as_row_zero, keep_status(ft.bitpack_model)),
    "the status word is not raised": bitpack_backend(after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": bitpack_backend(after=lambda c, r: dict(r, status=KEY_RANGE)),
    "one entry behind the count is written": bitpack_backend(after=bitpack_behind),
    "a code in two words loses its high part when read": bitpack_backend(bitpack_lossy),
    "a code in two words loses its high part when packed": bitpack_backend(after=bitpack_lossy_pack),
    "base is not added back": bitpack_backend(lambda c: dict(base=0) if c["what"] != "pack" else {}),
    "base is not taken off": bitpack_backend(only("pack", lambda c: dict(base=0))),
}

# -- dictionary encoding
def dict_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = ft.dict_model(c)
        res["keys"] = ft._full(case["capacity"], case["fill"], res["keys"][: min(res["distinct"], case["capacity"])])
        m = min(ft.counted(c["probe_count"], c["probe"].size), case["probe"].size)
        res["codes"] = ft._full(case["probe"].size, case["fill"], res["codes"][:m])
        return after(case, res) if after else res
    return run


def dict_unclamped(case):
    col, count = one_more(case["col"], case)
    probe, probe_count = one_more(case["probe"], case, "probe_count")
    return dict(col=col, count=count, probe=probe, probe_count=probe_count)


def dict_first_of_unaligned(case):
    ch = {}
    if case["offs"]["col"] and ft.counted(case["count"], case["size"]):
        ch.update(col=case["col"][1:], count=None if case["count"] is None else case["count"] - 1)
    return ch


def dict_ragged_last(case, res):
    m = ft.counted(case["probe_count"], case["probe"].size)
    if m % ft.ENCODE_TILE:
        res["codes"][m - 1] = case["fill"]
    return res


def dict_miss_is_zero(case, res):
    m = ft.counted(case["probe_count"], case["probe"].size)
    res["codes"][:m][res["codes"][:m] == dm.MISS] = 0
    return res


def dict_misses_off(case, res):
    if res["misses"] is not None:
        res["misses"] = int((res["codes"][: ft.counted(case["probe_count"], case["probe"].size)] == dm.MISS).sum()) + 1
    return res


def dict_full_table_writes_keys(case, res):
    if res["status"] == dm.TABLE_FULL:
        res["keys"][0] = 0
    return res


DICT_DEFECTS = {
    "the device count is ignored": dict_backend(lambda c: dict(count=None)),
    "the probe's device count is ignored": dict_backend(lambda c: dict(probe_count=None)),
    "the device count is not clamped": dict_backend(dict_unclamped),
    "signed compared as unsigned": dict_backend(lambda c: dict(flags=0)),
    "the first element of an unaligned column is dropped": dict_backend(dict_first_of_unaligned),
    "the last row of a ragged final tile is not encoded": dict_backend(after=dict_ragged_last),
    "the status word is not raised": dict_backend(after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": dict_backend(after=lambda c, r: dict(r, status=dm.TABLE_FULL)),
    "one entry behind the count is written": dict_backend(
        after=lambda c, r: behind(r, "codes", ft.counted(c["probe_count"], c["probe"].size))),
    "a dictionary miss is encoded as code 0": dict_backend(after=dict_miss_is_zero),
    "the number of misses is off by one": dict_backend(after=dict_misses_off),
    "a full table still writes a key": dict_backend(after=dict_full_table_writes_keys),
    "the capacity is taken one too large": dict_backend(lambda c: dict(capacity=c["capacity"] + 1)),
    "the capacity is taken one too small": dict_backend(lambda c: dict(capacity=max(c["capacity"] - 1, 1))),
}

# -- top-k
def topk_backend(change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = ft.topk_model(c)
        for name in ("out_keys", "out_rows"):
            res[name] = ft._full(case["k"], case["fill"], res[name][: min(c["k"], c["keys"].size, case["k"])])
        return after(case, res) if after else res
    return run


def topk_unstable(case, res):
    """the first two neighbours of a sorted answer with one key change places"""
    m = min(case["k"], case["size"])
    if case["sorted"]:
        at = np.flatnonzero(res["out_keys"][1:m] == res["out_keys"][: max(m - 1, 0)])
        if at.size:
            res["out_rows"][[at[0], at[0] + 1]] = res["out_rows"][[at[0] + 1, at[0]]]
    return res


def topk_ties_by_descending_row(case):
    """among rows equal to the k-th key the LAST ones are taken"""
    n = case["size"]
    return dict(keys=case["keys"][::-1].copy(), _mirror=n)


def topk_mirrored(case, res):
    m, n = min(case["k"], case["size"]), case["size"]
    rows = (n - 1 - res["out_rows"][:m].astype(np.int64)).astype(U)
    order = np.argsort(rows, kind="stable") if not case["sorted"] else np.arange(m)
    res["out_rows"][:m], res["out_keys"][:m] = rows[order], res["out_keys"][:m][order]
    return res


TOPK_DEFECTS = {
    "signed compared as unsigned": topk_backend(lambda c: dict(signed=False)),
    "largest is ignored": topk_backend(lambda c: dict(largest=False)),
    "sorted is ignored": topk_backend(lambda c: dict(sorted=True)),
    "the last row of a ragged final segment is dropped": topk_backend(
        lambda c: dict(keys=c["keys"][:-1]) if c["size"] % ft.S else {}),
    "the status word is not cleared": topk_backend(after=lambda c, r: dict(r, status=KEY_RANGE)),
    "one entry behind the count is written": topk_backend(after=lambda c, r: behind(r, "out_rows", min(c["k"], c["size"]))),
    "order among equal keys is unstable": topk_backend(after=topk_unstable),
    "ties at the k-th key are taken from the back": topk_backend(topk_ties_by_descending_row, topk_mirrored),
    "k is taken one too small": topk_backend(lambda c: dict(k=max(c["k"] - 1, 0))),
}


# -- the by-key operators
def split_at_segments(keys):
    """keys whose runs also end where a 4096-row segment ends: a run is split at the segment boundary"""
    heads = ft.sbm.head_flags(keys)
    heads[:: ft.S] = True
    return np.cumsum(heads).astype(U)


def by_key_backend(model, names, change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = model(c)
        if c["keys"] is not case["keys"] and "keys" in res:  # the output keys are the real ones
            heads = ft.rbm.heads(c["keys"])[: case["capacity"]]
            res["keys"] = ft._full(case["capacity"], case["fill"], case["keys"][heads])
        return after(case, res) if after else res
    return run


def narrow_sums(case, res):
    if "sums" in res:
        written = min(res.get("runs", case["size"]), case.get("capacity", case["size"]))
        res["sums"] = res["sums"].copy()
        res["sums"][:written] &= np.uint64(0xFFFFFFFF)
    return res


def unsigned_extremes(model):
    def after(case, res):
        if case["signed"]:
            plain = model(dict(case, signed=False))
            for name in ("mins", "maxs"):
                if name in res:
                    res[name] = plain[name]
        return res
    return after


def drop_last_row(case):
    return dict(keys=case["keys"][:-1], vals=case["vals"][:-1]) if case["size"] % ft.S else {}


def rbk_behind(case, res):
    written = min(res["runs"], case["capacity"])
    for name in case["cols"]:
        if written < case["capacity"]:
            res[name] = res[name].copy()
            res[name][written] = 0
    return res


RBK = (ft.reduce_by_key_model, ft.RBK_NAMES)
RBK_DEFECTS = {
    "a run is split at a segment boundary": by_key_backend(*RBK, lambda c: dict(keys=split_at_segments(c["keys"]))),
    "sums are truncated to 32 bits": by_key_backend(*RBK, after=narrow_sums),
    "signed sums are taken unsigned": by_key_backend(*RBK, after=lambda c, r: dict(
        r, **({"sums": ft.reduce_by_key_model(dict(c, signed=False))["sums"]} if "sums" in r else {}))),
    "MIN and MAX of signed values are taken unsigned": by_key_backend(*RBK, after=unsigned_extremes(ft.reduce_by_key_model)),
    "the last row of a ragged final segment is dropped": by_key_backend(*RBK, drop_last_row),
    "the status word is not raised": by_key_backend(*RBK, after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": by_key_backend(*RBK, after=lambda c, r: dict(r, status=4)),
    "one entry behind the count is written": by_key_backend(*RBK, after=rbk_behind),
    "the number of runs stops at the capacity": by_key_backend(
        *RBK, after=lambda c, r: dict(r, runs=min(r["runs"], c["capacity"]) if c["capacity"] else r["runs"])),
    "the run at the capacity is written too": by_key_backend(*RBK, lambda c: dict(capacity=c["capacity"] + 1) if c["capacity"] else {},
                                                            lambda c, r: {k: (v[: c["capacity"]] if isinstance(v, np.ndarray) else v)
                                                                          for k, v in r.items()}),
}


def sbk_last_row_unwritten(case, res):
    if case["size"] % ft.S:
        for name in case["cols"]:
            res[name] = res[name].copy()
            res[name][-1] = np.uint64(case["fill"] * 0x100000001) if res[name].dtype == np.uint64 else U(case["fill"])
    return res


SBK = (ft.scan_by_key_model, ft.SBK_NAMES)
SBK_DEFECTS = {
    "a run is split at a segment boundary": by_key_backend(*SBK, lambda c: dict(keys=split_at_segments(c["keys"]))),
    "sums are truncated to 32 bits": by_key_backend(*SBK, after=narrow_sums),
    "MIN and MAX of signed values are taken unsigned": by_key_backend(*SBK, after=unsigned_extremes(ft.scan_by_key_model)),
    "signed sums are taken unsigned": by_key_backend(*SBK, after=lambda c, r: dict(
        r, **({"sums": ft.scan_by_key_model(dict(c, signed=False))["sums"]} if "sums" in r else {}))),
    "the last row of a ragged final segment is not written": by_key_backend(*SBK, after=sbk_last_row_unwritten),
    "the status word is not cleared": by_key_backend(*SBK, after=lambda c, r: dict(r, status=KEY_RANGE)),
    "row numbers start at 0": by_key_backend(*SBK, after=lambda c, r: dict(
        r, **({"row_numbers": r["row_numbers"] - U(1)} if "row_numbers" in r else {}))),
}

# -- key-value sort, sorted search, join pairs
def after_model(model, change=None, after=None):
    def run(case):
        c = dict(case)
        if change:
            c.update(change(case))
        res = model(c)
        return after(case, res) if after else res
    return run


def sort_unstable(case, res):
    at = np.flatnonzero((res["keys"][1:] == res["keys"][:-1]) & (res["vals"][1:] != res["vals"][:-1]))
    if at.size:
        res["vals"][[at[0], at[0] + 1]] = res["vals"][[at[0] + 1, at[0]]]
    return res


def sort_last_row_stays(case, res):
    """the last row of a ragged final tile is left where it was"""
    if case["size"] % 64 and case["size"] > 1:
        head = ft.sort_pairs_model(dict(case, keys=case["keys"][:-1], vals=case["vals"][:-1]))
        last = U(case["size"] - 1) if case["argsort"] else case["vals"][-1]
        res = dict(res, keys=np.r_[head["keys"], case["keys"][-1]], vals=np.r_[head["vals"], last])
    return res


SORT_PAIRS_DEFECTS = {
    "signed compared as unsigned": after_model(ft.sort_pairs_model, lambda c: dict(signed=False)),
    "order among equal keys is unstable": after_model(ft.sort_pairs_model, after=sort_unstable),
    "the values stay behind": after_model(ft.sort_pairs_model, after=lambda c, r: dict(r, vals=r["vals"] if c["argsort"] else c["vals"])),
    "the last row of a ragged final tile stays": after_model(ft.sort_pairs_model, after=sort_last_row_stays),
    "the top digit is skipped": after_model(ft.sort_pairs_model, lambda c: dict(keys=c["keys"] & U(0x00FFFFFF)),
                                            lambda c, r: dict(r, keys=np.sort(c["keys"].view(np.int32) if c["signed"] else c["keys"]).view(U))),
    "the status word is not cleared": after_model(ft.sort_pairs_model, after=lambda c, r: dict(r, status=KEY_RANGE)),
}


def search_upper_for_lower(case, res):
    """pos is U(lo), the number of entries <= lo, where L(lo) is asked"""
    if "pos" in res and case["lo"] is not None:
        s = ft.ssm.flip(case["sorted"], case["signed"])
        res["pos"] = np.searchsorted(s, ft.ssm.flip(case["lo"], case["signed"]), side="right").astype(U)
    return res


def search_wrapping_count(case, res):
    """hi below lo: cnt is end - pos mod 2^32, not 0"""
    if "cnt" in res and case["lo"] is not None:
        s = ft.ssm.flip(case["sorted"], case["signed"])
        pos = np.searchsorted(s, ft.ssm.flip(case["lo"], case["signed"]), side="left")
        end = np.searchsorted(s, ft.ssm.flip(case["hi"] if case["hi"] is not None else case["lo"], case["signed"]), side="right")
        res["cnt"] = (end - pos).astype(np.int64).astype(U)
    return res


def search_without_first(case):
    return dict(sorted=case["sorted"][1:]) if case["offs"]["sorted"] and case["size"] else {}


SEARCH_DEFECTS = {
    "an upper bound is returned for a lower bound": after_model(ft.sorted_search_model, after=search_upper_for_lower),
    "signed compared as unsigned": after_model(ft.sorted_search_model, lambda c: dict(
        signed=False, sorted=np.sort(c["sorted"])) if c["signed"] else {}),
    "hi below lo gives a wrapped count": after_model(ft.sorted_search_model, after=search_wrapping_count),
    "hi is ignored": after_model(ft.sorted_search_model, lambda c: dict(hi=None) if c["lo"] is not None else {}),
    "lo is ignored": after_model(ft.sorted_search_model, lambda c: dict(lo=None) if c["hi"] is not None else {}),
    "the first element of an unaligned column is dropped": after_model(ft.sorted_search_model, search_without_first),
    "the last entry of a ragged final block is dropped": after_model(
        ft.sorted_search_model, lambda c: dict(sorted=c["sorted"][:-1]) if c["size"] % ft.ssm.FANOUT else {}),
    "the status word is not cleared": after_model(ft.sorted_search_model, after=lambda c, r: dict(r, status=KEY_RANGE)),
}


def pairs_behind(case, res):
    written = min(case["capacity"], case["total"])
    if written < case["capacity"]:
        res["out_probe"][written] = 0
    return res


def pairs_overrun(case, res):
    """the pair numbered `capacity` is written too: seen as one entry less room"""
    if 0 < case["capacity"] <= case["total"]:
        res["out_build"][-1] = res["out_build"][-1] ^ U(1)
    return res


def pairs_first_of_unaligned(case):
    if case["offs"]["cnt"] and case["size"]:
        cnt = case["cnt"].copy()
        cnt[0] = 0
        return dict(cnt=cnt)
    return {}


def pairs_range_as_zero(case):
    """a range that leaves the id buffer is read from id 0 on (the status word is still raised)"""
    bad = case["pos"].astype(np.int64) + case["cnt"] > case["ids"].size
    if not bad.any() or not case["ids"].size:
        return {}
    pos, cnt = case["pos"].copy(), case["cnt"].copy()
    pos[bad], cnt[bad] = 0, 1
    return dict(pos=pos, cnt=cnt)


JP = ft.join_pairs_model
JOIN_PAIRS_DEFECTS = {
    "pair totals are truncated to 32 bits": lambda c: JP(c, total_mask=0xFFFFFFFF),
    "left_outer is ignored": after_model(JP, lambda c: dict(left_outer=False)),
    "the probe row ids are ignored": after_model(JP, lambda c: dict(rid=None)),
    "the status word is not raised": after_model(JP, after=lambda c, r: dict(r, status=0)),
    "the status word is not cleared": after_model(JP, after=lambda c, r: dict(r, status=r["status"] | 4)),
    "one entry behind the count is written": after_model(JP, after=pairs_behind),
    "the last pair below the capacity is wrong": after_model(JP, after=pairs_overrun),
    "the first element of an unaligned column is dropped": after_model(JP, pairs_first_of_unaligned),
    "a range outside the id buffer is read from id 0": after_model(JP, pairs_range_as_zero, keep_status(JP)),
    "the total stops at the capacity": after_model(JP, after=lambda c, r: dict(
        r, total=min(r["total"], c["capacity"]) if c["capacity"] else r["total"])),
    "the last row of a ragged final chunk is dropped": after_model(
        JP, lambda c: dict(cnt=np.r_[c["cnt"][:-1], U(0)]) if c["size"] % 2048 else {}),
}

DEFECTS = {"sort_pairs": SORT_PAIRS_DEFECTS, "sorted_search": SEARCH_DEFECTS, "join_pairs": JOIN_PAIRS_DEFECTS,
           "topk": TOPK_DEFECTS, "reduce_by_key": RBK_DEFECTS, "scan_by_key": SBK_DEFECTS, "dict": DICT_DEFECTS, "select": SELECT_DEFECTS, "merge": MERGE_DEFECTS, "take": TAKE_DEFECTS, "bitpack": BITPACK_DEFECTS}
# per defect, the kinds of call that must each reject it (None: any one)
MUST_REJECT = {
    ("merge", "the device count is ignored"): ("setop", "merge"),
    ("merge", "the device count is not clamped"): ("setop", "merge"),
    ("merge", "the last element of a ragged final tile is dropped"): ("setop", "merge"),
    ("merge", "the first element of an unaligned column is dropped"): ("setop", "merge"),
    ("merge", "one entry behind the count is written"): ("setop", "merge"),
    ("take", "the device count is ignored"): ("take", "aggregate"),
    ("take", "the device count is not clamped"): ("take", "aggregate"),
    ("take", "a row id outside the column is gathered as row 0"): ("take", "aggregate"),
    ("take", "the last entry of a ragged final segment is dropped"): ("take", "aggregate"),
    ("bitpack", "the device count is ignored"): ("pack", "unpack", "select"),
    ("bitpack", "the device count is not clamped"): ("pack", "unpack", "select"),
    ("bitpack", "the last row of a ragged final tile or segment is dropped"): ("pack", "unpack", "select"),
    ("bitpack", "a row id outside the column is read as row 0"): ("unpack", "select"),
    ("bitpack", "one entry behind the count is written"): ("pack", "unpack", "select"),
    ("bitpack", "a code in two words loses its high part when read"): ("unpack", "select"),
    ("bitpack", "base is not added back"): ("unpack", "select"),
    ("bitpack", "the status word is not raised"): ("pack", "unpack", "select"),
}


def first_rejections(name, defect, backend):
    """-> {kind of call: the first draw on which check rejects the defective backend}"""
    op, caught = ft.OPERATORS[name], {}
    need = MUST_REJECT.get((name, defect))
    for case in cases_of(name):
        if case["what"] in caught or case["size"] > ft.MAX_ROWS:
            continue
        try:
            op.check(case, backend(case))
        except AssertionError:
            caught[case["what"]] = case["draw"]
            if need is None or all(w in caught for w in need):
                break
    return caught


@pytest.mark.parametrize("name,defect", [(n, d) for n in sorted(DEFECTS) for d in DEFECTS[n]])
def test_every_defect_is_rejected_by_some_draw(name, defect):
    caught = first_rejections(name, defect, DEFECTS[name][defect])
    need = MUST_REJECT.get((name, defect))
    print(f"{name}: {defect}: rejected on draw {caught}")
    if need is None:
        assert caught, "no draw rejects this defect"
    else:
        assert all(w in caught for w in need), f"not rejected by {[w for w in need if w not in caught]}"


def test_removing_a_dimension_is_noticed():
    """with every offset fixed at 0 the coverage no longer holds and the defects of unaligned columns go unnoticed"""
    flat = []
    for case in cases_of("select"):
        flat.append(dict(case, offs={k: 0 for k in case["offs"]}))
    op = ft.OPERATORS["select"]
    backend = SELECT_DEFECTS["the first element of an unaligned column is dropped"]
    for case in flat:
        op.check(case, backend(case))  # never rejected: the sweep would have no teeth for it
    assert {c["offs"]["col"] for c in flat} != {0, 1, 2, 3}


def test_the_query_plans_hold_every_step_and_their_check_has_teeth():
    """the twenty plans of the GPU test: 3 to 6 steps, 2 to 4 columns, every kind of step; the numpy answers pass, and one
    wrong entry, one missing entry or one wrong aggregate word in any step is rejected"""
    plans = list(ft.plan_draws(np.random.default_rng(211)))
    assert len(plans) == 20 and {s["step"] for p in plans for s in p["steps"]} == set(ft.PLAN_STEPS)
    seen = set()
    for plan in plans:
        assert 3 <= len(plan["steps"]) <= 6 and 2 <= len(plan["cols"]) <= 4 and plan["n"] <= 1 << 17
        want = ft.plan_model(plan)
        ft.check_plan(plan, want)
        for i, step in enumerate(plan["steps"]):
            wrong = list(want)
            if step["step"] == "aggregate":
                wrong[i] = (want[i][0], want[i][1] ^ (1 << 40), want[i][2], want[i][3])
            elif step["step"] == "dictionary":
                if not want[i][0].size:
                    continue
                wrong[i] = (want[i][0], np.r_[want[i][1][:-1], want[i][1][-1] ^ U(1)])
            elif want[i].size:
                wrong[i] = want[i][:-1]
            else:
                wrong[i] = np.zeros(1, U)
            with pytest.raises(AssertionError):
                ft.check_plan(plan, wrong)
            seen.add(step["step"])
    assert seen == set(ft.PLAN_STEPS)


def defects_document():
    """tests/FUZZ_DEFECTS.md: every defective backend with the first draw that rejects it"""
    lines = ["# Defective backends and the draws that reject them", "",
             "What `tests/test_fuzz_draws_host.py` asserts, written out: per operator of `tests/fuzz_testlib.py` its seed and number",
             "of draws, and for every defective backend (the numpy model with one defect) the first draw of the seeded set on which",
             "`check` rejects it, per kind of call.  `pytest tests/test_fuzz_draws_host.py -s` prints the same.", ""]
    for name in ft.OPERATORS:
        lines += [f"## {name} (seed {ft.OPERATORS[name].seed}, {len(cases_of(name))} draws)", ""]
        for defect, backend in DEFECTS[name].items():
            caught = first_rejections(name, defect, backend)
            lines.append(f"- {defect}: " + ", ".join(f"{w} draw {d}" for w, d in caught.items()))
        lines.append("")
    return lines


def test_the_written_list_of_defects_is_the_one_asserted():
    from pathlib import Path
    written = (Path(__file__).resolve().parent / "FUZZ_DEFECTS.md").read_text().split("\n## Not listed")[0].rstrip("\n")
    assert written == "\n".join(defects_document()).rstrip("\n")
