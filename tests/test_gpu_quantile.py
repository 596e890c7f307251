"""The quantile select on the GPU (dwarf_bench_amd/host/quantile_select.cpp through quantile_native): the raw entry point on
guarded buffers (tests/guard_testlib.py), the three output columns and the status word compared bit for bit with the numpy
model (tests/quantile_model.py).  The column and the list sit at offsets 0 .. 3 from a 16-byte boundary, guard words surround
the outputs, every input and the workspace, the workspace holds junk beforehand, and every case runs under both fill words: a
kernel that reads past an end and counts what it read answers differently under the two."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from dwarf_bench_amd import quantile_native as qn
from tests import quantile_model as qm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

ROUND = 8192  # positions of one round of a histogram workgroup
ROW_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 1, 65549)
BIG = (1 << 22) + 5  # 513 rounds of 8192 (257 of 16384 with sixteen slots): the persistent grids at their full size of two
#                      workgroups to a CU (one with sixteen slots), some workgroups taking a round more than the others
KINDS = ("equal", "two values", "low 10", "middle 11", "top 11", "dense", "reference", "random", "corners")
COUNTS = ("none", "zero", "one", "below", "at", "above", "huge")
U = np.uint32
TOP = (1 << 32) - 1


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_keys(n, kind, rng_seed=1):
    rng = np.random.default_rng(rng_seed + 31 * n)
    if kind == "equal":
        return np.full(n, 0xC0FFEE11, U)
    if kind == "two values":
        return np.array([0x12345678, 0x12345679], U)[rng.integers(0, 2, n)]
    if kind == "low 10":  # keys that differ only in the last level's digit
        return U(0xABCDE000) | rng.integers(0, 1 << 10, n).astype(U)
    if kind == "middle 11":
        return U(0x7FE00155) | (rng.integers(0, 1 << 11, n).astype(U) << U(10))
    if kind == "top 11":
        return U(0x000AB155) | (rng.integers(0, 1 << 11, n).astype(U) << U(21))
    if kind == "dense":
        return rng.permutation(np.arange(1, n + 1, dtype=U))
    if kind == "reference":
        return rng.integers(1, 10001, n).astype(U)
    if kind == "corners":
        return np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], U)[rng.integers(0, 4, n)]
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)


def rank_sets(m):
    """name -> (q_num, q_den) lists for a call over m candidates"""
    last = max(m - 1, 0)
    sets = {
        "first": [(0, 0)], "last": [(last, 0)], "lower median": [(1, 2)],
        "the same rank twice": [(m // 3, 0), (m // 3, 0)],
        "neighbours": [(m // 2, 0), (min(m // 2 + 1, last), 0)],
        "sixteen spread": [(i, 17) for i in range(1, 17)],
        "sixteen adjacent": [(min(m // 2 + i, last), 0) for i in range(16)],
        "no such row next to valid ones": [(0, 0), (m, 0), (1, 1), (TOP, 0), (1, 2)],
        "descending": [(1, 1), (3, 4), (1, 2), (1, 4), (0, 1)],
        "deciles": [(i, 10) for i in range(1, 10)],
    }
    return {name: ([q[0] for q in qs], [q[1] for q in qs]) for name, qs in sets.items()}


def count_of(kind, capacity):
    return {"none": None, "zero": 0, "one": 1, "below": capacity // 2 + 1, "at": capacity, "above": capacity + 1,
            "huge": (1 << 40) + 9}[kind]


def _p(t):
    return ptr(t) if t is not None else None


def call(col, num, den, flags=0, rows=None, count=None, col_off=0, list_off=0, out_offs=(1, 2, 3), fill=FILLS[0], ws_byte=0xC3):
    """one dbench_quantile_select_u32 on guarded buffers -> (values, below, equal, status)"""
    w = Watch(fill)
    n_col, n_q = col.size, len(num)
    d_col = w.col(n_col, col_off, data=col, freeze=True)
    d_rows = w.col(rows.size, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = None
    if count is not None:
        d_count = w.u64(1)
        d_count.fill_(count)
        w.freeze(d_count)
    outs = [w.col(n_q, off) for off in out_offs]
    nbytes = qn.workspace_bytes(n_q)
    ws = w.ws(nbytes)
    ws.fill_(ws_byte)
    rc = qn.select(ptr(d_col) if n_col else None, n_col, _p(d_rows), _p(d_count), rows.size if rows is not None else 0, num, den,
                   flags, *(ptr(o) for o in outs), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return tuple(o.cpu().numpy().view(U).copy() for o in outs) + (st,)


def same(got, want, what=""):
    for name, g, w_ in zip(("values", "below", "equal"), got, want):
        assert np.array_equal(g, w_), (what, name, [hex(int(v)) for v in g], [hex(int(v)) for v in w_])
    assert got[3] == want[3], (what, got[3], want[3])


def expect(col, num, den, flags=0, rows=None, count=None, what="", fills=FILLS, **how):
    """the call under both fill words, each bit for bit the model's -> the model's answer"""
    want = qm.select(col, num, den, flags, rows, count)
    for i, fill in enumerate(fills):
        same(call(col, num, den, flags, rows, count, fill=fill, ws_byte=(0xC3, 0x00, 0xFF)[i % 3], **how), want, what)
    return want


# ---- all rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_off", range(4))
def test_every_row_count_at_every_column_offset(col_off):
    for i, n in enumerate(ROW_COUNTS):
        kind = KINDS[(i + 2 * col_off) % len(KINDS)]
        sets = rank_sets(n)
        name = list(sets)[(i + col_off) % len(sets)]
        num, den = sets[name]
        values, below, equal, st = expect(make_keys(n, kind), num, den, flags=(i + col_off) % 2, col_off=col_off,
                                          out_offs=[(col_off + j) % 4 for j in (1, 2, 3)], what=(n, kind, name))
        assert st == 0 and (n > 0 or (not equal.any() and not values.any() and not below.any()))


@pytest.mark.parametrize("kind", KINDS)
def test_every_key_kind_under_every_rank_set(kind):
    n = 2 * ROUND + 1
    col = make_keys(n, kind)
    for i, (name, (num, den)) in enumerate(rank_sets(n).items()):
        for signed in ((0, 1) if kind in ("corners", "random") else (i % 2,)):
            values, below, equal, _ = expect(col, num, den, flags=signed, col_off=i % 4, what=(kind, name, signed))
            live = equal > 0
            x = values[live] ^ U(0x80000000 if signed else 0)
            digits = [len(set((x >> U(s)).tolist())) for s in (21, 10, 0)]  # distinct prefixes after each level
            if name == "sixteen spread":  # what the slots of levels 1 and 2 hold
                if kind == "top 11":
                    assert digits == [16, 16, 16]       # sixteen different top bins: every slot live from level 1 on
                elif kind == "middle 11":
                    assert digits == [1, 16, 16]        # one level-0 bin, sixteen level-1 bins
                elif kind == "low 10":
                    assert digits == [1, 1, 16]         # both shared: the last digit alone tells them apart
                elif kind == "equal":
                    assert digits == [1, 1, 1]          # sixteen ranks, one value
            if kind == "two values":  # neighbouring ranks share a value; both values share all but the last digit
                assert digits == ([1, 1, 1] if name == "neighbours" else [1, 1, 2] if name == "descending" else digits)
            if name == "the same rank twice":
                assert values[0] == values[1] and below[0] == below[1]
            if name == "no such row next to valid ones":
                assert live.tolist() == [True, False, True, False, True] and below[1] == n == below[3]
    if kind == "corners":  # the two orders disagree about where 0x80000000 lies
        lo_u = qm.select(col, [0], [0], 0)[0][0]
        lo_s = qm.select(col, [0], [0], qm.SIGNED)[0][0]
        assert (lo_u, lo_s) == (0, 0x80000000)


@pytest.mark.parametrize("n_q", (1, 3, 16))
def test_the_full_grid_with_several_rounds_per_workgroup(n_q):
    assert (BIG + ROUND - 1) // ROUND == 513
    col = np.random.default_rng(n_q).integers(0, 1 << 32, BIG, dtype=np.uint64).astype(U)
    if n_q == 16:
        col[::3] &= U(0x001FFFFF)  # a third of the rows under one top digit: ranks that share a level-0 bin
    num, den = [(1,), (1, 999, 0), tuple(range(1, 17))][(1, 3, 16).index(n_q)], [(2,), (4, 1000, 1), (17,) * 16][(1, 3, 16).index(n_q)]
    values, below, equal, st = expect(col, num, den, col_off=n_q % 4, fills=FILLS[:1], what=n_q)
    assert st == 0 and equal.all()


@pytest.mark.parametrize("listed", (False, True))
def test_every_kind_of_device_count(listed):
    n = ROUND + 301
    col = make_keys(n, "random")
    rows = np.random.default_rng(3).permutation(n).astype(U) if listed else None
    num, den = [1, 0, 1, 5], [2, 0, 1, 0]
    got = {}
    for kind in COUNTS:
        got[kind] = expect(col, num, den, rows=rows, count=count_of(kind, n), col_off=1, list_off=2, what=kind)
    assert not got["zero"][2].any() and all(np.array_equal(a, b) for a, b in zip(got["none"], got["huge"]))
    assert all(np.array_equal(a, b) for a, b in zip(got["at"], got["above"])) and not np.array_equal(got["below"][0], got["at"][0])
    assert got["one"][2].tolist() == [1, 1, 1, 0] and got["one"][1].tolist() == [0, 0, 0, 1]


# ---- lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("list_off", range(4))
def test_lists_sorted_shuffled_repeated_and_with_bad_ids(list_off):
    rng = np.random.default_rng(8 + list_off)
    n_col = 3000
    for i, m in enumerate((1, 5, 257, ROUND + 1, 2 * ROUND + 1)):
        col = make_keys(n_col, KINDS[(i + list_off) % len(KINDS)], rng_seed=i)
        num, den = list(rank_sets(m).values())[(3 * i + list_off) % 10]
        shuffled = rng.integers(0, n_col // 3, m).astype(U)  # unsorted, rows repeat, most rows never named
        for rows in (np.sort(shuffled), shuffled):
            expect(col, num, den, flags=i % 2, rows=rows, list_off=list_off, col_off=(i + 1) % 4, what=(m, "list"))
        bad = shuffled.copy()
        at = rng.integers(0, m, max(m // 40, 1))
        bad[at] = np.array([n_col, n_col + 1, 0x80000000, 0xFFFFFFFF], U)[rng.integers(0, 4, at.size)]
        want = expect(col, num, den, flags=i % 2, rows=bad, list_off=list_off, col_off=i % 4, what=(m, "bad ids"))
        assert want[3] == qm.KEY_RANGE  # raised, and those ids are no candidates:
        same(want, qm.select(col, num, den, i % 2, rows=bad[bad < n_col])[:3] + (qm.KEY_RANGE,))
        # behind the count the list may hold anything without a status
        behind = np.r_[shuffled, np.full(9, 0xFFFFFFFF, U)]
        assert expect(col, num, den, rows=behind, count=m, list_off=list_off, what=(m, "behind"))[3] == 0
    values, below, equal, st = expect(np.zeros(0, U), [0, 1], [0, 2], rows=np.array([0, 1, 2], U), list_off=list_off)
    assert st == qm.KEY_RANGE and not equal.any() and not below.any()  # an empty column: every id is outside it


def test_a_stale_workspace_and_repeated_calls_change_nothing():
    col = make_keys(3 * ROUND + 77, "reference")
    num, den = rank_sets(col.size)["deciles"]
    first = call(col, num, den)
    same(first, qm.select(col, num, den))
    for ws_byte in (0x00, 0xFF, 0x5A, 0x02):
        same(call(col, num, den, ws_byte=ws_byte, fill=FILLS[1]), first, ws_byte)
    rows = np.array([5, col.size, 7], U)  # a flagged call's status does not survive the next call on the same bytes:
    assert call(col, [0], [0], rows=rows)[3] == qm.KEY_RANGE  # (every call above started on junk, 0x02 in the status word)


# ---- the tensor API --------------------------------------------------------------------------------------------------------
def test_ops_quantiles_median_kth_value_and_bounds():
    rng = np.random.default_rng(21)
    n = (1 << 16) + 13
    host = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    t = torch.from_numpy(host.view(np.int32)).cuda()
    for signed in (False, True):
        ordered = np.sort(host.view(np.int32) if signed else host).astype(np.int64)
        qs = [0, n - 1, (1, 2), Fraction(1, 3), 0.25, 0.999, 1.0, n]
        values, below, equal = ops.quantiles(t, qs, signed=signed)
        want = qm.select(host, *ops._quantile_ranks(qs), qm.SIGNED if signed else 0)
        as_order = (lambda v: v.view(np.int32).astype(np.int64)) if signed else (lambda v: v.astype(np.int64))
        assert values.dtype == torch.int64 and values.tolist() == as_order(want[0]).tolist()
        assert below.tolist() == want[1].tolist() and equal.tolist() == want[2].tolist()
        assert values.tolist()[:3] == [ordered[0], ordered[-1], ordered[(n + 1) // 2 - 1]] and equal[-1] == 0 and below[-1] == n
        assert ops.median(t, signed=signed) == ordered[(n + 1) // 2 - 1]
        assert ops.kth_value(t, 12345, signed=signed) == ordered[12345]
        for parts in (2, 10, 17):
            bounds = ops.equi_depth_bounds(t, parts, signed=signed)
            assert bounds.tolist() == [ordered[-(-i * n // parts) - 1] for i in range(1, parts)]
    with pytest.raises(IndexError):
        ops.kth_value(t, n)
    with pytest.raises(IndexError):
        ops.median(t[:0])
    # through a list with its count on the device, on a reused plan
    rows = torch.from_numpy(rng.integers(0, n, 5000).astype(np.int32)).cuda()
    count = torch.tensor([3000], dtype=torch.int64, device="cuda")
    plan = ops.Quantiles(9)
    plan.launch(t, [(i, 10) for i in range(1, 10)], rows=rows, count=count)
    picked = np.sort(host[rows.cpu().numpy()[:3000]]).astype(np.int64)
    assert plan.result()[0].tolist() == [picked[-(-i * 3000 // 10) - 1] for i in range(1, 10)]
    plan.launch(t, [0.5], rows=rows, signed=True)
    assert plan.result()[0].tolist() == [np.sort(host.view(np.int32)[rows.cpu().numpy()])[2499]]
    with pytest.raises(IndexError):
        ops.median(t, rows=rows[:0])
    rows[7] = n
    with pytest.raises(Exception, match="status 0x2"):
        ops.quantiles(t, [0.5], rows=rows)
