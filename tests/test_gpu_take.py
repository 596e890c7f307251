"""Late materialisation on the GPU (dwarf_bench_amd/host/take_rows.cpp through take_native and ops): every result is
compared bit for bit with the numpy model (tests/take_model.py).  The raw entry points run on guarded buffers
(tests/guard_testlib.py): columns, lists and outputs off their 16-byte boundaries, each output by another amount, guard
words around everything, the entries behind the count untouched, the workspace holding anything."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from dwarf_bench_amd import take_native as tn
from tests import take_model as tm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

SEG = tn.SEGMENT_ROWS
# nothing and one, around a lane's four entries, around one segment (with a list off its boundary: around two), and two
# segments and a ragged rest: a workgroup's two waves and a second workgroup
CAPACITIES = (0, 1, 3, 4, 5, SEG - 1, SEG, SEG + 1, 2 * SEG + 3)
N_ROWS = 1777
U = np.uint32


def stream():
    return torch.cuda.current_stream().cuda_stream


def columns(k, n_rows=N_ROWS, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 32, n_rows, dtype=np.uint64).astype(U) for _ in range(k)]


def lists(m, n_rows, rng):
    """name -> a list of m row ids"""
    last = max(n_rows - 1, 0)
    inside = rng.integers(0, max(n_rows, 1), m, dtype=np.uint64).astype(U)
    yield "ascending", np.sort(inside)
    yield "shuffled", inside
    yield "one row throughout", np.full(m, n_rows // 3, U)
    yield "the last row", np.full(m, last, U)
    for bad in (n_rows, n_rows + 1, 0x80000000, 0xFFFFFFFF):
        some = inside.copy()
        some[rng.integers(0, max(m, 1), max(m // 5, 1 if m else 0))] = bad
        yield f"some {bad:#x}", some
    yield "all kinds of bad", np.where(rng.integers(0, 2, m) == 1, inside,
                                       rng.choice(np.array([n_rows, n_rows + 1, 0x80000000, 0xFFFFFFFF], U), m))


def call_take(cols, rows, count=None, flags=0, fill_word=0x0F1E2D3C, list_off=0, out_off=0, col_off=1, fill=FILLS[0],
              ws_byte=None):
    """one dbench_take_u32 on guarded buffers -> (outputs cut to m, status); checks the guards, the frozen inputs and
    that the entries [m, capacity) of every output still hold the guard fill.  Output c sits out_off + c words past a
    16-byte boundary, column c col_off + c words past one."""
    w = Watch(fill)
    k, n_rows, capacity = len(cols), int(cols[0].size), int(rows.size)
    d_cols = [w.col(n_rows, col_off + c, data=col, freeze=True) for c, col in enumerate(cols)]
    d_rows = w.col(capacity, list_off, data=rows, freeze=True)
    d_count = None
    if count is not None:
        d_count = w.u64(1)
        d_count.fill_(count - (1 << 64) if count >> 63 else count)
        w.freeze(d_count)
    d_outs = [w.col(capacity, out_off + c) for c in range(k)]
    nbytes = tn.workspace_bytes(capacity)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = tn.take([ptr(c) for c in d_cols], k, n_rows, ptr(d_rows), ptr(d_count) if d_count is not None else None, capacity,
                 flags, fill_word, [ptr(o) for o in d_outs], ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    m = tm.length(count, capacity)
    outs = [o.cpu().numpy().view(U) for o in d_outs]
    for o in outs:
        assert (o[m:] == U(fill)).all(), "entries behind the count were written"
    return [o[:m].copy() for o in outs], st


def expect_take(cols, rows, count=None, flags=0, fill_word=0x0F1E2D3C, **how):
    want, want_st = tm.take(cols, rows, count, flags, fill_word)
    got, st = call_take(cols, rows, count, flags, fill_word, **how)
    m = tm.length(count, rows.size)
    assert st == want_st, (st, want_st)
    for c, (g, wnt) in enumerate(zip(got, want)):
        assert np.array_equal(g, wnt[:m]), f"column {c}: {int((g != wnt[:m]).sum())} of {m} entries differ"
    return want_st


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_every_alignment_of_list_and_outputs(capacity):
    """list offset x output offset, the number of columns going round 1..4; output c and column c each another word on"""
    rng = np.random.default_rng(capacity)
    kinds = list(lists(capacity, N_ROWS, rng))
    seen = set()
    for list_off in range(4):
        for out_off in range(4):
            i = 4 * list_off + out_off
            k = 1 + (i + list_off) % 4
            name, rows = kinds[i % len(kinds)]
            flags = tn.OUTER if i % 3 == 0 else 0
            st = expect_take(columns(k), rows, flags=flags, list_off=list_off, out_off=out_off, col_off=1 + i % 3,
                             fill=FILLS[i % 2])
            seen.add((k, st))
    if capacity >= 5:
        assert {k for k, _ in seen} == {1, 2, 3, 4} and {st for _, st in seen} == {0, tm.KEY_RANGE}


@pytest.mark.parametrize("k", (1, 2, 3, 4))
def test_every_kind_of_list_with_and_without_outer(k):
    rng = np.random.default_rng(40 + k)
    cols = columns(k)
    for capacity in (SEG + 1, 2 * SEG + 3):
        for i, (name, rows) in enumerate(lists(capacity, N_ROWS, rng)):
            for flags in (0, tn.OUTER):
                st = expect_take(cols, rows, flags=flags, list_off=i % 4, out_off=(i + k) % 4, fill=FILLS[(i + flags) % 2])
                bad = rows[(rows >= N_ROWS) & ~((rows == 0xFFFFFFFF) & bool(flags))]
                assert st == (tm.KEY_RANGE if bad.size else 0), (name, flags)


@pytest.mark.parametrize("capacity", (5, SEG + 1, 2 * SEG + 3))
def test_counts_on_the_device_and_the_untouched_tail(capacity):
    rng = np.random.default_rng(capacity + 7)
    rows = rng.integers(0, N_ROWS, capacity, dtype=np.uint64).astype(U)
    rows[-1] = N_ROWS + 5  # the last entry is bad: it raises only when the count reaches it
    cols = columns(2)
    for i, count in enumerate((None, 0, 1, capacity - 1, capacity, capacity + 7, (1 << 32) + 1, (1 << 64) - 1)):
        st = expect_take(cols, rows, count=count, list_off=i % 4, out_off=(3 * i + 1) % 4, fill=FILLS[i % 2])
        assert st == (tm.KEY_RANGE if tm.length(count, capacity) == capacity else 0), count


def test_a_table_without_rows_fills_every_entry():
    empty = [np.zeros(0, U), np.zeros(0, U)]
    for i, capacity in enumerate((1, 5, SEG + 1)):
        rows = np.arange(capacity, dtype=U)
        assert expect_take(empty, rows, fill=FILLS[i % 2], list_off=i, out_off=i + 1) == tm.KEY_RANGE
        rows = np.full(capacity, 0xFFFFFFFF, U)
        assert expect_take(empty, rows, flags=tn.OUTER, fill=FILLS[i % 2], list_off=i + 1, out_off=i) == 0
        assert expect_take(empty, rows, fill=FILLS[i % 2], count=capacity - 1) == (tm.KEY_RANGE if capacity > 1 else 0)


# ---- aggregate ----------------------------------------------------------------------------------------------------------
def call_aggregate(col, rows=None, count=None, flags=0, list_off=0, col_off=1, fill=FILLS[0], ws_byte=None, ws_capacity=None):
    """one dbench_aggregate_rows_u32 on guarded buffers -> (the four uint64 words, status)"""
    w = Watch(fill)
    n_rows = int(col.size)
    d_col = w.col(n_rows, col_off, data=col, freeze=True)
    d_rows = d_count = None
    capacity = 0
    if rows is not None:
        capacity = int(rows.size)
        d_rows = w.col(capacity, list_off, data=rows, freeze=True)
        if count is not None:
            d_count = w.u64(1)
            d_count.fill_(count - (1 << 64) if count >> 63 else count)
            w.freeze(d_count)
    d_out = w.u64(4)
    nbytes = tn.workspace_bytes(capacity if ws_capacity is None else ws_capacity)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = tn.aggregate(ptr(d_col), n_rows, ptr(d_rows) if rows is not None else None,
                      ptr(d_count) if d_count is not None else None, capacity, flags, ptr(d_out), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return tuple(int(x) & tm.M64 for x in d_out.tolist()), st


def expect_aggregate(col, rows=None, count=None, flags=0, **how):
    want = tm.aggregate(col, rows, count, flags)
    got = call_aggregate(col, rows, count, flags, **how)
    assert got == want, (got, want)
    return want


def extreme_column(n_rows, rng):
    """values at both ends of both number lines, so that the 64-bit sum and the signedness matter"""
    edges = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], U)
    col = rng.integers(0, 1 << 32, n_rows, dtype=np.uint64).astype(U)
    at = rng.integers(0, n_rows, n_rows // 2)
    col[at] = edges[rng.integers(0, edges.size, at.size)]
    return col


@pytest.mark.parametrize("flags", (0, tn.SIGNED))
def test_aggregate_over_lists(flags):
    rng = np.random.default_rng(11 + flags)
    col = extreme_column(N_ROWS, rng)
    for capacity in CAPACITIES + (9 * SEG + 5,):  # (nine segments: a workgroup's second turn is not needed, a third workgroup is)
        for i, (name, rows) in enumerate(lists(capacity, N_ROWS, rng)):
            for outer in (0, tn.OUTER):
                if (i + bool(outer)) % 2:  # every kind with or without OUTER, in turn
                    continue
                (n, total, _, _), st = expect_aggregate(col, rows, flags=flags | outer, list_off=i % 4, col_off=(i + 1) % 4,
                                                        fill=FILLS[i % 2])
                assert n == int((rows < N_ROWS).sum()), name
    # the sum needs its 64 bits: thousands of 0xFFFFFFFF, each -1 as int32
    ones = np.full(N_ROWS, 0xFFFFFFFF, U)
    rows = rng.integers(0, N_ROWS, 5000, dtype=np.uint64).astype(U)
    (n, total, least, most), st = expect_aggregate(ones, rows, flags=flags)
    assert (n, st) == (5000, 0) and total == ((-5000) % (1 << 64) if flags else 5000 * 0xFFFFFFFF) and total >> 32
    low = np.full(N_ROWS, 0x80000000, U)
    (n, total, least, most), _ = expect_aggregate(low, rows, flags=flags)
    assert total == ((-5000 << 31) % (1 << 64) if flags else 5000 << 31) and least == most


@pytest.mark.parametrize("flags", (0, tn.SIGNED))
def test_aggregate_counts_empty_lists_and_candidates_all_out_of_range(flags):
    rng = np.random.default_rng(21)
    col = extreme_column(N_ROWS, rng)
    empty = (0, 0, (1 << 31) - 1 if flags else 0xFFFFFFFF, (-(1 << 31)) % (1 << 64) if flags else 0)
    capacity = 2 * SEG + 3
    rows = rng.integers(0, N_ROWS, capacity, dtype=np.uint64).astype(U)
    for i, count in enumerate((None, 0, 1, capacity - 1, capacity, capacity + 7, (1 << 32) + 1)):
        got, st = expect_aggregate(col, rows, count=count, flags=flags, list_off=i % 4, fill=FILLS[i % 2])
        assert st == 0 and got[0] == tm.length(count, capacity) and (count != 0 or got == empty)
    assert expect_aggregate(col, np.zeros(0, U), flags=flags) == (empty, 0)
    for bad, outer, want_st in ((N_ROWS, 0, 2), (0x80000000, tn.OUTER, 2), (0xFFFFFFFF, 0, 2), (0xFFFFFFFF, tn.OUTER, 0)):
        for capacity in (1, SEG + 1):
            got = expect_aggregate(col, np.full(capacity, bad, U), flags=flags | outer, list_off=capacity % 4)
            assert got == (empty, want_st), (bad, outer)
    assert expect_aggregate(np.zeros(0, U), np.arange(7, dtype=U), flags=flags) == (empty, 2)  # a table without rows


@pytest.mark.parametrize("flags", (0, tn.SIGNED))
def test_aggregate_over_all_rows(flags):
    rng = np.random.default_rng(31)
    empty = (0, 0, (1 << 31) - 1 if flags else 0xFFFFFFFF, (-(1 << 31)) % (1 << 64) if flags else 0)
    for i, n_rows in enumerate(CAPACITIES + (9 * SEG + 5, 100003)):
        col = extreme_column(n_rows, rng) if n_rows else np.zeros(0, U)
        # the smallest workspace (capacity 0: eight partial records) and one sized for the column
        for ws_capacity in (0, n_rows):
            got, st = expect_aggregate(col, flags=flags, col_off=i % 4, fill=FILLS[i % 2], ws_capacity=ws_capacity)
            assert st == 0 and got[0] == n_rows and (n_rows or got == empty)


def test_a_workspace_that_held_another_calls_data():
    """poisoned workspaces, and one workspace through aggregate -> take -> aggregate: identical outputs every time"""
    rng = np.random.default_rng(51)
    col = extreme_column(N_ROWS, rng)
    rows = rng.integers(0, N_ROWS + 3, 9 * SEG + 5, dtype=np.uint64).astype(U)
    for byte in (0x00, 0xFF, 0x5A):
        expect_take([col, col[::-1].copy()], rows, ws_byte=byte, list_off=1, out_off=2)
        expect_aggregate(col, rows, flags=tn.SIGNED, ws_byte=byte)
        expect_aggregate(col, ws_byte=byte, ws_capacity=N_ROWS)
    agg, taker = ops.AggregateRows(rows.size), ops.TakeRows(rows.size, 2)
    taker.ws, taker.ws_bytes = agg.ws, agg.ws_bytes  # one workspace for both plans
    d_col, d_rows = (torch.from_numpy(x.view(np.int32)).cuda() for x in (col, rows))
    inside = (rows % U(N_ROWS)).astype(U)
    good = torch.from_numpy(inside.view(np.int32)).cuda()
    want_bad, want_good = tm.aggregate(col, rows), tm.aggregate(col, inside)
    for _ in range(2):
        agg.launch(d_col, d_rows)
        assert agg.status() == tm.KEY_RANGE == want_bad[1]
        assert agg.result(strict=False) == tm.as_ints(want_bad[0], False)
        taker.launch([d_col, d_col], good)  # clears the status word the aggregate raised
        assert taker.status() == 0
        assert all(np.array_equal(o.cpu().numpy().view(U), col[inside]) for o in taker.result())
        agg.launch(d_col, good, signed=True)
        assert agg.result() == tm.as_ints(tm.aggregate(col, inside, flags=tm.SIGNED)[0], True)
        agg.launch(d_col, good)
        assert agg.result() == tm.as_ints(want_good[0], False)


# ---- the tensor API -----------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(U)


def test_ops_take_and_aggregate_rows():
    rng = np.random.default_rng(61)
    n = 50021
    cols = [extreme_column(n, rng) for _ in range(6)]
    rows = rng.integers(0, n, 3 * SEG + 1, dtype=np.uint64).astype(U)
    one = ops.take(dev(cols[0]), dev(rows))
    assert torch.is_tensor(one) and np.array_equal(host(one), cols[0][rows])
    six = ops.take([dev(c) for c in cols], dev(rows))  # more than four columns: groups of four
    assert isinstance(six, list) and len(six) == 6 and all(np.array_equal(host(g), c[rows]) for g, c in zip(six, cols))
    assert ops.take(dev(cols[0]), dev(np.zeros(0, U))).numel() == 0
    for signed in (False, True):
        flags = tm.SIGNED if signed else 0
        assert ops.aggregate_rows(dev(cols[1]), dev(rows), signed=signed) == tm.as_ints(tm.aggregate(cols[1], rows, flags=flags)[0], signed)
        assert ops.aggregate_rows(dev(cols[1]), signed=signed) == tm.as_ints(tm.aggregate(cols[1], flags=flags)[0], signed)
        assert ops.aggregate_rows(dev(cols[1]), dev(np.zeros(0, U)), signed=signed) == (0, 0, None, None)
    bad = rows.copy()
    bad[5] = n
    with pytest.raises(ops._capi.DbhipError, match="0x2"):
        ops.take(dev(cols[0]), dev(bad))
    with pytest.raises(ops._capi.DbhipError, match="0x2"):
        ops.aggregate_rows(dev(cols[0]), dev(bad))
    plan = ops.TakeRows(bad.size, 2)
    plan.launch([dev(cols[0]), dev(cols[1])], dev(bad), fill=-7)
    got = plan.result(strict=False)
    want, st = tm.take(cols[:2], bad, fill=-7)
    assert plan.status() == st == tm.KEY_RANGE and all(np.array_equal(host(g), w) for g, w in zip(got, want))
    plan.launch(dev(cols[2]), dev(rows))  # fewer columns than the plan holds, and the status is clear again
    assert len(plan.result()) == 1 and np.array_equal(host(plan.result()[0]), cols[2][rows])


def test_composition_with_select_sets_and_the_outer_join():
    rng = np.random.default_rng(71)
    n = 100003
    a, b, c = (rng.integers(0, 1000, n, dtype=np.uint64).astype(U) for _ in range(3))
    da, db, dc = dev(a), dev(b), dev(c)
    # select -> refine with the count on the device -> take of two columns and the aggregate of a third
    sel = ops.SelectRows(n)
    sel.launch(da, 100, 499)
    sel.refine(db, 0, 299)
    rows, count = sel.output()
    taker, agg = ops.TakeRows(n, 2), ops.AggregateRows(n)
    taker.launch([db, dc], rows, count)
    agg.launch(dc, rows, count)
    want = np.flatnonzero((a >= 100) & (a <= 499) & (b <= 299))
    got = taker.result()
    assert sel.status() == 0 and got[0].numel() == want.size
    assert np.array_equal(host(got[0]), b[want]) and np.array_equal(host(got[1]), c[want])
    assert agg.result() == (want.size, int(c[want].astype(np.uint64).sum()), int(c[want].min()), int(c[want].max()))
    outs, out_count = taker.output()
    assert out_count is count and all(o.numel() == n for o in outs)
    # the eager forms on select_range's result
    picked = ops.select_range(da, 100, 499)
    assert np.array_equal(host(ops.take(db, picked)), b[(a >= 100) & (a <= 499)])
    assert ops.aggregate_rows(db, picked)[0] == int(((a >= 100) & (a <= 499)).sum())
    # RowSets: the union of two selections, its count on the device
    other = ops.SelectRows(n)
    other.launch(db, 900, 999)
    sets = ops.RowSets(n, n)
    sets.launch("union", rows, other.output()[0], count, other.output()[1])
    wide_take, wide_agg = ops.TakeRows(2 * n, 1), ops.AggregateRows(2 * n)
    wide_take.launch(dc, sets.rows, sets.out_count)
    wide_agg.launch(dc, sets.rows, sets.out_count, signed=True)
    either = np.flatnonzero(((a >= 100) & (a <= 499) & (b <= 299)) | (b >= 900))
    assert np.array_equal(host(wide_take.result()[0]), c[either])
    assert wide_agg.result() == (either.size, int(c[either].astype(np.int64).sum()), int(c[either].min()), int(c[either].max()))
    assert np.array_equal(host(ops.take(dc, sets.result())), c[either])
    # the left-outer join: the build row of a probe row without a match is -1, filled under outer=True
    build = np.arange(0, 2000, 2, dtype=U)  # the even keys below 2000, each once
    probe = rng.integers(0, 2000, 5000, dtype=np.uint64).astype(U)
    payload = rng.integers(0, 1 << 32, build.size, dtype=np.uint64).astype(U)
    build_rows, probe_rows = ops.join_pairs(dev(build), dev(probe), left_outer=True)
    assert build_rows.numel() == probe.size
    got = host(ops.take(dev(payload), build_rows, outer=True, fill=0xDEADBEEF - (1 << 32)))
    keys = probe[host(probe_rows)]
    assert np.array_equal(got, np.where(keys % 2 == 0, payload[np.minimum(keys // 2, build.size - 1)], U(0xDEADBEEF)))
    hit = keys % 2 == 0
    n_hit, total, least, most = ops.aggregate_rows(dev(payload), build_rows, outer=True)
    assert (n_hit, total) == (int(hit.sum()), int(payload[keys[hit] // 2].astype(np.uint64).sum()))
    with pytest.raises(ops._capi.DbhipError, match="0x2"):
        ops.take(dev(payload), build_rows)  # without outer the same id is a row outside the column
    # JoinPairs' own buffers and device total, capacity above the total
    join = ops.HashJoin(build.size, probe.size)
    join.build(dev(build))
    join.probe(dev(probe))
    pairs = ops.JoinPairs(probe.size, probe.size + 100)
    pairs.launch(join.ids[: build.size], join.pos[: probe.size], join.cnt[: probe.size], None, True)
    taker = ops.TakeRows(pairs.capacity, 1)
    taker.launch(dev(payload), pairs.build_rows, pairs.total, outer=True, fill=5)
    got = taker.result()[0]
    keys = probe[host(pairs.probe_rows[: pairs.count()])]
    assert got.numel() == probe.size
    assert np.array_equal(host(got), np.where(keys % 2 == 0, payload[np.minimum(keys // 2, build.size - 1)], U(5)))
