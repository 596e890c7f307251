"""The selection vectors on the GPU (dwarf_bench_amd/host/select_rows.cpp through select_native and ops): every result is
compared exactly with the numpy model (tests/select_model.py).  The raw entry point runs on guarded buffers
(tests/guard_testlib.py): columns, lists and outputs off their 16-byte boundaries, guard words around everything, the
entries behind the count untouched, the workspace holding anything."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from dwarf_bench_amd import select_native as sn
from tests import select_model as sm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

# candidate counts at the edges of the kernels: nothing and one, a ballot row, a segment, a workgroup's two segments (and
# the eight of a wider build), many ragged segments, and 1026 segments: the scan kernel's 256 threads take 1024 counts a
# round, so a second round
SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 100003, (1 << 22) + 4097)
LO, HI = 0x7FFFFF00, 0x800000FF  # an interval on both sides of 2^31


def call(col, lo, hi, flags=0, rows=None, count=None, offs=(0, 0, 0), fill=FILLS[0], ws_byte=None, count_only=False):
    """one dbench_select_range_u32 on guarded buffers -> (row ids, status); checks the guards, the frozen inputs, the
    entries behind the count, and the count-only contract"""
    w = Watch(fill)
    n = int(col.size)
    d_col = w.col(n, offs[0], data=col, freeze=True)
    d_rows = d_in = None
    cand = n
    if rows is not None:
        cand = int(rows.size)
        d_rows = w.col(cand, offs[1], data=rows, freeze=True)
        if count is not None:
            d_in = w.u64(1)
            d_in.fill_(int(count))
            w.freeze(d_in)
    d_out = w.col(cand, offs[2])
    d_cnt = w.u64(1)
    nbytes = sn.workspace_bytes(cand)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = sn.select_range(ptr(d_col), n, ptr(d_rows) if rows is not None else None, ptr(d_in) if d_in is not None else None,
                         cand if rows is not None else 0, lo, hi, flags, None if count_only else ptr(d_out), ptr(d_cnt),
                         ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    k = int(d_cnt.item())
    assert 0 <= k <= cand
    out = d_out.cpu().numpy().view(np.uint32)
    kept = 0 if count_only else k
    assert (out[kept:] == fill).all(), "entries behind the count were written"
    return (k if count_only else out[:k].copy()), st


def expect(col, lo, hi, flags=0, rows=None, count=None, **how):
    want, want_st = sm.select_range(col, lo, hi, flags, in_rows=rows, in_count=count)
    got, st = call(col, lo, hi, flags, rows, count, **how)
    assert st == want_st, (st, want_st)
    assert got.size == want.size and np.array_equal(got, want), (got.size, want.size)
    return want


def column_of(mask, rng):
    """values inside [LO, HI] where mask is set, outside it (on both sides) elsewhere"""
    n = mask.size
    inside = rng.integers(LO, HI + 1, n, dtype=np.uint64)
    below, above = rng.integers(0, LO, n, dtype=np.uint64), rng.integers(HI + 1, 1 << 32, n, dtype=np.uint64)
    outside = np.where(rng.integers(0, 2, n) == 1, below, above)
    return np.where(mask, inside, outside).astype(np.uint32)


def masks(n, rng):
    rows = np.arange(n)
    yield "no match", np.zeros(n, dtype=bool)
    yield "all match", np.ones(n, dtype=bool)
    yield "row 0", rows == 0
    yield "last row", rows == n - 1
    yield "every 64th", rows % 64 == 0
    yield "alternating", rows % 2 == 1
    seg = (n // 4096) // 2  # all matches inside one segment, some of them
    yield "one segment", (rows // 4096 == seg) & (rng.integers(0, 3, n) == 0)


@pytest.mark.parametrize("n", SIZES)
def test_dense_patterns_at_the_kernel_edges(n):
    rng = np.random.default_rng(n + 1)
    for i, (name, mask) in enumerate(masks(n, rng)):
        col = column_of(mask, rng)
        how = dict(offs=(i % 4, 0, (i + 1) % 4), fill=FILLS[i % 2])
        want = expect(col, LO, HI, **how)
        assert np.array_equal(want, np.flatnonzero(mask)), name
        k, st = call(col, LO, HI, count_only=True, **how)
        assert (k, st) == (want.size, 0), name
    col = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for i, share in enumerate((0.0001, 0.01, 0.5)):
        expect(col, 0, int(share * (1 << 32)), offs=(i + 1, 0, i), fill=FILLS[i % 2])
    expect(col, 0, int(0.5 * (1 << 32)), sm.NEGATE, offs=(3, 0, 2))


@pytest.mark.parametrize("n", (4097, 100003))
def test_predicates_unsigned_signed_negated(n):
    rng = np.random.default_rng(5)
    edges = np.array([0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    col = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    col[rng.integers(0, n, n // 4)] = edges[rng.integers(0, edges.size, n // 4)]
    bounds = [(LO, HI), (0x80000000, 0x80000000), (0x7FFFFFFF, 0x7FFFFFFF), (0, 0xFFFFFFFF), (0x80000000, 0x7FFFFFFF),
              (0x7FFFFFFF, 0x80000000), (HI, LO), (0xFFFFFFFF, 0), (1, 0), (0xC0000000, 0x40000000), (0x40000000, 0xC0000000)]
    i = 0
    for lo, hi in bounds:
        for flags in (0, sm.SIGNED, sm.NEGATE, sm.SIGNED | sm.NEGATE):
            expect(col, lo, hi, flags, offs=(i % 4, 0, (i // 4) % 4), fill=FILLS[i % 2])
            i += 1


def lists(cand, n_col, rng):
    yield "sorted subset", np.sort(rng.choice(n_col, cand, replace=False)).astype(np.uint32)
    yield "shuffled", rng.permutation(n_col)[:cand].astype(np.uint32)
    yield "repeated", rng.integers(0, max(n_col // 100, 1), cand, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("cand", SIZES)
def test_lists_at_the_kernel_edges(cand):
    rng = np.random.default_rng(cand + 3)
    n_col = cand + cand // 3 + 5
    col = rng.integers(0, 1 << 32, n_col, dtype=np.uint64).astype(np.uint32)
    for i, (name, rows) in enumerate(lists(cand, n_col, rng)):
        how = dict(offs=(i, (i + 1) % 4, (i + 2) % 4), fill=FILLS[i % 2])
        expect(col, 0x40000000, 0xC0000000, rows=rows, **how)  # about half
        expect(col, 0x40000000, 0xC0000000, sm.SIGNED | sm.NEGATE, rows=rows, **how)
        expect(col, 0, 1 << 22, rows=rows, count=cand, **how)  # about 0.1 %
    rows = rng.permutation(n_col)[:cand].astype(np.uint32)
    expect(col, 0, 0xFFFFFFFF, rows=rows, offs=(1, 3, 2))  # every candidate: the list comes back
    expect(col, 0, 0xFFFFFFFF, sm.NEGATE, rows=rows, offs=(2, 2, 1))  # none
    want = expect(col, 0, 0x7FFFFFFF, rows=rows, offs=(0, 1, 3))
    k, st = call(col, 0, 0x7FFFFFFF, rows=rows, offs=(0, 1, 3), count_only=True)
    assert (k, st) == (want.size, 0)


@pytest.mark.parametrize("cand", (65, 4097, 100003))
def test_device_count_below_equal_above_the_capacity(cand):
    rng = np.random.default_rng(cand)
    col = rng.integers(0, 1000, 2 * cand, dtype=np.uint64).astype(np.uint32)
    rows = rng.permutation(2 * cand)[:cand].astype(np.uint32)
    for i, count in enumerate((0, 1, 64, cand // 2, cand - 1, cand, cand + 1, 1 << 40, None)):
        for flags in (0, sm.NEGATE):
            expect(col, 100, 600, flags, rows=rows, count=count, offs=(0, i % 4, (i + 1) % 4), fill=FILLS[i % 2])
    # behind the count the list may hold anything: it is not looked at
    rows[cand // 2:] = 0xFFFFFFFF
    expect(col, 100, 600, rows=rows, count=cand // 2, offs=(1, 1, 1))


@pytest.mark.parametrize("cand", (64, 4097, 100003))
def test_row_ids_outside_the_column_are_dropped_and_flagged(cand):
    rng = np.random.default_rng(cand + 9)
    n_col = cand // 2 + 7
    col = rng.integers(0, 1000, n_col, dtype=np.uint64).astype(np.uint32)
    rows = rng.integers(0, n_col, cand, dtype=np.uint64).astype(np.uint32)
    at = rng.choice(cand, max(cand // 50, 3), replace=False)
    rows[at] = rng.integers(n_col, 1 << 32, at.size, dtype=np.uint64).astype(np.uint32)
    rows[at[0]], rows[at[1]], rows[at[2]] = 0xFFFFFFFF, n_col, 0x80000000
    for flags in (0, sm.NEGATE, sm.SIGNED, sm.SIGNED | sm.NEGATE):
        for lo, hi in ((100, 600), (0, 0xFFFFFFFF), (1, 0)):
            want = sm.select_range(col, lo, hi, flags, in_rows=rows)
            assert want[1] == sm.KEY_RANGE and (want[0] < n_col).all()
            expect(col, lo, hi, flags, rows=rows, offs=(flags, 1, 2))
    # the next clean call on the same workspace leaves status 0; then the flagged one again, then a clean dense one
    plan = ops.SelectRows(cand)
    d_col, d_rows = torch.from_numpy(col.view(np.int32)).cuda(), torch.from_numpy(rows.view(np.int32)).cuda()
    clean = rows.copy()
    clean[at] = 0
    d_clean = torch.from_numpy(clean.view(np.int32)).cuda()
    for flagged in (True, False, True, False):
        plan.launch(d_col, 100, 600, rows=d_rows if flagged else d_clean, negate=True)
        torch.cuda.synchronize()
        assert plan.status() == (sm.KEY_RANGE if flagged else 0)
        got = plan.result(strict=False).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, sm.select_range(col, 100, 600, sm.NEGATE, in_rows=rows if flagged else clean)[0])
    plan.launch(d_col, 100, 600, rows=d_rows)
    with pytest.raises(ops._capi.DbhipError):
        plan.result()
    plan.launch(d_col, 100, 600)
    assert np.array_equal(plan.result().cpu().numpy().view(np.uint32), sm.select_range(col, 100, 600)[0])


def test_every_alignment_of_column_list_and_output():
    rng = np.random.default_rng(21)
    n_col, cand = 9001, 4097 + 130
    col = rng.integers(0, 1000, n_col, dtype=np.uint64).astype(np.uint32)
    rows = rng.integers(0, n_col, cand, dtype=np.uint64).astype(np.uint32)
    want_dense, want_list = sm.select_range(col, 250, 750)[0], sm.select_range(col, 250, 750, in_rows=rows)[0]
    for a in range(4):
        for b in range(4):
            for fill in FILLS:
                got, st = call(col, 250, 750, offs=(a, 0, b), fill=fill)
                assert st == 0 and np.array_equal(got, want_dense), (a, b)
                for c in range(4):
                    got, st = call(col, 250, 750, rows=rows, offs=(c, a, b), fill=fill)
                    assert st == 0 and np.array_equal(got, want_list), (c, a, b)


@pytest.mark.parametrize("n", (4097, 100003))
def test_the_workspace_may_hold_anything(n):
    rng = np.random.default_rng(n)
    col = rng.integers(0, 1000, n, dtype=np.uint64).astype(np.uint32)
    rows = rng.permutation(n)[: n // 2].astype(np.uint32)
    for ws_byte in (0x00, 0xFF, None):  # None: the guard's fill pattern
        for fill in FILLS:
            expect(col, 100, 300, ws_byte=ws_byte, fill=fill, offs=(1, 0, 3))
            expect(col, 100, 300, rows=rows, count=n // 3, ws_byte=ws_byte, fill=fill, offs=(1, 2, 3))
            expect(col, 5000, 6000, rows=rows, ws_byte=ws_byte, fill=fill)  # no match: no segment is written


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@pytest.mark.parametrize("n", (4097, 100003))
def test_chain_of_refinements_is_the_conjunction(n):
    rng = np.random.default_rng(n + 2)
    a, b, c = (rng.integers(0, 100, n, dtype=np.uint64).astype(np.uint32) for _ in range(3))
    da, db, dc = dev(a), dev(b), dev(c)
    pa, pb, pc = (a >= 10) & (a <= 80), b <= 50, (c >= 30) & (c <= 99)
    plan = ops.SelectRows(n)
    for _ in range(2):  # the second round starts on the other buffer
        plan.launch(da, 10, 80)
        plan.refine(db, 0, 50)
        plan.refine(dc, 30, 99)  # nothing was read back in between
        got = plan.result().cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.flatnonzero(pa & pb & pc))
        assert np.array_equal(got, sm.chain([a, b, c], [(10, 80), (0, 50), (30, 99)]))
    one = ops.select_range(da, 10, 80)
    two = ops.select_range(db, 0, 50, rows=one)
    three = ops.select_range(dc, 99, 30, rows=two, negate=True)  # the empty interval negated: every candidate
    assert np.array_equal(three.cpu().numpy().view(np.uint32), np.flatnonzero(pa & pb))
    signed = ops.select_range(dev((a.astype(np.int64) - 50).astype(np.int32)), -40, 30, signed=True)
    assert np.array_equal(signed.cpu().numpy(), np.flatnonzero(pa))


def test_ping_pong_never_hands_out_a_buffer_a_pending_launch_reads():
    n = 100003
    rng = np.random.default_rng(4)
    a, b = (rng.integers(0, 100, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    da, db = dev(a), dev(b)
    plan = ops.SelectRows(n)
    plan.launch(da, 0, 49)
    first = plan.result()
    keep = first.clone()
    plan.launch(db, 0, 49)  # a fresh launch: the view handed out last stays as it is
    second = plan.result()
    assert first.data_ptr() != second.data_ptr() and torch.equal(first, keep)
    plan.launch(db, 50, 99, rows=first)  # the list is the plan's own other buffer: the call may not write it
    third = plan.result()
    assert third.data_ptr() != first.data_ptr() and torch.equal(first, keep)
    assert np.array_equal(third.cpu().numpy().view(np.uint32), np.flatnonzero((a <= 49) & (b >= 50)))
    for i in range(5):  # a long chain alternates, every step reading the buffer the step before wrote
        plan.refine(da if i % 2 else db, 0, 99)
    assert np.array_equal(plan.result().cpu().numpy().view(np.uint32), np.flatnonzero((a <= 49) & (b >= 50)))


@pytest.mark.parametrize("n_build", (1, 4096, 65536, (1 << 17) + 5))
def test_semi_and_anti_join(n_build):
    rng = np.random.default_rng(n_build)
    n_probe = 50021
    build = rng.integers(1, 2 * n_build + 1, n_build, dtype=np.uint64).astype(np.uint32)  # keys repeat
    hits = build[rng.integers(0, n_build, n_probe)]
    misses = rng.integers(1 << 30, 1 << 31, n_probe, dtype=np.uint64).astype(np.uint32)
    d_build = dev(build)
    for share, probe in ((0, misses), (50, np.where(rng.integers(0, 2, n_probe) == 1, hits, misses)), (100, hits)):
        d_probe = dev(probe)
        semi = ops.semi_join(d_build, d_probe).cpu().numpy().view(np.uint32)
        anti = ops.semi_join(d_build, d_probe, anti=True).cpu().numpy().view(np.uint32)
        found = np.isin(probe, build)
        assert np.array_equal(semi, np.flatnonzero(found)), share
        assert np.array_equal(anti, np.flatnonzero(~found)), share
        assert np.intersect1d(semi, anti).size == 0
        assert np.array_equal(np.union1d(semi, anti), np.arange(n_probe))
        if share in (0, 100):
            assert (semi.size, anti.size) == ((0, n_probe) if share == 0 else (n_probe, 0))
