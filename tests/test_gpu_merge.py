"""The merge-path kernels on the GPU (dwarf_bench_amd/host/merge_sorted.cpp through merge_native and ops): every result
is compared exactly with the numpy model (tests/merge_model.py).  The raw entry points run on guarded buffers
(tests/guard_testlib.py): columns off their 16-byte boundaries, guard words around everything, frozen inputs, the
entries behind the count untouched, the workspace holding anything.  Sizes come from T = DBENCH_MERGE_TILE_ROWS."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import merge_native as mn
from dwarf_bench_amd import ops
from tests import merge_model as mm
from tests import merge_testlib as ml
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

T = mn.TILE_ROWS
KEYS, CARRIED, IDS = "keys only", "carried values", "row ids"
MODES = (KEYS, CARRIED, IDS)


def _count(w, value):
    if value is None:
        return None
    d = w.u64(1)
    d.fill_(int(value))
    w.freeze(d)
    return d


def call_merge(a, b, flags=0, mode=KEYS, a_vals=None, b_vals=None, a_count=None, b_count=None, offs=(0,) * 6,
               fill=FILLS[0], ws_byte=None):
    """one dbench_merge_u32 on guarded buffers; a and b are the capacity-sized columns -> (keys, values or None, count,
    status); checks the guards, the frozen inputs and the entries behind the count"""
    w = Watch(fill)
    na, nb = int(a.size), int(b.size)
    d_a, d_b = w.col(na, offs[0], data=a, freeze=True), w.col(nb, offs[1], data=b, freeze=True)
    d_av = d_bv = d_ov = None
    if mode == CARRIED:
        d_av, d_bv = w.col(na, offs[2], data=a_vals, freeze=True), w.col(nb, offs[3], data=b_vals, freeze=True)
    d_ok = w.col(na + nb, offs[4])
    if mode != KEYS:
        d_ov = w.col(na + nb, offs[5])
    d_ac, d_bc, d_oc = _count(w, a_count), _count(w, b_count), w.u64(1)
    nbytes = mn.workspace_bytes(na, nb)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = mn.merge(ptr(d_a), ptr(d_av) if d_av is not None else None, ptr(d_ac) if d_ac is not None else None, na,
                  ptr(d_b), ptr(d_bv) if d_bv is not None else None, ptr(d_bc) if d_bc is not None else None, nb,
                  flags | (mn.ROW_IDS if mode == IDS else 0), ptr(d_ok), ptr(d_ov) if d_ov is not None else None, ptr(d_oc),
                  ptr(ws), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    k = int(d_oc.item())
    assert 0 <= k <= na + nb
    keys = d_ok.cpu().numpy().view(np.uint32)
    assert (keys[k:] == fill).all(), "key entries behind the count were written"
    vals = None
    if d_ov is not None:
        vals = d_ov.cpu().numpy().view(np.uint32)
        assert (vals[k:] == fill).all(), "value entries behind the count were written"
        vals = vals[:k].copy()
    return keys[:k].copy(), vals, k, st


def expect_merge(a, b, flags=0, mode=KEYS, a_vals=None, b_vals=None, a_count=None, b_count=None, **how):
    want = mm.merge(a, b, flags | (mm.ROW_IDS if mode == IDS else 0), a_vals if mode == CARRIED else None,
                    b_vals if mode == CARRIED else None, a_count, b_count)
    got = call_merge(a, b, flags, mode, a_vals, b_vals, a_count, b_count, **how)
    assert got[2:] == want[2:], (got[2:], want[2:])
    assert np.array_equal(got[0], want[0]), "keys"
    assert (got[1] is None) == (want[1] is None) and (want[1] is None or np.array_equal(got[1], want[1])), "values"
    return want


def call_setop(op, a, b, a_count=None, b_count=None, offs=(0, 0, 0), fill=FILLS[0], ws_byte=None, count_only=False):
    """one dbench_setop_u32 on guarded buffers; out has exactly the op's room -> (rows or their number, status)"""
    w = Watch(fill)
    na, nb = int(a.size), int(b.size)
    d_a, d_b = w.col(na, offs[0], data=a, freeze=True), w.col(nb, offs[1], data=b, freeze=True)
    room = mn.set_bound(op, na, nb)
    d_out = w.col(room, offs[2])
    d_ac, d_bc, d_oc = _count(w, a_count), _count(w, b_count), w.u64(1)
    nbytes = mn.workspace_bytes(na, nb)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = mn.setop(op, ptr(d_a), ptr(d_ac) if d_ac is not None else None, na, ptr(d_b),
                  ptr(d_bc) if d_bc is not None else None, nb, None if count_only else ptr(d_out), ptr(d_oc), ptr(ws), nbytes,
                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    k = int(d_oc.item())
    assert 0 <= k <= room, (k, room)
    out = d_out.cpu().numpy().view(np.uint32)
    kept = 0 if count_only else k
    assert (out[kept:] == fill).all(), "entries behind the count were written"
    return (k if count_only else out[:k].copy()), st


def expect_setop(op, a, b, a_count=None, b_count=None, **how):
    want, want_k, want_st = mm.setop(op, a, b, a_count, b_count)
    got, st = call_setop(op, a, b, a_count, b_count, **how)
    assert st == want_st
    assert got.size == want_k and np.array_equal(got, want), (op, got.size, want_k)
    return want


def values_for(na, nb, rng):
    return (rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("na,nb", ml.sizes(T) + [ml.second_round(T)])
def test_merge_every_pattern_at_the_kernel_edges(na, nb):
    rng = np.random.default_rng(na * 7 + nb)
    a_vals, b_vals = values_for(na, nb, rng)
    i = 0
    for name, a, b in ml.key_patterns(na, nb, rng):
        both_orders = name in ("uniform", "edges of both orders")
        for signed in ((False, True) if both_orders else (bool(i % 2),)):
            if signed and both_orders:
                a, b = ml.sort_as(a, True), ml.sort_as(b, True)
            flags = mm.SIGNED if signed else 0
            # the model once: with full columns the row ids index cat(a, b) and cat(a_vals, b_vals)
            keys, ids, count, _ = mm.merge(a, b, flags | mm.ROW_IDS)
            carried = np.concatenate([a_vals, b_vals])[ids]
            for mode, want_vals in ((KEYS, None), (CARRIED, carried), (IDS, ids)):
                offs = tuple((i + j) % 4 for j in (0, 1, 3, 2, 1, 2))
                got = call_merge(a, b, flags, mode, a_vals, b_vals, offs=offs, fill=FILLS[i % 2])
                assert got[2:] == (count, 0), (name, mode)
                assert np.array_equal(got[0], keys), (name, mode, signed)
                assert (want_vals is None and got[1] is None) or np.array_equal(got[1], want_vals), (name, mode, signed)
                i += 1


@pytest.mark.parametrize("na,nb", ((T + 1, T - 1), (3 * T + 5, 100)))
def test_merge_device_counts_below_and_above_the_capacity(na, nb):
    rng = np.random.default_rng(na)
    a = np.sort(rng.integers(0, 5000, na, dtype=np.uint64)).astype(np.uint32)
    b = np.sort(rng.integers(0, 5000, nb, dtype=np.uint64)).astype(np.uint32)
    a_vals, b_vals = values_for(na, nb, rng)
    counts = [(0, 0), (0, None), (None, 0), (1, nb), (na, 1), (na // 2, nb // 3), (T, nb), (na - 1, nb - 1), (na, nb),
              (na + 1, nb), (na, nb + 1), (1 << 40, 1 << 33), (None, nb // 2), (na // 2, None)]
    for i, (ca, cb) in enumerate(counts):
        for mode in MODES:
            want = expect_merge(a, b, 0, mode, a_vals, b_vals, ca, cb, offs=tuple((i + j) % 4 for j in range(6)), fill=FILLS[i % 2])
            if mode == IDS and cb != 0:
                assert (want[1] >= na).any() and want[1].max() < na + nb  # B's ids start at the capacity, not the count
    # behind its count a column may hold anything, unsorted too: it is not looked at
    a[na // 2:], b[nb // 2:] = rng.permutation(na - na // 2).astype(np.uint32), 0
    for mode in MODES:
        expect_merge(a, b, 0, mode, a_vals, b_vals, na // 2, nb // 2, offs=(1, 2, 3, 0, 1, 2))


def test_merge_every_alignment_of_every_column():
    rng = np.random.default_rng(31)
    na, nb = T + 130, T // 2 + 7
    a = np.sort(rng.integers(0, 1000, na, dtype=np.uint64)).astype(np.uint32)
    b = np.sort(rng.integers(0, 1000, nb, dtype=np.uint64)).astype(np.uint32)
    a_vals, b_vals = values_for(na, nb, rng)
    want = {mode: mm.merge(a, b, mm.ROW_IDS if mode == IDS else 0, a_vals if mode == CARRIED else None,
                           b_vals if mode == CARRIED else None) for mode in MODES}
    for col in range(6):
        for off in range(4):
            offs = tuple(off if j == col else (off + j) % 4 for j in range(6))
            for mode in MODES:
                keys, vals, k, st = call_merge(a, b, 0, mode, a_vals, b_vals, offs=offs, fill=FILLS[(col + off) % 2])
                assert (k, st) == (na + nb, 0) and np.array_equal(keys, want[mode][0]), (offs, mode)
                assert vals is None or np.array_equal(vals, want[mode][1]), (offs, mode)


def test_the_workspace_may_hold_anything():
    rng = np.random.default_rng(8)
    na, nb = 3 * T + 5, 2 * T - 9
    a, b = np.sort(rng.choice(20 * T, na, replace=False)).astype(np.uint32), np.sort(rng.choice(20 * T, nb, replace=False)).astype(np.uint32)
    a_vals, b_vals = values_for(na, nb, rng)
    for ws_byte in (0x00, 0xFF, None):  # None: the guard's fill pattern
        for fill in FILLS:
            expect_merge(a, b, 0, CARRIED, a_vals, b_vals, ws_byte=ws_byte, fill=fill, offs=(1, 0, 3, 2, 1, 0))
            expect_merge(a, b, 0, IDS, a_count=na // 3, b_count=nb, ws_byte=ws_byte, fill=fill)
            for op in (mm.UNION, mm.INTERSECT, mm.DIFFERENCE):
                expect_setop(op, a, b, ws_byte=ws_byte, fill=fill, offs=(3, 1, 2))
            expect_setop(mm.INTERSECT, a, a[:0], ws_byte=ws_byte, fill=fill)  # nothing kept: no tile is written


@pytest.mark.parametrize("n", (1, 5, T, T + 7, 20011))
def test_set_operations_on_every_kind_of_pair(n):
    rng = np.random.default_rng(n + 4)
    for i, (name, a, b) in enumerate(ml.set_cases(n, rng)):
        for op, ref in ((mm.UNION, np.union1d), (mm.INTERSECT, np.intersect1d), (mm.DIFFERENCE, np.setdiff1d)):
            how = dict(offs=(i % 4, (i + op) % 4, (i + 2) % 4), fill=FILLS[(i + op) % 2])
            want = expect_setop(op, a, b, **how)
            assert np.array_equal(want, ref(a, b)), (name, op)
            k, st = call_setop(op, a, b, count_only=True, **how)
            assert (k, st) == (want.size, 0), (name, op)


def test_set_operations_with_a_second_round_of_the_scan():
    na, nb = ml.second_round(T)
    rows = np.arange(3 * (na + nb), dtype=np.uint32)
    a, b = rows[rows % 2 == 0][:na], rows[rows % 3 != 1][:nb]  # a third of A is in B: every tile keeps something
    assert (a.size, b.size) == (na, nb) and na + nb == 1025 * T + 3
    for op, ref in ((mm.UNION, np.union1d), (mm.INTERSECT, np.intersect1d), (mm.DIFFERENCE, np.setdiff1d)):
        want = expect_setop(op, a, b, offs=(op, 1, 2), fill=FILLS[op % 2])
        assert np.array_equal(want, ref(a, b))


def test_partner_pairs_across_tile_edges():
    a, b = ml.straddling(T)
    assert ml.pairs_on_tile_edges(a, b, T) == [1, 2, 3]  # at least one pair on merged positions k T - 1 and k T
    for swap in (False, True):
        x, y = (b, a) if swap else (a, b)
        assert ml.pairs_on_tile_edges(x, y, T) == [1, 2, 3]
        for op in (mm.UNION, mm.INTERSECT, mm.DIFFERENCE):
            for i, fill in enumerate(FILLS):
                want = expect_setop(op, x, y, offs=(i, 2 - i, 3), fill=fill)
            assert want.size == {mm.UNION: a.size + b.size - 3, mm.INTERSECT: 3, mm.DIFFERENCE: x.size - 3}[op]
        # the merge's tie order on the same edges: A's element of a pair first
        _, ids, _, _ = expect_merge(x, y, 0, IDS, offs=(1, 2, 0, 0, 3, 1))
        assert all(ids[k * T - 1] < x.size <= ids[k * T] for k in (1, 2, 3))


@pytest.mark.parametrize("n", (T + 1, 20011))
def test_set_operations_device_counts(n):
    rng = np.random.default_rng(n)
    a = np.sort(rng.choice(3 * n, n, replace=False)).astype(np.uint32)
    b = np.sort(rng.choice(3 * n, n - 5, replace=False)).astype(np.uint32)
    for i, (ca, cb) in enumerate(((0, 0), (0, None), (None, 0), (1, 1), (n // 2, n // 3), (T, n), (n - 1, n - 6), (n + 1, n),
                                  (1 << 40, 1 << 33), (n // 3, None))):
        for op in (mm.UNION, mm.INTERSECT, mm.DIFFERENCE):
            expect_setop(op, a, b, ca, cb, offs=(i % 4, (i + 1) % 4, (i + op) % 4), fill=FILLS[i % 2])
    a[n // 2:] = 3  # behind the count a list may hold anything
    expect_setop(mm.DIFFERENCE, a, b, n // 2, n // 2)


def test_unsorted_inputs_stay_inside_the_buffers():
    """the preconditions are not checked: on shuffled inputs only the guards, the count bound and a status read that
    returns are asserted (call_merge and call_setop assert them); the values are unspecified"""
    rng = np.random.default_rng(77)
    n = T + 7
    for trial in range(3):
        a, b = (rng.integers(0, 1 << (8 * trial + 8), n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
        a_vals, b_vals = values_for(n, n, rng)
        for mode in MODES:
            for flags in (0, mm.SIGNED):
                _, _, k, st = call_merge(a, b, flags, mode, a_vals, b_vals, offs=(trial, 1, 2, 3, 0, 1), fill=FILLS[trial % 2])
                assert (k, st) == (2 * n, 0)
        for op in (mm.UNION, mm.INTERSECT, mm.DIFFERENCE):
            for ca in (None, n // 2):
                got, st = call_setop(op, a, b, ca, None, offs=(1, trial, 3), fill=FILLS[trial % 2])
                assert st == 0 and got.size <= mn.set_bound(op, n, n)
    # descending lists: every partition point sits at an end, every A element meets an exhausted or a fresh B
    a, b = np.arange(5 * T, 0, -1, dtype=np.uint32), np.arange(3 * T, 0, -1, dtype=np.uint32)
    for op in (mm.UNION, mm.INTERSECT, mm.DIFFERENCE):
        got, st = call_setop(op, a, b, fill=FILLS[1])
        assert st == 0 and got.size <= mn.set_bound(op, a.size, b.size)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


@pytest.mark.parametrize("na,nb", ((T + 1, T - 1), (100003, 50021)))
def test_ops_merge_with_row_ids_is_the_argsort_of_the_concatenation(na, nb):
    rng = np.random.default_rng(na)
    for signed in (False, True):
        a = ml.sort_as(rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32) >> (0 if signed else 20), signed)
        b = ml.sort_as(rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32) >> (0 if signed else 20), signed)
        keys, ids = ops.merge_sorted(dev(a), dev(b), signed=signed, row_ids=True)
        cat = dev(np.concatenate([a, b]))
        perm = ops.radix_argsort_(cat, signed=signed)  # sorts cat in place
        assert torch.equal(ids, perm) and torch.equal(keys, cat)
        want = mm.merge(a, b, mm.ROW_IDS | (mm.SIGNED if signed else 0))
        assert np.array_equal(ids.cpu().numpy().view(np.uint32), want[1])
    av, bv = values_for(na, nb, rng)
    keys, vals = ops.merge_sorted(dev(a), dev(b), dev(av), dev(bv), signed=True)
    want = mm.merge(a, b, mm.SIGNED, av, bv)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(vals.cpu().numpy().view(np.uint32), want[1])
    keys, vals = ops.merge_sorted(dev(a), dev(b), signed=True)
    assert vals is None and np.array_equal(keys.cpu().numpy().view(np.uint32), want[0])
    plan = ops.MergeSorted(na, nb)  # a plan on shorter columns than it holds, and on empty ones
    plan.launch(dev(a[: na // 2]), dev(b[:0]), signed=True, row_ids=True)
    keys, ids = plan.result()
    assert plan.status() == 0 and plan.count() == na // 2 and np.array_equal(ids.cpu().numpy(), np.arange(na // 2))


@pytest.mark.parametrize("share", (0.0, 0.01, 0.5, 1.0))
def test_ops_select_any_is_the_disjunction(share):
    n = 100003
    rng = np.random.default_rng(int(share * 100) + 1)
    cols = [rng.integers(0, 1 << 31, n, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    hi = min(int(share * (1 << 31)), (1 << 31) - 1)  # lo = 1: share 0 is the empty interval [1, 0]
    if share == 1.0:
        cols = [np.maximum(c, 1) for c in cols]
    ka, kb = ((c >= 1) & (c <= hi) for c in cols)
    got = ops.select_any(dev(cols[0]), 1, hi, dev(cols[1]), 1, hi).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, np.flatnonzero(ka | kb))
    assert got.size == {0.0: 0, 1.0: n}.get(share, got.size)
    rows_a, rows_b = dev(np.flatnonzero(ka).astype(np.uint32)), dev(np.flatnonzero(kb).astype(np.uint32))
    assert np.array_equal(ops.union_rows(rows_a, rows_b).cpu().numpy().view(np.uint32), got)
    assert np.array_equal(ops.intersect_rows(rows_a, rows_b).cpu().numpy().view(np.uint32), np.flatnonzero(ka & kb))
    assert np.array_equal(ops.difference_rows(rows_a, rows_b).cpu().numpy().view(np.uint32), np.flatnonzero(ka & ~kb))


def test_ops_refuses_what_the_plans_do_not_hold():
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="plan holds"):
        ops.MergeSorted(8, 16).launch(d, d)
    with pytest.raises(ValueError, match="plan holds"):
        ops.RowSets(16, 8).launch("union", d, d)
    with pytest.raises(ValueError, match="both or neither"):
        ops.MergeSorted(16, 16).launch(d, d, a_vals=d)
    with pytest.raises(ValueError, match="row_ids"):
        ops.MergeSorted(16, 16).launch(d, d, a_vals=d, b_vals=d, row_ids=True)
    with pytest.raises(ValueError, match="values for"):
        ops.MergeSorted(16, 16).launch(d, d, a_vals=d[:8], b_vals=d)
    for bad in (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"),
                torch.zeros(1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="count"):
            ops.MergeSorted(16, 16).launch(d, d, a_count=bad)
        with pytest.raises(ValueError, match="count"):
            ops.RowSets(16, 16).launch("union", d, d, b_count=bad)
