"""Dictionary encoding on the GPU (dwarf_bench_amd/host/dict_encode.cpp through dict_native and ops): every result is
compared bit for bit with the numpy model (tests/dict_model.py) or with numpy itself.  The raw entry points run on guarded
buffers (tests/guard_testlib.py): columns and outputs off their 16-byte boundaries, guard words around everything, the
entries behind the count untouched, the workspace pre-filled with each of FILLS."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import dict_native as dn
from dwarf_bench_amd import ops
from tests import dict_model as dm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

U = np.uint32
BUILD_TILE, ENCODE_TILE = 1024, 4096  # rows of a workgroup at a time in the insert and the encode kernels
# nothing and one, around a lane's four rows, around a wave's 64 and 256, around one tile of either kernel, two tiles + 3
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, BUILD_TILE - 1, BUILD_TILE, BUILD_TILE + 1, ENCODE_TILE - 1, ENCODE_TILE,
         ENCODE_TILE + 1, 2 * ENCODE_TILE + 3)
LDS_CAPACITY = dn.LDS_SLOTS // 2  # the largest capacity whose table has LDS_SLOTS slots; one more: the global body
CAPACITIES = (1, 2, LDS_CAPACITY, LDS_CAPACITY + 1)
EDGES = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], U)


def stream():
    return torch.cuda.current_stream().cuda_stream


def u64_word(w, value):
    t = w.u64(1)
    t.fill_(value - (1 << 64) if value >> 63 else value)
    w.freeze(t)
    return t


class Built:
    """one dbench_dict_build_u32 on guarded buffers; the workspace stays for the encodes that follow"""

    def __init__(self, col, capacity, count=None, flags=0, col_off=1, keys_off=2, fill=FILLS[0], ws_byte=None):
        self.w, self.fill, self.flags, self.capacity = Watch(fill), fill, flags, capacity
        w = self.w
        col = np.asarray(col, dtype=U)
        d_col = w.col(col.size, col_off, data=col, freeze=True)
        d_count = u64_word(w, count) if count is not None else None
        self.d_keys = w.col(capacity, keys_off)
        self.d_out_count = w.u64(1)
        self.nbytes = dn.workspace_bytes(capacity)
        self.ws = w.ws(self.nbytes)
        if ws_byte is not None:
            self.ws.fill_(ws_byte)
        rc = dn.build(ptr(d_col), col.size, ptr(d_count) if d_count is not None else None, capacity, flags, ptr(self.d_keys),
                      ptr(self.d_out_count), ptr(self.ws), self.nbytes, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        self.status = ops.workspace_status(self.ws)
        w.check()
        self.d = int(self.d_out_count.item())
        assert 0 <= self.d <= capacity
        self.keys = self.d_keys.cpu().numpy().view(U)[: self.d].copy()

    def encode(self, col, count=None, col_off=1, out_off=3, misses=True, fill=None):
        """one dbench_dict_encode_u32 through this workspace -> (codes cut to m, the miss word or None)"""
        fill = self.fill if fill is None else fill
        w = Watch(fill)
        col = np.asarray(col, dtype=U)
        d_col = w.col(col.size, col_off, data=col, freeze=True)
        d_count = u64_word(w, count) if count is not None else None
        d_out = w.col(col.size, out_off)
        d_miss = w.u64(1) if misses else None
        frozen_ws = self.ws.clone()
        rc = dn.encode(ptr(d_col), col.size, ptr(d_count) if d_count is not None else None, ptr(d_out),
                       ptr(d_miss) if misses else None, ptr(self.ws), self.nbytes, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        w.check()
        self.w.check()
        assert torch.equal(self.ws, frozen_ws), "encode wrote the dictionary's workspace"
        m = dm.length(count, col.size)
        out = d_out.cpu().numpy().view(U)
        assert (out[m:] == U(fill)).all(), "entries behind the count were written"
        return out[:m].copy(), (int(d_miss.item()) if misses else None)


def expect(col, capacity, count=None, flags=0, **how):
    """build against the model, then the encode of the build column itself: every row's code names its value"""
    col = np.asarray(col, dtype=U)
    want_keys, want_st = dm.build(col, capacity, count, flags)
    b = Built(col, capacity, count, flags, **how)
    assert b.status == want_st, (b.status, want_st)
    assert b.d == want_keys.size and np.array_equal(b.keys, want_keys), (b.d, want_keys.size)
    codes, misses = b.encode(col, count, col_off=how.get("col_off", 1))
    want_codes, want_misses = dm.encode(want_keys, col, count, flags)
    assert np.array_equal(codes, want_codes) and misses == want_misses
    if want_st == 0:
        assert misses == 0 and np.array_equal(want_keys[codes], col[: codes.size])
    return b


def some_column(n, distinct, rng):
    """n rows over `distinct` values from all over the 32 bits, the four ends of the number lines among them"""
    values = np.unique(np.r_[EDGES, rng.integers(0, 1 << 32, distinct, dtype=np.uint64).astype(U)])
    values = rng.permutation(values)[:distinct]
    return values[rng.integers(0, values.size, n)] if n else np.zeros(0, U)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_counts_and_alignments(n):
    rng = np.random.default_rng(n)
    col = some_column(n, 37, rng)
    counts = (None, 0, n // 2, max(n - 1, 0), n, n + 7, (1 << 32) + 1, (1 << 64) - 1)
    for i, count in enumerate(counts):
        flags = dn.SIGNED if i % 2 else 0
        for capacity in ((64, LDS_CAPACITY + 1) if i % 4 == 0 else (64,)):
            expect(col, capacity, count, flags, col_off=i % 4, keys_off=(i + 1) % 4, fill=FILLS[i % 2])


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_number_of_distinct_values_around_the_capacity(capacity):
    rng = np.random.default_rng(capacity)
    absent = np.r_[EDGES, rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(U)]
    for i, d in enumerate(sorted({0, 1, 2, capacity - 1, capacity, capacity + 1})):
        flags = dn.SIGNED if i % 2 else 0
        values = rng.permutation(np.unique(np.r_[EDGES, rng.integers(0, 1 << 32, d + 8, dtype=np.uint64).astype(U)]))[:d]
        col = rng.permutation(np.r_[values, values[rng.integers(0, max(d, 1), d + 3)]]) if d else np.zeros(0, U)
        b = expect(col, capacity, None, flags, col_off=i % 4, keys_off=(i + 2) % 4, fill=FILLS[i % 2])
        assert b.status == (dm.TABLE_FULL if d > capacity else 0) and b.d == (0 if d > capacity else d)
        # a column of present and absent values, its miss count, and a second encode of the same dictionary
        probe = rng.permutation(np.r_[col[: 200], absent])
        want, want_misses = dm.encode(b.keys, probe, None, flags)
        for out_off in (0, 1):
            codes, misses = b.encode(probe, col_off=(i + out_off) % 4, out_off=out_off, misses=bool(out_off))
            assert np.array_equal(codes, want) and misses == (want_misses if out_off else None)
        if d > capacity:
            assert (want == dm.MISS).all()  # unusable until the next build


def test_key_shapes():
    rng = np.random.default_rng(5)
    n = 2 * ENCODE_TILE + 3
    for i, key in enumerate((0, 0xFFFFFFFF, 0x80000000, 12345)):  # all rows one key
        for capacity in (1, LDS_CAPACITY + 1):
            b = expect(np.full(n, key, U), capacity, flags=dn.SIGNED if i % 2 else 0, col_off=i % 4, fill=FILLS[i % 2])
            assert b.d == 1 and b.keys[0] == key
    distinct = rng.permutation(np.unique(rng.integers(0, 1 << 32, n + 100, dtype=np.uint64).astype(U)))[:n]  # all keys distinct
    for flags in (0, dn.SIGNED):
        assert expect(distinct, n, flags=flags, col_off=2).d == n
        assert expect(distinct[:LDS_CAPACITY], LDS_CAPACITY, flags=flags, col_off=3).d == LDS_CAPACITY
    for flags, want in ((0, [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]), (dn.SIGNED, [0x80000000, 0xFFFFFFFF, 0, 0x7FFFFFFF])):
        for capacity in (4, 5, LDS_CAPACITY + 1):
            b = expect(rng.permutation(np.repeat(EDGES, 70)), capacity, flags=flags)
            assert b.keys.tolist() == want
        assert expect(np.repeat(EDGES, 3), 3, flags=flags).status == dm.TABLE_FULL


@pytest.mark.parametrize("capacity", (8, 64))
def test_keys_that_share_one_home_slot_and_wrap_past_the_tables_end(capacity):
    """built against the stated hash: `capacity` keys (and one more) whose home is the third slot from the end, so the chain
    runs over the end of the table and on from slot 0"""
    slots = dm.slots(capacity)
    keys = dm.colliding_keys(capacity, slots - 3, capacity + 1)
    assert ((dm.hash32(keys) & U(slots - 1)) == slots - 3).all() and capacity > 3
    rng = np.random.default_rng(capacity)
    for flags in (0, dn.SIGNED):
        col = rng.permutation(np.repeat(keys[:capacity], 5))
        b = expect(col, capacity, flags=flags, fill=FILLS[flags])
        assert b.status == 0 and b.d == capacity
        other = dm.colliding_keys(capacity, slots - 3, capacity + 40)[capacity:]  # the same home, absent: the whole chain is walked
        codes, misses = b.encode(np.r_[other, keys[:capacity]])
        assert (codes[: other.size] == dm.MISS).all() and misses == other.size
        assert np.array_equal(b.keys[codes[other.size:]], keys[:capacity])
        full = expect(rng.permutation(np.repeat(keys, 5)), capacity, flags=flags, fill=FILLS[1 - flags])  # one key beyond
        assert full.status == dm.TABLE_FULL and full.d == 0


def test_a_workspace_that_held_anything_and_one_that_no_build_filled():
    rng = np.random.default_rng(9)
    col = some_column(5000, 300, rng)
    for byte in (0x00, 0xFF, 0x5A):
        for capacity in (300, LDS_CAPACITY + 1):
            expect(col, capacity, ws_byte=byte, fill=FILLS[byte & 1])
    # build after build on one workspace: a failed one, then a good one of another order
    plan = ops.Dictionary(col.size, 300)
    d_col = torch.from_numpy(col.view(np.int32)).cuda()
    for signed in (False, True, False):
        plan.build(d_col[:20], signed=signed)
        small = plan.result().cpu().numpy().view(U)
        assert np.array_equal(small, dm.ordered(col[:20], dm.SIGNED if signed else 0))
        plan.capacity, keep = 10, plan.capacity  # (the same workspace, a smaller dictionary in it)
        plan.build(d_col, signed=signed)
        assert plan.status() == dm.TABLE_FULL and int(plan.count_dev.item()) == 0
        assert bool((plan.encode(d_col) == -1).all())
        plan.capacity = keep
        plan.build(d_col, signed=signed)
        assert plan.status() == 0
        codes = plan.encode(d_col).cpu().numpy().view(U)
        assert np.array_equal(plan.result().cpu().numpy().view(U)[codes], col)
    # encode through bytes that no build wrote: every row misses, nothing is read outside them
    w = Watch(FILLS[0])
    for fill_byte in (None, 0x00, 0xFF):
        ws = w.ws(dn.workspace_bytes(64))
        if fill_byte is not None:
            ws.fill_(fill_byte)
        d_in, d_out, d_miss = w.col(777, 1, data=col[:777], freeze=True), w.col(777, 2), w.u64(1)
        assert dn.encode(ptr(d_in), 777, None, ptr(d_out), ptr(d_miss), ptr(ws), ws.numel(), stream()) == 0
        torch.cuda.synchronize()
        assert bool((d_out == -1).all()) and int(d_miss.item()) == 777
    w.check()


def test_encodes_on_several_streams_share_one_dictionary():
    rng = np.random.default_rng(13)
    col = some_column(50000, 3000, rng)
    d_col = torch.from_numpy(col.view(np.int32)).cuda()
    plan = ops.Dictionary(col.size, 3000)
    plan.build(d_col)
    keys = plan.result().cpu().numpy().view(U)
    probes = [rng.permutation(np.r_[col[:20000], rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(U)]) for _ in range(3)]
    d_probes = [torch.from_numpy(p.view(np.int32)).cuda() for p in probes]
    misses = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in probes]
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream() for _ in probes], []
    for s, p, m in zip(streams, d_probes, misses):
        with torch.cuda.stream(s):
            outs.append(plan.encode(p, misses=m))
    torch.cuda.synchronize()
    for p, o, m in zip(probes, outs, misses):
        want, want_misses = dm.encode(keys, p)
        assert np.array_equal(o.cpu().numpy().view(U), want) and int(m.item()) == want_misses > 0
    assert plan.status() == 0


# ---- combine ------------------------------------------------------------------------------------------------------------
def call_combine(outer, inner, outer_card, inner_card, count=None, offs=(1, 2, 3), alias=False, fill=FILLS[0]):
    """one dbench_dict_combine_u32 on guarded buffers -> (out cut to m, status); alias: out is outer itself"""
    w = Watch(fill)
    outer, inner = np.asarray(outer, dtype=U), np.asarray(inner, dtype=U)
    n = outer.size
    d_outer = w.col(n, offs[0], data=outer, freeze=not alias)
    d_inner = w.col(n, offs[1], data=inner, freeze=True)
    d_out = d_outer if alias else w.col(n, offs[2])
    d_count = u64_word(w, count) if count is not None else None
    d_oc, d_ic = u64_word(w, outer_card), u64_word(w, inner_card)
    ws = w.ws(256)
    rc = dn.combine(ptr(d_outer), ptr(d_inner), n, ptr(d_count) if d_count is not None else None, ptr(d_oc), ptr(d_ic), ptr(d_out),
                    ptr(ws), 256, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    m = dm.length(count, n)
    out = d_out.cpu().numpy().view(U)
    assert np.array_equal(out[m:], outer[m:] if alias else np.full(n - m, fill, U)), "entries behind the count were written"
    return out[:m].copy(), st


def expect_combine(outer, inner, outer_card, inner_card, count=None, **how):
    want, want_st = dm.combine(outer, inner, outer_card, inner_card, count)
    got, st = call_combine(outer, inner, outer_card, inner_card, count, **how)
    assert st == want_st and np.array_equal(got, want), (st, want_st)
    return got, st


def codes_below(card, n, rng, misses=True):
    c = rng.integers(0, card, n, dtype=np.uint64).astype(U)
    if n:
        c[rng.integers(0, n, 2)] = card - 1  # the largest code occurs
    if misses and n > 4:
        c[rng.integers(0, n, n // 7)] = dm.MISS
    return c


@pytest.mark.parametrize("n", (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2051))
def test_combine_sizes_counts_alignments_and_aliasing(n):
    rng = np.random.default_rng(100 + n)
    for i, count in enumerate((None, 0, n // 2, n, n + 7, (1 << 64) - 1)):
        oc, ic = (1000, 77) if i % 2 else (65537, 65535)  # 65537 x 65535 = 0xFFFFFFFF exactly: legal
        outer, inner = codes_below(oc, n, rng), codes_below(ic, n, rng)
        offs = (i % 4, (i + 1 + i // 4) % 4, (2 * i + 1) % 4)
        got, st = expect_combine(outer, inner, oc, ic, count, offs=offs, fill=FILLS[i % 2])
        assert st == 0
        expect_combine(outer, inner, oc, ic, count, offs=offs, alias=True, fill=FILLS[1 - i % 2])
        got, st = expect_combine(outer, inner, 65536, 65536, count, offs=offs, alias=bool(i % 2))  # 2^32: one too many
        assert st == dm.KEY_RANGE and (got == dm.MISS).all()


def test_combine_at_the_edge_of_32_bits():
    rng = np.random.default_rng(3)
    outer, inner = codes_below(65537, 3000, rng, misses=False), codes_below(65535, 3000, rng, misses=False)
    outer[:2], inner[:2] = 65536, 65534
    got, st = expect_combine(outer, inner, 65537, 65535)
    assert st == 0 and got[0] == 0xFFFFFFFE and (got != dm.MISS).all()
    outer[5], inner[6] = dm.MISS, dm.MISS
    got, st = expect_combine(outer, inner, 65537, 65535)
    assert (got == dm.MISS).sum() == 2 and got[5] == got[6] == dm.MISS
    for oc, ic in ((1 << 32, 1), (1, 1 << 32), (0xFFFFFFFF, 2), (1 << 63, 1 << 63), ((1 << 64) - 1, (1 << 64) - 1), (3, (1 << 32) // 3 + 1)):
        assert expect_combine(outer, inner, oc, ic)[1] == dm.KEY_RANGE, (oc, ic)
    for oc, ic in ((0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (0, 1 << 63), (3, 0xFFFFFFFF // 3)):
        assert expect_combine(outer % U(min(oc, 1 << 31) or 1), inner % U(min(ic, 1 << 31)), oc, ic)[1] == 0, (oc, ic)


# ---- the tensor API -----------------------------------------------------------------------------------------------------
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(U)


def test_ops_factorize_and_dictionary():
    rng = np.random.default_rng(21)
    col = some_column(733, 90, rng)
    for signed in (False, True):
        view = col.view(np.int32) if signed else col
        uniques, inverse = np.unique(view, return_inverse=True)
        codes, got = ops.factorize(dev(col), signed=signed)
        assert np.array_equal(host(got), uniques.view(U)) and np.array_equal(host(codes), inverse.astype(U))
        codes, got = ops.factorize(dev(col), signed=signed, capacity=uniques.size)  # the exact bound
        assert np.array_equal(host(codes), inverse.astype(U))
        with pytest.raises(ops._capi.DbhipError, match="0x4"):
            ops.factorize(dev(col), signed=signed, capacity=uniques.size - 1)
    codes, got = ops.factorize(dev(np.zeros(0, U)))
    assert codes.numel() == 0 and got.numel() == 0
    plan = ops.Dictionary(col.size, 128)
    plan.build(dev(col))
    probe = np.r_[col[:100], np.array([1, 2, 3], U)]
    misses = torch.zeros(1, dtype=torch.int64, device="cuda")
    codes = plan.encode(dev(probe), misses=misses)
    want, want_misses = dm.encode(np.unique(col), probe)
    assert np.array_equal(host(codes), want) and int(misses.item()) == want_misses and plan.count() == np.unique(col).size
    back = host(plan.decode(codes, fill=-5))
    assert np.array_equal(back, np.where(want == dm.MISS, U(0xFFFFFFFB), probe))
    count = torch.tensor([50], dtype=torch.int64, device="cuda")  # the length on the device
    out = torch.full((probe.size,), 77, dtype=torch.int32, device="cuda")
    assert plan.encode(dev(probe), count=count, out=out) is out
    assert np.array_equal(host(out)[:50], want[:50]) and bool((out[50:] == 77).all())


def tuples_of(cols):
    return np.stack([c.astype(np.int64) for c in cols], axis=1)


def test_ops_encode_columns_orders_rows_as_tuples():
    rng = np.random.default_rng(23)
    n = 611
    for k in (2, 3):
        cols = [some_column(n, d, rng) for d in (7, 13, 5)[:k]]
        codes, uniques, card = ops.encode_columns([dev(c) for c in cols])
        assert card == int(np.prod([np.unique(c).size for c in cols]))
        assert all(np.array_equal(host(u), np.unique(c)) for u, c in zip(uniques, cols))
        rows, inverse = np.unique(tuples_of(cols), axis=0, return_inverse=True)
        got = host(codes)
        assert got.max() < card
        assert np.array_equal(np.unique(got, return_inverse=True)[1], inverse.reshape(-1))  # the same order, the same ties
    signed = [c.view(np.int32) for c in cols]
    codes, uniques, card = ops.encode_columns([dev(c) for c in cols], signed=True)
    rows, inverse = np.unique(tuples_of(signed), axis=0, return_inverse=True)
    assert np.array_equal(np.unique(host(codes), return_inverse=True)[1], inverse.reshape(-1))
    wide = [np.arange(70000, dtype=U)] * 2  # 70000 x 70000 composites do not fit 32 bits
    with pytest.raises(ops._capi.DbhipError, match="do not fit"):
        ops.encode_columns([dev(c) for c in wide])


@pytest.mark.parametrize("dense_groups", (None, 1))
def test_ops_groupby_columns_against_numpy(dense_groups):
    """None: the dense group-by over the composite; 1: no cardinality fits, the hash group-by and a sort"""
    rng = np.random.default_rng(29)
    n = 777
    for k in (1, 2, 3):
        cols = [some_column(n, d, rng) for d in (11, 6, 4)[:k]]
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)  # sums wrap at 32 bits
        keys, sums, counts = ops.groupby_columns([dev(c) for c in cols], dev(vals), dense_groups=dense_groups)
        rows, inverse, want_counts = np.unique(tuples_of(cols), axis=0, return_inverse=True, return_counts=True)
        want_sums = np.zeros(rows.shape[0], np.uint64)
        np.add.at(want_sums, inverse.reshape(-1), vals.astype(np.uint64))
        assert len(keys) == k and all(np.array_equal(host(g), rows[:, c].astype(U)) for c, g in enumerate(keys))
        assert np.array_equal(host(sums), (want_sums & np.uint64(0xFFFFFFFF)).astype(U))
        assert np.array_equal(host(counts), want_counts.astype(U))
    keys, sums, counts = ops.groupby_columns([dev(np.zeros(0, U))] * 2, dev(np.zeros(0, U)), dense_groups=dense_groups)
    assert [t.numel() for t in keys + [sums, counts]] == [0, 0, 0, 0]


@pytest.mark.parametrize("k", (2, 3))
def test_ops_join_pairs_columns_against_a_dictionary_of_tuples(k):
    rng = np.random.default_rng(31 + k)
    nb, npr = 400, 650
    build = [some_column(nb, d, rng) for d in (9, 5, 3)[:k]]
    probe = [rng.permutation(np.r_[np.unique(b), np.array([1, 2, 3], U)])[rng.integers(0, np.unique(b).size + 3, npr)] for b in build]
    by_tuple = {}
    for r, t in enumerate(zip(*(b.tolist() for b in build))):
        by_tuple.setdefault(t, []).append(r)
    matches = [by_tuple.get(t, []) for t in zip(*(p.tolist() for p in probe))]
    assert any(not m for m in matches) and any(len(m) > 1 for m in matches)  # probe values absent from the build side too
    for left_outer in (False, True):
        want = [(b, r) for r, m in enumerate(matches) for b in (m or ([0xFFFFFFFF] if left_outer else []))]
        build_rows, probe_rows = ops.join_pairs_columns([dev(b) for b in build], [dev(p) for p in probe], left_outer=left_outer)
        got = sorted(zip(host(build_rows).tolist(), host(probe_rows).tolist()), key=lambda p: (p[1], p[0]))
        assert got == sorted(want, key=lambda p: (p[1], p[0]))
        assert np.array_equal(host(probe_rows), np.sort(host(probe_rows)))  # probe rows ascending
