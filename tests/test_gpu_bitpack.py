"""Bit-packed columns on the GPU (dwarf_bench_amd/host/bitpack.cpp through bitpack_native and ops): every result is
compared bit for bit with the numpy model (tests/bitpack_model.py), the filter also with dbench_select_range_u32 on the
decoded column.  The raw entry points run on guarded buffers (tests/guard_testlib.py): the packed words in a buffer of
exactly dbench_bitpack_words words, columns, lists and outputs off their 16-byte boundaries, guard words around
everything, the words and entries behind a count untouched, the workspace holding anything."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import bitpack_native as bn
from dwarf_bench_amd import ops
from tests import bitpack_model as bm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

SEG, TILE = bn.SEGMENT_ROWS, bn.TILE_ROWS
# nothing and one, around a group of 32 rows and a 16-byte chunk's 128, around pack's tile and the segment of unpack and
# select (a workgroup holds four tiles, two segments), and several workgroups with a ragged rest
ROW_COUNTS = (0, 1, 31, 32, 33, 127, 128, 129, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 4 * TILE + 5,
              (1 << 16) + 13)
WIDTHS = (1, 7, 8, 12, 17, 31, 32)
MID = SEG + 1234  # every width runs at this size
U = np.uint32
KINDS = ("random", "zeros", "ones")


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_codes(n, width, kind, seed=0):
    if kind == "zeros":
        return np.zeros(n, U)
    if kind == "ones":
        return np.full(n, bm.mask(width), U)
    return np.random.default_rng(1000 * width + seed).integers(0, 1 << width, n, dtype=np.uint64).astype(U)


def device_count(w, count):
    if count is None:
        return None
    d = w.u64(1)
    d.fill_(count - (1 << 64) if count >> 63 else count)
    w.freeze(d)
    return d


def call_pack(col, width, base=0, count=None, col_off=0, fill=FILLS[0], ws_byte=None, spare=0):
    """one dbench_bitpack_pack_u32 on guarded buffers -> (out_packed afterwards, status).  out_packed holds exactly
    words(capacity) + spare words and starts out as the guard fill."""
    w = Watch(fill)
    capacity = int(col.size)
    d_col = w.col(capacity, col_off, data=col, freeze=True)
    d_count = device_count(w, count)
    d_out = w.col(bn.words(capacity, width) + spare, 0)
    ws = w.ws(bn.workspace_bytes(0))
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = bn.pack(ptr(d_col), capacity, ptr(d_count) if d_count is not None else None, width, base, ptr(d_out), ptr(ws),
                 ws.numel(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return d_out.cpu().numpy().view(U).copy(), st


def expect_pack(col, width, base=0, count=None, fill=FILLS[0], **how):
    got, st = call_pack(col, width, base, count, fill=fill, **how)
    want, want_st = bm.pack(col, width, base, count, before=np.full(got.size, fill, U))
    m = bm.length(count, col.size)
    assert st == want_st, (st, want_st)
    assert np.array_equal(got[: bm.words(m, width)], want[: bm.words(m, width)]), "packed words differ"
    assert (got[bm.words(m, width):] == U(fill)).all(), "words behind the packed form were written"
    bits = np.unpackbits(got[: bm.words(m, width)].view(np.uint8), bitorder="little")
    assert not bits[m * width:].any(), "padding bits are not zero"
    return got[: bm.words(m, width)], st


def call_unpack(packed, n_rows, width, base=0, rows=None, count=None, flags=0, fill_word=0x0F1E2D3C, list_off=0, out_off=0,
                fill=FILLS[0], ws_byte=None):
    """one dbench_bitpack_unpack_u32 on guarded buffers -> (out afterwards, status); the packed words sit in a buffer of
    exactly their size"""
    w = Watch(fill)
    d_packed = w.col(bn.words(n_rows, width), 0, data=packed[: bn.words(n_rows, width)], freeze=True)
    entries = n_rows if rows is None else int(rows.size)
    d_rows = w.col(entries, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = device_count(w, count)
    d_out = w.col(entries, out_off)
    ws = w.ws(bn.workspace_bytes(0))
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = bn.unpack(ptr(d_packed) if n_rows else None, n_rows, width, base, ptr(d_rows) if d_rows is not None else None,
                   ptr(d_count) if d_count is not None else None, entries if rows is not None else 0, flags, fill_word,
                   ptr(d_out), ptr(ws), ws.numel(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return d_out.cpu().numpy().view(U).copy(), st


def expect_unpack(packed, n_rows, width, base=0, rows=None, count=None, flags=0, fill_word=0x0F1E2D3C, fill=FILLS[0], **how):
    got, st = call_unpack(packed, n_rows, width, base, rows, count, flags, fill_word, fill=fill, **how)
    want, want_st = bm.unpack(packed, n_rows, width, base, rows, count, flags, fill_word, before=np.full(got.size, fill, U))
    assert st == want_st, (st, want_st)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} entries differ"
    return st


def call_select(packed, n_rows, width, base, lo, hi, rows=None, count=None, flags=0, list_off=0, out_off=0, fill=FILLS[0],
                ws_byte=None, want_rows=True):
    """one dbench_bitpack_select_range_u32 on guarded buffers -> (the kept row ids or None, *out_count, status)"""
    w = Watch(fill)
    d_packed = w.col(bn.words(n_rows, width), 0, data=packed[: bn.words(n_rows, width)], freeze=True)
    candidates = n_rows if rows is None else int(rows.size)
    d_rows = w.col(candidates, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = device_count(w, count)
    d_out = w.col(candidates, out_off) if want_rows else None
    d_total = w.u64(1)
    nbytes = bn.workspace_bytes(candidates)
    ws = w.ws(nbytes)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    rc = bn.select_range(ptr(d_packed) if n_rows else None, n_rows, width, base, ptr(d_rows) if d_rows is not None else None,
                         ptr(d_count) if d_count is not None else None, candidates if rows is not None else 0, lo, hi, flags,
                         ptr(d_out) if d_out is not None else None, ptr(d_total), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    total = int(d_total.item())
    if d_out is None:
        return None, total, st
    out = d_out.cpu().numpy().view(U)
    assert 0 <= total <= candidates and (out[total:] == U(fill)).all(), "entries behind the count were written"
    return out[:total].copy(), total, st


def plain_select(values, lo, hi, rows=None, flags=0):
    """dbench_select_range_u32 on the decoded column, through ops (strict off: a row id outside is just dropped)"""
    col = torch.from_numpy(values.view(np.int32)).cuda()
    plan = ops.SelectRows(values.size if rows is None else rows.size)
    signed = bool(flags & bm.SIGNED)
    as_int = lambda v: v - (1 << 32) if signed and v >> 31 else v  # noqa: E731
    plan.launch(col, as_int(lo), as_int(hi), rows=None if rows is None else torch.from_numpy(rows.view(np.int32)).cuda(),
                signed=signed, negate=bool(flags & bm.NEGATE))
    return plan.result(strict=False).cpu().numpy().view(U)


def expect_select(packed, n_rows, width, base, lo, hi, rows=None, count=None, flags=0, values=None, **how):
    got, total, st = call_select(packed, n_rows, width, base, lo, hi, rows, count, flags, **how)
    want, want_st = bm.select_range(packed, n_rows, width, base, lo, hi, rows, count, flags)
    assert (st, total) == (want_st, want.size), (st, want_st, total, want.size)
    assert np.array_equal(got, want), "kept row ids differ"
    if values is not None and count is None:  # the entry point on the decoded column says the same
        assert np.array_equal(got, plain_select(values, lo, hi, rows, flags))
    return got


def bounds(width, base, share):
    """[lo, hi] in the value domain that keeps about `share` of uniform codes: nothing for 0 (lo > hi), every row for 1 (no
    wrap: base + 2^width <= 2^32 wherever this is used)"""
    top = bm.mask(width)
    if share == 0:
        return (base + top) & 0xFFFFFFFF, base
    if share == 1.0:
        return base, base + top
    lo = top // 4
    return base + lo, base + min(top, lo + max(int(share * (top + 1)) - 1, 0))


# ---- pack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_pack_every_row_count(n):
    for i, width in enumerate(WIDTHS):
        kind = KINDS[(i + n) % 3]
        # a base of zero, an ordinary one, and one that makes v - base wrap below zero for the values stored
        base = (0, 1000, 0xFFFFFF00)[(i + n // 2) % 3] if width < 32 else (0, 0x80000001)[n % 2]
        col = make_codes(n, width, kind, n) + U(base)  # mod 2^32
        packed, st = expect_pack(col, width, base, col_off=(i + n) % 4, fill=FILLS[i % 2])
        assert st == 0 and np.array_equal(bm.decode(packed, n, width, base), col)


@pytest.mark.parametrize("width", range(1, 33))
def test_pack_and_unpack_every_width(width):
    for kind in KINDS:
        base = 0 if width == 32 else 0xFFFFFFF0  # (wraps)
        col = make_codes(MID, width, kind) + U(base)
        packed, st = expect_pack(col, width, base, col_off=width % 4)
        assert st == 0
        assert expect_unpack(packed, MID, width, base, out_off=(width + 1) % 4) == 0
    rows = np.random.default_rng(width).integers(0, MID, 3000, dtype=np.uint64).astype(U)
    assert expect_unpack(packed, MID, width, base, rows=rows, list_off=width % 4, out_off=(width + 2) % 4) == 0


def test_pack_a_row_that_does_not_fit_raises_and_keeps_its_low_bits():
    for width in (1, 7, 12, 31):
        col = make_codes(TILE + 77, width, "random")
        col[[5, TILE + 3]] = [0xFFFFFFFF, 1 << width]  # DBENCH_DICT_MISS, and the first value past the width
        packed, st = expect_pack(col, width)
        assert st == bm.KEY_RANGE
        assert list(bm.unpack_codes(packed, col.size, width)[[5, TILE + 3]]) == [bm.mask(width), 0]
        col[[5, TILE + 3]] = 0
        assert expect_pack(col, width)[1] == 0
    assert expect_pack(np.array([0xFFFFFFFF, 0, 1 << 31], U), 32)[1] == 0  # every value fits in 32 bits


@pytest.mark.parametrize("capacity", (33, TILE + 1, 2 * SEG + 1))
def test_pack_device_count_and_the_words_behind_it(capacity):
    for i, width in enumerate((1, 12, 17, 32)):
        col = make_codes(capacity, width, "random", 7)
        for count in (0, 1, capacity // 2, capacity - 1, capacity, capacity + 1, (1 << 40) + 3, (1 << 64) - 1):
            expect_pack(col, width, count=count, spare=8, col_off=i, fill=FILLS[(i + count) % 2])


# ---- unpack -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_unpack_dense_every_row_count(n):
    for i, width in enumerate(WIDTHS):
        base = (0, 12345, 0xFFFFFFF0)[i % 3] if width < 32 else 7
        packed = bm.pack_codes(make_codes(n, width, KINDS[(i + n + 1) % 3], n), width)
        assert expect_unpack(packed, n, width, base, out_off=(i + n) % 4, fill=FILLS[i % 2]) == 0


def lists(m, n_rows, rng):
    inside = rng.integers(0, max(n_rows, 1), m, dtype=np.uint64).astype(U)
    yield "ascending", np.sort(inside), 0
    yield "shuffled", inside, 0
    yield "repeating", np.full(m, n_rows - 1 if n_rows else 0, U), 0 if n_rows else bm.KEY_RANGE
    for bad in (n_rows, 0x80000000, 0xFFFFFFFF):
        some = inside.copy()
        some[rng.integers(0, m, max(m // 7, 1))] = bad
        yield f"some {bad:#x}", some, bm.KEY_RANGE


@pytest.mark.parametrize("m", (1, 63, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 3))
def test_unpack_through_lists_at_every_alignment(m):
    n_rows = 5003
    rng = np.random.default_rng(m)
    kinds = list(lists(m, n_rows, rng))
    seen = set()
    for list_off in range(4):
        for out_off in range(4):
            i = 4 * list_off + out_off
            width = WIDTHS[i % len(WIDTHS)]
            base = 0 if width == 32 else 99
            packed = bm.pack_codes(make_codes(n_rows, width, "random", i), width)
            name, rows, want_st = kinds[i % len(kinds)]
            st = expect_unpack(packed, n_rows, width, base, rows=rows, list_off=list_off, out_off=out_off, fill=FILLS[i % 2])
            assert st == want_st, name
            seen.add(st)
    assert seen == {0, bm.KEY_RANGE}


def test_unpack_no_row_id_empty_column_and_count():
    n_rows, width, base = 777, 12, 5
    packed = bm.pack_codes(make_codes(n_rows, width, "random"), width)
    rows = np.array([3, bm.NO_ROW, 776, bm.NO_ROW, 0], U)
    assert expect_unpack(packed, n_rows, width, base, rows=rows) == bm.KEY_RANGE
    assert expect_unpack(packed, n_rows, width, base, rows=rows, flags=bn.OUTER) == 0
    assert expect_unpack(packed, n_rows, width, base, rows=np.r_[rows, U(777)], flags=bn.OUTER) == bm.KEY_RANGE
    # an empty column: every entry is filled, nothing is read
    empty = np.zeros(0, U)
    assert expect_unpack(empty, 0, width, base, rows=np.array([0, 1, bm.NO_ROW], U)) == bm.KEY_RANGE
    assert expect_unpack(empty, 0, width, base, rows=np.full(SEG + 5, bm.NO_ROW, U), flags=bn.OUTER) == 0
    assert expect_unpack(empty, 0, width, base) == 0
    # the entries behind a device count stay as they were, and a bad id behind it does not count
    rows = np.r_[np.random.default_rng(1).integers(0, n_rows, SEG + 100, dtype=np.uint64).astype(U), U(n_rows)]
    for count in (0, 1, 64, SEG, SEG + 100, SEG + 101, 1 << 40):
        want = bm.KEY_RANGE if count > SEG + 100 else 0
        assert expect_unpack(packed, n_rows, width, base, rows=rows, count=count, list_off=count % 4, out_off=1) == want


# ---- select -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_select_dense_every_row_count(n):
    for i, width in enumerate(WIDTHS):
        base = 0 if width == 32 else (0, 1 << 20)[i % 2]
        values = make_codes(n, width, "random", n) + U(base)
        packed = bm.pack_codes(values - U(base), width)
        share = (0.5, 0.01, 1.0, 0)[(i + n) % 4]
        lo, hi = bounds(width, base, share)
        negate = (i + n // 3) % 2 == 1
        got = expect_select(packed, n, width, base, lo, hi, flags=bn.NEGATE if negate else 0, values=values,
                            out_off=(i + n) % 4, fill=FILLS[i % 2])
        if share in (0, 1.0):
            assert got.size == (n if (share == 1.0) != negate else 0)


@pytest.mark.parametrize("width", range(1, 33))
def test_select_every_width_every_share(width):
    base = 0 if width == 32 else 0x1000
    values = make_codes(MID, width, "random", 5) + U(base)
    packed = bm.pack_codes(values - U(base), width)
    kept = []
    for share in (0, 0.01, 0.5):
        lo, hi = bounds(width, base, share)
        kept.append(expect_select(packed, MID, width, base, lo, hi, values=values).size)
    kept.append(expect_select(packed, MID, width, base, 0, 0xFFFFFFFF, values=values).size)  # the full range
    kept.append(expect_select(packed, MID, width, base, 0, 0xFFFFFFFF, flags=bn.NEGATE, values=values).size)
    assert kept[0] == 0 and kept[3] == MID and kept[4] == 0 and kept[0] <= kept[1] <= kept[2] <= kept[3]
    if width >= 10:
        assert 0 < kept[1] < 0.03 * MID and 0.4 * MID < kept[2] < 0.6 * MID


def test_select_signed_values_and_the_count_alone():
    n, width = SEG + 500, 9
    values = np.random.default_rng(2).integers(-200, 300, n).astype(np.int32).view(U)  # int32 values on both sides of zero
    base = int(values.view(np.int32).min()) & 0xFFFFFFFF
    packed, st = bm.pack(values, width, base)
    assert st == 0
    for lo, hi in ((-100, 100), (-200, -1), (0, 299), (100, -100), (-(1 << 31), (1 << 31) - 1)):
        for flags in (bn.SIGNED, bn.SIGNED | bn.NEGATE):
            got = expect_select(packed, n, width, base, lo & 0xFFFFFFFF, hi & 0xFFFFFFFF, flags=flags, values=values)
            v = values.view(np.int32)
            inside = (v >= lo) & (v <= hi)
            assert np.array_equal(got, np.nonzero(~inside if flags & bn.NEGATE else inside)[0])
        unsigned = expect_select(packed, n, width, base, lo & 0xFFFFFFFF, hi & 0xFFFFFFFF, values=values)
        _, total, st = call_select(packed, n, width, base, lo & 0xFFFFFFFF, hi & 0xFFFFFFFF, want_rows=False)
        assert (total, st) == (unsigned.size, 0)  # out_rows == NULL: the count alone


@pytest.mark.parametrize("m", (1, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 3))
def test_select_through_lists(m):
    n_rows = 6007
    rng = np.random.default_rng(m)
    for i, width in enumerate(WIDTHS):
        base = 0 if width == 32 else 31
        values = make_codes(n_rows, width, "random", i) + U(base)
        packed = bm.pack_codes(values - U(base), width)
        rows = rng.integers(0, n_rows, m, dtype=np.uint64).astype(U)  # unsorted, with repeats
        lo, hi = bounds(width, base, (0.5, 0.01, 1.0)[i % 3])
        flags = (0, bn.NEGATE)[i % 2]
        expect_select(packed, n_rows, width, base, lo, hi, rows=rows, flags=flags, values=values, list_off=i % 4,
                      out_off=(i + 1) % 4)
        bad = rows.copy()
        bad[rng.integers(0, m, max(m // 9, 1))] = (n_rows, 0xFFFFFFFF, 0x80000000)[i % 3]  # never kept, not even negated
        _, total, st = call_select(packed, n_rows, width, base, lo, hi, rows=bad, flags=flags, want_rows=False)
        got = expect_select(packed, n_rows, width, base, lo, hi, rows=bad, flags=flags, values=values, list_off=(i + 2) % 4)
        assert st == bm.KEY_RANGE and total == got.size and (got < n_rows).all()
        for count in (0, m // 2, m, m + 5):
            expect_select(packed, n_rows, width, base, lo, hi, rows=bad, count=count, flags=flags, out_off=count % 4)
    empty = np.zeros(0, U)
    assert expect_select(empty, 0, 8, 0, 0, 0xFFFFFFFF, rows=np.array([0, 5], U)).size == 0  # an empty column keeps nothing


def test_select_second_round_of_the_scan():
    """1025 segments: the scan (launch_rowlist_scan, 1024 counts a round) runs a second round, and the one row of the last
    segment lands behind everything the first round counted.  Width 1, a 512 KiB column; the kept rows lie in the first
    segment, in segment 1023 and in segment 1024, mirrored, so that the reversed list keeps entries in the same three"""
    n, width, base = 1024 * SEG + 1, 1, 7
    front = np.array([0, 5, SEG - 1], np.int64)
    ones = np.r_[front, n - 1 - front]
    assert sorted(set(ones // SEG)) == [0, 1023, 1024] and (ones // SEG == 1024).sum() == 1
    codes = np.zeros(n, U)
    codes[ones] = 1
    packed = bm.pack_codes(codes, width)
    assert packed.size * 4 == 512 * 1024 + 16 and bn.workspace_bytes(n) >= 256 + 2 * 4 * 1025
    got = expect_select(packed, n, width, base, base + 1, base + 1, out_off=1)
    assert np.array_equal(got, np.sort(ones).astype(U))
    rows = np.arange(n - 1, -1, -1, dtype=np.int64).astype(U)  # the same length, back to front
    got = expect_select(packed, n, width, base, base + 1, base + 1, rows=rows, list_off=3, out_off=2, fill=FILLS[1])
    assert np.array_equal(got, np.sort(ones)[::-1].astype(U))
    # (the other side of the predicate: every segment of both rounds is full but for the six rows)
    _, total, st = call_select(packed, n, width, base, base + 1, base + 1, flags=bn.NEGATE, want_rows=False)
    assert (total, st) == (n - ones.size, 0)


def test_a_dirty_workspace_changes_nothing():
    n, width, base = 2 * SEG + 77, 12, 1000
    values = make_codes(n, width, "random") + U(base)
    values_bad = values.copy()
    values_bad[9] = base - 1  # does not fit: the first call raises, the second must not inherit the status word
    rows = np.random.default_rng(4).integers(0, n, SEG + 9, dtype=np.uint64).astype(U)
    rows[[5, SEG + 2]] = [n, n + 1]  # outside the column
    lo, hi = bounds(width, base, 0.5)
    first_bad = call_pack(values_bad, width, base)
    assert first_bad[1] == bm.KEY_RANGE
    for ws_byte in (None, 0xFF, 0x02):
        p, st = call_pack(values, width, base, ws_byte=ws_byte)
        assert st == 0 and np.array_equal(p, bm.pack_codes(values - U(base), width))
        d, st = call_unpack(p, n, width, base, ws_byte=ws_byte)
        assert st == 0 and np.array_equal(d, values)
        t, st = call_unpack(p, n, width, base, rows=rows, ws_byte=ws_byte)
        assert st == bm.KEY_RANGE and np.array_equal(t, bm.unpack(p, n, width, base, rows, fill=0x0F1E2D3C)[0])
        s, total, st = call_select(p, n, width, base, lo, hi, ws_byte=ws_byte)
        assert st == 0 and np.array_equal(s, bm.select_range(p, n, width, base, lo, hi)[0])
        s, total, st = call_select(p, n, width, base, lo, hi, rows=rows, ws_byte=ws_byte)
        assert st == bm.KEY_RANGE and np.array_equal(s, bm.select_range(p, n, width, base, lo, hi, rows)[0])


# ---- the tensor front door ----------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def test_ops_pack_picks_width_and_base_and_round_trips():
    rng = np.random.default_rng(6)
    n = SEG + 321
    col = (rng.integers(0, 3000, n) + 70000).astype(U)
    pc = ops.pack(dev(col))
    assert (pc.width, pc.base, pc.n_rows) == (int(col.max() - col.min()).bit_length(), int(col.min()), n)
    assert pc.nbytes == 4 * bm.words(n, pc.width) and pc.packed.data_ptr() % 16 == 0
    assert np.array_equal(pc.packed.cpu().numpy().view(U), bm.pack(col, pc.width, pc.base)[0])
    assert np.array_equal(ops.unpack(pc).cpu().numpy().view(U), col)
    signed = rng.integers(-40, 40, n).astype(np.int32)
    ps = ops.pack(dev(signed), signed=True)
    assert (ps.width, ps.base) == (int(signed.max() - signed.min()).bit_length(), int(signed.min()) & 0xFFFFFFFF)
    assert np.array_equal(ops.unpack(ps).cpu().numpy(), signed)
    got = ops.select_range_packed(ps, -5, 5, signed=True).cpu().numpy()
    assert np.array_equal(got, np.nonzero((signed >= -5) & (signed <= 5))[0])
    one = ops.pack(dev(np.full(100, 9, U)))  # a constant column: one bit
    assert (one.width, one.base) == (1, 9) and not one.packed.any()
    none = ops.pack(dev(np.zeros(0, U)))
    assert (none.width, none.n_rows, none.nbytes) == (1, 0, 0) and ops.unpack(none).numel() == 0
    with pytest.raises(Exception, match="status"):
        ops.pack(dev(col), 8, 70000)  # 3000 values do not fit in eight bits
    with pytest.raises(ValueError, match="base"):
        ops.pack(dev(col), base=70001 + 3000)
    rows = rng.integers(0, n, 500).astype(U)
    assert np.array_equal(ops.unpack(pc, dev(rows)).cpu().numpy().view(U), col[rows])
    with pytest.raises(Exception, match="status"):
        ops.unpack(pc, dev(np.array([1, n], U)))
    assert list(ops.unpack(pc, dev(np.array([1, 0xFFFFFFFF], U)), outer=True, fill=-7).cpu().numpy()) == [int(col[1]), -7]
    count = torch.tensor([123], dtype=torch.int64, device="cuda")
    assert np.array_equal(ops.unpack(pc, dev(rows), count=count).cpu().numpy().view(U), col[rows[:123]])
    got = ops.select_range_packed(pc, 70100, 70200, rows=dev(rows)).cpu().numpy().view(U)
    assert np.array_equal(got, rows[(col[rows] >= 70100) & (col[rows] <= 70200)])


def test_select_rows_chain_mixes_packed_and_plain_columns():
    rng = np.random.default_rng(8)
    n = 2 * SEG + 99
    a, b, c = (rng.integers(0, 1 << w, n).astype(U) for w in (12, 32, 5))
    pa, pc_ = ops.pack(dev(a), 12), ops.pack(dev(c + U(100)), 5, 100)
    plan = ops.SelectRows(n)
    plan.launch(pa, 1000, 3000)                 # packed
    plan.refine(dev(b), 0, 1 << 31)             # plain
    plan.refine(pc_, 104, 120, negate=True)     # a second packed one
    got = plan.result().cpu().numpy().view(U)
    want = np.nonzero((a >= 1000) & (a <= 3000) & (b <= 1 << 31) & ~((c + 100 >= 104) & (c + 100 <= 120)))[0]
    assert got.size and np.array_equal(got, want)
    plan.launch(dev(a), 1000, 3000)  # a tensor, as before
    assert np.array_equal(plan.result().cpu().numpy().view(U), np.nonzero((a >= 1000) & (a <= 3000))[0])


def test_dictionary_codes_pack_at_its_width():
    rng = np.random.default_rng(10)
    n, cap = SEG + 50, 300
    col = rng.choice(rng.integers(0, 1 << 32, cap, dtype=np.uint64).astype(U), n)
    d = ops.Dictionary(n, cap)
    d.build(dev(col))
    codes = d.encode(dev(col))
    assert d.packed_width() == 9
    plan = ops.BitPack(n, d.packed_width())
    plan.launch(codes)
    pc = plan.result()
    keys, inverse = np.unique(col, return_inverse=True)
    assert np.array_equal(ops.unpack(pc).cpu().numpy().view(U), inverse.astype(U))
    assert np.array_equal(pc.packed.cpu().numpy().view(U), bm.pack_codes(inverse.astype(U), 9))
    missing = d.encode(dev(np.r_[col[:10], U(12345)]))  # very likely a value the dictionary does not hold: DICT_MISS
    if int(missing[-1]) == -1:
        plan.launch(missing)
        assert plan.status() == ops.DEV_KEY_RANGE
