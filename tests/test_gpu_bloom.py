"""The Bloom filter on the GPU (dwarf_bench_amd/host/bloom_filter.cpp through bloom_native): the raw entry points on guarded
buffers (tests/guard_testlib.py), every filter and every row-id list compared bit for bit with the numpy model
(tests/bloom_model.py).  Columns and lists sit off their 16-byte boundaries, guard words surround the filter, every input and
every output, the entries behind a count stay untouched, and the workspace holds anything beforehand.  Few bits per key (2
and 4) make false positives common, so that their exact set is what is compared."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import bloom_native as bl
from dwarf_bench_amd import ops
from dwarf_bench_amd import select_native as sn
from tests import bloom_model as blm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu

SEG = sn.SEGMENT_ROWS
# nothing and one, around a lane's four keys, a wave's row of 256 and a segment, several workgroups with a ragged rest
ROW_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, (1 << 16) + 13)
SEAMS = (SEG - 1, SEG, SEG + 1, 2 * SEG + 1)
WORDS = (1, 2, 3, 64, 1000, 65537)
KINDS = ("random", "equal", "dense", "reference", "special")
COUNTS = ("none", "zero", "one", "below", "at", "above", "huge")
U, W = np.uint32, np.uint64


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_keys(n, kind, seed=0, rng_seed=1):
    rng = np.random.default_rng(rng_seed + 31 * n)
    if kind == "equal":
        return np.full(n, 0xC0FFEE11, U)
    if kind == "dense":
        return np.arange(1, n + 1, dtype=U)
    if kind == "reference":
        return rng.integers(1, 10001, n).astype(U)
    if kind == "special":
        return np.array([0, seed & 0xFFFFFFFF, 0xFFFFFFFF], U)[rng.integers(0, 3, n)]
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)


def count_of(kind, capacity):
    return {"none": None, "zero": 0, "one": 1, "below": capacity // 2 + 1, "at": capacity, "above": capacity + 1,
            "huge": (1 << 40) + 9}[kind]


def device_count(w, count):
    if count is None:
        return None
    d = w.u64(1)
    d.fill_(count)
    w.freeze(d)
    return d


def _p(t):
    return ptr(t) if t is not None else None


def whole(fill, n_words):
    return np.full(n_words, (fill & 0xFFFFFFFF) * 0x100000001, W)


def call_build(col, n_words, seed=0, rows=None, count=None, flags=0, before=None, col_off=0, list_off=0, fill=FILLS[0],
               ws_byte=0xC3):
    """one dbench_bloom_build_u32 on guarded buffers -> (the filter afterwards, status).  The filter holds exactly n_words
    words and starts out as the guard fill, or as `before`"""
    w = Watch(fill)
    d_col = w.col(col.size, col_off, data=col, freeze=True)
    d_rows = w.col(rows.size, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = device_count(w, count)
    d_filter = w.u64(n_words)
    if before is not None:
        d_filter.copy_(torch.from_numpy(np.ascontiguousarray(before).view(np.int64)))
    ws = w.ws(bl.workspace_bytes(0))
    ws.fill_(ws_byte)
    rc = bl.build(ptr(d_col) if col.size else None, col.size, _p(d_rows), _p(d_count), rows.size if rows is not None else 0,
                  seed, flags, ptr(d_filter), n_words, ptr(ws), ws.numel(), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return d_filter.cpu().numpy().view(W).copy(), st


def expect_build(col, n_words, seed=0, rows=None, count=None, flags=0, before=None, fill=FILLS[0], **how):
    got, st = call_build(col, n_words, seed, rows, count, flags, before, fill=fill, **how)
    want, want_st = blm.build(col, n_words, seed, rows, count, flags, before=whole(fill, n_words) if before is None else before)
    assert st == want_st, (st, want_st)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {n_words} filter words differ, the first at {int(bad[0])}: {int(got[bad[0]]):#x}, the model has {int(want[bad[0]]):#x}"
    return got


def call_probe(filt, col, seed=0, rows=None, count=None, flags=0, col_off=0, list_off=0, out_off=0, fill=FILLS[0],
               ws_byte=0x3C, want_rows=True):
    """one dbench_bloom_probe_u32 on guarded buffers -> (the kept row ids or None, *out_count, status)"""
    w = Watch(fill)
    d_filter = w.u64(filt.size)
    d_filter.copy_(torch.from_numpy(np.ascontiguousarray(filt).view(np.int64)))
    w.freeze(d_filter)
    d_col = w.col(col.size, col_off, data=col, freeze=True)
    candidates = int(col.size if rows is None else rows.size)
    d_rows = w.col(candidates, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = device_count(w, count)
    d_out = w.col(candidates, out_off) if want_rows else None
    d_total = w.u64(1)
    nbytes = bl.workspace_bytes(candidates)
    ws = w.ws(nbytes)
    ws.fill_(ws_byte)
    rc = bl.probe(ptr(d_filter), filt.size, seed, ptr(d_col) if col.size else None, col.size, _p(d_rows), _p(d_count),
                  candidates if rows is not None else 0, flags, _p(d_out), ptr(d_total), ptr(ws), nbytes, stream())
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


def expect_probe(filt, col, seed=0, rows=None, count=None, flags=0, fill=FILLS[0], **how):
    got, total, st = call_probe(filt, col, seed, rows, count, flags, fill=fill, **how)
    want, want_total, want_st = blm.probe(filt, col, seed, rows, count, flags)
    assert (total, st) == (want_total, want_st), (total, want_total, st, want_st)
    if got is not None:
        assert np.array_equal(got, want), f"{int((got != want).sum()) if got.size == want.size else 'all'} row ids differ"
    return total


# ---- build -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_off", range(4))
def test_build_every_row_count_at_every_column_offset(col_off):
    for i, n in enumerate(ROW_COUNTS):
        n_words, kind, seed = WORDS[(i + col_off) % len(WORDS)], KINDS[(i + 2 * col_off) % len(KINDS)], (0, 12345)[i % 2]
        expect_build(make_keys(n, kind, seed), n_words, seed, col_off=col_off, fill=FILLS[(i + col_off) % 2])


@pytest.mark.parametrize("kind", KINDS)
def test_build_every_key_kind_at_every_filter_size(kind):
    n = 2 * SEG + 77
    for i, n_words in enumerate(WORDS):
        seed = (0, 0x9E3779B9, 0xFFFFFFFF)[i % 3]
        got = expect_build(make_keys(n, kind, seed), n_words, seed, col_off=i % 4, fill=FILLS[i % 2])
        if n_words == 65537 and kind == "random":
            assert int((got >> W(32)).astype(bool).sum()) > 1000  # bits above bit 31 are set


@pytest.mark.parametrize("listed", (False, True))
def test_build_every_kind_of_device_count(listed):
    n = SEG + 301
    col = make_keys(n, "random")
    rows = np.random.default_rng(3).permutation(n).astype(U) if listed else None
    filters = {}
    for i, kind in enumerate(COUNTS):
        count = count_of(kind, n)
        filters[kind] = expect_build(col, 997, 5, rows=rows, count=count, col_off=1, list_off=2, fill=FILLS[i % 2])
    assert not filters["zero"].any() and np.array_equal(filters["none"], filters["huge"])
    assert np.array_equal(filters["at"], filters["above"]) and not np.array_equal(filters["below"], filters["at"])
    assert 1 <= int(np.unpackbits(filters["one"].view(np.uint8)).sum()) <= 4


def test_build_through_lists_unsorted_repeated_and_with_bad_ids():
    rng = np.random.default_rng(8)
    n_col = 3000
    col = make_keys(n_col, "random")
    for i, m in enumerate((1, 5, 257, SEG + 1, 2 * SEG + 1)):
        rows = rng.integers(0, n_col // 3, m).astype(U)  # unsorted, rows repeat, most rows never named
        expect_build(col, 211, 1, rows=rows, list_off=i % 4, col_off=(i + 1) % 4)
        bad = rows.copy()
        bad[rng.integers(0, m, max(m // 40, 1))] = np.array([n_col, n_col + 1, 0x80000000, 0xFFFFFFFF], U)[rng.integers(0, 4, max(m // 40, 1))]
        got, st = call_build(col, 211, 1, rows=bad, list_off=(i + 2) % 4)
        assert st == blm.KEY_RANGE  # raised, and nothing inserted for those ids:
        assert np.array_equal(got, blm.build(col[bad[bad < n_col]], 211, 1)[0])
        # behind the count the list may hold anything without a status
        behind = np.r_[rows, np.full(9, 0xFFFFFFFF, U)]
        got, st = call_build(col, 211, 1, rows=behind, count=m, list_off=i % 4)
        assert st == 0 and np.array_equal(got, blm.build(col, 211, 1, rows=rows)[0])
    got, st = call_build(np.zeros(0, U), 64, 0, rows=np.array([0, 1, 2], U))  # an empty column: every id is outside it
    assert st == blm.KEY_RANGE and not got.any()


def test_build_accumulates_or_clears_and_a_stale_workspace_changes_nothing():
    a, b = make_keys(SEG + 9, "random", rng_seed=4), make_keys(2 * SEG + 3, "reference", rng_seed=5)
    for n_words in (1, 3, 1000):
        first = expect_build(a, n_words, 7)  # a clearing build onto a filter full of guard fill
        both = expect_build(b, n_words, 7, flags=bl.ACCUMULATE, before=first, col_off=3, fill=FILLS[1])
        assert np.array_equal(both, blm.build(np.r_[a, b], n_words, 7)[0])
        assert np.array_equal(expect_build(b, n_words, 7, before=first), blm.build(b, n_words, 7)[0])  # clears what it held
        expect_build(a, n_words, 7, flags=bl.ACCUMULATE)  # onto the guard fill itself
        for ws_byte in (0x00, 0xFF, 0x5A):
            assert np.array_equal(expect_build(a, n_words, 7, ws_byte=ws_byte), first)
    # a status left by a flagged call does not survive the next one on the same bytes: every call above started on 0xC3


# ---- probe -----------------------------------------------------------------------------------------------------------------
def filter_for(keys, bits, seed):
    return blm.build(keys, blm.words(keys.size, bits), seed)[0]


@pytest.mark.parametrize("bits", (2, 4))
@pytest.mark.parametrize("n", SEAMS)
def test_probe_dense_at_the_segment_seams(n, bits):
    rng = np.random.default_rng(n + bits)
    build = make_keys(n // 3 + 1, "random", rng_seed=9)
    filt = filter_for(build, bits, 11)
    col = np.where(rng.random(n) < 0.3, build[rng.integers(0, build.size, n)], make_keys(n, "random", rng_seed=10))
    for off in range(4):
        kept = expect_probe(filt, col, 11, col_off=off, out_off=(off + 1) % 4, fill=FILLS[off % 2])
        out = expect_probe(filt, col, 11, flags=bl.NEGATE, col_off=off, out_off=(off + 3) % 4)
        assert kept + out == n and kept > 0.3 * n * 0.9 and out > 0
    assert int(blm.may_hold(filt, col, 11).sum()) > int(np.isin(col, build).sum())  # false positives exist
    assert expect_probe(filt, col, 11, want_rows=False) == expect_probe(filt, col, 11)  # out_rows == NULL: the count alone


@pytest.mark.parametrize("negate", (False, True))
@pytest.mark.parametrize("n", SEAMS)
def test_probe_lists_at_the_segment_seams_with_every_kind_of_count(n, negate):
    rng = np.random.default_rng(2 * n + negate)
    n_col = 5000
    col = make_keys(n_col, "random", rng_seed=12)
    filt = filter_for(col[::3], 4, 0)
    flags = bl.NEGATE if negate else 0
    rows = rng.integers(0, n_col, n).astype(U)  # unsorted, with repeats
    for i, kind in enumerate(COUNTS):
        count = count_of(kind, n)
        spoiled = rows.copy()
        if count is not None and count < n:
            spoiled[count:] = 0xFFFFFFFF  # behind the count: ids outside the column, without a status
        expect_probe(filt, col, 0, rows=spoiled, count=count, flags=flags, list_off=i % 4, out_off=(i + 1) % 4, col_off=(i + 2) % 4,
                     fill=FILLS[i % 2], want_rows=kind != "above")
    bad = rows.copy()
    bad[[0, n // 2, n - 1]] = [n_col, 0x80000000, 0xFFFFFFFF]
    got, total, st = call_probe(filt, col, 0, rows=bad, flags=flags, list_off=3)
    assert st == blm.KEY_RANGE and total == got.size and not (got >= n_col).any()  # never kept, not even under negate
    assert np.array_equal(got, blm.probe(filt, col, 0, rows=bad, flags=flags)[0])


def test_probe_small_sizes_empty_filters_full_filters_and_the_build_column():
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257):
        col = make_keys(n, "random", rng_seed=13)
        filt = filter_for(col[: n // 2], 2, 3)
        for negate in (0, bl.NEGATE):
            expect_probe(filt, col, 3, flags=negate, col_off=n % 4)
            expect_probe(filt, col, 3, rows=np.arange(n, dtype=U)[::-1].copy(), flags=negate, list_off=(n + 1) % 4)
    col = make_keys(SEG + 5, "special", seed=77)
    for n_words in (1, 3, 64):
        zeros, ones = np.zeros(n_words, W), np.full(n_words, 0xFFFFFFFFFFFFFFFF, W)
        assert expect_probe(zeros, col, 77) == 0 and expect_probe(zeros, col, 77, flags=bl.NEGATE) == col.size
        assert expect_probe(ones, col, 77) == col.size and expect_probe(ones, col, 77, flags=bl.NEGATE) == 0
    got, total, st = call_probe(np.full(3, 0xFFFFFFFFFFFFFFFF, W), np.zeros(0, U), rows=np.array([0, 5], U))
    assert (total, st) == (0, blm.KEY_RANGE)  # an empty column: no candidate counts


@pytest.mark.parametrize("kind", KINDS)
def test_probing_the_column_a_filter_was_built_from_returns_every_row(kind):
    n = (1 << 16) + 13
    col = make_keys(n, kind, seed=9)
    for bits in (2, 16):
        filt = expect_build(col, blm.words(n, bits), 9, col_off=1)
        got, total, st = call_probe(filt, col, 9, col_off=2, out_off=3)
        assert (total, st) == (n, 0) and np.array_equal(got, np.arange(n, dtype=U))
        assert call_probe(filt, col, 9, flags=bl.NEGATE)[1] == 0
