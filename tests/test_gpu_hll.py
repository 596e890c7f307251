"""The HyperLogLog sketch on the GPU (dwarf_bench_amd/host/hll_sketch.cpp through hll_native): the raw entry points on guarded
buffers (tests/guard_testlib.py), the registers and the histogram compared bit for bit with the numpy model
(tests/hll_model.py).  Every column sits at its own offset from a 16-byte boundary, guard words surround the registers, the
histogram, every input and the workspace, and the workspace and the outputs hold anything beforehand."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import hll_native as hl
from dwarf_bench_amd import ops
from dwarf_bench_amd import select_native as sn
from tests import hll_model as hm
from tests.guard_testlib import FILLS, Watch, ptr
from tests.test_gpu_bloom import ROW_COUNTS

pytestmark = pytest.mark.gpu

SEG = sn.SEGMENT_ROWS
BIG = (1 << 22) + 5  # the grid at its full size (hl.MAX_GRID workgroups), two and three segments to a workgroup
PS = (4, 5, 11, 14)
KINDS = ("random", "equal", "dense", "reference", "special")
COUNTS = ("none", "zero", "one", "below", "at", "above", "huge")
U, B = np.uint32, np.uint8


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


def make_cols(n, k, kind, seed=0, rng_seed=1):
    return [make_keys(n, kind if j == 0 else KINDS[(KINDS.index(kind) + j) % len(KINDS)], seed, rng_seed + 7 * j) for j in range(k)]


def count_of(kind, capacity):
    return {"none": None, "zero": 0, "one": 1, "below": capacity // 2 + 1, "at": capacity, "above": capacity + 1,
            "huge": (1 << 40) + 9}[kind]


def _p(t):
    return ptr(t) if t is not None else None


def guarded_registers(w, p, before=None):
    """2^p bytes, 4-byte aligned, inside a guarded byte buffer: they start out as the fill, or as `before`"""
    regs = w.ws(1 << p)
    if before is not None:
        regs.copy_(torch.from_numpy(np.ascontiguousarray(before).view(B)))
    return regs


def guarded_hist(w):
    """64 uint32 words, 8-byte aligned, in a guarded run of uint64 words"""
    return w.u64(hl.HIST_WORDS // 2)


def call_build(cols, p, seed=0, rows=None, count=None, flags=0, before=None, offs=(0, 1, 2, 3), list_off=0, fill=FILLS[0],
               ws_byte=0xC3):
    """one dbench_hll_build_u32 on guarded buffers -> (registers, histogram, status)"""
    w = Watch(fill)
    n_col = cols[0].size
    d_cols = [w.col(n_col, offs[j], data=c, freeze=True) for j, c in enumerate(cols)]
    d_rows = w.col(rows.size, list_off, data=rows, freeze=True) if rows is not None else None
    d_count = None
    if count is not None:
        d_count = w.u64(1)
        d_count.fill_(count)
        w.freeze(d_count)
    d_regs, d_hist = guarded_registers(w, p, before), guarded_hist(w)
    nbytes = hl.workspace_bytes(p)
    ws = w.ws(nbytes)
    ws.fill_(ws_byte)
    rc = hl.build([ptr(c) if n_col else None for c in d_cols], n_col, _p(d_rows), _p(d_count),
                  rows.size if rows is not None else 0, seed, flags, p, ptr(d_regs), ptr(d_hist), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return d_regs.cpu().numpy().copy(), d_hist.cpu().numpy().view(U).copy(), st


def same(got, want, what=""):
    regs, hist, st = got
    want_regs, want_hist, want_st = want
    assert st == want_st, (what, st, want_st)
    bad = np.flatnonzero(regs != want_regs)
    assert bad.size == 0, (f"{what}: {bad.size} of {regs.size} registers differ, the first at {int(bad[0])}: {int(regs[bad[0]])}, "
                           f"the model has {int(want_regs[bad[0]])}")
    assert np.array_equal(hist, want_hist), (what, hist, want_hist)


def expect_build(cols, p, seed=0, rows=None, count=None, flags=0, before=None, fill=FILLS[0], **how):
    got = call_build(cols, p, seed, rows, count, flags, before, fill=fill, **how)
    held = np.full(1 << p, fill & 0xFF, B) if before is None else before  # (both fills repeat one byte)
    same(got, hm.build(cols, p, seed, rows, count, flags, before=held), (p, cols[0].size, len(cols)))
    return got[0]


# ---- build -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_off", range(4))
def test_build_every_row_count_at_every_column_offset(col_off):
    for i, n in enumerate(ROW_COUNTS):
        p, kind, seed = PS[(i + col_off) % 4], KINDS[(i + 2 * col_off) % len(KINDS)], (0, 12345)[i % 2]
        k = 1 + (i + col_off) % 4
        offs = [(col_off + 3 * j) % 4 for j in range(4)]  # every column at its own offset
        regs = expect_build(make_cols(n, k, kind, seed), p, seed, offs=offs, fill=FILLS[(i + col_off) % 2])
        assert bool(regs.any()) == (n > 0)


@pytest.mark.parametrize("k", (1, 2, 3, 4))
def test_build_every_key_kind_at_every_p_and_column_count(k):
    n = 2 * SEG + 77
    for i, kind in enumerate(KINDS):
        for j, p in enumerate(PS):
            seed = (0, 0x9E3779B9, 0xFFFFFFFF)[(i + j) % 3]
            expect_build(make_cols(n, k, kind, seed, rng_seed=i), p, seed, offs=[(i + j + 2 * c) % 4 for c in range(4)],
                         fill=FILLS[(i + j) % 2])


@pytest.mark.parametrize("p", PS)
def test_build_the_full_grid_with_several_segments_per_workgroup(p):
    assert (BIG + SEG - 1) // SEG > 2 * hl.MAX_GRID
    col = np.random.default_rng(p).integers(0, 1 << 32, BIG, dtype=np.uint64).astype(U)
    k = 2 if p == 11 else 1
    cols = [col, (col >> U(7)) * U(3)][:k]
    regs = expect_build(cols, p, 99, offs=(p % 4, 3, 0, 0))
    e = hm.estimate(hm.histogram(regs), p)
    truth = np.unique(col).size
    assert abs(e - truth) <= 4 * hm.relative_error(p) * truth


@pytest.mark.parametrize("p", PS)
def test_keys_built_against_the_hash_take_their_rank_from_g(p):
    """h has its low 32 - p bits zero: a 32-bit clz, or a rank that ignores the g half, gives 32 - p + 1 for every key"""
    for seed in (0, 0xDEADBEEF):
        keys = hm.keys_ranked_by_g(SEG + 300, p, seed, np.random.default_rng(p + seed))
        regs = expect_build([keys], p, seed, offs=(1, 0, 0, 0))
        assert int(regs.max()) > 32 - p + 1 and int(regs[regs > 0].min()) >= 32 - p + 1


@pytest.mark.parametrize("listed", (False, True))
def test_build_every_kind_of_device_count(listed):
    n = SEG + 301
    cols = make_cols(n, 2, "random")
    rows = np.random.default_rng(3).permutation(n).astype(U) if listed else None
    got = {}
    for i, kind in enumerate(COUNTS):
        got[kind] = expect_build(cols, 11, 5, rows=rows, count=count_of(kind, n), offs=(1, 3, 0, 0), list_off=2, fill=FILLS[i % 2])
    assert not got["zero"].any() and np.array_equal(got["none"], got["huge"])
    assert np.array_equal(got["at"], got["above"]) and not np.array_equal(got["below"], got["at"])
    assert int((got["one"] > 0).sum()) == 1


def test_build_through_lists_unsorted_repeated_and_with_bad_ids():
    rng = np.random.default_rng(8)
    n_col = 3000
    for i, m in enumerate((1, 5, 257, SEG + 1, 2 * SEG + 1)):
        k, p = 1 + i % 4, PS[i % 4]
        cols = make_cols(n_col, k, "random", rng_seed=i)
        rows = rng.integers(0, n_col // 3, m).astype(U)  # unsorted, rows repeat, most rows never named
        expect_build(cols, p, 1, rows=rows, list_off=i % 4, offs=[(i + 1 + j) % 4 for j in range(4)])
        bad = rows.copy()
        bad[rng.integers(0, m, max(m // 40, 1))] = np.array([n_col, n_col + 1, 0x80000000, 0xFFFFFFFF], U)[rng.integers(0, 4, max(m // 40, 1))]
        got = call_build(cols, p, 1, rows=bad, list_off=(i + 2) % 4)
        assert got[2] == hm.KEY_RANGE  # raised, and nothing inserted for those ids:
        same(got, hm.build([c[bad[bad < n_col]] for c in cols], p, 1)[:2] + (hm.KEY_RANGE,))
        # behind the count the list may hold anything without a status
        behind = np.r_[rows, np.full(9, 0xFFFFFFFF, U)]
        same(call_build(cols, p, 1, rows=behind, count=m, list_off=i % 4), hm.build(cols, p, 1, rows=rows))
    regs, hist, st = call_build([np.zeros(0, U)], 5, 0, rows=np.array([0, 1, 2], U))  # an empty column: every id is outside it
    assert st == hm.KEY_RANGE and not regs.any() and hist[0] == 32


def test_build_accumulates_or_replaces_and_a_stale_workspace_changes_nothing():
    a, b = make_cols(SEG + 9, 2, "random", rng_seed=4), make_cols(2 * SEG + 3, 2, "reference", rng_seed=5)
    for p in PS:
        first = expect_build(a, p, 7)  # onto registers full of guard fill
        both = expect_build(b, p, 7, flags=hl.ACCUMULATE, before=first, offs=(3, 2, 0, 0), fill=FILLS[1])
        assert np.array_equal(both, hm.build([np.r_[x, y] for x, y in zip(a, b)], p, 7)[0])
        assert np.array_equal(expect_build(b, p, 7, before=first), hm.build(b, p, 7)[0])  # replaces what they held
        # onto bytes above q+1: the guard fill itself (0x5A = 90, 0xA5 = 165), and a few among valid ones
        for fill in FILLS:
            got = call_build(a, p, 7, flags=hl.ACCUMULATE, fill=fill)
            assert got[2] == hm.KEY_RANGE and (got[0] == 64 - p + 1).all() and got[1][64 - p + 1] == 1 << p
        spoiled = first.copy()
        spoiled[[0, 7, (1 << p) - 1]] = [64 - p + 2, 255, 200]
        got = call_build(b, p, 7, flags=hl.ACCUMULATE, before=spoiled)
        same(got, hm.build(b, p, 7, flags=hl.ACCUMULATE, before=spoiled))
        assert got[2] == hm.KEY_RANGE and got[0][7] == 64 - p + 1
        edge = first.copy()
        edge[3] = 64 - p + 1  # q+1 itself is a valid byte
        assert call_build(b, p, 7, flags=hl.ACCUMULATE, before=edge)[2] == 0
        for ws_byte in (0x00, 0xFF, 0x5A):  # two calls give identical output, whatever the workspace held
            assert np.array_equal(expect_build(a, p, 7, ws_byte=ws_byte), first)
    # a status left by a flagged call does not survive the next one on the same bytes: every call above started on 0xC3


# ---- merge -----------------------------------------------------------------------------------------------------------------
def call_merge(dst, src, p, fill=FILLS[0], ws_byte=0x3C, same_buffer=False, ws_p=None):
    w = Watch(fill)
    d_dst = guarded_registers(w, p, dst)
    d_src = d_dst if same_buffer else guarded_registers(w, p, src)
    if not same_buffer:
        w.freeze(d_src)
    d_hist = guarded_hist(w)
    nbytes = hl.workspace_bytes(p if ws_p is None else ws_p)
    ws = w.ws(nbytes)
    ws.fill_(ws_byte)
    rc = hl.merge(ptr(d_dst), ptr(d_src), p, ptr(d_hist), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    st = ops.workspace_status(ws)
    w.check()
    return d_dst.cpu().numpy().copy(), d_hist.cpu().numpy().view(U).copy(), st


@pytest.mark.parametrize("p", PS)
def test_merge_is_the_build_of_the_union_and_recounts_in_place(p):
    a, b = make_cols(3 * SEG + 5, 1, "random", rng_seed=p), make_cols(SEG - 3, 1, "dense")
    ra, rb = hm.build(a, p, 3)[0], hm.build(b, p, 3)[0]
    for i, (dst, src) in enumerate(((ra, rb), (rb, ra), (ra, np.zeros(1 << p, B)), (np.zeros(1 << p, B), rb))):
        got = call_merge(dst, src, p, fill=FILLS[i % 2], ws_byte=(0x00, 0xFF, 0x3C, 0x77)[i], ws_p=(None, 4)[i % 2])
        same(got, hm.merge(dst, src, p), (p, i))
    same(call_merge(ra, rb, p), hm.build([np.r_[a[0], b[0]]], p, 3))
    same(call_merge(ra, None, p, same_buffer=True), (ra, hm.histogram(ra), 0))  # src == dst: the histogram alone
    spoiled = rb.copy()
    spoiled[[1, (1 << p) - 2]] = [64 - p + 2, 0xFF]
    for dst, src in ((ra, spoiled), (spoiled, ra)):  # the clamp and the status on either side
        got = call_merge(dst, src, p)
        same(got, hm.merge(dst, src, p))
        assert got[2] == hm.KEY_RANGE and got[0][1] == 64 - p + 1
    got = call_merge(spoiled, None, p, same_buffer=True)
    same(got, hm.merge(spoiled, spoiled, p))
    assert got[2] == hm.KEY_RANGE


# ---- the tensor API --------------------------------------------------------------------------------------------------------
def test_ops_sketch_builds_merges_and_estimates():
    rng = np.random.default_rng(21)
    n = (1 << 16) + 13
    a = rng.integers(0, 50000, n).astype(U)
    b = rng.integers(40000, 90000, n).astype(U)
    ta, tb = (torch.from_numpy(x.view(np.int32)).cuda() for x in (a, b))
    for p in (4, 12, 14):
        s, t = ops.HyperLogLog(p, 5), ops.HyperLogLog(p, 5)
        assert s.estimate() == 0.0
        s.build(ta)
        t.build(tb)
        assert np.array_equal(s.registers.cpu().numpy(), hm.build(a, p, 5)[0])
        assert s.estimate() == hm.estimate(hm.build(a, p, 5)[1], p)
        s.merge(t)
        want = hm.build(np.r_[a, b], p, 5)
        assert np.array_equal(s.registers.cpu().numpy(), want[0]) and np.array_equal(s.hist.cpu().numpy().view(U), want[1])
        truth = np.unique(np.r_[a, b]).size
        assert abs(s.estimate() - truth) <= 4 * ops.hll_relative_error(p) * truth
        u = ops.HyperLogLog(p, 5)
        u.build(ta)
        u.build(tb, accumulate=True)
        assert torch.equal(u.registers, s.registers) and u.estimate() == s.estimate()
    rows = torch.from_numpy(rng.integers(0, n, 5000).astype(np.int32)).cuda()
    count = torch.tensor([3000], dtype=torch.int64, device="cuda")
    s = ops.HyperLogLog()
    s.build([ta, tb], rows=rows, count=count)
    picked = rows.cpu().numpy()[:3000]
    assert s.estimate() == hm.estimate(hm.build([a[picked], b[picked]], 12, 0)[1], 12)
    e = ops.approx_count_distinct([ta, tb])
    truth = np.unique(a.astype(np.uint64) << np.uint64(32) | b).size
    assert abs(e - truth) <= 4 * ops.hll_relative_error(12) * truth
    assert ops.approx_count_distinct(ta[:0]) == 0.0 and ops.approx_count_distinct(ta, rows=rows[:0]) == 0.0
    rows[7] = n
    with pytest.raises(Exception, match="status 0x2"):
        ops.approx_count_distinct(ta, rows=rows)
