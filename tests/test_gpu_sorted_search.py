"""The sorted search on the GPU (include/dbhip_sorted_search.h) against tests/sorted_search_model.py, bit for bit, on guarded
buffers (tests/guard_testlib.py): frozen inputs, output columns of exactly n entries, an index workspace of exactly the
queried size that holds the fill pattern before the build, the status word read after every call, every guard looked at after
every call.  Column sizes sit on every boundary of the fence ladder's geometry, with the default top level and with top = 64,
where a small column already takes one, two and three levels down and ends every level in a ragged block."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import guard_testlib as gt
from tests import sorted_search_model as sm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "dwarf_bench_amd" / "_lib"
U32 = np.uint32
KEY_RANGE = 2  # DBHIP_DEV_KEY_RANGE
GEOMETRIES = [(m, 0) for m in (0, 1, 63, 64, 65, 4095, 4096, 4097, 16384, 16385, (1 << 18) + 1, (1 << 20) + 1)] + [
    (65, 64), (4097, 64), (262145, 64)]


def _lib():
    from dwarf_bench_amd import _capi
    return _capi, _capi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sign(signed):
    return U32(0x80000000) if signed else U32(0)


def column(m, kind, signed):
    """an ascending column of m entries, built in the x domain and flipped back"""
    i = np.arange(m, dtype=np.uint64)
    if kind == "distinct":  # from 0 to nearly 2^32 - 1: crosses zero as int32, crosses 2^31 as uint32
        x = i * np.uint64(0xFFFFFFFF // max(m - 1, 1))
    elif kind == "one value":
        x = np.full(m, 0x80000007, dtype=np.uint64)
    elif kind == "runs across block edges":  # equal keys over entries 60..70, 4090..4100 and the column's last 70
        x = i * np.uint64(16) + np.uint64(5)
        for a, b in ((60, 70), (4090, 4100), (max(m - 70, 0), m)):
            if a < m:
                x[a:b] = x[a]
        x = np.maximum.accumulate(x)
    elif kind == "a run over a 4096 block":  # one key over 4096 + 700 entries from entry 3000 on, and short runs
        x = (i // np.uint64(3)) * np.uint64(7)
        x[3000: 3000 + 4096 + 700] = x[min(3000, m - 1)] if m else 0
        x = np.maximum.accumulate(x)
    elif kind == "extremes":  # 0 and 0xFFFFFFFF in the x domain, several of each
        x = i * np.uint64(0xFFFFFFFF // max(m - 1, 1))
        x[: min(3, m)] = 0
        x[max(m - 3, 0):] = 0xFFFFFFFF
    else:
        raise ValueError(kind)
    x = x.astype(U32)
    assert np.all(x[1:] >= x[:-1])
    return x ^ _sign(signed)


def probes(col, signed, top, seed):
    """-> (lo, hi): below and above the column, every fence of every level and each +- 1, 0 and 0xFFFFFFFF, random values;
    hi is lo, lo + a band, or below lo"""
    rng = np.random.default_rng(seed)
    ladder = sm.levels(col, signed, top)
    fences = np.concatenate(ladder[1:] + [ladder[0][:: max(ladder[0].size // 500, 1)], ladder[0][-3:]]).astype(U32)
    xl = np.concatenate([fences, fences + U32(1), fences - U32(1), np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFF,
                                                                           0x80000000], dtype=U32),
                         rng.integers(0, 1 << 32, 997, dtype=np.uint64).astype(U32)])
    if ladder[0].size:
        xl = np.concatenate([xl, ladder[0][:1] - U32(1), ladder[0][-1:] + U32(1)])
    band = rng.choice(np.array([0, 0, 1, 5, 1 << 12, 1 << 28], dtype=np.uint64), xl.size)
    xh = np.minimum(xl.astype(np.uint64) + band, 0xFFFFFFFF).astype(U32)
    below = rng.integers(0, 8, xl.size) == 0
    xh[below] = xl[below] - U32(3)  # lo > hi (or a wrap to the top: any pair of values is a valid question)
    return xl ^ _sign(signed), xh ^ _sign(signed)


def run(col, lo, hi, signed, top, fill, want_pos=True, want_cnt=True, repeat=1):
    """index build + search on guarded buffers -> (pos, cnt, watch, ws, tensors): every guard and the status word checked"""
    capi, lib = _lib()
    m = col.size
    n = (lo if lo is not None else hi).size
    w = gt.Watch(fill)
    d_col = w.col(m, offset_words=1, data=col, freeze=True)  # the column needs only its natural alignment
    d_lo = w.col(n, data=lo, freeze=True) if lo is not None else None
    d_hi = w.col(n, data=hi, freeze=True) if hi is not None else None
    d_pos = w.col(n) if want_pos else None
    d_cnt = w.col(n) if want_cnt else None
    nbytes = lib.dbhip_sorted_index_workspace_bytes(m, top)
    assert nbytes == sm.workspace_bytes(m, top)
    ws = w.ws(nbytes)
    p = lambda t: gt.ptr(t) if t is not None else None  # noqa: E731
    capi.check(lib.dbhip_sorted_index_build_u32(p(d_col), m, int(signed), top, p(ws), nbytes, _stream()), "build")
    torch.cuda.synchronize()
    w.check()
    assert ws[:4].view(torch.int32).item() == 0, "the build leaves a clean status word"
    outs = []
    for _ in range(repeat):
        for t in (d_pos, d_cnt):
            if t is not None:
                t.fill_(gt.i32(fill))
        capi.check(lib.dbhip_sorted_search_u32(p(d_col), m, p(d_lo), p(d_hi), n, p(d_pos), p(d_cnt), p(ws), nbytes,
                                                _stream()), "search")
        torch.cuda.synchronize()
        w.check()
        assert ws[:4].view(torch.int32).item() == 0, "no input raises a status"
        outs.append(tuple(t.cpu().numpy().view(U32).copy() if t is not None else None for t in (d_pos, d_cnt)))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert (a is None and b is None) or np.array_equal(a, b), "repeated calls on one workspace differ"
    return outs[0][0], outs[0][1], w, ws, (d_col, d_lo, d_hi, d_pos, d_cnt)


def words(col, lo, hi, pos, cnt, signed, fill=gt.FILLS[0]):
    """dbhip_check_sorted_search_u32 on guarded buffers -> its four words"""
    capi, lib = _lib()
    n = next(c for c in (lo, hi, pos, cnt) if c is not None).size
    w = gt.Watch(fill)
    cols = [w.col(c.size, offset_words=k % 4, data=c, freeze=True) if c is not None else None
            for k, c in enumerate((col, lo, hi, pos, cnt))]
    res = w.u64(4)
    ws = w.ws(lib.dbhip_check_sorted_search_workspace_bytes(n))
    p = lambda t: gt.ptr(t) if t is not None else None  # noqa: E731
    capi.check(lib.dbhip_check_sorted_search_u32(p(cols[0]), col.size, int(signed), p(cols[1]), p(cols[2]), n, p(cols[3]),
                                                  p(cols[4]), gt.ptr(res), gt.ptr(ws), ws.numel(), _stream()), "check")
    torch.cuda.synchronize()
    w.check()
    assert ws[:4].view(torch.int32).item() == 0
    return tuple(int(v) & sm.NONE for v in res.cpu().tolist())


def _kinds(m):
    kinds = ["distinct", "one value", "extremes"]
    if m > 70:
        kinds.append("runs across block edges")
    if m > 3000 + 4096 + 700:
        kinds.append("a run over a 4096 block")
    return kinds


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("m,top", GEOMETRIES)
def test_every_geometry_and_column_shape(m, top, signed):
    for k, kind in enumerate(_kinds(m)):
        col = column(m, kind, signed)
        lo, hi = probes(col, signed, top, seed=m + k)
        fill = gt.FILLS[(k + int(signed)) % 2]
        shapes = [(lo, hi), (lo, None)] if k % 2 == 0 else [(lo, hi), (None, hi), (lo, lo.copy())]
        for a, b in shapes:
            pos, cnt, *_ = run(col, a, b, signed, top, fill)
            want_pos, want_cnt = sm.search(col, a, b, signed)
            assert np.array_equal(pos, want_pos), (kind, "pos")
            assert np.array_equal(cnt, want_cnt), (kind, "cnt")
            if kind == "distinct":  # the validator on a right answer: word for word its model, which accepts
                got = words(col, a, b, pos, cnt, signed, fill)
                assert got == sm.check(col, a, b, pos, cnt, signed) == (0, sm.NONE, int(cnt.sum()), 0)


@pytest.mark.parametrize("signed", [False, True])
def test_null_columns_and_repeated_calls(signed):
    m, top = 4097, 64
    col = column(m, "runs across block edges", signed)
    lo, hi = probes(col, signed, top, seed=9)
    want_pos, want_cnt = sm.search(col, lo, hi, signed)
    pos, cnt, *_ = run(col, lo, hi, signed, top, gt.FILLS[0], want_pos=False, repeat=3)  # cnt alone still needs L(lo)
    assert pos is None and np.array_equal(cnt, want_cnt)
    pos, cnt, *_ = run(col, lo, None, signed, top, gt.FILLS[1], want_cnt=False, repeat=2)  # searchsorted, left
    assert cnt is None and np.array_equal(pos, want_pos)
    pos, cnt, *_ = run(col, None, hi, signed, top, gt.FILLS[0], want_pos=False)  # searchsorted, right
    assert np.array_equal(cnt, sm.search(col, None, hi, signed)[1])
    pos, cnt, *_ = run(col, None, hi, signed, top, gt.FILLS[1])
    assert not pos.any() and np.array_equal(cnt, sm.search(col, None, hi, signed)[1])
    assert words(col, None, hi, None, cnt, signed) == sm.check(col, None, hi, None, cnt, signed)
    assert words(col, lo, None, want_pos, None, signed) == (0, sm.NONE, 0, 0)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 2047, 2048, 2049, 3 * 2048 + 257 + 2])
def test_probe_counts(n):
    m, top, signed = 4097, 64, True
    col = column(m, "distinct", signed)
    lo, hi = (np.resize(c, n) for c in probes(col, signed, top, seed=n))
    assert lo.size == n and hi.size == n
    pos, cnt, *_ = run(col, lo, hi, signed, top, gt.FILLS[n % 2])
    want_pos, want_cnt = sm.search(col, lo, hi, signed)
    assert np.array_equal(pos, want_pos) and np.array_equal(cnt, want_cnt)


def test_many_workgroups_each_stage_the_top_level():
    """more tiles than resident workgroups: every workgroup loops, and the default top level fills all of its LDS"""
    m, n = (1 << 20) + 1, (1 << 21) + 77
    col = column(m, "distinct", False)
    rng = np.random.default_rng(12)
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    hi = lo + rng.integers(0, 1 << 14, n).astype(U32)
    pos, cnt, *_ = run(col, lo, hi, False, 0, gt.FILLS[0])
    want_pos, want_cnt = sm.search(col, lo, hi)
    assert np.array_equal(pos, want_pos) and np.array_equal(cnt, want_cnt)


@pytest.mark.parametrize("signed", [False, True])
def test_validator_agrees_with_its_model_word_for_word(signed):
    m, top = 4097, 64
    col = column(m, "runs across block edges", signed)
    lo, hi = probes(col, signed, top, seed=21)
    pos, cnt = sm.search(col, lo, hi, signed)
    n = lo.size
    rng = np.random.default_rng(22)

    def agree(a, b, p, c, expect_ok=None):
        got = words(col, a, b, p, c, signed, gt.FILLS[int(rng.integers(0, 2))])
        assert got == sm.check(col, a, b, p, c, signed)
        if expect_ok is not None:
            assert (got[0] == 0) == expect_ok, got
        return got

    agree(lo, hi, pos, cnt, True)
    hit = int(np.nonzero((cnt > 1) & (pos > 0) & (pos + cnt < m))[0][0])
    empty = int(np.nonzero(sm.flip(hi, signed) < sm.flip(lo, signed))[0][0])
    for row, dpos, dcnt in ((hit, 1, -1), (hit, -1, 1), (hit, 0, 1), (hit, 0, -1), (hit, 0, m), (hit, m + 1, 0),
                            (empty, 0, 1), (n - 1, 1, 0), (0, 0xFFFFFFFF, 0), (0, 0, 0xFFFFFFFF)):
        p, c = pos.copy(), cnt.copy()
        p[row:row + 1] += U32(dpos & 0xFFFFFFFF)  # (an array add wraps silently)
        c[row:row + 1] += U32(dcnt & 0xFFFFFFFF)
        got = agree(lo, hi, p, c, False)
        assert got[1] == row
    # foreign answers: those of other probe values, of the other signedness, of another column
    other_lo, other_hi = probes(col, signed, top, seed=23)
    agree(other_lo[:n], other_hi[:n], pos, cnt, False)
    agree(lo, hi, *sm.search(col ^ U32(0x80000000), lo, hi, not signed))
    agree(lo, hi, *sm.search(column(m, "distinct", signed), lo, hi, signed), False)
    agree(lo, None, pos, cnt)
    agree(None, hi, pos, cnt, False)
    # garbage: every read is range-checked, whatever the columns hold
    garbage = [rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32) for _ in range(2)]
    agree(lo, hi, garbage[0], garbage[1], False)
    agree(lo, hi, np.full(n, 0xFFFFFFFF, dtype=U32), np.full(n, 0xFFFFFFFF, dtype=U32), False)
    agree(lo, hi, np.full(n, m, dtype=U32), np.zeros(n, dtype=U32))
    empty_col = col[:0]
    assert words(empty_col, lo, hi, pos * U32(0), cnt * U32(0), signed) == (0, sm.NONE, 0, 0)
    assert words(empty_col, lo, hi, pos, cnt, signed) == sm.check(empty_col, lo, hi, pos, cnt, signed)


@pytest.mark.parametrize("m,top", [(4097, 64), (262145, 64), (16385, 0), ((1 << 18) + 1, 0)])
def test_an_unsorted_column_keeps_the_answer_in_bounds(m, top):
    """the answer is unspecified; pos <= m and pos + cnt <= m, and the guards, are not"""
    rng = np.random.default_rng(m)
    col = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U32)
    lo = rng.choice(col, 5003)
    hi = lo + rng.integers(0, 1 << 30, lo.size).astype(U32)
    for a, b in ((lo, hi), (lo, None), (None, hi)):
        pos, cnt, *_ = run(col, a, b, False, top, gt.FILLS[0])
        assert np.all(pos.astype(np.int64) <= m) and np.all(pos.astype(np.int64) + cnt.astype(np.int64) <= m)


def test_a_workspace_built_for_another_column_is_refused():
    """on the host where the size tells, on the device (0 / 0 in every row, DBHIP_DEV_KEY_RANGE) where only the header does"""
    capi, lib = _lib()
    m, top = 4097, 64
    col = column(m, "distinct", False)
    lo, hi = probes(col, False, top, seed=31)
    n = lo.size
    pos, cnt, w, ws, (d_col, d_lo, d_hi, d_pos, d_cnt) = run(col, lo, hi, False, top, gt.FILLS[0])
    assert cnt.any()

    def search(m_now, nbytes=ws.numel()):
        d_pos.fill_(7)
        d_cnt.fill_(7)
        rc = lib.dbhip_sorted_search_u32(gt.ptr(d_col), m_now, gt.ptr(d_lo), gt.ptr(d_hi), n, gt.ptr(d_pos), gt.ptr(d_cnt),
                                         gt.ptr(ws), nbytes, _stream())
        torch.cuda.synchronize()
        w.check()
        return rc, ws[:4].view(torch.int32).item()

    assert search(1 << 26) == (-2, 0)  # no index of 2^26 entries fits: DBHIP_EWORKSPACE, nothing ran
    assert bool((d_pos == 7).all())
    rc, status = search(m - 1)  # the size fits, the header says 4097
    assert (rc, status) == (0, KEY_RANGE) and not d_pos.any() and not d_cnt.any()
    capi.check(lib.dbhip_sorted_index_build_u32(gt.ptr(d_col), m, 0, top, gt.ptr(ws), ws.numel(), _stream()), "build")
    assert search(m) == (0, 0) and np.array_equal(d_cnt.cpu().numpy().view(U32), cnt)
    rc, status = search(m, nbytes=256)  # shorter than the index the header describes (256 passes the host: top unknown)
    assert (rc, status) == (0, KEY_RANGE) and not d_cnt.any()
    ws[4:].random_(0, 256)  # a header that was never built
    rc, status = search(m)
    assert rc == 0 and not d_pos.any() and not d_cnt.any()
    w.check()


# ---- the range join ------------------------------------------------------------------------------------------------------
def _join(build, lo, hi, **kw):
    from dwarf_bench_amd import ops
    dev = lambda c: torch.from_numpy(c.view(np.int32)).cuda() if c is not None else None  # noqa: E731
    b, p = ops.range_join(dev(build), dev(lo), dev(hi), **kw)
    return b.cpu().numpy().view(U32), p.cpu().numpy().view(U32)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("left_outer", [False, True])
def test_range_join_against_the_model(left_outer, signed):
    rng = np.random.default_rng(41 + left_outer)
    m, n = 20011, 3001
    build = (rng.integers(0, 3000, m).astype(U32) - U32(1500)) * U32(3)  # duplicates; crosses zero as int32
    lo = (rng.integers(0, 3400, n).astype(U32) - U32(1700)) * U32(3)
    hi = lo + rng.integers(0, 30, n).astype(U32) - U32(3)  # some empty intervals
    lo[5], hi[5] = (0x80000000, 0x7FFFFFFF) if signed else (0, 0xFFFFFFFF)  # a probe row that matches every build row
    lo[6:9] = 0x7FFFFF00 if signed else 0xFFFFFF00  # rows that match nothing
    hi[6:9] = lo[6:9] + U32(5)
    want = sm.range_join(build, lo, hi, signed, left_outer)
    assert want[0].size > m
    for capacity in (None, want[0].size, want[0].size + 1000):
        got = _join(build, lo, hi, left_outer=left_outer, capacity=capacity, signed=signed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    from dwarf_bench_amd import _capi
    with pytest.raises(_capi.DbhipError, match=str(want[0].size)):
        _join(build, lo, hi, left_outer=left_outer, capacity=want[0].size - 1, signed=signed)
    # the equality join and the ASOF side
    for a, b in ((lo, None), (None, hi[:64])):
        want = sm.range_join(build, a, b, signed, left_outer)
        got = _join(build, a, b, left_outer=left_outer, signed=signed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_range_join_m_times_one():
    build = np.full(70001, 9, dtype=U32)
    lo, hi = np.array([9], dtype=U32), np.array([9], dtype=U32)
    got = _join(build, lo, hi)
    assert np.array_equal(got[0], np.arange(build.size, dtype=U32)) and not got[1].any()
    got = _join(build, lo + U32(1), hi + U32(1), left_outer=True)
    assert got[0].tolist() == [0xFFFFFFFF] and got[1].tolist() == [0]
    assert _join(build, lo + U32(1), None)[0].size == 0


# ---- the dwarf -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1000, 100000])
def test_range_join_dwarf_through_its_cli(size):
    import os
    exe = LIB / "dwarf_bench_range_join"
    cmd = [str(exe), "RangeJoinHip", "--device=hip", f"--input_size={size}", "--iterations=2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 2
    env = {**os.environ, "DWARF_BENCH_INJECT_FAULT": "1"}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ncorrect results") == 2 and "Caught exception" not in r.stderr, r.stderr
