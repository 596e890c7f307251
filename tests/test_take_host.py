"""The late-materialisation entry points (dwarf_bench_amd/host/take_rows.hpp, in libdbench.so) without a GPU: the exported
symbols, the header's constants against the binding's and the model's, the workspace query's bound, the host-side
argument checks (all before any HIP call, argument errors before workspace errors) and the tensor API's refusals.
Every call below fails on the host: the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import take_native as tn
from tests import take_model as tm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "take_rows.hpp"
FAKE = 1 << 30  # 256-byte aligned
N, CAP = 100002, 50000  # a capacity whose workspace is larger than the smallest one
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
COLS = [FAKE + i * STEP for i in range(4)]
OUTS = [FAKE + (4 + i) * STEP for i in range(4)]
ROWS, COUNT, OUT, WS = (FAKE + (8 + i) * STEP for i in range(4))


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return tn.lib()


def test_libdbench_exports_exactly_the_three_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_(?:take|aggregate)\w*)$", out, flags=re.M))
    assert names == ["dbench_aggregate_rows_u32", "dbench_take_u32", "dbench_take_workspace_bytes"] == sorted(tn.ENTRY_POINTS)
    # the three families of libdbench.so keep their names apart, and the dbhip_* surface is include/'s
    assert not [n for n in names if n.startswith(("dbench_select_", "dbench_merge_", "dbench_setop_"))]
    assert not re.findall(r"\bdbhip_(?:take|aggregate_rows)\w*$", out, flags=re.M)


def test_header_constants_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_TAKE_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_TAKE_MAX_COLS": tn.MAX_COLS, "DBENCH_TAKE_SEGMENT_ROWS": tn.SEGMENT_ROWS,
                   "DBENCH_TAKE_OUTER": tn.OUTER, "DBENCH_TAKE_SIGNED": tn.SIGNED}
    assert (tn.MAX_COLS, tn.OUTER, tn.SIGNED) == (4, 1, 2)
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(tn.ENTRY_POINTS)
    assert (tm.OUTER, tm.SIGNED, tm.NO_ROW) == (tn.OUTER, tn.SIGNED, tn.NO_ROW)
    assert tn.SEGMENT_ROWS % 256 == 0  # whole groups of four entries per lane
    from dwarf_bench_amd import ops
    assert tm.KEY_RANGE == ops.DEV_KEY_RANGE


def test_workspace_query_keeps_its_bound(lib):
    text = HEADER.read_text()
    assert "at most 1024 + capacity / 128 and never more than 65792" in text
    S = tn.SEGMENT_ROWS
    last = 0
    for c in sorted(SIZES + (3, 4, 5, S - 1, S, S + 1, 2 * S + 3, 4 * S - 1, 4 * S, 4 * S + 1, 8191 * S, 8192 * S, 8192 * S + 1)):
        got = tn.workspace_bytes(c)
        assert got % 256 == 0 and 512 <= got <= min(1024 + c // 128, 65792) and got >= last, (c, got)
        # the header, and one 32-byte record per workgroup of four waves, a wave per segment, up to 2048 of them
        assert got >= 256 + 32 * min(max(-(-c // S) // 4, 1), 2048), (c, got)
        last = got
    assert tn.workspace_bytes(0) == 512 and tn.workspace_bytes((1 << 32) - 1) == 65792
    for c in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert tn.workspace_bytes(c) == 0, c


def _take(cols=None, k=1, n=N, rows=ROWS, count=None, cap=CAP, flags=0, fill=0, outs=None, w=WS, wb=None):
    if wb is None:
        wb = tn.workspace_bytes(cap) or 1 << 40
    cols = COLS[:k] if cols is None else cols
    outs = OUTS[:k] if outs is None else outs
    return tn.take(cols, k, n, rows, count, cap, flags, fill, outs, w, wb, None)


def _agg(col=COLS[0], n=N, rows=ROWS, count=None, cap=CAP, flags=0, out=OUT, w=WS, wb=None):
    if wb is None:
        wb = tn.workspace_bytes(cap) or 1 << 40
    return tn.aggregate(col, n, rows, count, cap, flags, out, w, wb, None)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for k in (1, 2, 3, 4):
        for kw in ({}, dict(flags=tn.OUTER), dict(count=COUNT), dict(fill=0xFFFFFFFF), dict(n=0, cols=[None] * k),
                   dict(cap=0, rows=None), dict(cap=0, rows=None, cols=[None] * k), dict(cap=0),
                   dict(cap=0, count=COUNT)):
            assert _take(k=k, wb=0, **kw) == EWORKSPACE, (k, kw)
    for kw in ({}, dict(flags=tn.OUTER), dict(flags=tn.SIGNED), dict(flags=tn.OUTER | tn.SIGNED), dict(count=COUNT),
               dict(rows=None), dict(rows=None, cap=0), dict(rows=None, n=0, col=None),
               dict(cap=0, col=None), dict(n=0, col=None)):
        assert _agg(wb=0, **kw) == EWORKSPACE, kw


def test_every_argument_error_of_take_one_at_a_time(lib):
    for flags in (tn.SIGNED, tn.SIGNED | tn.OUTER, 4, 8, 7, -1, 1 << 16):  # unknown flag bits, and SIGNED on take
        assert _take(flags=flags) == EINVAL, flags
    for k in (0, 5, 6, 1 << 16):  # n_cols outside 1..4
        assert tn.take(COLS, k, N, ROWS, None, CAP, 0, 0, OUTS, WS, 1 << 20, None) == EINVAL, k
    assert tn.take(None, 1, N, ROWS, None, CAP, 0, 0, OUTS, WS, 1 << 20, None) == EINVAL  # no array at all
    assert tn.take(COLS, 1, N, ROWS, None, CAP, 0, 0, None, WS, 1 << 20, None) == EINVAL
    for n, cap in ((1 << 32, CAP), (N, 1 << 32), ((1 << 32) + 5, 7), (1 << 40, 1 << 40)):  # a size of 2^32 or more
        assert _take(n=n, cap=cap) == EINVAL, (n, cap)
    for k in (1, 2, 3, 4):
        for c in range(k):
            cols, outs = list(COLS[:k]), list(OUTS[:k])
            cols[c] = None
            assert _take(k=k, cols=cols) == EINVAL, (k, c)  # a NULL column with n_rows > 0 and capacity > 0
            outs[c] = None
            assert _take(k=k, outs=outs) == EINVAL and _take(k=k, outs=outs, cap=0, rows=None) == EINVAL, (k, c)
    assert _take(rows=None) == EINVAL  # NULL rows with capacity > 0
    assert _take(rows=None, cap=0, count=COUNT) == EINVAL  # count without rows
    for off in (1, 2, 3):  # misaligned pointers
        assert _take(rows=ROWS + off) == EINVAL
        for k in (1, 4):
            for c in range(k):
                cols, outs = list(COLS[:k]), list(OUTS[:k])
                cols[c] += off
                outs[c] += off
                assert _take(k=k, cols=cols) == EINVAL and _take(k=k, outs=outs) == EINVAL, (k, c, off)
    for off in (1, 2, 4, 12):
        assert _take(count=COUNT + off) == EINVAL, off


def test_every_argument_error_of_aggregate_one_at_a_time(lib):
    for flags in (4, 8, 7, -1, 1 << 16):
        assert _agg(flags=flags) == EINVAL, flags
    for n, cap in ((1 << 32, CAP), (N, 1 << 32), ((1 << 32) + 5, 7)):
        assert _agg(n=n, cap=cap) == EINVAL, (n, cap)
    assert _agg(col=None) == EINVAL and _agg(col=None, rows=None) == EINVAL  # a NULL column with rows to read
    assert _agg(rows=None, count=COUNT) == EINVAL  # count without rows
    assert _agg(out=None) == EINVAL
    for off in (1, 2, 3):
        assert _agg(col=COLS[0] + off) == EINVAL and _agg(rows=ROWS + off) == EINVAL
    for off in (1, 2, 4, 12):
        assert _agg(count=COUNT + off) == EINVAL and _agg(out=OUT + off) == EINVAL, off


def test_outputs_may_not_overlap_inputs_or_each_other(lib):
    for k in (1, 2, 4):
        for c in range(k):
            def at(where, **kw):
                outs = list(OUTS[:k])
                outs[c] = where
                return _take(k=k, outs=outs, **kw)
            for col in COLS[:k]:  # against every input column: the column itself, one word shared at either end
                for where in (col, col + 4 * (N - 1), col - 4 * (CAP - 1)):
                    assert at(where) == EINVAL, (k, c, where)
                assert at(col + 4 * N, wb=0) == EWORKSPACE and at(col - 4 * CAP, wb=0) == EWORKSPACE  # touching ranges
            for where in (ROWS, ROWS + 4 * (CAP - 1), ROWS - 4 * (CAP - 1)):  # the list
                assert at(where) == EINVAL, (k, c, where)
            assert at(ROWS + 4 * CAP, wb=0) == EWORKSPACE
            assert at(COUNT, count=COUNT) == EINVAL and at(COUNT - 4 * (CAP - 1), count=COUNT) == EINVAL  # the count word
            assert at(COUNT + 8, count=COUNT, wb=0) == EWORKSPACE and at(COUNT, wb=0) == EWORKSPACE  # (no count given)
            for other in range(k):  # another output
                if other != c:
                    assert at(OUTS[other]) == EINVAL and at(OUTS[other] + 4 * (CAP - 1)) == EINVAL, (k, c, other)
                    assert at(OUTS[other] + 4 * CAP, wb=0) == EWORKSPACE
    # the aggregate's four result words
    for where in (COLS[0], COLS[0] + 4 * N - 8, COLS[0] - 24, ROWS, ROWS + 4 * CAP - 8, ROWS - 24):
        assert _agg(out=where) == EINVAL, where
    assert _agg(out=COLS[0] + 4 * N, wb=0) == EWORKSPACE and _agg(out=ROWS - 32, wb=0) == EWORKSPACE
    assert _agg(out=COUNT, count=COUNT) == EINVAL and _agg(out=COUNT - 24, count=COUNT) == EINVAL
    assert _agg(out=COUNT + 8, count=COUNT, wb=0) == EWORKSPACE
    assert _agg(out=ROWS, rows=None, wb=0) == EWORKSPACE  # over all rows there is no list to overlap


def test_workspace_errors_come_after_argument_errors(lib):
    full = tn.workspace_bytes(CAP)
    assert full > tn.workspace_bytes(0) == 512
    for call in (_take, _agg):
        assert call(wb=full - 1) == EWORKSPACE and call(wb=0) == EWORKSPACE and call(w=None) == EWORKSPACE
        assert call(w=WS + 64) == EWORKSPACE and call(w=WS + 128) == EWORKSPACE
        assert call(cap=0, rows=None, wb=511) == EWORKSPACE  # no entries: the header and one padded record
        assert call(flags=4, wb=0) == EINVAL and call(cap=1 << 32, wb=0) == EINVAL and call(rows=ROWS + 2, w=None) == EINVAL
        assert call(rows=None, count=COUNT, w=WS + 64) == EINVAL
    assert _take(flags=tn.SIGNED, wb=0) == EINVAL and _take(outs=[COLS[0]], w=None) == EINVAL
    assert _take(cols=[None], wb=full - 1) == EINVAL and _agg(out=None, wb=0) == EINVAL
    # the aggregate over all rows asks for the workspace of capacity 0, whatever capacity says
    assert _agg(rows=None, wb=511) == EWORKSPACE and _agg(rows=None, cap=1 << 20, wb=511) == EWORKSPACE


def test_ops_refuses_wrong_arguments_before_any_device_call():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("TakeRows", "take", "AggregateRows", "aggregate_rows"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.take(t, t), lambda: ops.take([t, t], t), lambda: ops.take(t.float(), t), lambda: ops.take(t.long(), t),
                 lambda: ops.aggregate_rows(t), lambda: ops.aggregate_rows(t, t), lambda: ops.aggregate_rows(t.float()),
                 lambda: ops.aggregate_rows(t.long(), t)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError, match="cols"):
        ops.take([], t)
    with pytest.raises(ValueError, match="8 rows"):
        ops.take([t, t[:8]], t)  # columns of different lengths
    for fill in (1 << 32, -(1 << 31) - 1, 1.5, True):
        with pytest.raises(ValueError, match="fill"):
            ops.take(t, t, fill=fill)
    plan = ops.TakeRows(16, 2, device="cpu")  # the plan itself is plain memory
    assert plan.ws_bytes == tn.workspace_bytes(16) and len(plan.outs) == 2 and all(o.numel() == 16 for o in plan.outs)
    agg = ops.AggregateRows(16, device="cpu")
    assert agg.ws_bytes == plan.ws_bytes and agg.out.numel() == 4 and agg.out.dtype == torch.int64
    for p in (plan, agg):
        with pytest.raises(ValueError):
            p.result()  # nothing launched yet
        with pytest.raises(ValueError):
            p.output()
    with pytest.raises(ValueError, match="on the GPU"):
        plan.launch(t, t)
    with pytest.raises(ValueError, match="cols"):
        plan.launch([t, t, t], t)  # more columns than the plan holds
    with pytest.raises(ValueError, match="on the GPU"):
        agg.launch(t, t)
    with pytest.raises(ValueError, match="count"):
        agg.launch(t, None, count=torch.zeros(1, dtype=torch.int64))
    for n_cols in (0, 5, -1):
        with pytest.raises(ValueError, match="n_cols"):
            ops.TakeRows(16, n_cols, device="cpu")
    for cls in (ops.TakeRows, ops.AggregateRows):
        for cap in (1 << 32, 1 << 40):
            with pytest.raises(ValueError):
                cls(cap, device="cpu")
    assert "take_rows.hpp" in ops.__doc__ and "select_rows.hpp" in ops.__doc__ and "merge_sorted.hpp" in ops.__doc__
