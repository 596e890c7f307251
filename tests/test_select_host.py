"""The selection vectors (dwarf_bench_amd/host/select_rows.hpp, in libdbench.so) without a GPU: the exported symbols, the
header's constants against the binding's, the workspace query's bound, the host-side argument checks (all before any
HIP call, argument errors before workspace errors) and the tensor API's refusals.  Every call below fails on the host:
the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import select_native as sn
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "select_rows.hpp"
FAKE = 1 << 20  # 256-byte aligned
N, CAP = 100003, 5000


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return sn.lib()


def test_libdbench_exports_exactly_the_two_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_select_\w+)$", out, flags=re.M))
    assert names == ["dbench_select_range_u32", "dbench_select_workspace_bytes"] == sorted(sn.ENTRY_POINTS)
    assert not re.findall(r"\bdbhip_\w*select\w*$", out, flags=re.M)  # the dbhip_* surface is the headers' under include/


def test_header_constants_are_the_bindings():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_SELECT_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_SELECT_SEGMENT_ROWS": sn.SEGMENT_ROWS, "DBENCH_SELECT_SIGNED": sn.SIGNED,
                   "DBENCH_SELECT_NEGATE": sn.NEGATE}
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(sn.ENTRY_POINTS)
    from tests import select_model as sm
    assert (sm.SIGNED, sm.NEGATE) == (sn.SIGNED, sn.NEGATE)
    from dwarf_bench_amd import ops
    assert sm.KEY_RANGE == ops.DEV_KEY_RANGE


def test_workspace_query_keeps_its_bound(lib):
    assert "at most 4096 + c / 4" in HEADER.read_text()
    last = 0
    for c in sorted(SIZES + (63, 64, 65, 4095, 4097, 32767, 32768, 32769, (1 << 22) + 4097)):
        got = sn.workspace_bytes(c)
        assert got % 256 == 0 and 256 <= got <= 4096 + c // 4 and got >= last, (c, got)
        assert got >= 256 + c // 8  # the header and one mask bit per candidate
        last = got
    for c in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert sn.workspace_bytes(c) == 0, c


def _call(col=FAKE, n=N, rows=None, count=None, cap=0, lo=1, hi=2, flags=0, out=FAKE + (1 << 24), out_count=FAKE + (1 << 26),
          w=FAKE + (1 << 27), wb=None):
    if wb is None:
        wb = sn.workspace_bytes(cap if rows else n) or 1 << 40
    return sn.select_range(col, n, rows, count, cap, lo, hi, flags, out, out_count, w, wb, None)


LIST = dict(rows=FAKE + (1 << 25), cap=CAP)


def test_every_argument_error_one_at_a_time(lib):
    for flags in (4, 8, 7, -1, 1 << 16):  # unknown flag bits
        assert _call(flags=flags) == EINVAL, flags
    assert _call(n=1 << 32) == EINVAL and _call(n=(1 << 32) + 5) == EINVAL  # a size out of range
    assert _call(cap=1 << 32, **{k: v for k, v in LIST.items() if k != "cap"}) == EINVAL
    assert _call(cap=1 << 32) == EINVAL  # also where the list is absent
    assert _call(col=None) == EINVAL  # col NULL with n_col > 0
    assert _call(out_count=None) == EINVAL
    assert _call(count=FAKE + (1 << 23)) == EINVAL  # in_count without in_rows
    for off in (1, 2, 3):  # misaligned pointers
        assert _call(col=FAKE + off) == EINVAL
        assert _call(out=FAKE + (1 << 24) + off) == EINVAL
        assert _call(rows=LIST["rows"] + off, cap=CAP) == EINVAL
    for off in (1, 2, 4, 12):
        assert _call(out_count=FAKE + (1 << 26) + off) == EINVAL
        assert _call(count=FAKE + (1 << 23) + off, **LIST) == EINVAL


def test_out_rows_may_not_overlap_an_input(lib):
    assert _call(out=FAKE) == EINVAL  # the column itself
    assert _call(out=FAKE + 4 * (N - 1)) == EINVAL and _call(out=FAKE - 4 * (N - 1)) == EINVAL  # one word shared
    assert _call(out=LIST["rows"], **LIST) == EINVAL
    assert _call(out=LIST["rows"] + 4 * (CAP - 1), **LIST) == EINVAL
    assert _call(out=LIST["rows"] - 4 * (CAP - 1), **LIST) == EINVAL
    assert _call(out=FAKE + 4 * (N - 1), **LIST) == EINVAL  # the column, in list mode
    # touching ranges do not overlap: these calls get as far as the workspace check
    assert _call(out=FAKE + 4 * N, wb=0) == EWORKSPACE and _call(out=FAKE - 4 * N, wb=0) == EWORKSPACE
    assert _call(out=LIST["rows"] + 4 * CAP, wb=0, **LIST) == EWORKSPACE
    assert _call(out=LIST["rows"] - 4 * CAP, wb=0, **LIST) == EWORKSPACE


def test_workspace_errors_come_after_argument_errors(lib):
    full = sn.workspace_bytes(N)
    assert _call(wb=full - 1) == EWORKSPACE and _call(wb=0) == EWORKSPACE and _call(w=None) == EWORKSPACE
    assert _call(w=FAKE + (1 << 27) + 64) == EWORKSPACE and _call(w=FAKE + (1 << 27) + 128) == EWORKSPACE
    assert _call(wb=sn.workspace_bytes(CAP) - 1, **LIST) == EWORKSPACE
    assert _call(n=0, col=None, wb=255) == EWORKSPACE and _call(n=0, col=None, w=None) == EWORKSPACE  # no rows: the header
    assert _call(out=None, wb=full - 1) == EWORKSPACE  # the count-only call needs all of it too
    assert _call(count=FAKE + (1 << 23), wb=0, **LIST) == EWORKSPACE  # a valid list call
    # an argument error comes first
    assert _call(flags=4, wb=0) == EINVAL and _call(col=None, w=None) == EINVAL
    assert _call(out_count=None, wb=full - 1) == EINVAL and _call(out=FAKE, w=FAKE + 64) == EINVAL
    assert _call(count=FAKE + (1 << 23), wb=0) == EINVAL and _call(col=FAKE + 2, wb=0) == EINVAL
    assert _call(n=1 << 32, wb=0) == EINVAL


def test_ops_refuses_host_tensors_wrong_types_and_bounds_out_of_range():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("SelectRows", "select_range", "semi_join"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.select_range(t, 0, 1), lambda: ops.select_range(t.float(), 0, 1),
                 lambda: ops.select_range(t.long(), 0, 1), lambda: ops.semi_join(t, t)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    for lo, hi, signed in ((-1, 5, False), (0, 1 << 32, False), (0, 1 << 31, True), (-(1 << 31) - 1, 0, True),
                           (0.5, 1, False), (0, None, False), (True, 1, False)):
        with pytest.raises(ValueError, match="lo|hi"):
            ops.select_range(t, lo, hi, signed=signed)
    assert ops._bounds(-1, -(1 << 31), True) == (0xFFFFFFFF, 0x80000000)
    assert ops._bounds(0, (1 << 32) - 1, False) == (0, 0xFFFFFFFF)
    plan = ops.SelectRows(16, device="cpu")  # the plan itself is plain memory
    assert plan.ws_bytes == sn.workspace_bytes(16) and len(plan.rows) == 2
    with pytest.raises(ValueError, match="on the GPU"):
        plan.launch(t, 0, 1)
    with pytest.raises(ValueError):
        plan.refine(t, 0, 1)  # nothing launched yet
    with pytest.raises(ValueError):
        ops.SelectRows(1 << 32, device="cpu")
    doc = ops.semi_join.__doc__
    assert "0xFFFFFFFF" in doc and "dropped" in doc
    assert "select_rows.hpp" in ops.__doc__
