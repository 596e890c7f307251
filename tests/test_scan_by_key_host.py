"""The scan by key (include/dbhip_scan_by_key.h) without a GPU: the workspace queries against the bound the header states,
the host-side argument checks (all before any HIP call, in the header's order) and the tensor API's refusals."""
import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE, INCLUDE, OK, SIZES

HEADER = "dbhip_scan_by_key.h"
COLS = ("run", "num", "osum", "omn", "omx")


def test_workspace_queries():
    lib = _capi.lib()
    ws, cws = lib.dbhip_scan_by_key_workspace_bytes, lib.dbhip_check_scan_by_key_workspace_bytes
    header = (INCLUDE / HEADER).read_text()
    assert "dbhip_scan_by_key_workspace_bytes(n) <= 2048 + n / 64, a multiple of 256" in header
    for n in SIZES:
        got = ws(n)
        # include/dbhip_scan_by_key.h: 2048 + n / 64; and it holds 64 bytes per 4096-row segment behind the header
        assert got % 256 == 0 and 256 <= got <= 2048 + n // 64, (n, got)
        assert got >= 256 + 64 * ((n + 4095) // 4096), (n, got)
        assert n + 5 >= 1 << 32 or ws(n + 5) >= got
        assert cws(n) == 256  # a bare header
    for n in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert ws(n) == 0 and cws(n) == 0, n


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fn = lib.dbhip_scan_by_key_u32
    fake = 1 << 20  # 256-byte aligned, never dereferenced: every call below fails on the host first
    n = 100003

    def call(keys=fake, vals=fake, n=n, signed=0, run=fake, num=fake, osum=fake, omn=fake, omx=fake, w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_scan_by_key_workspace_bytes(n) or 1 << 40
        return fn(keys, vals, n, signed, run, num, osum, omn, omx, w, wb, None)

    none = dict.fromkeys(COLS)
    for signed in (0, 1):
        kw = dict(signed=signed)
        assert call(n=1 << 32, **kw) == EINVAL and call(n=(1 << 32) + 7, **kw) == EINVAL
        assert call(keys=None, **kw) == EINVAL  # n > 0
        assert call(**none, **kw) == EINVAL and call(vals=None, **none, **kw) == EINVAL  # no column at all
        assert call(vals=None, **kw) == EINVAL  # a value column without values
        for c in COLS[2:]:
            assert call(vals=None, **{**none, c: fake}, **kw) == EINVAL
        for off in (4, 8, 12):
            assert call(keys=fake + off, **kw) == EINVAL and call(vals=fake + off, **kw) == EINVAL
            for c in COLS:
                assert call(**{c: fake + off}, **kw) == EINVAL
                assert call(**{**none, c: fake + off}, **kw) == EINVAL
        full = lib.dbhip_scan_by_key_workspace_bytes(n)
        assert call(wb=full - 1, **kw) == EWORKSPACE and call(wb=0, **kw) == EWORKSPACE and call(w=None, **kw) == EWORKSPACE
        assert call(w=fake + 64, **kw) == EWORKSPACE and call(w=fake + 128, **kw) == EWORKSPACE
        assert call(n=n + 20 * 4096, wb=full, **kw) == EWORKSPACE  # a workspace sized for fewer rows
        for c in COLS[:2]:  # the key-only columns need no values, but their workspace
            assert call(vals=None, **{**none, c: fake}, wb=full - 1, **kw) == EWORKSPACE
        # an argument error comes before the workspace error
        assert call(keys=None, wb=0, **kw) == EINVAL and call(**none, w=fake + 64, **kw) == EINVAL
        assert call(num=fake + 4, wb=0, **kw) == EINVAL and call(n=1 << 32, w=None, **kw) == EINVAL
        assert call(vals=None, w=None, **kw) == EINVAL
        # a call that is wrong in every way at once is still an argument error
        assert call(n=1 << 32, keys=None, vals=None, **none, w=fake + 64, wb=0, **kw) == EINVAL
        # empty calls: fine without a workspace and without columns; a workspace that is passed is checked
        assert call(keys=None, vals=None, n=0, **none, w=None, wb=0, **kw) == OK
        assert call(keys=None, vals=None, n=0, **none, w=fake + 64, **kw) == EWORKSPACE
        assert call(keys=None, vals=None, n=0, **none, wb=8, **kw) == EWORKSPACE
        assert call(keys=fake + 4, n=0, **none, w=None, **kw) == EINVAL  # the alignment rule still holds
        assert call(n=0, omx=fake + 8, w=None, **kw) == EINVAL
        assert call(vals=None, n=0, w=None, **kw) == EINVAL  # and so does the values rule


def test_validator_argument_errors_need_no_device():
    lib = _capi.lib()
    chk = lib.dbhip_check_scan_by_key_u32
    fake = 1 << 20

    def call(keys=fake, vals=fake, n=100, signed=0, run=fake, num=fake, osum=fake, omn=fake, omx=fake, res=fake, w=fake,
             wb=256):
        return chk(keys, vals, n, signed, run, num, osum, omn, omx, res, w, wb, None)

    none = dict.fromkeys(COLS)
    assert call(res=None) == EINVAL and call(res=fake + 4) == EINVAL and call(keys=None) == EINVAL
    assert call(**none) == EINVAL and call(vals=None) == EINVAL
    for c in COLS[2:]:
        assert call(vals=None, **{**none, c: fake}) == EINVAL
    assert call(n=1 << 32) == EINVAL and call(n=1 << 32, signed=1) == EINVAL
    assert call(res=None, n=0, keys=None, vals=None) == EINVAL
    assert call(wb=255) == EWORKSPACE and call(w=None) == EWORKSPACE and call(w=fake + 64) == EWORKSPACE
    for c in COLS[:2]:
        assert call(vals=None, **{**none, c: fake}, wb=0) == EWORKSPACE  # key-only columns: a valid call
    assert call(keys=None, wb=0) == EINVAL and call(res=None, w=None) == EINVAL  # an argument error comes first


def test_ops_has_the_plan_and_refuses_host_tensors_wrong_types_and_slices():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("ScanByKey", "scan_by_key", "window_sorted", "check_scan_by_key", "SCAN_BY_KEY_CHUNK_ROWS",
                 "SCAN_BY_KEY_SEGMENT_ROWS"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.scan_by_key(t, t), lambda: ops.window_sorted(t, t),
                 lambda: ops.check_scan_by_key(t, t, t, t, t.long(), t, t)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()  # not on the GPU
    with pytest.raises(ValueError, match="on the GPU"):
        ops.window_sorted(t.float(), t)  # nor the right type
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what ScanByKey.launch asks of its columns: a t[1:] slice starts 4 bytes off
    with pytest.raises(ValueError):
        ops.ScanByKey(1 << 32, device="cpu")
    with pytest.raises(ValueError):
        ops.ScanByKey(-1, device="cpu")
    plan = ops.ScanByKey(16, device="cpu")  # the plan itself is plain memory; launch refuses what it is given
    with pytest.raises(ValueError, match="on the GPU"):
        plan.launch(t, t)
