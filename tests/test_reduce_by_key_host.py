"""The reduce by key (include/dbhip_reduce_by_key.h) without a GPU: the workspace queries against the bounds the header
states, the host-side argument checks (all before any HIP call) and the tensor API's refusals."""
import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE, OK, SIZES


def test_workspace_queries():
    lib = _capi.lib()
    ws, cws = lib.dbhip_reduce_by_key_workspace_bytes, lib.dbhip_check_reduce_by_key_workspace_bytes
    for n in SIZES:
        got = ws(n)
        # include/dbhip_reduce_by_key.h: 2048 + n / 64; and it holds 56 bytes per 4096-row segment behind the header
        assert got % 256 == 0 and 256 <= got <= 2048 + n // 64, (n, got)
        assert got >= 256 + 56 * ((n + 4095) // 4096), (n, got)
        assert n + 5 >= 1 << 32 or ws(n + 5) >= got
        for runs in (0, 1, 1000, n):
            c = cws(n, runs)
            # two words per run, a header, the scan's own workspace
            assert c % 256 == 0 and c >= 256 + 8 * runs + lib.dbhip_exclusive_scan_u32_workspace_bytes(runs), (n, runs)
            assert c <= 1024 + 8 * runs + lib.dbhip_exclusive_scan_u32_workspace_bytes(runs), (n, runs)
    for n in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert ws(n) == 0 and cws(n, 5) == 0 and cws(5, n) == 0, n


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fn = lib.dbhip_reduce_by_key_u32
    fake = 1 << 20  # 256-byte aligned, never dereferenced: every call below fails on the host first
    n = 100003
    cols = ("ok", "oc", "osum", "omn", "omx")

    def call(keys=fake, vals=fake, n=n, signed=0, ok=fake, oc=fake, osum=fake, omn=fake, omx=fake, cap=1000, runs=fake,
             w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_reduce_by_key_workspace_bytes(n) or 1 << 40
        return fn(keys, vals, n, signed, ok, oc, osum, omn, omx, cap, runs, w, wb, None)

    none = dict.fromkeys(cols)
    for signed in (0, 1):
        kw = dict(signed=signed)
        assert call(n=1 << 32, **kw) == EINVAL and call(n=(1 << 32) + 7, **kw) == EINVAL
        assert call(keys=None, **kw) == EINVAL and call(runs=None, **kw) == EINVAL  # n > 0
        assert call(cap=0, **kw) == EINVAL  # columns without room
        for c in cols:
            assert call(cap=0, **{**none, c: fake}, **kw) == EINVAL
        assert call(**none, **kw) == EINVAL  # room without a column
        assert call(vals=None, **kw) == EINVAL  # a value aggregate without values
        for c in cols[2:]:
            assert call(vals=None, **{**none, c: fake}, **kw) == EINVAL
        for off in (4, 8, 12):
            assert call(keys=fake + off, **kw) == EINVAL and call(vals=fake + off, **kw) == EINVAL
            for c in cols:
                assert call(**{c: fake + off}, **kw) == EINVAL
        full = lib.dbhip_reduce_by_key_workspace_bytes(n)
        assert call(wb=full - 1, **kw) == EWORKSPACE and call(wb=0, **kw) == EWORKSPACE and call(w=None, **kw) == EWORKSPACE
        assert call(w=fake + 64, **kw) == EWORKSPACE and call(w=fake + 128, **kw) == EWORKSPACE
        assert call(cap=0, **none, wb=full - 1, **kw) == EWORKSPACE  # the count-only call needs its workspace too
        assert call(n=n + 20 * 4096, wb=full, **kw) == EWORKSPACE  # a workspace sized for fewer rows
        # an argument error comes before the workspace error
        assert call(keys=None, wb=0, **kw) == EINVAL and call(runs=None, w=fake + 64, **kw) == EINVAL
        assert call(oc=fake + 4, wb=0, **kw) == EINVAL and call(n=1 << 32, w=None, **kw) == EINVAL
        assert call(cap=0, w=None, **kw) == EINVAL and call(**none, wb=0, **kw) == EINVAL
        # empty calls: fine without a workspace, a run counter and input columns; a workspace that is passed is checked
        assert call(keys=None, vals=None, n=0, **none, cap=0, runs=None, w=None, wb=0, **kw) == OK
        assert call(keys=None, vals=None, n=0, **none, cap=0, runs=None, w=fake + 64, **kw) == EWORKSPACE
        assert call(keys=None, vals=None, n=0, **none, cap=0, runs=None, wb=8, **kw) == EWORKSPACE
        assert call(keys=fake + 4, n=0, **none, cap=0, runs=None, w=None, **kw) == EINVAL  # the alignment rule still holds
        assert call(n=0, cap=0, runs=None, w=None, **kw) == EINVAL  # and so does the capacity rule


def test_validator_argument_errors_need_no_device():
    lib = _capi.lib()
    chk = lib.dbhip_check_reduce_by_key_u32
    fake = 1 << 20
    cols = ("ok", "oc", "osum", "omn", "omx")

    def call(keys=fake, vals=fake, n=100, signed=0, ok=fake, oc=fake, osum=fake, omn=fake, omx=fake, runs=10, res=fake,
             w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_check_reduce_by_key_workspace_bytes(n, runs) or 1 << 40
        return chk(keys, vals, n, signed, ok, oc, osum, omn, omx, runs, res, w, wb, None)

    assert call(res=None) == EINVAL and call(keys=None) == EINVAL and call(vals=None) == EINVAL
    for c in cols:
        assert call(**{c: None}) == EINVAL
    assert call(n=1 << 32) == EINVAL and call(runs=1 << 32, signed=1) == EINVAL
    assert call(res=None, n=0, runs=0, keys=None, vals=None) == EINVAL
    full = lib.dbhip_check_reduce_by_key_workspace_bytes(100, 10)
    assert call(wb=full - 1) == EWORKSPACE and call(w=None) == EWORKSPACE and call(w=fake + 64) == EWORKSPACE
    assert call(keys=None, wb=0) == EINVAL and call(res=None, w=None) == EINVAL  # an argument error comes first


def test_ops_has_the_plan_and_refuses_host_tensors_wrong_types_and_slices():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("ReduceByKey", "reduce_by_key", "groupby_sorted", "check_reduce_by_key", "REDUCE_BY_KEY_CHUNK_ROWS",
                 "REDUCE_BY_KEY_SEGMENT_ROWS"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.reduce_by_key(t, t), lambda: ops.groupby_sorted(t, t),
                 lambda: ops.check_reduce_by_key(t, t, t[:3], t[:3], t[:3].long(), t[:3], t[:3])):
        with pytest.raises(ValueError, match="on the GPU"):
            call()  # not on the GPU
    with pytest.raises(ValueError, match="on the GPU"):
        ops.groupby_sorted(t.float(), t)  # nor the right type
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what ReduceByKey.launch asks of its columns: a t[1:] slice starts 4 bytes off
    with pytest.raises(ValueError):
        ops.ReduceByKey(1 << 32, 1, device="cpu")
    with pytest.raises(ValueError):
        ops.ReduceByKey(16, -1, device="cpu")
