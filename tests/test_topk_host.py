"""The top-k (include/dbhip_topk.h) without a GPU: the workspace query against the bound the header states, the host-side
argument checks (all before any HIP call) and the tensor API's refusals."""
import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE, OK, SIZES


def test_workspace_query():
    lib = _capi.lib()
    ws = lib.dbhip_topk_workspace_bytes
    for n in SIZES:
        for k in (0, 1, 1024, n):
            m = min(k, n)
            got = ws(n, k)
            # include/dbhip_topk.h: 4 MiB + n / 128 + 16 min(k, n)
            assert got % 256 == 0 and 256 <= got <= (4 << 20) + n // 128 + 16 * m, (n, k, got)
            # and it holds what the call carves from it: two words per segment twice, four columns of m, the sort's own
            assert got >= 256 + 16 * ((n + 4095) // 4096) + 16 * m + lib.dbhip_radix_sort_pairs_workspace_bytes(m, 8), (n, k)
            assert ws(n, k + 5) >= got
    for n in (1 << 32, (1 << 32) + 1, 1 << 40):
        for k in (0, 1, 1024, n):
            assert ws(n, k) == 0, (n, k)


@pytest.mark.parametrize("name", ["dbhip_topk_u32", "dbhip_topk_i32"])
def test_argument_errors_need_no_device(name):
    lib = _capi.lib()
    fn = getattr(lib, name)
    fake = 1 << 20  # 256-byte aligned, never dereferenced: every call below fails on the host first
    n = 100003

    def call(keys=fake, n=n, k=1000, largest=0, srt=1, ok=fake, orow=fake, w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_topk_workspace_bytes(n, k) or 1 << 40
        return fn(keys, n, k, largest, srt, ok, orow, w, wb, None)

    for largest in (0, 1):
        for srt in (0, 1):
            kw = dict(largest=largest, srt=srt)
            assert call(keys=None, **kw) == EINVAL  # n > 0
            assert call(keys=None, k=0, **kw) == EINVAL  # also when nothing is asked for
            assert call(ok=None, **kw) == EINVAL and call(orow=None, **kw) == EINVAL  # m > 0
            assert call(n=1 << 32, **kw) == EINVAL and call(n=(1 << 32) + 7, k=1, **kw) == EINVAL
            for off in (4, 8, 12):
                assert call(keys=fake + off, **kw) == EINVAL
                assert call(ok=fake + off, **kw) == EINVAL and call(orow=fake + off, **kw) == EINVAL
            full = lib.dbhip_topk_workspace_bytes(n, 1000)
            assert call(wb=full - 1, **kw) == EWORKSPACE and call(wb=0, **kw) == EWORKSPACE
            assert call(w=None, **kw) == EWORKSPACE
            assert call(w=fake + 64, **kw) == EWORKSPACE and call(w=fake + 128, **kw) == EWORKSPACE
            # a workspace sized for a smaller k does not do for a larger one
            assert call(k=5000, wb=full, **kw) == EWORKSPACE
            # an argument error comes before the workspace error
            assert call(keys=None, wb=0, **kw) == EINVAL and call(ok=None, w=fake + 64, **kw) == EINVAL
            assert call(orow=fake + 4, wb=0, **kw) == EINVAL and call(n=1 << 32, w=None, **kw) == EINVAL
            # empty calls: fine without a workspace and without output columns; a workspace that is passed is checked
            assert call(k=0, ok=None, orow=None, w=None, wb=0, **kw) == OK
            assert call(keys=None, n=0, ok=None, orow=None, w=None, wb=0, **kw) == OK
            assert call(k=0, w=fake + 64, **kw) == EWORKSPACE and call(k=0, wb=8, **kw) == EWORKSPACE
            assert call(keys=None, n=0, w=fake + 128, **kw) == EWORKSPACE
            assert call(keys=fake + 4, k=0, w=None, **kw) == EINVAL  # the alignment rule holds for an empty call too


def test_validator_argument_errors_need_no_device():
    chk = _capi.lib().dbhip_check_topk_u32
    fake = 1 << 20

    def call(keys=fake, n=100, ok=fake, orow=fake, k=10, largest=0, signed=0, res=fake):
        return chk(keys, n, ok, orow, k, largest, signed, res, None)

    assert call(res=None) == EINVAL and call(keys=None) == EINVAL
    assert call(ok=None) == EINVAL and call(orow=None) == EINVAL
    assert call(n=1 << 32) == EINVAL and call(n=(1 << 32) + 1, largest=1, signed=1) == EINVAL
    assert call(res=None, k=0) == EINVAL and call(res=None, n=0, keys=None) == EINVAL


def test_ops_has_the_plan_and_refuses_host_tensors_and_slices():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("TopK", "topk", "check_topk", "TOPK_CHUNK_ROWS", "TOPK_SEGMENT_ROWS"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.topk(t, 3)  # not on the GPU
    with pytest.raises(ValueError):
        ops.check_topk(t, t[:3], t[:3])
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what TopK.launch asks of its column: a t[1:] slice starts 4 bytes off
