"""The join's pair table (dbhip_join_pairs_u32, dbhip_check_join_pairs_u32) without a GPU: the workspace query and the
host-side argument checks (all before any HIP call)."""
import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE


def test_workspace_query():
    ws = _capi.lib().dbhip_join_pairs_workspace_bytes
    for n in (0, 1, 1023, 1024, 1025, 4096, 100003, 1 << 20, (1 << 22) + 1, 1 << 24, (1 << 24) + 5, 1 << 30, (1 << 32) - 1):
        assert ws(n) % 256 == 0 and ws(n) >= 256 + 8 * n, n  # a 64-bit offset per probe row behind the header
    for n in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert ws(n) == 0, n


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fn = lib.dbhip_join_pairs_u32
    fake = 1 << 20  # 256-aligned, never dereferenced: every call below fails on the host first
    n = 100003

    def call(ids=fake, nb=5000, rid=None, pos=fake, cnt=fake, n=n, outer=0, cap=1000, ob=fake, op=fake, total=fake, w=fake,
             wb=None):
        if wb is None:
            wb = lib.dbhip_join_pairs_workspace_bytes(n) or 1 << 40
        return fn(ids, nb, rid, pos, cnt, n, outer, cap, ob, op, total, w, wb, None)

    for outer in (0, 1):
        assert call(ids=None, outer=outer) == EINVAL  # n_build > 0
        assert call(pos=None, outer=outer) == EINVAL and call(cnt=None, outer=outer) == EINVAL
        assert call(total=None, outer=outer) == EINVAL
        assert call(w=None, outer=outer) == EINVAL  # no workspace at all with n_probe > 0: an argument error
        assert call(ob=None, outer=outer) == EINVAL and call(op=None, outer=outer) == EINVAL  # capacity > 0
        assert call(ob=None, op=None, outer=outer) == EINVAL
        assert call(n=1 << 32, outer=outer) == EINVAL and call(n=(1 << 32) + 7, outer=outer) == EINVAL
        assert call(nb=(1 << 31) + 1, outer=outer) == EINVAL
        wsb = lib.dbhip_join_pairs_workspace_bytes(n)
        assert call(wb=wsb - 1, outer=outer) == EWORKSPACE and call(wb=0, outer=outer) == EWORKSPACE
        assert call(w=fake + 64, outer=outer) == EWORKSPACE and call(w=fake + 128, outer=outer) == EWORKSPACE
        # an argument error comes before the workspace error
        assert call(pos=None, wb=0, outer=outer) == EINVAL and call(ob=None, w=fake + 64, outer=outer) == EINVAL
        # n_probe == 0: a workspace that is passed is still checked
        assert call(n=0, w=fake + 64, outer=outer) == EWORKSPACE and call(n=0, wb=8, outer=outer) == EWORKSPACE
        assert call(n=0, ob=None, outer=outer) == EINVAL  # a capacity without its column


def test_validator_argument_errors_need_no_device():
    chk = _capi.lib().dbhip_check_join_pairs_u32
    fake = 1 << 20

    def call(bk=fake, nb=100, pk=fake, npr=50, ids=fake, rid=None, pos=fake, cnt=fake, outer=0, ob=fake, op=fake, pairs=70,
             res=fake):
        return chk(bk, nb, pk, npr, ids, rid, pos, cnt, outer, ob, op, pairs, res, None)

    assert call(res=None) == EINVAL
    assert call(bk=None) == EINVAL and call(pk=None) == EINVAL and call(ids=None) == EINVAL
    assert call(pos=None) == EINVAL and call(cnt=None) == EINVAL
    assert call(ob=None) == EINVAL and call(op=None) == EINVAL
    assert call(npr=1 << 32) == EINVAL and call(nb=(1 << 31) + 1) == EINVAL


def test_ops_has_the_plan_and_refuses_host_tensors():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("JoinPairs", "join_pairs", "check_join_pairs"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.check_join_pairs(t, t, t, t, t, t, t)  # not on the GPU
