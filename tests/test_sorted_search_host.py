"""The sorted search (include/dbhip_sorted_search.h) without a GPU: the workspace query against the model and the bound the
header states, the host-side argument checks (all before any HIP call, in the header's order), the tensor API's refusals and no
scratch in the kernels."""
import re
import subprocess

import pytest

from dwarf_bench_amd import _capi
from tests import sorted_search_model as sm
from tests.capi_testlib import EINVAL, EWORKSPACE, INCLUDE, OK, ROOT, SIZES
from tests.test_sorted_search_model import BOUNDARIES

HEADER = "dbhip_sorted_search.h"


def test_workspace_query_is_the_model_and_keeps_its_bound():
    lib = _capi.lib()
    ws, cws = lib.dbhip_sorted_index_workspace_bytes, lib.dbhip_check_sorted_search_workspace_bytes
    header = (INCLUDE / HEADER).read_text()
    assert "dbhip_sorted_index_workspace_bytes(m, top_entries) <= 1536 + m / 15" in header
    for top in (0,) + sm.TOPS:
        for m in BOUNDARIES + (4095, 4096, 4097, 262145, 100003):
            got = ws(m, top)
            assert got == sm.workspace_bytes(m, top) and got % 256 == 0 and 256 <= got <= 1536 + m // 15, (m, top, got)
    assert ws(16384, 0) == 256 and ws(16385, 0) == 256 + 1280 and ws(65, 64) == 512
    for m in ((1 << 31) + 1, 1 << 32, 1 << 40):
        assert ws(m, 0) == 0 and ws(m, 64) == 0, m
    for bad in (1, 2, 32, 63, 65, 96, 1000, 16383, 16385, 32768, 1 << 31):
        assert ws(1000, bad) == 0, bad
    for n in SIZES:
        assert cws(n) == 256
    assert cws(1 << 32) == 0 and cws(1 << 40) == 0


def test_index_build_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20  # 256-byte aligned, never dereferenced: every call below fails on the host first
    m = 100003

    def call(s=fake, m=m, signed=0, top=0, w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_sorted_index_workspace_bytes(m, top) or 1 << 40
        return lib.dbhip_sorted_index_build_u32(s, m, signed, top, w, wb, None)

    for signed in (0, 1):
        kw = dict(signed=signed)
        assert call(m=(1 << 31) + 1, **kw) == EINVAL
        for bad in (1, 63, 65, 96, 32768):
            assert call(top=bad, **kw) == EINVAL
        assert call(s=None, **kw) == EINVAL
        full = lib.dbhip_sorted_index_workspace_bytes(m, 0)
        assert call(wb=full - 1, **kw) == EWORKSPACE and call(wb=0, **kw) == EWORKSPACE and call(w=None, **kw) == EWORKSPACE
        assert call(w=fake + 64, **kw) == EWORKSPACE and call(w=fake + 128, **kw) == EWORKSPACE
        assert call(top=64, wb=full, **kw) == EWORKSPACE  # a deeper ladder needs more
        # an argument error comes before the workspace error, and in the header's order
        assert call(s=None, wb=0, **kw) == EINVAL and call(top=65, w=None, **kw) == EINVAL
        assert call(m=(1 << 31) + 1, top=65, s=None, w=fake + 64, wb=0, **kw) == EINVAL
        assert call(s=None, m=0, w=None, **kw) == EWORKSPACE  # m == 0 needs no column, but its header


def test_search_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20
    m, n = 100003, 5000

    def call(s=fake, m=m, lo=fake, hi=fake, n=n, pos=fake, cnt=fake, w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_sorted_index_workspace_bytes(m, 0) or 1 << 40
        return lib.dbhip_sorted_search_u32(s, m, lo, hi, n, pos, cnt, w, wb, None)

    assert call(m=(1 << 31) + 1) == EINVAL and call(n=1 << 32) == EINVAL and call(n=(1 << 32) + 7) == EINVAL
    assert call(lo=None, hi=None) == EINVAL
    assert call(pos=None, cnt=None) == EINVAL
    assert call(cnt=None) == EINVAL  # hi given without a count column
    assert call(s=None) == EINVAL
    for off in (4, 8, 12):
        for name in ("lo", "hi", "pos", "cnt"):
            assert call(**{name: fake + off}) == EINVAL, (name, off)
            assert call(**{name: fake + off}, n=0) == EINVAL  # the alignment rule holds for an empty call too
        assert call(s=fake + off, n=0) == OK  # the column needs only its natural alignment
    full = lib.dbhip_sorted_index_workspace_bytes(m, 0)
    assert call(wb=full - 1) == EWORKSPACE and call(wb=0) == EWORKSPACE and call(w=None) == EWORKSPACE
    assert call(w=fake + 64) == EWORKSPACE and call(w=fake + 128) == EWORKSPACE
    assert call(m=1 << 26, wb=full) == EWORKSPACE  # no index of 2^26 entries is that short
    # an argument error comes before the workspace error, and in the header's order
    assert call(lo=None, hi=None, wb=0) == EINVAL and call(cnt=None, w=None) == EINVAL
    assert call(lo=fake + 4, w=fake + 64) == EINVAL and call(s=None, wb=0) == EINVAL
    assert call(m=(1 << 31) + 1, lo=None, hi=None, pos=None, cnt=None, s=None, w=fake + 64, wb=0) == EINVAL
    # valid shapes with no rows: nothing is launched
    assert call(n=0) == OK and call(n=0, hi=None, cnt=None) == OK and call(n=0, lo=None, pos=None) == OK
    assert call(n=0, s=None) == OK and call(n=0, m=0, s=None) == OK
    assert call(n=0, w=None) == EWORKSPACE and call(n=0, wb=255) == EWORKSPACE


def test_validator_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20

    def call(s=fake, m=1000, signed=0, lo=fake, hi=fake, n=100, pos=fake, cnt=fake, res=fake, w=fake, wb=256):
        return lib.dbhip_check_sorted_search_u32(s, m, signed, lo, hi, n, pos, cnt, res, w, wb, None)

    assert call(res=None) == EINVAL and call(res=fake + 4) == EINVAL
    assert call(m=(1 << 31) + 1) == EINVAL and call(n=1 << 32) == EINVAL
    assert call(lo=None, hi=None) == EINVAL and call(pos=None, cnt=None) == EINVAL and call(cnt=None) == EINVAL
    assert call(pos=None) == EINVAL  # lo and cnt given: the end needs pos
    assert call(s=None) == EINVAL
    assert call(wb=255) == EWORKSPACE and call(w=None) == EWORKSPACE and call(w=fake + 64) == EWORKSPACE
    assert call(lo=None, pos=None, wb=0) == EWORKSPACE and call(hi=None, cnt=None, wb=0) == EWORKSPACE  # valid calls
    assert call(lo=fake + 4, hi=fake + 8, pos=fake + 12, cnt=fake + 4, wb=0) == EWORKSPACE  # natural alignment is enough
    assert call(res=None, w=None) == EINVAL and call(s=None, wb=0) == EINVAL  # an argument error comes first


def test_ops_has_the_plan_and_refuses_host_tensors_wrong_types_and_slices():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("SortedSearch", "sorted_search", "check_sorted_search", "range_join", "SORTED_SEARCH_FANOUT",
                 "SORTED_SEARCH_TOP"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.sorted_search(t, t), lambda: ops.range_join(t, t, t),
                 lambda: ops.check_sorted_search(t, t, t, t, t), lambda: ops.sorted_search(t.float(), t)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError):
        ops.sorted_search(t, None, None)
    for bad in (dict(m=-1, n=1), dict(m=1, n=-1), dict(m=(1 << 31) + 1, n=1), dict(m=1, n=1 << 32), dict(m=1, n=1, top=96)):
        with pytest.raises(ValueError):
            ops.SortedSearch(device="cpu", **bad)
    plan = ops.SortedSearch(16, 16, device="cpu", top=64)  # the plan itself is plain memory
    assert plan.ws_bytes == 256
    with pytest.raises(ValueError, match="index"):
        plan.search(t)
    with pytest.raises(ValueError, match="on the GPU"):
        plan.index(t)
    doc = ops.range_join.__doc__
    assert "unique" in doc and "stable" in doc


def test_code_object_has_no_scratch(tmp_path):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--save-temps", "-c", str(ROOT / "dwarf_bench_amd" / "csrc" / "sorted_search.hip"), "-o",
                    str(tmp_path / "ss.o")], check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "sorted_search-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    bodies = dict(re.findall(r"^(_ZN\S*ss_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M))
    assert len(bodies) == 6, sorted(bodies)  # header, fence, three searches, check
    meta = re.findall(r"\.name:\s+(_ZN\S*ss_\w+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 6 and all(size == "0" for _, size in meta), meta
    assert "scratch_" not in "".join(bodies.values())
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", asm)
    assert sorted(int(v) for v in lds) == [0, 0, 0, 65536, 65536, 65536]  # the top level: two workgroups a compute unit
