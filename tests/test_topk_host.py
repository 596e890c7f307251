"""The top-k (include/dbhip_topk.h) without a GPU: the second header declared, bound and exported, the workspace query
against the bound the header states, the host-side argument checks (all before any HIP call), the tensor API's refusals,
the dwarf lists of the seven CLIs, and the capture test of every entry point that works on a stream."""
import re
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi
from tests.test_join_pairs_host import DEFAULT, OTHER_CLIS

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "dwarf_bench_amd" / "_lib"
EINVAL, EWORKSPACE, OK = -1, -2, 0
SIZES = (0, 1, 1023, 1024, 1025, 4096, 100003, 1 << 20, (1 << 22) + 1, 1 << 24, (1 << 24) + 5, 1 << 30, (1 << 32) - 1)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(dbhip_[a-z0-9_]+)\s*\(", text)))


def test_entry_points_are_declared_bound_and_exported():
    names = _declared("dbhip_topk.h")
    assert names == ["dbhip_check_topk_u32", "dbhip_topk_i32", "dbhip_topk_u32", "dbhip_topk_workspace_bytes"]
    assert names == sorted(_capi.TOPK_SIGNATURES)
    lib = _capi.lib()
    for name in names:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _capi.TOPK_SIGNATURES[name][1] and fn.restype == _capi.TOPK_SIGNATURES[name][0], name


def test_the_first_header_and_its_table_are_what_they_were():
    assert _declared("dbhip.h") == sorted(_capi.SIGNATURES)
    assert not set(_capi.SIGNATURES) & set(_capi.TOPK_SIGNATURES)
    assert not any("topk" in name for name in _capi.SIGNATURES)


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
    header = (ROOT / "include" / "dbhip_topk.h").read_text()
    assert f"#define DBHIP_TOPK_CHUNK_ROWS {ops.TOPK_CHUNK_ROWS} " in header
    assert f"#define DBHIP_TOPK_SEGMENT_ROWS {ops.TOPK_SEGMENT_ROWS} " in header
    assert ops.TOPK_CHUNK_ROWS % 8192 == 0 and ops.TOPK_CHUNK_ROWS % ops.TOPK_SEGMENT_ROWS == 0
    t = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.topk(t, 3)  # not on the GPU
    with pytest.raises(ValueError):
        ops.check_topk(t, t[:3], t[:3])
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what TopK.launch asks of its column: a t[1:] slice starts 4 bytes off


def _names(exe):
    r = subprocess.run([str(exe), "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    return [l.strip() for l in r.stdout.splitlines() if l.startswith("\t")]


ALL_OTHER_CLIS = {**OTHER_CLIS, "dwarf_bench_join_pairs": sorted(DEFAULT + ["JoinPairsHip"])}


def _built():
    if not all((LIB / exe).exists() for exe in list(ALL_OTHER_CLIS) + ["dwarf_bench_topk"]):
        from dwarf_bench_amd import build
        build.build_hip()
        build.build_host()


def test_topk_cli_lists_the_default_set_plus_its_dwarf():
    _built()
    assert _names(LIB / "dwarf_bench_topk") == sorted(DEFAULT + ["TopKHip"])


@pytest.mark.parametrize("exe", sorted(ALL_OTHER_CLIS))
def test_the_other_clis_list_what_they_listed_before(exe):
    _built()
    assert _names(LIB / exe) == ALL_OTHER_CLIS[exe]


def test_every_stream_working_entry_point_has_a_capture_test():
    """what a COVERAGE row in tests/graph_testlib.py says for the entry points of dbhip.h"""
    pytest.importorskip("torch")
    from tests import graph_testlib as gl
    from tests import test_gpu_topk_graph as tg
    assert sorted(tg.COVERAGE) == _declared("dbhip_topk.h")
    assert [name for name, test in tg.COVERAGE.items() if test == gl.NO_STREAM_WORK] == ["dbhip_topk_workspace_bytes"]
    source = (ROOT / "tests" / "test_gpu_topk_graph.py").read_text()
    for name, test in tg.COVERAGE.items():
        if test == gl.NO_STREAM_WORK:
            continue
        assert callable(getattr(tg, test, None)) and test.startswith("test_"), (name, test)
        body = source.split(f"def {test}(")[1].split("\ndef ")[0]
        assert "capture" in body or "run_family" in body, (name, test)
