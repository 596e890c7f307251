"""The public C surface without a GPU, one check per fact and one case per header of dwarf_bench_amd/_capi.HEADERS: the
header, its table of ctypes signatures and the symbols libdbhip.so exports name the same entry points with the same
types; the tables share no name; include/ holds exactly those headers; the constants of dwarf_bench_amd/ops are the
headers' #defines; and every entry point is captured into a hipGraph by a test that exists, or is excused.  Adding a
header means adding its row to COUNTS, NAMES, FAMILY_WORDS and GRAPH_TESTS here (INTEGRATION.md has the checklist)."""
import ctypes as C
import importlib
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi, build
from tests import capi_testlib as ct

HEADERS = list(_capi.HEADERS)
COUNTS = {"dbhip.h": 73, "dbhip_topk.h": 4, "dbhip_reduce_by_key.h": 4, "dbhip_scan_by_key.h": 4, "dbhip_sorted_search.h": 5}
# names a header must declare: all of them for the four family headers, and for dbhip.h the entry points of the general
# group-by, the key-value sort and the join's pair table
NAMES = {
    "dbhip.h": ["dbhip_groupby_hash_workspace_bytes", "dbhip_groupby_hash_u32", "dbhip_check_distinct_workspace_bytes",
                "dbhip_check_distinct_u32", "dbhip_radix_sort_pairs_workspace_bytes", "dbhip_radix_sort_pairs_u32",
                "dbhip_radix_sort_pairs_i32", "dbhip_check_sorted_pairs_u32", "dbhip_join_pairs_workspace_bytes",
                "dbhip_join_pairs_u32", "dbhip_check_join_pairs_u32"],
    "dbhip_topk.h": ["dbhip_check_topk_u32", "dbhip_topk_i32", "dbhip_topk_u32", "dbhip_topk_workspace_bytes"],
    "dbhip_reduce_by_key.h": ["dbhip_check_reduce_by_key_u32", "dbhip_check_reduce_by_key_workspace_bytes",
                              "dbhip_reduce_by_key_u32", "dbhip_reduce_by_key_workspace_bytes"],
    "dbhip_scan_by_key.h": ["dbhip_check_scan_by_key_u32", "dbhip_check_scan_by_key_workspace_bytes", "dbhip_scan_by_key_u32",
                            "dbhip_scan_by_key_workspace_bytes"],
    "dbhip_sorted_search.h": ["dbhip_check_sorted_search_u32", "dbhip_check_sorted_search_workspace_bytes",
                              "dbhip_sorted_index_build_u32", "dbhip_sorted_index_workspace_bytes", "dbhip_sorted_search_u32"],
}
# the words that mark a family header's names: each of its names holds one, no name of another header does
FAMILY_WORDS = {"dbhip_topk.h": ("topk",), "dbhip_reduce_by_key.h": ("reduce_by_key",), "dbhip_scan_by_key.h": ("scan_by_key",),
                "dbhip_sorted_search.h": ("sorted_search", "sorted_index")}
# the module whose COVERAGE table says which test captures which entry point of the header
GRAPH_TESTS = {"dbhip.h": "graph_testlib", "dbhip_topk.h": "test_gpu_topk_graph",
               "dbhip_reduce_by_key.h": "test_gpu_reduce_by_key_graph", "dbhip_scan_by_key.h": "test_gpu_scan_by_key_graph",
               "dbhip_sorted_search.h": "test_gpu_sorted_search_graph"}
# entry points of dbhip.h that go uncaptured besides the queries: the status read-back and the calibration call too
EXCUSED = {"dbhip.h": ["dbhip_version", "dbhip_device_info", "dbhip_radix_sort_rank_mode", "dbhip_workspace_status",
                       "dbhip_radix_sort_prepare"]}


def test_the_headers_of_include_are_the_tables():
    on_disk = sorted(p.name for p in ct.INCLUDE.glob("*.h"))
    assert on_disk == sorted(_capi.HEADERS), "include/ and _capi.HEADERS name different headers"
    assert sorted(p.name for p in build.public_headers()) == on_disk, "build.public_headers() misses a header of include/"
    assert sorted(COUNTS) == sorted(NAMES) == sorted(GRAPH_TESTS) == on_disk
    assert sorted(FAMILY_WORDS) == sorted(h for h in on_disk if h != "dbhip.h")


def test_row_counts():
    assert {h: len(t) for h, t in _capi.HEADERS.items()} == COUNTS


def test_tables_are_pairwise_disjoint():
    for i, a in enumerate(HEADERS):
        for b in HEADERS[i + 1:]:
            shared = set(_capi.HEADERS[a]) & set(_capi.HEADERS[b])
            assert not shared, (a, b, sorted(shared))
    for header, words in FAMILY_WORDS.items():
        for other, table in _capi.HEADERS.items():
            for name in table:
                assert any(w in name for w in words) == (other == header), (header, other, name)


@pytest.mark.parametrize("header", HEADERS)
def test_header_and_table_name_the_same_entry_points(header):
    names = ct.declared(header)
    table = sorted(_capi.HEADERS[header])
    assert names == table, (header, sorted(set(names) ^ set(table)))
    assert set(NAMES[header]) <= set(names), (header, sorted(set(NAMES[header]) - set(names)))


def _exported():
    """the dbhip_* functions in libdbhip.so's dynamic symbol table"""
    ct.ensure_built()
    nm = shutil.which("nm") or shutil.which("llvm-nm", path=str(Path(build._hipcc()).resolve().parents[1] / "llvm" / "bin"))
    assert nm, "neither nm nor llvm-nm found"
    out = subprocess.run([nm, "-D", "--defined-only", str(_capi.lib_path())], capture_output=True, text=True, check=True).stdout
    return sorted(re.findall(r"^\S+ T (dbhip_[a-z0-9_]+)$", out, flags=re.M))


def test_library_exports_the_declared_symbols_and_no_other():
    want = sorted(name for header in HEADERS for name in ct.declared(header))
    got = _exported()
    assert got == want, sorted(set(got) ^ set(want))
    assert _capi.lib().dbhip_version() == ct.defines("dbhip.h")["DBHIP_VERSION"] == 1


def _is_pointer(argtype):
    return argtype in (C.c_void_p, C.c_char_p) or issubclass(argtype, C._Pointer)


@pytest.mark.parametrize("header", HEADERS)
def test_bound_types_are_the_tables_and_the_headers(header):
    """what lib() bound is the table's row, and the row is the header's prototype: the same scalar type for every scalar,
    a pointer type for every pointer (dbhip_stream_t is one)"""
    lib = _capi.lib()
    protos = ct.prototypes(header)
    assert sorted(protos) == ct.declared(header), header  # the prototype reader sees every declaration
    for name, (res, args) in _capi.HEADERS[header].items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, (header, name)
        want_res, want_args = protos[name]
        assert res == want_res, (header, name, "restype", res, want_res)
        assert len(args) == len(want_args), (header, name, len(args), len(want_args))
        for i, (got, want) in enumerate(zip(args, want_args)):
            assert _is_pointer(got) if want == ct.POINTER else got == want, (header, name, f"argument {i}", got, want)


def _ops_relations(header, ops):
    if header == "dbhip_topk.h":
        return ops.TOPK_CHUNK_ROWS % 8192 == 0 and ops.TOPK_CHUNK_ROWS % ops.TOPK_SEGMENT_ROWS == 0
    if header == "dbhip_reduce_by_key.h":
        return ops.REDUCE_BY_KEY_CHUNK_ROWS == 8 * ops.REDUCE_BY_KEY_SEGMENT_ROWS
    if header == "dbhip_scan_by_key.h":
        return ops.SCAN_BY_KEY_CHUNK_ROWS == 8 * ops.SCAN_BY_KEY_SEGMENT_ROWS
    if header == "dbhip_sorted_search.h":
        from tests import sorted_search_model as sm
        return (ops.SORTED_SEARCH_FANOUT, ops.SORTED_SEARCH_TOP) == (sm.FANOUT, sm.TOP)
    raise AssertionError(f"no relation for {header}")


@pytest.mark.parametrize("header", HEADERS)
def test_python_constants_are_the_headers_defines(header):
    values = ct.defines(header)
    if header == "dbhip.h":  # the error codes the host tests and the bindings' messages use
        codes = {name: values[name] for name in ("DBHIP_OK", "DBHIP_EINVAL", "DBHIP_EWORKSPACE", "DBHIP_ENODEVICE")}
        assert list(codes.values()) == [ct.OK, ct.EINVAL, ct.EWORKSPACE, ct.ENODEVICE]
        assert _capi._ERR == {v: k for k, v in codes.items() if v != 0}
        return
    pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    assert len(values) == 2, (header, values)  # every family header has two tuning constants today
    for name, value in values.items():
        assert getattr(ops, name[len("DBHIP_"):]) == value, (header, name)
    assert _ops_relations(header, ops), header


def _coverage(header):
    """name -> None for an excused entry point, else (test file, test function); both row formats: graph_testlib's
    (file, test) pairs and one-line reasons, and the family files' test names of their own file and NO_STREAM_WORK"""
    from tests import graph_testlib as gl
    module = importlib.import_module(f"tests.{GRAPH_TESTS[header]}")
    rows = {}
    for name, where in module.COVERAGE.items():
        if header == "dbhip.h" and isinstance(where, str):
            assert where.strip() and "\n" not in where, name  # a one-line reason
            rows[name] = None
        elif header == "dbhip.h":
            rows[name] = tuple(where)
        elif where == gl.NO_STREAM_WORK:
            rows[name] = None
        else:
            assert callable(getattr(module, where, None)), (header, name, where)
            rows[name] = (f"tests/{GRAPH_TESTS[header]}.py", where)
    return rows


@pytest.mark.parametrize("header", HEADERS)
def test_every_entry_point_is_captured_or_excused(header):
    """found by reading the test files; only queries (and what EXCUSED names) go uncaptured"""
    pytest.importorskip("torch")
    rows = _coverage(header)
    names = ct.declared(header)
    assert sorted(rows) == names, (header, sorted(set(rows) ^ set(names)))
    excused = sorted(name for name, where in rows.items() if where is None)
    assert excused == sorted([n for n in names if n.endswith("_workspace_bytes")] + EXCUSED.get(header, [])), header
    sources = {}
    for name, where in rows.items():
        if where is None:
            continue
        path, test = where
        if path not in sources:
            assert (ct.ROOT / path).is_file(), (header, name, path)
            sources[path] = (ct.ROOT / path).read_text()
        assert test.startswith("test_"), (header, name, test)
        assert re.search(rf"^def {re.escape(test)}\(", sources[path], flags=re.M), (header, name, path, test)
        if header == "dbhip.h":
            assert "graph_testlib" in sources[path] or "torch.cuda.graph" in sources[path], (name, path)
        body = sources[path].split(f"\ndef {test}(")[1].split("\ndef ")[0]
        assert "capture" in body or "run_family" in body, (header, name, test)
