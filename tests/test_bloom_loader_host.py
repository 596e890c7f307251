"""dwarf_bench_amd/_dbench.py binds the Bloom filter's entry points (bloom_native, one of LATER_FAMILIES) on the one handle
of libdbench.so, with its table's types, beside the five families the loader started with; no name is shared."""
import importlib

from dwarf_bench_amd import _dbench, bloom_native
from tests.capi_testlib import ensure_built


def test_bloom_native_shares_the_one_handle_with_every_entry_point_bound():
    ensure_built()
    h = _dbench.lib()
    assert bloom_native.lib() is h and bloom_native.lib is _dbench.lib
    assert len(bloom_native.ENTRY_POINTS) == 4
    for name, (res, args) in bloom_native.ENTRY_POINTS.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_five_families_stay_and_share_no_name():
    assert _dbench.FAMILIES == ("select_native", "merge_native", "take_native", "dict_native", "bitpack_native")
    assert _dbench.LATER_FAMILIES == ("bloom_native",) and not set(_dbench.FAMILIES) & set(_dbench.LATER_FAMILIES)
    seen = {}
    for family in _dbench.FAMILIES:
        for name in importlib.import_module(f"dwarf_bench_amd.{family}").ENTRY_POINTS:
            seen[name] = family
    assert len(seen) == 17
    assert not set(seen) & set(bloom_native.ENTRY_POINTS)
    assert all(name.startswith("dbench_bloom_") for name in bloom_native.ENTRY_POINTS)
