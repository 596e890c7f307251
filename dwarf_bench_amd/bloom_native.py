"""ctypes binding of the Bloom filter entry points (dwarf_bench_amd/host/bloom_filter.{hpp,cpp} in libdbench.so): build a
filter of 64-bit words from the 32-bit keys of a column, over all rows or through a row-id list, and probe a column against
it into a row-id list with its count on the device.  The kernels are HIP for gfx950 in bloom_filter.cpp; the contract (the
format, the sizing query, the flags, the workspace) is the header's comment.  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of bloom_filter.hpp (tests/test_bloom_host.py holds the two together)
ACCUMULATE = 1
NEGATE = 2

_vp, _sz, _int, _u32, _uint = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint
ENTRY_POINTS = {
    "dbench_bloom_words": (_sz, [_sz, _uint]),
    "dbench_bloom_workspace_bytes": (_sz, [_sz]),
    "dbench_bloom_build_u32": (_int, [_vp, _sz, _vp, _vp, _sz, _u32, _int, _vp, _sz, _vp, _sz, _vp]),
    "dbench_bloom_probe_u32": (_int, [_vp, _sz, _u32, _vp, _sz, _vp, _vp, _sz, _int, _vp, _vp, _vp, _sz, _vp]),
}


def words(n_keys: int, bits_per_key: int) -> int:
    """the uint64 words of a filter: max(1, ceil(n_keys * bits_per_key / 64)); 0 for bits_per_key outside 1..64 or a
    result of 2^32 or more"""
    return int(lib().dbench_bloom_words(n_keys, bits_per_key & 0xFFFFFFFF))


def workspace_bytes(candidates: int) -> int:
    return int(lib().dbench_bloom_workspace_bytes(candidates))


def build(col, n_col: int, rows, count, capacity: int, seed: int, flags: int, filter, n_words: int, workspace,
          workspace_bytes: int, stream) -> int:
    """dbench_bloom_build_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_bloom_build_u32(col, n_col, rows, count, capacity, seed & 0xFFFFFFFF, flags, filter, n_words,
                                            workspace, workspace_bytes, stream))


def probe(filter, n_words: int, seed: int, col, n_col: int, in_rows, in_count, in_capacity: int, flags: int, out_rows,
          out_count, workspace, workspace_bytes: int, stream) -> int:
    """dbench_bloom_probe_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_bloom_probe_u32(filter, n_words, seed & 0xFFFFFFFF, col, n_col, in_rows, in_count, in_capacity,
                                            flags, out_rows, out_count, workspace, workspace_bytes, stream))
