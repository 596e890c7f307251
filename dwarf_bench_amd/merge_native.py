"""ctypes binding of the merge-path entry points (dwarf_bench_amd/host/merge_sorted.{hpp,cpp} in libdbench.so): the
stable merge of two sorted (key, value) columns, and union / intersection / difference of two strictly ascending
row-id lists.  The kernels are HIP for gfx950 in merge_sorted.cpp; the contract (sizes, tie order, value modes,
workspace layout) is the header's comment.  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of merge_sorted.hpp (tests/test_merge_host.py holds the two together)
TILE_ROWS = 2048
SIGNED = 1
ROW_IDS = 2
UNION, INTERSECT, DIFFERENCE = 0, 1, 2

_vp, _sz, _int = C.c_void_p, C.c_size_t, C.c_int
ENTRY_POINTS = {
    "dbench_merge_workspace_bytes": (_sz, [_sz, _sz]),
    "dbench_merge_u32": (_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dbench_setop_u32": (_int, [_int, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
}


def workspace_bytes(a_capacity: int, b_capacity: int) -> int:
    return int(lib().dbench_merge_workspace_bytes(a_capacity, b_capacity))


def set_bound(op: int, a_capacity: int, b_capacity: int) -> int:
    """the entries `out` of dbench_setop_u32 has room for"""
    return {UNION: a_capacity + b_capacity, INTERSECT: min(a_capacity, b_capacity), DIFFERENCE: a_capacity}[op]


def merge(a_keys, a_vals, a_count, a_capacity: int, b_keys, b_vals, b_count, b_capacity: int, flags: int, out_keys,
          out_vals, out_count, workspace, workspace_bytes: int, stream) -> int:
    """dbench_merge_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_merge_u32(a_keys, a_vals, a_count, a_capacity, b_keys, b_vals, b_count, b_capacity, flags,
                                      out_keys, out_vals, out_count, workspace, workspace_bytes, stream))


def setop(op: int, a, a_count, a_capacity: int, b, b_count, b_capacity: int, out, out_count, workspace,
          workspace_bytes: int, stream) -> int:
    """dbench_setop_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_setop_u32(op, a, a_count, a_capacity, b, b_count, b_capacity, out, out_count, workspace,
                                      workspace_bytes, stream))
