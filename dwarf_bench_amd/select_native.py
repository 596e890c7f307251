"""ctypes binding of the selection-vector entry points (dwarf_bench_amd/host/select_rows.{hpp,cpp} in libdbench.so):
row ids under a range predicate on a 32-bit column, over all rows or over a row-id list.  The kernels are HIP for
gfx950 in select_rows.cpp; the contract (candidates, predicate, workspace layout) is the header's comment.
No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of select_rows.hpp (tests/test_select_host.py holds the two together)
SEGMENT_ROWS = 4096
SIGNED = 1
NEGATE = 2

_vp, _sz, _u32, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
ENTRY_POINTS = {
    "dbench_select_workspace_bytes": (_sz, [_sz]),
    "dbench_select_range_u32": (_int, [_vp, _sz, _vp, _vp, _sz, _u32, _u32, _int, _vp, _vp, _vp, _sz, _vp]),
}


def workspace_bytes(candidates: int) -> int:
    return int(lib().dbench_select_workspace_bytes(candidates))


def select_range(col: int, n_col: int, in_rows: int | None, in_count: int | None, in_capacity: int, lo: int, hi: int,
                 flags: int, out_rows: int | None, out_count: int | None, workspace: int | None, workspace_bytes: int,
                 stream: int | None) -> int:
    """dbench_select_range_u32 on raw addresses; lo and hi are 32-bit patterns.  -> its return code"""
    return int(lib().dbench_select_range_u32(col, n_col, in_rows, in_count, in_capacity, lo & 0xFFFFFFFF,
                                             hi & 0xFFFFFFFF, flags, out_rows, out_count, workspace, workspace_bytes,
                                             stream))
