"""ctypes binding of the late-materialisation entry points (dwarf_bench_amd/host/take_rows.{hpp,cpp} in libdbench.so):
take, the gather of up to four 32-bit columns through a row-id list, and aggregate, COUNT / 64-bit SUM / MIN / MAX of a
column over a row-id list or over all its rows.  The kernels are HIP for gfx950 in take_rows.cpp; the contract (length,
fill, the "no row" id, workspace layout) is the header's comment.  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of take_rows.hpp (tests/test_take_host.py holds the two together)
MAX_COLS = 4
SEGMENT_ROWS = 1024
OUTER = 1
SIGNED = 2
NO_ROW = 0xFFFFFFFF  # the row id DBENCH_TAKE_OUTER fills or skips without raising

_vp, _sz, _int, _u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
ENTRY_POINTS = {
    "dbench_take_workspace_bytes": (_sz, [_sz]),
    "dbench_take_u32": (_int, [_vp, _sz, _sz, _vp, _vp, _sz, _int, _u32, _vp, _vp, _sz, _vp]),
    "dbench_aggregate_rows_u32": (_int, [_vp, _sz, _vp, _vp, _sz, _int, _vp, _vp, _sz, _vp]),
}


def workspace_bytes(capacity: int) -> int:
    return int(lib().dbench_take_workspace_bytes(capacity))


def pointers(addresses):
    """a host array of device addresses (None = NULL) as dbench_take_u32 takes cols and outs; None: no array at all"""
    if addresses is None:
        return None
    return (C.c_void_p * len(addresses))(*addresses)


def take(cols, n_cols: int, n_rows: int, rows, count, capacity: int, flags: int, fill: int, outs, workspace,
         workspace_bytes: int, stream) -> int:
    """dbench_take_u32 on raw addresses (None = NULL); cols and outs: sequences of addresses.  -> its return code"""
    return int(lib().dbench_take_u32(pointers(cols), n_cols, n_rows, rows, count, capacity, flags, fill & 0xFFFFFFFF,
                                     pointers(outs), workspace, workspace_bytes, stream))


def aggregate(col, n_rows: int, rows, count, capacity: int, flags: int, out, workspace, workspace_bytes: int, stream) -> int:
    """dbench_aggregate_rows_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_aggregate_rows_u32(col, n_rows, rows, count, capacity, flags, out, workspace, workspace_bytes,
                                               stream))
