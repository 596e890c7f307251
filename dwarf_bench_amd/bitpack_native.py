"""ctypes binding of the bit-packed column entry points (dwarf_bench_amd/host/bitpack.{hpp,cpp} in libdbench.so): pack
a 32-bit column in `width` bits per row over a base, unpack it densely or through a row-id list, and the range filter on
the packed codes that returns row ids.  The kernels are HIP for gfx950 in bitpack.cpp; the contract (format, length, fill,
the "no row" id, workspace layout) is the header's comment.  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of bitpack.hpp (tests/test_bitpack_host.py holds the two together)
SEGMENT_ROWS = 4096
TILE_ROWS = 2048
SIGNED = 1
NEGATE = 2
OUTER = 4
NO_ROW = 0xFFFFFFFF  # the row id DBENCH_BITPACK_OUTER fills without raising

_vp, _sz, _int, _u32, _uint = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint
ENTRY_POINTS = {
    "dbench_bitpack_words": (_sz, [_sz, _uint]),
    "dbench_bitpack_workspace_bytes": (_sz, [_sz]),
    "dbench_bitpack_pack_u32": (_int, [_vp, _sz, _vp, _uint, _u32, _vp, _vp, _sz, _vp]),
    "dbench_bitpack_unpack_u32": (_int, [_vp, _sz, _uint, _u32, _vp, _vp, _sz, _int, _u32, _vp, _vp, _sz, _vp]),
    "dbench_bitpack_select_range_u32": (_int, [_vp, _sz, _uint, _u32, _vp, _vp, _sz, _u32, _u32, _int, _vp, _vp, _vp, _sz,
                                               _vp]),
}


def words(n_rows: int, width: int) -> int:
    """the uint32 words of a packed column; 0 for a width outside 1..32 or n_rows >= 2^32"""
    return int(lib().dbench_bitpack_words(n_rows, width & 0xFFFFFFFF))


def workspace_bytes(capacity: int) -> int:
    return int(lib().dbench_bitpack_workspace_bytes(capacity))


def pack(col, capacity: int, count, width: int, base: int, out_packed, workspace, workspace_bytes: int, stream) -> int:
    """dbench_bitpack_pack_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_bitpack_pack_u32(col, capacity, count, width & 0xFFFFFFFF, base & 0xFFFFFFFF, out_packed,
                                             workspace, workspace_bytes, stream))


def unpack(packed, n_rows: int, width: int, base: int, rows, count, capacity: int, flags: int, fill: int, out, workspace,
           workspace_bytes: int, stream) -> int:
    """dbench_bitpack_unpack_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_bitpack_unpack_u32(packed, n_rows, width & 0xFFFFFFFF, base & 0xFFFFFFFF, rows, count, capacity,
                                               flags, fill & 0xFFFFFFFF, out, workspace, workspace_bytes, stream))


def select_range(packed, n_rows: int, width: int, base: int, in_rows, in_count, in_capacity: int, lo: int, hi: int,
                 flags: int, out_rows, out_count, workspace, workspace_bytes: int, stream) -> int:
    """dbench_bitpack_select_range_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_bitpack_select_range_u32(packed, n_rows, width & 0xFFFFFFFF, base & 0xFFFFFFFF, in_rows, in_count,
                                                     in_capacity, lo & 0xFFFFFFFF, hi & 0xFFFFFFFF, flags, out_rows,
                                                     out_count, workspace, workspace_bytes, stream))
