"""ctypes binding of the dictionary-encoding entry points (dwarf_bench_amd/host/dict_encode.{hpp,cpp} in libdbench.so):
build, the distinct values of a 32-bit column in order with a table value -> rank in the workspace; encode, a column's
rows replaced by the ranks of their values; combine, the codes of two columns folded into the code of the pair.  The
kernels are HIP for gfx950 in dict_encode.cpp; the contract (length, overflow, the miss code, workspace layout) is the
header's comment.  No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C

from ._dbench import lib  # noqa: F401  the one handle of libdbench.so, every family's ENTRY_POINTS bound

# the #defines of dict_encode.hpp (tests/test_dict_host.py holds the two together)
SIGNED = 1
MISS = 0xFFFFFFFF  # the code of a value the dictionary does not hold: take's "no row" id
LDS_SLOTS = 8192   # the largest table the encode kernel keeps in LDS

_vp, _sz, _int = C.c_void_p, C.c_size_t, C.c_int
ENTRY_POINTS = {
    "dbench_dict_workspace_bytes": (_sz, [_sz]),
    "dbench_dict_build_u32": (_int, [_vp, _sz, _vp, _sz, _int, _vp, _vp, _vp, _sz, _vp]),
    "dbench_dict_encode_u32": (_int, [_vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dbench_dict_combine_u32": (_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


def slots(capacity: int) -> int:
    """dict_slots of dict_layout.hpp: the smallest power of two >= 2 * capacity, at least 2"""
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


def workspace_bytes(capacity: int) -> int:
    return int(lib().dbench_dict_workspace_bytes(capacity))


def build(col, n: int, count, capacity: int, flags: int, out_keys, out_count, workspace, workspace_bytes: int, stream) -> int:
    """dbench_dict_build_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_dict_build_u32(col, n, count, capacity, flags, out_keys, out_count, workspace, workspace_bytes,
                                           stream))


def encode(col, n: int, count, out_codes, out_misses, workspace, workspace_bytes: int, stream) -> int:
    """dbench_dict_encode_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_dict_encode_u32(col, n, count, out_codes, out_misses, workspace, workspace_bytes, stream))


def combine(outer, inner, n: int, count, outer_card, inner_card, out, workspace, workspace_bytes: int, stream) -> int:
    """dbench_dict_combine_u32 on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_dict_combine_u32(outer, inner, n, count, outer_card, inner_card, out, workspace, workspace_bytes,
                                             stream))
