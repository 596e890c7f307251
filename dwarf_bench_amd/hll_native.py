"""ctypes binding of the HyperLogLog entry points (dwarf_bench_amd/host/hll_sketch.{hpp,cpp} in libdbench.so): build a sketch
of 2^p one-byte registers from the rows of 1 .. 4 32-bit columns, over all rows or through a row-id list, merge two sketches,
and estimate the number of distinct rows on the host from the 256-byte histogram every build and merge writes.  The kernels
are HIP for gfx950 in hll_sketch.cpp; the contract (the format, the flag, the workspace) is the header's comment.

The family is bound here, on the one handle of _dbench.lib(), on the first call of lib(): no second copy of the library is
loaded.  No fallback: a missing library or a missing symbol raises."""
from __future__ import annotations

import ctypes as C

from . import _dbench

# the #defines of hll_sketch.hpp and hll_layout.hpp (tests/test_hll_host.py holds them together)
ACCUMULATE = 1
MAX_GRID = 512
MIN_P, MAX_P, MAX_COLS, HIST_WORDS = 4, 14, 4, 64

_vp, _sz, _int, _u32, _uint, _dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint, C.c_double
ENTRY_POINTS = {
    "dbench_hll_workspace_bytes": (_sz, [_uint]),
    "dbench_hll_build_u32": (_int, [_vp, _int, _sz, _vp, _vp, _sz, _u32, _int, _uint, _vp, _vp, _vp, _sz, _vp]),
    "dbench_hll_merge": (_int, [_vp, _vp, _uint, _vp, _vp, _sz, _vp]),
    "dbench_hll_estimate": (_dbl, [_vp, _uint]),
}
_bound = None


def lib() -> C.CDLL:
    """_dbench.lib(), with this family's entry points bound on it"""
    global _bound
    h = _dbench.lib()
    if _bound is not h:
        for name, (res, args) in ENTRY_POINTS.items():
            fn = getattr(h, name)  # AttributeError if the .so does not export the symbol
            fn.restype = res
            fn.argtypes = args
        _bound = h
    return h


def workspace_bytes(p: int) -> int:
    """0 for p outside 4 .. 14"""
    return int(lib().dbench_hll_workspace_bytes(p & 0xFFFFFFFF))


def build(cols, n_col: int, rows, count, capacity: int, seed: int, flags: int, p: int, registers, hist, workspace,
          workspace_bytes: int, stream, n_cols: int | None = None) -> int:
    """dbench_hll_build_u32 on raw addresses (None = NULL); cols: a sequence of up to four column addresses, or None for a
    NULL array.  n_cols: what the call is told (default: len(cols)).  -> its return code"""
    arr = None
    if cols is not None:
        arr = (C.c_void_p * MAX_COLS)(*(list(cols)[:MAX_COLS]))
        if n_cols is None:
            n_cols = len(cols)
    return int(lib().dbench_hll_build_u32(arr, n_cols or 0, n_col, rows, count, capacity, seed & 0xFFFFFFFF, flags,
                                          p & 0xFFFFFFFF, registers, hist, workspace, workspace_bytes, stream))


def merge(dst, src, p: int, hist, workspace, workspace_bytes: int, stream) -> int:
    """dbench_hll_merge on raw addresses (None = NULL).  -> its return code"""
    return int(lib().dbench_hll_merge(dst, src, p & 0xFFFFFFFF, hist, workspace, workspace_bytes, stream))


def estimate(hist, p: int) -> float:
    """dbench_hll_estimate on a host histogram: a sequence of 64 counts.  -1.0: invalid"""
    words = (C.c_uint32 * HIST_WORDS)(*[int(v) & 0xFFFFFFFF for v in hist])
    return float(lib().dbench_hll_estimate(words, p & 0xFFFFFFFF))
