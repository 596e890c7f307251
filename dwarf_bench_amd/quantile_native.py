"""ctypes binding of the quantile select's entry points (dwarf_bench_amd/host/quantile_select.{hpp,cpp} in libdbench.so): the
values at up to 16 ranks of a 32-bit column — absolute ranks or PERCENTILE_DISC fractions, resolved on the device against the
number of valid candidates — over all rows or through a row-id list with its device count, each with the number of candidates
below it and equal to it.  The kernels are HIP for gfx950 in quantile_select.cpp; the contract (the candidates, the ranks, the
answers, the workspace) is the header's comment.

The family is bound here, on the one handle of _dbench.lib(), on the first call of lib(): no second copy of the library is
loaded.  No fallback: a missing library or a missing symbol raises."""
from __future__ import annotations

import ctypes as C

from . import _dbench

# the #defines of quantile_select.hpp (tests/test_quantile_host.py holds them together)
MAX_RANKS = 16
SIGNED = 1

_vp, _sz, _int = C.c_void_p, C.c_size_t, C.c_int
ENTRY_POINTS = {
    "dbench_quantile_workspace_bytes": (_sz, [_int]),
    "dbench_quantile_select_u32": (_int, [_vp, _sz, _vp, _vp, _sz, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
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


def workspace_bytes(n_q: int) -> int:
    """0 for n_q outside 1 .. 16"""
    return int(lib().dbench_quantile_workspace_bytes(n_q))


def select(col, n_col: int, rows, count, capacity: int, q_num, q_den, flags: int, out_values, out_below, out_equal, workspace,
           workspace_bytes: int, stream, n_q: int | None = None) -> int:
    """dbench_quantile_select_u32 on raw addresses (None = NULL); q_num, q_den: sequences of uint32 (host values), or None for
    a NULL array.  n_q: what the call is told (default: len(q_num)).  -> its return code"""
    def words(q):
        return None if q is None else (C.c_uint32 * max(len(q), 1))(*[int(v) & 0xFFFFFFFF for v in q])
    if n_q is None:
        n_q = len(q_num) if q_num is not None else 0
    return int(lib().dbench_quantile_select_u32(col, n_col, rows, count, capacity, words(q_num), words(q_den), n_q, flags,
                                                out_values, out_below, out_equal, workspace, workspace_bytes, stream))
