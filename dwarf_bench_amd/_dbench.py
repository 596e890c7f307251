"""The one loader of libdbench.so for the row-id operator bindings (select_native, merge_native, take_native,
dict_native, bitpack_native, and the later families: bloom_native): the library is loaded once per process and the entry
points of all families are bound on the one handle.  Each module keeps its table as ENTRY_POINTS and re-exports `lib`.
No fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import importlib
from pathlib import Path

from . import _capi

_LIB = Path(__file__).resolve().parent / "_lib" / "libdbench.so"
FAMILIES = ("select_native", "merge_native", "take_native", "dict_native", "bitpack_native")
LATER_FAMILIES = ("bloom_native",)  # families added behind the five, bound on the same handle in the same loop
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not _LIB.exists():
            raise _capi.DbhipError(f"{_LIB} is missing: run `python -m dwarf_bench_amd.build`")
        _capi.lib()  # libdbhip.so first (RTLD_GLOBAL), same HIP runtime as torch
        h = C.CDLL(str(_LIB), mode=C.RTLD_GLOBAL)
        for family in FAMILIES + LATER_FAMILIES:  # imported here, not at the top: the modules import this one
            for name, (res, args) in importlib.import_module(f"{__package__}.{family}").ENTRY_POINTS.items():
                fn = getattr(h, name)  # AttributeError if the .so does not export the symbol
                fn.restype = res
                fn.argtypes = args
        _lib = h
    return _lib
