"""The dictionary-encoding entry points (dwarf_bench_amd/host/dict_encode.hpp, in libdbench.so) without a GPU: the
exported symbols, the header's constants against the binding's and the model's, the workspace query's properties, the
host-side argument checks (all before any HIP call, argument errors before workspace errors) and the tensor API's
refusals.  Every call below fails on the host: the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import _capi
from dwarf_bench_amd import dict_native as dn
from tests import dict_model as dm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HOST = ROOT / "dwarf_bench_amd" / "host"
FAKE = 1 << 30  # 256-byte aligned
N, CAP = 100002, 50000
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
COL, INNER, COUNT, KEYS, OUT_COUNT, CODES, MISSES, CARD_A, CARD_B, WS = (FAKE + i * STEP for i in range(10))


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return dn.lib()


def test_libdbench_exports_exactly_the_four_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_dict\w*)$", out, flags=re.M))
    assert names == sorted(dn.ENTRY_POINTS) == ["dbench_dict_build_u32", "dbench_dict_combine_u32", "dbench_dict_encode_u32",
                                                "dbench_dict_workspace_bytes"]
    assert not re.findall(r"\bdbhip_dict\w*$", out, flags=re.M)  # the dbhip_* surface is include/'s


def test_header_constants_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", (HOST / "dict_encode.hpp").read_text(), flags=re.S)
    got = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"^#define (DBENCH_DICT_\w+) (\w+)", text, flags=re.M)}
    assert got == {"DBENCH_DICT_SIGNED": dn.SIGNED, "DBENCH_DICT_MISS": dn.MISS, "DBENCH_DICT_LDS_SLOTS": dn.LDS_SLOTS}
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(dn.ENTRY_POINTS)
    assert (dn.SIGNED, dn.MISS, dn.LDS_SLOTS) == (1, 0xFFFFFFFF, 8192) and (dm.SIGNED, dm.MISS) == (dn.SIGNED, dn.MISS)
    from dwarf_bench_amd import take_native as tn
    assert dn.MISS == tn.NO_ROW  # decode is take with OUTER
    layout = (HOST / "dict_layout.hpp").read_text()
    assert '#include "dict_encode.hpp"' in layout and "0x85ebca6bu" in layout and "0xc2b2ae35u" in layout
    assert dn.LDS_SLOTS * 8 == 64 * 1024  # the LDS body's table: 64 KiB of the compute unit's 160


def test_workspace_query_properties(lib):
    sort_bytes = _capi.lib().dbhip_radix_sort_workspace_bytes
    last = 0
    caps = sorted(set(range(1, 300)) | {c for c in SIZES if 1 <= c < 1 << 31} |
                  {4095, 4096, 4097, (1 << 20) - 1, (1 << 20) + 1, (1 << 30) + 1, (1 << 31) - 2, (1 << 31) - 1})
    for c in caps:
        got = dn.workspace_bytes(c)
        assert got % 256 == 0 and got >= last, (c, got, last)
        up = lambda x: -(-x // 256) * 256  # noqa: E731
        assert got == 256 + up(8 * dn.slots(c)) + 2 * up(4 * c) + up(sort_bytes(c, 8)), c  # the header's regions
        last = got
    assert dn.workspace_bytes(1) == 256 + 256 + 2 * 256 + -(-sort_bytes(1, 8) // 256) * 256
    for c in (0, 1 << 31, (1 << 31) + 1, 1 << 32, 1 << 40):  # no legal call
        assert dn.workspace_bytes(c) == 0, c


def _build(col=COL, n=N, count=None, cap=CAP, flags=0, keys=KEYS, out_count=OUT_COUNT, w=WS, wb=None):
    if wb is None:
        wb = dn.workspace_bytes(cap) or 1 << 40
    return dn.build(col, n, count, cap, flags, keys, out_count, w, wb, None)


def _encode(col=COL, n=N, count=None, codes=CODES, misses=None, w=WS, wb=None):
    if wb is None:
        wb = dn.workspace_bytes(CAP)
    return dn.encode(col, n, count, codes, misses, w, wb, None)


def _combine(outer=COL, inner=INNER, n=N, count=None, oc=CARD_A, ic=CARD_B, out=CODES, w=WS, wb=256):
    return dn.combine(outer, inner, n, count, oc, ic, out, w, wb, None)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for kw in ({}, dict(flags=dn.SIGNED), dict(count=COUNT), dict(n=0, col=None), dict(n=0), dict(cap=1),
               dict(cap=(1 << 31) - 1, keys=1 << 40), dict(n=(1 << 32) - 1, cap=1, col=1 << 41)):  # (far from the others)
        assert _build(wb=0, **kw) == EWORKSPACE, kw
    for kw in ({}, dict(count=COUNT), dict(misses=MISSES), dict(count=COUNT, misses=MISSES), dict(n=0, col=None, codes=None),
               dict(n=0, misses=MISSES)):
        assert _encode(wb=0, **kw) == EWORKSPACE, kw
    for kw in ({}, dict(count=COUNT), dict(out=COL), dict(n=0, outer=None, inner=None, out=None), dict(oc=CARD_A, ic=CARD_A)):
        assert _combine(wb=0, **kw) == EWORKSPACE, kw


def test_every_argument_error_of_build_one_at_a_time(lib):
    for flags in (2, 4, 3, -1, 1 << 16):
        assert _build(flags=flags) == EINVAL, flags
    for cap in (0, 1 << 31, (1 << 31) + 1, 1 << 32, 1 << 40):
        assert _build(cap=cap) == EINVAL, cap
    for n in (1 << 32, (1 << 32) + 5, 1 << 40):
        assert _build(n=n) == EINVAL, n
    assert _build(col=None) == EINVAL and _build(keys=None) == EINVAL and _build(out_count=None) == EINVAL
    assert _build(n=0, col=None, keys=None) == EINVAL and _build(n=0, col=None, out_count=None) == EINVAL
    for off in (1, 2, 3):
        assert _build(col=COL + off) == EINVAL and _build(keys=KEYS + off) == EINVAL, off
    for off in (1, 2, 4, 12):
        assert _build(count=COUNT + off) == EINVAL and _build(out_count=OUT_COUNT + off) == EINVAL, off


def test_every_argument_error_of_encode_and_combine_one_at_a_time(lib):
    for n in (1 << 32, (1 << 32) + 5, 1 << 40):
        assert _encode(n=n) == EINVAL and _combine(n=n) == EINVAL, n
    assert _encode(col=None) == EINVAL and _encode(codes=None) == EINVAL
    assert _combine(outer=None) == EINVAL and _combine(inner=None) == EINVAL and _combine(out=None) == EINVAL
    assert _combine(oc=None) == EINVAL and _combine(ic=None) == EINVAL and _combine(n=0, oc=None) == EINVAL
    for off in (1, 2, 3):
        assert _encode(col=COL + off) == EINVAL and _encode(codes=CODES + off) == EINVAL, off
        assert _combine(outer=COL + off) == EINVAL and _combine(inner=INNER + off) == EINVAL and _combine(out=CODES + off) == EINVAL
    for off in (1, 2, 4, 12):
        assert _encode(count=COUNT + off) == EINVAL and _encode(misses=MISSES + off) == EINVAL, off
        assert _combine(count=COUNT + off) == EINVAL and _combine(oc=CARD_A + off) == EINVAL and _combine(ic=CARD_B + off) == EINVAL


def test_outputs_may_not_overlap_inputs_or_each_other(lib):
    # build: the keys against the column and the count, the count word against all three
    for where in (COL, COL + 4 * (N - 1), COL - 4 * (CAP - 1)):
        assert _build(keys=where) == EINVAL, where
    assert _build(keys=COL + 4 * N, wb=0) == EWORKSPACE and _build(keys=COL - 4 * CAP, wb=0) == EWORKSPACE  # touching ranges
    assert _build(keys=COUNT, count=COUNT) == EINVAL and _build(keys=COUNT - 4 * (CAP - 1), count=COUNT) == EINVAL
    assert _build(keys=COUNT, wb=0) == EWORKSPACE  # (no count given)
    for where in (COL, COL + 4 * N - 8, KEYS, KEYS + 4 * CAP - 8):
        assert _build(out_count=where) == EINVAL, where
    assert _build(out_count=COUNT, count=COUNT) == EINVAL and _build(out_count=COUNT + 8, count=COUNT, wb=0) == EWORKSPACE
    assert _build(out_count=KEYS + 4 * CAP, wb=0) == EWORKSPACE
    # encode: the codes against the column, the count and the miss word
    for where in (COL, COL + 4 * (N - 1), COL - 4 * (N - 1)):
        assert _encode(codes=where) == EINVAL, where
    assert _encode(codes=COL + 4 * N, wb=0) == EWORKSPACE
    assert _encode(codes=COUNT, count=COUNT) == EINVAL and _encode(codes=MISSES - 4 * (N - 1), misses=MISSES) == EINVAL
    assert _encode(misses=COL) == EINVAL and _encode(misses=COUNT, count=COUNT) == EINVAL
    assert _encode(misses=COL + 4 * N, wb=0) == EWORKSPACE
    # combine: out may be outer itself, nothing else
    assert _combine(out=COL, wb=0) == EWORKSPACE
    for where in (COL + 4, COL - 4, COL + 4 * (N - 1), INNER, INNER + 4 * (N - 1), INNER - 4 * (N - 1)):
        assert _combine(out=where) == EINVAL, where
    assert _combine(out=COL + 4 * N, wb=0) == EWORKSPACE and _combine(out=INNER - 4 * N, wb=0) == EWORKSPACE
    for word in ("count", "oc", "ic"):
        assert _combine(out=COUNT, **{word: COUNT}) == EINVAL and _combine(out=COUNT - 4 * (N - 1), **{word: COUNT}) == EINVAL, word


def test_workspace_errors_come_after_argument_errors(lib):
    full = dn.workspace_bytes(CAP)
    assert full > dn.workspace_bytes(1) >= 1024
    assert _build(wb=full - 1) == EWORKSPACE and _build(wb=0) == EWORKSPACE and _build(w=None) == EWORKSPACE
    assert _build(w=WS + 64) == EWORKSPACE and _build(w=WS + 128) == EWORKSPACE
    assert _build(cap=4 * CAP, wb=full) == EWORKSPACE  # a workspace sized for a smaller capacity
    assert _build(flags=2, wb=0) == EINVAL and _build(cap=0, wb=0) == EINVAL and _build(col=COL + 2, w=None) == EINVAL
    assert _build(keys=COL, w=WS + 64) == EINVAL
    # encode is not told the capacity: it asks for the bytes of capacity 1
    least = dn.workspace_bytes(1)
    assert _encode(wb=least - 1) == EWORKSPACE and _encode(wb=0) == EWORKSPACE and _encode(w=None) == EWORKSPACE
    assert _encode(w=WS + 64) == EWORKSPACE and _encode(n=1 << 32, wb=0) == EINVAL and _encode(codes=COL, w=None) == EINVAL
    # combine: 256 bytes of its own
    assert _combine(wb=255) == EWORKSPACE and _combine(w=None) == EWORKSPACE and _combine(w=WS + 128) == EWORKSPACE
    assert _combine(oc=None, wb=0) == EINVAL and _combine(out=INNER, w=None) == EINVAL


def test_ops_refuses_wrong_arguments_before_any_device_call():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("Dictionary", "factorize", "encode_columns", "groupby_columns", "join_pairs_columns"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.factorize(t), lambda: ops.factorize(t.float()), lambda: ops.encode_columns([t, t]),
                 lambda: ops.groupby_columns([t, t], t), lambda: ops.join_pairs_columns([t, t], [t, t])):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError, match="two or more"):
        ops.encode_columns([t])
    with pytest.raises(ValueError, match="8 rows"):
        ops.encode_columns([t, t[:8]])
    with pytest.raises(ValueError, match="columns"):
        ops.join_pairs_columns([t, t], [t])
    plan = ops.Dictionary(16, device="cpu")  # the plan itself is plain memory; capacity 0 means n
    assert plan.capacity == 16 and plan.ws_bytes == dn.workspace_bytes(16) and plan.keys.numel() == 16
    assert ops.Dictionary(1000, 10, device="cpu").ws_bytes == dn.workspace_bytes(10)
    assert ops.Dictionary(0, device="cpu").capacity == 1  # an empty column still has a dictionary
    for call in (plan.result, plan.count, lambda: plan.encode(t), lambda: plan.decode(t)):
        with pytest.raises(ValueError, match="nothing was built"):
            call()
    with pytest.raises(ValueError, match="on the GPU"):
        plan.build(t)
    for cap in (1 << 31, 1 << 40):
        with pytest.raises(ValueError):
            ops.Dictionary(16, cap, device="cpu")
    assert "dict_encode.hpp" in ops.__doc__
    assert (ops.DICT_MISS, ops.DICT_LDS_SLOTS) == (dn.MISS, dn.LDS_SLOTS)
