"""The bit-packed column entry points (dwarf_bench_amd/host/bitpack.hpp, in libdbench.so) without a GPU: the exported
symbols, the header's constants against the binding's and the model's, the word count against the model, the workspace
query's properties, the host-side argument checks (all before any HIP call, argument errors before workspace errors) and
the tensor API's refusals.  Every call below fails on the host: the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import bitpack_native as bn
from tests import bitpack_model as bm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "bitpack.hpp"
FAKE = 1 << 30  # 256-byte aligned
N, CAP, WIDTH = 100002, 50000, 12
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
COL, PACKED, ROWS, COUNT, OUT, OUT_COUNT, WS = (FAKE + i * STEP for i in range(7))
ROW_COUNTS = (0, 1, 31, 32, 33, 127, 128, 129, 4097, (1 << 32) - 1)


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return bn.lib()


def test_libdbench_exports_exactly_the_bitpack_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_bitpack\w*)$", out, flags=re.M))
    assert names == sorted(bn.ENTRY_POINTS) and len(names) == 5
    assert all(n.startswith("dbench_bitpack_") for n in names)
    # the families of libdbench.so keep their names apart: nothing new under another family's prefix
    other = re.findall(r"\b(dbench_(?:select_|dict|take|aggregate|merge_|setop_)\w*)$", out, flags=re.M)
    assert not [n for n in other if "bitpack" in n] and not re.findall(r"\bdbhip_bitpack\w*$", out, flags=re.M)


def test_header_constants_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_BITPACK_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_BITPACK_SEGMENT_ROWS": bn.SEGMENT_ROWS, "DBENCH_BITPACK_TILE_ROWS": bn.TILE_ROWS,
                   "DBENCH_BITPACK_SIGNED": bn.SIGNED, "DBENCH_BITPACK_NEGATE": bn.NEGATE, "DBENCH_BITPACK_OUTER": bn.OUTER}
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(bn.ENTRY_POINTS)
    assert (bm.SIGNED, bm.NEGATE, bm.OUTER, bm.NO_ROW) == (bn.SIGNED, bn.NEGATE, bn.OUTER, bn.NO_ROW)
    assert (bm.SEGMENT_ROWS, bm.TILE_ROWS) == (bn.SEGMENT_ROWS, bn.TILE_ROWS)
    # the select flags mean what those of select_rows.hpp mean, and OUTER collides with neither
    from dwarf_bench_amd import select_native as sn
    assert (bn.SIGNED, bn.NEGATE) == (sn.SIGNED, sn.NEGATE) and bn.OUTER & (bn.SIGNED | bn.NEGATE) == 0
    assert bn.SEGMENT_ROWS % 128 == 0 and bn.TILE_ROWS % 128 == 0  # whole 16-byte chunks at every width
    from dwarf_bench_amd import ops
    assert bm.KEY_RANGE == ops.DEV_KEY_RANGE
    assert "DBENCH_DICT_MISS" in HEADER.read_text()  # what a missing code does to pack is said there


def test_words_equal_the_model(lib):
    for width in range(1, 33):
        for n in ROW_COUNTS:
            assert bn.words(n, width) == bm.words(n, width) and bn.words(n, width) % 4 == 0, (n, width)
        for n in (1 << 32, (1 << 32) + 1, 1 << 40):
            assert bn.words(n, width) == 0, (n, width)
    for width in (0, 33, 34, 64, 1 << 16, -1):
        for n in ROW_COUNTS:
            assert bn.words(n, width) == 0, (n, width)
    assert bn.words(1 << 26, 12) * 4 == 96 << 20


def test_workspace_query_keeps_its_properties(lib):
    assert "at most 1536 + capacity / 7" in HEADER.read_text()
    S = bn.SEGMENT_ROWS
    last = 0
    for c in sorted(SIZES + (3, S - 1, S, S + 1, 2 * S + 3, 64 * S - 1, 64 * S, 64 * S + 1)):
        got = bn.workspace_bytes(c)
        segments = -(-c // S)
        assert got % 256 == 0 and got >= last and 256 + 520 * segments <= got <= 1536 + c // 7, (c, got)
        last = got
    assert bn.workspace_bytes(0) == 256
    for c in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert bn.workspace_bytes(c) == 0, c
    from dwarf_bench_amd import select_native as sn
    for c in SIZES:  # a SelectRows plan's workspace serves both kinds of column
        assert bn.workspace_bytes(c) <= sn.workspace_bytes(c), c


def _pack(col=COL, cap=CAP, count=None, width=WIDTH, base=0, out=PACKED, w=WS, wb=None):
    return bn.pack(col, cap, count, width, base, out, w, 1 << 20 if wb is None else wb, None)


def _unpack(packed=PACKED, n=N, width=WIDTH, base=0, rows=ROWS, count=None, cap=CAP, flags=0, fill=0, out=OUT, w=WS, wb=None):
    return bn.unpack(packed, n, width, base, rows, count, cap, flags, fill, out, w, 1 << 20 if wb is None else wb, None)


def _select(packed=PACKED, n=N, width=WIDTH, base=0, rows=ROWS, count=None, cap=CAP, lo=1, hi=5, flags=0, out=OUT,
            out_count=OUT_COUNT, w=WS, wb=None):
    if wb is None:
        wb = bn.workspace_bytes(cap if rows else n) or 1 << 40
    return bn.select_range(packed, n, width, base, rows, count, cap, lo, hi, flags, out, out_count, w, wb, None)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for width in (1, 7, 12, 31, 32):
        for kw in ({}, dict(count=COUNT), dict(base=0xFFFFFFFF), dict(col=COL + 4), dict(col=COL + 12), dict(cap=0),
                   dict(cap=0, col=None, out=None)):
            assert _pack(width=width, wb=0, **kw) == EWORKSPACE, (width, kw)
        for kw in ({}, dict(flags=bn.OUTER), dict(count=COUNT), dict(fill=0xFFFFFFFF), dict(rows=None), dict(rows=None, cap=1 << 40),
                   dict(rows=ROWS + 4, out=OUT + 8), dict(n=0, packed=None), dict(cap=0), dict(rows=None, n=0, packed=None, out=None)):
            assert _unpack(width=width, wb=0, **kw) == EWORKSPACE, (width, kw)
        for kw in ({}, dict(flags=bn.SIGNED), dict(flags=bn.NEGATE), dict(flags=bn.SIGNED | bn.NEGATE), dict(count=COUNT),
                   dict(rows=None), dict(out=None), dict(lo=9, hi=3), dict(n=0, packed=None), dict(rows=ROWS + 4, out=OUT + 12)):
            assert _select(width=width, wb=0, **kw) == EWORKSPACE, (width, kw)


def test_every_argument_error_one_at_a_time(lib):
    for call in (_pack, _unpack, _select):
        for width in (0, 33, 34, 64, -1, 1 << 16):  # a width outside 1..32
            assert call(width=width) == EINVAL, (call.__name__, width)
        assert call(cap=1 << 32) == EINVAL and call(cap=1 << 40) == EINVAL  # a size of 2^32 or more
    for call in (_unpack, _select):
        assert call(n=1 << 32) == EINVAL and call(n=(1 << 32) + 5, cap=7) == EINVAL
        assert call(rows=None, count=COUNT) == EINVAL  # count without rows
        assert call(packed=None) == EINVAL  # a NULL column with rows to read
        for off in (4, 8, 12, 1, 2):  # the format demands a 16-byte aligned column
            assert call(packed=PACKED + off) == EINVAL, off
        for off in (1, 2, 3):
            assert call(rows=ROWS + off) == EINVAL and call(out=OUT + off) == EINVAL
        for off in (1, 2, 4, 12):
            assert call(count=COUNT + off) == EINVAL, off
    # unknown flag bits: pack has none, unpack knows OUTER, select SIGNED and NEGATE
    for flags in (bn.SIGNED, bn.NEGATE, bn.OUTER | bn.SIGNED, 8, 16, -1, 1 << 16):
        assert _unpack(flags=flags) == EINVAL, flags
    for flags in (bn.OUTER, bn.OUTER | bn.SIGNED, 8, 15, -1, 1 << 16):
        assert _select(flags=flags) == EINVAL, flags
    # pack
    assert _pack(col=None) == EINVAL and _pack(out=None) == EINVAL
    for off in (1, 2, 3):
        assert _pack(col=COL + off) == EINVAL
    for off in (4, 8, 12, 1):
        assert _pack(out=PACKED + off) == EINVAL, off
    for off in (1, 2, 4, 12):
        assert _pack(count=COUNT + off) == EINVAL
    # unpack and select: outputs
    assert _unpack(out=None) == EINVAL and _unpack(rows=None, out=None) == EINVAL
    assert _select(out_count=None) == EINVAL
    for off in (1, 2, 4, 12):
        assert _select(out_count=OUT_COUNT + off) == EINVAL


def test_outputs_may_not_overlap_inputs(lib):
    words = 4 * bn.words(CAP, WIDTH)  # bytes of the packed form of CAP rows
    for where in (COL, COL + 4 * CAP - 16, COL - words + 16):
        assert _pack(out=where) == EINVAL, where
    assert _pack(out=COL + (4 * CAP + 15) // 16 * 16, wb=0) == EWORKSPACE and _pack(out=COL - words, wb=0) == EWORKSPACE
    assert _pack(out=COUNT, count=COUNT) == EINVAL and _pack(out=COUNT, wb=0) == EWORKSPACE  # (no count given)
    packed_bytes = 4 * bn.words(N, WIDTH)
    for call in (_unpack, _select):
        for where in (PACKED, PACKED + packed_bytes - 4, PACKED - 4 * (CAP - 1), ROWS, ROWS + 4 * (CAP - 1), ROWS - 4 * (CAP - 1)):
            assert call(out=where) == EINVAL, (call.__name__, where)
        assert call(out=PACKED + packed_bytes, wb=0) == EWORKSPACE and call(out=ROWS + 4 * CAP, wb=0) == EWORKSPACE
    # dense: the output holds n rows
    assert _unpack(rows=None, out=PACKED - 4 * (N - 1)) == EINVAL and _unpack(rows=None, out=PACKED - 4 * N, wb=0) == EWORKSPACE
    assert _select(rows=None, out=PACKED - 4 * (N - 1)) == EINVAL and _select(rows=None, out=PACKED - 4 * N, wb=0) == EWORKSPACE
    assert _unpack(out=COUNT, count=COUNT) == EINVAL


def test_workspace_errors_come_after_argument_errors(lib):
    full = bn.workspace_bytes(CAP)
    assert full > bn.workspace_bytes(0) == 256
    for call in (_pack, _unpack):  # the header alone
        assert call(wb=255) == EWORKSPACE and call(wb=0) == EWORKSPACE and call(w=None) == EWORKSPACE
        assert call(w=WS + 64) == EWORKSPACE and call(w=WS + 128) == EWORKSPACE
    assert _select(wb=full - 1) == EWORKSPACE and _select(wb=0) == EWORKSPACE and _select(w=None) == EWORKSPACE
    assert _select(w=WS + 128) == EWORKSPACE
    assert _select(rows=None, wb=bn.workspace_bytes(N) - 1) == EWORKSPACE  # dense: the candidates are the rows
    for call in (_pack, _unpack, _select):
        assert call(width=0, wb=0) == EINVAL and call(width=33, w=None) == EINVAL and call(cap=1 << 32, wb=0) == EINVAL
    assert _unpack(flags=8, wb=0) == EINVAL and _select(flags=bn.OUTER, w=None) == EINVAL
    assert _unpack(packed=PACKED + 4, wb=0) == EINVAL and _select(packed=PACKED + 8, w=WS + 64) == EINVAL
    assert _pack(out=COL, wb=0) == EINVAL and _unpack(out=PACKED, w=None) == EINVAL
    assert _unpack(rows=None, count=COUNT, wb=0) == EINVAL and _select(rows=None, count=COUNT, w=WS + 64) == EINVAL


def test_ops_refuses_wrong_arguments_before_any_device_call(lib):
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("PackedColumn", "BitPack", "pack", "unpack", "select_range_packed"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    pc = ops.PackedColumn(t, 32, 12, 5)  # the column itself is plain memory
    assert (pc.n_rows, pc.width, pc.base, pc.nbytes, len(pc)) == (32, 12, 5, 48, 32) and pc.packed.numel() == 12
    assert ops.PackedColumn(t, 4, 32, -1).base == 0xFFFFFFFF
    for width in (0, 33, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="width"):
            ops.PackedColumn(t, 4, width)
    for base in (1 << 32, -(1 << 31) - 1, 1.5, True):
        with pytest.raises(ValueError, match="base"):
            ops.PackedColumn(t, 4, 8, base)
    with pytest.raises(ValueError, match="n_rows"):
        ops.PackedColumn(t, 1 << 32, 8)
    with pytest.raises(ValueError, match="words"):
        ops.PackedColumn(t, 33, 16)  # 17 words rounded up to 20
    with pytest.raises(ValueError, match="16-byte"):
        ops.PackedColumn(t[1:], 4, 8)
    with pytest.raises(ValueError, match="int32"):
        ops.PackedColumn(t.long(), 4, 8)
    for call in (lambda: ops.pack(t, 8), lambda: ops.pack(t.float(), 8), lambda: ops.unpack(pc), lambda: ops.unpack(pc, t),
                 lambda: ops.select_range_packed(pc, 0, 1), lambda: ops.select_range_packed(pc, 0, 1, rows=t)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError, match="PackedColumn"):
        ops.unpack(t)
    with pytest.raises(ValueError, match="PackedColumn"):
        ops.select_range_packed(t, 0, 1)
    for fill in (1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="fill"):
            ops.unpack(pc, fill=fill)
    with pytest.raises(ValueError, match="lo"):
        ops.select_range_packed(pc, -1, 1)
    plan = ops.BitPack(100, 12, 7, device="cpu")
    assert plan.ws_bytes == bn.workspace_bytes(100) and plan.packed.numel() == bn.words(100, 12) == 40
    for method in (plan.result, plan.output):
        with pytest.raises(ValueError):
            method()  # nothing launched yet
    with pytest.raises(ValueError, match="on the GPU"):
        plan.launch(t)
    for width in (0, 33):
        with pytest.raises(ValueError, match="width"):
            ops.BitPack(16, width, device="cpu")
    for cap in (1 << 32, 1 << 40):
        with pytest.raises(ValueError):
            ops.BitPack(cap, 8, device="cpu")
    sel = ops.SelectRows(16, device="cpu")
    with pytest.raises(ValueError, match="on the GPU"):
        sel.launch(pc, 0, 1)
    d = ops.Dictionary(16, 4096, device="cpu")
    assert d.packed_width() == 12
    assert [ops.Dictionary(16, c, device="cpu").packed_width() for c in (1, 2, 3, 4, 5, 256, 257, 4097)] == [1, 1, 2, 2, 3, 8, 9, 13]
    assert "bitpack.hpp" in ops.__doc__ and "take_rows.hpp" in ops.__doc__
