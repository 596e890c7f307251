"""The merge-path entry points (dwarf_bench_amd/host/merge_sorted.hpp, in libdbench.so) without a GPU: the exported
symbols, the header's constants against the binding's and the model's, the workspace query's bound, the host-side
argument checks (all before any HIP call, argument errors before workspace errors) and the tensor API's refusals.
Every call below fails on the host: the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import merge_native as mn
from tests import merge_model as mm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "merge_sorted.hpp"
FAKE = 1 << 30  # 256-byte aligned
NA, NB = 100002, 5000  # even: a count word may sit directly behind a column
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
A_KEYS, A_VALS, B_KEYS, B_VALS, OUT_KEYS, OUT_VALS, A_COUNT, B_COUNT, OUT_COUNT, WS = (FAKE + i * STEP for i in range(10))


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return mn.lib()


def test_libdbench_exports_exactly_the_three_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_(?:merge|setop)_\w+)$", out, flags=re.M))
    assert names == ["dbench_merge_u32", "dbench_merge_workspace_bytes", "dbench_setop_u32"] == sorted(mn.ENTRY_POINTS)
    assert not [n for n in names if n.startswith("dbench_select_")]
    assert not re.findall(r"\bdbhip_(?:merge_sorted|setop)\w*$", out, flags=re.M)  # the dbhip_* surface is include/'s


def test_header_constants_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_(?:MERGE|SETOP)_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_MERGE_TILE_ROWS": mn.TILE_ROWS, "DBENCH_MERGE_SIGNED": mn.SIGNED, "DBENCH_MERGE_ROW_IDS": mn.ROW_IDS,
                   "DBENCH_SETOP_UNION": mn.UNION, "DBENCH_SETOP_INTERSECT": mn.INTERSECT,
                   "DBENCH_SETOP_DIFFERENCE": mn.DIFFERENCE}
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(mn.ENTRY_POINTS)
    assert (mm.SIGNED, mm.ROW_IDS, mm.UNION, mm.INTERSECT, mm.DIFFERENCE) == (mn.SIGNED, mn.ROW_IDS, mn.UNION, mn.INTERSECT,
                                                                              mn.DIFFERENCE)
    assert mn.TILE_ROWS % 2 == 0 and mn.TILE_ROWS >= 64
    from dwarf_bench_amd import ops
    assert ops.SET_OPS == {"union": mn.UNION, "intersect": mn.INTERSECT, "difference": mn.DIFFERENCE}
    assert mm.STATUS == ops.DEV_OK


def test_workspace_query_keeps_its_bound(lib):
    assert "<= 4096 + (a_capacity + b_capacity) / 4" in HEADER.read_text()
    T = mn.TILE_ROWS
    edge = sorted(set(SIZES + (T - 1, T, T + 1, 1024 * T, 1024 * T + 1, 1025 * T + 3, (1 << 31) - 1, 1 << 31)))
    last = 0
    for total in edge:
        for a in sorted(x for x in {0, 1, total // 2, total - 1, total} if 0 <= x <= total):
            got = mn.workspace_bytes(a, total - a)
            assert got % 256 == 0 and 256 <= got <= 4096 + total // 4, (a, total, got)
            assert got == mn.workspace_bytes(total - a, a) and got >= last
            assert got >= 256 + 3 * 4 * (total // T)  # the header, and three words per tile
        last = mn.workspace_bytes(0, total)
    for a in (0, 1, 1 << 20, 1 << 31):  # monotone in either capacity alone
        steps = [mn.workspace_bytes(a, b) for b in (0, 1, T, T + 1, 1 << 20, (1 << 31) - 1)]
        assert steps == sorted(steps) and steps == [mn.workspace_bytes(b, a) for b in (0, 1, T, T + 1, 1 << 20, (1 << 31) - 1)]
    for a, b in ((1 << 32, 0), (0, 1 << 32), (1 << 31, 1 << 31), ((1 << 32) - 1, 1), (1 << 40, 5), (5, 1 << 40)):
        assert mn.workspace_bytes(a, b) == 0, (a, b)
    assert mn.workspace_bytes((1 << 32) - 2, 1) > 0


def _merge(a=A_KEYS, av=None, ac=None, na=NA, b=B_KEYS, bv=None, bc=None, nb=NB, flags=0, out=OUT_KEYS, ov=None,
           oc=OUT_COUNT, w=WS, wb=None):
    if wb is None:
        wb = mn.workspace_bytes(na, nb) or 1 << 40
    return mn.merge(a, av, ac, na, b, bv, bc, nb, flags, out, ov, oc, w, wb, None)


def _setop(op=mn.UNION, a=A_KEYS, ac=None, na=NA, b=B_KEYS, bc=None, nb=NB, out=OUT_KEYS, oc=OUT_COUNT, w=WS, wb=None):
    if wb is None:
        wb = mn.workspace_bytes(na, nb) or 1 << 40
    return mn.setop(op, a, ac, na, b, bc, nb, out, oc, w, wb, None)


CARRIED = dict(av=A_VALS, bv=B_VALS, ov=OUT_VALS)
IDS = dict(flags=mn.ROW_IDS, ov=OUT_VALS)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for kw in ({}, CARRIED, IDS, dict(flags=mn.SIGNED), dict(flags=mn.SIGNED | mn.ROW_IDS, ov=OUT_VALS),
               dict(ac=A_COUNT, bc=B_COUNT), dict(na=0, a=None), dict(nb=0, b=None), dict(na=0, a=None, nb=0, b=None, out=None),
               dict(na=0, a=None, av=None, bv=B_VALS, ov=OUT_VALS)):
        assert _merge(wb=0, **kw) == EWORKSPACE, kw
    for op in (mn.UNION, mn.INTERSECT, mn.DIFFERENCE):
        for kw in ({}, dict(out=None), dict(ac=A_COUNT, bc=B_COUNT), dict(na=0, a=None), dict(na=0, a=None, nb=0, b=None)):
            assert _setop(op, wb=0, **kw) == EWORKSPACE, (op, kw)


def test_every_argument_error_of_the_merge_one_at_a_time(lib):
    for flags in (4, 8, 7, -1, 1 << 16):  # unknown flag bits
        assert _merge(flags=flags) == EINVAL, flags
    for na, nb in ((1 << 32, 0), (0, 1 << 32), (1 << 31, 1 << 31), ((1 << 32) - 1, 1), ((1 << 32) + 5, 7)):  # capacities
        assert _merge(na=na, nb=nb) == EINVAL, (na, nb)
    assert _merge(a=None) == EINVAL and _merge(b=None) == EINVAL and _merge(out=None) == EINVAL  # NULL column, capacity > 0
    assert _merge(oc=None) == EINVAL
    assert _merge(a=None, na=0, ac=A_COUNT) == EINVAL and _merge(b=None, nb=0, bc=B_COUNT) == EINVAL  # a count without column
    # the value-column rules
    assert _merge(av=A_VALS) == EINVAL and _merge(bv=B_VALS) == EINVAL and _merge(av=A_VALS, bv=B_VALS) == EINVAL  # keys only
    assert _merge(flags=mn.ROW_IDS) == EINVAL  # row ids without out_vals
    assert _merge(av=A_VALS, **IDS) == EINVAL and _merge(bv=B_VALS, **IDS) == EINVAL and _merge(av=A_VALS, bv=B_VALS, **IDS) == EINVAL
    assert _merge(ov=OUT_VALS) == EINVAL and _merge(ov=OUT_VALS, av=A_VALS) == EINVAL and _merge(ov=OUT_VALS, bv=B_VALS) == EINVAL
    for off in (1, 2, 3):  # misaligned columns
        for name, at in (("a", A_KEYS), ("b", B_KEYS), ("out", OUT_KEYS), ("av", A_VALS), ("bv", B_VALS), ("ov", OUT_VALS)):
            assert _merge(**{**CARRIED, name: at + off}) == EINVAL, (name, off)
    for off in (1, 2, 4, 12):  # misaligned counts
        assert _merge(oc=OUT_COUNT + off) == EINVAL and _merge(ac=A_COUNT + off) == EINVAL and _merge(bc=B_COUNT + off) == EINVAL


def test_every_argument_error_of_the_set_operations_one_at_a_time(lib):
    for op in (3, 4, -1, 1 << 16):
        assert _setop(op) == EINVAL, op
    for na, nb in ((1 << 32, 0), (0, 1 << 32), (1 << 31, 1 << 31), ((1 << 32) - 1, 1)):
        assert _setop(na=na, nb=nb) == EINVAL, (na, nb)
    assert _setop(a=None) == EINVAL and _setop(b=None) == EINVAL and _setop(oc=None) == EINVAL
    assert _setop(a=None, na=0, ac=A_COUNT) == EINVAL and _setop(b=None, nb=0, bc=B_COUNT) == EINVAL
    for off in (1, 2, 3):
        assert _setop(a=A_KEYS + off) == EINVAL and _setop(b=B_KEYS + off) == EINVAL and _setop(out=OUT_KEYS + off) == EINVAL
    for off in (1, 2, 4, 12):
        assert _setop(oc=OUT_COUNT + off) == EINVAL and _setop(ac=A_COUNT + off) == EINVAL and _setop(bc=B_COUNT + off) == EINVAL


def test_outputs_may_not_overlap_inputs_or_each_other(lib):
    rows = NA + NB
    # out_keys and out_vals against every input column: the column itself, one word shared at either end
    for name in ("out", "ov"):
        for col, n in ((A_KEYS, NA), (B_KEYS, NB), (A_VALS, NA), (B_VALS, NB)):
            for at in (col, col + 4 * (n - 1), col - 4 * (rows - 1)):
                assert _merge(**{**CARRIED, name: at}) == EINVAL, (name, col, at)
            # touching ranges do not overlap: these calls get as far as the workspace check
            assert _merge(wb=0, **{**CARRIED, name: col + 4 * n}) == EWORKSPACE
            assert _merge(wb=0, **{**CARRIED, name: col - 4 * rows}) == EWORKSPACE
    assert _merge(**{**CARRIED, "ov": OUT_KEYS}) == EINVAL  # the two outputs
    assert _merge(**{**CARRIED, "ov": OUT_KEYS + 4 * (rows - 1)}) == EINVAL
    assert _merge(wb=0, **{**CARRIED, "ov": OUT_KEYS + 4 * rows}) == EWORKSPACE
    assert _merge(**{**IDS, "ov": A_KEYS}) == EINVAL
    # the count words
    assert _merge(oc=OUT_KEYS) == EINVAL and _merge(oc=A_KEYS + 8) == EINVAL and _merge(oc=B_KEYS + 4 * NB - 8) == EINVAL
    assert _merge(oc=A_COUNT, ac=A_COUNT) == EINVAL and _merge(oc=B_COUNT, bc=B_COUNT) == EINVAL
    assert _merge(out=A_COUNT - 8, ac=A_COUNT) == EINVAL  # the output's second word is the count
    assert _merge(wb=0, oc=A_KEYS + 4 * NA) == EWORKSPACE and _merge(wb=0, oc=OUT_KEYS + 4 * rows) == EWORKSPACE
    # the set operations: out has room for the op's bound
    for op in (mn.UNION, mn.INTERSECT, mn.DIFFERENCE):
        bound = mn.set_bound(op, NA, NB)
        assert bound == {mn.UNION: rows, mn.INTERSECT: NB, mn.DIFFERENCE: NA}[op]
        for col, n in ((A_KEYS, NA), (B_KEYS, NB)):
            for at in (col, col + 4 * (n - 1), col - 4 * (bound - 1)):
                assert _setop(op, out=at) == EINVAL, (op, col, at)
            assert _setop(op, out=col + 4 * n, wb=0) == EWORKSPACE and _setop(op, out=col - 4 * bound, wb=0) == EWORKSPACE
        assert _setop(op, oc=OUT_KEYS + 4 * bound - 8) == EINVAL and _setop(op, oc=OUT_KEYS + 4 * bound, wb=0) == EWORKSPACE
        assert _setop(op, oc=A_KEYS) == EINVAL and _setop(op, oc=A_COUNT, ac=A_COUNT) == EINVAL
    # the count-only call has no output column to overlap
    assert _setop(out=None, wb=0) == EWORKSPACE


def test_workspace_errors_come_after_argument_errors(lib):
    full = mn.workspace_bytes(NA, NB)
    for call in (_merge, _setop):
        assert call(wb=full - 1) == EWORKSPACE and call(wb=0) == EWORKSPACE and call(w=None) == EWORKSPACE
        assert call(w=WS + 64) == EWORKSPACE and call(w=WS + 128) == EWORKSPACE
        assert call(na=0, a=None, nb=0, b=None, out=None, wb=255) == EWORKSPACE  # no rows: the header and the padded arrays
        assert call(a=None, w=None) == EINVAL and call(oc=None, wb=full - 1) == EINVAL and call(na=1 << 32, wb=0) == EINVAL
        assert call(a=A_KEYS + 2, wb=0) == EINVAL and call(out=A_KEYS, w=WS + 64) == EINVAL
    assert _merge(flags=4, wb=0) == EINVAL and _merge(av=A_VALS, wb=0) == EINVAL and _merge(flags=mn.ROW_IDS, w=None) == EINVAL
    assert _setop(7, wb=0) == EINVAL and _setop(out=None, wb=full - 1) == EWORKSPACE
    assert _merge(wb=full - 1, **CARRIED) == EWORKSPACE and _merge(wb=full - 1, **IDS) == EWORKSPACE


def test_ops_refuses_host_tensors_wrong_types_and_capacities_exceeded():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("MergeSorted", "merge_sorted", "RowSets", "union_rows", "intersect_rows", "difference_rows", "select_any"):
        assert hasattr(ops, name), name
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: ops.merge_sorted(t, t), lambda: ops.merge_sorted(t.float(), t), lambda: ops.merge_sorted(t, t.long()),
                 lambda: ops.union_rows(t, t), lambda: ops.intersect_rows(t.long(), t), lambda: ops.difference_rows(t, t.float()),
                 lambda: ops.select_any(t, 0, 1, t, 0, 1)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError, match="lo|hi"):
        ops.select_any(t, -1, 1, t, 0, 1)
    with pytest.raises(ValueError, match="lo|hi"):
        ops.select_any(t, 0, 1, t, 0, 1 << 32)
    with pytest.raises(ValueError, match="16 and 8 rows"):
        ops.select_any(t, 0, 1, t[:8], 0, 1)  # two row spaces
    plan = ops.MergeSorted(16, 8, device="cpu")  # the plan itself is plain memory
    assert plan.ws_bytes == mn.workspace_bytes(16, 8) and plan.out_keys.numel() == plan.out_vals.numel() == 24
    sets = ops.RowSets(16, 8, device="cpu")
    assert sets.ws_bytes == plan.ws_bytes and sets.rows.numel() == 24
    with pytest.raises(ValueError, match="on the GPU"):
        plan.launch(t, t[:8])
    with pytest.raises(ValueError, match="on the GPU"):
        sets.launch("union", t, t[:8])
    for p in (plan, sets):
        with pytest.raises(ValueError):
            p.result()  # nothing launched yet
    with pytest.raises(ValueError, match="op"):
        sets.launch("xor", t, t)
    with pytest.raises(ValueError, match="op"):
        sets.launch(3, t, t)
    for cls in (ops.MergeSorted, ops.RowSets):
        for a, b in ((1 << 32, 0), (1 << 31, 1 << 31), (0, 1 << 32)):
            with pytest.raises(ValueError):
                cls(a, b, device="cpu")
    select = ops.SelectRows(16, device="cpu")
    with pytest.raises(ValueError):
        select.output()  # nothing launched yet
    assert "select_rows.hpp" in ops.__doc__ and "merge_sorted.hpp" in ops.__doc__
