"""The quantile select's entry points (dwarf_bench_amd/host/quantile_select.hpp, in libdbench.so) without a GPU: the exported
symbols, the header's constants and prototypes against the binding's and the model's, the workspace query, the host-side
argument checks (all before any HIP call, argument errors before workspace errors), the tensor API's refusals and the binding
on the one library handle.  Every select below fails on the host: the device pointers are fake and never dereferenced."""
import re
import subprocess
from fractions import Fraction

import pytest

from dwarf_bench_amd import _dbench
from dwarf_bench_amd import quantile_native as qn
from tests import quantile_model as qm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "quantile_select.hpp"
FAKE = 1 << 30  # 256-byte aligned
N, CAP = 100002, 50000
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
COL, ROWS, COUNT, VALUES, BELOW, EQUAL, WS = (FAKE + i * STEP for i in range(7))
TOP = (1 << 32) - 1


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return qn.lib()


def test_libdbench_exports_exactly_the_two_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_quantile\w*)$", out, flags=re.M))
    assert names == sorted(qn.ENTRY_POINTS) and len(names) == 2
    assert all(n.startswith("dbench_quantile_") for n in names)
    assert not re.findall(r"\b(?:dbhip_quantile|dbench_\w+_quantile)\w*$", out, flags=re.M)  # none under another prefix
    for word in ("hll", "bloom", "take", "topk"):
        assert not [n for n in names if word in n], word


def test_header_constants_and_prototypes_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_QUANTILE_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_QUANTILE_MAX_RANKS": qn.MAX_RANKS, "DBENCH_QUANTILE_SIGNED": qn.SIGNED}
    protos = dict(re.findall(r"\b(dbench_\w+)\s*\(([^)]*)\)", text))
    assert sorted(protos) == sorted(qn.ENTRY_POINTS)
    for name, args in protos.items():  # as many parameters as the binding passes
        assert len(args.split(",")) == len(qn.ENTRY_POINTS[name][1]), name
    assert (qm.MAX_RANKS, qm.SIGNED) == (16, 1) == (qn.MAX_RANKS, qn.SIGNED)
    from dwarf_bench_amd import ops
    assert qm.KEY_RANGE == ops.DEV_KEY_RANGE and ops.QUANTILE_MAX_RANKS == 16


def test_workspace_query(lib):
    for n_q in (0, -1, 17, 18, 64, 1 << 20, -(1 << 31)):
        assert qn.workspace_bytes(n_q) == 0, n_q
    sizes = [qn.workspace_bytes(n_q) for n_q in range(1, 17)]
    assert all(s >= 256 + 512 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)  # non-decreasing in n_q
    assert len(set(sizes)) == 3 and sizes[0] < sizes[1] == sizes[3] < sizes[4] == sizes[15]  # slot capacities 1, 4, 16
    assert sizes[15] < 1 << 20  # no state per row: well under a MiB whatever the column


def _select(col=COL, n=N, rows=ROWS, count=None, cap=CAP, num=(1,), den=(2,), n_q=None, flags=0, values=VALUES, below=BELOW,
            equal=EQUAL, w=WS, wb=None):
    return qn.select(col, n, rows, count, cap, num, den, flags, values, below, equal, w, 1 << 30 if wb is None else wb, None,
                     n_q=n_q)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for kw in ({}, dict(flags=qn.SIGNED), dict(count=COUNT), dict(rows=None), dict(rows=None, count=COUNT),
               dict(rows=None, cap=0), dict(col=COL + 4, rows=ROWS + 12), dict(n=0, col=None), dict(cap=0),
               dict(rows=None, n=0, col=None), dict(values=VALUES + 4, below=BELOW + 8, equal=EQUAL + 12),
               dict(num=(0,), den=(0,)), dict(num=(TOP,), den=(0,)), dict(num=(TOP,), den=(TOP,)), dict(num=(0,), den=(1,)),
               dict(num=(5, 5), den=(0, 0)), dict(num=tuple(range(16)), den=(16,) * 16), dict(num=(3, 1, 2), den=(3, 2, 0)),
               dict(below=VALUES + 4, equal=VALUES + 8), dict(num=(1, 2), den=(2, 2), below=VALUES + 8, equal=VALUES + 16)):
        assert _select(wb=0, **kw) == EWORKSPACE, kw


def test_every_argument_error_one_at_a_time(lib):
    for flags in (2, 3, 4, 8, -1, 1 << 16):  # unknown flag bits
        assert _select(flags=flags) == EINVAL, flags
    for n_q in (0, -1, 17, 1 << 20):  # n_q outside 1 .. 16
        assert _select(num=(1,) * 16, den=(2,) * 16, n_q=n_q) == EINVAL, n_q
    assert _select(num=None, n_q=1) == EINVAL and _select(den=None, n_q=1) == EINVAL
    assert _select(values=None) == EINVAL and _select(below=None) == EINVAL and _select(equal=None) == EINVAL
    for num, den in (((2,), (1,)), ((TOP,), (TOP - 1,)), ((1, 3), (2, 2)), ((0,) * 15 + (7,), (1,) * 15 + (6,))):  # q_num > q_den > 0
        assert _select(num=num, den=den) == EINVAL, (num, den)
    assert _select(cap=1 << 32) == EINVAL and _select(cap=1 << 40) == EINVAL  # a size of 2^32 or more
    assert _select(n=1 << 32) == EINVAL and _select(n=(1 << 32) + 5, cap=7) == EINVAL
    assert _select(col=None) == EINVAL and _select(col=None, rows=None) == EINVAL  # a NULL column with rows to read
    for off in (1, 2, 3):  # the column, the list or an output off a 4-byte boundary
        assert _select(col=COL + off) == EINVAL and _select(rows=ROWS + off) == EINVAL
        assert _select(values=VALUES + off) == EINVAL and _select(below=BELOW + off) == EINVAL and _select(equal=EQUAL + off) == EINVAL
    for off in (1, 2, 4, 12):  # count off an 8-byte boundary
        assert _select(count=COUNT + off) == EINVAL, off


def test_every_overlap(lib):
    outs = ("values", "below", "equal")
    for n_q in (1, 3, 16):
        num, den, size = (1,) * n_q, (2,) * n_q, 4 * n_q
        for name in outs:
            for where in (COL, COL + 4 * N - 4, COL - size + 4, ROWS, ROWS + 4 * CAP - 4, ROWS - size + 4):
                assert _select(num=num, den=den, **{name: where}) == EINVAL, (n_q, name, where)
            assert _select(num=num, den=den, count=COUNT, **{name: COUNT}) == EINVAL
            assert _select(num=num, den=den, count=COUNT, **{name: COUNT + 4}) == EINVAL
            assert _select(num=num, den=den, count=COUNT, **{name: COUNT - size + 4}) == EINVAL
            # just in front of and just behind an input; the count's bytes without a count; the list's bytes without a list
            for where in (COL + 4 * N, COL - size, ROWS + 4 * CAP, ROWS - size, COUNT):
                assert _select(num=num, den=den, wb=0, **{name: where}) == EWORKSPACE, (n_q, name, where)
            assert _select(num=num, den=den, count=COUNT, wb=0, **{name: COUNT + 8}) == EWORKSPACE
            assert _select(num=num, den=den, rows=None, wb=0, **{name: ROWS}) == EWORKSPACE
        for a, b in (("values", "below"), ("values", "equal"), ("below", "equal")):  # an output against another output
            at = dict(values=VALUES, below=BELOW, equal=EQUAL)
            assert _select(num=num, den=den, **{b: at[a]}) == EINVAL, (n_q, a, b)
            assert _select(num=num, den=den, **{b: at[a] + size - 4}) == EINVAL
            assert _select(num=num, den=den, **{b: at[a] - size + 4}) == EINVAL
            assert _select(num=num, den=den, wb=0, **{b: at[a] + size}) == EWORKSPACE
            assert _select(num=num, den=den, wb=0, **{b: at[a] - size}) == EWORKSPACE


def test_workspace_errors_come_after_argument_errors(lib):
    for n_q in (1, 4, 5, 16):
        num, den = (1,) * n_q, (2,) * n_q
        full = qn.workspace_bytes(n_q)
        assert _select(num=num, den=den, wb=full - 1) == EWORKSPACE and _select(num=num, den=den, wb=0) == EWORKSPACE
        assert _select(num=num, den=den, w=None) == EWORKSPACE
        assert _select(num=num, den=den, w=WS + 64) == EWORKSPACE and _select(num=num, den=den, w=WS + 128) == EWORKSPACE
    assert _select(num=(1,) * 5, den=(2,) * 5, wb=qn.workspace_bytes(4)) == EWORKSPACE
    assert _select(flags=4, wb=0) == EINVAL and _select(n_q=17, w=None) == EINVAL and _select(cap=1 << 32, wb=0) == EINVAL
    assert _select(values=None, w=WS + 64) == EINVAL and _select(num=(2,), den=(1,), wb=0) == EINVAL
    assert _select(count=COUNT + 4, w=None) == EINVAL and _select(values=COL, wb=0) == EINVAL and _select(col=None, wb=0) == EINVAL
    assert _select(below=VALUES, w=None) == EINVAL and _select(rows=ROWS + 2, wb=0) == EINVAL


def test_ops_refuses_wrong_arguments_before_any_device_call(lib):
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("Quantiles", "quantiles", "kth_value", "median", "equi_depth_bounds"):
        assert hasattr(ops, name), name
    assert "host/quantile_select.hpp" in ops.__doc__
    t = torch.zeros(16, dtype=torch.int32)
    for n_q in (0, 17, -1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="n_q: expected"):
            ops.Quantiles(n_q, device="cpu")
    plan = ops.Quantiles(3, device="cpu")
    assert (plan.n_q, plan.ws_bytes) == (3, qn.workspace_bytes(3)) and plan.ws.numel() >= plan.ws_bytes
    assert plan.out.dtype == torch.int32 and tuple(plan.out.shape) == (3, 3)
    with pytest.raises(ValueError, match="nothing was launched"):
        plan.result()
    for qs in ([], [0.5] * 17, list(range(17))):  # no rank, more than 16 ranks
        with pytest.raises(ValueError, match="one to 16 ranks"):
            ops.quantiles(t, qs)
    with pytest.raises(ValueError, match="the plan holds 3"):
        plan.launch(t, [0, 1, 2, 3])
    for q in (-0.1, 1.5, float("nan"), float("inf"), (3, 2), (-1, 2), Fraction(3, 2), Fraction(-1, 2)):  # q outside [0, 1]
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            ops.quantiles(t, [q])
    for q in (-1, 1 << 32):
        with pytest.raises(ValueError, match="absolute rank"):
            ops.quantiles(t, [q])
    for q in ((1, 0), (1, 1 << 32), (0, -2)):
        with pytest.raises(ValueError, match="denominator"):
            ops.quantiles(t, [q])
    for q in (True, "0.5", None, (1, 2, 3), (0.5, 1), [1, 2]):
        with pytest.raises(ValueError, match="expected an int, a"):
            ops.quantiles(t, [q])
    assert ops._quantile_ranks([0, 7, (1, 2), Fraction(2, 6), 0.25, 1.0, 0.0, TOP]) == (
        [0, 7, 1, 1, 1, 1, 0, TOP], [0, 0, 2, 3, 4, 1, 1, 0])
    assert ops._quantile_ranks(0.1) == ([1], [10]) and ops._quantile_ranks(5) == ([5], [0])
    for call in (lambda: ops.quantiles(t, [0.5]), lambda: plan.launch(t, [0.5]), lambda: ops.median(t),
                 lambda: ops.kth_value(t, 3), lambda: ops.equi_depth_bounds(t, 4), lambda: ops.quantiles(t.float(), [0.5])):
        with pytest.raises(ValueError, match="on the GPU"):  # wrong device, wrong dtype
            call()
    for parts in (0, 1, 18, 2.5, True, None):
        with pytest.raises(ValueError, match="parts: expected"):
            ops.equi_depth_bounds(t, parts)
    for k in (1.5, True, None):
        with pytest.raises(ValueError, match="k: expected"):
            ops.kth_value(t, k)


def test_the_binding_lives_on_the_one_handle(lib):
    assert qn.lib() is _dbench.lib() is lib
    assert "quantile_native" not in _dbench.FAMILIES + _dbench.LATER_FAMILIES
    for name, (res, args) in qn.ENTRY_POINTS.items():
        fn = getattr(_dbench.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    from dwarf_bench_amd import hll_native, select_native
    assert hll_native.lib() is qn.lib() is select_native.lib()  # no second copy of the library
