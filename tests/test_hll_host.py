"""The HyperLogLog entry points (dwarf_bench_amd/host/hll_sketch.hpp, in libdbench.so) without a GPU: the exported symbols,
the header's constants and prototypes against the binding's and the model's, the workspace query, the host-side argument
checks (all before any HIP call, argument errors before workspace errors), the host estimator against the model, the tensor
API's refusals and the binding on the one library handle.  Every build and merge below fails on the host: the pointers are
fake and never dereferenced."""
import math
import re
import subprocess

import numpy as np
import pytest

from dwarf_bench_amd import _dbench
from dwarf_bench_amd import hll_native as hl
from tests import hll_model as hm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "hll_sketch.hpp"
LAYOUT = ROOT / "dwarf_bench_amd" / "host" / "hll_layout.hpp"
FAKE = 1 << 30  # 256-byte aligned
N, CAP, P = 100002, 50000, 12
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
C0, C1, C2, C3, ROWS, COUNT, REGS, HIST, SRC, WS = (FAKE + i * STEP for i in range(10))
COLS = (C0, C1, C2, C3)


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return hl.lib()


def test_libdbench_exports_exactly_the_four_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_hll\w*)$", out, flags=re.M))
    assert names == sorted(hl.ENTRY_POINTS) and len(names) == 4
    assert all(n.startswith("dbench_hll_") for n in names)
    assert not re.findall(r"\b(?:dbhip_hll|dbench_\w+_hll)\w*$", out, flags=re.M)  # none under another prefix
    for word in ("dict", "take", "aggregate", "bloom"):
        assert not [n for n in names if word in n], word


def test_header_constants_and_prototypes_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_HLL_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_HLL_ACCUMULATE": hl.ACCUMULATE, "DBENCH_HLL_MAX_GRID": hl.MAX_GRID}
    protos = dict(re.findall(r"\b(dbench_\w+)\s*\(([^)]*)\)", text))
    assert sorted(protos) == sorted(hl.ENTRY_POINTS)
    for name, args in protos.items():  # as many parameters as the binding passes
        assert len(args.split(",")) == len(hl.ENTRY_POINTS[name][1]), name
    layout = {k: int(v) for k, v in re.findall(r"^#define DBENCH_HLL_(\w+) (\d+)$", LAYOUT.read_text(), flags=re.M)}
    assert layout == {"MIN_P": hl.MIN_P, "MAX_P": hl.MAX_P, "MAX_COLS": hl.MAX_COLS, "HIST_WORDS": hl.HIST_WORDS}
    assert (hm.MIN_P, hm.MAX_P, hm.MAX_COLS, hm.HIST_WORDS, hm.ACCUMULATE) == (4, 14, 4, 64, 1) == (
        hl.MIN_P, hl.MAX_P, hl.MAX_COLS, hl.HIST_WORDS, hl.ACCUMULATE)
    from dwarf_bench_amd import ops
    assert hm.KEY_RANGE == ops.DEV_KEY_RANGE


def test_workspace_query(lib):
    for p in (0, 1, 3, 15, 16, 64, 1 << 20, 0xFFFFFFFF):
        assert hl.workspace_bytes(p) == 0, p
    sizes = [hl.workspace_bytes(p) for p in range(4, 15)]
    assert all(s >= 256 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    for p, s in zip(range(4, 15), sizes):  # the header, the partial histograms, one partial sketch per workgroup
        assert s == 256 + 64 * 256 + hl.MAX_GRID * (1 << p), p


def _build(cols=COLS[:1], n_cols=None, n=N, rows=ROWS, count=None, cap=CAP, seed=0, flags=0, p=P, regs=REGS, hist=HIST, w=WS,
           wb=None):
    return hl.build(cols, n, rows, count, cap, seed, flags, p, regs, hist, w, 1 << 30 if wb is None else wb, None, n_cols=n_cols)


def _merge(dst=REGS, src=SRC, p=P, hist=HIST, w=WS, wb=None):
    return hl.merge(dst, src, p, hist, w, 1 << 30 if wb is None else wb, None)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for p in (4, 5, 11, 12, 14):
        for kw in ({}, dict(flags=hl.ACCUMULATE), dict(count=COUNT), dict(rows=None), dict(rows=None, count=COUNT),
                   dict(rows=None, cap=0), dict(seed=0xFFFFFFFF), dict(cols=COLS[:2]), dict(cols=COLS[:3]), dict(cols=COLS),
                   dict(cols=(C0 + 4, C1 + 8, C2 + 12, C3), rows=ROWS + 12), dict(n=0, cols=(None, None)), dict(cap=0),
                   dict(rows=None, n=0, cols=(None,)), dict(regs=REGS + 4), dict(hist=HIST + 8),
                   dict(cols=(C0, C0)), dict(cols=(C0, None, None, None), n_cols=1)):
            assert _build(p=p, wb=0, **kw) == EWORKSPACE, (p, kw)
        for kw in ({}, dict(src=REGS), dict(dst=REGS + 4, src=SRC + 4), dict(hist=HIST + 8), dict(src=REGS + (1 << p)),
                   dict(src=REGS - (1 << p))):
            assert _merge(p=p, wb=0, **kw) == EWORKSPACE, (p, kw)


def test_every_argument_error_one_at_a_time(lib):
    for flags in (2, 3, 4, 8, -1, 1 << 16):  # unknown flag bits
        assert _build(flags=flags) == EINVAL, flags
    for p in (0, 3, 15, 16, 64, 0xFFFFFFFF):  # p outside 4 .. 14
        assert _build(p=p) == EINVAL and _merge(p=p) == EINVAL, p
    for n_cols in (0, -1, 5, 1 << 20):  # n_cols outside 1 .. 4
        assert _build(cols=COLS, n_cols=n_cols) == EINVAL, n_cols
    assert _build(cap=1 << 32) == EINVAL and _build(cap=1 << 40) == EINVAL  # a size of 2^32 or more
    assert _build(n=1 << 32) == EINVAL and _build(n=(1 << 32) + 5, cap=7) == EINVAL
    assert _build(regs=None) == EINVAL and _build(hist=None) == EINVAL and _build(cols=None, n_cols=1) == EINVAL
    for k in range(1, 5):  # a NULL column with rows to read: any of them
        for j in range(k):
            cols = list(COLS[:k])
            cols[j] = None
            assert _build(cols=cols) == EINVAL, (k, j)
    for off in (1, 2, 3):  # registers, a list or a column off a 4-byte boundary
        assert _build(regs=REGS + off) == EINVAL and _build(rows=ROWS + off) == EINVAL
        for j in range(4):
            cols = list(COLS)
            cols[j] += off
            assert _build(cols=cols) == EINVAL, (off, j)
    for off in (1, 2, 4, 12):  # hist and count off an 8-byte boundary
        assert _build(hist=HIST + off) == EINVAL and _build(count=COUNT + off) == EINVAL, off
        assert _merge(hist=HIST + off) == EINVAL
    # merge alone
    assert _merge(dst=None) == EINVAL and _merge(src=None) == EINVAL and _merge(hist=None) == EINVAL
    for off in (1, 2, 3):
        assert _merge(dst=REGS + off) == EINVAL and _merge(src=SRC + off) == EINVAL


def test_every_overlap(lib):
    m = 1 << P
    # build: the registers and the histogram against every column, the list, the count and each other
    for j in range(4):
        for where in (COLS[j], COLS[j] + 4 * N - 4, COLS[j] - m + 4):
            assert _build(cols=COLS, regs=where) == EINVAL, (j, where)
        for where in (COLS[j], COLS[j] + 4 * N - 8, COLS[j] - 256 + 8):
            assert _build(cols=COLS, hist=where) == EINVAL, (j, where)
        assert _build(cols=COLS, regs=COLS[j] + 4 * N, wb=0) == EWORKSPACE and _build(cols=COLS, regs=COLS[j] - m, wb=0) == EWORKSPACE
        assert _build(cols=COLS, hist=COLS[j] + 4 * N, wb=0) == EWORKSPACE and _build(cols=COLS, hist=COLS[j] - 256, wb=0) == EWORKSPACE
    assert _build(regs=C1, wb=0) == EWORKSPACE  # (a column the call does not read)
    for where in (ROWS, ROWS + 4 * CAP - 4, ROWS - m + 4):
        assert _build(regs=where) == EINVAL, where
    assert _build(hist=ROWS) == EINVAL and _build(hist=ROWS + 4 * CAP - 8) == EINVAL and _build(hist=ROWS - 248) == EINVAL
    assert _build(regs=ROWS + 4 * CAP, wb=0) == EWORKSPACE and _build(regs=ROWS, rows=None, wb=0) == EWORKSPACE
    assert _build(regs=COUNT, count=COUNT) == EINVAL and _build(regs=COUNT - m + 4, count=COUNT) == EINVAL
    assert _build(hist=COUNT, count=COUNT) == EINVAL and _build(hist=COUNT - 248, count=COUNT) == EINVAL
    assert _build(regs=COUNT, wb=0) == EWORKSPACE and _build(regs=COUNT + 8, count=COUNT, wb=0) == EWORKSPACE
    for where in (REGS, REGS + m - 8, REGS - 248):
        assert _build(hist=where) == EINVAL and _merge(hist=where) == EINVAL, where
    assert _build(hist=REGS + m, wb=0) == EWORKSPACE and _build(hist=REGS - 256, wb=0) == EWORKSPACE
    # merge: hist against src, and src against dst unless they are equal
    for where in (SRC, SRC + m - 8, SRC - 248):
        assert _merge(hist=where) == EINVAL, where
    for where in (REGS + 4, REGS + m - 4, REGS - m + 4):
        assert _merge(src=where) == EINVAL, where
    assert _merge(src=REGS, wb=0) == EWORKSPACE and _merge(src=REGS + m, wb=0) == EWORKSPACE


def test_workspace_errors_come_after_argument_errors(lib):
    full = hl.workspace_bytes(P)
    assert _build(wb=full - 1) == EWORKSPACE and _build(wb=0) == EWORKSPACE and _build(w=None) == EWORKSPACE
    assert _build(w=WS + 64) == EWORKSPACE and _build(w=WS + 128) == EWORKSPACE
    assert _build(p=14, wb=hl.workspace_bytes(13)) == EWORKSPACE
    merge_needs = 256 + 64 * 256  # the header and the partial histograms
    assert _merge(wb=merge_needs - 1) == EWORKSPACE and _merge(wb=0) == EWORKSPACE and _merge(w=None) == EWORKSPACE
    assert _merge(w=WS + 128) == EWORKSPACE and merge_needs <= hl.workspace_bytes(4)
    assert _build(flags=4, wb=0) == EINVAL and _build(p=15, w=None) == EINVAL and _build(cap=1 << 32, wb=0) == EINVAL
    assert _build(regs=None, w=WS + 64) == EINVAL and _build(hist=HIST + 4, wb=0) == EINVAL and _build(cols=(None,), wb=0) == EINVAL
    assert _build(count=COUNT + 4, w=None) == EINVAL and _build(regs=C0, wb=0) == EINVAL and _build(cols=COLS, n_cols=5, wb=0) == EINVAL
    assert _merge(p=3, wb=0) == EINVAL and _merge(src=None, w=None) == EINVAL and _merge(src=REGS + 4, wb=0) == EINVAL
    assert _merge(hist=REGS, w=WS + 64) == EINVAL


def random_histogram(rng, p):
    """a histogram some sketch of 2^p registers could have: m registers thrown at the values 0 .. q+1"""
    q, m = 64 - p, 1 << p
    kind = int(rng.integers(0, 4))
    if kind == 0:    # as a sketch of n keys has them: geometric in the rank
        n = int(2 ** rng.uniform(0, 30))
        lam = n / m
        ranks = np.arange(q + 2)
        cdf = np.exp(-lam / 2.0 ** np.minimum(ranks, q))  # P(register <= k)
        cdf[q + 1] = 1.0
        pmf = np.diff(np.r_[0.0, cdf]).clip(0)
        hist = rng.multinomial(m, pmf / pmf.sum())
    elif kind == 1:  # anything
        hist = rng.multinomial(m, rng.dirichlet(np.ones(q + 2)))
    elif kind == 2:  # mostly empty
        hist = rng.multinomial(m, np.r_[0.99, np.full(q + 1, 0.01 / (q + 1))])
    else:            # mostly saturated
        hist = rng.multinomial(m, np.r_[np.full(q + 1, 0.01 / (q + 1)), 0.99])
    return [int(v) for v in hist] + [0] * (64 - q - 2)


def test_estimate_equals_the_model(lib):
    rng = np.random.default_rng(11)
    seen = 0
    for p in range(4, 15):
        for _ in range(40):
            hist = random_histogram(rng, p)
            assert sum(hist) == 1 << p
            got, want = hl.estimate(hist, p), hm.estimate(hist, p)
            if math.isinf(want) or want == 0.0:
                assert got == want
            else:
                assert want > 0 and abs(got - want) <= 1e-12 * want, (p, hist, got, want)
                seen += 1
    assert seen > 350  # of 440: the rest drew an empty or a saturated sketch (small p, few or very many keys)
    # sketches of real key sets: the estimate the model tests hold within four standard errors
    for p, n in ((4, 100), (11, 10 ** 4), (14, 10 ** 5)):
        hist = hm.build(np.arange(1, n + 1, dtype=np.uint32), p, 0xDEADBEEF)[1]
        got = hl.estimate(hist, p)
        assert abs(got - hm.estimate(hist, p)) <= 1e-12 * got and abs(got - n) <= 4 * hm.relative_error(p) * n


def test_estimate_corners_and_refusals(lib):
    for p in range(4, 15):
        m, q = 1 << p, 64 - p
        empty = [m] + [0] * 63
        assert hl.estimate(empty, p) == 0.0  # exactly
        full = [0] * 64
        full[q + 1] = m
        assert math.isinf(hl.estimate(full, p)) and hl.estimate(full, p) > 0
        one = empty[:]
        one[0], one[3] = m - 1, 1
        assert 0.9 < hl.estimate(one, p) < 1.1
        for bad in ([m - 1] + [0] * 63, [m + 1] + [0] * 63, [0] * 64, [m - 1] + [0] * (q + 1) + [1] + [0] * (62 - q - 1),
                    [m - 1] + [0] * 62 + [1]):
            assert len(bad) == 64 and hl.estimate(bad, p) == -1.0 == hm.estimate(bad, p), (p, bad)
    for p in (0, 3, 15, 64, 0xFFFFFFFF):
        assert hl.estimate([1 << min(p, 20)] + [0] * 63, p) == -1.0, p
    assert lib.dbench_hll_estimate(None, 12) == -1.0


def test_ops_refuses_wrong_arguments_before_any_device_call(lib):
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("HyperLogLog", "approx_count_distinct", "hll_relative_error"):
        assert hasattr(ops, name), name
    assert "host/hll_sketch.hpp" in ops.__doc__
    assert ops.hll_relative_error(12) == 1.04 / 64 and ops.hll_relative_error(4) == 0.26 and ops.hll_relative_error(14) == 1.04 / 128
    for p in (3, 15, 0, -1, 1.5, True, None, "12"):
        with pytest.raises(ValueError, match="p: expected"):
            ops.hll_relative_error(p)
        with pytest.raises(ValueError, match="p: expected"):
            ops.HyperLogLog(p, device="cpu")
        with pytest.raises(ValueError, match="p: expected"):
            ops.approx_count_distinct(torch.zeros(4, dtype=torch.int32), p=p)
    for seed in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            ops.HyperLogLog(12, seed, device="cpu")
    sketch = ops.HyperLogLog(device="cpu")
    assert (sketch.p, sketch.seed, sketch.m, sketch.ws_bytes) == (12, 0, 4096, hl.workspace_bytes(12))
    assert sketch.registers.dtype == torch.uint8 and sketch.registers.numel() == 4096
    assert sketch.hist.dtype == torch.int32 and sketch.hist.numel() == 64 and sketch.hist.tolist() == [4096] + [0] * 63
    assert sketch.ws.numel() >= sketch.ws_bytes
    t = torch.zeros(16, dtype=torch.int32)
    for call in (lambda: sketch.build(t), lambda: sketch.build([t, t]), lambda: sketch.build(t.float()),
                 lambda: ops.approx_count_distinct(t), lambda: ops.approx_count_distinct((t, t, t, t))):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    for cols in ([], [t] * 5):
        with pytest.raises(ValueError, match="one to 4 columns"):
            sketch.build(cols)
    with pytest.raises(ValueError, match="columns of one table"):
        sketch.build([t, t[:5]])
    with pytest.raises(ValueError, match="expected a tensor"):
        sketch.build([t, 5])
    with pytest.raises(ValueError, match="HyperLogLog"):
        sketch.merge(t)
    with pytest.raises(ValueError, match="does not merge"):
        sketch.merge(ops.HyperLogLog(11, device="cpu"))
    with pytest.raises(ValueError, match="does not merge"):
        sketch.merge(ops.HyperLogLog(12, 1, device="cpu"))
    with pytest.raises(ValueError, match="on the GPU"):
        sketch.merge(ops.HyperLogLog(12, device="cpu"))


def test_the_binding_lives_on_the_one_handle(lib):
    assert hl.lib() is _dbench.lib() is lib
    assert "hll_native" not in _dbench.FAMILIES + _dbench.LATER_FAMILIES
    for name, (res, args) in hl.ENTRY_POINTS.items():
        fn = getattr(_dbench.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    from dwarf_bench_amd import bloom_native, select_native
    assert bloom_native.lib() is hl.lib() is select_native.lib()  # no second copy of the library
