"""The Bloom filter entry points (dwarf_bench_amd/host/bloom_filter.hpp, in libdbench.so) without a GPU: the exported
symbols, the header's constants against the binding's and the model's, the two size queries, the host-side argument checks
(all before any HIP call, argument errors before workspace errors) and the tensor API's refusals.  Every call below fails
on the host: the pointers are fake and never dereferenced."""
import re
import subprocess

import pytest

from dwarf_bench_amd import bloom_native as bl
from dwarf_bench_amd import select_native as sn
from tests import bloom_model as blm
from tests.capi_testlib import EINVAL, EWORKSPACE, LIB, ROOT, SIZES, ensure_built

HEADER = ROOT / "dwarf_bench_amd" / "host" / "bloom_filter.hpp"
FAKE = 1 << 30  # 256-byte aligned
N, CAP, WORDS = 100002, 50000, 30000
STEP = 1 << 24  # bytes between the fake buffers: more than any of them holds
COL, FILTER, ROWS, COUNT, OUT, OUT_COUNT, WS = (FAKE + i * STEP for i in range(7))


@pytest.fixture(scope="module")
def lib():
    ensure_built()
    return bl.lib()


def test_libdbench_exports_exactly_the_bloom_entry_points(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB / "libdbench.so")], capture_output=True, text=True,
                         check=True, timeout=60).stdout
    names = sorted(re.findall(r"\b(dbench_bloom\w*)$", out, flags=re.M))
    assert names == sorted(bl.ENTRY_POINTS) and len(names) == 4
    assert all(n.startswith("dbench_bloom_") for n in names)
    assert not re.findall(r"\bdbhip_bloom\w*$", out, flags=re.M)
    other = re.findall(r"\b(dbench_(?:select_|dict|take|aggregate|merge_|setop_|bitpack_)\w*)$", out, flags=re.M)
    assert other and not [n for n in other if "bloom" in n]


def test_header_constants_are_the_bindings_and_the_models():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    got = {k: int(v) for k, v in re.findall(r"^#define (DBENCH_BLOOM_\w+) (\d+)", text, flags=re.M)}
    assert got == {"DBENCH_BLOOM_ACCUMULATE": bl.ACCUMULATE, "DBENCH_BLOOM_NEGATE": bl.NEGATE}
    assert sorted(re.findall(r"\b(dbench_\w+)\s*\(", text)) == sorted(bl.ENTRY_POINTS)
    assert (blm.ACCUMULATE, blm.NEGATE) == (bl.ACCUMULATE, bl.NEGATE) == (1, 2)
    assert bl.NEGATE == sn.NEGATE  # what DBENCH_SELECT_NEGATE means
    from dwarf_bench_amd import ops
    assert blm.KEY_RANGE == ops.DEV_KEY_RANGE


def test_workspace_query_is_selects(lib):
    for c in SIZES + (0, 1, 4095, 4096, 4097, 2 * 4096 + 1, (1 << 32) - 1):
        assert bl.workspace_bytes(c) == sn.workspace_bytes(c) != 0, c
    for c in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert bl.workspace_bytes(c) == 0 == sn.workspace_bytes(c), c
    assert bl.workspace_bytes(0) >= 256


def test_words_equal_the_model(lib):
    counts = (0, 1, 3, 4, 5, 63, 64, 65, 1000, 1 << 16, 1 << 24, (1 << 26) - 1, 1 << 26, (1 << 26) + 1, (1 << 32) - 1, 1 << 32,
              (1 << 35) - 1, 1 << 35, (1 << 38) - 1, 1 << 38, 1 << 40, 1 << 63, (1 << 64) - 1)
    for bits in (1, 2, 7, 8, 12, 16, 24, 63, 64):
        for n in counts:
            assert bl.words(n, bits) == blm.words(n, bits), (n, bits)
    for bits in (0, 65, 128, 1 << 16, -1):
        for n in counts:
            assert bl.words(n, bits) == 0, (n, bits)
    assert bl.words(1 << 24, 16) * 8 == 32 << 20 and bl.words(0, 16) == 1 and bl.words(1 << 32, 64) == 0
    assert bl.words((1 << 32) - 1, 64) == (1 << 32) - 1 and bl.words(1 << 32, 63) == 63 << 26


def _build(col=COL, n=N, rows=ROWS, count=None, cap=CAP, seed=0, flags=0, filt=FILTER, words=WORDS, w=WS, wb=None):
    return bl.build(col, n, rows, count, cap, seed, flags, filt, words, w, 1 << 20 if wb is None else wb, None)


def _probe(filt=FILTER, words=WORDS, seed=0, col=COL, n=N, rows=ROWS, count=None, cap=CAP, flags=0, out=OUT,
           out_count=OUT_COUNT, w=WS, wb=None):
    if wb is None:
        wb = bl.workspace_bytes(cap if rows else n) or 1 << 40
    return bl.probe(filt, words, seed, col, n, rows, count, cap, flags, out, out_count, w, wb, None)


def test_valid_calls_get_as_far_as_the_workspace_check(lib):
    """every mode with wb = 0: the argument checks pass, the workspace check answers"""
    for words in (1, 2, 3, 1000, (1 << 32) - 1):
        far = dict(filt=1 << 44) if words > 1000 else {}  # 32 GiB of filter: away from the other fake buffers
        for kw in ({}, dict(flags=bl.ACCUMULATE), dict(count=COUNT), dict(rows=None), dict(rows=None, count=COUNT),
                   dict(rows=None, cap=0), dict(seed=0xFFFFFFFF),
                   dict(col=COL + 4, rows=ROWS + 12), dict(n=0, col=None), dict(cap=0), dict(rows=None, n=0, col=None),
                   dict(filt=FILTER + 8)):
            assert _build(words=words, wb=0, **{**kw, **far}) == EWORKSPACE, (words, kw)
        for kw in ({}, dict(flags=bl.NEGATE), dict(count=COUNT), dict(rows=None), dict(out=None), dict(seed=0xFFFFFFFF),
                   dict(n=0, col=None), dict(rows=ROWS + 4, out=OUT + 12, col=COL + 8), dict(filt=FILTER + 8), dict(cap=0)):
            assert _probe(words=words, wb=0, **{**kw, **far}) == EWORKSPACE, (words, kw)


def test_every_argument_error_one_at_a_time(lib):
    for call in (_build, _probe):
        for words in (0, 1 << 32, (1 << 32) + 1, 1 << 40):  # n_words == 0 or >= 2^32
            assert call(words=words) == EINVAL, (call.__name__, words)
        assert call(cap=1 << 32) == EINVAL and call(cap=1 << 40) == EINVAL  # a size of 2^32 or more
        assert call(n=1 << 32) == EINVAL and call(n=(1 << 32) + 5, cap=7) == EINVAL
        assert call(filt=None) == EINVAL  # a NULL filter
        assert call(col=None) == EINVAL   # a NULL column with rows to read
        for off in (1, 2, 4, 12):         # a filter off an 8-byte boundary
            assert call(filt=FILTER + off) == EINVAL, off
        for off in (1, 2, 3):             # a list or column off a 4-byte boundary
            assert call(col=COL + off) == EINVAL and call(rows=ROWS + off) == EINVAL
        for off in (1, 2, 4, 12):         # a count off an 8-byte boundary
            assert call(count=COUNT + off) == EINVAL, off
    # unknown flag bits: build knows ACCUMULATE only, probe NEGATE only
    for flags in (bl.NEGATE, bl.ACCUMULATE | bl.NEGATE, 4, 8, -1, 1 << 16):
        assert _build(flags=flags) == EINVAL, flags
    for flags in (bl.ACCUMULATE, bl.ACCUMULATE | bl.NEGATE, 4, 8, -1, 1 << 16):
        assert _probe(flags=flags) == EINVAL, flags
    # probe alone
    assert _probe(out_count=None) == EINVAL
    assert _probe(rows=None, count=COUNT) == EINVAL  # in_count without in_rows
    for off in (1, 2, 3):
        assert _probe(out=OUT + off) == EINVAL
    for off in (1, 2, 4, 12):
        assert _probe(out_count=OUT_COUNT + off) == EINVAL


def test_every_overlap(lib):
    fb = 8 * WORDS
    # build: the filter against col, the list and the count
    for where in (COL, COL + 4 * N - 8, COL - fb + 8, ROWS, ROWS + 4 * CAP - 8, ROWS - fb + 8):
        assert _build(filt=where) == EINVAL, where
    assert _build(filt=COL + (4 * N + 7) // 8 * 8, wb=0) == EWORKSPACE and _build(filt=COL - fb, wb=0) == EWORKSPACE
    assert _build(filt=ROWS + 4 * CAP, wb=0) == EWORKSPACE and _build(filt=ROWS - fb, wb=0) == EWORKSPACE
    assert _build(filt=COUNT, count=COUNT) == EINVAL and _build(filt=COUNT - fb + 8, count=COUNT) == EINVAL
    assert _build(filt=COUNT, wb=0) == EWORKSPACE and _build(filt=COUNT + 8, count=COUNT, wb=0) == EWORKSPACE
    assert _build(filt=ROWS, rows=None, wb=0) == EWORKSPACE  # (no list given)
    # probe: out_rows against the filter, col and in_rows
    for where in (FILTER, FILTER + fb - 4, FILTER - 4 * (CAP - 1), COL, COL + 4 * (N - 1), COL - 4 * (CAP - 1), ROWS,
                  ROWS + 4 * (CAP - 1), ROWS - 4 * (CAP - 1)):
        assert _probe(out=where) == EINVAL, where
    for where in (FILTER + fb, FILTER - 4 * CAP, COL + 4 * N, COL - 4 * CAP, ROWS + 4 * CAP, ROWS - 4 * CAP):
        assert _probe(out=where, wb=0) == EWORKSPACE, where
    # dense: the output holds n rows
    assert _probe(rows=None, out=FILTER - 4 * (N - 1)) == EINVAL and _probe(rows=None, out=FILTER - 4 * N, wb=0) == EWORKSPACE


def test_workspace_errors_come_after_argument_errors(lib):
    full = bl.workspace_bytes(CAP)
    assert full > bl.workspace_bytes(0) >= 256
    assert _build(wb=255) == EWORKSPACE and _build(wb=0) == EWORKSPACE and _build(w=None) == EWORKSPACE  # the header alone
    assert _build(w=WS + 64) == EWORKSPACE and _build(w=WS + 128) == EWORKSPACE
    assert _probe(wb=full - 1) == EWORKSPACE and _probe(wb=0) == EWORKSPACE and _probe(w=None) == EWORKSPACE
    assert _probe(w=WS + 128) == EWORKSPACE
    assert _probe(rows=None, wb=bl.workspace_bytes(N) - 1) == EWORKSPACE  # dense: the candidates are the rows
    for call in (_build, _probe):
        assert call(words=0, wb=0) == EINVAL and call(words=1 << 32, w=None) == EINVAL and call(cap=1 << 32, wb=0) == EINVAL
        assert call(flags=4, wb=0) == EINVAL and call(filt=None, w=WS + 64) == EINVAL and call(filt=FILTER + 4, wb=0) == EINVAL
        assert call(col=None, wb=0) == EINVAL and call(count=COUNT + 4, w=None) == EINVAL
    assert _build(filt=COL, wb=0) == EINVAL and _probe(out=FILTER, w=None) == EINVAL
    assert _probe(out_count=None, wb=0) == EINVAL and _probe(rows=None, count=COUNT, w=WS + 64) == EINVAL


def test_ops_refuses_wrong_arguments_before_any_device_call(lib):
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("BloomFilter", "bloom_words", "bloom_build", "select_in_bloom"):
        assert hasattr(ops, name), name
    assert hasattr(ops.SelectRows, "launch_in") and hasattr(ops.SelectRows, "refine_in")
    assert "host/bloom_filter.hpp" in ops.__doc__
    assert ops.bloom_words(1 << 24) == 1 << 22 and ops.bloom_words(0) == 1 and ops.bloom_words(5, 64) == 5
    for bits in (0, 65, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="bits_per_key"):
            ops.bloom_words(100, bits)
    for n in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="n_keys"):
            ops.bloom_words(n)
    with pytest.raises(ValueError, match="2\\^32"):
        ops.bloom_words(1 << 32, 64)
    t = torch.zeros(16, dtype=torch.int32)
    bloom = ops.BloomFilter(10, 7, device="cpu")
    assert (bloom.n_words, bloom.seed, bloom.ws_bytes) == (10, 7, 256)
    assert bloom.filter.dtype == torch.int64 and bloom.filter.numel() == 10
    for n_words in (0, -1, 1 << 32, 1.5, True, None):
        with pytest.raises(ValueError, match="n_words"):
            ops.BloomFilter(n_words, device="cpu")
    for seed in (-1, 1 << 32, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            ops.BloomFilter(4, seed, device="cpu")
    for call in (lambda: bloom.build(t), lambda: bloom.build(t.float()), lambda: bloom.build(t, rows=t),
                 lambda: ops.bloom_build(t), lambda: ops.select_in_bloom(bloom, t), lambda: ops.select_in_bloom(bloom, t, rows=t),
                 lambda: ops.semi_join(t, t, bloom_bits=16)):
        with pytest.raises(ValueError, match="on the GPU"):
            call()
    with pytest.raises(ValueError, match="BloomFilter"):
        ops.select_in_bloom(t, t)
    sel = ops.SelectRows(16, device="cpu")
    assert sel.ws_bytes >= bl.workspace_bytes(16)
    with pytest.raises(ValueError, match="BloomFilter"):
        sel.launch_in(t, t)
    with pytest.raises(ValueError, match="on the GPU"):
        sel.launch_in(bloom, t)
    with pytest.raises(ValueError, match="nothing was launched"):
        sel.refine_in(bloom, t)
    for bits in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match="bits_per_key"):
            ops.semi_join(t, t, bloom_bits=bits)
