"""The top-k (include/dbhip_topk.h) on the GPU against numpy: np.argsort(kind="stable") on the masked keys, the first
m = min(k, n), re-sorted by row for sorted=False (tests/topk_model.py).  Every call here runs on guarded buffers
(tests/guard_testlib.py): the key column frozen, output columns of exactly k entries whose entries [m, k) must keep the
guard word, a workspace of exactly the queried size.

C = ops.TOPK_CHUNK_ROWS is one workgroup's rows in the count and write kernels, S = ops.TOPK_SEGMENT_ROWS one wave's."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import topk_model as tm
from tests.guard_testlib import FILLS, Watch, i32, ptr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_topk"
M32 = 0xFFFFFFFF
INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF
ORDERS = [(False, False), (False, True), (True, False), (True, True)]  # (largest, signed)
C, S = 32768, 4096


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_the_tests_know_the_chunk_size():
    assert (_ops().TOPK_CHUNK_ROWS, _ops().TOPK_SEGMENT_ROWS) == (C, S)


def uniform(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


class Column:
    """a frozen, guarded key column on the device and its stable argsorts under the four orders (computed once)"""

    def __init__(self, host, fill=FILLS[0]):
        self.host = np.ascontiguousarray(host, dtype=np.uint32)
        self.n = self.host.size
        self.watch = Watch(fill)
        self.dev = self.watch.col(self.n, data=self.host, freeze=True)
        self._order = {}

    def want(self, k, largest, signed, srt):
        key = (largest, signed)
        if key not in self._order:
            self._order[key] = np.argsort(self.host ^ tm.mask(largest, signed), kind="stable").astype(np.uint32)
        rows = self._order[key][:min(k, self.n)]
        if not srt:
            rows = np.sort(rows)
        return self.host[rows], rows

    def run(self, k, largest=False, signed=False, srt=True, fill=FILLS[1], poison=None, ws=None):
        """one guarded call -> (keys, rows) as uint32 host arrays; the status word read, every guard looked at"""
        lib = _lib()
        n, m = self.n, min(k, self.n)
        w = Watch(fill)
        out_keys, out_rows = w.col(k), w.col(k)
        ws_bytes = lib.dbhip_topk_workspace_bytes(n, k)
        if ws is None:
            ws = w.ws(ws_bytes)
            if poison is not None:
                poison(ws)
        fn = lib.dbhip_topk_i32 if signed else lib.dbhip_topk_u32
        rc = fn(ptr(self.dev), n, k, int(largest), int(srt), ptr(out_keys), ptr(out_rows), ptr(ws), ws_bytes, _stream())
        assert rc == 0, rc
        assert _ops().workspace_status(ws) == 0
        w.check()
        self.watch.check()
        if k > m:  # behind entry m nothing is written
            assert bool((out_keys[m:] == i32(fill)).all()) and bool((out_rows[m:] == i32(fill)).all())
        return out_keys[:m].cpu().numpy().view(np.uint32), out_rows[:m].cpu().numpy().view(np.uint32)

    def check(self, k, largest=False, signed=False, srt=True, **kw):
        got_keys, got_rows = self.run(k, largest, signed, srt, **kw)
        want_keys, want_rows = self.want(k, largest, signed, srt)
        what = (self.n, k, largest, signed, srt)
        assert np.array_equal(got_rows, want_rows), what
        assert np.array_equal(got_keys, want_keys), what


# ---- every seam ------------------------------------------------------------------------------------------------------------
SEAM_N = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, C - 1, C, C + 1, 2 * C + 3, 100003, (1 << 20) + 777]
SEAM_K = [0, 1, 2, 63, 64, 65, 8191, 8192, 8193]


@pytest.mark.parametrize("n", SEAM_N)
def test_every_seam(n):
    """a wave, a tile, the one-tile sort, a segment, a chunk, ragged ends; every k of the list (and n - 1, n, n + 5) that
    is <= n + 5, all four orders, sorted both ways; k = n, smallest first: ops.radix_argsort_ as a second witness"""
    ops = _ops()
    col = Column(uniform(n, seed=n))
    ks = sorted({k for k in SEAM_K + [n - 1, n, n + 5] if 0 <= k <= n + 5})
    call = 0
    for k in ks:
        for largest, signed in ORDERS:
            for srt in (True, False):
                col.check(k, largest, signed, srt, fill=FILLS[call % 2])
                call += 1
    for signed in (False, True):
        keys = col.dev.clone()
        perm = ops.radix_argsort_(keys, signed=signed).cpu().numpy().view(np.uint32)
        got_keys, got_rows = col.run(n, False, signed, True)
        assert np.array_equal(got_rows, perm) and np.array_equal(got_keys, keys.cpu().numpy().view(np.uint32))


# ---- ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 0x80000000, 0xFFFFFFFF])
def test_all_keys_equal(value):
    n = 2 * C + 3
    col = Column(np.full(n, value, dtype=np.uint32))
    for k in (1, 2, 64, S, S + 1, C, C + 1, n - 1, n):
        for largest, signed in ORDERS:
            col.check(k, largest, signed, True)
            col.check(k, largest, signed, False)


def test_two_values_around_the_end_of_the_better_run():
    n = 100003
    rng = np.random.default_rng(5)
    low = rng.random(n) < 0.3
    for a, b in ((7, 9), (0x7FFFFFFF, 0x80000000), (0, 0xFFFFFFFF)):
        col = Column(np.where(low, np.uint32(a), np.uint32(b)))
        for largest, signed in ORDERS:
            better = int(((col.host ^ tm.mask(largest, signed)) == (col.host ^ tm.mask(largest, signed)).min()).sum())
            for k in (better // 2, better - 1, better, better + 1):  # inside the better run, its last row, one past it
                col.check(k, largest, signed, True)
                col.check(k, largest, signed, False)


@pytest.mark.parametrize("cut", [S, C])
def test_ties_across_a_cut(cut):
    """the threshold key on rows cut-2 .. cut+2, everything else worse: k = 1 .. 5 takes them in row order, across two
    waves' segments and across two workgroups' chunks"""
    n = 2 * C + 3
    for largest, signed in ORDERS:
        msk = tm.mask(largest, signed)
        host = (np.uint32(0x40000000) | (uniform(n, 3) >> np.uint32(4))) ^ msk  # worse than the threshold in this order
        host[cut - 2: cut + 3] = np.uint32(0x3FFFFFFF) ^ msk
        col = Column(host)
        for k in range(1, 7):
            for srt in (True, False):
                got_keys, got_rows = col.run(k, largest, signed, srt)
                if k <= 5:
                    assert got_rows.tolist() == list(range(cut - 2, cut - 2 + k)), (k, largest, signed, srt)
                want_keys, want_rows = col.want(k, largest, signed, srt)
                assert np.array_equal(got_rows, want_rows) and np.array_equal(got_keys, want_keys)


def test_about_105_rows_per_value():
    n = (1 << 20) + 777
    col = Column(np.uint32(1) + uniform(n, 9) % np.uint32(10000))
    for k in (1, 104, 105, 106, 1000):
        for largest, signed in ORDERS:
            col.check(k, largest, signed, True)
            col.check(k, largest, signed, False)


# ---- digits ------------------------------------------------------------------------------------------------------------------
def test_keys_that_differ_in_one_byte_only():
    n = 100003
    u = uniform(n, 11)
    for shift in (24, 0):  # the top byte, the bottom byte
        col = Column((np.uint32(0x00345600) if shift == 24 else np.uint32(0x12345600)) | ((u & np.uint32(0xFF)) << np.uint32(shift)))
        for k in (1, 390, 391, 5000, n):
            for largest, signed in ORDERS:
                col.check(k, largest, signed, True)
                col.check(k, largest, signed, False)


@pytest.mark.parametrize("below,above", [(0x00FFFFFF, 0x01000000), (0x0100FFFF, 0x01010000), (0x7FFFFFFF, 0x80000000)])
def test_thresholds_at_digit_boundaries(below, above):
    """`below` and `above` are neighbours whose difference carries through the lower digits; 1000 rows of each among rows
    spread far to both sides, k on either side of each run's ends"""
    n = 50021
    rng = np.random.default_rng(13)
    host = np.where(rng.random(n) < 0.5, np.uint32(below) - np.uint32(2) - (uniform(n, 14) % np.uint32(0x00F00000)),
                    np.uint32(above) + np.uint32(2) + (uniform(n, 15) % np.uint32(0x00F00000))).astype(np.uint32)
    rows = rng.permutation(n)
    host[rows[:1000]] = below
    host[rows[1000:2000]] = above
    col = Column(host)
    for largest, signed in ORDERS:
        x = np.sort(host ^ tm.mask(largest, signed))
        first = int(np.searchsorted(x, min(below ^ int(tm.mask(largest, signed)), above ^ int(tm.mask(largest, signed)))))
        for k in (first, first + 1, first + 999, first + 1000, first + 1001, first + 1999, first + 2000, first + 2001):
            col.check(k, largest, signed, True)
            col.check(k, largest, signed, False)


def test_signed_columns_with_the_ends_of_the_range():
    n = 70001
    host = uniform(n, 17)
    rows = np.random.default_rng(18).permutation(n)
    for j, v in enumerate((INT_MIN, 0xFFFFFFFF, 0, INT_MAX)):  # INT_MIN, -1, 0, INT_MAX: 50 rows each
        host[rows[50 * j: 50 * j + 50]] = v
    col = Column(host)
    for largest in (False, True):
        for k in (1, 49, 50, 51, 100, n // 2, n - 1, n):
            col.check(k, largest, True, True)
            col.check(k, largest, True, False)


# ---- where the selected rows lie ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_sorted_input(descending):
    """all of the answer in the first chunk, or in the last"""
    n = 4 * C + 1234
    host = np.sort(uniform(n, 19))
    col = Column(host[::-1] if descending else host)
    for k in (1, 1000, C + 5):
        for largest, signed in ((False, False), (True, False), (True, True)):
            col.check(k, largest, signed, True)
            col.check(k, largest, signed, False)


def test_ninety_percent_one_value():
    n = 4 * C + 1234
    rng = np.random.default_rng(21)
    col = Column(np.where(rng.random(n) < 0.9, np.uint32(0x80001234), uniform(n, 22)))
    for k in (1, 1000, n // 20, n // 2, n - 3):
        for largest, signed in ORDERS:
            col.check(k, largest, signed, True)
            col.check(k, largest, signed, False)


# ---- the other digit width -------------------------------------------------------------------------------------------------
WIDTH_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from dwarf_bench_amd import ops
from tests import topk_model as tm
n = 2 * ops.TOPK_CHUNK_ROWS + 3
u = np.random.default_rng(81).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
cols = {"uniform": u, "[1,10000]": np.uint32(1) + u % np.uint32(10000), "equal": np.full(n, 0x80000000, dtype=np.uint32),
        "low byte": np.uint32(0x7FFFFF00) | (u & np.uint32(0xFF)), "top bits": u & np.uint32(0xFFE00000)}
calls = 0
for name, host in cols.items():
    keys = torch.from_numpy(host.view(np.int32)).cuda()
    for k in (1, 1000, 8193, n // 2, n):
        for largest, signed in ((False, False), (True, True), (False, True), (True, False)):
            for srt in (True, False):
                got_keys, got_rows = ops.topk(keys, k, largest=largest, signed=signed, sorted=srt)
                want_keys, want_rows = tm.topk(host, k, largest, signed, sorted=srt)
                assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows), (name, k, largest, signed, srt)
                assert np.array_equal(got_keys.cpu().numpy().view(np.uint32), want_keys), (name, k, largest, signed, srt)
                calls += 1
print("agreed on", calls, "calls")
"""


@pytest.mark.parametrize("bits", ["8", "11"])
def test_both_digit_widths_in_a_process_of_their_own(bits):
    """the digit width of the select is fixed when a process makes its first call (DBHIP_TOPK_BITS, a knob for
    measurements): both widths, whichever is the default, over uniform and crowded columns and columns that differ only
    in the lowest or only in the highest digit"""
    import sys
    r = subprocess.run([sys.executable, "-c", WIDTH_CHILD, str(ROOT)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "DBHIP_TOPK_BITS": bits})
    assert r.returncode == 0 and "agreed on 200 calls" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- bounds and dirt ---------------------------------------------------------------------------------------------------------
def test_one_plan_three_inputs_and_a_dirty_workspace():
    """one guarded workspace for three inputs in a row, poisoned with zeros, 0xFF and random bytes in between; a status
    word left set by the call before is clean afterwards"""
    n, k = 2 * C + 3, 1000
    w = Watch(FILLS[0])
    ws = w.ws(_lib().dbhip_topk_workspace_bytes(n, k))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(99)
    inputs = [uniform(n, 31), np.uint32(1) + uniform(n, 32) % np.uint32(10000), np.full(n, 0xFFFFFFFF, dtype=np.uint32)]
    for round_, how in enumerate(("zeros", "0xff", "random", "status")):
        for j, host in enumerate(inputs):
            if how == "zeros":
                ws.zero_()
            elif how == "0xff":
                ws.fill_(0xFF)
            elif how == "random":
                ws.copy_(torch.randint(0, 256, ws.shape, dtype=torch.uint8, device="cuda", generator=gen))
            else:
                ws[:4] = torch.tensor([8, 0, 0, 0], dtype=torch.uint8, device="cuda")  # DBHIP_DEV_RANK_ORDER left behind
                assert _ops().workspace_status(ws) == 8
            largest, signed = ORDERS[(round_ + j) % 4]
            Column(host).check(k, largest, signed, j % 2 == 0, ws=ws)
    w.check()


def test_empty_calls_write_nothing_and_clean_the_status_word():
    lib = _lib()
    w = Watch(FILLS[1])
    keys, out_keys, out_rows = w.col(1000, data=uniform(1000, 41), freeze=True), w.col(16), w.col(16)
    ws = w.ws(lib.dbhip_topk_workspace_bytes(1000, 16))
    for n, k in ((1000, 0), (0, 16), (0, 0)):
        ws.fill_(0xFF)
        assert lib.dbhip_topk_u32(ptr(keys), n, k, 0, 1, ptr(out_keys), ptr(out_rows), ptr(ws), ws.numel(), _stream()) == 0
        assert _ops().workspace_status(ws) == 0
        assert bool((out_keys == i32(FILLS[1])).all()) and bool((out_rows == i32(FILLS[1])).all())
        w.check()


def test_the_tensor_api():
    ops = _ops()
    host = uniform(100003, 43)
    keys = torch.from_numpy(host.view(np.int32)).cuda()
    for largest, signed, srt in ((False, False, True), (True, True, True), (False, True, False)):
        got_keys, got_rows = ops.topk(keys, 777, largest=largest, signed=signed, sorted=srt)
        want_keys, want_rows = tm.topk(host, 777, largest, signed, sorted=srt)
        assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows)
        assert np.array_equal(got_keys.cpu().numpy().view(np.uint32), want_keys)
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), host)  # the column is read only
    assert [t.numel() for t in ops.topk(keys, 0)] == [0, 0] and [t.numel() for t in ops.topk(keys[:0], 5)] == [0, 0]
    assert ops.topk(keys, 200000)[1].numel() == 100003
    with pytest.raises(ValueError):
        ops.topk(keys[1:], 5)  # starts 4 bytes past a 16-byte boundary
    with pytest.raises(ValueError):
        ops.TopK(100003, 5).launch(keys[:100000])  # another size than the plan's
    with pytest.raises(ValueError):
        ops.topk(keys.to(torch.int64), 5)


# ---- the validator -----------------------------------------------------------------------------------------------------------
def _words(keys_dev, out_keys, out_rows, largest, signed):
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
    return _ops().check_topk(keys_dev, to(out_keys), to(out_rows), largest, signed)


def _mutations(host, ok, orow, at, rng):
    """the kinds of damage of tests/test_topk_model.py at entry `at` of the right table (ok, orow)"""
    n, m = host.size, orow.size
    if at + 1 < m:
        k2, r2 = ok.copy(), orow.copy()
        k2[[at, at + 1]], r2[[at, at + 1]] = ok[[at + 1, at]], orow[[at + 1, at]]
        yield "swapped", k2, r2
    same = np.flatnonzero(host == ok[at])
    for other in (same[same < orow[at]][-1:], same[same > orow[at]][:1]):
        if other.size:
            r2 = orow.copy()
            r2[at] = other[0]
            yield "tie replaced", ok, r2
    if m > 1:
        k2, r2 = ok.copy(), orow.copy()
        j = (at + 1) % m
        k2[at], r2[at] = ok[j], orow[j]
        yield "duplicated", k2, r2
    for row in (n, M32):
        r2 = orow.copy()
        r2[at] = row
        yield "row id out of range", ok, r2
    k2 = ok.copy()
    k2[at] ^= np.uint32(1 << int(rng.integers(0, 32)))
    yield "wrong key", k2, orow
    outside = np.setdiff1d(np.arange(n, dtype=np.uint32), orow)
    if outside.size:
        k2, r2 = ok.copy(), orow.copy()
        r2[-1] = outside[int(rng.integers(0, outside.size))]
        k2[-1] = host[r2[-1]]
        yield "last entry from outside the answer", k2, r2


@pytest.mark.parametrize("largest,signed", ORDERS)
def test_validator_words_equal_the_models(largest, signed):
    """right tables and every kind of damage at entries 0, 63 | 64, m-2 | m-1 and 16 random places; keys in [1, 300] so that
    every entry has ties on both sides"""
    rng = np.random.default_rng(51)
    n, k = 20011, 5000
    host = np.uint32(1) + uniform(n, 52) % np.uint32(300)
    if signed:
        host = host - np.uint32(150)  # both signs
    keys_dev = torch.from_numpy(host.view(np.int32)).cuda()
    ok, orow = tm.topk(host, k, largest, signed)
    words = _words(keys_dev, ok, orow, largest, signed)
    assert words == tm.check_words(host, ok, orow, largest, signed) == (0, k - 1)
    seen = set()
    for at in [0, 63, 64, k - 2, k - 1] + sorted(rng.integers(0, k, 16).tolist()):
        for what, k2, r2 in _mutations(host, ok, orow, at, rng):
            words = _words(keys_dev, k2, r2, largest, signed)
            assert words == tm.check_words(host, k2, r2, largest, signed), (what, at)
            assert not tm.verdict(words, k, n), (what, at, words)
            seen.add(what)
    assert len(seen) == 6, seen
    # the tables the device itself makes are accepted
    got_keys, got_rows = _ops().topk(keys_dev, k, largest=largest, signed=signed)
    assert _ops().check_topk(keys_dev, got_keys, got_rows, largest, signed) == (0, k - 1)


@pytest.mark.parametrize("label", ["0", "1", "2", "63", "64", "65", "255", "256", "257", "W-1", "W", "W+1", "W+257", "2W+3"])
def test_validator_at_the_grid_seams(label):
    """W = compute units * 8 * 256 threads in the capped grid: up to 2W + 3 rows the stride loop takes a second and third
    trip.  k = n: the table is the whole stable argsort; then k = n / 2 with one row id replaced"""
    from tests.test_gpu_validators import size_of
    w = _ops().device_info()[1] * 8 * 256
    n = size_of(label, w)
    host = uniform(n, 61) >> np.uint32(12)
    keys_dev = torch.from_numpy(host.view(np.int32)).cuda()
    for largest, signed in ((False, False), (True, True)):
        for k in sorted({n, n // 2, min(n, 1)}):
            ok, orow = tm.topk(host, k, largest, signed)
            words = _words(keys_dev, ok, orow, largest, signed)
            assert words == tm.check_words(host, ok, orow, largest, signed) and tm.verdict(words, k, n), (k, words)
            if k:
                r2 = orow.copy()
                r2[k // 2] = (int(r2[k // 2]) + 1) % max(n, 2)
                words = _words(keys_dev, ok, r2, largest, signed)
                assert words == tm.check_words(host, ok, r2, largest, signed) and not tm.verdict(words, k, n), (k, words)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def _cli(size, iterations, env=None):
    return subprocess.run([str(CLI), "TopKHip", "--device=hip", f"--input_size={size}", f"--iterations={iterations}"],
                          capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


DEVICE_CHECK = {"DWARF_BENCH_VALIDATE_MAX": "1"}  # above one row the dwarf asks dbhip_check_topk_u32
SIZES = [(1024, 9), (1 << 24, 3)]


@pytest.mark.parametrize("env", [{}, DEVICE_CHECK, {"DWARF_BENCH_TOPK_LARGEST": "1"}, {"DWARF_BENCH_TOPK_K": "1"},
                                 {"DWARF_BENCH_TOPK_K": "n"}, {"DWARF_BENCH_TOPK_K": "n", **DEVICE_CHECK},
                                 {"DWARF_BENCH_TOPK_LARGEST": "1", **DEVICE_CHECK}], ids=lambda e: "+".join(e) or "default")
@pytest.mark.parametrize("size,iterations", SIZES)
def test_cli_results_are_valid(size, iterations, env):
    env = {name: str(size) if value == "n" else value for name, value in env.items()}
    r = _cli(size, iterations, env)
    assert r.returncode == 0, r.stderr
    assert "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == iterations


@pytest.mark.parametrize("env", [{}, DEVICE_CHECK], ids=["host check", "device check"])
@pytest.mark.parametrize("size,iterations", SIZES)
def test_cli_fault_injection_flips_valid(size, iterations, env):
    r = _cli(size, iterations, {**env, "DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ncorrect results") == iterations and "Caught exception" not in r.stderr, r.stderr


def test_sixteen_million_rows():
    n, k = (1 << 24) + 5, 1000
    host = uniform(n, 71)
    keys = torch.from_numpy(host.view(np.int32)).cuda()
    want_keys, want_rows = tm.topk(host, k)
    got_keys, got_rows = _ops().topk(keys, k)
    assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows)
    assert np.array_equal(got_keys.cpu().numpy().view(np.uint32), want_keys)
    assert _ops().check_topk(keys, got_keys, got_rows) == (0, k - 1)
