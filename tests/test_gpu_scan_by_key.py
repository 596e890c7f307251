"""dbhip_scan_by_key_u32 and its validator (include/dbhip_scan_by_key.h) on the GPU against numpy
(tests/scan_by_key_model.py); everything is compared with array_equal.  Every call runs on guarded buffers
(tests/guard_testlib.py): both input columns frozen, output columns of exactly n entries, a workspace of exactly the queried
size, poisoned before the call, the status word read after it, and every guard looked at after every call.

S = ops.SCAN_BY_KEY_SEGMENT_ROWS is one wave's rows in the two streaming kernels, C = ops.SCAN_BY_KEY_CHUNK_ROWS one
workgroup's."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import graph_testlib as gl
from tests import reduce_by_key_model as rm
from tests import scan_by_key_model as sm
from tests.guard_testlib import FILLS, Watch, ptr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_window"
C, S = 32768, 4096
NAMES = sm.NAMES
M64 = (1 << 64) - 1
INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_the_tests_know_the_segment_and_chunk_size():
    assert (_ops().SCAN_BY_KEY_CHUNK_ROWS, _ops().SCAN_BY_KEY_SEGMENT_ROWS) == (C, S)
    assert _ops().SCAN_BY_KEY_COLUMNS == NAMES


# ---- columns -------------------------------------------------------------------------------------------------------------
def uniform(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def run_keys(n, mean, seed):
    """random run lengths with the given mean, every run its own key (in no order)"""
    run = np.cumsum(np.random.default_rng(seed).random(n) < 1.0 / mean, dtype=np.uint64)
    return ((run * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def heads_at(n, rows):
    """keys whose heads are row 0 and `rows`"""
    flags = np.zeros(n, dtype=bool)
    flags[[r for r in rows if 0 < r < n]] = True
    flags[0] = True
    return np.cumsum(flags).astype(np.uint32) * np.uint32(40503)


def key_shapes(n, seed):
    yield "one run", np.full(n, 0xDEADBEEF, dtype=np.uint32)
    yield "all distinct", np.random.default_rng(seed).permutation(n).astype(np.uint32) + np.uint32(17)
    for mean in (1.5, 40, 5000):
        yield f"runs of mean {mean}", run_keys(n, mean, seed + int(mean))
    # A A B A: the run number mod 2, the same key in runs that are not neighbours
    yield "a key that returns", (np.cumsum(np.random.default_rng(seed + 3).random(n) < 1 / 3.0) % 2).astype(np.uint32)
    between = np.arange(n, dtype=np.uint32) + np.uint32(100)
    between[n // 5: n - n // 5] = 7
    yield "one long run between distinct rows", between


class Input:
    """two frozen, guarded columns on the device and the model's answer under both signednesses (computed once)"""

    def __init__(self, keys, vals, fill=FILLS[0]):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint32)
        self.vals = np.ascontiguousarray(vals, dtype=np.uint32)
        self.n = self.keys.size
        self.watch = Watch(fill)
        self.dkeys = self.watch.col(self.n, data=self.keys, freeze=True)
        self.dvals = self.watch.col(self.n, data=self.vals, freeze=True)
        self._want = {}

    def want(self, signed):
        if signed not in self._want:
            self._want[signed] = dict(zip(NAMES, sm.scan_by_key(self.keys, self.vals, signed)))
        return self._want[signed]

    def call(self, signed=False, cols=NAMES, fill=FILLS[1], poison="0xff", ws=None, with_vals=True):
        """one guarded call -> {column: host array}; checks every guard, both inputs and the status word"""
        lib = _lib()
        n = self.n
        w = Watch(fill)
        out = {name: (w.u64(n) if name == "sums" else w.col(n)) for name in cols}
        ws_bytes = lib.dbhip_scan_by_key_workspace_bytes(n)
        if ws is None:
            ws = w.ws(ws_bytes)
            gl.poison(ws, poison)
        args = [ptr(out[name]) if name in out else None for name in NAMES]
        rc = lib.dbhip_scan_by_key_u32(ptr(self.dkeys), ptr(self.dvals) if with_vals else None, n, int(signed), *args,
                                       ptr(ws), ws_bytes, _stream())
        assert rc == 0, rc
        assert _ops().workspace_status(ws) == 0
        w.check()
        self.watch.check()
        return {name: (t.cpu().numpy().view(np.uint64) if name == "sums" else t.cpu().numpy().view(np.uint32))
                for name, t in out.items()}

    def check(self, signed=False, cols=NAMES, what="", **kw):
        got = self.call(signed, cols, **kw)
        want = self.want(signed)
        for name in cols:
            bad = np.flatnonzero(got[name] != want[name])
            assert bad.size == 0, (f"{what}: {name} (n = {self.n}, signed = {signed}): {bad.size} rows differ, the first at "
                                   f"{bad[:1]}: got {got[name][bad[:1]]}, expected {want[name][bad[:1]]}")
        return got


# ---- every size, every key shape -------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C + 3, 100003, (1 << 20) + 777]


@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_key_shape(n):
    vals = uniform(n, seed=n + 1)
    call = 0
    for what, keys in key_shapes(n, seed=n):
        inp = Input(keys, vals, fill=FILLS[call % 2])
        for signed in (False, True):
            inp.check(signed, what=what, fill=FILLS[(call + 1) % 2], poison=gl.POISONS[call % 3])
            call += 1


# ---- built seams -------------------------------------------------------------------------------------------------------------
def test_heads_at_and_around_every_cut():
    n = 2 * C + S + 37
    vals = uniform(n, 3)
    cuts = (S - 1, S, S + 1, C - 1, C, C + 1)
    cases = [(f"one head at row {p}", heads_at(n, [p])) for p in cuts]
    cases.append(("heads at all of them", heads_at(n, cuts)))
    for p in (S, C):  # a run that ends exactly at a cut, among distinct rows
        keys = np.arange(n, dtype=np.uint32) + np.uint32(9)
        keys[p - 700: p] = 3
        cases.append((f"a run that ends in front of row {p}", keys))
        keys = keys.copy()
        keys[p: p + 300] = 4
        cases.append((f"and the next one starts there ({p})", keys))
    for i, (what, keys) in enumerate(cases):
        inp = Input(keys, vals, fill=FILLS[i % 2])
        for signed in (False, True):
            inp.check(signed, what=what)


def test_runs_over_several_segments_and_where_their_extremes_lie():
    n = 2 * C + 37
    rng = np.random.default_rng(4)
    lo, hi = S + S // 2, C + 2 * S + S // 3  # a run over more than three segments and over the chunk cut
    for background in ("distinct", "equal"):
        keys = (np.arange(n, dtype=np.uint32) + np.uint32(50)) if background == "distinct" else np.full(n, 5, dtype=np.uint32)
        keys[lo: hi + 1] = 0xF0000000
        last_seg = (hi // S) * S  # the run's last segment starts here
        for small_first in (True, False):
            vals = rng.integers(1000, 2000, n).astype(np.uint32)
            early, late = lo + 10, last_seg + 20
            small, big = 7, 0x7FFFFFF0  # the extremes under both signednesses
            vals[early if small_first else late] = small
            vals[late if small_first else early] = big
            inp = Input(keys, vals)
            for signed in (False, True):
                got = inp.check(signed, what=f"{background}, small first = {small_first}")
                # at the run's last row one extreme comes from an earlier segment's carry, the other from this segment
                assert got["mins"][hi] == small and got["maxs"][hi] == big and got["row_numbers"][hi] == hi - lo + 1
                assert (got["mins"][late - 1] == small) == small_first and (got["maxs"][late - 1] == big) == (not small_first)


# ---- values --------------------------------------------------------------------------------------------------------------------
def test_values_whose_sums_pass_32_bits_and_the_ends_of_the_signed_range():
    n = 3 * S + 11
    rng = np.random.default_rng(21)
    ones = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    ends = np.array([INT_MIN, INT_MAX, 0xFFFFFFFF, 0, INT_MIN, 1], dtype=np.uint32)[rng.integers(0, 6, n)]
    waves = np.tile(np.array([5, 0xFFFFFFF6, 0xFFFFFFFD, 40], dtype=np.uint32), n // 4 + 1)[:n]  # 5, -10, -3, 40
    crossing = heads_at(n, [S - 2, 2 * S + 5])  # a run from row S - 2 over all of segment 1 into segment 2
    for keys in (crossing, run_keys(n, 40, 23), np.full(n, 1, dtype=np.uint32)):
        for vals in (ones, ends, waves):
            inp = Input(keys, vals)
            for signed in (False, True):
                inp.check(signed)
    want = Input(crossing, ones).want(False)
    assert int(want["sums"][S - 1]) == 2 * 0xFFFFFFFF > 1 << 32 and int(want["sums"][2 * S + 4]) == (S + 7) * 0xFFFFFFFF
    signed_sums = Input(crossing, waves).want(True)["sums"].view(np.int64)
    assert signed_sums[1] < 0 < signed_sums[3]  # go negative and come back


# ---- more records than the carry workgroup has threads -------------------------------------------------------------------------
CARRY_N = 2 * 1024 * S + S + 1
CARRY_SHAPES = {"one run": lambda n: np.full(n, 77, dtype=np.uint32),
                "all distinct": lambda n: np.arange(n, dtype=np.uint32) * np.uint32(2654435761),
                "runs of mean 40": lambda n: run_keys(n, 40, 31),
                "runs of mean 3 S": lambda n: run_keys(n, 3 * S, 33)}


def _carry_blocks(keys):
    """per block of ceil(segments / 1024) consecutive segments (one thread's records in the carry kernel): the heads of its
    segments, as a list of arrays"""
    segments = (keys.size + S - 1) // S
    per = (segments + 1023) // 1024
    flags = np.zeros(segments * S, dtype=bool)
    flags[:keys.size] = sm.head_flags(keys)
    per_segment = flags.reshape(segments, S).sum(axis=1)
    return [per_segment[i: i + per] for i in range(0, segments, per)], flags


def test_the_carry_shapes_cover_every_kind_of_block():
    """over the shapes below: a block without a head, a block whose segments all have heads, and a block boundary inside a
    run — with more than one record per thread"""
    assert (CARRY_N + S - 1) // S > 2 * 1024
    seen = set()
    for name, make in CARRY_SHAPES.items():
        blocks, flags = _carry_blocks(make(CARRY_N))
        assert len(blocks[0]) == 3
        seen |= {"no head" for b in blocks[1:] if b.sum() == 0}
        seen |= {"all heads" for b in blocks if (b > 0).all()}
        seen |= {"boundary inside a run" for i in range(1, len(blocks)) if not flags[i * 3 * S]}
    assert seen == {"no head", "all heads", "boundary inside a run"}


@pytest.mark.parametrize("shape", list(CARRY_SHAPES))
def test_a_thread_of_the_carry_kernel_owns_several_records(shape):
    n = CARRY_N
    inp = Input(CARRY_SHAPES[shape](n), uniform(n, 32))
    inp.check(signed=shape in ("one run", "runs of mean 3 S"), what=shape)


# ---- optional columns, workspace -------------------------------------------------------------------------------------------------
def test_optional_columns():
    n = 2 * C + 3
    inp = Input(run_keys(n, 40, 41), uniform(n, 42))
    for signed in (False, True):
        for name in NAMES:
            inp.check(signed, cols=(name,))
        inp.check(signed, cols=NAMES)
    for cols in (("run_ids", "row_numbers"), ("run_ids",), ("row_numbers",)):  # no value column at all
        inp.check(cols=cols, with_vals=False)
        inp.check(cols=cols, with_vals=True)


def test_two_calls_on_one_workspace_and_poisoned_workspaces():
    n = 2 * C + 3
    a = Input(run_keys(n, 40, 61), uniform(n, 62))
    b = Input(np.full(n, 9, dtype=np.uint32), uniform(n, 63))
    w = Watch(FILLS[0])
    ws = w.ws(_lib().dbhip_scan_by_key_workspace_bytes(n))
    for poison in gl.POISONS:
        gl.poison(ws, poison)
        for inp in (a, b, a, a):
            inp.check(ws=ws)
            inp.check(signed=True, ws=ws)
        w.check()


def test_an_empty_call_clears_the_status_word_and_writes_nothing():
    lib = _lib()
    w = Watch(FILLS[0])
    ws = w.ws(256)
    ws.fill_(0xFF)
    cols = [w.col(0) for _ in range(2)] + [w.u64(0)] + [w.col(0) for _ in range(2)]
    keys, vals = w.col(0), w.col(0)
    assert lib.dbhip_scan_by_key_u32(ptr(keys), ptr(vals), 0, 0, *(ptr(c) for c in cols), ptr(ws), 256, _stream()) == 0
    assert _ops().workspace_status(ws) == 0
    w.check()
    assert lib.dbhip_scan_by_key_u32(None, None, 0, 0, None, None, None, None, None, None, 0, _stream()) == 0


# ---- the validator -----------------------------------------------------------------------------------------------------------
def _check_words(inp, table, signed, cols=NAMES, fill=FILLS[0]):
    """one guarded validator call on device copies of `table` -> the four words"""
    lib = _lib()
    w = Watch(fill)
    dev = {}
    for name in cols:
        dev[name] = w.u64(inp.n) if name == "sums" else w.col(inp.n)
        dev[name].copy_(torch.from_numpy(np.ascontiguousarray(table[name]).view(np.int64 if name == "sums" else np.int32)))
        w.freeze(dev[name])
    res = w.u64(4)
    ws = w.ws(lib.dbhip_check_scan_by_key_workspace_bytes(inp.n))
    ws.fill_(0xA5)
    rc = lib.dbhip_check_scan_by_key_u32(ptr(inp.dkeys), ptr(inp.dvals), inp.n, int(signed),
                                         *(ptr(dev[name]) if name in dev else None for name in NAMES), ptr(res), ptr(ws),
                                         ws.numel(), _stream())
    assert rc == 0, rc
    assert _ops().workspace_status(ws) == 0
    w.check()
    inp.watch.check()
    return tuple(int(x) & M64 for x in res.cpu().tolist())


@pytest.mark.parametrize("signed", [False, True])
def test_validator_accepts_right_tables_and_counts_what_a_poked_word_breaks(signed):
    n = 2 * C + 3
    inp = Input(run_keys(n, 40, 91), uniform(n, 92))
    right = inp.want(signed)
    flags = sm.head_flags(inp.keys)
    heads = int(flags.sum())
    assert _check_words(inp, right, signed) == (0, M64, heads, 0)
    for name in NAMES:  # every column alone
        assert _check_words(inp, right, signed, cols=(name,)) == (0, M64, heads, 0)
    a_head = int(np.flatnonzero(flags)[heads // 2])
    inside = int(np.flatnonzero(~flags)[n // 3])
    assert not flags[inside] and flags[a_head]
    rows = (0, a_head, inside, S - 1, S, C, n - 1)  # row 0, a head, a non-head, rows at the seams, the last row
    for i, name in enumerate(NAMES):
        for row in rows:
            table = {k: v.copy() for k, v in right.items()}
            table[name][row] ^= table[name].dtype.type(1 << (row % 31))
            words = _check_words(inp, table, signed, fill=FILLS[(i + row) % 2])
            assert words == sm.check_words(inp.keys, inp.vals, *(table[k] for k in NAMES), signed=signed), (name, row)
            assert words[0] in (1, 2) and words[1] == row and words[2] == heads, (name, row, words)
    # a table of the other signedness, and garbage: the model's words, and nothing read out of bounds (the guards)
    other = inp.want(not signed)
    junk = {name: (uniform(2 * n, 5).view(np.uint64) if name == "sums" else uniform(n, 6 + i)) for i, name in enumerate(NAMES)}
    for table in (other, junk):
        words = _check_words(inp, table, signed)
        assert words == sm.check_words(inp.keys, inp.vals, *(table[k] for k in NAMES), signed=signed) and words[0] > 0


# ---- the front door ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,groups", [(100003, 1000), ((1 << 20) + 777, 10000)])
def test_window_sorted_against_numpy_and_the_sorted_groupby(n, groups):
    ops = _ops()
    rng = np.random.default_rng(n + groups)
    keys = rng.integers(0, groups, n, dtype=np.uint64).astype(np.uint32) * np.uint32(2654435761)  # all over the range
    vals = uniform(n, 71)
    dk, dv = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    for signed, signed_keys in ((False, False), (True, False), (False, True), (True, True)):
        order = np.argsort(keys.view(np.int32) if signed_keys else keys, kind="stable")
        want = (keys[order], order.astype(np.uint32)) + sm.scan_by_key(keys[order], vals[order], signed)
        got = ops.window_sorted(dk, dv, signed=signed, signed_keys=signed_keys)
        assert len(got) == 7 and got[4].dtype == torch.int64
        for name, g, w in zip(("sorted_keys", "row_ids") + NAMES, got, want):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.uint64) if name == "sums" else g.view(np.uint32), w), (name, signed, signed_keys)
        # run_ids index the rows of the sort-based group-by of the same input
        gk, gc, gs, gmn, gmx = ops.groupby_sorted(dk, dv, signed=signed, signed_keys=signed_keys)
        run = got[2].long()
        assert int(run.max()) + 1 == gk.numel() and torch.equal(gk[run], got[0])
        closes = got[3] == gc[run]  # the last row of every run carries the run's totals
        assert int(closes.sum()) == gk.numel()
        for mine, theirs in ((got[4], gs), (got[5], gmn), (got[6], gmx)):
            assert torch.equal(mine[closes], theirs)
        words = ops.check_scan_by_key(got[0], dv[got[1].long()], *got[2:], signed=signed)
        assert sm.verdict(words, keys[order]), words
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys) and np.array_equal(dv.cpu().numpy().view(np.uint32), vals)


def test_scan_by_key_front_door():
    ops = _ops()
    n = 100003
    keys, vals = run_keys(n, 40, 81), uniform(n, 82)
    dk, dv = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    for signed in (False, True):
        got = ops.scan_by_key(dk, dv, signed=signed)
        for name, g, w in zip(NAMES, got, sm.scan_by_key(keys, vals, signed)):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.uint64) if name == "sums" else g.view(np.uint32), w), (name, signed)
        assert sm.verdict(ops.check_scan_by_key(dk, dv, *got, signed=signed), keys)
    got = ops.scan_by_key(dk, None)
    assert got[2:] == (None, None, None) and np.array_equal(got[0].cpu().numpy().view(np.uint32),
                                                            sm.scan_by_key(keys, vals)[0])
    assert sm.verdict(ops.check_scan_by_key(dk, None, got[0], got[1]), keys)
    # the run numbers are the rows of reduce_by_key's table
    table = rm.reduce_by_key(keys, vals)
    assert np.array_equal(table[0][got[0].cpu().numpy().view(np.uint32)], keys)


def _cli(env=None):
    return subprocess.run([str(CLI), "WindowSortedHip", "--device=hip", "--input_size=100003", "--groups_count=1000",
                           "--iterations=3"], capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})


def test_cli_reports_a_valid_result():
    r = _cli()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 3


def test_cli_fault_injection_flips_valid():
    r = _cli({"DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ncorrect results") == 3 and "Caught exception" not in r.stderr, r.stderr
