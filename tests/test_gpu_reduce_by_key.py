"""dbhip_reduce_by_key_u32 (include/dbhip_reduce_by_key.h) on the GPU against numpy (tests/reduce_by_key_model.py: heads =
flatnonzero(r_[True, k[1:] != k[:-1]]), add / minimum / maximum.reduceat, diff for the counts); everything is compared
with array_equal.  Every call runs on guarded buffers (tests/guard_testlib.py): both input columns frozen, output columns
of exactly `capacity` entries whose untouched entries must keep the guard word, a workspace of exactly the queried size,
poisoned before the call, the status word read after it.

S = ops.REDUCE_BY_KEY_SEGMENT_ROWS is one wave's rows in the count and reduce kernels, C = ops.REDUCE_BY_KEY_CHUNK_ROWS one
workgroup's."""
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import reduce_by_key_model as rm
from tests.guard_testlib import FILLS, Watch, i32, i64, ptr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_groupby_sorted"
C, S = 32768, 4096
TABLE_FULL = 4
NAMES = ("keys", "counts", "sums", "mins", "maxs")
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
    assert (_ops().REDUCE_BY_KEY_CHUNK_ROWS, _ops().REDUCE_BY_KEY_SEGMENT_ROWS) == (C, S)


# ---- columns -------------------------------------------------------------------------------------------------------------
def uniform(n, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def run_keys(n, mean, seed, distinct=True):
    """random run lengths with the given mean; distinct: every run its own key (in no order), otherwise the run number
    mod 7: grouped but unsorted, the same key in runs that are not neighbours"""
    rng = np.random.default_rng(seed)
    run = np.cumsum(rng.random(n) < 1.0 / mean, dtype=np.uint64)
    if not distinct:
        return (run % np.uint64(7)).astype(np.uint32)
    return ((run * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def key_shapes(n, seed):
    yield "all distinct", (np.random.default_rng(seed).permutation(n).astype(np.uint32) + np.uint32(17))
    yield "all equal", np.full(n, 0xDEADBEEF, dtype=np.uint32)
    for mean in (1.5, 40, 5000):
        yield f"runs of mean {mean}", run_keys(n, mean, seed + int(mean))
    yield "grouped but unsorted", run_keys(n, 3, seed + 3, distinct=False)


class Table:
    """what one guarded call returned: the written entries of the columns that were passed, R, and the status word"""

    def __init__(self, cols, runs, status):
        self.cols, self.runs, self.status = cols, runs, status


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
            self._want[signed] = dict(zip(NAMES, rm.reduce_by_key(self.keys, self.vals, signed)))
        return self._want[signed]

    @property
    def runs(self):
        return self.want(False)["keys"].size

    def call(self, signed=False, capacity=None, cols=NAMES, fill=FILLS[1], poison=0xA5, ws=None, with_vals=True):
        """one guarded call; capacity None: R.  Checks every guard, the untouched entries and *out_runs."""
        lib = _lib()
        n, R = self.n, self.runs
        cap = R if capacity is None else capacity
        w = Watch(fill)
        out = {name: (w.u64(cap) if name == "sums" else w.col(cap)) for name in cols} if cap else {}
        runs = w.u64(1)
        ws_bytes = lib.dbhip_reduce_by_key_workspace_bytes(n)
        if ws is None:
            ws = w.ws(ws_bytes)
            ws.fill_(poison)
        args = [ptr(out[name]) if name in out else None for name in NAMES]
        rc = lib.dbhip_reduce_by_key_u32(ptr(self.dkeys), ptr(self.dvals) if with_vals else None, n, int(signed), *args, cap,
                                         ptr(runs), ptr(ws), ws_bytes, _stream())
        assert rc == 0, rc
        status = _ops().workspace_status(ws)
        w.check()
        self.watch.check()
        assert int(runs.item()) == R, (int(runs.item()), R)
        written = min(R, cap)
        got = {}
        for name, t in out.items():
            guard = i64(fill) if name == "sums" else i32(fill)
            assert bool((t[written:] == guard).all()), f"{name}: entries behind run {written} were written"
            host = t[:written].cpu().numpy()
            got[name] = host.view(np.uint64) if name == "sums" else host.view(np.uint32)
        return Table(got, int(runs.item()), status)

    def check(self, signed=False, capacity=None, cols=NAMES, want_status=None, **kw):
        t = self.call(signed, capacity, cols, **kw)
        R = self.runs
        cap = R if capacity is None else capacity
        full = cap < R and cap > 0
        assert t.status == (TABLE_FULL if full else 0) if want_status is None else t.status == want_status, t.status
        want = self.want(signed)
        for name in (cols if cap else ()):
            assert np.array_equal(t.cols[name], want[name][:cap]), (name, self.n, signed, cap)
        return t


# ---- every size, every key shape -------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C + 3, 100003, (1 << 20) + 777]


@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_key_shape(n):
    vals = uniform(n, seed=n + 1)
    call = 0
    for what, keys in key_shapes(n, seed=n):
        inp = Input(keys, vals, fill=FILLS[call % 2])
        for signed in (False, True):
            inp.check(signed, fill=FILLS[(call + 1) % 2], poison=(0xFF, 0x00, 0xA5)[call % 3])
            call += 1


# ---- built seams -------------------------------------------------------------------------------------------------------------
def _seams(unit):
    n = 4 * unit + 37
    base = np.random.default_rng(unit).permutation(n).astype(np.uint32)  # every row its own run
    equal = np.full(n, 5, dtype=np.uint32)

    def over(background, *ranges):
        keys = background.copy()
        for j, (lo, hi) in enumerate(ranges):  # rows lo .. hi inclusive, a key no other row has
            keys[lo:hi + 1] = 0xF0000000 + j
        return keys
    yield "a run ends at the last row of a unit, the next starts at its first", over(base, (unit - 10, unit - 1), (unit, unit + 5))
    yield "a run of the two rows around the cut", over(base, (unit - 1, unit))
    yield "a run that is exactly units 1 and 2", over(base, (unit, 3 * unit - 1))
    yield "the same among equal keys", over(equal, (unit, 3 * unit - 1))
    yield "a run from the middle of unit 0 to the middle of unit 3", over(base, (unit // 2, 3 * unit + unit // 2))
    yield "the same among equal keys", over(equal, (unit // 2, 3 * unit + unit // 2))
    yield "runs of one row at both ends", over(equal, (0, 0), (n - 1, n - 1))
    yield "runs of one row at both ends of distinct rows", over(base, (0, 0), (n - 1, n - 1))


@pytest.mark.parametrize("unit", [S, C])
def test_runs_built_across_the_cuts(unit):
    vals = uniform(4 * unit + 37, seed=unit + 9)
    for i, (what, keys) in enumerate(_seams(unit)):
        inp = Input(keys, vals)
        for signed in (False, True):
            inp.check(signed, fill=FILLS[i % 2])


# ---- values --------------------------------------------------------------------------------------------------------------------
def test_values_whose_sums_pass_32_bits_and_the_ends_of_the_signed_range():
    n = 100003
    rng = np.random.default_rng(21)
    ones = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    ends = np.array([INT_MIN, INT_MAX, 0xFFFFFFFF, 0, INT_MIN, 1], dtype=np.uint32)[rng.integers(0, 6, n)]
    negative = (np.uint32(0x80000000) | (uniform(n, 22) >> np.uint32(1)))  # every value below zero as int32
    for keys in (run_keys(n, 40, 23), run_keys(n, 5000, 24), np.full(n, 1, dtype=np.uint32)):
        for vals in (ones, ends, negative):
            inp = Input(keys, vals)
            for signed in (False, True):
                inp.check(signed)
    want = Input(np.full(n, 1, dtype=np.uint32), ones).want(False)
    assert int(want["sums"][0]) == n * 0xFFFFFFFF > 1 << 32  # the shape does what its name says
    assert Input(run_keys(n, 40, 23), negative).want(True)["sums"].view(np.int64).max() < 0


# ---- more segments than the stitch workgroup has threads ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one run", "all distinct", "runs of mean 40"])
def test_a_thread_of_the_scans_owns_several_segments(shape):
    n = 3 * (1 << 22) + 12345
    assert (n + S - 1) // S > 2 * 1024
    keys = {"one run": lambda: np.full(n, 77, dtype=np.uint32),
            "all distinct": lambda: np.arange(n, dtype=np.uint32) * np.uint32(2654435761),
            "runs of mean 40": lambda: run_keys(n, 40, 31)}[shape]()
    inp = Input(keys, uniform(n, 32))
    inp.check(signed=shape != "all distinct")


# ---- optional columns, capacity, workspace -------------------------------------------------------------------------------------
def test_optional_columns():
    n = 2 * C + 3
    inp = Input(run_keys(n, 40, 41), uniform(n, 42))
    for signed in (False, True):
        for name in NAMES:
            inp.check(signed, cols=(name,))
            inp.check(signed, cols=tuple(x for x in NAMES if x != name))
    for cols in (("counts",), ("keys", "counts"), ("keys",)):  # DISTINCT with counts: no value column at all
        inp.check(cols=cols, with_vals=False)


@pytest.mark.parametrize("mean", [1.5, 40, 5000])
def test_capacity(mean):
    n = 100003
    inp = Input(run_keys(n, mean, 51), uniform(n, 52))
    R = inp.runs
    assert R > 6
    for cap in (R, R + 5, R - 1, 1):
        for signed in (False, True):
            t = inp.check(signed, capacity=cap)
            assert t.runs == R and t.status == (TABLE_FULL if cap < R else 0)
    t = inp.check(capacity=0)  # the count-only call never raises the flag
    assert t.runs == R and t.status == 0 and t.cols == {}


def test_two_calls_on_one_workspace_and_poisoned_workspaces():
    n = 2 * C + 3
    a = Input(run_keys(n, 40, 61), uniform(n, 62))
    b = Input(np.full(n, 9, dtype=np.uint32), uniform(n, 63))
    w = Watch(FILLS[0])
    ws = w.ws(_lib().dbhip_reduce_by_key_workspace_bytes(n))
    for poison in (0xFF, 0x00):
        ws.fill_(poison)
        for inp in (a, b, a, a):
            inp.check(ws=ws)
            inp.check(signed=True, capacity=1, ws=ws)  # leaves TABLE_FULL behind (a), or not (b)
            inp.check(ws=ws)
        w.check()


# ---- the front door ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,groups", [(100003, 1 << 32), (100003, 1000), ((1 << 20) + 777, 10000)])
def test_groupby_sorted_against_numpy_and_the_hash_groupby(n, groups):
    ops = _ops()
    rng = np.random.default_rng(n + groups % 1000)
    keys = rng.integers(0, groups, n, dtype=np.uint64).astype(np.uint32)
    if groups < 1 << 32:
        keys = keys * np.uint32(2654435761)  # crowded, all over the range
    vals = uniform(n, 71)
    dk, dv = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    for signed, signed_keys in ((False, False), (True, False), (False, True), (True, True)):
        order = np.argsort(keys.view(np.int32) if signed_keys else keys, kind="stable")
        want = rm.reduce_by_key(keys[order], vals[order], signed)
        got = ops.groupby_sorted(dk, dv, signed=signed, signed_keys=signed_keys)
        assert got[2].dtype == torch.int64
        for name, g, w in zip(NAMES, got, want):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.uint64) if name == "sums" else g.view(np.uint32), w), (name, signed, signed_keys)
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys) and np.array_equal(dv.cpu().numpy().view(np.uint32), vals)
    # a second witness: the hash group-by's wrapping sums and counts, its rows sorted by key
    got = [t.cpu().numpy() for t in ops.groupby_sorted(dk, dv)]
    hk, hs, hc = (t.cpu().numpy().view(np.uint32) for t in ops.groupby_hash(dk, dv))
    order = np.argsort(hk, kind="stable")
    assert np.array_equal(got[0].view(np.uint32), hk[order]) and np.array_equal(got[1].view(np.uint32), hc[order])
    assert np.array_equal((got[2].view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32), hs[order])


def test_reduce_by_key_front_door_and_its_validator():
    ops = _ops()
    n = 100003
    keys, vals = run_keys(n, 40, 81), uniform(n, 82)
    dk, dv = torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    for signed in (False, True):
        got = ops.reduce_by_key(dk, dv, signed=signed)
        for name, g, w in zip(NAMES, got, rm.reduce_by_key(keys, vals, signed)):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.uint64) if name == "sums" else g.view(np.uint32), w), (name, signed)
        words = ops.check_reduce_by_key(dk, dv, *got, signed=signed)
        assert rm.verdict(words) and words == rm.check_words(keys, vals, *(g.cpu().numpy() for g in got), signed)
    with pytest.raises(Exception):
        ops.reduce_by_key(dk, dv, capacity=3)  # DBHIP_DEV_TABLE_FULL


def _cli(env=None):
    import os
    return subprocess.run([str(CLI), "GroupBySortedHip", "--device=hip", "--input_size=100003", "--groups_count=1000",
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
