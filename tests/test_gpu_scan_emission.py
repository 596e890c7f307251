"""The match emission of the two-launch scan (scan_chunk_kernel: count_wave_matches / emit_wave_matches / chunk_step of
csrc/scan.hip) on inputs built to sit on its boundaries, through dbhip_copy_if_lt_i32.

Geometry the patterns are built on: a workgroup tile is 32768 elements, a wave of it 2048 contiguous elements, a row of
the wave 256 (one 16-byte load per lane), a lane's share of a row 4 components.  Element i of a tile belongs to
wave i // 2048, row (i % 2048) // 256, lane (i % 256) // 4, component i % 4.

Every case is compared with numpy (src[src < f]) and with oracle.pyoracle.copy_if_lt, runs once on a 16-byte aligned
source and once on the same values offset by one element (the bounds-checked kernel), and checks what the call may write:
`out` carries 64 guard elements behind n and is pre-filled with a sentinel; out[m:] must still hold it after the call (one
store per match and nothing else).  Matching elements are distinct negative numbers (filter 0) wherever the pattern allows,
so that a match at a wrong rank shows.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TILE, WAVE_ELEMS, ROW, GUARD = 32768, 2048, 256, 64
SENTINEL = 0x5A5A5A5A  # never a source value: sources are in [1, 10000] or negative

SIZES = [1, 255, 256, 257,              # row edge
         2047, 2048, 2049,              # wave tile
         32767, 32768, 32769,           # workgroup tile
         3 * 32768 + 5,                 # odd tile count
         (1 << 20) + 3]                 # 33 tiles, the last one partial


def _pos(wave, row, lane, comp):
    return wave * WAVE_ELEMS + row * ROW + lane * 4 + comp


# one match per tile at (row, lane, comp) of the first (0) and of the last (15) wave of the tile
SINGLES = {f"one_w{w}_r{r}_l{l}_c{c}": _pos(w, r, l, c)
           for w in (0, 15) for (r, l, c) in ((0, 0, 0), (0, 63, 3), (7, 0, 0), (7, 63, 3))}


def _mask(pattern, n):
    """which elements match, from the element index alone"""
    i = np.arange(n, dtype=np.int64)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern in SINGLES:
        return i % TILE == SINGLES[pattern]
    if pattern.startswith("comp"):
        return i % 4 == int(pattern[4:])
    if pattern == "odd_lanes":
        return (i % ROW) // 4 % 2 == 1
    if pattern == "upper_lanes":  # lanes >= 32: the ranks come out of the mbcnt_hi half
        return (i % ROW) // 4 >= 32
    if pattern == "alternate_rows":
        return (i // ROW) % 2 == 0
    raise ValueError(pattern)


MASKED = ["none", "all", *SINGLES, "comp0", "comp1", "comp2", "comp3", "odd_lanes", "upper_lanes", "alternate_rows"]
UNIFORM = {"uniform_f5": 5, "uniform_f101": 101, "uniform_f751": 751}  # about 0.04 %, 1 % and 7.5 % of [1, 10000]


def _host_case(pattern, n, seed=42):
    """(host int32 column, filter): built on the host from a seed and a mask"""
    base = po.gen_uniform_u32(n, seed, 1, 10000).astype(np.int32)
    if pattern in UNIFORM:
        return base, UNIFORM[pattern]
    m = _mask(pattern, n)
    host = base.copy()
    host[m] = -1 - (np.flatnonzero(m) % 1000003).astype(np.int32)  # distinct enough to pin every match to its rank
    return host, 0


def _device_source(host, offset):
    """the column on the device, starting `offset` elements behind a 16-byte boundary"""
    buf = torch.empty(host.size + 4, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    src = buf[offset: offset + host.size]
    src.copy_(torch.from_numpy(host))
    return src


def _run_guarded(plan, src, filt):
    """launch on a sentinel-filled output with guard elements; returns (result on the host, what lies behind it)"""
    n = src.numel()
    plan.out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    plan.launch(src, filt, dense=False)
    m = plan.result().numel()
    whole = plan.out.cpu().numpy()
    return whole[:m], whole[m:]


@pytest.fixture(scope="module")
def expected():
    """(pattern, n) -> (host column, filter, numpy's answer): computed once, shared and left unchanged"""
    cache = {}

    def get(pattern, n):
        if (pattern, n) not in cache:
            host, filt = _host_case(pattern, n)
            want = host[host < filt]
            host.setflags(write=False)
            want.setflags(write=False)
            cache[(pattern, n)] = (host, filt, want)
        return cache[(pattern, n)]

    return get


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", MASKED + list(UNIFORM))
def test_emission_pattern(pattern, n, expected):
    from dwarf_bench_amd import ops
    host, filt, want = expected(pattern, n)
    assert np.array_equal(po.copy_if_lt(host, filt), want)  # the two references agree
    plan = ops.CopyIfLt(n)
    for offset in (0, 1):  # scan_chunk_kernel<true, true> / <false, false>
        got, behind = _run_guarded(plan, _device_source(host, offset), filt)
        assert got.shape == want.shape and np.array_equal(got, want), (pattern, n, offset)
        assert behind.size == n + GUARD - want.size and np.all(behind == SENTINEL), (pattern, n, offset)


def test_several_tiles_per_chunk():
    """From 2^26 rows on chunk_layout gives a chunk more than one tile, and a workgroup alternates between its two
    register sets.  2^26 + 32768 + 5: two tiles per chunk, the last chunk a full tile and a 5-element one.  torch's
    boolean indexing on the device is the reference here (the column is too long for a quick host comparison)."""
    from dwarf_bench_amd import ops
    n = (1 << 26) + TILE + 5
    src = ops.gen_uniform_u32(n, 42, 1, 10000)
    i = torch.arange(n, device="cuda")
    src[(i // ROW) % 3 == 0] = 20000  # empty rows between the others
    src[(i // WAVE_ELEMS) % 5 == 0] = 20000  # and waves without a match
    del i
    plan = ops.CopyIfLt(n)
    for filt in (101, 751):
        plan.out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        plan.launch(src, filt, dense=False)
        got = plan.result()
        want = src[src < filt]
        assert got.numel() == want.numel() and torch.equal(got, want), filt
        assert bool((plan.out[want.numel():] == SENTINEL).all()), filt
        del got, want


def test_plan_reuse_across_filters(expected):
    """the same plan at filter 101, then 5, then 101 on the same source: the third result equals the first"""
    from dwarf_bench_amd import ops
    n = (1 << 20) + 3
    host, _, _ = expected("uniform_f101", n)
    src = _device_source(host, 0)
    plan = ops.CopyIfLt(n)
    results = []
    for filt in (101, 5, 101):
        plan.launch(src, filt, dense=False)
        results.append(plan.result().cpu().numpy().copy())
        assert np.array_equal(results[-1], host[host < filt]), filt
    assert np.array_equal(results[0], results[2])


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_scan_emission as t
from dwarf_bench_amd import ops
for n in (257, 2049, 32769, 3 * 32768 + 5, (1 << 20) + 3):
    for pattern in ("all", "one_w15_r7_l63_c3", "comp2", "upper_lanes", "alternate_rows", "uniform_f101"):
        host, filt = t._host_case(pattern, n)
        want = host[host < filt]
        got, behind = t._run_guarded(ops.CopyIfLt(n), t._device_source(host, 0), filt)
        assert np.array_equal(got, want), (pattern, n)
        assert np.all(behind == t.SENTINEL), (pattern, n)
print("plain loads ok")
"""


def test_aligned_source_with_plain_loads():
    """DBHIP_SCAN_NT=0 is read once per process: a fresh child runs scan_chunk_kernel<true, false> on the aligned source"""
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "DBHIP_SCAN_NT": "0"}, cwd=str(ROOT))
    assert r.returncode == 0 and "plain loads ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
