"""dwarf_bench_amd/host/hll_layout.hpp on the host: tests/cpp/hll_layout_check.cpp is a stand-alone program that runs the two
hash chains of a key tuple, the placement of a hash and the estimator — the text the kernels of hll_sketch.cpp run — and
prints what they give; every line is compared here with tests/hll_model.py.  That pins, among other things, p = 4 and p = 14,
w == 0, w with only its lowest valid bit set and w with bits only in its g half (a 32-bit clz fails those).  Built with hipcc
(fmix32 lives in csrc/dbhip_common.hpp); no GPU is needed."""
import math
import subprocess

import numpy as np
import pytest

from tests import hll_model as hm
from tests.capi_testlib import ROOT

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "hll_layout_check.cpp"
SEEDS = (0, 0xDEADBEEF)
PS = (4, 5, 11, 14)
U, W = np.uint32, np.uint64


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hll_layout") / "hll_layout_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", str(HOST), "-I",
                    str(ROOT / "dwarf_bench_amd" / "csrc"), str(SOURCE), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hll layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_every_printed_hash_is_the_models(printed):
    rows = np.array([[int(x) for x in f[1:]] for f in printed if f[0] == "H"], dtype=np.uint64)
    assert rows.shape == (len(SEEDS) * 4 * 206, 8)
    for seed in SEEDS:
        for k in (1, 2, 3, 4):
            mine = rows[(rows[:, 0] == seed) & (rows[:, 1] == k)]
            assert mine.shape[0] == 206
            cols = [mine[:, 2 + j].astype(U) for j in range(k)]
            assert [int(c) for c in cols[0][:6]] == [0, 1, seed, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
            h, g = hm.hash_tuples(cols, seed)
            assert np.array_equal(h.astype(W), mine[:, 6]) and np.array_equal(g.astype(W), mine[:, 7]), (seed, k)
            assert not np.array_equal(h, g)
            if k > 1:  # the order of the columns matters, and so does the last column
                h2, g2 = hm.hash_tuples(cols[::-1], seed)
                assert int((h2 != h).sum()) > 190
                h3, _ = hm.hash_tuples(cols[:-1], seed)
                assert int((h3 != h).sum()) > 190
    a, b = (rows[(rows[:, 0] == s) & (rows[:, 1] == 1)] for s in SEEDS)  # the seed moves a key: key 0 and key 1
    assert (a[0, 6], a[0, 7]) != (b[0, 6], b[0, 7]) and (a[1, 6], a[1, 7]) != (b[1, 6], b[1, 7])


def test_every_printed_place_is_the_models(printed):
    rows = np.array([[int(x) for x in f[1:]] for f in printed if f[0] == "P"], dtype=np.uint64)
    assert rows.shape == (len(PS) * (13 + 64 + 300), 5)
    for p in PS:
        q = 64 - p
        mine = rows[rows[:, 0] == p]
        h, g = mine[:, 1].astype(U), mine[:, 2].astype(U)
        idx, rank = hm.place(h, g, p)
        assert np.array_equal(idx.astype(W), mine[:, 3]) and np.array_equal(rank.astype(W), mine[:, 4]), p
        got = {(int(a), int(b)): (int(i), int(r)) for a, b, i, r in mine[:, 1:]}
        assert got[(0, 0)] == (0, q + 1)                                   # w == 0
        assert got[(0xFFFFFFFF << (32 - p) & 0xFFFFFFFF, 0)] == ((1 << p) - 1, q + 1)  # w == 0 behind a full index
        assert got[(0, 1)] == (0, q)                                       # only the lowest valid bit of w
        assert got[(0, 0x80000000)] == (0, 32 - p + 1)                     # bits only in the g half
        assert got[(0, 0xFFFFFFFF)] == (0, 32 - p + 1)
        assert got[(1, 0)] == (0, 32 - p)                                  # the lowest bit of the h half
        assert got[(0x80000000, 0)] == (1 << (p - 1), q + 1)               # the top bit belongs to the index
        assert got[(1 << (31 - p), 0)] == (0, 1)                           # the first bit behind the index: rank 1
        assert int(rank.min()) == 1 and int(rank.max()) == q + 1 and int(idx.max()) == (1 << p) - 1
        assert int((rank > 33 - p).sum()) > 30  # ranks that a 32-bit clz of the h half cannot give


def test_every_printed_estimate_is_the_models(printed):
    rows = [(int(f[1]), f[2], float(f[3])) for f in printed if f[0] == "E"]
    assert len(rows) == 4 * len(PS)
    for p, what, got in rows:
        m, q = 1 << p, 64 - p
        hist = [0] * 64
        if what == "empty":
            hist[0] = m
        elif what == "saturated":
            hist[q + 1] = m
        elif what == "ones":
            hist[1] = m
        else:
            hist[1], hist[2], hist[0], hist[7] = m // 2, m // 4, m // 8, m // 8
        want = hm.estimate(hist, p)
        if what == "empty":
            assert got == 0.0 == want
        elif what == "saturated":
            assert math.isinf(got) and math.isinf(want) and got > 0
        else:
            assert got > 0 and abs(got - want) <= 1e-12 * want, (p, what, got, want)
        if what == "ones":  # every register 1: z = m / 2, so m / ln 2
            assert m / 2 < got < 2 * m


def test_the_kernels_run_the_same_text():
    kernels = (HOST / "hll_sketch.cpp").read_text()
    shared = (HOST / "hll_layout.hpp").read_text()
    assert '#include "hll_layout.hpp"' in kernels and '#include "hll_layout.hpp"' in SOURCE.read_text()
    for name in ("hll_hash_first", "hll_hash_next", "hll_place"):
        assert f" {name}(" in shared and f"{name}(" in kernels and f"{name}(" in SOURCE.read_text(), name
    assert "hll_estimate(" in kernels and "hll_estimate(" in SOURCE.read_text()
    assert "#define DBENCH_HLL_FN __host__ __device__ inline" in shared and shared.count("DBENCH_HLL_FN ") >= 5
    assert "__builtin_clzll" in shared and f"{hm.GOLDEN:#X}"[2:] in shared.upper()
    assert (hm.MIN_P, hm.MAX_P, hm.MAX_COLS, hm.HIST_WORDS) == tuple(
        int(shared.split(f"#define DBENCH_HLL_{n} ")[1].split()[0]) for n in ("MIN_P", "MAX_P", "MAX_COLS", "HIST_WORDS"))
