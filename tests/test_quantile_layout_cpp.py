"""dwarf_bench_amd/host/quantile_layout.hpp on the host: tests/cpp/quantile_layout_check.cpp is a stand-alone program that runs
the rank formula, the digits of the three levels and the bin test — the text qs_pick of quantile_select.cpp runs — and prints
what they give; every line is compared here with tests/quantile_model.py.  That pins m in {0, 1, 2, 3, 2^32 - 1}, the fractions
0/1, 1/1, 1/2, 1/3, 999999999/10^9 and a denominator of 2^32 - 1, the absolute ranks 0, m - 1, m and 2^32 - 1, and histograms
with empty bins in front of, between and behind the hit.  Built with g++; no GPU is needed."""
import subprocess

import numpy as np
import pytest

from tests import quantile_model as qm
from tests.capi_testlib import ROOT

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "quantile_layout_check.cpp"
TOP = (1 << 32) - 1


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("quantile_layout") / "quantile_layout_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", str(HOST), str(SOURCE), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "quantile layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_every_printed_rank_is_the_models(printed):
    rows = [[int(x) for x in f[1:]] for f in printed if f[0] == "R"]
    assert len(rows) == 11 * (14 + 6)
    for num, den, m, live, r in rows:
        want = qm.rank(num, den, m)
        assert (live, r) == ((0, 0) if want is None else (1, want)), (num, den, m, live, r, want)
    got = {(num, den, m): (live, r) for num, den, m, live, r in rows}
    for m in (0, 1, 2, 3, TOP):
        for frac in ((0, 1), (1, 1), (1, 2), (1, 3), (999999999, 10 ** 9), (1, TOP), (TOP, TOP)):
            assert frac + (m,) in got, (frac, m)
        for k in (0, (m - 1) & TOP, m, TOP):
            assert (k, 0, m) in got, (k, m)
        assert got[(m, 0, m)] == (0, 0) and got[(0, 0, m)] == (int(m > 0), 0)
    assert got[(1, 2, 1)] == (1, 0) and got[(1, 2, 2)] == (1, 0) and got[(1, 2, 3)] == (1, 1) and got[(1, 2, 4)] == (1, 1)  # lower
    assert got[(1, 1, TOP)] == (1, TOP - 1) and got[(1, 2, TOP)] == (1, (TOP + 1) // 2 - 1) and got[(0, 1, TOP)] == (1, 0)
    assert got[(999999999, 10 ** 9, TOP)] == (1, -(-999999999 * TOP // 10 ** 9) - 1)  # a product beyond 2^61
    assert got[(TOP - 1, TOP, TOP)] == (1, TOP - 2) and got[(1, TOP, TOP)] == (1, 0) and got[(TOP, TOP, 3)] == (1, 2)
    assert got[(1, 1, 0)] == (0, 0) == got[(0, 1, 0)] and got[(TOP, 0, TOP)] == (0, 0) and got[(TOP - 1, 0, TOP)] == (1, TOP - 1)


def test_every_printed_digit_is_the_models(printed):
    rows = [[int(x) for x in f[1:]] for f in printed if f[0] == "D"]
    assert len(rows) == 10 * 3
    for x, level, d, shift, width, high in rows:
        assert (shift, width) == (qm.SHIFTS[level], qm.WIDTHS[level])
        assert d == (x >> shift) & ((1 << width) - 1)
        assert high == (TOP >> (shift + width) << (shift + width) if level else 0)
    assert sum(qm.WIDTHS) == 32 and qm.SHIFTS == (21, 10, 0)


def test_every_printed_bin_is_the_models(printed):
    hists = {int(f[1]): [int(x) for x in f[2:]] for f in printed if f[0] == "G"}
    picks = [[int(x) for x in f[1:]] for f in printed if f[0] == "B"]
    assert len(hists) == 10 and len(picks) > 100
    shapes = set()
    for h, rem, got_bin, got_before in picks:
        bins = np.array(hists[h], np.uint64)
        ends = np.cumsum(bins)
        if rem >= int(ends[-1]):
            assert (got_bin, got_before) == (-1, 0), (h, rem)
            continue
        want = int(np.searchsorted(ends, rem, "right"))  # the first bin whose end lies behind rem
        assert (got_bin, got_before) == (want, int(ends[want] - bins[want])), (h, rem, got_bin, want)
        assert bins[want] > 0
        shapes.add((bool((bins[:want] == 0).any()) and want > 0, bool((bins[want + 1:] == 0).any()),
                    bool(want > 1 and bins[0] > 0 and (bins[1:want] == 0).any())))
    assert {s[0] for s in shapes} == {False, True} and {s[1] for s in shapes} == {False, True} and any(s[2] for s in shapes)


def test_the_kernels_run_the_same_text():
    kernels = (HOST / "quantile_select.cpp").read_text()
    shared = (HOST / "quantile_layout.hpp").read_text()
    assert '#include "quantile_layout.hpp"' in kernels and '#include "quantile_layout.hpp"' in SOURCE.read_text()
    for name in ("qs_resolve_rank", "qs_bin_holds", "qs_shift", "qs_radix", "qs_high_mask"):
        assert f" {name}(" in shared and f"{name}(" in kernels and f"{name}(" in SOURCE.read_text(), name
    assert "#define DBENCH_QUANTILE_FN __host__ __device__ inline" in shared and shared.count("DBENCH_QUANTILE_FN ") >= 7
