"""dwarf_bench_amd/host/bloom_layout.hpp on the host: tests/cpp/bloom_layout_check.cpp is a stand-alone program that runs
the placement of a key and the sizing query — the text the kernels of bloom_filter.cpp run — and prints what they give;
every line is compared here with tests/bloom_model.py.  That pins, among other things, masks with bits above bit 31 and
the 64-bit multiply at n_words = 2^32 - 1.  Built with hipcc (fmix32 lives in csrc/dbhip_common.hpp); no GPU is needed."""
import subprocess

import numpy as np
import pytest

from tests import bloom_model as blm
from tests.capi_testlib import ROOT

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "bloom_layout_check.cpp"
SIZES = (1, 2, 3, 64, 1000, 65537, (1 << 32) - 1)
SEEDS = (0, 12345)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bloom_layout") / "bloom_layout_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", str(HOST), "-I",
                    str(ROOT / "dwarf_bench_amd" / "csrc"), str(SOURCE), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bloom layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_every_printed_place_is_the_models(printed):
    places = np.array([[int(x) for x in f[1:]] for f in printed if f[0] == "P"], dtype=np.uint64)
    assert places.shape == (len(SEEDS) * len(SIZES) * 1006, 5)
    seen = set()
    for seed in SEEDS:
        for n_words in SIZES:
            at = (places[:, 0] == seed) & (places[:, 1] == n_words)
            keys = places[at, 2].astype(np.uint32)
            assert keys.size == 1006
            assert [int(k) for k in keys[:6]] == [0, 1, seed, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
            word, mask = blm.place(keys, n_words, seed)
            assert np.array_equal(word.astype(np.uint64), places[at, 3]), (seed, n_words)
            assert np.array_equal(mask, places[at, 4]), (seed, n_words)
            seen.add((seed, n_words))
            if n_words == (1 << 32) - 1:  # the product needs all 64 bits: words beyond 2^31 are reached
                assert int(word.max()) > 1 << 31
    assert len(seen) == len(SEEDS) * len(SIZES)
    assert int((places[:, 4] >> np.uint64(32)).astype(bool).sum()) > places.shape[0] // 2  # bits above bit 31
    a, b = (places[(places[:, 0] == s) & (places[:, 1] == 1000)] for s in SEEDS)  # the seed moves a key: key 0 and key 1
    assert (a[0, 3], a[0, 4]) != (b[0, 3], b[0, 4]) and (a[1, 3], a[1, 4]) != (b[1, 3], b[1, 4])


def test_every_printed_word_count_is_the_models(printed):
    rows = [[int(x) for x in f[1:]] for f in printed if f[0] == "W"]
    assert len(rows) == 25 * 14
    refused = 0
    for n, bits, got in rows:
        assert got == blm.words(n, bits), (n, bits, got)
        refused += got == 0
    assert refused > 50 and {(n, b) for n, b, g in rows if g == 0} >= {(5, 0), (5, 65), (1 << 32, 64), (1 << 38, 1), (1 << 63, 2)}
    assert [blm.words(0, 16), blm.words(1, 1), blm.words(4, 16), blm.words(5, 16), blm.words(1 << 24, 16)] == [1, 1, 1, 2, 1 << 22]


def test_the_kernels_run_the_same_text():
    kernels = (HOST / "bloom_filter.cpp").read_text()
    shared = (HOST / "bloom_layout.hpp").read_text()
    assert '#include "bloom_layout.hpp"' in kernels and '#include "bloom_layout.hpp"' in SOURCE.read_text()
    for name in ("bloom_words", "bloom_place"):
        assert f" {name}(" in shared and f"{name}(" in kernels and f"{name}(" in SOURCE.read_text(), name
    assert "#define DBENCH_BLOOM_FN __host__ __device__ inline" in shared and shared.count("DBENCH_BLOOM_FN ") >= 5
    assert "1ull <<" in shared and "0x9E3779B9u" in shared and f"{blm.GOLDEN:#X}"[2:] in shared.upper()
