"""dwarf_bench_amd/host/merge_path.hpp on the host: tests/cpp/merge_path_check.cpp is a stand-alone program that runs
the diagonal search, the clamped tile extents and the serial merge — the text the kernels of merge_sorted.cpp run — over
every pair of sizes in [0, 9] x [0, 9] with a tile of 4, random sizes against std::merge, and shuffled inputs, on arrays
that check every index.  The program, and only it, is built with -fsanitize=address,undefined where the host compiler
has the runtimes (plain otherwise); nothing loaded into Python runs under a sanitizer."""
import shutil
import subprocess

import pytest

from dwarf_bench_amd import merge_native as mn
from tests.capi_testlib import ROOT

SOURCE = ROOT / "tests" / "cpp" / "merge_path_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("merge_path") / "merge_path_check"
    base = [cxx, "-O1", "-g", "-std=c++17", "-w", "-I", str(ROOT / "dwarf_bench_amd" / "host"), str(SOURCE), "-o", str(exe)]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600).returncode == 0
    if not sanitized:  # no sanitizer runtimes beside this compiler: the checked arrays still see every index
        subprocess.run(base, check=True, timeout=600)
    return exe, sanitized


def test_merge_path_on_the_host_every_small_size_random_and_unsorted(check_tool):
    exe, sanitized = check_tool
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print("sanitizers:", "address,undefined" if sanitized else "none (no runtimes)", "|", r.stdout.strip())
    assert r.returncode == 0 and "merge path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_kernels_run_the_same_text():
    """merge_sorted.cpp includes merge_path.hpp and calls its three functions, as the host check does"""
    kernels = (ROOT / "dwarf_bench_amd" / "host" / "merge_sorted.cpp").read_text()
    shared = (ROOT / "dwarf_bench_amd" / "host" / "merge_path.hpp").read_text()
    assert '#include "merge_path.hpp"' in kernels and '#include "merge_path.hpp"' in SOURCE.read_text()
    for name in ("mp_diagonal", "mp_tile_extents", "mp_serial_merge"):
        assert f" {name}(" in shared and f"{name}" in kernels and name in SOURCE.read_text(), name
    header = (ROOT / "dwarf_bench_amd" / "host" / "merge_sorted.hpp").read_text()
    assert f"#define DBENCH_MERGE_TILE_ROWS {mn.TILE_ROWS} " in header and "kMpTile = DBENCH_MERGE_TILE_ROWS" in kernels
    assert shared.count("DBENCH_MP_FN ") >= 3 and "#define DBENCH_MP_FN __host__ __device__ inline" in shared
