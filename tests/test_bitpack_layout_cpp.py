"""dwarf_bench_amd/host/bitpack_layout.hpp on the host: tests/cpp/bitpack_layout_check.cpp is a stand-alone program that
runs the word count, the bit position, the insert of a group and the extract — the text the kernels of bitpack.cpp run —
over every width 1..32 at every row count 0..300 against a bit-by-bit reference, over a ladder of row indices up to
2^32 - 1 on a fake column, and against the exported queries' answers.  The program, and only it, is built with
-fsanitize=address,undefined where the host compiler has the runtimes (plain otherwise); nothing loaded into Python runs
under a sanitizer."""
import shutil
import subprocess

import pytest

from dwarf_bench_amd import bitpack_native as bn
from tests.capi_testlib import ROOT, SIZES, ensure_built

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "bitpack_layout_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ROWS = [0, 1, 31, 32, 33, 127, 128, 129, 4097, 65537, (1 << 26) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("bitpack_layout") / "bitpack_layout_check"
    base = [cxx, "-O1", "-g", "-std=c++17", "-w", "-I", str(HOST), str(SOURCE), "-o", str(exe)]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600).returncode == 0
    if not sanitized:  # no sanitizer runtimes beside this compiler: the checked arrays still see every index
        subprocess.run(base, check=True, timeout=600)
    return exe, sanitized


def test_bitpack_layout_on_the_host_every_width_and_a_ladder(check_tool, tmp_path):
    exe, sanitized = check_tool
    ensure_built()
    table = tmp_path / "answers.txt"  # what the exported queries say
    lines = [f"W {n} {w} {bn.words(n, w)}\n" for w in range(0, 35) for n in ROWS]
    lines += [f"S {c} {bn.workspace_bytes(c)}\n" for c in SIZES + (4095, 4097, 1 << 32, 1 << 40)]
    table.write_text("".join(lines))
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, timeout=300)
    print("sanitizers:", "address,undefined" if sanitized else "none (no runtimes)", "|", r.stdout.strip())
    assert r.returncode == 0 and "bitpack layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_kernels_run_the_same_text():
    """bitpack.cpp includes bitpack_layout.hpp and calls its functions, as the host check does"""
    kernels = (HOST / "bitpack.cpp").read_text()
    shared = (HOST / "bitpack_layout.hpp").read_text()
    assert '#include "bitpack_layout.hpp"' in kernels and '#include "bitpack_layout.hpp"' in SOURCE.read_text()
    for name in ("bitpack_words", "bitpack_mask", "bitpack_extract", "bitpack_extract_staged", "bitpack_group_word",
                 "bitpack_layout"):
        assert f" {name}(" in shared and f"{name}(" in kernels and f"{name}(" in SOURCE.read_text(), name
    assert "bitpack_bit(" in shared and "bitpack_funnel(" in shared
    assert "bitpack_insert_group(" in SOURCE.read_text() and "bitpack_funnel(" in SOURCE.read_text()
    assert shared.count("DBENCH_BITPACK_FN ") >= 8 and "#define DBENCH_BITPACK_FN __host__ __device__ inline" in shared
    header = (HOST / "bitpack.hpp").read_text()
    assert f"#define DBENCH_BITPACK_SEGMENT_ROWS {bn.SEGMENT_ROWS} " in header
    assert f"#define DBENCH_BITPACK_TILE_ROWS {bn.TILE_ROWS} " in header
