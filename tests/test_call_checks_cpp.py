"""dwarf_bench_amd/host/call_checks.hpp on the host: tests/cpp/call_checks_check.cpp is a stand-alone program that runs the
argument checks the dbench_* entry points share — overlap in both argument orders, touching and one byte short of it, at
the top of the address space; outputs_overlap at the first and the last index; words_past_16; fits_32 around 2^32.  The
program, and only it, is built with -fsanitize=address,undefined where the host compiler has the runtimes (plain
otherwise); nothing loaded into Python runs under a sanitizer."""
import shutil
import subprocess

import pytest

from tests.capi_testlib import ROOT

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "call_checks_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
FAMILIES = ("select_rows", "merge_sorted", "take_rows", "dict_encode", "bitpack")


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("call_checks") / "call_checks_check"
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", str(HOST), str(SOURCE), "-o", str(exe)]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600).returncode == 0
    if not sanitized:  # no sanitizer runtimes beside this compiler
        subprocess.run(base, check=True, timeout=600)
    return exe, sanitized


def test_call_checks_on_the_host(check_tool):
    exe, sanitized = check_tool
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print("sanitizers:", "address,undefined" if sanitized else "none (no runtimes)", "|", r.stdout.strip())
    assert r.returncode == 0 and "call checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_entry_points_run_the_same_text():
    """the header has no HIP in it; the five operators reach it through rowlist.hpp and define none of it again"""
    shared = (HOST / "call_checks.hpp").read_text()
    assert "hip_runtime" not in shared and "__device__" not in shared and "dbhip_common" not in shared
    assert '#include "call_checks.hpp"' in SOURCE.read_text()
    rowlist = (HOST / "rowlist.hpp").read_text()
    assert '#include "call_checks.hpp"' in rowlist
    for name in ("addr", "words_past_16", "fits_32", "overlap", "outputs_overlap"):
        assert f" {name}(" in shared and f"{name}(" in SOURCE.read_text(), name
    for family in FAMILIES:
        text = (HOST / f"{family}.cpp").read_text()
        assert '#include "rowlist.hpp"' in text, family
        assert "overlap(" in text and "begin_call(" in text, family
        for definition in ("bool overlap(", "unsigned words_past_16(", "size_t clamped_count(", "uintptr_t addr(",
                           "_scan_kernel(", "struct Range ", "Pred {"):
            assert definition not in text, (family, definition)
    for header in ("call_checks.hpp", "rowlist.hpp"):  # the C surface stays the five families' headers'
        assert "dbench_" not in (HOST / header).read_text().replace("dbench_*", ""), header
