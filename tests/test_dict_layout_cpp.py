"""dwarf_bench_amd/host/dict_layout.hpp on the host: tests/cpp/dict_layout_check.cpp is a stand-alone program that runs
the hash, the slot count, the workspace regions and the insert and find loops — the text the kernels of dict_encode.cpp
run — over every capacity 1..4096 and a ladder up to 2^31 - 1, against the exported workspace query, and over tables
whose probe chains wrap past the end.  The program, and only it, is built with -fsanitize=address,undefined where the
host compiler has the runtimes (plain otherwise); nothing loaded into Python runs under a sanitizer."""
import shutil
import subprocess

import pytest

from dwarf_bench_amd import _capi
from dwarf_bench_amd import dict_native as dn
from tests.capi_testlib import ROOT, ensure_built

HOST = ROOT / "dwarf_bench_amd" / "host"
SOURCE = ROOT / "tests" / "cpp" / "dict_layout_check.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
LADDER = [4097, 5000, 65535, 65536, 65537, 100003, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 24) + 5, (1 << 26) - 1, 1 << 26,
          (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 2, (1 << 31) - 1]


@pytest.fixture(scope="module")
def check_tool(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("dict_layout") / "dict_layout_check"
    base = [cxx, "-O1", "-g", "-std=c++17", "-w", "-I", str(HOST), str(SOURCE), "-o", str(exe)]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600).returncode == 0
    if not sanitized:  # no sanitizer runtimes beside this compiler: the checked table still sees every index
        subprocess.run(base, check=True, timeout=600)
    return exe, sanitized


def test_dict_layout_on_the_host_every_small_capacity_and_a_ladder(check_tool, tmp_path):
    exe, sanitized = check_tool
    ensure_built()
    sort_bytes = _capi.lib().dbhip_radix_sort_workspace_bytes
    table = tmp_path / "layouts.txt"  # capacity, the inner sort's workspace bytes, the exported query's answer
    table.write_text("".join(f"{c} {sort_bytes(c, 8)} {dn.workspace_bytes(c)}\n" for c in list(range(1, 4097)) + LADDER))
    r = subprocess.run([str(exe), str(table)], capture_output=True, text=True, timeout=300)
    print("sanitizers:", "address,undefined" if sanitized else "none (no runtimes)", "|", r.stdout.strip())
    assert r.returncode == 0 and "dict layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_kernels_run_the_same_text():
    """dict_encode.cpp includes dict_layout.hpp and calls its functions, as the host check does"""
    kernels = (HOST / "dict_encode.cpp").read_text()
    shared = (HOST / "dict_layout.hpp").read_text()
    assert '#include "dict_layout.hpp"' in kernels and '#include "dict_layout.hpp"' in SOURCE.read_text()
    for name in ("dict_hash", "dict_layout", "dict_insert", "dict_find_after", "dict_find_slot"):
        assert f" {name}(" in shared and f"{name}(" in kernels and f"{name}(" in SOURCE.read_text(), name
    assert shared.count("DBENCH_DICT_FN ") >= 7 and "#define DBENCH_DICT_FN __host__ __device__ inline" in shared
    header = (HOST / "dict_encode.hpp").read_text()
    assert f"#define DBENCH_DICT_LDS_SLOTS {dn.LDS_SLOTS}\n" in header and "s_table[DBENCH_DICT_LDS_SLOTS]" in kernels
