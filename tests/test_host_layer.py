"""C++ host layer (dwarf_bench_amd/host): the reference's plugin frame re-created.  CPU only.
Compared against outputs of the REFERENCE's own common/{result,options}.cpp (tests/golden/ref_vectors.json)."""
import json
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "dwarf_bench_amd" / "host"
LIB = ROOT / "dwarf_bench_amd" / "_lib"


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host") / "host_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", str(HOST), str(ROOT / "tests/cpp/host_selftest.cpp"),
                    str(HOST / "dwarf_api.cpp"), "-DSELFTEST_NO_REGISTRY", "-o", str(exe),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    return exe


@pytest.fixture(scope="module")
def refv(golden_dir):
    return json.loads((golden_dir / "ref_vectors.json").read_text())


def test_csv_and_printing_match_reference_code(selftest, refv, tmp_path):
    for i, case in enumerate(refv["csv"]):
        path = tmp_path / f"r{i}.csv"
        args = [str(selftest), "csv", str(path), case["dwarf"], case["device_type"].lower(), case["header"] or "-",
                str(len(case["kinds"]))]
        for kind, size, t in zip(case["kinds"], case["buf_sizes"], case["times_us"]):
            args += [str(kind), str(size)] + [repr(float(x)) for x in t]
        printed = ""
        for _ in range(2):  # second run appends without a header (common/result.cpp:60-66)
            printed = subprocess.run(args, check=True, capture_output=True, text=True).stdout
        assert path.read_text() == case["csv_after_two_writes"]
        assert printed == case["printed"]


def test_device_type_parse_print(selftest, refv):
    for case in refv["device_type"]:
        out = subprocess.run([str(selftest), "devtype", case["in"]], check=True, capture_output=True, text=True).stdout.split()
        if case["in"].lower() == "hip":  # the one addition
            assert out == ["4", "HIP"]
        else:
            assert out == [str(case["enum"]), case["to_string"]]


def test_registry_semantics(selftest):
    out = subprocess.run([str(selftest), "registry"], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["111", "2"]


def _cli():
    exe = LIB / "dwarf_bench"
    if not exe.exists():
        from dwarf_bench_amd import build
        build.build_hip()
        build.build_host()
    return exe


def test_cli_list_and_exit_codes():
    exe = _cli()
    r = subprocess.run([str(exe), "list"], capture_output=True, text=True)
    assert r.returncode == 0
    names = [l.strip() for l in r.stdout.splitlines() if l.startswith("\t")]
    assert names == sorted(["DPLScanHip", "GroupByHip", "GroupByLocalHip", "HashBuildHip", "HashBuildNonBitmaskHip", "JoinHip",
                            "JoinOmnisciHip", "NestedLoopJoinHip", "PartitionedJoinHip", "ProbeHip", "RadixHip", "ReduceHip",
                            "TBBSort", "TwoPassScan", "TwoPassScanHip"])
    assert "DWARF_BENCH_ROOT is set to" in r.stdout
    r = subprocess.run([str(exe), "NoSuchDwarf"], capture_output=True, text=True)
    assert r.returncode == 1 and "List supported dwarfs" in r.stderr  # main.cpp:75-79
    r = subprocess.run([str(exe), "--help", "RadixHip"], capture_output=True, text=True)
    assert r.returncode == 0 and "--input_size" in r.stdout and "--groups_count" in r.stdout
    env = dict(os.environ, DWARF_BENCH_ROOT="/some/where")
    r = subprocess.run([str(exe), "list"], capture_output=True, text=True, env=env)
    assert "DWARF_BENCH_ROOT is set to /some/where" in r.stdout


def test_reference_usage_example_compiles_against_our_header():
    """A client written the way the reference's example/bench_usage/main.cpp:4-33 uses the library (designated
    RunConfig initialisers in the reference's member order, enums streamed, Measurement fields read) must compile
    against this build's <bench.hpp>.  The client is tests/cpp/bench_usage_client.cpp, so the check needs nothing
    outside the repository."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", str(HOST), str(ROOT / "tests/cpp/bench_usage_client.cpp")],
                   check=True)


def test_baseline_config_1_as_written_runs_on_the_host(tmp_path):
    """BASELINE.json configs[0], verbatim: `TwoPassScan --device=cpu --input_size=1024 --iterations=9` — nine valid
    Results and the reference's CSV (scan/scan.cpp:184-195, common/result.cpp:59-91).  The host dwarf needs no GPU."""
    exe = _cli()
    path = tmp_path / "scan.csv"
    r = subprocess.run([str(exe), "TwoPassScan", "--device=cpu", "--input_size=1024", "--iterations=9", "--report_path", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "incorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    lines = path.read_text().splitlines()
    assert lines[0] == "device_type,buf_size_bytes,host_time_ms,kernel_time_ms"
    assert len(lines) == 10 and all(l.startswith("CPU,4096,") for l in lines[1:])
    r = subprocess.run([str(exe), "TwoPassScan", "--device=cpu", "--input_size=1024", "--iterations=9"], capture_output=True, text=True,
                       timeout=120)  # without a report path every Result is printed (common/result.cpp:5-18, :42-57)
    assert r.returncode == 0 and r.stdout.count("Kernel duration:") == 9 and r.stdout.count("Host duration:") == 9


def test_host_dwarfs_on_ragged_sizes_and_the_wrong_device(tmp_path):
    """TwoPassScan / TBBSort (sort/tbbsort.cpp:15-48) validate every iteration against std::copy_if /
    std::sort: sizes that are not a multiple of the thread count (the reference kernel drops that tail, ours does
    not), an empty column, several sizes in one run; asked for --device=hip they throw like the reference's device
    selection does for a type it does not serve (caught by main: exit code 0, main.cpp:97-100)."""
    exe = _cli()
    for dwarf in ("TwoPassScan", "TBBSort"):
        path = tmp_path / f"{dwarf}.csv"
        r = subprocess.run([str(exe), dwarf, "--device", "cpu", "--input_size", "0", "1", "1000003", "262144", "--iterations", "3",
                            "--report_path", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "incorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
        sizes = [l.split(",")[1] for l in path.read_text().splitlines()[1:]]
        assert sizes == ["0"] * 3 + ["4"] * 3 + [str(4 * 1000003)] * 3 + [str(4 * 262144)] * 3
        r = subprocess.run([str(exe), dwarf, "--device", "hip", "--input_size", "1024"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "is the host dwarf" in r.stderr
