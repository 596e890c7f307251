"""Test-only helpers for the public C surface and the CLIs built from host/main.cpp: what a header under include/
declares, what an executable lists, the error codes of include/dbhip.h, and the table of dwarf sets.  Nothing here
touches a device.  Never imported by the product."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
LIB = ROOT / "dwarf_bench_amd" / "_lib"
OK, EINVAL, EWORKSPACE, ENODEVICE = 0, -1, -2, -3  # DBHIP_OK, DBHIP_EINVAL, DBHIP_EWORKSPACE, DBHIP_ENODEVICE
# row counts around the segment, chunk and 32-bit edges of the workspace queries
SIZES = (0, 1, 1023, 1024, 1025, 4096, 100003, 1 << 20, (1 << 22) + 1, 1 << 24, (1 << 24) + 5, 1 << 30, (1 << 32) - 1)

# what populate_registry() registers: the list of `dwarf_bench list`
DEFAULT = ["DPLScanHip", "GroupByHip", "GroupByLocalHip", "HashBuildHip", "HashBuildNonBitmaskHip", "JoinHip",
           "JoinOmnisciHip", "NestedLoopJoinHip", "PartitionedJoinHip", "ProbeHip", "RadixHip", "ReduceHip", "TBBSort",
           "TwoPassScan", "TwoPassScanHip"]
# executable -> the dwarfs it lists beyond DEFAULT; dwarf_bench_<set> is host/main.cpp built for that row of kDwarfSets
# (host/register_dwarfs.cpp) by the SETS rule of host/Makefile
CLI_SETS = {
    "dwarf_bench": [],
    "dwarf_bench_experimental": ["CuckooHashBuildHip"],
    "dwarf_bench_slab": ["SlabHashBuildHip", "SlabJoinHip", "SlabProbeHip"],
    "dwarf_bench_groupby_hash": ["GroupByHashHip"],
    "dwarf_bench_sort_pairs": ["RadixPairsHip"],
    "dwarf_bench_join_pairs": ["JoinPairsHip"],
    "dwarf_bench_topk": ["TopKHip"],
    "dwarf_bench_groupby_sorted": ["GroupBySortedHip"],
    "dwarf_bench_window": ["WindowSortedHip"],
    "dwarf_bench_range_join": ["RangeJoinHip"],
}


def _code(header):
    return re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)


def declared(header):
    """the entry points a header under include/ declares, sorted"""
    return sorted(set(re.findall(r"\b(dbhip_[a-z0-9_]+)\s*\(", _code(header))))


_SCALARS = {"int": C.c_int, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
POINTER = "pointer"  # any pointer parameter, dbhip_stream_t included: the bindings pass them as addresses


def prototypes(header):
    """name -> (restype, [argtype, ...]) as the header's C text has them: ctypes scalars, POINTER for every pointer"""
    out = {}
    for ret, name, params in re.findall(r"^(\w+)\s+(dbhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _code(header), flags=re.M):
        args = []
        for p in (p.strip() for p in params.split(",")):
            words = p.replace("const", " ").replace("*", " ").split()
            if p == "void":
                continue
            args.append(POINTER if "*" in p or words[0] == "dbhip_stream_t" else _SCALARS[words[0]])
        out[name] = (_SCALARS[ret], args)
    return out


def defines(header):
    """the integer constants a header defines: DBHIP_NAME -> value"""
    return {name: int(value) for name, value in re.findall(r"^#define (DBHIP_\w+) \(?(-?\d+)u?\)?", _code(header), flags=re.M)}


def ensure_built():
    """libdbhip.so and every executable of CLI_SETS exist (a test that starts one calls this first)"""
    if not all((LIB / f).exists() for f in ["libdbhip.so", *CLI_SETS]):
        from dwarf_bench_amd import build
        build.build_hip()
        build.build_host()


def cli_names(exe):
    """the dwarfs `<exe> list` prints, in its order"""
    ensure_built()
    r = subprocess.run([str(LIB / exe), "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (exe, r.stderr[-500:])
    return [line.strip() for line in r.stdout.splitlines() if line.startswith("\t")]
