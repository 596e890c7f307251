"""The general group-by (dbhip_groupby_hash_u32) without a GPU: the workspace query, the host-side argument
checks (before any HIP call), the compiled code object of csrc/groupby_hash.hip and the shape tests' constructed inputs."""
import re
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE

ROOT = Path(__file__).resolve().parents[1]


def test_workspace_query():
    ws = _capi.lib().dbhip_groupby_hash_workspace_bytes
    assert ws(1 << 31, 0) > 0 and ws((1 << 31) + 1, 0) == 0
    for n in (0, 1, 1000, 1 << 20, 1 << 24, 1 << 26):
        for mg in (0, 1, 64, 4096, 4097, 1 << 16, 1 << 20):
            b = ws(n, mg)
            assert b % 256 == 0 and b >= 256, (n, mg)
            groups = min(mg or n, n)
            assert b >= 256 + 12 * max(64, 2 * groups), (n, mg)  # the global table: 12-byte slots, two per group
            assert b <= 65 * n + (2 << 20), (n, mg)  # dbhip.h: at most 65 bytes per row plus 2 MiB
    # grows with n and with the bound
    assert ws(1 << 20, 0) < ws(1 << 22, 0) < ws(1 << 24, 0)
    assert ws(1 << 24, 64) < ws(1 << 24, 1 << 16) < ws(1 << 24, 1 << 20) <= ws(1 << 24, 0)
    assert ws(1 << 24, 4096) <= ws(1 << 24, 4097)


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20  # 256-aligned, never dereferenced: every call below fails on the host first
    n, mg = 4096, 100
    wsb = lib.dbhip_groupby_hash_workspace_bytes(n, mg)

    def call(keys=fake, vals=fake, n=n, mg=mg, ok=fake, os_=fake, oc=fake, og=fake, w=fake, wb=wsb):
        return lib.dbhip_groupby_hash_u32(keys, vals, n, mg, ok, os_, oc, og, w, wb, None)

    assert call(keys=None) == EINVAL and call(vals=None) == EINVAL
    assert call(ok=None) == EINVAL and call(os_=None) == EINVAL and call(og=None) == EINVAL
    assert call(keys=fake + 4) == EINVAL and call(vals=fake + 8) == EINVAL  # 16-byte alignment
    assert call(n=(1 << 31) + 1, wb=1 << 40) == EINVAL
    assert call(w=None) == EWORKSPACE and call(w=fake + 64) == EWORKSPACE and call(wb=wsb - 1) == EWORKSPACE
    assert call(n=1 << 20, mg=0, wb=wsb) == EWORKSPACE  # a workspace sized for fewer groups
    dist = lib.dbhip_check_distinct_u32
    dwb = lib.dbhip_check_distinct_workspace_bytes(n)
    assert dwb >= 2 * 4 * n
    assert dist(None, n, fake, fake, dwb, None) == EINVAL and dist(fake, n, None, fake, dwb, None) == EINVAL
    assert dist(fake, n, fake, None, dwb, None) == EWORKSPACE and dist(fake, n, fake, fake, dwb - 1, None) == EWORKSPACE


def test_ops_refuses_unaligned_columns_and_large_bounds():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    t = torch.zeros(17, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what GroupByHash.launch applies to both columns
    with pytest.raises(ValueError):
        ops.GroupByHash(16, max_groups=1 << 32, device="cpu")


def test_code_object_has_no_scratch_and_uses_lds_cas(tmp_path):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--save-temps", "-c", str(ROOT / "dwarf_bench_amd" / "csrc" / "groupby_hash.hip"), "-o",
                    str(tmp_path / "gbh.o")], check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "groupby_hash-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    bodies = dict(re.findall(r"^(_ZN\S*gbh_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M))
    assert len(bodies) == 6, sorted(bodies)  # lds, global, part, giant, compact, finish
    meta = re.findall(r"\.name:\s+(_ZN\S*gbh_\w+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 6 and all(size == "0" for _, size in meta), meta
    assert "scratch_" not in "".join(bodies.values())
    lds = next(b for name, b in bodies.items() if "gbh_lds_kernel" in name)
    assert "ds_cmpst" in lds and "ds_add_u32" in lds
    assert "global_atomic_cmpswap " in lds  # the flush / overflow into the global table


# ---- the constructed inputs of tests/test_gpu_groupby_hash_shapes.py do what their names say ----------------------
import numpy as np  # noqa: E402

from tests import groupby_hash_testlib as gl  # noqa: E402


@pytest.mark.parametrize("n", [4097, 1 << 20, 1 << 21, (1 << 21) + 3, 1 << 23, (1 << 26) - 5, (1 << 27) + 5, 160_000_001,
                               81920 * 2048, 81920 * 2048 + 1, (1 << 28) + 12345])
def test_restated_partition_geometry_matches_the_library(n):
    """the workspace of path b carries the partition step's meta words (k1 and parts): the restated jl_layout gives the
    library's byte count, so a changed kJlRowsPerPart or level split fails here and not silently in the shape tests"""
    ws = _capi.lib().dbhip_groupby_hash_workspace_bytes
    for mg in (0, 5000):
        assert ws(n, mg) == gl.workspace_bytes(n, mg), (n, mg)


def test_partition_step_sizes_reach_every_histogram_variant():
    want = {1 << 21: "one level", (1 << 21) + 3: "plain", 1 << 23: "plain", (1 << 26) - 5: "fused",
            (1 << 27) + 5: "fused16", 81920 * 2048: "fused16", 81920 * 2048 + 1: "digits", (1 << 28) + 12345: "digits"}
    assert {n: gl.hist_variant(n) for n in want} == want
    assert gl.hist_variant((1 << 28) + 12345, digits=False) == "plain"
    assert [n for n in want if gl.hist_variant(n) == "digits"] == [n for n, _ in gl.PARTITION_STEP_SIZES if _]


def test_hash_restatements():
    k = np.array([0, 1, 2, 0xDEADBEEF, gl.M32], dtype=np.uint32)
    assert np.array_equal(gl.fmix32_inv(gl.fmix32(k)), k)
    assert (gl.lds_home(k) >> 1 == gl.sub_home(k)).all() and (gl.lds_home(k) < 8192).all()
    assert np.array_equal(gl.global_home(k, 1 << 13), gl.lds_home(k))  # multiply-shift by a power of two: the top bits
    ref = gl.expect(k[[0, 1, 0, 4, 4]], np.array([gl.M32, 5, 2, 7, gl.M32], dtype=np.uint32))
    assert [a.tolist() for a in ref] == [[0, 1, gl.M32], [1, 5, 6], [2, 1, 2]]
    keys, vals, (uk, us, uc) = gl.pool_input(100000, 3, distinct=1000)
    want = gl.expect(keys, vals)
    assert np.array_equal(uk, want[0]) and np.array_equal(us, want[1]) and np.array_equal(uc, want[2])
    assert 0.005 < np.mean(keys == gl.M32) < 0.015 and uc.max() > 0.08 * keys.size


def _rows_of_partition(case, p):
    return case.keys[gl.pid(case.keys, case.facts["parts"]) == p]


@pytest.mark.parametrize("name", sorted(gl.CASES))
def test_construction(name):
    c = gl.CASES[name]()
    f = c.facts
    assert c.keys.dtype == np.uint32 and c.vals.dtype == np.uint32 and c.keys.size == c.vals.size
    if name.startswith("lds_home"):
        d = int(name.split("_")[2])
        assert 0 < c.max_groups <= gl.LDS_MAX_GROUPS  # path a
        shared = np.unique(c.keys[c.keys != gl.M32])
        assert shared.size == d + (1 if "extras" in name else 0) and shared.size > gl.PROBE
        assert (gl.lds_home(shared) == f["home"]).all()  # one home: past kGbhProbe keys the rows go global
        assert c.distinct <= c.max_groups
        if "extras" in name:
            assert (c.keys == gl.M32).mean() > 0.05 and np.bincount(np.unique(c.keys, return_inverse=True)[1]).max() > c.keys.size // 5
    elif name.startswith("sub_overflow") or name == "bound_global_only":
        p = f["partition"]
        assert f["parts"] == gl.part_layout(c.keys.size)[0]
        rows = _rows_of_partition(c, p)
        assert np.array_equal(np.unique(rows), np.unique(f["mine"]))
        assert np.unique(rows).size > gl.SUB_SLOTS  # more distinct keys than the sub-table holds
        if name.endswith("40000"):  # a giant, and each slice alone has more distinct keys than slots
            assert rows.size > gl.GIANT_ROWS and min(gl.GIANT_ROWS, rows.size - gl.GIANT_ROWS) > gl.SUB_SLOTS
            assert np.unique(rows).size == rows.size
        else:
            assert rows.size <= gl.GIANT_ROWS
        if name == "bound_global_only":
            others = np.unique(c.keys[gl.pid(c.keys, f["parts"]) != p])
            assert c.max_groups == c.distinct - 1 > gl.LDS_MAX_GROUPS  # path b, the bound one below the answer
            # what gbh_part_kernel can write directly stays below the bound: only the compaction passes it
            assert others.size + gl.SUB_SLOTS < c.max_groups
            assert np.bincount(gl.pid(others, f["parts"])).max() < gl.SUB_SLOTS // 8  # no other partition overflows
    elif name.startswith("sub_cluster"):
        mine = f["mine"]
        assert mine.size > gl.PROBE and np.unique(mine).size == mine.size
        assert (gl.pid(mine, f["parts"]) == f["partition"]).all() and (gl.sub_home(mine) == f["home"]).all()
        assert np.isin(mine, c.keys).all() and _rows_of_partition(c, f["partition"]).size <= gl.GIANT_ROWS
    elif name.startswith("giant_edge"):
        assert _rows_of_partition(c, f["partition"]).size == f["part_rows"] == int(name.split("_")[2])
        sizes = np.bincount(gl.pid(c.keys, f["parts"]), minlength=f["parts"])
        assert (np.delete(sizes, f["partition"]) <= gl.GIANT_ROWS).all()
    elif name.startswith("many_giants"):
        sizes = np.bincount(gl.pid(c.keys, f["parts"]), minlength=f["parts"])
        assert np.unique(f["partitions"]).size == f["hot"].size == 64
        for p, key, per in zip(f["partitions"], f["hot"], f["per"]):
            rows = _rows_of_partition(c, p)
            assert rows.size == per > gl.GIANT_ROWS and (rows == key).all()  # a giant of one key: crowds in every wave
        ff = name.endswith("_ff")
        assert ((c.keys == gl.M32).mean() > 0.01) == ff
        # 0xFFFFFFFF's rows are one more giant: its side sum comes out of gbh_giant_kernel
        assert (sizes > gl.GIANT_ROWS).sum() == 64 + ff
        assert (sizes[gl.pid(np.array([gl.M32], dtype=np.uint32), f["parts"])[0]] > gl.GIANT_ROWS) == ff
    elif name.startswith("crowd"):
        n = c.keys.size
        assert 0 < c.max_groups <= gl.LDS_MAX_GROUPS and n % 4 == 0  # path a, no tail rows
        assert c.distinct <= c.max_groups
        for st, comp, lanes in f["steps"]:
            wave = c.keys[gl.wave_rows(st, np.arange(64), comp)]
            on = wave == f["crowd_key"]
            assert on.sum() == f["lanes_on_key"] and np.array_equal(np.flatnonzero(on), np.sort(lanes))
            ff = f["ff_lanes"]
            assert (wave[:ff] == gl.M32).all() and wave[ff] == f["crowd_key"]  # the first active lane carries it
        assert len(f["steps"]) > 50
    else:
        raise AssertionError(f"no construction check for {name}")
