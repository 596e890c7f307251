"""The C-ABI library on a CPU-only box (no compute calls here: there is no GPU): workspace queries, argument errors
and the join's partition geometry.  tests/test_capi_headers.py holds the headers, the bindings and the exports together."""
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi

ROOT = Path(__file__).resolve().parents[1]


def test_workspace_queries_need_no_gpu():
    lib = _capi.lib()
    assert lib.dbhip_copy_if_lt_i32_workspace_bytes(1 << 28) >= 256 + (1 << 28) // 8192 * 8
    assert lib.dbhip_radix_sort_workspace_bytes(1 << 24, 8) % 256 == 0
    assert lib.dbhip_radix_sort_workspace_bytes(1 << 24, 5) == 0
    assert lib.dbhip_groupby_sum_u32_workspace_bytes(1 << 26, 1 << 16) >= 128 * (1 << 16) * 4
    assert lib.dbhip_join_workspace_bytes(1 << 20) >= 20 * (1 << 20)  # 12-byte table slots per row + 8-byte (key, row id) pairs
    assert lib.dbhip_ujoin_workspace_bytes(1000) >= 2 * 2048 * 4


WORKSPACE_SIZES = (0, 1, 2048, 2049, 65535, 65536, (1 << 18) - 1, 1 << 18, 1 << 21, (1 << 21) + 1, (1 << 24) + 5, 1 << 26,
                   (1 << 26) + 1, 81920 * 2048, 81920 * 2048 + 1, 1 << 30, 1 << 31)


def _workspace_table(lib):
    """every workspace query whose answer depends on the partitioner's geometry or meta array, at the row counts where
    the code changes branch: one or two scatter levels, giants on or off, each histogram variant, the row limit"""
    table = {}
    for n in WORKSPACE_SIZES:
        row = {"join": lib.dbhip_join_workspace_bytes(n), "ujoin": lib.dbhip_ujoin_workspace_bytes(n),
               "radix n x n": lib.dbhip_join_radix_workspace_bytes(n, n),
               "radix n x n/3+1": lib.dbhip_join_radix_workspace_bytes(n, n // 3 + 1),
               "groupby_hash any": lib.dbhip_groupby_hash_workspace_bytes(n, 0),
               "groupby_hash 4096": lib.dbhip_groupby_hash_workspace_bytes(n, 4096)}
        for parts in (1, 8, 1024):  # 1024: pjoin.hip kPjMaxParts, the largest allowed
            row[f"pjoin_partition {parts}"] = lib.dbhip_pjoin_partition_workspace_bytes(n, parts)
        table[str(n)] = row
    return table


def test_workspace_sizes_are_those_of_the_undivided_partitioner():
    """tests/golden/workspace_bytes.json: what the library answered before the partitioner became a unit of its own
    (csrc/partition.hip, one description of its meta array) — recorded from a CPU build of that commit with
    _workspace_table; a caller's allocation must neither grow nor fall short"""
    import json
    want = json.loads((ROOT / "tests" / "golden" / "workspace_bytes.json").read_text())
    assert sorted(want) == sorted(str(n) for n in WORKSPACE_SIZES)
    got = _workspace_table(_capi.lib())
    assert all(row["join"] > 0 and row["pjoin_partition 1024"] > 0 for row in got.values())  # real sizes, not refusals
    for n in want:
        assert got[n] == want[n], n


def test_argument_errors_are_reported_without_a_device():
    lib = _capi.lib()
    # null pointers / bad sizes are rejected on the host before any HIP call
    assert lib.dbhip_copy_if_lt_i32(None, 16, 5, None, None, None, 0, None) == -1
    assert lib.dbhip_radix_sort_u32(None, None, 16, 7, None, 0, None) == -1
    assert lib.dbhip_groupby_sum_u32(None, None, 16, 4, None, None, 0, None) == -1


def test_product_has_no_oracle_import():
    """The product package must never import oracle/ (no CPU fallback)."""
    for py in (ROOT / "dwarf_bench_amd").rglob("*.py"):
        src = py.read_text()
        assert "pyoracle" not in src and "import oracle" not in src and "from oracle" not in src, py


@pytest.fixture(scope="module")
def layout_tool(tmp_path_factory):
    """tests/cpp/join_layout_check.cpp built with hipcc against join_common.hpp (runs without a GPU)"""
    import subprocess
    exe = tmp_path_factory.mktemp("layout") / "join_layout_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", str(ROOT / "dwarf_bench_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "join_layout_check.cpp"), "-o", str(exe)], check=True, timeout=600)
    return exe


def test_join_partition_geometry_for_every_row_count(layout_tool):
    """join_common.hpp jl_layout over row counts up to 2^31, for the build's and the radix join's rows per partition:
    at most 1024 level-0 buckets, a power-of-two level-1 fan-out, partitions that hold their rows (tests/cpp/
    join_layout_check.cpp; a geometry with 1171 level-0 buckets at 2^30 rows once made that join take a minute)"""
    import subprocess
    r = subprocess.run([str(layout_tool)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "join layout ok" in r.stdout, r.stdout[-2000:]


def _compiled_plans(layout_tool, pairs, env=None):
    """join_layout_check with "n_side:n_build" arguments -> {(n_side, n_build, rows per partition): ((parts, k1, k2,
    variant, t0, t1) as compiled, the meta array's word offsets and total)}"""
    import os
    import subprocess
    r = subprocess.run([str(layout_tool)] + [f"{a}:{b}" for a, b in pairs], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 2 * len(pairs)
    out = {}
    for line in lines:
        f = line.split()
        n_side, n_build, rows, parts, k1, k2 = map(int, f[:6])
        out[(n_side, n_build, rows)] = ((parts, k1, k2, f[6].replace("_", " "), int(f[7]), int(f[8])), tuple(map(int, f[9:])))
    assert len(out) == len(lines)
    return out


def test_side_plan_restates_the_compiled_geometry(layout_tool):
    """tests/join_testlib.side_plan — (parts, k1, k2) AND the histogram variant and tile shapes — against jl_layout and
    jl_side_plan (csrc/partition.hpp) as compiled, at every size the layout tests use, at the probe sides of the radix
    join laid out by ANOTHER column's geometry (with and without the fused histograms' scratch), and +-3 rows around the
    partition counts where the histogram variant changes (8192: fused, 32768: fused16, 81920: the digit column), for both
    rows per partition; under the forced tile shapes and DBHIP_JL_DIGITS=0 too; and the variants and tile shapes the layout
    tests rely on.  The meta array's size as compiled is the one groupby_hash_testlib.workspace_bytes assumes."""
    from tests import join_testlib as jt
    per_part = (jt.JL_ROWS_PER_PART, jt.JR_ROWS_PER_PART)
    sizes = set(jt.layout_sizes())
    for parts in (8192, 32768, 81920):
        for rows in per_part:
            sizes.update(parts * rows + d for d in range(-3, 4))
    pairs = {(n, n) for n in sizes}
    for n, radix, _ in jt.LAYOUT_TABLE:
        large, small = jt.radix_probe_sizes(n)
        pairs.update(((large, n), (small, n), (128 * radix[0] - 1, n), (128 * radix[0], n)))
    pairs.add((jt.HEADLINE_PROBE, jt.HEADLINE_BUILD))
    pairs = sorted(pairs)
    compiled = _compiled_plans(layout_tool, pairs)
    assert len(compiled) == 2 * len(pairs)
    for (n_side, n_build, rows), (plan, meta) in compiled.items():
        assert (rows in per_part) and jt.side_plan(n_side, n_build, rows) == plan, (n_side, n_build, rows, plan)
        parts, k1 = plan[:2]
        assert meta[-1] == (2 * 64 + 2) * k1 + 2 + 3 * parts + 1 and list(meta) == sorted(set(meta)) and meta[0] == 0
    forced = [(1 << 20, 1 << 20), ((1 << 26) + 5, (1 << 26) + 5), (170_000_001, 170_000_001), (jt.HEADLINE_PROBE, jt.HEADLINE_BUILD)]
    for t0, t1 in ((0, 2), (1, 0), (None, 1), (2, None)):
        env = {k: str(v) for k, v in (("DBHIP_JL_T0", t0), ("DBHIP_JL_T1", t1)) if v is not None}
        for (n_side, n_build, rows), (plan, _) in _compiled_plans(layout_tool, forced, env).items():
            assert jt.side_plan(n_side, n_build, rows, t0, t1) == plan, (t0, t1, n_side, n_build, rows, plan)
    for (n_side, n_build, rows), (plan, _) in _compiled_plans(layout_tool, forced, {"DBHIP_JL_DIGITS": "0"}).items():
        assert jt.side_plan(n_side, n_build, rows, digits=False) == plan, (n_side, n_build, rows, plan)
    # the variant changes exactly there (parts is a multiple of k2 = 64 below 2^26 rows: 8128 partitions, then 8192)
    for rows in per_part:
        for last, below, above in ((8128, "plain", "fused"), (32768, "fused", "fused16"), (81920, "fused16", "digits")):
            got = [jt.side_plan(n, n, rows)[3] for n in (last * rows, last * rows + 1)]
            assert got == [below, above], (rows, last, got)
    for n, radix, hashed in jt.LAYOUT_TABLE:
        assert jt.side_plan(n, n, jt.JR_ROWS_PER_PART) == radix and jt.side_plan(n, n, jt.JL_ROWS_PER_PART) == hashed
        large, small = jt.radix_probe_sizes(n)
        parts = radix[0]
        assert large >= 128 * parts and jt.side_plan(large, n, jt.JR_ROWS_PER_PART)[3] == radix[3]
        want_small = "plain" if radix[3] in ("fused", "fused16") else radix[3]
        assert jt.side_plan(small, n, jt.JR_ROWS_PER_PART)[3] == want_small
        assert jt.side_plan(128 * parts - 1, n, jt.JR_ROWS_PER_PART)[3] == want_small  # one row short of the scratch
    hb = jt.HEADLINE_BUILD
    assert (jt.side_plan(hb, hb, jt.JR_ROWS_PER_PART), jt.side_plan(hb, hb, jt.JL_ROWS_PER_PART)) == jt.HEADLINE_PLANS
    assert jt.side_plan(jt.HEADLINE_PROBE, hb, jt.JR_ROWS_PER_PART)[3:] == ("digits", 2, 1)
    assert [jt.side_plan(1 << 20, 1 << 20, 1792, t0, t1)[4:] for t0, t1 in ((0, 2), (1, 0), (None, 1))] == [(0, 1), (1, 0), (2, 1)]


def test_guarded_columns_start_where_they_say():
    """join_testlib.guarded on the host: the view starts offset words past a 16-byte boundary, the guards around it
    are checked by assert_guards, and a write into one is caught"""
    import torch
    from tests import join_testlib as jt
    for off in range(6):
        base, view = jt.guarded(37, off, 0x5A5A5A5A, device="cpu")
        assert view.numel() == 37 and (view.data_ptr() - base.data_ptr()) // 4 == jt.GUARD_WORDS + off
        view.fill_(7)
        jt.assert_guards(base, view, 0x5A5A5A5A)
        for at in (jt.GUARD_WORDS + off - 1, jt.GUARD_WORDS + off + 37):
            base[at] = 1
            with pytest.raises(AssertionError):
                jt.assert_guards(base, view, 0x5A5A5A5A)
            base[at] = 0x5A5A5A5A
    assert torch.equal(view, torch.full((37,), 7, dtype=torch.int32))


def test_radix_join_refuses_probe_sides_its_32_bit_row_indices_cannot_walk():
    """The radix join's fused kernel steps through a partition's probe rows with 32-bit indices, 4 * 512 rows at a time:
    n_probe above 2^32 - 2048 is DBHIP_EINVAL in the partition and match calls (include/dbhip.h).  The workspace passed
    is one byte short of what the sizes need, so a call the bound lets through stops at the workspace check
    (DBHIP_EWORKSPACE) before it looks for a device: the fake pointers reach nothing on a box with a GPU either."""
    lib = _capi.lib()
    bound = (1 << 32) - 2048
    fake = 1 << 20  # 256-byte aligned, never dereferenced
    n_build = 1000
    for n_probe, want in ((bound + 1, -1), (bound, -2), ((1 << 32) - 1, -1), (1 << 32, -1)):
        short = lib.dbhip_join_radix_workspace_bytes(n_build, n_probe) - 1
        assert lib.dbhip_join_radix_partition_u32(1, fake, None, n_probe, n_build, n_probe, fake, short, None) == want, n_probe
        assert lib.dbhip_join_radix_partition_u32(0, fake, None, n_build, n_build, n_probe, fake, short, None) == want, n_probe
        assert lib.dbhip_join_radix_match_u32(n_build, n_probe, fake, fake, fake, fake, fake, short, None) == want, n_probe
