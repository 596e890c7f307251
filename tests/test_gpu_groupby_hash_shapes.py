"""dbhip_groupby_hash_u32 on inputs built against its hashes (tests/groupby_hash_testlib.py: every construction is
checked on the CPU by tests/test_groupby_hash_host.py): the LDS probe bound, sub-table overflow, giant-partition edges,
the crowd threshold, the bound met in every path, and path b at every histogram variant of the partition step.  Every
result is compared with an exact numpy reference."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from dwarf_bench_amd import ops  # noqa: E402
from tests import groupby_hash_testlib as gl  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _run(keys, vals, max_groups, counts=True):
    """-> keys, sums, counts (or None) in output order, as uint32"""
    k, s, c = ops.groupby_hash(_dev(keys), _dev(vals), max_groups or None, counts=counts)
    u = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)  # noqa: E731
    return u(k), u(s), u(c)


def _agree(got, want, counts=True):
    k, s, c = got
    o = np.argsort(k, kind="stable")
    assert np.array_equal(k[o], want[0]), "keys"
    assert np.array_equal(s[o], want[1]), "sums"
    if counts:
        assert np.array_equal(c[o], want[2]), "counts"
    else:
        assert c is None


def _check(case, max_groups=None, counts=True):
    got = _run(case.keys, case.vals, case.max_groups if max_groups is None else max_groups, counts)
    _agree(got, gl.expect(case.keys, case.vals), counts)
    return got


def _tail_holds(out_keys, mine, need, slack=256):
    """path evidence, not the contract: gbh_part_kernel writes its groups first and gbh_compact_kernel appends the global
    table's behind them, so `need` keys that went through the global table sit among the last need + slack rows
    (slack: keys of other partitions that met a 64-step cluster by chance)"""
    tail = out_keys[out_keys != gl.M32][-(need + slack):]
    return int(np.isin(tail, mine).sum()) >= need


@pytest.mark.parametrize("name", ["lds_home_65", "lds_home_100", "lds_home_4096", "lds_home_100_extras"])
def test_lds_probe_overflow(name):
    """path a, LDS probe overflow: more than kGbhProbe distinct keys on one LDS home, so a workgroup's rows of the keys
    past the 64th slot go to the global table (gbh_add<true> -> gbh_global_add); with 0xFFFFFFFF rows and a hot key
    (the side sum, the crowd) in the same input.  Bounds: exactly the distinct count, and path a's largest."""
    case = gl.CASES[name]()
    _check(case)  # max_groups = the distinct count (plus 0xFFFFFFFF): the exact bound
    _check(case, max_groups=gl.LDS_MAX_GROUPS)
    _check(case, counts=False)


@pytest.mark.parametrize("n", [1 << 21, 1 << 23])
@pytest.mark.parametrize("d", [4097, 6000])
def test_sub_table_overflow(n, d):
    """path b, sub-table overflow: one partition (of 1024 partitions, one scatter level; of 4096, two) with more distinct
    keys than its kGbhSubSlots-slot sub-table: the keys that find no slot are added to the global table and appended by
    gbh_compact_kernel behind the directly written groups"""
    case = gl.CASES[f"sub_overflow_{n}_{d}"]()
    k, _, _ = _check(case)
    assert _tail_holds(k, case.facts["mine"], d - gl.SUB_SLOTS)


@pytest.mark.parametrize("n", [1 << 21, 1 << 23])
def test_sub_table_probe_cluster(n):
    """path b, sub-table probe overflow: 80 keys of one partition on one sub-table home; past kGbhProbe steps they go to
    the global table although the sub-table is half empty"""
    case = gl.CASES[f"sub_cluster_{n}"]()
    k, _, _ = _check(case)
    assert _tail_holds(k, case.facts["mine"], case.facts["mine"].size - gl.PROBE)


@pytest.mark.parametrize("n", [1 << 21, 1 << 23])
def test_giant_slices_overflow_the_sub_table(n):
    """path b, giant partition whose slices overflow: 40000 distinct keys in one partition (two slices, 32768 and 7232
    rows, each with more distinct keys than sub-table slots): gbh_giant_kernel's slices flush into the global table,
    their overflow goes there directly"""
    case = gl.CASES[f"sub_overflow_{n}_40000"]()
    k, _, _ = _check(case)
    assert _tail_holds(k, case.facts["mine"], case.facts["mine"].size)  # a giant's keys all come out of the compaction
    _check(case, counts=False)


@pytest.mark.parametrize("rows", [gl.GIANT_ROWS, gl.GIANT_ROWS + 1])
def test_giant_partition_edge(rows):
    """path b, the giant threshold: a partition of exactly kGbhGiantRows rows stays on gbh_part_kernel, one row more is
    listed and cut into two slices (32768 + 1 rows) by gbh_giant_kernel"""
    case = gl.CASES[f"giant_edge_{rows}"]()
    _check(case)
    _check(case, counts=False)


@pytest.mark.parametrize("name", ["many_giants", "many_giants_ff"])
def test_many_giants(name):
    """path b, several giants: 64 partitions of one hot key each (two or three slices each, a crowd in every wave), one
    more of 0xFFFFFFFF rows whose side sum is taken in the slices: every listed giant is sliced, none is lost"""
    case = gl.CASES[name]()
    _check(case)
    _check(case, counts=False)


@pytest.mark.parametrize("name", ["crowd_15", "crowd_16", "crowd_17", "crowd_16_after_ff"])
def test_crowd_threshold(name):
    """path a, the crowd shortcut of gbh_wave_row: one key on 15 (below kGbhCrowd), 16 and 17 of the 64 rows of a wave
    step, the wave's first active key; and on 16 rows whose first active lane follows lanes of 0xFFFFFFFF"""
    case = gl.CASES[name]()
    _check(case)


_PINNED = r"""
import sys
import numpy as np, torch
from dwarf_bench_amd import ops
from tests import groupby_hash_testlib as gl
bad = []
for name in sys.argv[1:]:
    case = gl.CASES[name]()
    k, s, c = ops.groupby_hash(torch.from_numpy(case.keys.view(np.int32)).cuda(),
                               torch.from_numpy(case.vals.view(np.int32)).cuda(), case.max_groups or None)
    k, s, c = (t.cpu().numpy().view(np.uint32) for t in (k, s, c))
    o = np.argsort(k, kind="stable")
    want = gl.expect(case.keys, case.vals)
    if not all(np.array_equal(a, b) for a, b in zip((k[o], s[o], c[o]), want)):
        bad.append(name)
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("path", ["lds", "part", "global"])
def test_constructed_inputs_on_every_path(path):
    """every constructed input with DBHIP_GBH_PATH pinned (read once: a fresh process per value) — the LDS probe bound,
    sub-table overflow, giants and crowds through whichever path is pinned"""
    names = [n for n in gl.CASES if n != "bound_global_only"]
    r = subprocess.run([sys.executable, "-c", _PINNED] + names, capture_output=True, text=True, timeout=900,
                       env={**os.environ, "DBHIP_GBH_PATH": path}, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _bounded(keys, vals, bound):
    """run with guard words behind all three output columns (the pattern of test_more_keys_than_the_bound) -> status,
    groups, keys, sums, counts of the rows written"""
    n = keys.size
    plan = ops.GroupByHash(n, bound)
    guard = 0x5A5A5A5A
    for name in ("keys", "sums", "counts"):
        setattr(plan, name, torch.full((bound + 64,), guard, dtype=torch.int32, device="cuda"))
    plan.launch(_dev(keys), _dev(vals))
    torch.cuda.synchronize()
    st = ops.workspace_status(plan.ws)
    g = int(plan.groups.item())
    for name in ("keys", "sums", "counts"):
        assert (getattr(plan, name)[bound:].cpu().numpy() == guard).all(), name
    u = lambda t: t[:g].cpu().numpy().view(np.uint32)  # noqa: E731
    return st, g, u(plan.keys), u(plan.sums), u(plan.counts)


@pytest.mark.parametrize("name,bound", [("lds_home_100", 65), ("lds_home_100_extras", 100), ("crowd_16", 150),
                                        ("sub_overflow_2097152_6000", 2_000_000), ("sub_cluster_2097152", 5000),
                                        ("many_giants_ff", 100000), ("giant_edge_32769", 4097)])
def test_bound_on_constructed_inputs(name, bound):
    """the max_groups bound on inputs that overflow the LDS tables, the sub-tables and the giants' slices: fewer
    max_groups than distinct keys -> DBHIP_DEV_TABLE_FULL, *out_groups == max_groups, nothing written past the bound,
    every key written distinct and one of the input's"""
    case = gl.CASES[name]()
    assert case.distinct > bound
    st, g, k, _, _ = _bounded(case.keys, case.vals, bound)
    assert st & ops.DEV_TABLE_FULL and g == bound
    assert np.unique(k).size == g and np.isin(k, case.keys).all()


def test_bound_passed_only_by_global_table_rows():
    """the bound passed in gbh_compact_kernel alone: the directly written groups stay below it, the global table's
    (one partition's overflow) pass it by one.  No table filled early, so every row written is exact."""
    case = gl.CASES["bound_global_only"]()
    st, g, k, s, c = _bounded(case.keys, case.vals, case.max_groups)
    assert st & ops.DEV_TABLE_FULL and g == case.max_groups
    wk, ws, wc = gl.expect(case.keys, case.vals)
    at = np.searchsorted(wk, k)
    assert np.unique(k).size == g and np.array_equal(wk[at], k)
    assert np.array_equal(ws[at], s) and np.array_equal(wc[at], c)
    assert np.setdiff1d(wk, k).size == 1 and np.isin(np.setdiff1d(wk, k), case.facts["mine"]).all()


# ---- path b at every histogram variant of the partition step --------------------------------------------------------
def _fits(n):
    need = ops._capi.lib().dbhip_groupby_hash_workspace_bytes(n, 0) + 5 * 4 * n + (1 << 30)  # inputs, outputs, slack
    free, _ = torch.cuda.mem_get_info()
    if need > free:
        pytest.skip(f"{n} rows need {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free")


_DIGITS_OFF = r"""
import sys
import numpy as np, torch
from dwarf_bench_amd import ops
from tests import groupby_hash_testlib as gl
n = int(sys.argv[1])
keys, vals, want = gl.pool_input(n, n)
k, s, c = ops.groupby_hash(torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda())
del keys, vals
k, s, c = (t.cpu().numpy().view(np.uint32) for t in (k, s, c))
o = np.argsort(k, kind="stable")
ok = all(np.array_equal(a, b) for a, b in zip((k[o], s[o], c[o]), want))
print("OK" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("n,digits_off", gl.PARTITION_STEP_SIZES)
def test_partition_step_variants(n, digits_off):
    """path b through every histogram of jl_partition_side (gl.hist_variant: one scatter level, plain, fused, fused16,
    the 16-bit digit column), the vals column riding where the join carries row ids; about 2^20 pool keys, a hot key on
    10 % of the rows and 0xFFFFFFFF on 1 %.  At the digit-column sizes once more with DBHIP_JL_DIGITS=0."""
    _fits(n)
    keys, vals, want = gl.pool_input(n, n)
    _agree(_run(keys, vals, 0), want)
    del keys, vals
    if digits_off:
        torch.cuda.empty_cache()
        r = subprocess.run([sys.executable, "-c", _DIGITS_OFF, str(n)], capture_output=True, text=True, timeout=900,
                           env={**os.environ, "DBHIP_JL_DIGITS": "0"}, cwd=str(ROOT))
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
