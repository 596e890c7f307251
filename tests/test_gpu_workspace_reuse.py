"""One plan, one workspace, several inputs.  Every plan of ops owns a workspace and is meant to be reused, and the C
ABI promises nothing about a workspace's contents between calls (the C++ dwarfs run every iteration on one hipMalloc'd
buffer; the multi-GPU engine runs every step and sub-join on one that grows and is never cleared).  Each test here runs
one plan through inputs chosen to leave state behind for the next — spilled partitions (more distinct keys than a
sub-table has slots), giant partitions (hot keys), different internal paths — and checks every result against numpy or
the oracle.  The poisoned cases fill the workspace with 0xFF bytes or random bytes before the first call."""
import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests.join_testlib import (check_grouped_join, check_radix_result, dev, keys_of_partition, keys_of_partition_of,
                                radix_parts)

pytestmark = pytest.mark.gpu

POISONS = ["zeros", "0xff", "random"]


def _poison(ws: torch.Tensor, how: str) -> None:
    if how == "0xff":
        ws.fill_(0xFF)
    elif how == "random":
        g = torch.Generator(device=ws.device)
        g.manual_seed(1234)
        ws.copy_(torch.randint(0, 256, ws.shape, dtype=torch.uint8, device=ws.device, generator=g))


def _crowded(n, mine, per_key, rng, seed=42):
    """n uniform keys in [0, n), of which len(mine) * per_key rows carry the keys `mine` (per_key rows each)"""
    build = po.gen_uniform_u32(n, seed, 0, n - 1)
    build[: mine.size * per_key] = np.repeat(mine, per_key)
    return rng.permutation(build)


def _probe(m, n, hits, rng, seed=43):
    """m probe rows: uniform keys in [0, n), every third row one of `hits`"""
    probe = po.gen_uniform_u32(m, seed, 0, n - 1)
    for i, h in enumerate(hits):
        probe[i::3 * len(hits)] = h[rng.integers(0, h.size, probe[i::3 * len(hits)].size)]
    return probe


# ---- one-to-many join (ops.HashJoin) --------------------------------------------------------------------------------
# Probe sides of 2^22 rows: every probe thread walks several rows, so a thread that meets a spilled partition's marked
# sub-table goes over rows of other partitions again (jl_probe_kernel's second pass through the spill directory).
M = 1 << 22


@pytest.mark.parametrize("poison", POISONS)
def test_hash_join_spilled_partitions_move_below_2_18(poison):
    """below 2^18 build rows the build kernel's workgroup builds a spilled partition's table at once: spill partition 1,
    then partition 5 (probes of 1's keys now go to an ordinary sub-table), then uniform keys, then partition 1 again"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(5)
    n = 1 << 16
    p1, p5 = keys_of_partition(n, 1, 4000), keys_of_partition(n, 5, 4000)
    plan = ops.HashJoin(n, M)
    _poison(plan.ws, poison)
    check_grouped_join(_crowded(n, p1[:3500], 1, rng), _probe(M, n, [p1], rng), plan)
    check_grouped_join(_crowded(n, p5, 9, rng), _probe(M, n, [p1, p5], rng), plan)
    if poison == "zeros":
        check_grouped_join(po.gen_uniform_u32(n, 44, 0, n - 1), _probe(M, n, [p1, p5], rng), plan)
        check_grouped_join(_crowded(n, p1[:3500], 3, rng), _probe(M, n, [p1, p5], rng), plan)


@pytest.mark.parametrize("poison", POISONS)
def test_hash_join_spills_and_giants_from_2_18(poison):
    """from 2^18 build rows spilled partitions are listed and built at the end of jl_giant_ids, and partitions above
    32768 rows are giants: spill partition 2; then make it a giant that does not spill (one hot key); then a giant
    that spills (3500 keys x 20 rows); then uniform keys; then spill partition 7 with probes of 2's keys"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(7)
    n = 1 << 18
    p2, p7 = keys_of_partition(n, 2, 3800), keys_of_partition(n, 7, 3800)
    plan = ops.HashJoin(n, M)
    _poison(plan.ws, poison)
    check_grouped_join(_crowded(n, p2[:3500], 1, rng), _probe(M, n, [p2], rng), plan)
    giant = _crowded(n, p2[:1], 40000, rng)
    check_grouped_join(giant, _probe(M, n, [p2, p2[:1]], rng), plan)
    if poison != "zeros":
        return
    check_grouped_join(_crowded(n, p2[:3500], 20, rng), _probe(M, n, [p2], rng), plan)
    check_grouped_join(po.gen_uniform_u32(n, 45, 0, n - 1), _probe(M, n, [p2, p7], rng), plan)
    check_grouped_join(_crowded(n, p7[:3500], 1, rng), _probe(M, n, [p2, p7], rng), plan)
    check_grouped_join(giant, _probe(M, n, [p2, p7, p2[:1]], rng), plan)


# ---- radix join (ops.RadixJoin) --------------------------------------------------------------------------------------
def _radix(plan, build, probe, matches=1):
    plan.partition_build(dev(build))
    plan.partition_probe(dev(probe))
    for _ in range(matches):
        plan.match()
        check_radix_result(build, probe, plan.result())


@pytest.mark.parametrize("poison", POISONS)
def test_radix_join_match_repeats_and_spills_move_below_2_18(poison):
    """both sides below 2^18 rows (the fused kernel spills inline): a partition of 36000 rows and 4000 distinct keys
    matched three times on one partitioned pair — every match takes its spill table from the pool afresh — then a
    spill of another partition, then uniform keys"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(11)
    nb, npr = 1 << 16, (1 << 17) + 77
    parts = radix_parts(nb)
    pa, pb = keys_of_partition_of(parts, parts // 3, 4300), keys_of_partition_of(parts, parts // 3 + 4, 4300)
    plan = ops.RadixJoin(nb, npr)
    _poison(plan.ws, poison)
    _radix(plan, _crowded(nb, pa[:4000], 9, rng), _probe(npr, nb, [pa], rng), matches=3)
    _radix(plan, _crowded(nb, pb[:3500], 1, rng), _probe(npr, nb, [pa, pb], rng), matches=2)
    if poison == "zeros":
        _radix(plan, po.gen_uniform_u32(nb, 46, 0, nb - 1), _probe(npr, nb, [pa, pb], rng))


@pytest.mark.parametrize("poison", POISONS)
def test_radix_join_spills_giants_and_repeated_matches_from_2_18(poison):
    """2^18 build rows, 2^20 probe rows: spilled partitions are listed for jl_giant_ids, giants exist on either side.
    A giant that spills (3500 keys x 20 rows) matched three times; the same partition then a giant through a hot build
    key and a hot probe key of 40000 rows, neither spilling; then a plain spill of it; then uniform keys and a spill of
    another partition"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(13)
    nb, npr = 1 << 18, 1 << 20
    parts = radix_parts(nb)
    pa, pb = keys_of_partition_of(parts, parts // 5, 3800), keys_of_partition_of(parts, parts // 5 + 9, 3800)
    plan = ops.RadixJoin(nb, npr)
    _poison(plan.ws, poison)
    _radix(plan, _crowded(nb, pa[:3500], 20, rng), _probe(npr, nb, [pa], rng), matches=3)
    hot_probe = _probe(npr, nb, [pa], rng)
    hot_probe[rng.permutation(npr)[:40000]] = pa[1]
    _radix(plan, _crowded(nb, pa[:1], 40000, rng), hot_probe, matches=2)
    if poison != "zeros":
        return
    _radix(plan, _crowded(nb, pa[:3500], 1, rng), _probe(npr, nb, [pa], rng), matches=2)
    _radix(plan, po.gen_uniform_u32(nb, 47, 0, nb - 1), _probe(npr, nb, [pa, pb], rng))
    _radix(plan, _crowded(nb, pb[:3500], 1, rng), _probe(npr, nb, [pa, pb], rng), matches=2)


# ---- unique-key payload join (ops.UniqueJoin) ------------------------------------------------------------------------
def _unique_crowd(n, mine, rng):
    rest = np.setdiff1d(po.gen_unique_sorted_u32(2 * n, 11), mine)[: n - mine.size]
    ak = np.concatenate([mine, rest]).astype(np.uint32)
    assert np.unique(ak).size == n
    return rng.permutation(ak)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("n", [1 << 16, 1 << 18])
def test_unique_join_spilled_partitions_move(n, poison):
    """spill partition 2 (9000 of its keys), then partition 6 with probes of 2's keys, then keys without a crowd; rows
    against the oracle's unique-key join"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(17)
    m = n // 2 + 13
    p2, p6 = keys_of_partition(n, 2, 9400), keys_of_partition(n, 6, 9400)
    plan = ops.UniqueJoin(n, m)
    _poison(plan.ws, poison)
    builds = [_unique_crowd(n, p2[:9000], rng), _unique_crowd(n, p6[:9000], rng), _unique_crowd(n, p6[:0], rng)]
    for ak in builds if poison == "zeros" else builds[:2]:
        bk = np.unique(np.concatenate([p2[rng.integers(0, p2.size, m // 4)], p6[rng.integers(0, p6.size, m // 4)],
                                       po.gen_unique_sorted_u32(m, 12)]))[:m].astype(np.uint32)
        bk = rng.permutation(np.pad(bk, (0, m - bk.size), constant_values=0))
        av, bv = po.gen_uniform_u32(n, 13, 0, 2**32 - 2), po.gen_uniform_u32(m, 14, 0, 2**32 - 2)
        plan.build(dev(ak), dev(av))
        plan.probe(dev(bk), dev(bv))
        ok, o1, o2 = (t.cpu().numpy().view(np.uint32) for t in plan.result())
        ek, e1, e2 = po.ujoin(ak, av, bk, bv)
        assert np.array_equal(ok, ek) and np.array_equal(o1, e1) and np.array_equal(o2, e2)


# ---- every other plan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", POISONS)
def test_copy_if_plan_reused_across_variants_and_alignments(poison):
    """sparse, dense, sparse again; an unaligned source (the chunked path without 16-byte loads); other filters"""
    from dwarf_bench_amd import ops
    n = 250007
    plan = ops.CopyIfLt(n)
    _poison(plan.ws, poison)
    base = ops.gen_uniform_u32(n + 1, 42, 1, 10000)
    cases = [(base[:n], 5001, False), (base[:n], 5001, True), (base[1:], 37, False), (base[1:], 9000, True),
             (base[:n], 5, False)]
    for src, filt, dense in cases:
        plan.launch(src, filt, dense=dense)
        assert np.array_equal(plan.result().cpu().numpy(), po.copy_if_lt(src.cpu().numpy(), filt))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("bits", [4, 8])
def test_radix_sort_plan_reused_across_signedness_and_distributions(bits, poison):
    from dwarf_bench_amd import ops
    n = 300007
    plan = ops.RadixSort(n, bits)
    _poison(plan.ws, poison)
    rng = np.random.default_rng(19)
    inputs = [(po.gen_uniform_u32(n, 1, 0, 2**32 - 1), False),
              (rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32).view(np.uint32), True),
              (np.repeat(np.array([7, 7 << 24, 0xFFFFFFFF], np.uint32), -(-n // 3))[:n], False),
              (po.gen_uniform_u32(n, 2, 0, 100), True)]
    for host, signed in inputs:
        keys = dev(host)
        plan.launch(keys, signed)
        want = np.sort(host.view(np.int32)) if signed else np.sort(host)
        assert ops.workspace_status(plan.ws) == 0
        got = keys.cpu().numpy()
        assert np.array_equal(got if signed else got.view(np.uint32), want)


@pytest.mark.parametrize("poison", POISONS)
def test_group_by_plan_reused_across_table_modes_and_phases(poison):
    """2^25 rows, 2^16 groups: small values take the packed table (header mode 1), full-range values the wide one
    (mode 2); then the same plan through partial + merge with 4 private tables and with the library's choice"""
    from dwarf_bench_amd import ops
    n, groups = 1 << 25, 1 << 16
    plan = ops.GroupBySum(n, groups)
    _poison(plan.ws, poison)
    keys = ops.gen_uniform_u32(n, 42, 0, groups - 1)
    hk = keys.cpu().numpy().view(np.uint32)
    for (vlo, vhi), mode in (((1, 10000), 1), ((0, 2**32 - 1), 2)):
        vals = ops.gen_uniform_u32(n, 43, vlo, vhi)
        plan.launch(keys, vals)
        got = plan.result().cpu().numpy().view(np.uint32)
        assert int(plan.ws[4:8].view(torch.int32).item()) == mode
        assert np.array_equal(got, po.groupby_sum(hk, vals.cpu().numpy().view(np.uint32), groups))
    k2 = ops.gen_uniform_u32(n, 44, 0, 999)
    v2 = ops.gen_uniform_u32(n, 45, 1, 10000)
    want = po.groupby_sum(k2.cpu().numpy().view(np.uint32), v2.cpu().numpy().view(np.uint32), groups)
    for executors in (4, 0):
        plan.partial(k2, v2, executors)
        plan.merge(executors)
        assert np.array_equal(plan.result().cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("poison", POISONS)
def test_bitmask_table_reused_after_reset(poison):
    from dwarf_bench_amd import ops
    size = 1 << 16
    t = ops.BitmaskTable(size, hash_kind=1, seed=421)
    _poison(t.ws, poison)
    a = po.gen_unique_sorted_u32(30000, 3)
    b = np.setdiff1d(po.gen_unique_sorted_u32(30000, 4), a).astype(np.uint32)
    for keys, other in ((a, b), (b, a)):
        t.reset()
        vals = keys ^ np.uint32(0x5A5A5A5A)
        t.insert(dev(keys), dev(vals))
        t.check()
        got, found = t.lookup(dev(keys))
        assert bool((found == 1).all()) and np.array_equal(got.cpu().numpy().view(np.uint32), vals)
        _, found = t.lookup(dev(other))
        assert not bool(found.any())  # nothing of the previous fill is left


@pytest.mark.parametrize("poison", POISONS)
def test_cuckoo_table_reused_after_reset(poison):
    from dwarf_bench_amd import ops
    n = 1 << 18
    t = ops.CuckooTable(4 * n, hash_kind=2, seeds=ops.cuckoo_seed_pair(0, 0))
    _poison(t.ws, poison)
    a = po.gen_unique_sorted_u32(n, 21)
    b = np.setdiff1d(po.gen_unique_sorted_u32(n, 22), a).astype(np.uint32)
    for keys, other in ((a, b), (b, a)):
        t.reset()
        vals = keys ^ np.uint32(0x3C3C3C3C)
        t.insert(dev(keys), dev(vals))
        assert t.status() == ops.DEV_OK
        got, found = t.lookup(dev(keys))
        assert bool((found == 1).all()) and np.array_equal(got.cpu().numpy().view(np.uint32), vals)
        _, found = t.lookup(dev(other))
        assert not bool(found.any())


@pytest.mark.parametrize("poison", POISONS)
def test_exclusive_scan_plan_reused_across_paths(poison):
    """16-byte aligned columns take the single-launch path with its chunk hand-off, others the three-launch one"""
    from dwarf_bench_amd import ops
    n = 250007
    plan = ops.ExclusiveScan(n)
    _poison(plan.ws, poison)
    base = ops.gen_uniform_u32(n + 1, 42, 0, 2**32 - 1)
    small = ops.gen_uniform_u32(n + 1, 43, 0, 3)
    for src, init in ((base[:n], 0), (base[1:], 77), (small[:n], 2**32 - 5), (small[1:], 0), (base[:n], 1)):
        plan.launch(src, init)
        h = src.cpu().numpy().view(np.uint32).astype(np.uint64)
        want = ((np.uint64(init) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(h)[:-1]])) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        assert np.array_equal(plan.result().cpu().numpy().view(np.uint32), want)


def test_reduce_over_several_inputs():
    from dwarf_bench_amd import ops
    for n, lo, hi in ((1 << 20, -2**31, 2**31 - 1), (77777, 0, 1), ((1 << 22) + 3, -1000, 1000), (1, 5, 5)):
        host = np.random.default_rng(n).integers(lo, hi + 1, n, dtype=np.int64).astype(np.int32)
        assert int(ops.reduce_sum(torch.from_numpy(host).cuda()).item()) == po.reduce_sum(host)
