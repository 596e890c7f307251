"""Test-only helpers for the one-to-many joins (ops.HashJoin, ops.RadixJoin): keys constructed against the partition
hash of join_lds.hip, the partition counts of join_common.hpp restated, and the checks every join test applies.
Never imported by the product."""
import numpy as np
import torch

from oracle import pyoracle as po
from tests.pjoin_testlib import fmix32


def dev(a):
    """uint32 numpy column -> int32 tensor on the GPU (same bits)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def keys_of_partition_of(parts, partition, how_many):
    """the first `how_many` keys >= 1 that the partition hash (join_lds.hip jl_pid: the high bits of fmix32(key) * parts)
    puts into `partition` of `parts`"""
    cand = np.arange(1, 1 + how_many * parts * 2, dtype=np.uint64)
    mine = cand[(fmix32(cand) * np.uint64(parts)) >> np.uint64(32) == partition][:how_many]
    assert mine.size == how_many
    return mine.astype(np.uint32)


def build_parts(n_build):
    """partitions of the one-to-many build (join_common.hpp jl_layout, kJlRowsPerPart = 2048 rows per partition)"""
    want = min(max(1, -(-n_build // 2048)), 1 << 20)
    lg = want.bit_length() - 1  # floor(log2(want))
    k2 = 1 if want <= 1024 else 1 << (lg // 2)
    return -(-want // k2) * k2


def keys_of_partition(n_build, partition, how_many):
    """distinct keys that the build of n_build rows puts into one partition"""
    return keys_of_partition_of(build_parts(n_build), partition, how_many)


def radix_parts(n_build):
    """partitions of the radix join (join_common.hpp jl_layout with kJrRowsPerPart = 1792 rows per partition)"""
    want = min(max(1, -(-n_build // 1792)), 1 << 20)
    lg = (want - 1).bit_length()
    if want <= 1024:
        k2 = 1
    else:
        lgs = lg - 1 if (1 << lg) != want else lg
        k2 = 1 << (lgs // 2)
    k1 = -(-want // k2)
    while k1 > 1024:
        k2 *= 2
        k1 = -(-want // k2)
    return k1 * k2


def check_grouped_join(build, probe, plan=None):
    """Build and probe through `plan` (a fresh ops.HashJoin when None), then: counts per probe row against numpy; ids a
    permutation of the build rows in which every key's rows are ONE run; every hit's range starts and ends inside its
    key's run (with the count right, the range IS the run)."""
    from dwarf_bench_amd import ops
    if plan is None:
        plan = ops.HashJoin(len(build), len(probe))
    plan.build(dev(build))
    plan.probe(dev(probe))
    pos, cnt, ids = (t.cpu().numpy().view(np.uint32) for t in plan.result())
    assert np.array_equal(cnt.astype(np.uint64), po.join_counts_fast(build, probe))
    assert np.array_equal(np.sort(ids), np.arange(len(build), dtype=np.uint32))
    in_order = build[ids]
    assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == np.unique(build).size
    hit = cnt > 0
    assert np.array_equal(in_order[pos[hit]], probe[hit])
    assert np.array_equal(in_order[pos[hit] + cnt[hit] - 1], probe[hit])


def check_radix_result(build, probe, result):
    """the radix join's (rid, pos, cnt, ids): rid and ids permutations, every probe row's count against numpy (found
    through its row id), every key's ids one run, every hit's range starts and ends on its key"""
    rid, pos, cnt, ids = (t.cpu().numpy().view(np.uint32) for t in result)
    assert np.array_equal(np.sort(rid), np.arange(len(probe), dtype=np.uint32))
    assert np.array_equal(np.sort(ids), np.arange(len(build), dtype=np.uint32))
    assert np.array_equal(cnt, po.join_counts_fast(build, probe).astype(np.uint32)[rid])
    in_order = build[ids]
    assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == np.unique(build).size
    hit = cnt > 0
    assert np.array_equal(in_order[pos[hit]], probe[rid[hit]])
    assert np.array_equal(in_order[pos[hit] + cnt[hit] - 1], probe[rid[hit]])
