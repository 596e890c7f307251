"""Test-only helpers for the one-to-many joins (ops.HashJoin, ops.RadixJoin): keys constructed against the partition
hash of partition.hpp, its geometry and side plan restated (the one restatement under tests/: the group-by's helpers
call it), and the checks every join test applies.  torch is imported where a helper needs it, so the numpy-only
helpers can use the restatement.  Never imported by the product."""
import numpy as np

from oracle import pyoracle as po
from tests.pjoin_testlib import fmix32


def dev(a):
    """uint32 numpy column -> int32 tensor on the GPU (same bits)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def keys_of_partition_of(parts, partition, how_many):
    """the first `how_many` keys >= 1 that the partition hash (partition.hpp jl_pid: the high bits of fmix32(key) * parts)
    puts into `partition` of `parts`"""
    cand = np.arange(1, 1 + how_many * parts * 2, dtype=np.uint64)
    mine = cand[(fmix32(cand) * np.uint64(parts)) >> np.uint64(32) == partition][:how_many]
    assert mine.size == how_many
    return mine.astype(np.uint32)


JL_ROWS_PER_PART = 2048  # join_common.hpp kJlRowsPerPart: the hash and unique joins and the group-by's path b
JR_ROWS_PER_PART = 1792  # kJrRowsPerPart: the radix join
FUSED_MAX_PARTS = 32768  # partition.hpp kJlFusedMaxParts
FUSED16_MAX_PARTS = 80 * 1024  # kJlFused16MaxParts
HIST_ROWS = 64 * 4  # kJlGroups x kJlFusedWgPerGroup: the rows of the fused histograms' scratch


def layout(n_build, rows_per_part):
    """(parts, k1, k2) of partition.hpp jl_geometry(n_build, rows_per_part) with DBHIP_JL_K2_BIAS = 0"""
    want = min(max(1, -(-int(n_build) // rows_per_part)), 1 << 20)
    lg = (want - 1).bit_length()  # ceil(log2(want))
    if want <= 1024:
        k2 = 1
    else:
        lgs = lg - 1 if (1 << lg) != want else lg
        k2 = 1 << (lgs // 2)
    k1 = -(-want // k2)
    while k1 > 1024:
        k2 *= 2
        k1 = -(-want // k2)
    return k1 * k2, k1, k2


def shape_for(k1, k2, t0=None, t1=None):
    """the tile shapes of partition.hpp jl_side_plan: the shape ids (t0, t1) of the two scatter levels, DBHIP_JL_T0 / DBHIP_JL_T1 forced
    when given (t1 = 2 reads as 1)"""
    s0 = 2 if k1 >= 512 else 0
    s1 = 1 if k2 >= 512 else 0
    if t0 is not None:
        s0 = t0
    if t1 is not None:
        s1 = min(t1, 1)
    return s0, s1


def side_plan(n_side, n_build, rows_per_part, t0=None, t1=None, digits=True):
    """partition.hpp jl_side_plan: what jl_partition_side does with a column of n_side rows laid out by the geometry of n_build rows
    (the radix join partitions its probe side with the build side's): -> (parts, k1, k2, variant, t0, t1).  variant is
    the histogram it runs — 'one level', 'plain', 'fused', 'fused16' or 'digits' — including the fused histograms' need
    for scratch: 256 rows of `parts` counters in the level-1 output region of 8 * n_side bytes, i.e. n_side >= 128 *
    parts.  The digit column needs no scratch; DBHIP_JL_DIGITS=0 (digits=False) turns it back into 'plain'."""
    parts, k1, k2 = layout(n_build, rows_per_part)
    scratch = int(n_side) * 8 >= HIST_ROWS * parts * 4
    if k2 == 1:
        variant = "one level"
    elif 8192 <= parts <= FUSED_MAX_PARTS and scratch:
        variant = "fused"
    elif FUSED_MAX_PARTS < parts <= FUSED16_MAX_PARTS and scratch:
        variant = "fused16"
    elif digits and parts > FUSED16_MAX_PARTS and k2 <= 65536:
        variant = "digits"
    else:
        variant = "plain"
    return (parts, k1, k2, variant) + shape_for(k1, k2, t0, t1)


def build_parts(n_build):
    """partitions of the one-to-many build (jl_layout with kJlRowsPerPart = 2048 rows per partition)"""
    return layout(n_build, JL_ROWS_PER_PART)[0]


def keys_of_partition(n_build, partition, how_many):
    """distinct keys that the build of n_build rows puts into one partition"""
    return keys_of_partition_of(build_parts(n_build), partition, how_many)


def radix_parts(n_build):
    """partitions of the radix join (jl_layout with kJrRowsPerPart = 1792 rows per partition)"""
    return layout(n_build, JR_ROWS_PER_PART)[0]


# ---- columns that do not start on a 16-byte boundary, with guard words around them -----------------------------------
GUARD_WORDS = 16


def guarded(n, offset_words, fill, device="cuda"):
    """-> (base, view): an int32 column of n words that starts `offset_words` 4-byte words after a 16-byte boundary, in
    a fresh allocation (torch's: 512-byte aligned) whose other words — at least GUARD_WORDS on each side — hold `fill`"""
    import torch
    base = torch.full((GUARD_WORDS + offset_words + n + GUARD_WORDS,), fill, dtype=torch.int32, device=device)
    assert base.data_ptr() % 16 == 0
    view = base[GUARD_WORDS + offset_words: GUARD_WORDS + offset_words + n]
    assert view.data_ptr() % 16 == 4 * (offset_words % 4)
    return base, view


def assert_guards(base, view, fill):
    """every word of `base` outside `view` still holds `fill`"""
    at = (view.data_ptr() - base.data_ptr()) // 4
    assert at >= GUARD_WORDS and base.numel() - at - view.numel() >= GUARD_WORDS
    for part, where in ((base[:at], "in front of"), (base[at + view.numel():], "behind")):
        bad = (part != fill).nonzero()
        assert bad.numel() == 0, f"{bad.numel()} guard words {where} the column overwritten"


def check_grouped_join(build, probe, plan=None):
    """Build and probe through `plan` (a fresh ops.HashJoin when None), then check_grouped_result."""
    from dwarf_bench_amd import ops
    if plan is None:
        plan = ops.HashJoin(len(build), len(probe))
    plan.build(dev(build))
    plan.probe(dev(probe))
    check_grouped_result(build, probe, plan.result())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_grouped_result(build, probe, result, first=0, counts=None):
    """the row-ordered join's (pos, cnt, ids), ids holding first + build row: counts per probe row against numpy (or
    `counts`, join_counts_fast precomputed); ids a permutation of the build rows in which every key's rows are ONE run;
    every hit's range starts and ends inside its key's run (with the count right, the range IS the run)."""
    pos, cnt, ids = (_u32(t) for t in result)
    ids = ids - np.uint32(first)
    want = po.join_counts_fast(build, probe) if counts is None else counts
    assert np.array_equal(cnt.astype(np.uint64), want)
    assert np.array_equal(np.sort(ids), np.arange(len(build), dtype=np.uint32))
    in_order = build[ids]
    assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == np.unique(build).size
    hit = cnt > 0
    assert np.array_equal(in_order[pos[hit]], probe[hit])
    assert np.array_equal(in_order[pos[hit] + cnt[hit] - 1], probe[hit])


def check_radix_result(build, probe, result, build_first=0, probe_first=0, counts=None):
    """the radix join's (rid, pos, cnt, ids), rid holding probe_first + probe row and ids build_first + build row: rid
    and ids permutations, every probe row's count against numpy (or `counts`, join_counts_fast precomputed; found
    through its row id), every key's ids one run, every hit's range starts and ends on its key"""
    rid, pos, cnt, ids = (_u32(t) for t in result)
    rid, ids = rid - np.uint32(probe_first), ids - np.uint32(build_first)
    assert np.array_equal(np.sort(rid), np.arange(len(probe), dtype=np.uint32))
    assert np.array_equal(np.sort(ids), np.arange(len(build), dtype=np.uint32))
    want = po.join_counts_fast(build, probe) if counts is None else counts
    assert np.array_equal(cnt, want.astype(np.uint32)[rid])
    in_order = build[ids]
    assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == np.unique(build).size
    hit = cnt > 0
    assert np.array_equal(in_order[pos[hit]], probe[rid[hit]])
    assert np.array_equal(in_order[pos[hit] + cnt[hit] - 1], probe[rid[hit]])


# ---- the sizes of tests/test_gpu_join_layouts.py and what the partition step does at each -------------------------------
# build rows -> side_plan(n, n, ...) of the radix join (1792 rows per partition) and of the hash join (2048)
LAYOUT_TABLE = [
    (1 << 20, (586, 586, 1, "one level", 2, 0), (512, 512, 1, "one level", 2, 0)),
    ((1 << 21) + 3, (1184, 37, 32, "plain", 0, 0), (1056, 33, 32, "plain", 0, 0)),
    ((1 << 24) + 5, (9408, 147, 64, "fused", 0, 0), (8256, 129, 64, "fused", 0, 0)),
    ((1 << 26) + 5, (37504, 293, 128, "fused16", 0, 0), (32896, 257, 128, "fused16", 0, 0)),
    (170_000_001, (94976, 371, 256, "digits", 0, 0), (83200, 325, 256, "digits", 0, 0)),
]
HEADLINE_BUILD, HEADLINE_PROBE = (1 << 29) + 12345, (1 << 22) + 77  # level 1 in 1024 x 8 tiles: the 2^30 join's geometry
HEADLINE_PLANS = ((300032, 586, 512, "digits", 2, 1), (262656, 513, 512, "digits", 2, 1))
SMALL_PROBE = 20011  # far below 128 rows per partition at every two-level size: the fused histograms have no scratch


def radix_probe_sizes(n_build):
    """(large, small) probe sides of the radix join of n_build rows: the large one just above the 128 rows per build
    partition from which the fused histograms have their scratch (it takes the build side's variant), the small one far
    below (the plain histograms where the build side's are fused)"""
    return max(128 * radix_parts(n_build) + 5, SMALL_PROBE + 1), SMALL_PROBE


def layout_sizes():
    """every row count tests/test_gpu_join_layouts.py hands the joins"""
    sizes = {HEADLINE_BUILD, HEADLINE_PROBE}
    for n, _, _ in LAYOUT_TABLE:
        sizes.add(n)
        sizes.update(radix_probe_sizes(n))
        sizes.add(n // 2 + 13)  # the unique join's probe side
    return sorted(sizes)
