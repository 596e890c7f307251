"""Test-only helpers for the hash group-by (dbhip_groupby_hash_u32, csrc/groupby_hash.hip): its hashes restated in
numpy (the radix partition geometry is join_testlib's restatement), inputs constructed against them (one named case per
branch of the kernel file), and exact references.  Numpy only: the CPU tests check the constructions, the GPU tests run
them.  Never imported by the product."""
import numpy as np

from tests import join_testlib as jt
from tests.pjoin_testlib import fmix32

M32 = 0xFFFFFFFF
GOLD = 0x9E3779B1                  # groupby_hash.hip gbh_home / gbh_add: fmix32(key) * 0x9E3779B1
GOLD_INV = pow(GOLD, -1, 1 << 32)
LDS_LG = 13                        # kGbhLdsLg: path a's 8192-slot table
SUB_LG = 12                        # kGbhSubLg: path b's 4096-slot sub-table
SUB_SLOTS = 1 << SUB_LG
LDS_MAX_GROUPS = 4096              # kGbhLdsMaxGroups: path a up to this bound
PROBE = 64                         # kGbhProbe: LDS steps before a row goes to the global table
CROWD = 16                         # kGbhCrowd: lanes of a wave on one key that are summed before the add
GIANT_ROWS = 32768                 # kGbhGiantRows: a partition above this is sliced
WS_ALIGN = WS_HEADER = 256         # dbhip_common.hpp kWsAlign, kWsHeader


def fmix32_inv(h):
    """inverse of fmix32 (murmur3's 32-bit finaliser is a bijection; tools/fuzz_gpu.py fmix32_inv)"""
    h = np.asarray(h).astype(np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7ED1B41D)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h ^= h >> np.uint64(26)
    h = (h * np.uint64(0xA5CB9243)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def _mixed(keys):
    return (fmix32(np.asarray(keys, dtype=np.uint32)) * np.uint64(GOLD)) & np.uint64(M32)


def pid(keys, parts):
    """partition of each key: partition.hpp jl_pid, (fmix32(key) * parts) >> 32"""
    return ((fmix32(np.asarray(keys, dtype=np.uint32)) * np.uint64(parts)) >> np.uint64(32)).astype(np.int64)


def lds_home(keys):
    """path a's LDS home: groupby_hash.hip gbh_add, (fmix32(key) * 0x9E3779B1) >> (32 - kGbhLdsLg)"""
    return (_mixed(keys) >> np.uint64(32 - LDS_LG)).astype(np.int64)


def sub_home(keys):
    """path b's sub-table home: groupby_hash.hip gbh_add with kGbhSubLg, (fmix32(key) * 0x9E3779B1) >> 20"""
    return (_mixed(keys) >> np.uint64(32 - SUB_LG)).astype(np.int64)


def global_home(keys, slots):
    """the global table's home: groupby_hash.hip gbh_home, ((fmix32(key) * 0x9E3779B1 mod 2^32) * slots) >> 32"""
    return ((_mixed(keys) * np.uint64(slots)) >> np.uint64(32)).astype(np.int64)


def part_layout(n):
    """(parts, k1, k2) of path b's partition step: partition.hpp jl_geometry(n) with kJlRowsPerPart rows per partition"""
    return jt.layout(n, jt.JL_ROWS_PER_PART)


def hist_variant(n, digits=True):
    """which histogram jl_partition_side (partition.hip) runs for path b at n rows: 'one level', 'plain', 'fused',
    'fused16' or 'digits' (the 16-bit digit column; DBHIP_JL_DIGITS=0 turns it back into 'plain')"""
    return jt.side_plan(n, n, jt.JL_ROWS_PER_PART, digits=digits)[3]


def workspace_bytes(n, max_groups):
    """groupby_hash.hip gbh_layout(n, max_groups).total for path b (the CPU test compares it with the library's, which
    ties part_layout to the compiled geometry)"""
    def up(x):
        return -(-x // WS_ALIGN) * WS_ALIGN
    groups = min(max_groups or n, n)
    slots = max(2 * groups, 64)
    parts, k1, k2 = part_layout(n)
    off = WS_HEADER + up((n // GIANT_ROWS + 1) * 4) + 3 * up(slots * 4)
    pairs = up(max(n, 1) * 8)
    meta_bytes = 8 * ((2 * 64 + 2) * k1 + 2 + 3 * parts + 1)
    return up(off + pairs + (pairs if k2 > 1 else 0) + meta_bytes)


# ---- key constructions ---------------------------------------------------------------------------------------------
def _unique_keep(keys, count):
    keys = keys[keys != M32]
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)][:count]
    assert keys.size == count
    return keys


def keys_on_home(rng, count, lg, home):
    """`count` distinct keys whose mixed hash has top `lg` bits `home`: (fmix32(k) * 0x9E3779B1) >> (32 - lg) == home"""
    low = rng.choice(1 << (32 - lg), size=count + 8, replace=False).astype(np.uint64)
    x = (np.uint64(home) << np.uint64(32 - lg)) | low
    return _unique_keep(fmix32_inv((x * np.uint64(GOLD_INV)) & np.uint64(M32)), count)


def keys_in_partition(rng, count, parts, p):
    """`count` distinct keys that jl_pid puts into partition p of `parts`"""
    lo = -(-(p << 32) // parts)
    hi = -(-((p + 1) << 32) // parts)
    h = lo + rng.choice(hi - lo, size=count + 8, replace=False).astype(np.uint64)
    keys = _unique_keep(fmix32_inv(h), count)
    assert (pid(keys, parts) == p).all()
    return keys


def keys_in_partition_on_sub_home(rng, count, parts, p, home):
    """`count` distinct keys of partition p whose path-b sub-table home is `home` (a rejection search over the keys of
    that home)"""
    found = np.zeros(0, dtype=np.uint32)
    space = 1 << (32 - SUB_LG)
    start = 0
    while found.size < count:
        assert start < space, "not enough keys"
        low = np.arange(start, min(start + (1 << 20), space), dtype=np.uint64)
        start += 1 << 20
        x = (np.uint64(home) << np.uint64(32 - SUB_LG)) | low
        k = fmix32_inv((x * np.uint64(GOLD_INV)) & np.uint64(M32))
        found = np.concatenate([found, k[(pid(k, parts) == p) & (k != M32)]])
    keys = found[rng.permutation(found.size)[:count]]
    return keys


def background(rng, n, parts=None, avoid=(), distinct=None):
    """n keys, uniform over the 32-bit range (or drawn from a pool of `distinct` keys), none 0xFFFFFFFF and none in a
    partition of `avoid`"""
    avoid = np.asarray(list(avoid), dtype=np.int64)
    pool = None
    if distinct is not None:
        pool = rng.choice(M32, size=distinct * 2 + 64, replace=False).astype(np.uint32)
        if avoid.size:
            pool = pool[~np.isin(pid(pool, parts), avoid)]
        pool = pool[:distinct]
    keys = np.empty(n, dtype=np.uint32)
    bad = np.ones(n, dtype=bool)
    while bad.any():
        m = int(bad.sum())
        keys[bad] = pool[rng.integers(0, pool.size, m)] if pool is not None else \
            rng.integers(0, M32, size=m, dtype=np.uint64).astype(np.uint32)
        bad[bad] = np.isin(pid(keys[bad], parts), avoid) if avoid.size else False
    return keys


def rand_vals(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def wave_rows(step, lanes, component=0):
    """rows that path a's lanes `lanes` handle in one wave step: lane l of the wave at 16-byte index 64 * step + l takes
    rows 4 * (64 * step + l) + {0, 1, 2, 3}, one component per step (gbh_lds_kernel)"""
    return 4 * (64 * step + np.asarray(lanes, dtype=np.int64)) + component


# ---- the named cases -------------------------------------------------------------------------------------------------
class Case:
    """keys, vals, the bound to call with, the branch it drives and what the construction promises (`facts`, checked
    on the CPU by tests/test_groupby_hash_host.py)"""

    def __init__(self, name, keys, vals, max_groups, branch, **facts):
        self.name, self.keys, self.vals, self.max_groups, self.branch, self.facts = name, keys, vals, max_groups, branch, facts

    @property
    def distinct(self):
        return int(np.unique(self.keys).size)


def _finish(rng, keys):
    perm = rng.permutation(keys.size)
    return keys[perm]


def case_lds_home(d, bound=None, extras=False):
    """path a: d distinct keys on one LDS home; beyond kGbhProbe of them a workgroup's rows go to the global table
    (gbh_add<true> -> gbh_global_add).  extras: plus 0xFFFFFFFF rows and a hot key on the same home."""
    rng = np.random.default_rng(1000 + d + (7 if extras else 0))
    n = 1 << 20
    home = int(rng.integers(0, 1 << LDS_LG))
    shared = keys_on_home(rng, d + (1 if extras else 0), LDS_LG, home)
    keys = shared[:d][rng.integers(0, d, n)]
    if extras:
        keys[rng.random(n) < 0.3] = shared[d]        # a hot key, on the same home
        keys[rng.random(n) < 0.1] = M32              # the side sum
    mg = bound if bound is not None else d + (2 if extras else 0)
    return Case(f"lds_home_{d}{'_extras' if extras else ''}", keys, rand_vals(rng, n), mg, "LDS probe overflow",
                home=home, shared=shared)


def case_sub_overflow(n, d):
    """path b: one partition holds d > kGbhSubSlots distinct keys (3 rows each at most); the keys that find no slot
    go to the global table and are appended by gbh_compact_kernel.  d large enough makes the partition a giant
    whose slices overflow the sub-table as well."""
    rng = np.random.default_rng(n + d)
    parts = part_layout(n)[0]
    p = int(rng.integers(0, parts))
    mine = keys_in_partition(rng, d, parts, p)
    per = 1 if d * 2 > GIANT_ROWS else 3
    rows = np.repeat(mine, rng.integers(1, per + 1, d))
    keys = _finish(rng, np.concatenate([background(rng, n - rows.size, parts, avoid=[p]), rows]))
    return Case(f"sub_overflow_{n}_{d}", keys, rand_vals(rng, n), 0, "sub-table overflow" if rows.size <= GIANT_ROWS
                else "giant slices overflow the sub-table", parts=parts, partition=p, mine=mine, part_rows=rows.size)


def case_sub_cluster(n, c=80):
    """path b: c keys on one sub-table home inside an otherwise uniform partition: past kGbhProbe steps they go to the
    global table"""
    rng = np.random.default_rng(n + c + 1)
    parts = part_layout(n)[0]
    p = int(rng.integers(0, parts))
    home = int(rng.integers(0, SUB_SLOTS))
    mine = keys_in_partition_on_sub_home(rng, c, parts, p, home)
    keys = background(rng, n - 2 * c)
    keys = _finish(rng, np.concatenate([keys, mine, mine]))
    return Case(f"sub_cluster_{n}_{c}", keys, rand_vals(rng, n), 0, "sub-table probe overflow", parts=parts,
                partition=p, home=home, mine=mine)


def case_giant_edge(rows):
    """path b: one partition of exactly `rows` rows, a hot key and distinct others: 32768 stays on gbh_part_kernel,
    32769 goes to gbh_giant_kernel in two slices"""
    n = 1 << 21
    rng = np.random.default_rng(rows)
    parts = part_layout(n)[0]
    p = int(rng.integers(0, parts))
    mine = keys_in_partition(rng, 2001, parts, p)
    part = np.concatenate([np.full(rows - 2000, mine[0], dtype=np.uint32), mine[1:]])
    keys = _finish(rng, np.concatenate([background(rng, n - rows, parts, avoid=[p]), part]))
    return Case(f"giant_edge_{rows}", keys, rand_vals(rng, n), 0, "giant" if rows > GIANT_ROWS else "largest normal partition",
                parts=parts, partition=p, part_rows=rows)


def case_many_giants(count=64, ff=False):
    """path b: `count` hot keys in distinct partitions of nothing else, each 32769 to 70535 rows (two or three slices
    each, every wave of a slice one crowd); ff: 5 % of the other rows 0xFFFFFFFF, one more giant partition (its side
    sum comes out of the giant slices)"""
    n = 1 << 23
    rng = np.random.default_rng(count * 3 + ff)
    parts = part_layout(n)[0]
    ps = rng.choice(parts, size=count, replace=False)
    hot = np.concatenate([keys_in_partition(rng, 1, parts, int(p)) for p in ps])
    per = rng.integers(GIANT_ROWS + 1, 2 * GIANT_ROWS + 5000, count)
    rows = np.repeat(hot, per)
    rest = background(rng, n - rows.size, parts, avoid=ps, distinct=200000)
    if ff:
        rest[rng.random(rest.size) < 0.05] = M32
    keys = _finish(rng, np.concatenate([rest, rows]))
    return Case(f"many_giants_{count}{'_ff' if ff else ''}", keys, rand_vals(rng, n), 0, "several giants", parts=parts,
                partitions=ps, hot=hot, per=per)


def case_crowd(lanes_on_key, ff_lanes=0):
    """path a: one key on exactly `lanes_on_key` of the 64 rows one wave step covers, the first of them the wave's
    first active lane (after `ff_lanes` lanes of 0xFFFFFFFF); 16 or more: the crowd shortcut of gbh_wave_row"""
    rng = np.random.default_rng(50 + lanes_on_key + 100 * ff_lanes)
    n = 1 << 16
    pool = rng.choice(M32, size=200, replace=False).astype(np.uint32)
    keys = pool[1 + rng.integers(0, 199, n)]
    crowd_key = pool[0]
    steps = np.arange(0, n // 256, 3)  # every third wave step of the input, component 0..3 in turn
    lanes_all = []
    for j, st in enumerate(steps):
        lanes = np.concatenate([[ff_lanes], ff_lanes + 1 + rng.choice(63 - ff_lanes, lanes_on_key - 1, replace=False)])
        comp = j % 4
        keys[wave_rows(st, np.arange(ff_lanes), comp)] = M32
        keys[wave_rows(st, lanes, comp)] = crowd_key
        others = np.setdiff1d(np.arange(ff_lanes, 64), lanes)
        keys[wave_rows(st, others, comp)] = pool[1 + (np.arange(others.size) % 199)]  # none of them the crowd key
        lanes_all.append((int(st), comp, lanes))
    return Case(f"crowd_{lanes_on_key}{f'_after_{ff_lanes}_ff' if ff_lanes else ''}", keys, rand_vals(rng, n), 201,
                "crowd" if lanes_on_key >= CROWD else "below the crowd threshold", crowd_key=crowd_key, steps=lanes_all,
                ff_lanes=ff_lanes, lanes_on_key=lanes_on_key)


def case_bound_global_only():
    """path b with a bound that only the global table's rows pass: 3000 pool keys spread over the partitions plus one
    partition of 6000 distinct keys, max_groups = distinct - 1.  The rows gbh_part_kernel writes directly (at most
    kGbhSubSlots of the big partition plus the others) stay below the bound; gbh_compact_kernel's appends pass it."""
    n = 1 << 21
    rng = np.random.default_rng(77)
    parts = part_layout(n)[0]
    p = int(rng.integers(0, parts))
    mine = keys_in_partition(rng, 6000, parts, p)
    keys = _finish(rng, np.concatenate([background(rng, n - mine.size, parts, avoid=[p], distinct=3000), mine]))
    c = Case("bound_global_only", keys, rand_vals(rng, n), 0, "bound passed in gbh_compact_kernel", parts=parts,
             partition=p, mine=mine)
    c.max_groups = c.distinct - 1
    return c


# every constructed case the GPU tests run, by name (the CPU test checks each construction)
CASES = {
    **{f"lds_home_{d}": (lambda d=d: case_lds_home(d)) for d in (65, 100, 4096)},
    "lds_home_100_extras": lambda: case_lds_home(100, extras=True),
    **{f"sub_overflow_{n}_{d}": (lambda n=n, d=d: case_sub_overflow(n, d))
       for n in (1 << 21, 1 << 23) for d in (4097, 6000, 40000)},
    **{f"sub_cluster_{n}": (lambda n=n: case_sub_cluster(n)) for n in (1 << 21, 1 << 23)},
    "giant_edge_32768": lambda: case_giant_edge(GIANT_ROWS),
    "giant_edge_32769": lambda: case_giant_edge(GIANT_ROWS + 1),
    "many_giants": lambda: case_many_giants(),
    "many_giants_ff": lambda: case_many_giants(ff=True),
    **{f"crowd_{c}": (lambda c=c: case_crowd(c)) for c in (15, 16, 17)},
    "crowd_16_after_ff": lambda: case_crowd(16, ff_lanes=5),
    "bound_global_only": case_bound_global_only,
}

# path b at every histogram variant of the partition step: (rows, also run with DBHIP_JL_DIGITS=0)
PARTITION_STEP_SIZES = [(1 << 21, False), ((1 << 21) + 3, False), (1 << 23, False), ((1 << 26) - 5, False),
                        ((1 << 27) + 5, False), (81920 * 2048, False), (81920 * 2048 + 1, True), ((1 << 28) + 12345, True)]


# ---- exact references ------------------------------------------------------------------------------------------------
def expect(keys, vals):
    """(sorted distinct keys, uint32 wrap-around sums, counts): a stable sort and np.add.reduceat in uint64"""
    keys = np.asarray(keys, dtype=np.uint32)
    if keys.size == 0:
        z = np.zeros(0, dtype=np.uint32)
        return z, z, z
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    sums = np.add.reduceat(np.asarray(vals, dtype=np.uint32)[order].astype(np.uint64), starts) & np.uint64(M32)
    counts = np.diff(np.concatenate([starts, [keys.size]]))
    return ks[starts], sums.astype(np.uint32), counts.astype(np.uint32)


def pool_input(n, seed, distinct=1 << 20):
    """keys = pool[idx] for a pool of `distinct` keys with 0xFFFFFFFF at index 0 (about 1 % of the rows) and a hot key at
    index 1 (about 10 %), random 32-bit vals, and the exact reference from idx alone: np.bincount over the low and the
    high 16 bits of vals (each half-sum stays below 2^53: exact in float64).  -> keys, vals, (keys, sums, counts) sorted
    by key"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, M32, size=distinct + distinct // 8, dtype=np.uint64).astype(np.uint32))
    pool = rng.permutation(pool)[: distinct - 1]
    pool = np.concatenate([[np.uint32(M32)], pool]).astype(np.uint32)
    idx = rng.integers(2, pool.size, size=n, dtype=np.int32)
    r = rng.random(n, dtype=np.float32)
    idx[r < 0.1] = 1
    idx[r < 0.01] = 0
    del r
    keys = pool[idx]
    vals = rand_vals(rng, n)
    cnt = np.bincount(idx, minlength=pool.size)
    lo = np.bincount(idx, weights=(vals & np.uint32(0xFFFF)).astype(np.float64), minlength=pool.size)
    hi = np.bincount(idx, weights=(vals >> np.uint32(16)).astype(np.float64), minlength=pool.size)
    del idx
    sums = ((lo.astype(np.uint64) + (hi.astype(np.uint64) << np.uint64(16))) & np.uint64(M32)).astype(np.uint32)
    seen = cnt > 0
    order = np.argsort(pool[seen])
    return keys, vals, (pool[seen][order], sums[seen][order], cnt[seen][order].astype(np.uint32))
