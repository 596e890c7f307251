"""Seeded randomised parity sweep: many (size, parameter, distribution) combinations per dwarf against the oracle,
to catch tail / alignment / boundary cases the hand-picked sizes miss.  Deterministic (fixed seeds)."""
import numpy as np
import pytest
import torch

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _sizes(rng, count, hi_log2):
    """log-uniform sizes plus neighbours of powers of two and of the kernels' tile sizes"""
    out = [int(2 ** rng.uniform(0, hi_log2)) for _ in range(count)]
    for base in (64, 256, 1024, 2048, 4096, 8192, 32768, 1 << 16, 1 << 17, 1 << 20):
        out += [base + int(d) for d in rng.integers(-3, 4, size=2)]
    return [max(1, s) for s in out]


def _keys(rng, n, kind):
    if kind == 0:
        return po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 1, 10000)           # the reference's distribution
    if kind == 1:
        return po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, 2**32 - 1)       # full range
    if kind == 2:
        return np.full(n, int(rng.integers(0, 2**32 - 1)), dtype=np.uint32)             # all equal
    if kind == 3:
        return rng.integers(0, 4, size=n, dtype=np.uint32) * np.uint32(0x01000000)      # only one byte varies
    if kind == 5:                                                                       # 90 % one value, the rest anything
        k = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, 2**32 - 1)
        k[rng.random(n) < 0.9] = np.uint32(rng.integers(0, 2**32 - 1))
        return k
    if kind == 6:                                                                       # two distinct values in every byte
        return np.where(rng.integers(0, 2, size=n) == 1, np.uint32(0xFFFFFFFF), np.uint32(0))
    return np.sort(po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, max(n, 1)))  # sorted, many duplicates


def test_fuzz_scan():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(101)
    for n in _sizes(rng, 40, 23):
        src = _keys(rng, n, int(rng.integers(0, 2))).view(np.int32)
        filt = int(rng.choice([-5, 0, 1, 5, 101, 5001, 10001, 2**31 - 1]))
        off = int(rng.integers(0, 4))  # 4-byte-granular misalignment of the source pointer
        buf = _dev(np.concatenate([np.zeros(off, dtype=np.int32), src]))
        got = ops.copy_if_lt(buf[off:], filt).cpu().numpy()
        assert np.array_equal(got, po.copy_if_lt(src, filt)), (n, filt, off)
        got = ops.copy_if_lt(buf[off:], filt, dense=True).cpu().numpy()  # the single-launch entry point
        assert np.array_equal(got, po.copy_if_lt(src, filt)), ("dense", n, filt, off)


def test_fuzz_sort():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(102)
    for n in _sizes(rng, 40, 21):
        keys = _keys(rng, n, int(rng.integers(0, 8)))
        bits = int(rng.choice([4, 8]))
        signed = bool(rng.integers(0, 2))
        t = _dev(keys)
        ops.radix_sort_(t, signed=signed, radix_bits=bits)
        got = t.cpu().numpy()
        want = np.sort(keys.view(np.int32)) if signed else np.sort(keys).view(np.int32)
        assert np.array_equal(got, want), (n, bits, signed)


def test_fuzz_groupby():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(103)
    for n in _sizes(rng, 30, 21):
        groups = int(rng.choice([1, 2, 3, 20, 64, 1000, 4096, 32768, 32769, 65536, 70001, 200000]))
        keys = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, groups - 1)
        if rng.integers(0, 3) == 0:
            keys[:] = keys[0]  # one hot group
        vals = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, int(rng.choice([1, 10000, 2**32 - 1])))
        got = ops.groupby_sum(_dev(keys), _dev(vals), groups).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, po.groupby_sum(keys, vals, groups)), (n, groups)


def test_fuzz_join():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(104)
    for nb in _sizes(rng, 24, 20):
        npr = max(1, int(nb * rng.uniform(0.3, 2.0)))
        hi = int(rng.choice([10, 10000, max(nb - 1, 1), 2**32 - 2]))
        build = po.gen_uniform_u32(nb, int(rng.integers(1, 1 << 30)), 0, hi)
        probe = po.gen_uniform_u32(npr, int(rng.integers(1, 1 << 30)), 0, hi)
        if hi == 10 and nb > 300000:
            continue  # millions of duplicates per key: covered by the dedicated skew tests, slow to verify here
        pos, cnt, ids = (t.cpu().numpy().view(np.uint32) for t in ops.hash_join(_dev(build), _dev(probe)))
        assert np.array_equal(cnt, po.join_counts_fast(build, probe).astype(np.uint32)), (nb, npr, hi)
        assert np.array_equal(np.sort(ids), np.arange(nb, dtype=np.uint32)), (nb, npr, hi)
        hit = np.flatnonzero(cnt > 0)
        if hit.size:
            for which in (0, -1):  # first and last id of every bucket carry the probe key
                at = pos[hit] + (cnt[hit] - 1 if which else 0)
                assert np.array_equal(build[ids[at]], probe[hit]), (nb, npr, hi)


def test_fuzz_joins_with_hot_keys():
    """both join paths on 2^18 .. 2^21 build rows with zero to three hot keys of 2 .. 60 % of a side, narrow and wide key
    ranges (50 distinct keys: every partition that holds rows is a giant one): counts per probe row, ids a permutation in
    which every key is one run, ranges that start and end in their key's run — against numpy"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(2026)
    for _ in range(10):
        nb = int(rng.integers(1 << 18, 1 << 21))
        npr = int(rng.integers(1000, 1 << 20))
        hi = int(rng.choice([nb, 10000, 2**32 - 2, 50]))
        hb = rng.integers(0, hi, nb, dtype=np.uint64).astype(np.uint32)
        hp = rng.integers(0, hi, npr, dtype=np.uint64).astype(np.uint32)
        for _k in range(int(rng.integers(0, 4))):
            key = np.uint32(rng.integers(0, hi))
            frac = rng.choice([0.02, 0.1, 0.3, 0.6])
            side = rng.integers(0, 3)
            if side in (0, 2):
                hb[rng.random(nb) < frac] = key
            if side in (1, 2):
                hp[rng.random(npr) < frac] = key
        want = po.join_counts_fast(hb, hp).astype(np.uint32)
        runs = np.unique(hb).size
        pos, cnt, ids = (t.cpu().numpy().view(np.uint32) for t in ops.hash_join(_dev(hb), _dev(hp)))
        assert np.array_equal(cnt, want) and np.array_equal(np.sort(ids), np.arange(nb, dtype=np.uint32))
        in_order, hit = hb[ids], cnt > 0
        assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == runs
        assert np.array_equal(in_order[pos[hit]], hp[hit]) and np.array_equal(in_order[pos[hit] + cnt[hit] - 1], hp[hit])
        rid, pos, cnt, ids = (t.cpu().numpy().view(np.uint32) for t in ops.radix_join(_dev(hb), _dev(hp)))
        assert np.array_equal(np.sort(rid), np.arange(npr, dtype=np.uint32)) and np.array_equal(cnt, want[rid])
        assert np.array_equal(np.sort(ids), np.arange(nb, dtype=np.uint32))
        in_order, hit = hb[ids], cnt > 0
        assert np.count_nonzero(in_order[1:] != in_order[:-1]) + 1 == runs
        assert np.array_equal(in_order[pos[hit]], hp[rid[hit]]) and np.array_equal(in_order[pos[hit] + cnt[hit] - 1], hp[rid[hit]])


def test_fuzz_ujoin():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(105)
    for nb in _sizes(rng, 20, 20):
        npr = max(1, int(nb * rng.uniform(0.3, 2.0)))
        ak = po.gen_unique_sorted_u32(nb, int(rng.integers(1, 1 << 20)))
        bk = po.gen_unique_sorted_u32(npr, int(rng.integers(1, 1 << 20)))
        if rng.integers(0, 2):
            rng.shuffle(ak)
        av = po.gen_uniform_u32(nb, 7, 0, 2**32 - 2)
        bv = po.gen_uniform_u32(npr, 8, 0, 2**32 - 2)
        plan = ops.UniqueJoin(nb, npr)
        plan.build(_dev(ak), _dev(av))
        plan.probe(_dev(bk), _dev(bv))
        ok, o1, o2 = (t.cpu().numpy().view(np.uint32) for t in plan.result())
        ek, e1, e2 = po.ujoin(ak, av, bk, bv)
        assert np.array_equal(ok, ek) and np.array_equal(o1, e1) and np.array_equal(o2, e2), (nb, npr)


def test_fuzz_partition_and_reduce():
    from dwarf_bench_amd import ops
    from tests.pjoin_testlib import dest_of
    rng = np.random.default_rng(106)
    for n in _sizes(rng, 20, 21):
        parts = int(rng.choice([1, 2, 3, 5, 8, 16, 100, 256]))
        keys = _keys(rng, n, int(rng.integers(0, 2)))
        first = int(rng.integers(0, 2**31))
        ok, orid, cnt = ops.partition_by_hash(_dev(keys), first, parts)
        d = dest_of(keys, parts)
        c = cnt.cpu().numpy()
        assert np.array_equal(c, np.bincount(d, minlength=parts)), (n, parts)
        r2 = orid.cpu().numpy().view(np.uint32).astype(np.int64) - first
        assert np.array_equal(np.sort(r2), np.arange(n)) and np.array_equal(keys[r2], ok.cpu().numpy().view(np.uint32))
        assert np.all(np.diff(d[r2]) >= 0)  # bucket-major
        src = keys.view(np.int32)
        assert int(ops.reduce_sum(_dev(src)).cpu()[0]) == po.reduce_sum(src), n


def _gbh_keys(rng, n, kind):
    """_keys' distributions plus kind 8: keys on one path-b sub-table home (tests/groupby_hash_testlib.py)"""
    if kind == 8:
        from tests.groupby_hash_testlib import SUB_LG, keys_on_home
        pool = keys_on_home(rng, int(rng.integers(65, 5000)), SUB_LG, int(rng.integers(0, 1 << SUB_LG)))
        return pool[rng.integers(0, pool.size, n)]
    return _keys(rng, n, kind)


def test_fuzz_groupby_hash():
    """the hash group-by on seeded sizes and key distributions, bound at, above, below the true distinct count and
    none, counts on and off: exact keys, sums and counts; below the bound only the status and the bound"""
    from dwarf_bench_amd import ops
    from tests.groupby_hash_testlib import expect
    rng = np.random.default_rng(107)
    for n in _sizes(rng, 24, 21):
        keys = _gbh_keys(rng, n, int(rng.integers(0, 9)))
        vals = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, int(rng.choice([1, 10000, 2**32 - 1])))
        want = expect(keys, vals)
        d = want[0].size
        which = int(rng.integers(0, 4))
        bound = [d, d + int(rng.integers(1, 5000)), max(1, d - int(rng.integers(1, max(2, d)))), 0][which]
        counts = bool(rng.integers(0, 2))
        plan = ops.GroupByHash(n, bound)
        plan.launch(_dev(keys), _dev(vals), counts=counts)
        st = ops.workspace_status(plan.ws)
        if bound and bound < d:
            assert st & ops.DEV_TABLE_FULL and int(plan.groups.item()) == bound, (n, d, bound)
            continue
        assert st == ops.DEV_OK, (n, d, bound, st)
        k, s, c = plan.result()
        k = k.cpu().numpy().view(np.uint32)
        o = np.argsort(k, kind="stable")
        assert np.array_equal(k[o], want[0]) and np.array_equal(s.cpu().numpy().view(np.uint32)[o], want[1]), (n, d, bound)
        if counts:
            assert np.array_equal(c.cpu().numpy().view(np.uint32)[o], want[2]), (n, d, bound)


def test_fuzz_cuckoo():
    """the cuckoo table (hash_kind 2) built through ops.cuckoo_build at load 0.1-0.45 from shuffled full-range unique
    keys, a second insert into the non-empty table, lookups of present and absent keys against the inserted pairs; duplicate keys
    against the documented rule (the h1 slot wins)"""
    from dwarf_bench_amd import ops
    from tests.cuckoo_model import positions_np
    rng = np.random.default_rng(108)
    for n in _sizes(rng, 12, 20)[::2]:
        size = max(8, int(n / rng.uniform(0.1, 0.45)))
        keys = rng.choice(2**32 - 1, size=n, replace=False).astype(np.uint32)  # 0xFFFFFFFF is the empty key
        vals = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        half = n // 2
        table, _ = ops.cuckoo_build(_dev(keys[:half]), _dev(vals[:half]), table_size=size, seed=int(rng.integers(0, 1000)))
        table.insert(_dev(keys[half:]), _dev(vals[half:]))
        if table.status() != ops.DEV_OK:  # a second insert may fail legitimately: rebuild the whole set instead
            assert table.status() == ops.DEV_TABLE_FULL
            table, _ = ops.cuckoo_build(_dev(keys), _dev(vals), table_size=size)
        q = np.concatenate([keys, rng.integers(0, 2**32 - 1, size=n + 7, dtype=np.uint64).astype(np.uint32)])
        q = q[rng.permutation(q.size)]
        gv, gf = (t.cpu().numpy().view(np.uint32) for t in table.lookup(_dev(q)))
        order = np.argsort(keys)
        at = np.minimum(np.searchsorted(keys[order], q), n - 1)
        wf = (keys[order][at] == q).astype(np.uint32)
        wv = np.where(wf == 1, vals[order][at], 0).astype(np.uint32)
        assert np.array_equal(gf, wf) and np.array_equal(gv, wv), (n, size)
    # duplicates: every row stored (distinct positions), a lookup answers from h1 when h1 holds the key, else from h2.
    # A key has two slots, so twice at most, and few of them: two duplicated keys in one component of the cuckoo graph
    # cannot both be placed, whatever the seeds
    for n in (1000, 50000):
        uniq = rng.choice(2**32 - 1, size=n, replace=False).astype(np.uint32)
        keys = rng.permutation(np.concatenate([uniq, uniq[:8]]))
        vals = np.arange(keys.size, dtype=np.uint32)
        table, _ = ops.cuckoo_build(_dev(keys), _dev(vals), table_size=16 * keys.size)
        sk, sv = (t.cpu().numpy().view(np.uint32) for t in table.slots())
        assert np.array_equal(np.sort(sv[sk != 0xFFFFFFFF]), vals) and np.array_equal(keys[sv[sk != 0xFFFFFFFF]], sk[sk != 0xFFFFFFFF])
        p1 = positions_np(uniq, 2, table.seeds[0], table.size)
        p2 = positions_np(uniq, 2, table.seeds[1], table.size)
        at = np.where(sk[p1] == uniq, p1, p2)
        assert (sk[at] == uniq).all()
        gv, gf = (t.cpu().numpy().view(np.uint32) for t in table.lookup(_dev(uniq)))
        assert gf.all() and np.array_equal(gv, sv[at]), n


def test_fuzz_slab():
    """the slab table on random multiplicities (many distinct keys in few buckets: concurrent groups grow one chain):
    every stored row found once, none lost; join_probe against a numpy join"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(109)
    for n in _sizes(rng, 10, 19)[::3]:
        distinct = max(1, int(n / rng.choice([1, 2, 10, 300])))
        keys = rng.choice(2**32 - 1, size=distinct, replace=False).astype(np.uint32)[rng.integers(0, distinct, n)]
        uniq = np.unique(keys)  # the keys stored
        buckets = max(int(rng.choice([1, 3, 64, max(1, n // 20)])), n // 4096)  # chains of up to 128 slabs
        t = ops.SlabTable(buckets, -(-n // 32) + buckets + ops.SLAB_MAX_GROUPS)
        res = t.insert(_dev(keys), _dev(np.arange(n, dtype=np.uint32)), want_results=True).cpu().numpy()
        assert (res == 1).all() and t.status() == ops.DEV_OK, (n, buckets)
        K, V, _, _ = t.slabs()
        K, V = K.cpu().numpy().view(np.uint32), V.cpu().numpy().view(np.uint32)
        full = K != 0xFFFFFFFF
        assert np.array_equal(np.sort(V[full]), np.arange(n, dtype=np.uint32)), (n, buckets)  # each row once
        assert np.array_equal(keys[V[full]], K[full])
        gv, gf = (x.cpu().numpy().view(np.uint32) for x in t.lookup(_dev(uniq)))
        assert gf.all() and np.array_equal(keys[gv], uniq), (n, buckets)
        # join_probe: a hit carries (key, some build row's value of that key, the probe value), a miss three -1
        probe = np.concatenate([uniq[rng.integers(0, uniq.size, n // 2 + 1)],
                                rng.integers(0, 2**32 - 1, n // 2 + 1, dtype=np.uint64).astype(np.uint32)])
        pv = rng.integers(0, 2**32, probe.size, dtype=np.uint64).astype(np.uint32)
        ok, ob, op_ = (x.cpu().numpy().view(np.uint32) for x in t.join_probe(_dev(probe), _dev(pv)))
        hit = np.isin(probe, uniq)
        assert np.array_equal(ok, np.where(hit, probe, np.uint32(0xFFFFFFFF))), (n, buckets)
        assert np.array_equal(op_, np.where(hit, pv, np.uint32(0xFFFFFFFF)))
        assert (ob[~hit] == 0xFFFFFFFF).all() and np.array_equal(keys[ob[hit]], probe[hit])


# ---- the row-id operators: the seeded draws of tests/fuzz_testlib.py ------------------------------------------------------
# Every dimension of a draw is drawn on its own (tests/test_fuzz_draws_host.py shows, without a GPU, that each set holds
# every category and rejects a list of defective backends).  Each draw runs once through the raw entry point on guarded
# buffers and is compared exactly with the operator's numpy model; the draws of a sweep share one guarded workspace that
# starts as random bytes and is never cleared; every fourth draw also goes through the tensor front door.
def _sweep(name):
    from tests import fuzz_gpu_testlib as fg
    from tests.test_fuzz_draws_host import DRAWS
    s = fg.sweep(name)
    assert s.calls == DRAWS[name] and s.doors == -(-s.calls // 4)


def test_fuzz_sort_pairs():
    """dbhip_radix_sort_pairs_u32 and _i32, carried values and the argsort, both digit widths, every key distribution:
    the stable order of numpy"""
    _sweep("sort_pairs")


def test_fuzz_sorted_search_and_range_join():
    """the fence ladder built into the shared workspace and the search through it: column sizes at fan-out 64 and every
    allowed top_entries, each top_entries, the column off its boundary, lo, hi or both, hi below lo, either output NULL;
    every fourth draw through ops.sorted_search and ops.range_join"""
    _sweep("sorted_search")


def test_fuzz_join_pairs():
    """dbhip_join_pairs_u32 on the (ids, pos, cnt) of a join, with and without probe row ids, every column at its own
    offset, capacities below, at and above the total and the count-only call, ranges that leave the id buffer, totals
    beyond 2^32"""
    _sweep("join_pairs")


def test_fuzz_topk():
    """dbhip_topk_u32 and _i32: n at the segment's and the chunk's seams, k from 0 to n + 5, largest, signed, sorted, every
    key distribution (ties at the k-th key by ascending row)"""
    _sweep("topk")


def test_fuzz_reduce_by_key():
    """dbhip_reduce_by_key_u32: run lengths 1, about 1.5, about 40 and one run, a key that returns, each output column
    given or NULL, capacities below, at and above the number of runs and the count-only call, sums past 2^32"""
    _sweep("reduce_by_key")


def test_fuzz_scan_by_key():
    """dbhip_scan_by_key_u32: the same run shapes, each output column given or NULL, signed and unsigned values at both
    ends of the range"""
    _sweep("scan_by_key")


def test_fuzz_dictionary():
    """dbench_dict_build_u32 and the encode of another column through the dictionary it left: capacities below, at and
    above the number of distinct values, both orders, both device counts, present and absent values, the miss count"""
    _sweep("dict")


def test_fuzz_select():
    """dbench_select_range_u32 over all rows and through lists: sizes at the segment's seams and one draw of more than
    1024 segments, offsets of column, list and output, every kind of device count, signed, negate, the count alone"""
    _sweep("select")


def test_fuzz_merge_and_set_operations():
    """dbench_setop_u32 (one draw of more than 1024 tiles) and dbench_merge_u32 in its three value modes: sizes at the
    tile's seams split every way over A and B, both device counts, duplicates across the tile edges, both orders"""
    _sweep("merge")


def test_fuzz_take_and_aggregate():
    """dbench_take_u32 of one to four columns and dbench_aggregate_rows_u32: every column, list and output at its own
    offset, row ids outside the column with and without OUTER, sums past 2^32, values at both ends of the signed range"""
    _sweep("take")


def test_fuzz_bitpack():
    """pack, unpack and the filter on packed codes: widths 1 to 32 over a base, rows that do not fit, codes across word
    edges, lists with ids outside the column, one filter of more than 1024 segments"""
    _sweep("bitpack")


def test_fuzz_row_id_queries():
    """twenty random plans of 3 to 6 steps over 2 to 4 columns of up to 2^17 rows - select, refine, union / intersect /
    difference of two earlier lists, take, aggregate, the filter on a packed copy of a column, encode and decode through a
    dictionary - every count on the device until the one synchronisation at the end, against the same plan in numpy"""
    from tests import fuzz_gpu_testlib as fg
    from tests import fuzz_testlib as ft
    plans = list(ft.plan_draws(np.random.default_rng(211)))
    assert len(plans) == 20 and {s["step"] for p in plans for s in p["steps"]} == set(ft.PLAN_STEPS)
    for plan in plans:
        assert 3 <= len(plan["steps"]) <= 6 and 2 <= len(plan["cols"]) <= 4 and plan["n"] <= 1 << 17
        fg.check_plan(plan, fg.run_plan(plan))
