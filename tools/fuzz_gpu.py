"""development aid: randomized parity runs of the HIP paths against numpy (sizes, alignments, value distributions the
fixed test lists do not cover).  The eleven newer operators (sort pairs, join pairs, top-k, reduce- and scan-by-key,
sorted search, select, merge and set operations, take and aggregate, dictionary, bit-packed columns) run the draws of
tests/fuzz_testlib.py through tests/fuzz_gpu_testlib.py on guarded buffers, a few per round, on one never-cleared
workspace per operator, and one random query plan over the row-id operators per round: the tool needs the repository's
tests directory beside it.  python tools/fuzz_gpu.py [seconds] [seed]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from dwarf_bench_amd import ops
from tests import fuzz_gpu_testlib as fg
from tests import fuzz_testlib as ft

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
t_end = time.time() + budget
done = {"scan": 0, "dense": 0, "sort": 0, "groupby": 0, "xscan": 0, "reduce": 0, "join": 0, "radix_join": 0, "crowded": 0, "ujoin": 0,
        "groupby_hash": 0, "cuckoo": 0, "slab": 0, "plans": 0}
done.update({name: 0 for name in ft.OPERATORS})
ROW_ID_DRAWS = 4  # per operator and round
sweeps = {name: (fg.Sweep(name, 1 << 20, seed), fg.endless(name, 1000 * seed + 7)) for name in ft.OPERATORS}
plans = ft.plan_draws(np.random.default_rng(seed), plans=1 << 30)


def rand_n():
    kind = rng.integers(0, 4)
    if kind == 0:
        return int(rng.integers(0, 5000))
    if kind == 1:
        return int(rng.choice([4096, 8192, 32768, 65536, 1 << 20])) + int(rng.integers(-3, 4))
    if kind == 2:
        return int(rng.integers(5000, 3_000_000))
    return int(rng.integers(3_000_000, 20_000_000))


def rand_values(n, dtype):
    kind = rng.integers(0, 6)
    if kind == 0:
        v = rng.integers(0, 2**32, n, dtype=np.uint64)
    elif kind == 1:
        v = rng.integers(1, 10001, n, dtype=np.uint64)
    elif kind == 2:
        v = np.full(n, int(rng.integers(0, 2**32)), dtype=np.uint64)
    elif kind == 3:
        v = rng.integers(0, 4, n, dtype=np.uint64) << int(rng.integers(0, 30))
    elif kind == 4:
        v = np.sort(rng.integers(0, 2**32, n, dtype=np.uint64))[::-1].copy()
    else:
        v = rng.integers(0, 2**32, n, dtype=np.uint64) & np.uint64(0xFFFF00FF)
    return v.astype(np.uint32).view(dtype)


def fmix32_inv(h):
    """inverse of the joins' key hash (murmur3's 32-bit finaliser is a bijection)"""
    h = h.astype(np.uint64) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7ED1B41D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h ^= h >> np.uint64(26)
    h = (h * np.uint64(0xA5CB9243)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def crowd(count, bits=None, top=None):
    """`count` distinct keys whose hashes share their top `bits` bits: whatever the join's geometry, they meet in one
    partition (or in a few neighbours when it has more than 2^bits partitions) — more keys than an LDS sub-table holds"""
    bits = int(rng.integers(12, 22)) if bits is None else bits
    top = int(rng.integers(0, 1 << bits)) if top is None else top
    space = 1 << (32 - bits)
    low = rng.choice(space, size=min(count, space), replace=False).astype(np.uint64)
    keys = fmix32_inv((np.uint64(top) << np.uint64(32 - bits)) | low)
    return keys[keys != 0xFFFFFFFF], bits, top


it = 0
while time.time() < t_end:
    it += 1
    n = rand_n()
    off = int(rng.integers(0, 4))
    # ---- scan, both entry points, unaligned views
    host = rand_values(n + off, np.int32)
    dev = torch.from_numpy(host).cuda()[off:]
    filt = int(rng.choice([np.iinfo(np.int32).min, -5, 0, 5, 5001, 2**30, np.iinfo(np.int32).max,
                           int(host[rng.integers(0, len(host))]) if len(host) else 1]))
    want = host[off:][host[off:] < filt]
    for dense in (False, True):
        got = ops.copy_if_lt(dev, filt, dense=dense).cpu().numpy()
        assert np.array_equal(got, want), ("scan", n, off, filt, dense)
        done["dense" if dense else "scan"] += 1
    # ---- reduce, exclusive scan
    assert int(ops.reduce_sum(dev)) & 0xFFFFFFFF == int(host[off:].astype(np.int64).sum()) & 0xFFFFFFFF, ("reduce", n, off)
    done["reduce"] += 1
    if n:
        u = torch.from_numpy(host.view(np.uint32).astype(np.int64).astype(np.int32)).cuda()[off:]
        exp = np.concatenate((np.zeros(1, np.uint64), np.cumsum(host[off:].view(np.uint32).astype(np.uint64))[:-1])) & np.uint64(0xFFFFFFFF)
        got = ops.exclusive_scan(u).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp.astype(np.uint32)), ("xscan", n, off)
        done["xscan"] += 1
    # ---- sort (16-byte aligned columns), both widths, signed and unsigned
    if n:
        keys = rand_values(n, np.uint32)
        for bits in (8, 4):
            signed = bool(rng.integers(0, 2))
            d = torch.from_numpy(keys.view(np.int32).copy()).cuda()
            ops.radix_sort_(d, signed=signed, radix_bits=bits)
            got = d.cpu().numpy()
            exp = np.sort(keys.view(np.int32)) if signed else np.sort(keys).view(np.int32)
            assert np.array_equal(got, exp), ("sort", n, bits, signed)
            done["sort"] += 1
    # ---- group-by
    if n:
        groups = int(rng.choice([1, 7, 64, 1000, 4096, 40000, 65536, 100000]))
        gk = (rand_values(n, np.uint32).astype(np.uint64) % groups).astype(np.uint32)
        gv = rand_values(n, np.uint32)
        got = ops.groupby_sum(torch.from_numpy(gk.view(np.int32)).cuda(), torch.from_numpy(gv.view(np.int32)).cuda(), groups)
        exp = np.zeros(groups, dtype=np.uint64)
        np.add.at(exp, gk, gv.astype(np.uint64))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), (exp & 0xFFFFFFFF).astype(np.uint32)), ("groupby", n, groups)
        done["groupby"] += 1
    # ---- one-to-many join, both forms: counts for every probe row, id lists for a sample of them
    nb, npb = min(rand_n(), 4_000_000), min(rand_n(), 4_000_000)
    if nb and npb:
        dom = int(rng.choice([4, 1000, max(nb // 4, 1), nb, 4 * nb, 2**32 - 1]))
        bk = rng.integers(0, dom, nb, dtype=np.uint64).astype(np.uint32)
        pk = rng.integers(0, dom, npb, dtype=np.uint64).astype(np.uint32)
        if dom <= 4 and nb > 200_000:  # a handful of keys with hundreds of thousands of rows each: keep it bounded
            bk = bk[:200_000].copy(); nb = bk.size
        if it % 3 == 0:  # a crowd: thousands of distinct keys in one partition (the spill tables), each with a few rows
            mine, bits, top = crowd(int(rng.integers(100, 30000)))
            per = int(rng.integers(1, 12))
            rows = np.repeat(mine[: max(1, min(mine.size, nb // per))], per)[:nb]
            bk[: rows.size] = rows
            bk = rng.permutation(bk)
            others, _, _ = crowd(2000, bits, top)  # the same partition: some of them build keys, most of them misses
            pk[::3] = mine[rng.integers(0, mine.size, pk[::3].size)]
            pk[1::3] = others[rng.integers(0, others.size, pk[1::3].size)]
            dom = -mine.size
            done["crowded"] += 1
        uniq, inv_cnt = np.unique(bk, return_counts=True)
        idx = np.searchsorted(uniq, pk)
        idx[idx >= uniq.size] = 0
        want_cnt = np.where(uniq[idx] == pk, inv_cnt[idx], 0).astype(np.uint32)
        order = np.argsort(bk, kind="stable")
        starts = np.concatenate((np.zeros(1, np.int64), np.cumsum(inv_cnt)[:-1]))
        d_bk, d_pk = torch.from_numpy(bk.view(np.int32)).cuda(), torch.from_numpy(pk.view(np.int32)).cuda()
        hj = ops.HashJoin(nb, npb)
        hj.build(d_bk); hj.probe(d_pk)
        pos, cnt, ids = (t.cpu().numpy() for t in hj.result())
        assert np.array_equal(cnt.view(np.uint32), want_cnt), ("join cnt", nb, npb, dom)
        for r in rng.integers(0, npb, 64):
            c = int(want_cnt[r])
            if c:
                exp_rows = order[starts[idx[r]]: starts[idx[r]] + c]
                assert np.array_equal(np.sort(ids[pos[r]: pos[r] + c]), np.sort(exp_rows)), ("join ids", nb, npb, dom, int(r))
        done["join"] += 1
        rid, rpos, rcnt, rids = (t.cpu().numpy() for t in ops.radix_join(d_bk, d_pk))
        assert np.array_equal(np.sort(rid), np.arange(npb)), ("radix join rows", nb, npb, dom)
        assert np.array_equal(rcnt.view(np.uint32), want_cnt[rid]), ("radix join cnt", nb, npb, dom)
        for j in rng.integers(0, npb, 64):
            c, r = int(rcnt[j]), int(rid[j])
            if c:
                exp_rows = order[starts[idx[r]]: starts[idx[r]] + c]
                assert np.array_equal(np.sort(rids[rpos[j]: rpos[j] + c]), np.sort(exp_rows)), ("radix join ids", nb, npb, dom, r)
        done["radix_join"] += 1
    # ---- unique-key payload join: hits carry (key, build value, probe value), misses three 0xFFFFFFFF
    nu = min(rand_n(), 3_000_000)
    if nu:
        if it % 2:
            uk, _, _ = crowd(min(nu, 200_000), bits=int(rng.integers(8, 14)))
        else:
            uk = np.unique(rng.integers(0, int(rng.choice([4 * nu, 2**32 - 1])), nu, dtype=np.uint64).astype(np.uint32))
        uk = rng.permutation(uk)
        uv = rng.integers(0, 2**32 - 1, uk.size, dtype=np.uint64).astype(np.uint32)
        m = min(rand_n(), 3_000_000) or 1
        qk = rng.integers(0, 2**32 - 1, m, dtype=np.uint64).astype(np.uint32)
        qk[::2] = uk[rng.integers(0, uk.size, qk[::2].size)]
        qv = rng.integers(0, 2**32 - 1, m, dtype=np.uint64).astype(np.uint32)
        uj = ops.UniqueJoin(uk.size, m)
        uj.build(torch.from_numpy(uk.view(np.int32)).cuda(), torch.from_numpy(uv.view(np.int32)).cuda())
        uj.probe(torch.from_numpy(qk.view(np.int32)).cuda(), torch.from_numpy(qv.view(np.int32)).cuda())
        ok_, ob, op_ = (t.cpu().numpy().view(np.uint32) for t in uj.result())
        srt = np.argsort(uk, kind="stable")
        at = np.searchsorted(uk[srt], qk)
        at[at >= uk.size] = 0
        hit = uk[srt][at] == qk
        miss = np.uint32(0xFFFFFFFF)
        assert np.array_equal(ok_, np.where(hit, qk, miss)), ("ujoin keys", uk.size, m)
        assert np.array_equal(ob, np.where(hit, uv[srt][at], miss)), ("ujoin build vals", uk.size, m)
        assert np.array_equal(op_, np.where(hit, qv, miss)), ("ujoin probe vals", uk.size, m)
        done["ujoin"] += 1
    # ---- hash group-by: any keys (a crowd on one partition every third round), a bound at, above or below the answer
    ng = min(rand_n(), 4_000_000)
    if ng:
        if it % 3 == 0:
            pool = crowd(int(rng.integers(100, 6000)))[0]
            gk = pool[rng.integers(0, pool.size, ng)]
        else:
            gk = rand_values(ng, np.uint32)
        gv = rand_values(ng, np.uint32)
        uk, inv = np.unique(gk, return_inverse=True)
        d = uk.size
        bound = int(rng.choice([d, d + int(rng.integers(1, 100)), max(1, d - 1), 0]))
        counts = bool(rng.integers(0, 2))
        plan = ops.GroupByHash(ng, bound)
        plan.launch(torch.from_numpy(gk.view(np.int32)).cuda(), torch.from_numpy(gv.view(np.int32)).cuda(), counts=counts)
        st = ops.workspace_status(plan.ws)
        if bound and bound < d:
            assert st & ops.DEV_TABLE_FULL and int(plan.groups.item()) == bound, ("groupby_hash bound", ng, d, bound)
        else:
            k, s, c = plan.result()
            k = k.cpu().numpy().view(np.uint32)
            o = np.argsort(k)
            sums = np.zeros(d, dtype=np.uint64)
            np.add.at(sums, inv, gv.astype(np.uint64))
            assert np.array_equal(k[o], uk), ("groupby_hash keys", ng, d, bound)
            assert np.array_equal(s.cpu().numpy().view(np.uint32)[o], (sums & 0xFFFFFFFF).astype(np.uint32)), ("groupby_hash sums", ng, d)
            if counts:
                assert np.array_equal(c.cpu().numpy().view(np.uint32)[o], np.bincount(inv).astype(np.uint32)), ("groupby_hash counts", ng, d)
        done["groupby_hash"] += 1
    # ---- cuckoo table (hash kind 2): unique keys at load 0.1-0.45, lookups of present and absent keys
    nc = min(rand_n(), 2_000_000)
    if nc:
        ck = rng.choice(2**32 - 1, size=nc, replace=False).astype(np.uint32)
        cv = rand_values(nc, np.uint32)
        table, _ = ops.cuckoo_build(torch.from_numpy(ck.view(np.int32)).cuda(), torch.from_numpy(cv.view(np.int32)).cuda(),
                                    table_size=max(8, int(nc / rng.uniform(0.1, 0.45))), seed=it)
        q = np.concatenate([ck, rng.integers(0, 2**32 - 1, nc, dtype=np.uint64).astype(np.uint32)])
        gv_, gf_ = (t.cpu().numpy().view(np.uint32) for t in table.lookup(torch.from_numpy(q.view(np.int32)).cuda()))
        srt = np.argsort(ck)
        at = np.minimum(np.searchsorted(ck[srt], q), nc - 1)
        hit = ck[srt][at] == q
        assert np.array_equal(gf_, hit.astype(np.uint32)) and np.array_equal(gv_, np.where(hit, cv[srt][at], 0)), ("cuckoo", nc)
        done["cuckoo"] += 1
    # ---- slab table: random multiplicities in few or many buckets, every row stored once and found
    ns = min(rand_n(), 1_000_000)
    if ns:
        sk = rand_values(ns, np.uint32) % np.uint32(max(1, ns // int(rng.choice([1, 3, 50]))))
        sk[sk == 0xFFFFFFFF] = 0
        buckets = max(int(rng.choice([1, 7, max(1, ns // 20)])), ns // 4096)
        st_ = ops.SlabTable(buckets, -(-ns // 32) + buckets + ops.SLAB_MAX_GROUPS)
        st_.insert(torch.from_numpy(sk.view(np.int32)).cuda(), torch.arange(ns, dtype=torch.int32, device="cuda"))
        assert st_.status() == ops.DEV_OK, ("slab status", ns, buckets)
        K, V, _, _ = st_.slabs()
        K, V = K.cpu().numpy().view(np.uint32), V.cpu().numpy().view(np.uint32)
        full = K != 0xFFFFFFFF
        assert np.array_equal(np.sort(V[full]), np.arange(ns, dtype=np.uint32)) and np.array_equal(sk[V[full]], K[full]), ("slab rows", ns, buckets)
        uq = np.unique(sk)
        lv, lf = (t.cpu().numpy().view(np.uint32) for t in st_.lookup(torch.from_numpy(uq.view(np.int32)).cuda()))
        assert lf.all() and np.array_equal(sk[lv], uq), ("slab lookup", ns, buckets)
        done["slab"] += 1
    # ---- the row-id operators: seeded draws with every dimension drawn on its own, and one random query plan
    for name, (sweep, cases) in sweeps.items():
        for _ in range(ROW_ID_DRAWS):
            case = next(cases)
            try:
                sweep.step(case)
            except AssertionError as e:
                raise AssertionError(f"{name}: {fg.describe(case)}: {e}") from e
            done[name] += 1
    plan = next(plans)
    fg.check_plan(plan, fg.run_plan(plan))
    done["plans"] += 1
    if it % 10 == 0:
        print(f"{it} iterations {done}", flush=True)
print("fuzz ok", it, done)
