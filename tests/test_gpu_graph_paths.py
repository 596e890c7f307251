"""One capture, replays whose data take another device-side path than the captured run.

include/dbhip.h promises that nothing allocates, frees or synchronises, "so a call sequence can be captured into a
hipGraph".  A graph freezes every host-side decision and every kernel argument; what the kernels decide from the data —
skipped sort passes, packed or wide group-by tables, spilled and giant join partitions, the side sum of key 0xFFFFFFFF,
a status word — changes from replay to replay.  A word that an eager call clears on its host path but no node of the
captured sequence clears would make the replay AFTER a flagged or spilling replay wrong, and only that one.

Every family below captures its call sequence on the first input of a list, replays the others in order and the first
one again (tests/graph_testlib.run_family): a flagged replay is always followed by a clean one whose status must read 0.
Before every replay the outputs hold a guard word and the workspace a poison; after it the status word, the oracle's
answer, and an eager run of the same calls on the same input in a second set of buffers (bitwise where the header
defines the output uniquely, in a canonical form where it leaves an order open).

What path an input takes is observed through the status value, the group-by's mode word, or it is the construction's
own guarantee as the test that owns the construction argues it (tests/test_gpu_workspace_reuse.py, join_testlib,
groupby_hash_testlib, test_gpu_buffer_bounds)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests import graph_testlib as gl
from tests import groupby_hash_testlib as gh
from tests import join_testlib as jt
from tests import sort_pass_testlib as sp
from tests.cuckoo_model import CuckooModel, mix64_np, murmur3_x86_32_np
from tests.graph_testlib import Buffers, Input, run_family, u32
from tests.guard_testlib import FILLS, i32, i64
from tests.pjoin_testlib import dest_of, fmix32
from tests.slab_model import SlabModel
from tests.test_gpu_buffer_bounds import _kernel_would_pack, _packed_case, _sample_rows, _sum64
from tests.validator_model import fingerprint as _host_fingerprint, weighted_sum as _weighted
from tests.test_gpu_workspace_reuse import _crowded, _probe, _unique_crowd

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF
OK, KEY_RANGE, TABLE_FULL = 0, 2, 4


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _i32(n):
    return torch.empty(max(int(n), 1), dtype=torch.int32, device="cuda")[: int(n)]


def _i64(n):
    return torch.empty(int(n), dtype=torch.int64, device="cuda")


def _ws(nbytes):
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _off(n, words):
    """an int32 column of n words that starts `words` 4-byte words past a 16-byte boundary"""
    base = _i32(n + 8)
    assert base.data_ptr() % 16 == 0
    return base[words: words + n]


def _rc(rc):
    assert rc == 0, rc


# ---- scan ---------------------------------------------------------------------------------------------------------------
SCAN_FILTER = 50


def _scan_inputs(n):
    ref = po.gen_uniform_u32(n, 1, 1, 10000)
    last = po.gen_uniform_u32(n, 4, SCAN_FILTER, 10000)
    last[-1000:] = po.gen_uniform_u32(1000, 5, 1, SCAN_FILTER - 1)  # matches in the last chunk only
    return [Input([ref], name="reference column"),
            Input([po.gen_uniform_u32(n, 2, SCAN_FILTER, 10000)], name="no row matches"),
            Input([po.gen_uniform_u32(n, 3, 1, SCAN_FILTER - 1)], name="every row matches"),
            Input([last], name="matches in the last chunk only")]


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_scan_replays_change_the_selectivity(n, dense, unaligned):
    """dbhip_copy_if_lt_i32 / _dense_i32 with the filter (and, unaligned, the columns' alignment) frozen: 1 % of the rows
    match, none, all, the last 1000.  out[out_size, n) is never written: those words keep the guard."""
    lib = _lib()
    fn = lib.dbhip_copy_if_lt_dense_i32 if dense else lib.dbhip_copy_if_lt_i32
    ws_bytes = lib.dbhip_copy_if_lt_i32_workspace_bytes(n)

    def make():
        src, out = _off(n, 1 if unaligned else 0), _off(n, 3 if unaligned else 0)
        size, ws = _i64(1), _ws(ws_bytes)

        def read():
            m = int(size.item())
            assert 0 <= m <= n
            return {"out": out[:m].cpu().numpy(), "size": np.array([m]), "rest": out[m:].cpu().numpy()}
        return Buffers([src], [out, size], [ws], [ws], lambda: _rc(fn(src.data_ptr(), n, SCAN_FILTER, out.data_ptr(),
                       size.data_ptr(), ws.data_ptr(), ws_bytes, _s())), read)

    def check(inp, got):
        assert np.array_equal(got["out"], po.copy_if_lt(inp.cols[0].view(np.int32), SCAN_FILTER))
        assert np.unique(got["rest"]).size <= 1 and (got["rest"].size == 0 or
                                                     int(got["rest"][0]) in [i32(f) for f in FILLS])

    def canon(r):  # the two instances hold different guard words behind the matches
        return {"out": r["out"], "size": r["size"]}
    run_family(make, _scan_inputs(n), check, canon)


# ---- exclusive scan, the three-launch path of unaligned columns ---------------------------------------------------------
@pytest.mark.parametrize("place", [(1, 0, False), (0, 3, False), (1, 1, True)], ids=["src+1", "dst+3", "in place"])
@pytest.mark.parametrize("n", [4097, (1 << 20) + 5])
def test_exclusive_scan_three_launch_path(n, place):
    """src one word, dst three words off a 16-byte boundary, and in place on an unaligned column: three launches whose
    middle one scans the tile sums in the workspace.  Full-range values and all-ones words wrap the sum around."""
    lib = _lib()
    so, do, in_place = place
    ws_bytes = lib.dbhip_exclusive_scan_u32_workspace_bytes(n)
    init = 0xFFFFFF00

    def make():
        src = _off(n, so)
        dst = src if in_place else _off(n, do)
        ws = _ws(ws_bytes)
        return Buffers([src], [] if in_place else [dst], [ws], [ws],
                       lambda: _rc(lib.dbhip_exclusive_scan_u32(src.data_ptr(), n, init, dst.data_ptr(), ws.data_ptr(),
                                                                ws_bytes, _s())), lambda: {"dst": u32(dst)})

    def check(inp, got):
        h = inp.cols[0].astype(np.uint64)
        want = (np.uint64(init) + np.concatenate([np.zeros(1, np.uint64), np.cumsum(h)[:-1]])) & np.uint64(M32)
        assert np.array_equal(got["dst"], want.astype(np.uint32))

    inputs = [Input([po.gen_uniform_u32(n, 1, 0, M32)], name="full range"),
              Input([po.gen_uniform_u32(n, 2, 0, 3)], name="small values"),
              Input([np.full(n, M32, np.uint32)], name="every word 0xFFFFFFFF"),
              Input([po.gen_uniform_u32(n, 3, 0, M32)], name="full range again")]
    run_family(make, inputs, check)


# ---- sorts ----------------------------------------------------------------------------------------------------------------
def _sort_inputs(n, pairs):
    full = po.gen_uniform_u32(n, 1, 0, M32)
    # behind the captured run (pass 0 executed): pass 0 skipped, then executed again with the passes between the two
    # ends skipped (tests/sort_pass_testlib.py: exactly the bytes of the mask vary, the others hold a constant)
    cols = [(full, "full range"), (sp.keys_for(0x00FF0000, n, 5, sp.BASE_NEG), "only byte 2 varies: pass 0 skipped"),
            (sp.keys_for(0xFF0000FF, n, 6, sp.BASE), "bytes 0 and 3 vary"),
            (po.gen_uniform_u32(n, 2, 1, 10000), "keys in [1, 10000]: skipped passes"),
            (np.full(n, 0x80000007, np.uint32), "all keys equal: no pass runs"),
            (np.sort(po.gen_uniform_u32(n, 3, 0, M32)), "already sorted"), (po.gen_uniform_u32(n, 4, 0, M32), "full range")]
    return [Input([k] + ([po.gen_uniform_u32(n, 10 + i, 0, M32)] if pairs else []), name=name)
            for i, (k, name) in enumerate(cols)]


@pytest.mark.parametrize("n", [4097, (1 << 20) + 777])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("kind", ["u32", "i32", "pairs_u32", "pairs_i32"])
def test_sort_replays_change_the_executed_passes(kind, bits, n):
    """keys-only and key-value sorts with real values, unsigned and signed.  Keys in [1, 10000] skip the upper passes,
    so the result comes out of the other ping-pong buffer than in the captured run; equal keys run no pass at all.
    The keys in order, the values vals_in[stable argsort], status 0 (DBHIP_DEV_RANK_ORDER would show here)."""
    lib = _lib()
    pairs, signed = kind.startswith("pairs"), kind.endswith("i32")
    fn = getattr(lib, "dbhip_radix_sort_" + kind)
    ws_bytes = lib.dbhip_radix_sort_workspace_bytes(n, bits)

    def make():
        keys, tmp, ws = _i32(n), _i32(n), _ws(ws_bytes)
        if not pairs:
            return Buffers([keys], [tmp], [ws], [ws], lambda: _rc(fn(keys.data_ptr(), tmp.data_ptr(), n, bits,
                           ws.data_ptr(), ws_bytes, _s())), lambda: {"keys": u32(keys)})
        vals, tmpv = _i32(n), _i32(n)
        return Buffers([keys, vals], [tmp, tmpv], [ws], [ws],
                       lambda: _rc(fn(keys.data_ptr(), vals.data_ptr(), tmp.data_ptr(), tmpv.data_ptr(), n, bits, 0,
                                      ws.data_ptr(), ws_bytes, _s())), lambda: {"keys": u32(keys), "vals": u32(vals)})

    def check(inp, got):
        k = inp.cols[0]
        order = np.argsort(k.view(np.int32) if signed else k, kind="stable")
        assert np.array_equal(got["keys"], k[order])
        if pairs:
            assert np.array_equal(got["vals"], inp.cols[1][order])
    run_family(make, _sort_inputs(n, pairs), check)


def test_sort_prepare_is_refused_inside_a_capture():
    """dbhip_radix_sort_prepare, the one call that allocates and synchronises, returns DBHIP_EINVAL while its stream is
    being captured, leaves the capture intact, and the sort captured behind it replays correctly"""
    lib = _lib()
    n, bits = (1 << 18) + 3, 8
    ws_bytes = lib.dbhip_radix_sort_workspace_bytes(n, bits)
    keys, tmp, ws = _i32(n), _i32(n), _ws(ws_bytes)
    rcs = []

    def run():
        rcs.append(lib.dbhip_radix_sort_prepare(_s()))
        _rc(lib.dbhip_radix_sort_u32(keys.data_ptr(), tmp.data_ptr(), n, bits, ws.data_ptr(), ws_bytes, _s()))
    gl.fill(keys, po.gen_uniform_u32(n, 1, 0, M32))
    g = gl.capture(run)
    assert rcs[0] in (0, 1) and rcs[1] == -1, rcs  # eager: the rank mode; inside the capture: DBHIP_EINVAL
    for seed, hi in ((2, M32), (3, 10000), (4, M32)):
        host = po.gen_uniform_u32(n, seed, 0, hi)
        gl.fill(keys, host)
        gl.poison(ws, "0xff")
        g.replay()
        torch.cuda.synchronize()
        assert gl.status(ws) == 0 and np.array_equal(u32(keys), np.sort(host))


# ---- dense group-by ---------------------------------------------------------------------------------------------------------
def _gb_want(k, v, groups):
    """exact wrap-around sums of the rows whose key is below groups (two 16-bit halves through float64 bincounts)"""
    ok = k < groups
    k, v = k[ok].astype(np.int64), v[ok]
    lo = np.bincount(k, weights=(v & np.uint32(0xFFFF)).astype(np.float64), minlength=groups).astype(np.uint64)
    hi = np.bincount(k, weights=(v >> np.uint32(16)).astype(np.float64), minlength=groups).astype(np.uint64)
    return ((lo + (hi << np.uint64(16))) & np.uint64(M32)).astype(np.uint32)


def _gb_make(n, groups, tables, mode_word=False):
    lib = _lib()
    ws_bytes = lib.dbhip_groupby_sum_u32_workspace_bytes(n, groups)

    def make():
        keys, vals, out, ws = _i32(n), _i32(n), _i32(groups), _ws(ws_bytes)

        def run():
            if tables is None:
                _rc(lib.dbhip_groupby_sum_u32(keys.data_ptr(), vals.data_ptr(), n, groups, out.data_ptr(),
                                              ws.data_ptr(), ws_bytes, _s()))
            else:
                _rc(lib.dbhip_groupby_partial_u32(keys.data_ptr(), vals.data_ptr(), n, groups, tables, ws.data_ptr(),
                                                  ws_bytes, _s()))
                _rc(lib.dbhip_groupby_merge_u32(groups, tables, out.data_ptr(), ws.data_ptr(), _s()))

        def read():
            r = {"out": u32(out)}
            if mode_word:
                r["mode"] = np.array([int(ws[4:8].view(torch.int32).item())])
            return r
        return Buffers([keys, vals], [out], [ws], [ws], run, read)
    return make


@pytest.mark.parametrize("groups", [64, 40000, 65536])
@pytest.mark.parametrize("tables", [None, 0, 3], ids=["fused", "partial+merge, 0", "partial+merge, 3"])
def test_dense_groupby_replays(tables, groups):
    """the fused call and partial + merge: uniform keys, every row one group (one hot counter), one key equal to
    `groups` (DBHIP_DEV_KEY_RANGE, that row ignored, every other group right), full-range values (wrap-around)"""
    n = (1 << 20) + 8
    one = np.full(n, groups // 3, np.uint32)
    flagged = po.gen_uniform_u32(n, 5, 0, groups - 1)
    flagged[n // 2 + 1] = groups
    inputs = [Input([po.gen_uniform_u32(n, 1, 0, groups - 1), po.gen_uniform_u32(n, 2, 1, 10000)], name="uniform"),
              Input([one, po.gen_uniform_u32(n, 3, 1, 10000)], name="every row one group"),
              Input([flagged, po.gen_uniform_u32(n, 6, 1, 10000)], status=KEY_RANGE, name="one key == groups"),
              Input([po.gen_uniform_u32(n, 7, 0, groups - 1), po.gen_uniform_u32(n, 8, 0, M32)], name="full-range values")]

    def check(inp, got):
        assert np.array_equal(got["out"], _gb_want(inp.cols[0], inp.cols[1], groups))
    seen = run_family(_gb_make(n, groups, tables), inputs, check)
    assert [s[0] for s in seen] == [0, 0, KEY_RANGE, 0, 0]


def test_dense_groupby_packed_wide_packed_under_one_capture():
    """2^25 rows, 65536 groups: the kernel chooses its tables from a 768-row sample of the data.  Captured on BASELINE's
    column (packed tables, mode word 1); replayed on test_gpu_buffer_bounds._packed_case('wide values') with the sampled
    windows wide as well, so that the kernel must take the wide tables (mode 2); then the packing column again (1)."""
    from dwarf_bench_amd import ops
    n, groups = 1 << 25, 65536
    cus = ops.device_info()[1]
    packing = [po.gen_uniform_u32(n, 42, 0, groups - 1), po.gen_uniform_u32(n, 43, 1, 10000)]
    wk, wv = _packed_case(n, groups, "wide values")
    wv[_sample_rows(n)] = M32
    assert _kernel_would_pack(n, groups, packing[0], packing[1], cus)[0]
    assert not _kernel_would_pack(n, groups, wk, wv, cus)[0]
    inputs = [Input(packing, name="packing column", mode=1), Input([wk, wv], name="wide values", mode=2)]

    def check(inp, got):
        assert int(got["mode"][0]) == inp.facts["mode"], ("mode word", got["mode"])
        assert np.array_equal(got["out"], _gb_want(inp.cols[0], inp.cols[1], groups))
    run_family(_gb_make(n, groups, None, mode_word=True), inputs, check)


# ---- hash group-by ----------------------------------------------------------------------------------------------------------
def _gbh_inputs(path):
    """-> n, max_groups, inputs.  'part': 2^21 rows under a bound of n - 1000 groups (above 4096: the partitioned path);
    'lds': 2^20 rows under a bound of 4096 (private LDS tables).  The giant-partition case is
    groupby_hash_testlib.CASES['giant_edge_32769'] (a partition of 32769 rows: two slices of gbh_giant_kernel); path a
    has no partitions, its entry of that place is CASES['lds_home_100_extras'] (100 keys on one LDS home, a hot key and
    0xFFFFFFFF rows on the same home: rows overflow into the global table)."""
    rng = np.random.default_rng(31)
    if path == "part":
        n = 1 << 21
        mg = n - 1000
        pool = np.unique(rng.integers(0, M32, size=1 << 20, dtype=np.uint64).astype(np.uint32))  # the bound holds them
        special = gh.CASES["giant_edge_32769"]()
        over = rng.permutation(np.arange(7, 7 + n, dtype=np.uint32))  # n distinct keys
    else:
        n = 1 << 20
        mg = gh.LDS_MAX_GROUPS
        pool = rng.choice(M32, size=3000, replace=False).astype(np.uint32)
        special = gh.CASES["lds_home_100_extras"]()
        over = rng.choice(M32, size=5000, replace=False).astype(np.uint32)[rng.integers(0, 5000, n)]
    assert special.keys.size == n and special.distinct <= mg

    def uniform():
        return pool[rng.integers(0, pool.size, n)]
    hot = uniform()
    hot[rng.random(n) < 0.5] = hot[0]
    ff = uniform()
    ff[rng.random(n) < 0.1] = M32
    assert np.unique(over).size > mg
    cols = [(uniform(), OK, "uniform"), (hot, OK, "a hot key on half the rows"), (ff, OK, "rows carrying 0xFFFFFFFF"),
            (special.keys, OK, special.name), (over, TABLE_FULL, "more distinct keys than max_groups"),
            (uniform(), OK, "uniform again")]
    return n, mg, [Input([k, gh.rand_vals(rng, n)], status=st, name=name) for k, st, name in cols]


@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no counts"])
@pytest.mark.parametrize("path", ["lds", "part"])
def test_hash_groupby_replays(path, counts):
    """dbhip_groupby_hash_u32 on each of its two paths (chosen on the host from max_groups alone, so frozen).  Rows are
    unordered: compared sorted by key.  Above the bound: DBHIP_DEV_TABLE_FULL, *out_groups == max_groups, and the
    replay after it is clean again."""
    lib = _lib()
    n, mg, inputs = _gbh_inputs(path)
    ws_bytes = lib.dbhip_groupby_hash_workspace_bytes(n, mg)

    def make():
        keys, vals, ws = _i32(n), _i32(n), _ws(ws_bytes)
        ok, osum, ocnt, og = _i32(mg), _i32(mg), _i32(mg), _i64(1)

        def read():
            g = int(og.item())
            assert 0 <= g <= mg
            order = np.argsort(u32(ok[:g]), kind="stable")
            r = {"groups": np.array([g]), "keys": u32(ok[:g])[order], "sums": u32(osum[:g])[order]}
            if counts:
                r["counts"] = u32(ocnt[:g])[order]
            else:
                r["untouched"] = np.array([np.unique(u32(ocnt)).size])
            return r
        return Buffers([keys, vals], [ok, osum, ocnt, og], [ws], [ws], lambda: _rc(lib.dbhip_groupby_hash_u32(
            keys.data_ptr(), vals.data_ptr(), n, mg, ok.data_ptr(), osum.data_ptr(), ocnt.data_ptr() if counts else None,
            og.data_ptr(), ws.data_ptr(), ws_bytes, _s())), read)

    def check(inp, got):
        if not counts:
            assert int(got["untouched"][0]) == 1, "out_counts == NULL, yet the counts column was written"
        if inp.status == TABLE_FULL:
            assert int(got["groups"][0]) == mg
            assert np.unique(got["keys"]).size == got["keys"].size and np.isin(got["keys"], inp.cols[0]).all()
            return
        wk, wsum, wcnt = gh.expect(inp.cols[0], inp.cols[1])
        assert np.array_equal(got["keys"], wk) and np.array_equal(got["sums"], wsum)
        if counts:
            assert np.array_equal(got["counts"], wcnt)

    seen = run_family(make, inputs, check, _gbh_canon(mg))
    assert [s[0] for s in seen] == [0, 0, 0, 0, TABLE_FULL, 0, 0]


def _gbh_canon(mg):
    def canon(r):
        if int(r["groups"][0]) == mg:  # a full table: which of the keys it kept is not defined
            return {"groups": r["groups"]}
        return r
    return canon


# ---- the one-to-many joins ------------------------------------------------------------------------------------------------
FIRST_BUILD, FIRST_PROBE = 1 << 24, 1 << 28  # caller row ids: first + row


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _join_inputs(n, m, parts, hot_probe=False):
    """the join families' inputs, from the constructions of tests/test_gpu_workspace_reuse.py: 3500 distinct keys of one
    partition (more than its 3072-slot LDS sub-table: the partition spills; below 2^16 build rows there are no
    partitions and the keys are just keys), every other build row one key (a giant partition from 2^18 rows), both at
    once (the hot key on the even rows, the crowd on odd ones), one build row and one probe row carrying 0xFFFFFFFF"""
    rng = np.random.default_rng(n + m)
    crowd = jt.keys_of_partition_of(parts, parts // 3, 3800)[: min(3500, n // 2)]
    spill = _crowded(n, crowd, 1, rng)
    giant = po.gen_uniform_u32(n, 44, 0, n - 1)
    giant[::2] = crowd[0]
    both = giant.copy()
    both[1: 2 * crowd.size: 2] = crowd
    assert np.unique(both[np.isin(both, crowd)]).size == crowd.size
    flagged = po.gen_uniform_u32(n, 46, 0, n - 1)
    flagged[n // 3] = M32
    fprobe = _probe(m, n, [crowd], rng, 47)
    fprobe[5] = M32
    inputs = [Input([po.gen_uniform_u32(n, 42, 0, n - 1), _probe(m, n, [crowd], rng)], name="uniform"),
              Input([spill, _probe(m, n, [crowd], rng)], name="one partition spills"),
              Input([giant, _probe(m, n, [crowd, crowd[:1]], rng)], name="every other build row one key"),
              Input([both, _probe(m, n, [crowd, crowd[:1]], rng)], name="a giant that spills"),
              Input([flagged, fprobe], status=KEY_RANGE, name="a build row carrying 0xFFFFFFFF", dropped=n // 3)]
    if hot_probe:
        hp = _probe(m, n, [crowd], rng)
        hp[rng.permutation(m)[:40000]] = crowd[1]
        inputs.append(Input([_crowded(n, crowd[:1], min(40000, n // 2), rng), hp], name="a hot probe key"))
    inputs.append(Input([po.gen_uniform_u32(n, 48, 0, n - 1), _probe(m, n, [crowd], rng, 49)], name="uniform again"))
    return inputs


def _check_dropped(build, probe, rid, pos, cnt, ids):
    """a build with one row dropped (DBHIP_DEV_KEY_RANGE): every count against the build without its 0xFFFFFFFF rows (a
    probe row carrying 0xFFFFFFFF gets 0 / 0), every hit's range inside the id buffer and on its key at both ends"""
    kept = build[build != M32]
    want = po.join_counts_fast(kept, probe).astype(np.uint32)
    want[probe == M32] = 0
    assert np.array_equal(cnt, want[rid])
    assert not pos[probe[rid] == M32].any()
    hit = cnt > 0
    assert (pos[hit].astype(np.int64) + cnt[hit] <= build.size).all()
    first, last = ids[pos[hit]], ids[pos[hit] + cnt[hit] - 1]
    assert first.max() < build.size and last.max() < build.size
    assert np.array_equal(build[first], probe[rid[hit]]) and np.array_equal(build[last], probe[rid[hit]])


@pytest.mark.parametrize("with_ids", [False, True], ids=["join_build", "join_build_pairs"])
@pytest.mark.parametrize("n", [3000, 1 << 16, (1 << 18) + 5, 1 << 22])
def test_hash_join_replays(n, with_ids):
    """dbhip_join_build_u32 or _build_pairs_u32, dbhip_join_probe_u32, dbhip_join_answers_u32 in one graph.  3000 rows:
    the HBM table; 2^16: the build kernel builds a spilled partition's table at once; from 2^18: spilled partitions are
    listed and partitions above 32768 rows are giants (jl_giant_*); 2^22: two scatter levels."""
    lib = _lib()
    m = n
    ws_bytes = lib.dbhip_join_workspace_bytes(n)
    first = FIRST_BUILD if with_ids else 0
    rows = np.arange(n, dtype=np.uint32) + np.uint32(first)
    inputs = _join_inputs(n, m, jt.build_parts(n))
    if with_ids:
        for inp in inputs:
            inp.cols.append(rows)

    def make():
        build, probe, rid = _i32(n), _i32(m), _i32(n)
        ids, pos, cnt, ws = _i32(n), _i32(m), _i32(m), _ws(ws_bytes)
        ans = torch.empty((m, 2), dtype=torch.int64, device="cuda")

        def run():
            if with_ids:
                _rc(lib.dbhip_join_build_pairs_u32(build.data_ptr(), rid.data_ptr(), n, ids.data_ptr(), ws.data_ptr(),
                                                   ws_bytes, _s()))
            else:
                _rc(lib.dbhip_join_build_u32(build.data_ptr(), n, ids.data_ptr(), ws.data_ptr(), ws_bytes, _s()))
            _rc(lib.dbhip_join_probe_u32(probe.data_ptr(), m, ws.data_ptr(), n, pos.data_ptr(), cnt.data_ptr(), _s()))
            _rc(lib.dbhip_join_answers_u32(ids.data_ptr(), pos.data_ptr(), cnt.data_ptr(), m, ans.data_ptr(), _s()))

        def read():
            a = ans.cpu().numpy()
            p, c, i = u32(pos), u32(cnt), u32(ids)
            row = np.minimum(i[np.minimum(p, n - 1)] - np.uint32(first), np.uint32(n - 1))  # (clamped: check() judges them)
            return {"pos": p, "cnt": c, "ids": i, "ans_size": a[:, 1].copy(), "ans_off": a[:, 0] - ids.data_ptr(),
                    "key_at_pos": np.where(c > 0, u32(build)[row], 0)}
        return Buffers([build, probe] + ([rid] if with_ids else []), [ids, pos, cnt, ans], [ws], [ws], run, read)

    def check(inp, got):
        build, probe = inp.cols[0], inp.cols[1]
        pos, cnt, ids = got["pos"], got["cnt"], got["ids"]
        assert np.array_equal(got["ans_size"], cnt.astype(np.int64)), "answers: sizes"
        assert np.array_equal(got["ans_off"], 4 * pos.astype(np.int64)), "answers: pointers are not ids + pos"
        if "dropped" in inp.facts:
            hit = cnt > 0
            ok = ids.copy()
            sel = np.concatenate([pos[hit], pos[hit] + cnt[hit] - 1])
            assert (ok[sel] >= first).all()
            ok[sel] -= np.uint32(first)
            _check_dropped(build, probe, np.arange(m), pos, cnt, ok)
        else:
            jt.check_grouped_result(build, probe, (_t(pos), _t(cnt), _t(ids)), first=first)

    def canon(r):  # where a key's range lies in the id buffer and the order of the ids inside it are open
        return {k: r[k] for k in ("cnt", "ans_size", "key_at_pos")}
    seen = run_family(make, inputs, check, canon)
    assert [s[0] for s in seen] == [0, 0, 0, 0, KEY_RANGE, 0, 0]


@pytest.mark.parametrize("with_ids", [False, True], ids=["row numbers", "caller row ids"])
@pytest.mark.parametrize("call", ["steps", "one call"])
@pytest.mark.parametrize("nb", [1 << 16, 1 << 18])
def test_radix_join_replays(nb, call, with_ids):
    """partition build, partition probe, then the match captured twice in a row (the header allows the repeat: every
    match takes its spill tables afresh), or dbhip_join_radix_u32, which runs the three steps.  The build side's
    partition call opens a join and clears the status word: after the flagged input the next replay reads 0."""
    lib = _lib()
    m = 2 * nb + 77
    ws_bytes = lib.dbhip_join_radix_workspace_bytes(nb, m)
    fb, fp = (FIRST_BUILD, FIRST_PROBE) if with_ids else (0, 0)
    inputs = _join_inputs(nb, m, jt.radix_parts(nb), hot_probe=True)
    if with_ids:
        for inp in inputs:
            inp.cols += [np.arange(nb, dtype=np.uint32) + np.uint32(fb), np.arange(m, dtype=np.uint32) + np.uint32(fp)]

    def make():
        build, probe, brid, prid = _i32(nb), _i32(m), _i32(nb), _i32(m)
        ids, rid, pos, cnt, ws = _i32(nb), _i32(m), _i32(m), _i32(m), _ws(ws_bytes)
        bp, pp = (brid.data_ptr(), prid.data_ptr()) if with_ids else (None, None)
        outs = (ids.data_ptr(), rid.data_ptr(), pos.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws_bytes)

        def run():
            if call == "one call":
                _rc(lib.dbhip_join_radix_u32(build.data_ptr(), bp, nb, probe.data_ptr(), pp, m, *outs, _s()))
                return
            _rc(lib.dbhip_join_radix_partition_u32(0, build.data_ptr(), bp, nb, nb, m, ws.data_ptr(), ws_bytes, _s()))
            _rc(lib.dbhip_join_radix_partition_u32(1, probe.data_ptr(), pp, m, nb, m, ws.data_ptr(), ws_bytes, _s()))
            for _ in range(2):
                _rc(lib.dbhip_join_radix_match_u32(nb, m, *outs, _s()))
        return Buffers([build, probe] + ([brid, prid] if with_ids else []), [ids, rid, pos, cnt], [ws], [ws], run,
                       lambda: {"rid": u32(rid), "pos": u32(pos), "cnt": u32(cnt), "ids": u32(ids)})

    def check(inp, got):
        build, probe = inp.cols[0], inp.cols[1]
        if "dropped" in inp.facts:
            rid = got["rid"] - np.uint32(fp)
            assert np.array_equal(np.sort(rid), np.arange(m, dtype=np.uint32))
            hit = got["cnt"] > 0
            ok = got["ids"].copy()
            sel = np.concatenate([got["pos"][hit], got["pos"][hit] + got["cnt"][hit] - 1])
            assert (ok[sel] >= fb).all()
            ok[sel] -= np.uint32(fb)
            _check_dropped(build, probe, rid, got["pos"], got["cnt"], ok)
        else:
            jt.check_radix_result(build, probe, tuple(_t(got[k]) for k in ("rid", "pos", "cnt", "ids")), fb, fp)

    def canon(r):  # the partition order of the probe rows and the ids inside a range are open: counts by probe row
        order = np.argsort(r["rid"], kind="stable")
        return {"rid": r["rid"][order], "cnt": r["cnt"][order]}
    seen = run_family(make, inputs, check, canon)
    assert [s[0] for s in seen] == [0, 0, 0, 0, KEY_RANGE, 0, 0, 0]


# ---- unique-key join ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1 << 16, 1 << 18])
def test_unique_join_replays(n):
    """dbhip_ujoin_build_u32 + _probe_u32: 1000 rows take the small open-addressing table, 2^16 and 2^18 the
    LDS-partitioned one.  Unique keys; 9000 keys of one partition (it spills; at 1000 rows: other unique keys); probes
    that all miss; unique keys again.  Every output word is defined: bitwise against the oracle and the eager run."""
    lib = _lib()
    m = n // 2 + 13
    rng = np.random.default_rng(n)
    ws_bytes = lib.dbhip_ujoin_workspace_bytes(n)
    crowd = jt.keys_of_partition(n, 2, 9400)[:9000] if n >= 1 << 16 else np.zeros(0, np.uint32)

    def case(ak, misses, name):
        if misses:
            bk = np.setdiff1d(po.gen_unique_sorted_u32(4 * m, 12), ak)[:m].astype(np.uint32)
        else:
            bk = np.concatenate([ak[rng.integers(0, n, m // 2)], po.gen_unique_sorted_u32(m - m // 2, 12)]).astype(np.uint32)
        assert bk.size == m
        return Input([ak, po.gen_uniform_u32(n, 13, 0, M32 - 1), rng.permutation(bk), po.gen_uniform_u32(m, 14, 0, M32 - 1)],
                     name=name, misses=misses)
    inputs = [case(_unique_crowd(n, crowd[:0], rng), False, "unique keys"),
              case(_unique_crowd(n, crowd, rng), False, "a crowded partition"),
              case(rng.permutation(po.gen_unique_sorted_u32(n, 15)), True, "probes that all miss"),
              case(rng.permutation(po.gen_unique_sorted_u32(n, 16)), False, "unique keys again")]

    def make():
        ak, av, bk, bv = _i32(n), _i32(n), _i32(m), _i32(m)
        ok, o1, o2, ws = _i32(m), _i32(m), _i32(m), _ws(ws_bytes)

        def run():
            _rc(lib.dbhip_ujoin_build_u32(ak.data_ptr(), av.data_ptr(), n, ws.data_ptr(), ws_bytes, _s()))
            _rc(lib.dbhip_ujoin_probe_u32(bk.data_ptr(), bv.data_ptr(), m, ws.data_ptr(), n, ok.data_ptr(), o1.data_ptr(),
                                          o2.data_ptr(), _s()))
        return Buffers([ak, av, bk, bv], [ok, o1, o2], [ws], [ws], run,
                       lambda: {"key": u32(ok), "build_val": u32(o1), "probe_val": u32(o2)})

    def check(inp, got):
        ek, e1, e2 = po.ujoin(*inp.cols)
        assert np.array_equal(got["key"], ek) and np.array_equal(got["build_val"], e1) and np.array_equal(got["probe_val"], e2)
        if inp.facts["misses"]:
            assert (got["key"] == M32).all()
    run_family(make, inputs, check)


# ---- join pairs behind a captured join ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left_outer", [False, True], ids=["inner", "left outer"])
def test_join_pairs_behind_a_captured_join(left_outer):
    """build, probe and dbhip_join_pairs_u32 in ONE graph (the pair table fed by a captured join, not by eager answers),
    capacity frozen at 4 pairs per probe row.  The uniform answer; an answer in which every probe row carries one key;
    an answer of about 16 pairs per probe row (DBHIP_DEV_TABLE_FULL in the pair table's workspace, *out_pairs the full
    total, the first `capacity` pairs written, the join's own status 0); the uniform answer again."""
    lib = _lib()
    n = m = 1 << 16
    cap = 4 * m
    rng = np.random.default_rng(3)
    jws_bytes, pws_bytes = lib.dbhip_join_workspace_bytes(n), lib.dbhip_join_pairs_workspace_bytes(m)
    uni = po.gen_uniform_u32(n, 42, 0, n - 1)
    twice = int(next(k for k in uni if np.count_nonzero(uni == k) == 2))
    hot = po.gen_uniform_u32(n, 44, 0, n - 1)
    hot[rng.permutation(n)[:64]] = 777777
    hprobe = po.gen_uniform_u32(m, 45, 0, n - 1)
    hprobe[::4] = 777777
    inputs = [Input([uni, po.gen_uniform_u32(m, 43, 0, n - 1)], status=(0, 0), name="uniform"),
              Input([uni, np.full(m, twice, np.uint32)], status=(0, 0), name="every probe row one key"),
              Input([hot, hprobe], status=(0, TABLE_FULL), name="more pairs than the capacity"),
              Input([po.gen_uniform_u32(n, 46, 0, n - 1), po.gen_uniform_u32(m, 47, 0, n - 1)], status=(0, 0),
                    name="uniform again")]

    def make():
        build, probe = _i32(n), _i32(m)
        ids, pos, cnt, jws = _i32(n), _i32(m), _i32(m), _ws(jws_bytes)
        ob, op, total, pws = _i32(cap), _i32(cap), _i64(1), _ws(pws_bytes)

        def run():
            _rc(lib.dbhip_join_build_u32(build.data_ptr(), n, ids.data_ptr(), jws.data_ptr(), jws_bytes, _s()))
            _rc(lib.dbhip_join_probe_u32(probe.data_ptr(), m, jws.data_ptr(), n, pos.data_ptr(), cnt.data_ptr(), _s()))
            _rc(lib.dbhip_join_pairs_u32(ids.data_ptr(), n, None, pos.data_ptr(), cnt.data_ptr(), m, int(left_outer), cap,
                                         ob.data_ptr(), op.data_ptr(), total.data_ptr(), pws.data_ptr(), pws_bytes, _s()))
        return Buffers([build, probe], [ids, pos, cnt, ob, op, total], [jws, pws], [jws, pws], run,
                       lambda: {"ids": u32(ids), "pos": u32(pos), "cnt": u32(cnt), "build_rows": u32(ob),
                                "probe_rows": u32(op), "total": np.array([int(total.item())])})

    def check(inp, got):
        build, probe = inp.cols
        ids, pos, cnt = got["ids"], got["pos"], got["cnt"]
        jt.check_grouped_result(build, probe, (_t(pos), _t(cnt), _t(ids)))
        e = np.maximum(cnt, 1).astype(np.int64) if left_outer else cnt.astype(np.int64)
        total = int(e.sum())
        assert int(got["total"][0]) == total
        assert (total > cap) == (inp.status[1] == TABLE_FULL)
        rows = np.repeat(np.arange(m, dtype=np.int64), e)
        k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(e) - e, e)
        at = np.minimum(pos[rows].astype(np.int64) + k, n - 1)
        want_b = np.where(cnt[rows] > 0, ids[at], np.uint32(M32)).astype(np.uint32)
        w = min(total, cap)
        assert np.array_equal(got["build_rows"][:w], want_b[:w]) and np.array_equal(got["probe_rows"][:w], rows[:w].astype(np.uint32))
        for col in ("build_rows", "probe_rows"):  # nothing written past the pairs
            assert np.unique(got[col][w:]).size <= 1

    def canon(r):  # given (ids, pos, cnt) the table is unique; ids and pos are not: the probe rows, counts and total
        w = min(int(r["total"][0]), cap)
        return {"total": r["total"], "probe_rows": r["probe_rows"][:w], "cnt": r["cnt"]}
    seen = run_family(make, inputs, check, canon)
    assert seen == [(0, 0), (0, 0), (0, TABLE_FULL), (0, 0), (0, 0)]


# ---- tables: a table's whole life in one graph ------------------------------------------------------------------------------------
VAL_XOR = 0x3C3C3C3C


@pytest.mark.parametrize("hash_kind", [0, 1])
def test_bitmask_table_life_in_one_graph(hash_kind):
    """reset, insert, lookup.  Every row takes a slot of its own, so with the row count frozen a table cannot overflow
    on one input and fit the next: two graphs share ONE table here, `fit` (3000 rows into 4096 slots) and `over` (4196
    rows: 100 find no slot, DBHIP_DEV_TABLE_FULL), replayed fit, over, fit, over, fit.  The reset node of a graph must
    clear what the other graph's replay left: the status word, the occupancy bits, 4096 foreign keys."""
    lib = _lib()
    size, seed = 4096, 421
    sizes = {"fit": 3000, "over": size + 100}
    ws_bytes = lib.dbhip_bitmask_table_workspace_bytes(size)
    ws = _ws(ws_bytes)
    bufs, graphs = {}, {}
    for name, n in sizes.items():
        keys, vals, q, ov, of = _i32(n), _i32(n), _i32(n), _i32(n), _i32(n)
        bufs[name] = (keys, vals, q, ov, of)

        def life(n=n, b=bufs[name]):
            _rc(lib.dbhip_bitmask_table_reset(ws.data_ptr(), ws_bytes, size, _s()))
            _rc(lib.dbhip_bitmask_table_insert_u32(b[0].data_ptr(), b[1].data_ptr(), n, ws.data_ptr(), ws_bytes, size,
                                                   hash_kind, seed, 0, _s()))
            _rc(lib.dbhip_bitmask_table_lookup_u32(b[2].data_ptr(), n, ws.data_ptr(), size, hash_kind, seed,
                                                   b[3].data_ptr(), b[4].data_ptr(), _s()))
        for t in (keys, vals, q):
            t.zero_()
        graphs[name] = gl.capture(life)
    seen = []
    for i, name in enumerate(["fit", "over", "fit", "over", "fit"]):
        n = sizes[name]
        keys, vals, q, ov, of = bufs[name]
        mine = po.gen_unique_sorted_u32(2 * n, 30 + i)
        present, absent = mine[::2], mine[1::2]
        query = np.concatenate([present[: n // 2], absent[: n - n // 2]])
        gl.fill(keys, present)
        gl.fill(vals, present ^ np.uint32(VAL_XOR))
        gl.fill(q, query)
        ov.fill_(i32(FILLS[i % 2]))
        of.fill_(i32(FILLS[i % 2]))
        gl.poison(ws, gl.POISONS[i % 3])
        graphs[name].replay()
        torch.cuda.synchronize()
        seen.append(gl.status(ws))
        got_v, got_f = u32(ov), u32(of)
        assert set(np.unique(got_f).tolist()) <= {0, 1}, (i, name)
        assert not got_f[n // 2:].any() and not got_v[n // 2:].any(), (i, name, "a key that was never inserted is found")
        hit = got_f[: n // 2] == 1
        assert np.array_equal(got_v[: n // 2][hit], query[: n // 2][hit] ^ np.uint32(VAL_XOR)), (i, name)
        assert not got_v[: n // 2][~hit].any()
        if name == "fit":
            assert hit.all(), (i, "an inserted key is missing")
        else:  # 100 of the 4196 rows found no slot: at most 100 of the queried ones are missing
            assert np.count_nonzero(~hit) <= n - size, (i, np.count_nonzero(~hit))
    assert seen == [0, TABLE_FULL, 0, TABLE_FULL, 0], seen


def _cuckoo_model(size, kind, seeds, keys, vals, max_iter):
    m = CuckooModel(size, kind, seeds, murmur=lambda k, s: int(murmur3_x86_32_np([k], s)[0]))
    res = [m.insert(int(k), int(v), max_iter) for k, v in zip(keys, vals)]
    return m, np.array(res, dtype=np.uint32)


@pytest.mark.parametrize("serial", [1, 0], ids=["serial", "parallel"])
@pytest.mark.parametrize("hash_kind", [1, 2])
def test_cuckoo_table_life_in_one_graph(hash_kind, serial):
    """reset, insert, lookup, export with the seeds frozen at ops.cuckoo_seed_pair(2, 0), 1024 rows, 2275 slots.  Kind 1:
    the key set of test_gpu_cuckoo.py::test_rebuild_at_load_045 that cannot be placed under these seeds (a component of
    its cuckoo graph holds more keys than slots, so it fails in any insertion order).  Kind 2: three copies of one key
    for its two slots (test_bounded_give_up_and_the_empty_key).  Both raise DBHIP_DEV_TABLE_FULL; the inputs around them
    build cleanly (tests/cuckoo_model.py says so for the serial order), and the status reads 0 again.  Serial mode is
    compared with the model slot by slot; in both modes the inserted flags, the lookups and the export agree."""
    from dwarf_bench_amd import ops
    lib = _lib()
    n, size, max_iter = 1024, 2275, 1024  # max_iter = 0 means min(n, 100000) = 1024
    seeds = ops.cuckoo_seed_pair(2, 0)
    ws_bytes = lib.dbhip_cuckoo_table_workspace_bytes(size)
    failing = po.gen_unique_sorted_u32(n, 23)
    if hash_kind == 2:
        failing[1] = failing[2] = failing[0]
    inputs = []
    for keys, name in ((po.gen_unique_sorted_u32(n, 24), "clean"), (failing, "cannot be placed"),
                       (po.gen_unique_sorted_u32(n, 25), "clean"), (po.gen_unique_sorted_u32(n, 26), "clean")):
        vals = po.gen_uniform_u32(n, 5, 1, M32)
        model, res = _cuckoo_model(size, hash_kind, seeds, keys, vals, max_iter)
        assert (res == 1).all() == (name == "clean"), (name, "the model disagrees with the construction")
        inputs.append(Input([keys, vals], status=OK if name == "clean" else TABLE_FULL, name=name, model=model, res=res))

    def make():
        keys, vals, ws = _i32(n), _i32(n), _ws(ws_bytes)
        ins, lv, lf, ek, ev = _i32(n), _i32(n), _i32(n), _i32(size), _i32(size)

        def run():
            _rc(lib.dbhip_cuckoo_table_reset(ws.data_ptr(), ws_bytes, size, _s()))
            _rc(lib.dbhip_cuckoo_table_insert_u32(keys.data_ptr(), vals.data_ptr(), n, ws.data_ptr(), ws_bytes, size,
                                                  hash_kind, seeds[0], seeds[1], 0, serial, ins.data_ptr(), _s()))
            _rc(lib.dbhip_cuckoo_table_lookup_u32(keys.data_ptr(), n, ws.data_ptr(), size, hash_kind, seeds[0], seeds[1],
                                                  lv.data_ptr(), lf.data_ptr(), _s()))
            _rc(lib.dbhip_cuckoo_table_export_u32(ws.data_ptr(), size, ek.data_ptr(), ev.data_ptr(), _s()))
        return Buffers([keys, vals], [ins, lv, lf, ek, ev], [ws], [ws], run,
                       lambda: {"inserted": u32(ins), "vals": u32(lv), "found": u32(lf), "slot_keys": u32(ek),
                                "slot_vals": u32(ev)})

    def check(inp, got):
        keys, vals = inp.cols
        sk, sv = got["slot_keys"], got["slot_vals"]
        occ = sk != M32
        assert set(np.unique(got["inserted"]).tolist()) <= {0, 1}
        assert int(got["inserted"].sum()) == int(occ.sum()), "inserted flags against the occupied slots"
        assert not sv[~occ].any()
        stored = {}
        for k, v in zip(sk[occ].tolist(), sv[occ].tolist()):
            stored.setdefault(k, set()).add(v)
        pairs = set(zip(keys.tolist(), vals.tolist()))
        assert all((k, v) in pairs for k, vs in stored.items() for v in vs), "a slot holds a pair that was never inserted"
        for k, v, f in zip(keys.tolist(), got["vals"].tolist(), got["found"].tolist()):
            assert (f == 1) == (k in stored) and (v in stored[k] if f else v == 0), ("lookup against the export", k)
        if inp.status == OK:
            assert (got["inserted"] == 1).all() and (got["found"] == 1).all()
        else:
            assert int((got["inserted"] == 0).sum()) >= 1
        if serial:
            m = inp.facts["model"]
            assert np.array_equal(got["inserted"], inp.facts["res"])
            assert {i: (int(k), int(v)) for i, (k, v) in enumerate(zip(sk, sv)) if k != M32} == m.layout()
            for k, v, f in zip(keys.tolist(), got["vals"].tolist(), got["found"].tolist()):
                mv, mf = m.at(k)
                assert bool(f) == mf and (v == mv if mf else v == 0)

    def canon(r):  # the parallel insert's placement depends on the order the rows arrive in
        if serial:
            return r
        return {"found": r["found"], "vals": r["vals"]} if (r["inserted"] == 1).all() else {}
    seen = run_family(make, inputs, check, canon)
    assert [s[0] for s in seen] == [0, TABLE_FULL, 0, 0, 0]


SLAB_B, SLAB_POOL, SLAB_N = 7, 40, 1320


def _slab_keys(rng, per_bucket, hasher):
    """SLAB_N distinct keys with per_bucket[b] of them in bucket b (tests/slab_model.slab_hash)"""
    from tests.slab_model import slab_hash
    cand = rng.permutation(np.arange(1, 60000, dtype=np.uint32))
    bucket = np.array([slab_hash(int(k), *hasher, SLAB_B) for k in cand])
    keys = np.concatenate([cand[bucket == b][:c] for b, c in enumerate(per_bucket)])
    assert keys.size == SLAB_N == sum(per_bucket)
    return rng.permutation(keys)


def test_slab_table_life_in_one_graph():
    """reset, insert, lookup, join_probe, export: 7 buckets, a pool of 40 nodes, 1320 rows, the serial insert (one group
    in input order: the layout is tests/slab_model.py's, node by node; a concurrent insert may leave a pool node
    unlinked per row group, so no pool size both holds one input of 1320 rows for certain and is exhausted by another).
    188 or 192 keys per bucket need 6 slabs each, 35 pool nodes of 40: clean.  All 1320 keys in one bucket need 42
    slabs, 41 pool nodes: the pool runs out, the last 8 rows are not stored, DBHIP_DEV_TABLE_FULL.  The balanced input
    after it needs 35 nodes again and gets them only if the pool cursor starts from 0: pool_used reads 35."""
    from dwarf_bench_amd import ops
    lib = _lib()
    hasher = ops.SLAB_HASHER_TESTS
    nodes = SLAB_B + SLAB_POOL
    rng = np.random.default_rng(9)
    ws_bytes = lib.dbhip_slab_table_workspace_bytes(SLAB_B, SLAB_POOL)
    geo = (SLAB_B, SLAB_POOL) + tuple(hasher)
    inputs = []
    for per_bucket, name in (([192] + [188] * 6, "balanced"), ([0, 0, SLAB_N, 0, 0, 0, 0], "one bucket"),
                             ([188] * 6 + [192], "balanced"), ([190] * 6 + [180], "balanced")):
        keys = _slab_keys(rng, per_bucket, hasher)
        vals = po.gen_uniform_u32(SLAB_N, 6, 1, M32)
        probe = np.concatenate([keys[::2], keys[: SLAB_N // 2] + np.uint32(70000)])  # half present, half absent
        model = SlabModel(SLAB_B, SLAB_POOL, hasher)
        res = np.array([model.insert(int(k), int(v)) for k, v in zip(keys, vals)], dtype=np.uint32)
        full = name == "one bucket"
        assert (res == 1).all() != full and model.used == (SLAB_POOL if full else 35), (name, model.used)
        inputs.append(Input([keys, vals, probe, po.gen_uniform_u32(SLAB_N, 7, 0, M32 - 1)],
                            status=TABLE_FULL if full else OK, name=name, model=model, res=res))

    def make():
        keys, vals, pk, pv, ws = _i32(SLAB_N), _i32(SLAB_N), _i32(SLAB_N), _i32(SLAB_N), _ws(ws_bytes)
        ins, lv, lf = _i32(SLAB_N), _i32(SLAB_N), _i32(SLAB_N)
        jk, jb, jp = _i32(SLAB_N), _i32(SLAB_N), _i32(SLAB_N)
        ek, ev, en, used = _i32(nodes * 32), _i32(nodes * 32), _i32(nodes), _i32(1)

        def run():
            _rc(lib.dbhip_slab_table_reset(ws.data_ptr(), ws_bytes, SLAB_B, SLAB_POOL, _s()))
            _rc(lib.dbhip_slab_table_insert_u32(keys.data_ptr(), vals.data_ptr(), SLAB_N, ws.data_ptr(), ws_bytes, *geo, 1,
                                                ins.data_ptr(), _s()))
            _rc(lib.dbhip_slab_table_lookup_u32(keys.data_ptr(), SLAB_N, ws.data_ptr(), *geo, lv.data_ptr(),
                                                lf.data_ptr(), _s()))
            _rc(lib.dbhip_slab_table_join_probe_u32(pk.data_ptr(), pv.data_ptr(), SLAB_N, ws.data_ptr(), *geo,
                                                    jk.data_ptr(), jb.data_ptr(), jp.data_ptr(), _s()))
            _rc(lib.dbhip_slab_table_export_u32(ws.data_ptr(), SLAB_B, SLAB_POOL, ek.data_ptr(), ev.data_ptr(),
                                                en.data_ptr(), used.data_ptr(), _s()))
        return Buffers([keys, vals, pk, pv], [ins, lv, lf, jk, jb, jp, ek, ev, en, used], [ws], [ws], run,
                       lambda: {"inserted": u32(ins), "vals": u32(lv), "found": u32(lf), "join_key": u32(jk),
                                "join_build_val": u32(jb), "join_probe_val": u32(jp), "slab_keys": u32(ek).reshape(nodes, 32),
                                "slab_vals": u32(ev).reshape(nodes, 32), "next": u32(en), "pool_used": u32(used)})

    def check(inp, got):
        m = inp.facts["model"]
        keys, vals, pk, pv = inp.cols
        mk, mv, mn, mused = m.export()
        assert int(got["pool_used"][0]) == mused, ("pool_used", got["pool_used"], mused)
        assert np.array_equal(got["inserted"], inp.facts["res"])
        assert np.array_equal(got["slab_keys"], mk) and np.array_equal(got["slab_vals"], mv) and np.array_equal(got["next"], mn)
        for k, v, f in zip(keys.tolist(), got["vals"].tolist(), got["found"].tolist()):
            want, hit = m.find(k)
            assert bool(f) == hit and v == (want if hit else 0), ("lookup", k)
        for k, p, gk, gb, gp in zip(pk.tolist(), pv.tolist(), got["join_key"].tolist(), got["join_build_val"].tolist(),
                                    got["join_probe_val"].tolist()):
            want, hit = m.find(k)
            assert (gk, gb, gp) == ((k, want, p) if hit else (M32, M32, M32)), ("join_probe", k)
    seen = run_family(make, inputs, check)
    assert [s[0] for s in seen] == [0, TABLE_FULL, 0, 0, 0]


# ---- small calls, the generators ------------------------------------------------------------------------------------------------------
PJ_FIRST = (1 << 20) + 3


@pytest.mark.parametrize("parts", [1, 3, 256])
def test_small_calls_replay(parts):
    """dbhip_pjoin_partition_u32 (parts and first_row_id frozen), dbhip_gather_u32 over the partition's row ids,
    dbhip_reduce_sum_i32 and dbhip_nested_join_u32 in one graph.  Uniform keys, every key in one bucket, sorted keys."""
    lib = _lib()
    n, na, nb = 100003, 300, 97
    pbytes = lib.dbhip_pjoin_partition_workspace_bytes(n, parts)
    rng = np.random.default_rng(parts)
    one_bucket = np.full(n, 12345, np.uint32)
    inputs = []
    for keys, name in ((po.gen_uniform_u32(n, 7, 0, M32), "uniform"), (one_bucket, "one bucket"),
                       (np.sort(po.gen_uniform_u32(n, 8, 0, M32)), "sorted"), (po.gen_uniform_u32(n, 9, 0, 50), "51 keys")):
        inputs.append(Input([keys, po.gen_uniform_u32(n + 7, 5, 0, M32), rng.integers(0, n + 7, n).astype(np.uint32),
                             keys[:na] % np.uint32(50), po.gen_uniform_u32(na, 2, 0, M32),
                             keys[-nb:] % np.uint32(50), po.gen_uniform_u32(nb, 4, 0, M32)], name=name))

    def make():
        keys, table, idx = _i32(n), _i32(n + 7), _i32(n)
        ak, av, bk, bv = _i32(na), _i32(na), _i32(nb), _i32(nb)
        ok, orid, counts, ws = _i32(n), _i32(n), _i64(parts), _ws(pbytes)
        gathered, red = _i32(n), _i32(1)
        cells = [_i32(na * nb) for _ in range(3)]

        def run():
            _rc(lib.dbhip_pjoin_partition_u32(keys.data_ptr(), n, PJ_FIRST, parts, ok.data_ptr(), orid.data_ptr(),
                                              counts.data_ptr(), ws.data_ptr(), pbytes, _s()))
            _rc(lib.dbhip_gather_u32(table.data_ptr(), idx.data_ptr(), n, gathered.data_ptr(), _s()))
            _rc(lib.dbhip_reduce_sum_i32(keys.data_ptr(), n, red.data_ptr(), _s()))
            _rc(lib.dbhip_nested_join_u32(ak.data_ptr(), av.data_ptr(), bk.data_ptr(), bv.data_ptr(), na, nb,
                                          *(c.data_ptr() for c in cells), _s()))
        return Buffers([keys, table, idx, ak, av, bk, bv], [ok, orid, counts, gathered, red] + cells, [ws], [ws], run,
                       lambda: {"keys": u32(ok), "rids": u32(orid), "counts": counts.cpu().numpy(), "gathered": u32(gathered),
                                "sum": red.cpu().numpy(), **{f"cells{i}": u32(c) for i, c in enumerate(cells)}})

    def check(inp, got):
        keys, table, idx, ak, av, bk, bv = inp.cols
        want_counts = np.bincount(dest_of(keys, parts), minlength=parts)
        assert np.array_equal(got["counts"], want_counts)
        gr = got["rids"].astype(np.int64) - PJ_FIRST
        assert np.array_equal(np.sort(gr), np.arange(n)) and np.array_equal(keys[gr], got["keys"])
        assert np.array_equal(dest_of(got["keys"], parts), np.repeat(np.arange(parts), want_counts))
        assert np.array_equal(got["gathered"], table[idx])
        assert int(got["sum"][0]) == po.reduce_sum(keys.view(np.int32))
        for i, want in enumerate(po.nested_join(ak, av, bk, bv)):
            assert np.array_equal(got[f"cells{i}"], want.reshape(-1))

    def canon(r):  # the order of the pairs inside a bucket is open
        order = np.argsort(r["rids"], kind="stable")
        return {**{k: v for k, v in r.items() if k not in ("keys", "rids")}, "rids": r["rids"][order], "keys": r["keys"][order]}
    run_family(make, inputs, check, canon)


def test_generators_in_front_of_a_dwarf():
    """the host dwarfs' real sequence: the columns are generated on the device by the same graph that runs the dwarf on
    them.  dbhip_gen_unique_sorted_u32 makes the build keys, dbhip_gen_uniform_u32 the payloads, dbhip_gen_uniform_at_u32
    the probe keys at caller-given indices (the one column that changes from replay to replay), the unique-key join
    reads all of them; the generated columns are guard-filled before every replay."""
    lib = _lib()
    n, m, seed = 1 << 16, (1 << 15) + 13, 42
    ws_bytes = lib.dbhip_ujoin_workspace_bytes(n)
    rng = np.random.default_rng(1)
    inputs = [Input([rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)], name="random indices"),
              Input([np.arange(m, dtype=np.uint32)], name="ascending indices"),
              Input([np.full(m, 77, np.uint32)], name="one index")]
    ak = po.gen_unique_sorted_u32(n, seed, 1000)
    av, bv = po.gen_uniform_u32(n, seed + 1, 0, M32 - 1, 5), po.gen_uniform_u32(m, seed + 2, 0, M32 - 1, 1 << 33)

    def make():
        idx, gak, gav, gbk, gbv, ws = _i32(m), _i32(n), _i32(n), _i32(m), _i32(m), _ws(ws_bytes)
        ok, o1, o2 = _i32(m), _i32(m), _i32(m)

        def run():
            _rc(lib.dbhip_gen_unique_sorted_u32(gak.data_ptr(), n, seed, 1000, _s()))
            _rc(lib.dbhip_gen_uniform_u32(gav.data_ptr(), n, seed + 1, 5, 0, M32 - 1, _s()))
            _rc(lib.dbhip_gen_uniform_u32(gbv.data_ptr(), m, seed + 2, 1 << 33, 0, M32 - 1, _s()))
            _rc(lib.dbhip_gen_uniform_at_u32(gbk.data_ptr(), idx.data_ptr(), m, seed + 3, 10000, 10 * n + 19999, _s()))
            _rc(lib.dbhip_ujoin_build_u32(gak.data_ptr(), gav.data_ptr(), n, ws.data_ptr(), ws_bytes, _s()))
            _rc(lib.dbhip_ujoin_probe_u32(gbk.data_ptr(), gbv.data_ptr(), m, ws.data_ptr(), n, ok.data_ptr(), o1.data_ptr(),
                                          o2.data_ptr(), _s()))
        return Buffers([idx], [gak, gav, gbk, gbv, ok, o1, o2], [ws], [ws], run,
                       lambda: {"ak": u32(gak), "av": u32(gav), "bk": u32(gbk), "bv": u32(gbv), "key": u32(ok),
                                "build_val": u32(o1), "probe_val": u32(o2)})

    def check(inp, got):
        span = np.uint64(10 * n + 19999 - 10000 + 1)
        bk = (np.uint64(10000) + mix64_np(seed + 3, inp.cols[0]) % span).astype(np.uint32)
        for name, want in (("ak", ak), ("av", av), ("bk", bk), ("bv", bv)):
            assert np.array_equal(got[name], want), ("generated column", name)
        ek, e1, e2 = po.ujoin(ak, av, bk, bv)
        assert np.array_equal(got["key"], ek) and np.array_equal(got["build_val"], e1) and np.array_equal(got["probe_val"], e2)
    run_family(make, inputs, check)


# ---- validators: accept, reject, accept ---------------------------------------------------------------------------------------------
# Each validator sits in a graph of its own behind the graph of the call it judges; the test damages the result between
# the two on the second of three rounds.  include/dbhip.h: the result words are "zeroed by the call itself" — they hold
# a guard word before every replay and must read accept, reject, accept, with the exact counts of
# tests/test_gpu_buffer_bounds.py's host restatements.  Validators that take a workspace get it poisoned.
VN = 100003


class _Judge:
    """produce(): the call that is judged; validate(): the validator; result: its device words; wss: the validator's
    workspaces; damage(): spoils the result on the device; accept / reject: the words expected (a list, or a predicate
    over the list of words)"""

    def __init__(self, produce, validate, result, wss, damage, accept, reject, refill):
        self.produce, self.validate, self.result, self.wss = produce, validate, result, wss
        self.damage, self.accept, self.reject, self.refill = damage, accept, reject, refill


def _swap(t, i, j):
    a, b = t[i].clone(), t[j].clone()
    t[i], t[j] = b, a


def _judge_fingerprint():
    lib = _lib()
    filt = 37
    src_h = po.gen_uniform_u32(VN, 42, 1, 10000).view(np.int32)
    want = po.copy_if_lt(src_h, filt)
    m = want.size
    assert m > 100 and want[0] != want[1]
    src, out, size, ws = _i32(VN), _i32(VN), _i64(1), _ws(lib.dbhip_copy_if_lt_i32_workspace_bytes(VN))
    fbytes = lib.dbhip_check_fingerprint_workspace_bytes(m)
    res, fws = _i64(2), _ws(fbytes)
    damaged = want.copy()
    damaged[[0, 1]] = damaged[[1, 0]]
    return _Judge(lambda: _rc(lib.dbhip_copy_if_lt_i32(src.data_ptr(), VN, filt, out.data_ptr(), size.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _s())),
                  lambda: _rc(lib.dbhip_check_fingerprint_lt_i32(out.data_ptr(), m, filt, res.data_ptr(), fws.data_ptr(),
                                                                 fbytes, _s())),
                  res, [fws], lambda: _swap(out, 0, 1), _host_fingerprint(want), _host_fingerprint(damaged),
                  lambda: gl.fill(src, src_h))


def _judge_sorted(signed):
    lib = _lib()
    keys_h = po.gen_uniform_u32(VN, 7, 0, M32)
    keys, tmp, ws = _i32(VN), _i32(VN), _ws(lib.dbhip_radix_sort_workspace_bytes(VN, 8))
    res = _i64(3)
    fn = lib.dbhip_radix_sort_i32 if signed else lib.dbhip_radix_sort_u32
    srt = np.sort(keys_h.view(np.int32)).view(np.uint32) if signed else np.sort(keys_h)
    bad = srt.copy()
    bad[[10, 5000]] = bad[[5000, 10]]
    x = bad ^ np.uint32(0x80000000 if signed else 0)
    fps = [_sum64(mix64_np(0x5bd1e995, keys_h)), _sum64(keys_h)]
    return _Judge(lambda: _rc(fn(keys.data_ptr(), tmp.data_ptr(), VN, 8, ws.data_ptr(), ws.numel(), _s())),
                  lambda: _rc(lib.dbhip_check_sorted_u32(keys.data_ptr(), VN, int(signed), res.data_ptr(), _s())),
                  res, [], lambda: _swap(keys, 10, 5000), [0] + fps, [int(np.count_nonzero(x[:-1] > x[1:]))] + fps,
                  lambda: gl.fill(keys, keys_h))


def _judge_sorted_pairs():
    lib = _lib()
    keys_h = po.gen_uniform_u32(VN, 7, 0, 5000)  # many ties: the ids decide
    kin, keys, ids, tk, tv = _i32(VN), _i32(VN), _i32(VN), _i32(VN), _i32(VN)
    ws = _ws(lib.dbhip_radix_sort_pairs_workspace_bytes(VN, 8))
    res = _i64(2)
    perm = np.argsort(keys_h, kind="stable").astype(np.uint32)
    bad = perm.copy()
    bad[[3, 4]] = bad[[4, 3]]
    x, ko = keys_h[perm].astype(np.int64), keys_h[perm]
    desc = int(np.count_nonzero((x[:-1] > x[1:]) | ((x[:-1] == x[1:]) & (bad[:-1] >= bad[1:]))))
    mism = int(np.count_nonzero(keys_h[bad] != ko))
    assert desc >= 1

    def refill():
        gl.fill(kin, keys_h)
        gl.fill(keys, keys_h)
    return _Judge(lambda: _rc(lib.dbhip_radix_sort_pairs_u32(keys.data_ptr(), ids.data_ptr(), tk.data_ptr(), tv.data_ptr(), VN, 8,
                                                             1, ws.data_ptr(), ws.numel(), _s())),
                  lambda: _rc(lib.dbhip_check_sorted_pairs_u32(kin.data_ptr(), keys.data_ptr(), ids.data_ptr(), VN, 0,
                                                               res.data_ptr(), _s())),
                  res, [], lambda: _swap(ids, 3, 4), [0, 0], [desc, mism], refill)


def _judge_weighted_sum():
    lib = _lib()
    groups = 1000
    kh, vh = po.gen_uniform_u32(VN, 1, 0, groups - 1), po.gen_uniform_u32(VN, 2, 0, M32)
    keys, vals, out = _i32(VN), _i32(VN), _i32(groups)
    ws = _ws(lib.dbhip_groupby_sum_u32_workspace_bytes(VN, groups))
    res = _i64(4)
    sums = _gb_want(kh, vh, groups)
    bad = sums.copy()
    bad[7] += np.uint32(1)
    idx = np.arange(groups, dtype=np.uint32)

    def validate():  # the output's sums against the input's: both pairs of words in one graph
        _rc(lib.dbhip_check_weighted_sum_u32(None, out.data_ptr(), groups, res.data_ptr(), _s()))
        _rc(lib.dbhip_check_weighted_sum_u32(keys.data_ptr(), vals.data_ptr(), VN, res[2:].data_ptr(), _s()))

    def refill():
        gl.fill(keys, kh)
        gl.fill(vals, vh)

    def spoil():
        out[7] += 1
    assert _weighted(idx, sums) == _weighted(kh, vh) != _weighted(idx, bad)
    return _Judge(lambda: _rc(lib.dbhip_groupby_sum_u32(keys.data_ptr(), vals.data_ptr(), VN, groups, out.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), _s())),
                  validate, res, [], spoil, _weighted(idx, sums) + _weighted(kh, vh), _weighted(idx, bad) + _weighted(kh, vh),
                  refill)


def _join_parts(n, m, sort_build=False):
    """a captured hash join of uniform keys (and, for check_join, the sorted build column it wants)"""
    lib = _lib()
    bh, ph = po.gen_uniform_u32(n, 42, 1, n // 2), po.gen_uniform_u32(m, 43, 1, n // 2)
    build, probe, ids, pos, cnt = _i32(n), _i32(m), _i32(n), _i32(m), _i32(m)
    ws = _ws(lib.dbhip_join_workspace_bytes(n))
    srt, tmp, sws = _i32(n), _i32(n), _ws(lib.dbhip_radix_sort_workspace_bytes(n, 8))

    def produce():
        _rc(lib.dbhip_join_build_u32(build.data_ptr(), n, ids.data_ptr(), ws.data_ptr(), ws.numel(), _s()))
        _rc(lib.dbhip_join_probe_u32(probe.data_ptr(), m, ws.data_ptr(), n, pos.data_ptr(), cnt.data_ptr(), _s()))
        if sort_build:
            _rc(lib.dbhip_radix_sort_u32(srt.data_ptr(), tmp.data_ptr(), n, 8, sws.data_ptr(), sws.numel(), _s()))

    def refill():
        gl.fill(build, bh)
        gl.fill(probe, ph)
        gl.fill(srt, bh)
    return bh, ph, build, probe, ids, pos, cnt, srt, produce, refill


def _judge_permutation():
    lib = _lib()
    bh, ph, build, probe, ids, pos, cnt, srt, produce, refill = _join_parts(VN, VN)
    pbytes = lib.dbhip_check_permutation_workspace_bytes(VN)
    res, pws = _i64(1), _ws(pbytes)

    def spoil():  # one id seen before, one out of range
        ids[0] = ids[1]
        ids[VN - 1] = VN
    return _Judge(produce, lambda: _rc(lib.dbhip_check_permutation_u32(ids.data_ptr(), VN, res.data_ptr(), pws.data_ptr(), pbytes,
                                                                       _s())), res, [pws], spoil, [0], [2], refill)


def _judge_join():
    lib = _lib()
    bh, ph, build, probe, ids, pos, cnt, srt, produce, refill = _join_parts(VN, VN, sort_build=True)
    res = _i64(2)
    total = int(po.join_counts_fast(bh, ph).sum())

    def spoil():
        cnt[5] += 1
    return _Judge(produce, lambda: _rc(lib.dbhip_check_join_u32(srt.data_ptr(), VN, probe.data_ptr(), VN, pos.data_ptr(),
                                                                cnt.data_ptr(), ids.data_ptr(), build.data_ptr(), 0, 0, 0,
                                                                res.data_ptr(), _s())),
                  res, [], spoil, [0, total], [1, total + 1], refill)


def _judge_join_pairs():
    lib = _lib()
    bh, ph, build, probe, ids, pos, cnt, srt, produce_join, refill = _join_parts(VN, VN)
    total = int(po.join_counts_fast(bh, ph).sum())
    ob, op, tot, pws = _i32(total), _i32(total), _i64(1), _ws(lib.dbhip_join_pairs_workspace_bytes(VN))
    res = _i64(4)

    def produce():
        produce_join()
        _rc(lib.dbhip_join_pairs_u32(ids.data_ptr(), VN, None, pos.data_ptr(), cnt.data_ptr(), VN, 0, total, ob.data_ptr(),
                                     op.data_ptr(), tot.data_ptr(), pws.data_ptr(), pws.numel(), _s()))

    def spoil():  # the first pair's build row becomes a row that carries another key
        key = int(ph[int(u32(op[:1])[0])])
        ob[0] = int(np.flatnonzero(bh != key)[0])
    return _Judge(produce, lambda: _rc(lib.dbhip_check_join_pairs_u32(
        build.data_ptr(), VN, probe.data_ptr(), VN, ids.data_ptr(), None, pos.data_ptr(), cnt.data_ptr(), 0, ob.data_ptr(),
        op.data_ptr(), total, res.data_ptr(), _s())), res, [],
        spoil, lambda w: w[0] == 0 and w[1] == total and w[2] == w[3], lambda w: w[0] == 1 and w[1] == total and w[2] != w[3],
        refill)


def _judge_ujoin():
    lib = _lib()
    n = VN
    ak, av = po.gen_unique_sorted_u32(n, 11), po.gen_uniform_u32(n, 12, 0, M32 - 1)
    bk, bv = po.gen_unique_sorted_u32(n, 13), po.gen_uniform_u32(n, 14, 0, M32 - 1)
    hits = np.isin(bk, ak)
    first_hit = int(np.flatnonzero(hits)[0])
    cols = [_i32(n) for _ in range(4)]
    ok, o1, o2, ws = _i32(n), _i32(n), _i32(n), _ws(lib.dbhip_ujoin_workspace_bytes(n))
    res = _i64(2)

    def produce():
        _rc(lib.dbhip_ujoin_build_u32(cols[0].data_ptr(), cols[1].data_ptr(), n, ws.data_ptr(), ws.numel(), _s()))
        _rc(lib.dbhip_ujoin_probe_u32(cols[2].data_ptr(), cols[3].data_ptr(), n, ws.data_ptr(), n, ok.data_ptr(), o1.data_ptr(),
                                      o2.data_ptr(), _s()))

    def spoil():
        o1[first_hit] ^= 1

    def refill():
        for t, h in zip(cols, (ak, av, bk, bv)):
            gl.fill(t, h)
    return _Judge(produce, lambda: _rc(lib.dbhip_check_ujoin_u32(cols[0].data_ptr(), cols[1].data_ptr(), n, cols[2].data_ptr(),
                                                                 cols[3].data_ptr(), n, ok.data_ptr(), o1.data_ptr(),
                                                                 o2.data_ptr(), res.data_ptr(), _s())),
                  res, [], spoil, [0, int(hits.sum())], [1, int(hits.sum())], refill)


def _judge_distinct():
    lib = _lib()
    kh, vh = po.gen_uniform_u32(VN, 1, 0, 70000), po.gen_uniform_u32(VN, 2, 0, M32)
    g = int(np.unique(kh).size)
    keys, vals = _i32(VN), _i32(VN)
    ok, osum, og = _i32(VN), _i32(VN), _i64(1)
    ws = _ws(lib.dbhip_groupby_hash_workspace_bytes(VN, 0))
    dbytes = lib.dbhip_check_distinct_workspace_bytes(g)
    res, dws = _i64(1), _ws(dbytes)

    def spoil():
        ok[0] = ok[1]

    def refill():
        gl.fill(keys, kh)
        gl.fill(vals, vh)
    return _Judge(lambda: _rc(lib.dbhip_groupby_hash_u32(keys.data_ptr(), vals.data_ptr(), VN, 0, ok.data_ptr(), osum.data_ptr(),
                                                         None, og.data_ptr(), ws.data_ptr(), ws.numel(), _s())),
                  lambda: _rc(lib.dbhip_check_distinct_u32(ok.data_ptr(), g, res.data_ptr(), dws.data_ptr(), dbytes, _s())),
                  res, [dws], spoil, [0], [1], refill)


def _judge_gen_uniform():
    lib = _lib()
    first = 1 << 33
    col, res = _i32(VN), _i64(1)

    def spoil():
        col[9] ^= 1
    return _Judge(lambda: _rc(lib.dbhip_gen_uniform_u32(col.data_ptr(), VN, 42, first, 3, 10000, _s())),
                  lambda: _rc(lib.dbhip_check_gen_uniform_u32(col.data_ptr(), None, VN, 42, first, 3, 10000, res.data_ptr(), _s())),
                  res, [], spoil, [0], [1], lambda: None)


def _judge_pjoin_route():
    lib = _lib()
    parts, rank = 8, 3
    kh = po.gen_uniform_u32(VN, 7, 0, M32)
    dest = dest_of(kh, parts)
    counts = np.bincount(dest, minlength=parts)
    at, mine = int(counts[:rank].sum()), int(counts[rank])
    foreign = int(kh[np.flatnonzero(dest != rank)[0]])
    keys, ok, orid, oc = _i32(VN), _i32(VN), _i32(VN), _i64(parts)
    pbytes = lib.dbhip_pjoin_partition_workspace_bytes(VN, parts)
    ws, res = _ws(pbytes), _i64(1)

    def spoil():
        ok[at + 5] = foreign - (1 << 32) if foreign >> 31 else foreign
    return _Judge(lambda: _rc(lib.dbhip_pjoin_partition_u32(keys.data_ptr(), VN, 0, parts, ok.data_ptr(), orid.data_ptr(),
                                                            oc.data_ptr(), ws.data_ptr(), pbytes, _s())),
                  lambda: _rc(lib.dbhip_check_pjoin_route_u32(ok[at:].data_ptr(), mine, parts, rank, res.data_ptr(), _s())),
                  res, [], spoil, [0], [1], lambda: gl.fill(keys, kh))


JUDGES = {"fingerprint_lt_i32": _judge_fingerprint, "sorted_u32": lambda: _judge_sorted(False),
          "sorted_u32, signed": lambda: _judge_sorted(True), "sorted_pairs_u32": _judge_sorted_pairs,
          "weighted_sum_u32": _judge_weighted_sum, "permutation_u32": _judge_permutation, "join_u32": _judge_join,
          "join_pairs_u32": _judge_join_pairs, "ujoin_u32": _judge_ujoin, "distinct_u32": _judge_distinct,
          "gen_uniform_u32": _judge_gen_uniform, "pjoin_route_u32": _judge_pjoin_route}


@pytest.mark.parametrize("which", list(JUDGES))
def test_validators_accept_reject_accept(which):
    j = JUDGES[which]()
    j.refill()
    produce = gl.capture(j.produce)
    j.refill()
    produce.replay()  # the validator is captured, and warmed up, on a finished result
    torch.cuda.synchronize()
    validate = gl.capture(j.validate)
    for round_, (spoiled, want) in enumerate(((False, j.accept), (True, j.reject), (False, j.accept))):
        j.refill()
        produce.replay()
        torch.cuda.synchronize()
        if spoiled:
            j.damage()
        j.result.fill_(i64(FILLS[round_ % 2]))
        for ws in j.wss:
            gl.poison(ws, gl.POISONS[(round_ + 1) % 3])
        torch.cuda.synchronize()
        validate.replay()
        torch.cuda.synchronize()
        words = [int(x) & ((1 << 64) - 1) for x in j.result.cpu().tolist()]
        ok = want(words) if callable(want) else words == want
        assert ok, (which, round_, "damaged" if spoiled else "correct", words, None if callable(want) else want)
