"""The join result as a table of (build row, probe row) pairs (dbhip_join_pairs_u32, ops.JoinPairs, ops.join_pairs) on the
GPU.  The expected pairs always come from the key columns alone, computed on the host: up to 4096 build rows with the
oracle's seq_join (row indices as payloads), above with a numpy stable-argsort / searchsorted / repeat expansion.  The
comparison is the SORTED list of `probe row << 32 | build row`, every pair: nothing sampled, nothing skipped."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests import guard_testlib as gt
from tests import join_testlib as jt

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_join_pairs"
SENTINEL = 0xFFFFFFFF
KEY_RANGE, TABLE_FULL = 2, 4


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _packed(build_rows, probe_rows):
    return np.sort(probe_rows.astype(np.uint64) << np.uint64(32) | build_rows.astype(np.uint64))


def _numpy_join(build, probe):
    """(build rows, probe rows) of every matching pair, from the key columns alone"""
    order = np.argsort(build, kind="stable")
    sb = build[order]
    lo, hi = np.searchsorted(sb, probe, "left"), np.searchsorted(sb, probe, "right")
    cnt = (hi - lo).astype(np.int64)
    p = np.repeat(np.arange(probe.size, dtype=np.int64), cnt)
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    b = order[np.repeat(lo.astype(np.int64), cnt) + within]
    return b.astype(np.uint32), p.astype(np.uint32)


def _expected(build, probe, left_outer=False):
    """sorted probe row << 32 | build row of the join of the two key columns (left outer: a sentinel pair per probe row
    without a match)"""
    build, probe = np.asarray(build, dtype=np.uint32), np.asarray(probe, dtype=np.uint32)
    if 0 < build.size <= 4096 and probe.size:
        keys, b, p = po.seq_join(build, np.arange(build.size, dtype=np.uint32), probe, np.arange(probe.size, dtype=np.uint32))
        assert np.array_equal(build[b], keys) and np.array_equal(probe[p], keys)
    else:
        b, p = _numpy_join(build, probe)
    if left_outer:
        miss = np.setdiff1d(np.arange(probe.size, dtype=np.uint32), p)
        b = np.concatenate([b, np.full(miss.size, SENTINEL, dtype=np.uint32)])
        p = np.concatenate([p, miss])
    return _packed(b, p)


def _answer(route, build, probe):
    """-> (ids, pos, cnt, rid or None) of the join of the two host columns through HashJoin or RadixJoin"""
    from dwarf_bench_amd import ops
    if route == "hash":
        pos, cnt, ids = ops.hash_join(jt.dev(build), jt.dev(probe))
        return ids, pos, cnt, None
    rid, pos, cnt, ids = ops.radix_join(jt.dev(build), jt.dev(probe))
    return ids, pos, cnt, rid


def _expand(ids, pos, cnt, rid, left_outer, plan=None):
    """count-only call, exact allocation, fill -> (build rows, probe rows) as uint32 host arrays"""
    from dwarf_bench_amd import ops
    counter = ops.JoinPairs(pos.numel(), 0)
    counter.launch(ids, pos, cnt, rid, left_outer)
    total = counter.count()
    assert ops.workspace_status(counter.ws) == 0
    plan = plan or ops.JoinPairs(pos.numel(), total)
    plan.launch(ids, pos, cnt, rid, left_outer)
    b, p = plan.result()
    assert plan.count() == total and b.numel() == total and p.numel() == total
    return _u32(b), _u32(p)


def _join_and_compare(route, build, probe, left_outer, pairs=None):
    ids, pos, cnt, rid = _answer(route, build, probe)
    b, p = _expand(ids, pos, cnt, rid, left_outer)
    want = _expected(build, probe, left_outer)
    if pairs is not None and not left_outer:
        assert want.size == pairs, (want.size, pairs)
    print(f"{route} outer={left_outer} rows={build.size}x{probe.size} pairs={b.size}")
    assert b.size == want.size
    assert np.array_equal(_packed(b, p), want)
    if route == "hash" and b.size <= 1 << 24:  # probe-row order, inside a row the id buffer's order: the output is unique
        hpos, hcnt, hids = _u32(pos).astype(np.int64), _u32(cnt).astype(np.int64), _u32(ids)
        assert np.all(p[1:] >= p[:-1])
        e = np.maximum(hcnt, 1) if left_outer else hcnt
        rows = np.repeat(np.arange(probe.size, dtype=np.int64), e)
        k = np.arange(int(e.sum()), dtype=np.int64) - np.repeat(np.cumsum(e) - e, e)
        assert np.array_equal(p, rows.astype(np.uint32))
        hit = hcnt[rows] > 0
        assert np.array_equal(b[hit], hids[hpos[rows[hit]] + k[hit]]) and np.all(b[~hit] == SENTINEL)
    return b, p


SMALL = [  # build rows, key range, pairs of the inner join with seeds 1 (build) and 2 (probe)
    (128, 10000, 5), (256, 10000, None), (512, 10000, None), (1024, 10000, 114), (2048, 10000, None), (4096, 10000, 1737),
    (4096, 64, 263971)]


@pytest.mark.parametrize("left_outer", [False, True])
@pytest.mark.parametrize("route", ["hash", "radix"])
@pytest.mark.parametrize("n,key_hi,pairs", SMALL)
def test_reference_sizes(n, key_hi, pairs, route, left_outer):
    """the reference's test sizes with 37 more probe rows; keys as the reference draws them and a 64-key column"""
    build, probe = po.gen_uniform_u32(n, 1, 1, key_hi), po.gen_uniform_u32(n + 37, 2, 1, key_hi)
    _join_and_compare(route, build, probe, left_outer, pairs)


@pytest.mark.parametrize("left_outer", [False, True])
@pytest.mark.parametrize("route", ["hash", "radix"])
def test_all_rows_carry_one_key(route, left_outer):
    build, probe = np.full(1000, 77, dtype=np.uint32), np.full(1037, 77, dtype=np.uint32)
    _join_and_compare(route, build, probe, left_outer, 1037000)


@pytest.mark.parametrize("left_outer", [False, True])
@pytest.mark.parametrize("route", ["hash", "radix"])
def test_a_million_rows_a_side(route, left_outer):
    n = 1 << 20
    build, probe = po.gen_uniform_u32(n, 1, 1, n), po.gen_uniform_u32(n, 2, 1, n)
    _join_and_compare(route, build, probe, left_outer, 1047812)


@pytest.mark.parametrize("route", ["hash", "radix"])
def test_sides_that_share_no_key(route):
    n = 1 << 20
    build, probe = po.gen_uniform_u32(n, 1, 1, n), po.gen_uniform_u32(n, 2, n + 1, 2 * n)
    b, p = _join_and_compare(route, build, probe, False, 0)
    assert b.size == 0
    b, p = _join_and_compare(route, build, probe, True)
    assert b.size == n and np.all(b == SENTINEL) and np.array_equal(np.sort(p), np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("left_outer", [False, True])
def test_empty_sides(left_outer):
    from dwarf_bench_amd import ops
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    # no probe rows
    plan = ops.JoinPairs(0, 16)
    plan.total.fill_(-1)
    plan.launch(torch.arange(8, dtype=torch.int32, device="cuda"), empty, empty, None, left_outer)
    assert plan.count() == 0 and ops.workspace_status(plan.ws) == 0 and plan.result()[0].numel() == 0
    # no build rows: nothing matches
    n = 5000
    zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
    b, p = _expand(empty, zeros, zeros, None, left_outer)
    if left_outer:
        assert np.all(b == SENTINEL) and np.array_equal(p, np.arange(n, dtype=np.uint32))
    else:
        assert b.size == 0 and p.size == 0


@pytest.mark.parametrize("route", ["hash", "radix"])
def test_one_key_8192_by_8192(route):
    """2^26 pairs from 2^13 probe rows: every row's range is spread over 32 chunks of the expansion"""
    n = 1 << 13
    build, probe = np.full(n, 12345, dtype=np.uint32), np.full(n, 12345, dtype=np.uint32)
    _join_and_compare(route, build, probe, False, 1 << 26)


@pytest.mark.parametrize("left_outer", [False, True])
@pytest.mark.parametrize("route", ["hash", "radix"])
def test_every_other_build_row_carries_one_key(route, left_outer):
    n = 1 << 20
    probe = po.gen_uniform_u32(n, 2, 1, n)
    hot = probe[n // 3]  # the probe side's range holds the hot key
    build = po.gen_uniform_u32(n, 1, 1, n)
    build[1::2] = hot
    b, p = _join_and_compare(route, build, probe, left_outer)
    assert b.size >= n // 2


def _raw(ids, n_build, rid, pos, cnt, n_probe, left_outer, capacity, out_b, out_p, total, ws):
    from dwarf_bench_amd import _capi
    a = lambda t: gt.ptr(t) if t is not None else None  # noqa: E731
    rc = _capi.lib().dbhip_join_pairs_u32(a(ids), n_build, a(rid), a(pos), a(cnt), n_probe, int(left_outer), capacity,
                                          a(out_b), a(out_p), a(total), a(ws), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def _status(ws):
    from dwarf_bench_amd import ops
    return ops.workspace_status(ws)


@pytest.mark.parametrize("fill", gt.FILLS)
def test_totals_beyond_32_bits_and_a_capacity_below_them(fill):
    """2^17 probe rows with 2^17 ids each: 2^34 pairs.  Count-only: the total, a clean status.  capacity 2^20: TABLE_FULL,
    the total still 2^34, exactly the first 2^20 pairs written and not one word beside them."""
    from dwarf_bench_amd import _capi
    n = 1 << 17
    cap = 1 << 20
    w = gt.Watch(fill)
    ids = w.col(n, data=np.arange(n, dtype=np.uint32), freeze=True)
    pos = w.col(n, data=np.zeros(n, dtype=np.uint32), freeze=True)
    cnt = w.col(n, data=np.full(n, n, dtype=np.uint32), freeze=True)
    ws = w.ws(_capi.lib().dbhip_join_pairs_workspace_bytes(n))
    total = w.u64(1)
    _raw(ids, n, None, pos, cnt, n, False, 0, None, None, total, ws)
    assert _status(ws) == 0 and int(total.item()) == 1 << 34
    w.check()
    out_b, out_p = w.col(cap), w.col(cap)
    total.fill_(gt.i64(fill))
    _raw(ids, n, None, pos, cnt, n, False, cap, out_b, out_p, total, ws)
    assert _status(ws) == TABLE_FULL and int(total.item()) == 1 << 34
    assert np.array_equal(_u32(out_b), np.tile(np.arange(n, dtype=np.uint32), 8))
    assert np.array_equal(_u32(out_p), np.repeat(np.arange(8, dtype=np.uint32), n))
    w.check()


def test_the_plan_names_the_total_when_the_capacity_is_short():
    from dwarf_bench_amd import _capi, ops
    n = 4096
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    pos = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), 3, dtype=torch.int32, device="cuda")
    plan = ops.JoinPairs(n, 100)
    plan.launch(ids, pos, cnt)
    assert plan.count() == 3 * n
    with pytest.raises(_capi.DbhipError, match=str(3 * n)):
        plan.result()


@pytest.mark.parametrize("left_outer", [False, True])
def test_a_forged_answer_reads_nothing_outside_the_id_buffer(left_outer):
    """three rows whose range leaves ids[0..n_build): KEY_RANGE, those rows count as empty, the others are right"""
    from dwarf_bench_amd import ops
    build, probe = po.gen_uniform_u32(3000, 1, 1, 500), po.gen_uniform_u32(5000, 2, 1, 600)
    ids, pos, cnt, _ = _answer("hash", build, probe)
    hpos, hcnt = _u32(pos).copy(), _u32(cnt).copy()
    forged = (7, 2500, 4999)
    hpos[7], hcnt[7] = 2999, 2          # one id too many
    hpos[2500], hcnt[2500] = 3000, 1    # starts at the end
    hpos[4999], hcnt[4999] = 0xFFFFFFF0, 0xFFFFFFF0  # the 32-bit sum wraps
    fpos, fcnt = jt.dev(hpos), jt.dev(hcnt)
    counter = ops.JoinPairs(5000, 0)
    counter.launch(ids, fpos, fcnt, None, left_outer)
    total = counter.count()
    assert ops.workspace_status(counter.ws) == KEY_RANGE
    plan = ops.JoinPairs(5000, total)
    plan.launch(ids, fpos, fcnt, None, left_outer)
    assert ops.workspace_status(plan.ws) == KEY_RANGE and plan.count() == total
    b, p = _u32(plan.build_rows), _u32(plan.probe_rows)
    ok = np.ones(5000, dtype=bool)
    ok[list(forged)] = False
    want = _expected(build, probe, left_outer)
    keep = ok[(want >> np.uint64(32)).astype(np.int64)]
    want = want[keep]
    if left_outer:
        want = np.sort(np.concatenate([want, np.array([r << 32 | SENTINEL for r in forged], dtype=np.uint64)]))
    assert np.array_equal(_packed(b, p), want)


@pytest.mark.parametrize("fill", gt.FILLS)
@pytest.mark.parametrize("offsets", [(1, 1), (2, 2), (3, 3), (0, 0), (1, 3), (0, 2)])
def test_columns_that_start_off_a_16_byte_boundary(offsets, fill):
    """inputs and outputs 1, 2 and 3 words past a 16-byte boundary (and the two output columns at different distances),
    guard words around every buffer"""
    from dwarf_bench_amd import _capi
    nb, npr = 40000, 50011
    build, probe = po.gen_uniform_u32(nb, 1, 1, 3000), po.gen_uniform_u32(npr, 2, 1, 3500)
    ids, pos, cnt, rid = _answer("radix", build, probe)
    for left_outer in (False, True):
        w = gt.Watch(fill)
        off_in = offsets[0]
        g_ids = w.col(nb, off_in, data=ids, freeze=True)
        g_pos = w.col(npr, off_in, data=pos, freeze=True)
        g_cnt = w.col(npr, (off_in + 1) % 4 if offsets[0] != offsets[1] else off_in, data=cnt, freeze=True)
        g_rid = w.col(npr, off_in, data=rid, freeze=True)
        ws = w.ws(_capi.lib().dbhip_join_pairs_workspace_bytes(npr))
        total = w.u64(1)
        want = _expected(build, probe, left_outer)
        out_b, out_p = w.col(want.size, offsets[0]), w.col(want.size, offsets[1])
        _raw(g_ids, nb, g_rid, g_pos, g_cnt, npr, left_outer, want.size, out_b, out_p, total, ws)
        assert _status(ws) == 0 and int(total.item()) == want.size
        assert np.array_equal(_packed(_u32(out_b), _u32(out_p)), want)
        w.check()


def test_one_plan_three_inputs_on_a_dirty_workspace():
    from dwarf_bench_amd import ops
    nb, npr = 100000, 120007
    plan = None
    for seed, key_hi, fill in ((1, 50000, gt.FILLS[0]), (5, 900, gt.FILLS[1]), (9, 1 << 30, gt.FILLS[0])):
        build, probe = po.gen_uniform_u32(nb, seed, 1, key_hi), po.gen_uniform_u32(npr, seed + 1, 1, key_hi)
        want = _expected(build, probe, True)
        if plan is None:
            plan = ops.JoinPairs(npr, 20_000_000)
        plan.ws.view(torch.int32).fill_(gt.i32(fill))
        plan.total.fill_(gt.i64(fill))
        ids, pos, cnt, rid = _answer("radix", build, probe)
        plan.launch(ids, pos, cnt, rid, True)
        b, p = plan.result()
        assert np.array_equal(_packed(_u32(b), _u32(p)), want)


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()  # warm-up outside capture (lazy module loads, attribute calls)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def test_graph_capture_and_three_replays():
    """the join and the expansion captured as one linear sequence; the key columns refilled and replayed three times"""
    from dwarf_bench_amd import ops
    nb, npr = 1 << 18, (1 << 18) + 1000
    bk = torch.empty(nb, dtype=torch.int32, device="cuda")
    pk = torch.empty(npr, dtype=torch.int32, device="cuda")
    bk.copy_(ops.gen_uniform_u32(nb, 1, 1, nb))
    pk.copy_(ops.gen_uniform_u32(npr, 2, 1, nb))
    join = ops.HashJoin(nb, npr)
    plan = ops.JoinPairs(npr, 8 * npr)

    def run():
        join.build(bk)
        join.probe(pk)
        plan.launch(join.ids[:nb], join.pos[:npr], join.cnt[:npr], None, True)

    g = _capture(run)
    for seed, key_hi in ((11, nb), (12, nb // 4), (13, 1 << 31)):
        bk.copy_(ops.gen_uniform_u32(nb, seed, 1, key_hi))
        pk.copy_(ops.gen_uniform_u32(npr, seed + 100, 1, key_hi))
        plan.build_rows.fill_(-2)
        plan.probe_rows.fill_(-2)
        g.replay()
        torch.cuda.synchronize()
        assert ops.workspace_status(join.ws) == 0
        b, p = plan.result()
        want = _expected(_u32(bk), _u32(pk), True)
        assert np.array_equal(_packed(_u32(b), _u32(p)), want), seed


def _verdict(words, n_pairs):
    return words[0] == 0 and words[1] == n_pairs and words[2] == words[3]


def test_the_validator_reports_every_kind_of_damage():
    from dwarf_bench_amd import ops
    nb, npr = 30000, 31000
    build, probe = po.gen_uniform_u32(nb, 1, 1, 20000), po.gen_uniform_u32(npr, 2, 1, 20000)
    bk, pk = jt.dev(build), jt.dev(probe)
    for left_outer in (False, True):
        for route in ("hash", "radix"):
            ids, pos, cnt, rid = _answer(route, build, probe)
            plan = ops.JoinPairs(npr, 200000)
            plan.launch(ids, pos, cnt, rid, left_outer)
            b, p = plan.result()
            n = b.numel()

            def check(bb, pp):
                return ops.check_join_pairs(bk, pk, ids, pos, cnt, bb, pp, rid, left_outer)

            good = check(b, p)
            assert _verdict(good, n), good
            hb, hp = _u32(b), _u32(p)
            real = np.flatnonzero(hb != SENTINEL)
            # one build id xor 1
            bad = b.clone()
            at = int(real[len(real) // 2])
            bad[at] ^= 1
            assert not _verdict(check(bad, p), n)
            # two probe ids swapped between rows of different keys
            other = next(int(i) for i in real if probe[hp[i]] != probe[hp[at]])
            badp = p.clone()
            badp[at], badp[other] = p[other], p[at]
            words = check(b, badp)
            assert words[0] == 2 and not _verdict(words, n)
            # one pair dropped, one duplicated
            assert not _verdict(check(b[:-1], p[:-1]), n - 1)
            dup_b, dup_p = torch.cat([b, b[at:at + 1]]), torch.cat([p, p[at:at + 1]])
            words = check(dup_b, dup_p)
            assert words[0] == 0 and not _verdict(words, n + 1)
            if left_outer:  # a sentinel on a row that has matches: no bad pair, the fingerprints differ
                bad = b.clone()
                bad[at] = -1
                words = check(bad, p)
                assert words[0] == 0 and words[1] == n and words[2] != words[3]
            else:  # a sentinel in an inner join is a bad pair
                bad = b.clone()
                bad[at] = -1
                assert check(bad, p)[0] == 1


def test_the_validator_accepts_16m_rows_a_side():
    from dwarf_bench_amd import ops
    n = 1 << 24
    bk, pk = ops.gen_uniform_u32(n, 42, 1, n), ops.gen_uniform_u32(n, 43, 1, n)
    b, p = ops.join_pairs(bk, pk)
    join = ops.RadixJoin(n, n)
    join.partition_build(bk)
    join.partition_probe(pk)
    join.match()
    rid, pos, cnt, ids = join.result()
    plan = ops.JoinPairs(n, b.numel())
    plan.launch(ids, pos, cnt, rid)
    b2, p2 = plan.result()
    assert b2.numel() == b.numel()
    words = ops.check_join_pairs(bk, pk, ids, pos, cnt, b2, p2, rid)
    print("2^24 x 2^24:", b2.numel(), "pairs", words)
    assert _verdict(words, b2.numel()), words
    # the same pairs, whatever order inside a key's ids the two joins chose
    assert torch.equal(torch.sort((p.long() << 32) | (b.long() & 0xFFFFFFFF))[0],
                       torch.sort((p2.long() << 32) | (b2.long() & 0xFFFFFFFF))[0])


def test_join_pairs_both_orders_and_a_given_capacity():
    from dwarf_bench_amd import _capi, ops
    n = 200003
    build, probe = po.gen_uniform_u32(n, 1, 1, n // 4), po.gen_uniform_u32(n + 5, 2, 1, n // 4)
    bk, pk = jt.dev(build), jt.dev(probe)
    for left_outer in (False, True):
        want = _expected(build, probe, left_outer)
        for ordered in (False, True):
            b, p = ops.join_pairs(bk, pk, left_outer=left_outer, ordered=ordered)
            assert np.array_equal(_packed(_u32(b), _u32(p)), want)
            if ordered:
                assert bool((p[1:] >= p[:-1]).all())
            b, p = ops.join_pairs(bk, pk, left_outer=left_outer, capacity=want.size + 10, ordered=ordered)
            assert np.array_equal(_packed(_u32(b), _u32(p)), want)
        with pytest.raises(_capi.DbhipError, match=str(want.size)):
            ops.join_pairs(bk, pk, left_outer=left_outer, capacity=want.size - 1)


def _cli(args, env=None, timeout=600):
    return subprocess.run([str(CLI)] + args, capture_output=True, text=True, timeout=timeout,
                          env={**os.environ, **(env or {})})


@pytest.mark.parametrize("size", ["1024", "65536", "4194304"])
def test_cli_results_are_valid(size):
    r = _cli(["JoinPairsHip", "--device=hip", f"--input_size={size}", "--iterations=3"])
    assert r.returncode == 0, r.stderr
    assert "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 3


@pytest.mark.parametrize("size,limit", [("1024", None), ("4194304", "1024")])  # the host check / the device-side validators
def test_cli_fault_injection_flips_valid(size, limit):
    env = {"DWARF_BENCH_VALIDATE_MAX": limit} if limit else {}
    args = ["JoinPairsHip", "--device=hip", f"--input_size={size}", "--iterations=3"]
    r = _cli(args, env={**env, "DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("ncorrect results") == 3 and "Caught exception" not in r.stderr, r.stderr
    r = _cli(args, env=env)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 3
