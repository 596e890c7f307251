"""The slab table on the GPU (csrc/slab.hip through ops.SlabTable): the reference tests' known answers, exact parity of
the serial mode with the Python model of the reference's algorithm, the invariants of concurrent builds checked slab by
slab, the bounded pool, reused workspaces, ops.slab_join against seq_join, and the slab dwarfs of the dwarf_bench_slab
CLI."""
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests.slab_model import EMPTY_KEY, NONE, SlabModel

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_slab"
HASH_BUILD = (242792921, 653019598, 2147483647)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _buckets_of(keys, hasher, buckets):
    a, b, p = hasher
    k = keys.astype(np.uint64)
    return ((np.uint64(a) * k + np.uint64(b)) % np.uint64(p)) % np.uint64(buckets)


def _export(t):
    k, v, nxt, used = t.slabs()
    return _host(k), _host(v), _host(nxt), used


@pytest.fixture(scope="module")
def kats(golden_dir):
    return json.loads((golden_dir / "slab_kats.json").read_text())


def _pairs(case):
    if "inserts" in case:
        return np.array(case["inserts"], dtype=np.uint32)
    r = case["inserts_rule"]
    i = np.arange(r["i_from"], r["i_to"], dtype=np.uint64)
    return np.stack([i * i, i * i], axis=1).astype(np.uint32)


@pytest.mark.parametrize("name", ["insert", "find_and_insert_together_big", "find_and_insert_together"])
@pytest.mark.parametrize("serial", [True, False])
def test_reference_kats(kats, name, serial):
    from dwarf_bench_amd import ops
    case = next(c for c in kats["cases"] if c["name"] == name)
    pairs = _pairs(case)
    B = case["buckets"]
    t = ops.SlabTable(B, case["heap_nodes"] - B, tuple(case["hasher"]))
    res = _host(t.insert(_dev(pairs[:, 0]), _dev(pairs[:, 1]), serial=serial, want_results=True))
    assert res.tolist() == [1] * len(pairs) and t.status() == ops.DEV_OK
    keys, vals, nxt, used = _export(t)
    if case["asserted"].get("each_pair_in_root_slab_of_its_bucket"):
        for (k, v), b in zip(pairs, _buckets_of(pairs[:, 0], case["hasher"], B)):
            assert np.any((keys[b] == k) & (vals[b] == v)), (k, v)
    # every pair found: the KATs' keys are unique but for key 5 of "insert", whose first slot in chain order wins
    m = SlabModel(B, case["heap_nodes"] - B, tuple(case["hasher"]))
    for k, v in pairs.tolist():
        m.insert(k, v)
    got_v, got_f = (_host(x) for x in t.lookup(_dev(pairs[:, 0])))
    for (k, _), gv, gf in zip(pairs.tolist(), got_v, got_f):
        want_v, want_f = m.find(k)
        assert gf == 1 and want_f
        if serial or k != 5:
            assert gv == want_v, k
        else:
            assert gv in (2, 5)
    if serial:  # the reference's sequential layout, slot by slot
        mk, mv, mn, mu = m.export()
        assert np.array_equal(keys, mk) and np.array_equal(vals, mv) and np.array_equal(nxt, mn) and used == mu
        want = case["derived"].get("root_slabs_if_serial")
        if want:
            got = {str(b): [[s, int(keys[b][s]), int(vals[b][s])] for s in range(32) if keys[b][s] != EMPTY_KEY]
                   for b in range(B) if keys[b][0] != EMPTY_KEY}
            assert got == want


def test_serial_mode_matches_the_model_with_long_chains():
    """2,000 keys with duplicates in 7 buckets: chains of about 9 slabs, every slot, link and pool node as the model's"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 300, 2000).astype(np.uint32)
    vals = np.arange(2000, dtype=np.uint32)
    t = ops.SlabTable(7, 200, HASH_BUILD)
    t.insert(_dev(keys), _dev(vals), serial=True)
    assert t.status() == ops.DEV_OK
    m = SlabModel(7, 200, HASH_BUILD)
    assert all(m.insert(int(k), int(v)) for k, v in zip(keys, vals))
    got, want = _export(t), m.export()
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
    assert max(len(m.chain(b)) for b in range(7)) >= 8
    q = np.concatenate([keys[:500], np.arange(300, 400, dtype=np.uint32)])
    gv, gf = (_host(x) for x in t.lookup(_dev(q)))
    assert [(int(v), True) if f else (None, False) for v, f in zip(gv, gf)] == [m.find(int(k)) for k in q]


def _check_invariants(t, keys, hasher=HASH_BUILD):
    """the table built from (keys, row ids): per bucket the stored (key, row id) multiset is the input's, every pair in
    its bucket's chain, every slab but a chain's last full, max(1, ceil(count / 32)) linked slabs, unlinked pool nodes
    empty; lookups find every key with a row of that key and miss absent keys"""
    from dwarf_bench_amd import ops
    n, B = keys.size, t.buckets
    assert t.status() == ops.DEV_OK
    K, V, N, used = _export(t)
    assert used <= t.pool
    nxt = N.tolist()
    owner = np.full(t.nodes, -1, dtype=np.int64)
    slabs = np.zeros(B, dtype=np.int64)
    last = np.zeros(t.nodes, dtype=bool)
    for b in range(B):
        node, steps = b, 0
        while True:
            assert owner[node] == -1 and steps <= t.nodes
            owner[node] = b
            steps += 1
            if nxt[node] == NONE:
                break
            node = nxt[node]
            assert B <= node < t.nodes
        slabs[b], last[node] = steps, True
    fill = (K != EMPTY_KEY).sum(axis=1)
    linked = owner >= 0
    assert np.all(fill[linked & ~last] == 32)  # every slab but a chain's last is full
    assert np.all(fill[~linked] == 0) and np.all(V[~linked] == 0)  # spare pool nodes stay empty
    assert np.all(V[K == EMPTY_KEY] == 0)
    cnt = np.bincount(_buckets_of(keys, hasher, B).astype(np.int64), minlength=B)
    assert np.array_equal(slabs, np.maximum(1, -(-cnt // 32)))
    full = K != EMPTY_KEY
    node_of = np.broadcast_to(np.arange(t.nodes)[:, None], K.shape)[full]
    sk, sv = K[full], V[full]
    assert sk.size == n and np.array_equal(np.sort(sv), np.arange(n, dtype=np.uint32))  # each row once
    assert np.array_equal(keys[sv], sk)  # with its own key
    assert np.array_equal(owner[node_of], _buckets_of(sk, hasher, B).astype(np.int64))  # in its bucket's chain
    # lookups: present keys with a row id of that key, absent keys missed
    gv, gf = t.lookup(_dev(keys))
    gv, gf = _host(gv), _host(gf)
    assert np.all(gf == 1) and np.all(gv < n) and np.array_equal(keys[gv], keys)
    present = np.unique(keys)
    absent = np.setdiff1d(np.random.default_rng(9).integers(0, 2**32 - 1, 200000, dtype=np.uint64).astype(np.uint32),
                          present)[:100000]
    av, af = (_host(x) for x in t.lookup(_dev(absent)))
    assert not af.any() and not av.any()


def _build(keys, buckets=None, pool=None):
    from dwarf_bench_amd import ops
    n = keys.size
    b = buckets or ops.slab_buckets(n)
    t = ops.SlabTable(b, pool if pool is not None else b + ops.SLAB_MAX_GROUPS, HASH_BUILD)
    res = _host(t.insert(_dev(keys), _dev(np.arange(n, dtype=np.uint32)), want_results=True))
    assert np.all(res == 1) and t.status() == ops.DEV_OK
    return t


@pytest.mark.parametrize("lg", [20, 24])
def test_concurrent_build_unique_keys(lg):
    from dwarf_bench_amd import ops
    keys = _host(ops.gen_unique_sorted_u32(1 << lg, 11))
    keys = keys[np.random.default_rng(lg).permutation(keys.size)]
    _check_invariants(_build(keys), keys)


@pytest.mark.parametrize("lg", [20, 24])
def test_concurrent_build_reference_keys(lg):
    """SlabHashBuild's input: uniform keys in [1, 10000], each repeated about 2^lg / 10^4 times, chains ~2^lg / 320000
    slabs long"""
    from dwarf_bench_amd import ops
    keys = _host(ops.gen_uniform_u32(1 << lg, 21, 1, 10000))
    _check_invariants(_build(keys), keys)


def test_concurrent_build_one_key():
    """every row the same key: one chain of n / 32 slabs that every group appends to"""
    from dwarf_bench_amd import ops
    n = 1 << 16
    keys = np.full(n, 77, dtype=np.uint32)
    t = _build(keys, pool=n // 32 + ops.SLAB_MAX_GROUPS)
    _check_invariants(t, keys)


def test_pool_exhaustion_is_reported_and_bounded():
    """a pool far too small: the call returns, DBHIP_DEV_TABLE_FULL is raised, out_inserted marks exactly the stored
    rows, all of them are found, and a canary band behind the workspace in the same allocation is untouched"""
    from dwarf_bench_amd import ops
    B, P, n = 4, 8, 5000
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1000, n).astype(np.uint32)
    t = ops.SlabTable(B, P, HASH_BUILD)
    big = torch.full((t.ws_bytes + 8192,), 0x5A, dtype=torch.uint8, device="cuda")
    t.ws = big[: t.ws_bytes]
    t.reset()
    res = _host(t.insert(_dev(keys), _dev(np.arange(n, dtype=np.uint32)), want_results=True))
    torch.cuda.synchronize()
    assert t.status() == ops.DEV_TABLE_FULL and t.failed()
    assert bool((big[t.ws_bytes:] == 0x5A).all())
    K, V, N, used = _export(t)
    assert used == P
    full = K != EMPTY_KEY
    stored = np.sort(V[full])
    assert np.array_equal(stored, np.flatnonzero(res == 1).astype(np.uint32))
    assert 0 < stored.size <= (B + P) * 32 and np.array_equal(keys[V[full]], K[full])
    gv, gf = (_host(x) for x in t.lookup(_dev(keys[res == 1])))
    assert np.all(gf == 1) and np.array_equal(keys[gv], keys[res == 1])


def test_the_empty_key_is_refused():
    from dwarf_bench_amd import ops
    t = ops.SlabTable(16, 4, ops.SLAB_HASHER_TESTS)
    res = _host(t.insert(_dev([5, EMPTY_KEY, 6]), _dev([50, 99, 60]), want_results=True))
    assert res.tolist() == [1, 0, 1] and t.status() == ops.DEV_KEY_RANGE and not t.failed()
    K, V, _, _ = _export(t)
    assert int((K != EMPTY_KEY).sum()) == 2 and 99 not in V
    vals, found = (_host(x) for x in t.lookup(_dev([EMPTY_KEY, 5, 6, 7])))
    assert found.tolist() == [0, 1, 1, 0] and vals.tolist() == [0, 50, 60, 0]


@pytest.mark.parametrize("poison", ["ff", "random"])
def test_reset_of_a_poisoned_workspace(poison):
    """reset turns a 0xFF-filled or random-filled workspace into an empty table; a build on it is correct"""
    from dwarf_bench_amd import ops
    keys = _host(ops.gen_uniform_u32(1 << 18, 3, 1, 2000))
    B = ops.slab_buckets(keys.size)
    t = ops.SlabTable(B, B + ops.SLAB_MAX_GROUPS, HASH_BUILD)
    if poison == "ff":
        t.ws.fill_(0xFF)
    else:
        t.ws.copy_(torch.randint(0, 256, t.ws.shape, dtype=torch.uint8, device="cuda"))
    t.reset()
    K, V, N, used = _export(t)
    assert np.all(K == EMPTY_KEY) and not V.any() and np.all(N == NONE) and used == 0 and t.status() == ops.DEV_OK
    t.insert(_dev(keys), _dev(np.arange(keys.size, dtype=np.uint32)))
    _check_invariants(t, keys)


def test_two_builds_with_a_reset_between():
    from dwarf_bench_amd import ops
    first = _host(ops.gen_uniform_u32(1 << 18, 4, 1, 500))
    second = _host(ops.gen_unique_sorted_u32(1 << 18, 5))
    B = ops.slab_buckets(first.size)
    t = ops.SlabTable(B, B + ops.SLAB_MAX_GROUPS, HASH_BUILD)
    t.insert(_dev(first), _dev(np.arange(first.size, dtype=np.uint32)))
    _check_invariants(t, first)
    t.reset()
    t.insert(_dev(second), _dev(np.arange(second.size, dtype=np.uint32)))
    _check_invariants(t, second)


def _join_inputs(n, seed):
    from dwarf_bench_amd import ops
    return [_host(ops.gen_unique_sorted_u32(n, seed + i)) for i in range(4)]


def test_slab_join_on_sorted_unique_inputs():
    from dwarf_bench_amd import ops
    ak, av, bk, bv = _join_inputs(20000, 11)
    got = [_host(x) for x in ops.slab_join(_dev(ak), _dev(av), _dev(bk), _dev(bv))]
    want = po.seq_join(ak, av, bk, bv)
    assert want[0].size > 1000 and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_slab_join_on_shuffled_inputs_with_key_zero():
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(12)
    ak, av, bk, bv = _join_inputs(20000, 21)
    ak[0], bk[0] = 0, 0  # key 0 on both sides (the reference's compaction drops it)
    pa, pb = rng.permutation(ak.size), rng.permutation(bk.size)
    ak, av, bk, bv = ak[pa], av[pa], bk[pb], bv[pb]
    got = [_host(x) for x in ops.slab_join(_dev(ak), _dev(av), _dev(bk), _dev(bv))]
    want = po.seq_join(ak, av, bk, bv)
    assert 0 in got[0] and got[0].size == want[0].size > 1000
    g = sorted(zip(*(x.tolist() for x in got)))
    w = sorted(zip(*(x.tolist() for x in want)))
    assert g == w
    # probe-row order: the hits' probe values appear in the order of their probe rows
    pos = {int(v): i for i, v in enumerate(bv)}
    assert [pos[int(v)] for v in got[2]] == sorted(pos[int(v)] for v in got[2])


def _run(args, **kw):
    return subprocess.run([str(CLI)] + args, capture_output=True, text=True, timeout=900, **kw)


@pytest.mark.parametrize("dwarf", ["SlabHashBuildHip", "SlabProbeHip", "SlabJoinHip"])
def test_cli_slab_dwarfs(dwarf, tmp_path):
    sizes = ["1", "19", "128", "1000", "4096", "65536"]
    rep = tmp_path / "r.csv"
    r = _run([dwarf, "--device=hip", "--iterations", "3", f"--report_path={rep}", "--input_size"] + sizes)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert len(rep.read_text().splitlines()) == 1 + 3 * len(sizes)  # a header and one row per run
    r = _run([dwarf, "--device=hip", "--iterations", "1", "--input_size", str(1 << 24)])
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 1


@pytest.mark.parametrize("limit", ["16777216", "1"])  # host check / device-side check
@pytest.mark.parametrize("dwarf", ["SlabHashBuildHip", "SlabProbeHip", "SlabJoinHip"])
def test_cli_slab_validators_catch_an_injected_fault(dwarf, limit):
    env = {**os.environ, "DWARF_BENCH_VALIDATE_MAX": limit}
    r = _run([dwarf, "--device=hip", "--iterations", "2", "--input_size", "65536"], env=env)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    r = _run([dwarf, "--device=hip", "--iterations", "2", "--input_size", "65536"],
             env={**env, "DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0 and r.stderr.count("ncorrect results") == 2, r.stderr
