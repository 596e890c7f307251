"""The cuckoo table on the GPU (csrc/cuckoo.hip through ops.CuckooTable): the reference tests' known answers in serial
mode, exact parity of the serial mode with the Python model of the reference's algorithm, parallel builds checked slot by
slot, the rebuild loop, the bounded give-up path, and the CuckooHashBuildHip dwarf of the experimental CLI."""
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests.cuckoo_model import EMPTY_KEY, CuckooModel, murmur3_x86_32_np, positions_np

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_experimental"
VAL_XOR = 0x13579BDF  # vals = keys ^ VAL_XOR: a value that is not its key shows which word went where


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def kats(golden_dir):
    return json.loads((golden_dir / "cuckoo_kats.json").read_text())


def _kat_table(case, serial):
    from dwarf_bench_amd import ops
    t = ops.CuckooTable(case["table_size"], hash_kind=case["hash_kind"], seeds=tuple(case["seeds"]))
    ins = np.array(case["inserts"], dtype=np.uint32)
    res = t.insert(_dev(ins[:, 0]), _dev(ins[:, 1]), serial=serial, max_iter=case["max_iter"], want_results=True)
    return t, _host(res)


def _layout(t):
    k, v = (_host(x) for x in t.slots())
    return {i: (int(k[i]), int(v[i])) for i in range(len(k)) if k[i] != EMPTY_KEY}, k, v


@pytest.mark.parametrize("name", ["insert", "at", "fails_to_insert", "parallel_insertion"])
def test_reference_kats_serial(kats, name):
    case = next(c for c in kats["cases"] if c["name"] == name)
    t, res = _kat_table(case, serial=True)
    d, a = case["derived"], case["asserted"]
    assert res.tolist() == d["insert_results"]
    if "insert_results" in a:
        assert res.tolist() == a["insert_results"]
    layout, k, v = _layout(t)
    want = d.get("slots", d.get("slots_if_serial"))
    assert layout == {int(s): tuple(kv) for s, kv in want.items()}
    assert np.all(v[k == EMPTY_KEY] == 0)  # empty slots hold (0xFFFFFFFF, 0)
    if "keys_present_count" in a:
        assert int(np.isin(k, a["keys_present_count"]["keys"]).sum()) == a["keys_present_count"]["count"]
    if a.get("lookups"):
        q = np.array([l[0] for l in a["lookups"]], dtype=np.uint32)
        vals, found = (_host(x) for x in t.lookup(_dev(q)))
        for (key, val, f), gv, gf in zip(a["lookups"], vals, found):
            assert bool(gf) == f, key
            if val is not None:
                assert gv == val, key
    from dwarf_bench_amd import ops
    assert t.failed() == (0 in d["insert_results"])
    assert t.status() == (ops.DEV_TABLE_FULL if 0 in d["insert_results"] else ops.DEV_OK)


def test_reference_parallel_insertion_in_parallel_mode(kats):
    case = next(c for c in kats["cases"] if c["name"] == "parallel_insertion")
    t, res = _kat_table(case, serial=False)
    assert res.tolist() == [1] * 5 and not t.failed()
    q = np.array([l[0] for l in case["asserted"]["lookups"]], dtype=np.uint32)
    vals, found = (_host(x) for x in t.lookup(_dev(q)))
    assert found.tolist() == [1] * 5 and vals.tolist() == q.tolist()


@pytest.mark.parametrize("n,size,max_iter,kind", [(300, 1200, 0, 1), (300, 400, 0, 1), (500, 640, 37, 1), (257, 257, 300, 1),
                                                   (300, 400, 0, 2)])
def test_serial_mode_matches_the_model(n, size, max_iter, kind):
    """Murmur3 (the reference's) and splitmix64 hashers, a few hundred random keys; the loads past 0.5 make chains fail,
    so the dropped pairs and the per-insert results are compared too"""
    from dwarf_bench_amd import ops
    rng = np.random.default_rng(n * 7 + size)
    keys = rng.choice(np.uint32(0xFFFFFFFE), size=n, replace=False).astype(np.uint32)
    vals = keys ^ np.uint32(VAL_XOR)
    seeds = ops.cuckoo_seed_pair(size, 0)
    m = CuckooModel(size, kind, seeds, murmur=po.murmur3_x86_32)
    want = [m.insert(int(k), int(v), max_iter or min(n, 100000)) for k, v in zip(keys, vals)]
    t = ops.CuckooTable(size, hash_kind=kind, seeds=seeds)
    res = _host(t.insert(_dev(keys), _dev(vals), serial=True, max_iter=max_iter, want_results=True))
    assert res.tolist() == [int(w) for w in want]
    layout, _, _ = _layout(t)
    assert layout == m.layout()
    assert t.failed() == (not all(want))
    if size < 2 * n:
        assert not all(want), "a load past 0.5 was meant to make chains fail"
    got_v, got_f = (_host(x) for x in t.lookup(_dev(keys)))
    for k, gv, gf in zip(keys.tolist(), got_v.tolist(), got_f.tolist()):
        v, f = m.at(k)
        assert bool(gf) == f and (gv == v if f else gv == 0), k


def _check_build(t, keys, vals):
    """every key stored exactly once, at h1 or h2, with its own value; lookups find all of them; keys that were not
    inserted are never found"""
    s1, s2 = t.seeds
    sk, sv = (_host(x) for x in t.slots())
    occ = np.nonzero(sk != EMPTY_KEY)[0]
    assert np.array_equal(np.sort(sk[occ]), np.sort(keys))
    assert np.all(sv[sk == EMPTY_KEY] == 0)
    h1 = positions_np(sk[occ], t.kind, s1, t.size)
    h2 = positions_np(sk[occ], t.kind, s2, t.size)
    assert np.all((occ == h1) | (occ == h2))
    assert np.array_equal(sv[occ], sk[occ] ^ np.uint32(VAL_XOR))
    got_v, got_f = (_host(x) for x in t.lookup(_dev(keys)))
    assert np.all(got_f == 1) and np.array_equal(got_v, vals)
    absent = (keys - keys % 10) + (keys % 10 + 1) % 10  # another key of the same decade: never generated
    got_v, got_f = (_host(x) for x in t.lookup(_dev(absent)))
    assert not got_f.any() and not got_v.any()


@pytest.mark.parametrize("n,kind", [(1, 2), (1 << 10, 2), ((1 << 16) + 3, 2), (1 << 22, 2), (1, 1), (1 << 10, 1),
                                    ((1 << 16) + 3, 1)])
def test_parallel_build_at_load_one_quarter(n, kind):
    from dwarf_bench_amd import ops
    keys = po.gen_unique_sorted_u32(n, 21)
    vals = keys ^ np.uint32(VAL_XOR)
    t = ops.CuckooTable(4 * n, hash_kind=kind, seeds=ops.cuckoo_seed_pair(0, 0))
    res = _host(t.insert(_dev(keys), _dev(vals), want_results=True))
    assert t.status() == ops.DEV_OK and np.all(res == 1)
    _check_build(t, keys, vals)


def test_reference_hasher_pair_cannot_hold_2p22_keys():
    """The same 2^22 keys with the reference's two Murmur3 seeds (hash_kind 1): three components of this cuckoo graph
    hold more keys than slots (positions of related keys coincide, include/dbhip.h), so no placement exists.  The build
    must finish and say so; every key it kept sits at one of its two positions."""
    from dwarf_bench_amd import ops
    n = 1 << 22
    keys = po.gen_unique_sorted_u32(n, 21)
    vals = keys ^ np.uint32(VAL_XOR)
    t = ops.CuckooTable(4 * n, hash_kind=1, seeds=ops.cuckoo_seed_pair(0, 0))
    res = _host(t.insert(_dev(keys), _dev(vals), want_results=True))
    assert t.status() == ops.DEV_TABLE_FULL and 1 <= int((res == 0).sum()) <= 1000
    sk, sv = (_host(x) for x in t.slots())
    occ = np.nonzero(sk != EMPTY_KEY)[0]
    assert len(occ) == n - int((res == 0).sum())
    assert np.all((occ == positions_np(sk[occ], 1, t.seeds[0], t.size)) | (occ == positions_np(sk[occ], 1, t.seeds[1], t.size)))
    assert np.array_equal(sv[occ], sk[occ] ^ np.uint32(VAL_XOR))


def test_rebuild_at_load_045():
    from dwarf_bench_amd import ops
    n = 1 << 16
    keys = po.gen_unique_sorted_u32(n, 22)
    vals = keys ^ np.uint32(VAL_XOR)
    t, attempts = ops.cuckoo_build(_dev(keys), _dev(vals), table_size=int(n / 0.45), seed=5)
    assert 1 <= attempts <= 16 and t.status() == ops.DEV_OK
    _check_build(t, keys, vals)
    # 1024 keys, 2275 slots: the first seed pair of seed 2 makes a cuckoo graph with a component of more keys than
    # slots (checked on the host), the second does not: the build must fail once and then succeed
    keys = po.gen_unique_sorted_u32(1024, 23)
    vals = keys ^ np.uint32(VAL_XOR)
    t, attempts = ops.cuckoo_build(_dev(keys), _dev(vals), table_size=int(1024 / 0.45), seed=2, hash_kind=1)
    assert attempts == 2 and t.seeds == ops.cuckoo_seed_pair(2, 1)
    _check_build(t, keys, vals)


def test_overfull_build_gives_up_after_max_attempts():
    from dwarf_bench_amd import _capi, ops
    keys = po.gen_unique_sorted_u32(3000, 24)
    with pytest.raises(_capi.DbhipError, match="3 attempts failed"):
        ops.cuckoo_build(_dev(keys), _dev(keys), table_size=4000, max_attempts=3)


def test_bounded_give_up_and_the_empty_key():
    """three copies of one key for its two slots: the chain of one of them reaches max_iter, that row reports 0 and the
    status word TABLE_FULL; the launch finishes.  0xFFFFFFFF is not a key: KEY_RANGE, not inserted, never found."""
    from dwarf_bench_amd import ops
    seeds = ops.cuckoo_seed_pair(9, 0)
    size = 1 << 12
    key = next(k for k in range(1, 1000)
               if murmur3_x86_32_np([k], seeds[0])[0] % size != murmur3_x86_32_np([k], seeds[1])[0] % size)
    t = ops.CuckooTable(size, hash_kind=1, seeds=seeds)
    res = _host(t.insert(_dev([key] * 3), _dev([1, 2, 3]), max_iter=64, want_results=True))
    assert t.status() == ops.DEV_TABLE_FULL and t.failed()
    assert sorted(res.tolist()) == [0, 1, 1]
    sk, _ = (_host(x) for x in t.slots())
    assert int((sk == key).sum()) == 2 and int((sk != EMPTY_KEY).sum()) == 2
    t.reset()
    assert t.status() == ops.DEV_OK and not t.failed()
    res = _host(t.insert(_dev([5, EMPTY_KEY, 6]), _dev([50, 99, 60]), want_results=True))
    assert res.tolist() == [1, 0, 1] and t.status() == ops.DEV_KEY_RANGE and not t.failed()
    vals, found = (_host(x) for x in t.lookup(_dev([EMPTY_KEY, 5, 6, 7])))
    assert found.tolist() == [0, 1, 1, 0] and vals.tolist() == [0, 50, 60, 0]
    empty = ops.CuckooTable(16, hash_kind=1, seeds=seeds)  # every slot holds the empty pattern
    vals, found = (_host(x) for x in empty.lookup(_dev([EMPTY_KEY])))
    assert found.tolist() == [0] and vals.tolist() == [0]


def _run(args, **kw):
    return subprocess.run([str(CLI)] + args, capture_output=True, text=True, timeout=600, **kw)


def test_cli_cuckoo_dwarf():
    sizes = ["128", "256", "512", "1024", "2048", "4096"]
    r = _run(["CuckooHashBuildHip", "--device=hip", "--iterations", "10", "--input_size"] + sizes)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 60
    assert r.stdout.count("CuckooHashBuildHip: 4096 keys, 16384 slots: ") == 10
    r = _run(["CuckooHashBuildHip", "--device=hip", "--iterations", "1", "--input_size", str(1 << 24)])
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert r.stdout.count("Host duration:") == 1


@pytest.mark.parametrize("limit", ["16777216", "1"])  # host check / device-side check
def test_cli_cuckoo_validator_catches_an_injected_fault(limit):
    env = {**os.environ, "DWARF_BENCH_VALIDATE_MAX": limit}
    r = _run(["CuckooHashBuildHip", "--device=hip", "--iterations", "3", "--input_size", "65536"], env=env)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    r = _run(["CuckooHashBuildHip", "--device=hip", "--iterations", "3", "--input_size", "65536"],
             env={**env, "DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0 and r.stderr.count("ncorrect results") == 3, r.stderr
