"""The slab table without a GPU: the Python model against the reference tests' assertions, the exact bucket hash the
kernel computes without a 64-bit division, the C ABI's workspace query and argument checks (host-side, before any HIP
call), and the compiled code object of csrc/slab.hip."""
import json
import random
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE
from tests.slab_model import (EMPTY_KEY, NONE, SlabModel, barrett_constant, barrett_rem, barrett_rem_np, device_hash,
                              slab_hash)

ROOT = Path(__file__).resolve().parents[1]
REFERENCE_HASHERS = [(242792921, 653019598, 2147483647), (32, 48, 1031), (13, 24, 343)]
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def kats(golden_dir):
    return json.loads((golden_dir / "slab_kats.json").read_text())


def _pairs(case):
    if "inserts" in case:
        return [tuple(p) for p in case["inserts"]]
    r = case["inserts_rule"]
    assert r["key"] == "i*i" and r["value"] == "i*i"
    return [(i * i, i * i) for i in range(r["i_from"], r["i_to"])]


def _model(case):
    m = SlabModel(case["buckets"], case["heap_nodes"] - case["buckets"], tuple(case["hasher"]))
    return m, [m.insert(k, v) for k, v in _pairs(case)]


def test_model_reproduces_every_reference_assertion(kats):
    assert kats["empty_key"] == EMPTY_KEY and kats["slab_size"] == 32
    assert [c["name"] for c in kats["cases"]] == ["insert", "find_and_insert_together_big", "find_and_insert_together"]
    for case in kats["cases"]:
        m, results = _model(case)
        assert all(results), case["name"]
        a, d = case["asserted"], case["derived"]
        if a.get("each_pair_in_root_slab_of_its_bucket"):  # slab_tests.cpp:47-60, hasher at the default 1024 buckets
            for k, v in _pairs(case):
                b = slab_hash(k, *case["hasher"], case["buckets"])
                assert any(m.keys[b][s] == k and m.vals[b][s] == v for s in range(32)), (case["name"], k, v)
        finds = a.get("finds")
        if finds == "every key found with its value":
            finds = [[k, v, True] for k, v in _pairs(case)]
        for k, v, found in finds or []:
            assert m.find(k) == (v, found), (case["name"], k)
        if "root_slabs_if_serial" in d:
            assert {str(b): l for b, l in m.root_layout().items()} == d["root_slabs_if_serial"], case["name"]
        if "pool_used_if_serial" in d:
            assert m.used == d["pool_used_if_serial"]
            assert max(len(m.chain(b)) for b in range(case["buckets"])) == d["longest_chain_slabs"]


def test_model_duplicates_chains_and_pool_exhaustion():
    m = SlabModel(3, 2, (1, 0, 7))  # bucket = (k % 7) % 3
    for i in range(70):
        assert m.insert(3, i)  # bucket 0: 70 copies of one key fill the root, then 2 pool slabs with 6 slots left
    assert m.chain(0) == [0, 3, 4] and m.used == 2 and m.next[4] == NONE
    assert m.find(3) == (0, True)  # the first slot in chain order
    assert all(m.insert(3, 100 + i) for i in range(26))  # the last slab's 26 free slots still take rows
    assert not m.insert(3, 999) and m.used == 2  # then the pool is exhausted: not stored
    assert m.insert(1, 5) and m.find(1) == (5, True) and m.find(2) == (None, False)
    assert not m.insert(EMPTY_KEY, 1) and m.find(EMPTY_KEY) == (None, False)


def _hash_points(p):
    return [0, 1, 2, p - 1, p, p + 1, 2 * p, M32 - 1, M32]


def test_exact_hash_for_the_reference_hashers():
    """the kernel's division-free bucket equals ((A*k + B) % P) % buckets for the reference's three constant sets"""
    rng = random.Random(1)
    for a, b, p in REFERENCE_HASHERS:
        for buckets in (1, 2, 3, 7, 20, 343, 1000, 1024, 52428, 838860, 3355443, M32):
            keys = [k for k in _hash_points(p) if k <= M32] + [rng.randrange(1 << 32) for _ in range(200)]
            for k in keys:
                assert device_hash(k, a, b, p, buckets) == slab_hash(k, a, b, p, buckets), (a, b, p, buckets, k)


def test_exact_hash_for_random_parameters():
    rng = random.Random(2)
    for _ in range(3000):
        a, b = rng.randrange(1 << 32), rng.randrange(1 << 32)
        p = rng.choice([1, 2, 3, rng.randrange(1, 1 << 32), M32, M32 - 1, (1 << 31) - 1, (1 << 31) + 1])
        buckets = rng.choice([1, 5, 17, 999, rng.randrange(1, 1 << 32), M32])
        for k in _hash_points(p) + [rng.randrange(1 << 32)]:
            if k <= M32:
                assert device_hash(k, a, b, p, buckets) == slab_hash(k, a, b, p, buckets), (a, b, p, buckets, k)


def test_barrett_remainder_is_exact_over_the_whole_64_bit_range():
    """r = x - mulhi(x, floor((2^64-1)/d)) * d is below 3d, so two subtractions finish it (csrc/slab.hip sl_rem)"""
    rng = np.random.default_rng(3)
    for d in [1, 2, 3, 7, 1031, 343, 2147483647, M32, M32 - 1, 1 << 31] + [int(x) for x in rng.integers(1, 1 << 32, 40)]:
        xs = [0, 1, d - 1, d, d + 1, 2 * d, 3 * d - 1, (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 1 - ((1 << 64) - 1) % d,
              M32 * M32 + M32]
        for x in xs:
            m = barrett_constant(d)
            r0 = x - ((x * m) >> 64) * d
            assert 0 <= r0 < 3 * d, (d, x)
            assert barrett_rem(x, d) == x % d, (d, x)
        arr = rng.integers(0, np.iinfo(np.uint64).max, 20000, dtype=np.uint64, endpoint=True)
        arr = np.concatenate([arr, np.array([x for x in xs if x < (1 << 64)], dtype=np.uint64)])
        want = np.array([int(x) % d for x in arr], dtype=np.uint64)
        assert np.array_equal(barrett_rem_np(arr, d), want), d


def test_workspace_query():
    lib = _capi.lib()
    assert lib.dbhip_slab_table_workspace_bytes(0, 10) == 0
    assert lib.dbhip_slab_table_workspace_bytes(M32, 1) == 0 and lib.dbhip_slab_table_workspace_bytes(1, M32) == 0
    assert lib.dbhip_slab_table_workspace_bytes(1, 1 << 32) == 0
    for buckets, pool in ((1, 0), (1, 1), (7, 0), (1000, 1000), (838860, 838860), (M32 - 5, 5), (1, M32 - 1)):
        ws = lib.dbhip_slab_table_workspace_bytes(buckets, pool)
        assert ws % 256 == 0 and ws >= 256 + (buckets + pool) * (128 + 128 + 8), (buckets, pool)


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20  # a 256-aligned address that is never dereferenced: every call below fails on the host first
    B, P = 1024, 1024
    ws = lib.dbhip_slab_table_workspace_bytes(B, P)
    h = (13, 24, 343)

    def ins(keys=fake, vals=fake, n=16, w=fake, wb=ws, b=B, p=P, hash_=h, out=None):
        return lib.dbhip_slab_table_insert_u32(keys, vals, n, w, wb, b, p, *hash_, 0, out, None)

    # reset
    assert lib.dbhip_slab_table_reset(fake, ws, 0, P, None) == EINVAL
    assert lib.dbhip_slab_table_reset(fake, 1 << 44, M32, 1, None) == EINVAL
    assert lib.dbhip_slab_table_reset(None, ws, B, P, None) == EWORKSPACE
    assert lib.dbhip_slab_table_reset(fake + 8, ws, B, P, None) == EWORKSPACE
    assert lib.dbhip_slab_table_reset(fake, ws - 256, B, P, None) == EWORKSPACE
    # insert
    assert ins(keys=None) == EINVAL and ins(vals=None) == EINVAL
    assert ins(b=0) == EINVAL and ins(b=M32, p=1, wb=1 << 44) == EINVAL
    assert ins(hash_=(13, 24, 0)) == EINVAL
    assert ins(hash_=(1 << 32, 24, 343)) == EINVAL and ins(hash_=(13, 1 << 32, 343)) == EINVAL
    assert ins(hash_=(13, 24, 1 << 32)) == EINVAL
    assert ins(w=None) == EWORKSPACE and ins(w=fake + 64) == EWORKSPACE and ins(wb=ws - 1) == EWORKSPACE
    assert ins(n=0, keys=None, vals=None) == 0  # nothing to insert: no launch, no device needed

    # lookup and join probe
    def look(keys=fake, n=16, w=fake, b=B, p=P, hash_=h, vals=fake, found=fake):
        return lib.dbhip_slab_table_lookup_u32(keys, n, w, b, p, *hash_, vals, found, None)
    assert look(keys=None) == EINVAL and look(w=None) == EINVAL
    assert look(vals=None) == EINVAL and look(found=None) == EINVAL
    assert look(b=0) == EINVAL and look(hash_=(1, 2, 0)) == EINVAL and look(b=M32, p=1) == EINVAL

    def jp(keys=fake, pv=fake, w=fake, b=B, hash_=h, o=(fake, fake, fake)):
        return lib.dbhip_slab_table_join_probe_u32(keys, pv, 16, w, b, P, *hash_, *o, None)
    assert jp(keys=None) == EINVAL and jp(pv=None) == EINVAL and jp(w=None) == EINVAL
    assert jp(o=(None, fake, fake)) == EINVAL and jp(o=(fake, None, fake)) == EINVAL and jp(o=(fake, fake, None)) == EINVAL
    assert jp(b=0) == EINVAL and jp(hash_=(1, 2, 0)) == EINVAL
    # export
    exp = lib.dbhip_slab_table_export_u32
    assert exp(None, B, P, fake, fake, fake, fake, None) == EINVAL
    assert exp(fake, B, P, None, fake, fake, fake, None) == EINVAL
    assert exp(fake, B, P, fake, None, fake, fake, None) == EINVAL
    assert exp(fake, B, P, fake, fake, None, fake, None) == EINVAL
    assert exp(fake, B, P, fake, fake, fake, None, None) == EINVAL
    assert exp(fake, 0, P, fake, fake, fake, fake, None) == EINVAL
    assert exp(fake, M32, 1, fake, fake, fake, fake, None) == EINVAL


def test_code_object_has_no_scratch_and_no_64_bit_division(tmp_path):
    """no slab kernel spills to scratch; the bucket hash is mulhi-based: no call to a 64-bit division routine"""
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--save-temps", "-c", str(ROOT / "dwarf_bench_amd" / "csrc" / "slab.hip"), "-o", str(tmp_path / "sl.o")],
                   check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "slab-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    bodies = dict(re.findall(r"^(_ZN\S*sl_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M))
    assert len(bodies) == 4, sorted(bodies)  # insert, lookup, join probe, export
    insert = next(b for name, b in bodies.items() if "sl_insert_kernel" in name)
    assert "global_atomic_cmpswap " in insert and "global_atomic_add_x2" in insert  # slot / link CAS, pool cursor
    meta = re.findall(r"\.name:\s+(_ZN\S*sl_\w+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 4 and all(size == "0" for _, size in meta), meta
    text = "".join(bodies.values())
    assert "scratch_" not in text and "__udivdi3" not in text and "__umoddi3" not in text


def test_slab_buckets_is_the_reference_sizing_without_its_zero():
    from dwarf_bench_amd import ops
    assert [ops.slab_buckets(n) for n in (0, 1, 19, 20, 39, 40, 1 << 24)] == [1, 1, 1, 1, 1, 2, (1 << 24) // 20]
    assert int((1 << 24) / (32 * 0.625)) == ops.slab_buckets(1 << 24)  # calculate_buckets_count(n, 60)
