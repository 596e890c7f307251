"""The cuckoo table without a GPU: the Python model against the reference tests' assertions, the C ABI's workspace
query and argument checks (host-side, before any HIP call), and the compiled code object of csrc/cuckoo.hip."""
import json
import re
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE
from tests.cuckoo_model import EMPTY_KEY, CuckooModel

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def kats(golden_dir):
    return json.loads((golden_dir / "cuckoo_kats.json").read_text())


def _run_case(case):
    m = CuckooModel(case["table_size"], case["hash_kind"], case["seeds"])
    results = [m.insert(k, v, case["max_iter"]) for k, v in case["inserts"]]
    return m, results


def test_model_reproduces_every_reference_assertion(kats):
    assert kats["empty_key"] == EMPTY_KEY
    assert [c["name"] for c in kats["cases"]] == ["insert", "at", "fails_to_insert", "parallel_insertion"]
    for case in kats["cases"]:
        m, results = _run_case(case)
        a = case["asserted"]
        if "keys_present_count" in a:
            want = a["keys_present_count"]
            assert sum(k in want["keys"] for k in m.keys) == want["count"], case["name"]
        if "insert_results" in a:
            assert [int(r) for r in results] == a["insert_results"], case["name"]
        for key, val, found in a.get("lookups", []):
            got_val, got_found = m.at(key)
            assert got_found == found, (case["name"], key)
            if val is not None:
                assert got_val == val, (case["name"], key)
        # the serial layouts recorded beside the assertions are the model's
        d = case["derived"]
        assert [int(r) for r in results] == d["insert_results"], case["name"]
        slots = d.get("slots", d.get("slots_if_serial"))
        assert {int(s): tuple(kv) for s, kv in slots.items()} == m.layout(), case["name"]


def test_fails_to_insert_drops_the_carried_key_after_an_even_number_of_swaps(kats):
    """h1 == h2 (offsets 0, 0): 20 and 0 bounce in place size = 16 times and the original occupants end where they were"""
    case = next(c for c in kats["cases"] if c["name"] == "fails_to_insert")
    m, _ = _run_case(case)
    assert m.at(20) == (None, False) and m.at(0) == (None, False) and m.at(16) == (16, True) and m.at(4) == (4, True)


def test_workspace_query():
    lib = _capi.lib()
    assert lib.dbhip_cuckoo_table_workspace_bytes(0) == 0
    for size in (1, 7, 10, 1000, 1 << 24, (1 << 32) - 1):
        ws = lib.dbhip_cuckoo_table_workspace_bytes(size)
        assert ws >= 256 + 8 * size and ws % 256 == 0, size


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20  # a 256-aligned address that is never dereferenced: every call below fails on the host first
    size = 1024
    ws = lib.dbhip_cuckoo_table_workspace_bytes(size)
    too_big = 1 << 32

    def ins(keys=fake, vals=fake, n=16, w=fake, wb=ws, ts=size, kind=1, max_iter=0, out=None):
        return lib.dbhip_cuckoo_table_insert_u32(keys, vals, n, w, wb, ts, kind, 1, 2, max_iter, 0, out, None)

    # reset
    assert lib.dbhip_cuckoo_table_reset(fake, ws, 0, None) == EINVAL
    assert lib.dbhip_cuckoo_table_reset(fake, 1 << 40, too_big, None) == EINVAL
    assert lib.dbhip_cuckoo_table_reset(None, ws, size, None) == EWORKSPACE
    assert lib.dbhip_cuckoo_table_reset(fake + 8, ws, size, None) == EWORKSPACE
    assert lib.dbhip_cuckoo_table_reset(fake, ws - 256, size, None) == EWORKSPACE
    # insert
    assert ins(keys=None) == EINVAL
    assert ins(vals=None) == EINVAL
    assert ins(kind=3) == EINVAL and ins(kind=-1) == EINVAL
    assert ins(ts=0) == EINVAL and ins(ts=too_big, wb=1 << 40) == EINVAL
    assert ins(max_iter=(1 << 20) + 1) == EINVAL
    assert ins(max_iter=0xFFFFFFFF) == EINVAL
    assert ins(w=None) == EWORKSPACE and ins(w=fake + 64) == EWORKSPACE and ins(wb=ws - 1) == EWORKSPACE
    assert ins(n=0, keys=None, vals=None) == 0  # nothing to insert: no launch, no device needed
    # lookup
    def look(keys=fake, n=16, w=fake, ts=size, kind=1, vals=fake, found=fake):
        return lib.dbhip_cuckoo_table_lookup_u32(keys, n, w, ts, kind, 1, 2, vals, found, None)
    assert look(keys=None) == EINVAL and look(w=None) == EINVAL
    assert look(vals=None) == EINVAL and look(found=None) == EINVAL
    assert look(kind=3) == EINVAL and look(ts=0) == EINVAL and look(ts=too_big) == EINVAL
    # export
    assert lib.dbhip_cuckoo_table_export_u32(None, size, fake, fake, None) == EINVAL
    assert lib.dbhip_cuckoo_table_export_u32(fake, size, None, fake, None) == EINVAL
    assert lib.dbhip_cuckoo_table_export_u32(fake, size, fake, None, None) == EINVAL
    assert lib.dbhip_cuckoo_table_export_u32(fake, 0, fake, fake, None) == EINVAL
    assert lib.dbhip_cuckoo_table_export_u32(fake, too_big, fake, fake, None) == EINVAL


def test_code_object_swaps_with_one_atomic_and_has_no_scratch(tmp_path):
    """the insert kernel moves a pair with global_atomic_swap_x2 (not a CAS loop); no cuckoo kernel spills to scratch"""
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--save-temps", "-c", str(ROOT / "dwarf_bench_amd" / "csrc" / "cuckoo.hip"), "-o", str(tmp_path / "ck.o")],
                   check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "cuckoo-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    bodies = dict(re.findall(r"^(_ZN\S*ck_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M))
    assert len(bodies) == 4, sorted(bodies)  # insert, lookup, reset, export
    insert = next(b for name, b in bodies.items() if "ck_insert_kernel" in name)
    assert "global_atomic_swap_x2" in insert and "cmpswap" not in insert
    meta = re.findall(r"\.name:\s+(_ZN\S*ck_\w+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 4 and all(size == "0" for _, size in meta), meta
    assert "scratch_" not in "".join(bodies.values())


def test_vectorised_murmur_matches_the_oracle():
    import numpy as np
    from oracle import pyoracle as po
    from tests.cuckoo_model import mix64_np, murmur3_x86_32_np
    keys = np.array([0, 1, 2, 5, 258, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    for seed in (0, 1, 421, 0xDEADBEEF):
        assert murmur3_x86_32_np(keys, seed).tolist() == [po.murmur3_x86_32(int(k), seed) for k in keys]
        assert mix64_np(seed, keys).tolist() == [po.mix64(seed, int(k)) for k in keys]


def test_the_reference_hasher_pair_comes_in_swapped_pairs():
    """Why the dwarf does not hash with two Murmur3 seeds (hash_kind 1): Murmur3 of a 4-byte key is F(seed ^ f(k)), so the
    key k' with f(k') = f(k) ^ seed1 ^ seed2 lands on the two positions of k, swapped.  Here f is inverted on the host."""
    import numpy as np
    from tests.cuckoo_model import murmur3_x86_32_np

    def f(k):  # the key's block scramble (hashfunctions.hpp:100-104)
        k = (k * 0xcc9e2d51) & 0xFFFFFFFF
        k = ((k << 15) | (k >> 17)) & 0xFFFFFFFF
        return (k * 0x1b873593) & 0xFFFFFFFF

    def f_inv(x):
        x = (x * pow(0x1b873593, -1, 1 << 32)) & 0xFFFFFFFF
        x = ((x >> 15) | (x << 17)) & 0xFFFFFFFF
        return (x * pow(0xcc9e2d51, -1, 1 << 32)) & 0xFFFFFFFF

    s1, s2 = 0x1234567, 0x89ABCDE
    for k in (1, 77, 123456, 0xFFFFFFF0):
        k2 = f_inv(f(k) ^ s1 ^ s2)
        assert k2 != k
        h = lambda key, s: int(murmur3_x86_32_np(np.array([key], dtype=np.uint32), s)[0])
        assert (h(k2, s1), h(k2, s2)) == (h(k, s2), h(k, s1))


def test_seed_pairs_are_deterministic_and_distinct():
    """ops.cuckoo_seed_pair: the sequence the rebuild loop walks (the dwarf restates it in C++)"""
    from dwarf_bench_amd import ops
    pairs = [ops.cuckoo_seed_pair(0, a) for a in range(64)]
    assert pairs == [ops.cuckoo_seed_pair(0, a) for a in range(64)]
    assert all(s1 != s2 and 0 <= s1 < 1 << 32 and 0 <= s2 < 1 << 32 for s1, s2 in pairs)
    assert len(set(pairs)) == 64 and ops.cuckoo_seed_pair(1, 0) != pairs[0]
