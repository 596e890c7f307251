"""Scan, dense scan, prefix sum, radix sort, sort-pairs / argsort, dense group-by, reduce, nested-loop join, gather, the
partition step of the multi-GPU join, the bitmask and cuckoo tables and the validators write only their own buffers.

Every other parity test compares the first n words of a result with the oracle; torch's allocator rounds every block
to 512 bytes, so a stray word BEHIND a buffer lands in slack and is never seen.  Here every buffer a call writes has
exactly the size the call is entitled to and sits between guard words in one allocation (tests/guard_testlib.py), every
input column is frozen, and every case runs under two guard fills: a kernel that reads past the end of an input and uses
what it read gives two answers.  After every call: the status word, the oracle's (or numpy's) answer, every guard,
every input.  The calls go through the C ABI with raw pointers, as ops.py makes them.

Entry point -> test (every buffer it writes behind guards, every column it reads frozen):
  dbhip_copy_if_lt_i32, dbhip_copy_if_lt_dense_i32       test_scan_writes_its_matches_and_nothing_else, test_scan_seeded_sweep,
                                                         test_scan_with_more_chunks_than_compute_units_and_several_tiles_per_chunk
  dbhip_exclusive_scan_u32                               test_exclusive_scan_writes_n_words, test_exclusive_scan_seeded_sweep
  dbhip_radix_sort_u32 / _i32                            test_radix_sort_stays_inside_keys_tmp_and_workspace, test_sorts_seeded_sweep
  dbhip_radix_sort_pairs_u32 / _i32                      test_sort_pairs_and_argsort_stay_inside_their_four_columns, test_sorts_seeded_sweep
  dbhip_groupby_sum_u32, _partial_u32, _merge_u32        test_groupby_writes_groups_words_and_its_workspace,
                                                         test_groupby_packed_and_wide_tables_pinned, test_groupby_seeded_sweep
  dbhip_reduce_sum_i32                                   test_reduce_writes_one_word
  dbhip_nested_join_u32                                  test_nested_join_writes_its_cell_matrices
  dbhip_gather_u32                                       test_gather_writes_n_words
  dbhip_pjoin_partition_u32                              test_pjoin_partition_writes_n_pairs_and_parts_counts
  dbhip_bitmask_table_reset / _insert_u32 / _lookup_u32  test_bitmask_table_stays_inside_its_workspace
  dbhip_cuckoo_table_reset / _insert / _lookup / _export test_cuckoo_table_stays_inside_its_workspace
  dbhip_check_* (all ten, dbhip_check_pjoin_route_u32 too) test_validators_write_their_result_words_only
  dbhip_gen_uniform_u32 / _at_u32 / _unique_sorted_u32   test_generators_write_n_words
Left out on purpose: dbhip_join_*, dbhip_ujoin_*, dbhip_groupby_hash_u32 and dbhip_slab_table_* (guarded by
join_testlib, test_gpu_groupby_hash*.py and test_gpu_slab.py); dbhip_version, dbhip_device_info, dbhip_workspace_status,
dbhip_radix_sort_rank_mode and dbhip_radix_sort_prepare write no device buffer of the caller's.

Scan: neither copy_if variant writes out[out_size, n) (scan_move_kernel and flush_strip store exactly the matches), so
those words are checked to keep the fill as well.

At the end: the packed group-by, chosen by its own sample, on columns whose unsampled rows break the sample's
prediction (groupby.hip's header promises exact sums through the saturated counters' global path)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from tests import guard_testlib as gt
from tests import validator_model as vm
from tests.cuckoo_model import mix64_np, positions_np
from tests.guard_testlib import FILLS, ptr
from tests.pjoin_testlib import dest_of, fmix32

pytestmark = pytest.mark.gpu
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
DEV_KEY_RANGE = 2


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _status(ws):
    st = C.c_uint32(0xFFFFFFFF)
    assert _lib().dbhip_workspace_status(ptr(ws), C.byref(st), _stream()) == 0
    return st.value


def _words(t):
    """device uint64 result words as Python ints"""
    torch.cuda.synchronize()
    return [int(x) & M64 for x in t.cpu().tolist()]


def _check(w, what):
    """every guard intact, every input unchanged; a failure names the case"""
    torch.cuda.synchronize()
    try:
        w.check()
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _same(got, want_dev, what):
    assert got.numel() == want_dev.numel(), what
    bad = torch.nonzero(got != want_dev)
    assert bad.numel() == 0, f"{what}: {bad.numel()} words differ from the oracle, the first at {int(bad[0])}"


def _sweep_size(rng, draw, hi_log2, edges):
    """two draws in three log-uniform as they fall; every third one a path boundary, and only that one, +-3 rows"""
    if draw % 3:
        return max(1, int(2 ** rng.uniform(0, hi_log2)))
    return max(1, int(rng.choice(edges)) + int(rng.integers(-3, 4)))


# ---- scan / compaction -------------------------------------------------------------------------------------------------
SCAN_ENTRIES = ("dbhip_copy_if_lt_i32", "dbhip_copy_if_lt_dense_i32")
SCAN_SIZES = [1, 3, 63, 64, 65, 4095, 4097, 8191, 8193, 32767, 32769, 100003, (1 << 20) + 5, (1 << 22) + 12345]
SCAN_CHUNK = 32768  # the dense path's chunk and the two-launch path's tile (its chunk, below 2^26 rows)


def _scan_once(entry, dsrc, filt, so, oo, fill, want_dev, what):
    lib, n = _lib(), dsrc.numel()
    w = gt.Watch(fill)
    src = w.col(n, so, data=dsrc, freeze=True)
    out = w.col(n, oo)
    size = w.u64(1)
    nbytes = lib.dbhip_copy_if_lt_i32_workspace_bytes(n)
    ws = w.ws(nbytes)
    rc = getattr(lib, entry)(ptr(src), n, filt, ptr(out), ptr(size), ptr(ws), nbytes, _stream())
    assert rc == 0, (what, rc)
    assert _status(ws) == 0, what
    m = int(size.item())
    assert m == want_dev.numel(), (what, m, want_dev.numel())
    _same(out[:m], want_dev, what)
    # out[out_size, n) is the callee's by the contract ("room for n elements"), but neither variant writes there
    assert bool((out[m:] == gt.i32(fill)).all()), f"{what}: wrote into out[out_size, n)"
    _check(w, what)


def _scan_cases(n, seed):
    """(label, column, filter): the reference's values in [1, 10000] under filters that pass 0 %, 0.04 %, 50 % and 100 %,
    and every match in the last / the first chunk.  As int32 one fill word passes every filter, the other none."""
    base = po.gen_uniform_u32(n, seed, 1, 10000).view(np.int32)
    cases = [(f"filter {f}", base, f) for f in (1, 5, 5001, 10001)]
    last0 = (n - 1) // SCAN_CHUNK * SCAN_CHUNK
    tail = np.full(n, 9999, np.int32)
    tail[last0:] = base[last0:]
    head = np.full(n, 9999, np.int32)
    head[:SCAN_CHUNK] = base[:SCAN_CHUNK]
    return cases + [("matches in the last chunk", tail, 5001), ("matches in the first chunk", head, 5001)]


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("entry", SCAN_ENTRIES)
def test_scan_writes_its_matches_and_nothing_else(entry, n):
    """src at offsets 0..3 words x out at offsets 0..3 words: flush_strip takes its shift, scan_move_kernel its head,
    from the destination's ADDRESS"""
    for label, host, filt in _scan_cases(n, 42):
        dsrc, want = _dev(host), _dev(po.copy_if_lt(host, filt))
        for so in range(4):
            for oo in range(4):
                for fill in FILLS:
                    _scan_once(entry, dsrc, filt, so, oo, fill, want, (entry, n, label, so, oo, hex(fill)))


# The two-launch path above 2^22 rows (scan.hip chunk_layout, launch_chunked): more chunks than compute units from 2^23
# rows, so a workgroup walks several chunks in its grid-stride loop; from 2^26 rows a chunk holds tiles / 1024 tiles (2,
# then up to 8 at the headline's 2^28), the chunk kernel alternates its two register tiles and carries `running` from
# tile to tile, and the move kernel copies up to 262144 words per chunk.  Thinned to keep three 1 GiB columns per call
# cheap: one misaligned (src, out) pair and the aligned one, a sparse and a dense filter, both fills.
SCAN_LARGE_SIZES = [(1 << 23) + 5, (1 << 26) + 12345, (1 << 28) + 5]


def test_scan_large_sizes_restate_the_chunk_layout():
    """the sizes above reach the paths they are there for, by chunk_layout's own arithmetic (256 compute units)"""
    def layout(n):
        tiles = -(-n // 32768)
        tpc = min(max(tiles // 1024, 1), 8)
        return tpc, -(-n // (tpc * 32768))
    assert [layout(n)[0] for n in SCAN_LARGE_SIZES] == [1, 2, 8]
    assert all(layout(n)[1] > 256 for n in SCAN_LARGE_SIZES) and layout(SCAN_SIZES[-1])[1] <= 256
    assert all(n % 32768 and n % 4 for n in SCAN_LARGE_SIZES)  # a ragged last tile, a ragged last vector


@pytest.mark.parametrize("n", SCAN_LARGE_SIZES)
@pytest.mark.parametrize("entry", SCAN_ENTRIES)
def test_scan_with_more_chunks_than_compute_units_and_several_tiles_per_chunk(entry, n):
    host = po.gen_uniform_u32(n, 42, 1, 10000).view(np.int32)
    dsrc = _dev(host)
    for filt in (5, 5001):
        want = _dev(po.copy_if_lt(host, filt))
        for so, oo in ((1, 3), (0, 0)):
            for fill in FILLS:
                _scan_once(entry, dsrc, filt, so, oo, fill, want, (entry, n, filt, so, oo, hex(fill)))


def test_scan_seeded_sweep():
    rng = np.random.default_rng(201)
    for draw in range(30):
        n = _sweep_size(rng, draw, 22, [4096, 8192, 32768, 1 << 16, 1 << 20])
        filt = int(rng.choice([-5, 1, 5, 101, 5001, 10001]))
        so, oo = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        host = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 1, 10000).view(np.int32)
        dsrc, want = _dev(host), _dev(po.copy_if_lt(host, filt))
        for entry in SCAN_ENTRIES:
            for fill in FILLS:
                _scan_once(entry, dsrc, filt, so, oo, fill, want, ("draw", draw, entry, n, filt, so, oo, hex(fill)))


# ---- exclusive prefix sum ----------------------------------------------------------------------------------------------
XS_SIZES = [1, 3, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769, (1 << 22) + 5]
XS_PLACES = [(0, 0, False), (0, 1, False), (3, 0, False), (2, 2, False), (0, 0, True), (3, 3, True)]  # (src, dst, in place)


def _xscan_want(host, init):
    exp = np.zeros(host.size, dtype=np.uint64)
    np.cumsum(host[:-1], dtype=np.uint64, out=exp[1:])
    return ((exp + np.uint64(init)) & np.uint64(M32)).astype(np.uint32)


def _xscan_once(dsrc, init, so, do, in_place, fill, want_dev, what):
    lib, n = _lib(), dsrc.numel()
    w = gt.Watch(fill)
    src = w.col(n, so, data=dsrc, freeze=not in_place)
    dst = src if in_place else w.col(n, do)
    nbytes = lib.dbhip_exclusive_scan_u32_workspace_bytes(n)
    ws = w.ws(nbytes)
    rc = lib.dbhip_exclusive_scan_u32(ptr(src), n, init, ptr(dst), ptr(ws), nbytes, _stream())
    assert rc == 0, (what, rc)
    assert _status(ws) == 0, what
    _same(dst, want_dev, what)
    _check(w, what)


@pytest.mark.parametrize("n", XS_SIZES)
def test_exclusive_scan_writes_n_words(n):
    """one launch when src and dst are both 16-byte aligned, three otherwise (xscan.hip: src | dst); dst at an offset
    of its own; in place"""
    host = po.gen_uniform_u32(n, 3, 0, M32)  # wrap-around sums; a fill word read as input changes every later sum
    dsrc = _dev(host)
    for init in (77, 0xFFFFFF00):
        want = _dev(_xscan_want(host, init))
        for so, do, in_place in XS_PLACES:
            for fill in FILLS:
                _xscan_once(dsrc, init, so, do, in_place, fill, want, ("xscan", n, init, so, do, in_place, hex(fill)))


def test_exclusive_scan_seeded_sweep():
    rng = np.random.default_rng(202)
    for draw in range(30):
        n = _sweep_size(rng, draw, 22, [1024, 4096, 32768, 1 << 16, 1 << 20])
        so, do, in_place = int(rng.integers(0, 4)), int(rng.integers(0, 4)), bool(rng.integers(0, 4) == 0)
        init = int(rng.integers(0, 1 << 32))
        host = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, M32)
        dsrc, want = _dev(host), _dev(_xscan_want(host, init))
        for fill in FILLS:
            _xscan_once(dsrc, init, so, so if in_place else do, in_place, fill, want,
                        ("draw", draw, n, init, so, do, in_place, hex(fill)))


# ---- radix sort, sort-pairs, argsort -----------------------------------------------------------------------------------
# one tile (<= 8192 keys: one workgroup), the scatter that sums its own prefix (<= 32 chunks), the chunk scan kernel, and
# 2897 tiles: the first count at which 8-bit chunks hold two tiles (radix.hip rs_geometry), so the last chunk is short
SORT_SIZES = [1, 2, 4095, 4097, 8191, 8192, 8193, 100003, (1 << 20) + 777, 2897 * 8192 + 5]


def _sort_column(n, kind, seed=7):
    if kind == "full range":
        return po.gen_uniform_u32(n, seed, 0, M32)
    return po.gen_uniform_u32(n, seed, 1, 10000)  # upper digits constant: skipped passes, the result ends in either buffer


def _order(keys, signed):
    return keys.view(np.int32) if signed else keys


def _sort_once(dkeys, bits, signed, fill, want_dev, what):
    lib, n = _lib(), dkeys.numel()
    w = gt.Watch(fill)
    keys, tmp = w.col(n, 0, data=dkeys), w.col(n, 0)
    nbytes = lib.dbhip_radix_sort_workspace_bytes(n, bits)
    ws = w.ws(nbytes)
    fn = lib.dbhip_radix_sort_i32 if signed else lib.dbhip_radix_sort_u32
    rc = fn(ptr(keys), ptr(tmp), n, bits, ptr(ws), nbytes, _stream())
    assert rc == 0, (what, rc)
    assert _status(ws) == 0, what
    _same(keys, want_dev, what)
    _check(w, what)


def _pairs_once(dkeys, dvals, bits, signed, fill, want_keys, want_vals, what):
    """dvals None: the argsort — vals starts out holding the fill and is never read"""
    lib, n = _lib(), dkeys.numel()
    w = gt.Watch(fill)
    keys, vals = w.col(n, 0, data=dkeys), w.col(n, 0, data=dvals)
    tmp_keys, tmp_vals = w.col(n, 0), w.col(n, 0)
    nbytes = lib.dbhip_radix_sort_pairs_workspace_bytes(n, bits)
    ws = w.ws(nbytes)
    fn = lib.dbhip_radix_sort_pairs_i32 if signed else lib.dbhip_radix_sort_pairs_u32
    rc = fn(ptr(keys), ptr(vals), ptr(tmp_keys), ptr(tmp_vals), n, bits, int(dvals is None), ptr(ws), nbytes, _stream())
    assert rc == 0, (what, rc)
    assert _status(ws) == 0, what
    _same(keys, want_keys, what + ("keys",))
    _same(vals, want_vals, what + ("vals",))
    _check(w, what)


@pytest.mark.parametrize("n", SORT_SIZES)
def test_radix_sort_stays_inside_keys_tmp_and_workspace(n):
    for kind in ("full range", "1..10000"):
        host = _sort_column(n, kind)
        dkeys = _dev(host)
        for signed in (False, True):
            want = _dev(np.sort(_order(host, signed)))
            for bits in (4, 8):
                for fill in FILLS:
                    _sort_once(dkeys, bits, signed, fill, want, ("sort", n, kind, signed, bits, hex(fill)))


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_pairs_and_argsort_stay_inside_their_four_columns(n):
    for kind in ("full range", "1..10000"):
        host, hvals = _sort_column(n, kind), po.gen_uniform_u32(n, 9, 0, M32)
        dkeys, dvals = _dev(host), _dev(hvals)
        for signed in (False, True):
            perm = np.argsort(_order(host, signed), kind="stable")
            want_keys, want_vals, want_perm = _dev(host[perm]), _dev(hvals[perm]), _dev(perm.astype(np.uint32))
            for bits in (4, 8):
                for fill in FILLS:
                    what = ("pairs", n, kind, signed, bits, hex(fill))
                    _pairs_once(dkeys, dvals, bits, signed, fill, want_keys, want_vals, what)
                    _pairs_once(dkeys, None, bits, signed, fill, want_keys, want_perm, ("argsort",) + what[1:])
    # all keys equal: no pass runs; vals (pre-filled with the fill) must still become 0..n-1, keys stay, nothing else
    # is written
    same = torch.full((n,), 0x01234567, dtype=torch.int32, device="cuda")
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    for signed in (False, True):
        for bits in (4, 8):
            for fill in FILLS:
                _pairs_once(same, None, bits, signed, fill, same, ids, ("argsort of equal keys", n, signed, bits, hex(fill)))


def test_sorts_seeded_sweep():
    rng = np.random.default_rng(203)
    for draw in range(30):
        n = _sweep_size(rng, draw, 21, [4096, 8192, 1 << 16, 1 << 18, 1 << 20])
        bits, signed = int(rng.choice([4, 8])), bool(rng.integers(0, 2))
        kind = ("full range", "1..10000")[int(rng.integers(0, 2))]
        host = _sort_column(n, kind, int(rng.integers(1, 1 << 30)))
        hvals = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, M32)
        perm = np.argsort(_order(host, signed), kind="stable")
        dkeys, want_keys = _dev(host), _dev(host[perm])
        for fill in FILLS:
            what = ("draw", draw, n, kind, signed, bits, hex(fill))
            _sort_once(dkeys, bits, signed, fill, want_keys, what)
            _pairs_once(dkeys, _dev(hvals), bits, signed, fill, want_keys, _dev(hvals[perm]), what + ("pairs",))
            _pairs_once(dkeys, None, bits, signed, fill, want_keys, _dev(perm.astype(np.uint32)), what + ("argsort",))


# ---- dense group-by ----------------------------------------------------------------------------------------------------
GB_GROUPS = [1, 7, 64, 257, 32767, 32768, 32769, 65535, 65536, 65537, 200001]
GB_SIZES = [1, 5, 8191, 8193, 100003, (1 << 20) + 3]
GB_TABLES = (None, 0, 1, 3)  # None: the fused call; else max_private_tables of partial + merge


def _groupby_once(dk, dv, groups, tables, out_off, fill, want_dev, what, want_status=0, want_mode=None):
    lib, n = _lib(), dk.numel()
    w = gt.Watch(fill)
    keys, vals = w.col(n, 0, data=dk, freeze=True), w.col(n, 0, data=dv, freeze=True)
    out = w.col(groups, out_off)
    nbytes = lib.dbhip_groupby_sum_u32_workspace_bytes(n, groups)
    ws = w.ws(nbytes)
    if tables is None:
        rc = lib.dbhip_groupby_sum_u32(ptr(keys), ptr(vals), n, groups, ptr(out), ptr(ws), nbytes, _stream())
    else:
        rc = lib.dbhip_groupby_partial_u32(ptr(keys), ptr(vals), n, groups, tables, ptr(ws), nbytes, _stream())
        assert rc == 0, (what, rc)
        rc = lib.dbhip_groupby_merge_u32(groups, tables, ptr(out), ptr(ws), _stream())
    assert rc == 0, (what, rc)
    assert _status(ws) == want_status, (what, _status(ws))
    if want_mode is not None and groups > 32768:  # the header word gb_aggregate_big_kernel writes: 1 packed, 2 wide
        assert int(ws[4:8].view(torch.int32).item()) == want_mode, what
    _same(out, want_dev, what)
    _check(w, what)


def _groupby_sweep(groups_list=GB_GROUPS, want_mode=None, label="chosen"):
    """keys uniform over the groups, so both fill words (above every group count here) would raise DBHIP_DEV_KEY_RANGE
    if a guard were read as a key; values alternate between the reference's [1, 10000] and the full range"""
    case = 0
    for groups in groups_list:
        for n in GB_SIZES:
            keys = po.gen_uniform_u32(n, 42, 0, groups - 1)
            vals = po.gen_uniform_u32(n, 43, 1, 10000) if case % 2 == 0 else po.gen_uniform_u32(n, 43, 0, M32)
            dk, dv, want = _dev(keys), _dev(vals), _dev(po.groupby_sum(keys, vals, groups))
            for tables in GB_TABLES:
                for fill in FILLS:
                    case += 1
                    _groupby_once(dk, dv, groups, tables, case % 4, fill, want,
                                  ("groupby", label, groups, n, tables, case % 4, hex(fill)), want_mode=want_mode)
        # one key out of range: flagged, ignored, the other groups still right, nothing written elsewhere
        n = 100003
        keys, vals = po.gen_uniform_u32(n, 44, 0, groups - 1), po.gen_uniform_u32(n, 45, 1, 10000)
        keys[n // 2] = groups
        inside = keys < groups
        want = _dev(po.groupby_sum(keys[inside], vals[inside], groups))
        for tables in (None, 1):
            for fill in FILLS:
                _groupby_once(_dev(keys), _dev(vals), groups, tables, 0, fill, want,
                              ("groupby, one key out of range", label, groups, tables, hex(fill)),
                              want_status=DEV_KEY_RANGE, want_mode=want_mode)
    return case


def test_groupby_writes_groups_words_and_its_workspace():
    _groupby_sweep()


@pytest.mark.parametrize("mode,want_mode", [("force", 1), ("0", 2)])
def test_groupby_packed_and_wide_tables_pinned(mode, want_mode):
    """DBHIP_GB_PACKED=force / 0 pins the packed / the wide layout of the tables above 32768 groups (a fresh process:
    the library reads the variable once); one workspace size serves both layouts.
    A child that hangs, aborts or faults does NOT fail this test like any other: pytest.exit ends the whole session with
    return code 3 and no summary of the tests that had not run, because after a fault or a hang on the GPU nothing more
    is to be started on it."""
    prog = ("from tests import test_gpu_buffer_bounds as t\n"
            f"cases = t._groupby_sweep([g for g in t.GB_GROUPS if g > 32768], {want_mode}, 'DBHIP_GB_PACKED={mode}')\n"
            "print('bounds: ok', cases)\n")
    try:
        r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=900,
                           env={**os.environ, "DBHIP_GB_PACKED": mode}, cwd=os.path.dirname(os.path.dirname(__file__)))
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on it
        pytest.exit(f"the group-by child process ({mode}) hung: {e}", returncode=3)
    if r.returncode in (-6, -11, 134, 139):  # an abort or a fault on the GPU: nothing more is started on it
        pytest.exit(f"the group-by child process ({mode}) died with {r.returncode}: {r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0 and "bounds: ok" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-3000:])


def test_groupby_seeded_sweep():
    rng = np.random.default_rng(204)
    for draw in range(30):
        n = _sweep_size(rng, draw, 21, [8192, 1 << 16, 1 << 20])
        groups = int(rng.choice([1, 2, 3, 20, 64, 1000, 4096, 32768, 32769, 65536, 70001, 200000]))
        tables = (None, 0, 1, 3, 7)[int(rng.integers(0, 5))]
        keys = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, groups - 1)
        if rng.integers(0, 3) == 0:
            keys[:] = keys[0]  # one hot group
        vals = po.gen_uniform_u32(n, int(rng.integers(1, 1 << 30)), 0, int(rng.choice([1, 10000, M32])))
        want = _dev(po.groupby_sum(keys, vals, groups))
        for fill in FILLS:
            _groupby_once(_dev(keys), _dev(vals), groups, tables, draw % 4, fill, want,
                          ("draw", draw, n, groups, tables, hex(fill)))


# ---- reduce, nested-loop join ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 511, 16385, 300011])
def test_reduce_writes_one_word(n):
    host = po.gen_uniform_u32(n, 8, 0, M32).view(np.int32)  # wraps; either fill word read as input changes the sum
    want, dsrc = po.reduce_sum(host), _dev(host)
    for so in range(4):
        for fill in FILLS:
            what = ("reduce", n, so, hex(fill))
            w = gt.Watch(fill)
            src, out = w.col(n, so, data=dsrc, freeze=True), w.col(1, (so + 1) % 4)
            assert _lib().dbhip_reduce_sum_i32(ptr(src), n, ptr(out), _stream()) == 0, what
            assert int(out.item()) == want, what
            _check(w, what)


@pytest.mark.parametrize("na,nb", [(1, 1), (17, 257), (1000, 333)])
def test_nested_join_writes_its_cell_matrices(na, nb):
    ak, av = po.gen_uniform_u32(na, 1, 1, 50), po.gen_uniform_u32(na, 2, 0, M32)
    bk, bv = po.gen_uniform_u32(nb, 3, 1, 50), po.gen_uniform_u32(nb, 4, 0, M32)
    want = [_dev(c.reshape(-1)) for c in po.nested_join(ak, av, bk, bv)]
    for fill in FILLS:
        what = ("nested join", na, nb, hex(fill))
        w = gt.Watch(fill)
        ins = [w.col(len(a), i, data=a, freeze=True) for i, a in enumerate((ak, av, bk, bv))]
        outs = [w.col(na * nb, i) for i in (0, 1, 3)]
        rc = _lib().dbhip_nested_join_u32(*(ptr(t) for t in ins), na, nb, *(ptr(t) for t in outs), _stream())
        assert rc == 0, what
        for got, exp in zip(outs, want):
            _same(got, exp, what)
        _check(w, what)


# ---- gather and the partition step of the multi-GPU join ---------------------------------------------------------------
PJ_PARTS = [1, 3, 8, 256, 1024]
PJ_SIZES = [1, 5, 100003, (1 << 20) + 1]


@pytest.mark.parametrize("n", PJ_SIZES)
def test_gather_writes_n_words(n):
    for table_rows in (1, 1000, n + 7):
        table = po.gen_uniform_u32(table_rows, 5, 0, M32)
        idx = po.gen_uniform_u32(n, 6, 0, table_rows - 1)
        want = _dev(table[idx])
        for off, fill in enumerate(FILLS):
            what = ("gather", n, table_rows, hex(fill))
            w = gt.Watch(fill)
            t, i = w.col(table_rows, off, data=table, freeze=True), w.col(n, off + 1, data=idx, freeze=True)
            out = w.col(n, off + 2)
            assert _lib().dbhip_gather_u32(ptr(t), ptr(i), n, ptr(out), _stream()) == 0, what
            _same(out, want, what)
            _check(w, what)


@pytest.mark.parametrize("n", PJ_SIZES)
@pytest.mark.parametrize("parts", PJ_PARTS)
def test_pjoin_partition_writes_n_pairs_and_parts_counts(parts, n):
    lib, first = _lib(), 1 << 20
    keys = po.gen_uniform_u32(n, 7, 0, M32)
    dest = dest_of(keys, parts)
    want_counts = np.bincount(dest, minlength=parts)
    for fill in FILLS:
        what = ("pjoin partition", parts, n, hex(fill))
        w = gt.Watch(fill)
        src = w.col(n, 0, data=keys, freeze=True)
        out_keys, out_rids = w.col(n, 0), w.col(n, 0)
        counts = w.u64(parts)
        nbytes = lib.dbhip_pjoin_partition_workspace_bytes(n, parts)
        ws = w.ws(nbytes)
        rc = lib.dbhip_pjoin_partition_u32(ptr(src), n, first, parts, ptr(out_keys), ptr(out_rids), ptr(counts), ptr(ws),
                                           nbytes, _stream())
        assert rc == 0, (what, rc)
        assert _status(ws) == 0, what
        assert np.array_equal(counts.cpu().numpy(), want_counts), what
        gk, gr = _u32(out_keys), _u32(out_rids).astype(np.int64) - first
        assert np.array_equal(np.sort(gr), np.arange(n)), what                  # every row once
        assert np.array_equal(keys[gr], gk), what                               # with its own key
        assert np.array_equal(dest_of(gk, parts), np.repeat(np.arange(parts), want_counts)), what  # bucket-major
        _check(w, what)


@pytest.mark.parametrize("n", [0, 1, 5, 100003])
def test_generators_write_n_words(n):
    lib, first = _lib(), 1 << 33  # a logical index above 32 bits
    where = po.gen_uniform_u32(n, 6, 0, M32)
    wants = {
        "uniform": po.gen_uniform_u32(n, 42, 3, 10000, first),
        "uniform at": (np.uint64(3) + mix64_np(42, where) % np.uint64(9998)).astype(np.uint32),
        "unique sorted": po.gen_unique_sorted_u32(n, 42, 1000),
    }
    for off in range(4):
        for fill in FILLS:
            for kind, want in wants.items():
                what = ("gen", kind, n, off, hex(fill))
                w = gt.Watch(fill)
                out = w.col(n, off)
                if kind == "uniform":
                    rc = lib.dbhip_gen_uniform_u32(ptr(out), n, 42, first, 3, 10000, _stream())
                elif kind == "uniform at":
                    idx = w.col(n, (off + 1) % 4, data=where, freeze=True)
                    rc = lib.dbhip_gen_uniform_at_u32(ptr(out), ptr(idx), n, 42, 3, 10000, _stream())
                else:
                    rc = lib.dbhip_gen_unique_sorted_u32(ptr(out), n, 42, 1000, _stream())
                assert rc == 0, what
                assert np.array_equal(_u32(out), want), what
                _check(w, what)


# ---- bitmask-claimed table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_kind", [0, 1])
@pytest.mark.parametrize("size", [1, 31, 32, 33, 1000, (1 << 20) + 1])
def test_bitmask_table_stays_inside_its_workspace(size, hash_kind):
    """the bitmask's last word is partial at every size but 32: reset, insert and lookup through a workspace of exactly
    the queried bytes"""
    lib, seed = _lib(), 421
    n = max(1, size // 2)
    keys = po.gen_unique_sorted_u32(2 * n, 9)  # unique; the odd ones are inserted, the even ones are looked up and missing
    vals = po.gen_uniform_u32(2 * n, 10, 1, M32)
    for fill in FILLS:
        what = ("bitmask table", size, hash_kind, hex(fill))
        w = gt.Watch(fill)
        k, v = w.col(n, 1, data=keys[1::2], freeze=True), w.col(n, 2, data=vals[1::2], freeze=True)
        q = w.col(2 * n, 3, data=keys, freeze=True)
        out_vals, out_found = w.col(2 * n, 1), w.col(2 * n, 2)
        nbytes = lib.dbhip_bitmask_table_workspace_bytes(size)
        ws = w.ws(nbytes)
        assert lib.dbhip_bitmask_table_reset(ptr(ws), nbytes, size, _stream()) == 0, what
        _check(w, what + ("reset",))
        assert lib.dbhip_bitmask_table_insert_u32(ptr(k), ptr(v), n, ptr(ws), nbytes, size, hash_kind, seed, 0, _stream()) == 0
        assert _status(ws) == 0, what
        _check(w, what + ("insert",))
        rc = lib.dbhip_bitmask_table_lookup_u32(ptr(q), 2 * n, ptr(ws), size, hash_kind, seed, ptr(out_vals), ptr(out_found),
                                                _stream())
        assert rc == 0, what
        hit = np.arange(2 * n) % 2 == 1
        assert np.array_equal(_u32(out_found), hit.astype(np.uint32)), what
        assert np.array_equal(_u32(out_vals), np.where(hit, vals, 0)), what
        assert _status(ws) == 0, what
        _check(w, what + ("lookup",))


# ---- cuckoo table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_kind", [1, 2])
@pytest.mark.parametrize("size", [1, 2, 7, 8, 1001, (1 << 20) + 1])
def test_cuckoo_table_stays_inside_its_workspace(size, hash_kind):
    """reset clears the slots as 16-byte vectors and an odd last slot on its own (cuckoo.hip).  The keys are chosen on
    the host with distinct first positions, so every row lands in an empty slot whatever the interleaving: no build can
    fail, and the slot layout is known"""
    lib, seeds = _lib(), (12345, 678)
    n = max(1, size // 4)
    cand = np.arange(1, 8 * n + 64, dtype=np.uint32)
    h1 = positions_np(cand, hash_kind, seeds[0], size)
    _, firsts = np.unique(h1, return_index=True)
    keys = cand[np.sort(firsts)[:n]]
    assert keys.size == n
    vals = po.gen_uniform_u32(n, 10, 1, M32)
    missing = np.arange(8 * n + 64, 8 * n + 64 + n, dtype=np.uint32)
    want_keys, want_vals = np.full(size, M32, np.uint32), np.zeros(size, np.uint32)
    want_keys[positions_np(keys, hash_kind, seeds[0], size)] = keys
    want_vals[positions_np(keys, hash_kind, seeds[0], size)] = vals
    for fill in FILLS:
        what = ("cuckoo table", size, hash_kind, hex(fill))
        w = gt.Watch(fill)
        k, v = w.col(n, 1, data=keys, freeze=True), w.col(n, 2, data=vals, freeze=True)
        q = w.col(2 * n, 3, data=np.concatenate([keys, missing]), freeze=True)
        inserted, out_vals, out_found = w.col(n, 3), w.col(2 * n, 1), w.col(2 * n, 2)
        slot_keys, slot_vals = w.col(size, 1), w.col(size, 3)
        nbytes = lib.dbhip_cuckoo_table_workspace_bytes(size)
        ws = w.ws(nbytes)
        assert lib.dbhip_cuckoo_table_reset(ptr(ws), nbytes, size, _stream()) == 0, what
        _check(w, what + ("reset",))
        rc = lib.dbhip_cuckoo_table_insert_u32(ptr(k), ptr(v), n, ptr(ws), nbytes, size, hash_kind, seeds[0], seeds[1], 0, 0,
                                               ptr(inserted), _stream())
        assert rc == 0 and _status(ws) == 0, what
        assert bool((inserted == 1).all()), what
        _check(w, what + ("insert",))
        rc = lib.dbhip_cuckoo_table_lookup_u32(ptr(q), 2 * n, ptr(ws), size, hash_kind, seeds[0], seeds[1], ptr(out_vals),
                                               ptr(out_found), _stream())
        assert rc == 0, what
        assert np.array_equal(_u32(out_found), np.repeat(np.array([1, 0], np.uint32), n)), what
        assert np.array_equal(_u32(out_vals), np.concatenate([vals, np.zeros(n, np.uint32)])), what
        rc = lib.dbhip_cuckoo_table_export_u32(ptr(ws), size, ptr(slot_keys), ptr(slot_vals), _stream())
        assert rc == 0, what
        assert np.array_equal(_u32(slot_keys), want_keys) and np.array_equal(_u32(slot_vals), want_vals), what
        assert _status(ws) == 0, what
        _check(w, what + ("lookup, export",))


# ---- validators --------------------------------------------------------------------------------------------------------
# A validator reports what later runs rest on: it must not touch the columns it judges, and its result is exactly the
# 1, 2 or 3 words include/dbhip.h names.  Expected words: the kernels' definitions (check.hip's header) in numpy.
CHECK_SIZES = [0, 1, 65, 100003]


_host_fingerprint, _sum64, _weighted = vm.fingerprint, vm.sum64, vm.weighted_sum  # the validators' numpy model


@pytest.mark.parametrize("n", CHECK_SIZES)
def test_validators_write_their_result_words_only(n):
    lib = _lib()
    for off, fill in enumerate(FILLS):
        def run(what, words, want, call, *cols, ws_bytes=None):
            """cols: host columns, all frozen behind guards at mixed offsets; call(result, *column pointers[, ws, bytes])"""
            w = gt.Watch(fill)
            views = [w.col(len(c), (off + i) % 4, data=c, freeze=True) for i, c in enumerate(cols)]
            result = w.u64(words)
            extra = ()
            if ws_bytes is not None:
                extra = (ptr(w.ws(ws_bytes)), ws_bytes)
            rc = call(ptr(result), *(ptr(v) for v in views), *extra)
            assert rc == 0, (what, n, hex(fill), rc)
            assert _words(result) == want, (what, n, hex(fill), _words(result), want)
            _check(w, (what, n, hex(fill)))

        s = _stream()
        src = po.gen_uniform_u32(n, 42, 1, 10000).view(np.int32)
        for filt in (5, 5001) if n <= 65 else (5,):
            run("fingerprint", 2, _host_fingerprint(po.copy_if_lt(src, filt)),
                lambda r, a, ws, nb: lib.dbhip_check_fingerprint_lt_i32(a, n, filt, r, ws, nb, s), src,
                ws_bytes=lib.dbhip_check_fingerprint_workspace_bytes(n))

        keys = po.gen_uniform_u32(n, 7, 0, M32)
        for signed in (0, 1):
            x = keys ^ np.uint32(0x80000000 if signed else 0)
            want = [int(np.count_nonzero(x[:-1] > x[1:])), _sum64(mix64_np(0x5bd1e995, keys)), _sum64(keys)]
            run("sorted", 3, want, lambda r, a: lib.dbhip_check_sorted_u32(a, n, signed, r, s), keys)
            perm = np.argsort(keys.view(np.int32) if signed else keys, kind="stable").astype(np.uint32)
            run("sorted_pairs", 2, [0, 0],
                lambda r, a, b, c: lib.dbhip_check_sorted_pairs_u32(a, b, c, n, signed, r, s), keys, keys[perm], perm)
        if n > 1:  # ids that are no sort permutation: both counters count
            ids = np.arange(n, dtype=np.uint32)[::-1].copy()
            mism = int(np.count_nonzero(keys[ids] != keys))
            x = keys.astype(np.int64)
            desc = int(np.count_nonzero((x[:-1] > x[1:]) | ((x[:-1] == x[1:]) & (ids[:-1] >= ids[1:]))))
            run("sorted_pairs, not sorted", 2, [desc, mism],
                lambda r, a, b, c: lib.dbhip_check_sorted_pairs_u32(a, b, c, n, 0, r, s), keys, keys, ids)

        gkeys, gvals = po.gen_uniform_u32(n, 1, 0, 999), po.gen_uniform_u32(n, 2, 0, M32)
        run("weighted_sum", 2, _weighted(gkeys, gvals), lambda r, a, b: lib.dbhip_check_weighted_sum_u32(a, b, n, r, s), gkeys, gvals)
        run("weighted_sum by index", 2, _weighted(np.arange(n, dtype=np.uint32), gvals),
            lambda r, b: lib.dbhip_check_weighted_sum_u32(None, b, n, r, s), gvals)

        ids = np.random.default_rng(5).permutation(n).astype(np.uint32)
        pbytes = lib.dbhip_check_permutation_workspace_bytes(n)
        run("permutation", 1, [0], lambda r, a, ws, nb: lib.dbhip_check_permutation_u32(a, n, r, ws, nb, s), ids, ws_bytes=pbytes)
        if n > 1:
            twice = ids.copy()
            twice[0], twice[-1] = twice[1], n  # one id seen before, one out of range
            run("permutation, two bad ids", 1, [2],
                lambda r, a, ws, nb: lib.dbhip_check_permutation_u32(a, n, r, ws, nb, s), twice, ws_bytes=pbytes)

        dbytes = lib.dbhip_check_distinct_workspace_bytes(n)
        for what, col in (("distinct", po.gen_unique_sorted_u32(n, 3)[::-1].copy()), ("distinct, repeats", gkeys)):
            srt = np.sort(col)
            run(what, 1, [int(np.count_nonzero(srt[:-1] >= srt[1:]))],
                lambda r, a, ws, nb: lib.dbhip_check_distinct_u32(a, n, r, ws, nb, s), col, ws_bytes=dbytes)

        build, probe = po.gen_uniform_u32(n, 42, 1, max(n // 2, 1)), po.gen_uniform_u32(n, 43, 1, max(n // 2, 1))
        order = np.argsort(build, kind="stable").astype(np.uint32)
        srt = build[order]
        lb, ub = np.searchsorted(srt, probe, "left"), np.searchsorted(srt, probe, "right")
        cnt = (ub - lb).astype(np.uint32)
        pos = np.where(cnt > 0, lb, 0).astype(np.uint32)
        run("join", 2, [0, int(cnt.sum())],
            lambda r, a, b, c, d, e, f: lib.dbhip_check_join_u32(a, n, b, n, c, d, e, f, 0, 0, 0, r, s),
            srt, probe, pos, cnt, order, build)

        ubuild, ubvals = po.gen_unique_sorted_u32(n, 11), po.gen_uniform_u32(n, 12, 0, M32 - 1)
        uprobe, upvals = po.gen_unique_sorted_u32(n, 13), po.gen_uniform_u32(n, 14, 0, M32 - 1)
        at = np.minimum(np.searchsorted(ubuild, uprobe), max(n - 1, 0))
        hit = ubuild[at] == uprobe if n else np.zeros(0, bool)
        outs = [np.where(hit, c, np.uint32(M32)).astype(np.uint32) for c in (uprobe, ubvals[at] if n else ubvals, upvals)]
        run("ujoin", 2, [0, int(hit.sum())],
            lambda r, a, b, c, d, e, f, g: lib.dbhip_check_ujoin_u32(a, b, n, c, d, n, e, f, g, r, s),
            ubuild, ubvals, uprobe, upvals, *outs)

        first = 1 << 20
        column = po.gen_uniform_u32(n, 42, 3, 10000, first)
        run("gen_uniform", 1, [0], lambda r, a: lib.dbhip_check_gen_uniform_u32(a, None, n, 42, first, 3, 10000, r, s), column)
        where = (np.arange(n, dtype=np.uint32)[::-1] + np.uint32(first)).copy()
        run("gen_uniform at indices", 1, [0],
            lambda r, a, b: lib.dbhip_check_gen_uniform_u32(a, b, n, 42, 0, 3, 10000, r, s), column[::-1].copy(), where)
        run("gen_uniform, another seed", 1, [int(np.count_nonzero(column != po.gen_uniform_u32(n, 41, 3, 10000, first)))],
            lambda r, a: lib.dbhip_check_gen_uniform_u32(a, None, n, 41, first, 3, 10000, r, s), column)

        for parts, rank in ((1, 0), (8, 3), (1024, 1023)):
            run("pjoin_route", 1, [int(np.count_nonzero(dest_of(keys, parts) != rank))],
                lambda r, a: lib.dbhip_check_pjoin_route_u32(a, n, parts, rank, r, s), keys)


# ---- the packed group-by on rows its sample did not see ----------------------------------------------------------------
SAMPLE_VECTORS = 64  # gb_aggregate_big_kernel: wave 0 reads three windows of 64 16-byte vectors


def _sample_rows(n):
    """the rows gb_aggregate_big_kernel samples: vectors [0, 64), [n4/2, n4/2 + 64), [n4 - 64, n4) with n4 = n / 4"""
    n4 = n // 4
    starts = (0, n4 // 2, n4 - SAMPLE_VECTORS)
    return np.concatenate([np.arange(4 * a, 4 * (a + SAMPLE_VECTORS)) for a in starts])


def _packed_case(n, groups, kind):
    """BASELINE's distribution (uniform keys, values in [1, 10000]) inside the three sampled windows, hostile outside"""
    rng = np.random.default_rng(groups + n % 7)
    rows = _sample_rows(n)
    assert rows.size == 768 and np.unique(rows).size == 768 and rows.max() < n
    keys, vals = po.gen_uniform_u32(n, 42, 0, groups - 1), po.gen_uniform_u32(n, 43, 1, 10000)
    # the sampled keys: every residue key & 1023 at most once over the 768 rows (1024 residues), so no counter of the
    # kernel's key test passes 1 and the key condition holds by construction; the multiple of 1024 on top is uniform
    residue = rng.permutation(1024)[:768]
    window_keys = (residue + 1024 * rng.integers(0, (groups - 1 - residue) // 1024 + 1)).astype(np.uint32)
    assert window_keys.max() < groups
    window_vals = vals[rows].copy()
    if kind == "wide values":            # the part above 16 bits spills on every row
        vals[:] = M32
    elif kind == "one key, 65535":       # carry counters saturate and drain all the time
        keys[:], vals[:] = groups // 3, 65535
    elif kind == "one table word":       # the existing skew_one_pair: both halves carry, and into each other
        keys = ((np.arange(n, dtype=np.uint32) & 1) + np.uint32(groups - 2 - (groups & 1))).astype(np.uint32)
        vals = po.gen_uniform_u32(n, 22, 0xFF00, 0x1FFFF)
    else:                                # crowds in every wave
        assert kind == "sorted keys"
        keys = np.sort(keys)
    keys[rows], vals[rows] = window_keys, window_vals
    return keys, vals


def _kernel_would_pack(n, groups, keys, vals, cus):
    """gb_aggregate_big_kernel's decision restated over the 768 sampled rows (float32, as the kernel computes)"""
    rows = _sample_rows(n)
    sk, sv = keys[rows], vals[rows]
    vmax = int(sv.max())
    kmax = int(np.bincount(sk & 1023, minlength=1024).max())
    f = np.float32
    mu = f(256.0) * f(int((sv >> 8).sum())) / f(rows.size)
    ranges = -(-groups // 65536)
    range_groups = (-(-groups // ranges) + 7) & ~7
    chunk_slots = max(1, min(cus, 256) // ranges)
    lam = f(n) / (f(chunk_slots) * f(range_groups))
    top = lam * mu + f(3.0) * np.sqrt(lam * f(vmax) * (mu + f(1.0)), dtype=f)
    return n >= 1 << 25 and vmax < 65536 and kmax < 8 and float(top) < 65536.0, (vmax, kmax, float(top))


@pytest.mark.parametrize("n", [1 << 25, (1 << 25) + 3])
@pytest.mark.parametrize("groups", [65536, 65535, 40000])
@pytest.mark.parametrize("kind", ["wide values", "one key, 65535", "one table word", "sorted keys"])
def test_packed_groupby_chosen_by_its_sample_on_rows_the_sample_did_not_see(kind, groups, n):
    """The slow path by design (the call's time is printed).  The sample's own figure over the 768 rows: top = 39696 at
    65536 and 65535 groups, 54358 at 40000 groups, against the bound of 65536."""
    from dwarf_bench_amd import ops
    keys, vals = _packed_case(n, groups, kind)
    packs, seen = _kernel_would_pack(n, groups, keys, vals, ops.device_info()[1])
    assert packs, ("the sample would not choose the packed table", seen)
    k, v = _dev(keys), _dev(vals)
    plan = ops.GroupBySum(n, groups)
    plan.launch(k, v)  # (warm-up: the first launch of a kernel loads its code object)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan.launch(k, v)
    got = plan.result()
    ms = (time.perf_counter() - t0) * 1e3
    print(f"packed group-by, {kind}, {groups} groups, n = {n}: {ms:.2f} ms (sample: vmax, kmax, top = {seen})")
    assert int(plan.ws[4:8].view(torch.int32).item()) == 1, "the kernel chose the wide tables: this test proves nothing"
    assert np.array_equal(_u32(got), po.groupby_sum(keys, vals, groups))
