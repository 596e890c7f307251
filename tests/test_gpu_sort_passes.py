"""The radix sorts on every pattern of skipped passes (csrc/radix.hip; the columns: tests/sort_pass_testlib.py, proven to
reach their paths by tests/test_sort_pass_model.py on the CPU).

Which passes run is decided on the device, and four things hang on it: the ping-pong parity of every later pass, whether
the finalize kernel copies tmp back, which buffer rs_chunk_hist counts from, and which pass of the argsort makes the
row ids (the first EXECUTED one).  A wrong decision gives a plausible, mis-sorted or mis-paired result under status 0.
Here every non-empty set of executed passes is sorted: all 15 with 8-bit digits and all 255 with 4-bit digits on the
one-workgroup path (5000 and 8192 keys) and on the fused-scan path (100003 keys: 13 chunks), all 15 and a list of 20
on the rs_chunk_scan path (33 * 8192 + 5 keys: 34 chunks, a ragged last tile and a ragged last 16-byte vector).

Per pass set two columns: whole digits vary, and one bit per executed digit varies (the lowest or the highest, see
sort_pass_testlib.columns; two values per digit is the crowded ranking path and leaves far more rows than distinct
keys, so every output position rests on the tie order).  Per column 12 sorts: unsigned and signed order x keys only
(dbhip_radix_sort_{u32,i32}), pairs with random 32-bit values and argsort (dbhip_radix_sort_pairs_{u32,i32} with
vals_are_row_ids 0 and 1) x the two guard fills.  Against numpy on the host, no tolerance: order =
np.argsort(view, kind="stable"), once per column and order; keys == keys[order], values == vals[order] or == order,
status word 0 (DBHIP_DEV_RANK_ORDER is a failure like any other value).  The calls go through the C ABI on guarded
buffers of exactly the entitled size (tests/guard_testlib.py); tmp, tmp_vals, the argsort's vals and the workspace
hold the guard fill when a call starts, so a result read from the wrong ping-pong buffer is the fill and not an
earlier call's right answer; every guard is looked at after every call.

Sorts per pytest case of test_every_set_of_executed_passes[bits-n-part] (pass sets x 2 columns x 12 sorts):
  8-bit, each of the four sizes, one part:               15 x 24 = 360
  4-bit, 5000 / 8192 / 100003, parts 0..6 (32 sets):     32 x 24 = 768
  4-bit, 5000 / 8192 / 100003, part 7 (sets 225..255):   31 x 24 = 744
  4-bit, 33 * 8192 + 5, one part (the list of 20):       20 x 24 = 480
29 cases, 20280 sorts.  The parts only cut the 255 sets into cases of a few seconds; together they walk all of them.

Then one plan of ops.RadixSort and one of ops.RadixSortPairs reused, workspace untouched, over columns that execute
bytes {3}, {0, 2}, {1, 2, 3}, {}, {1}, all (12 sorts per column, 72 per case), and the front doors the sort feeds:
ops.groupby_sorted and ops.topk on keys that vary only in the top byte (sign bit included) and only in byte 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guard_testlib as gt
from tests import reduce_by_key_model as rm
from tests import sort_pass_testlib as sp
from tests import topk_model as tm
from tests.guard_testlib import FILLS, ptr

pytestmark = pytest.mark.gpu
MODES = ("keys", "pairs", "argsort")
SORTS_PER_COLUMN = 2 * len(MODES) * len(FILLS)


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def _ops():
    from dwarf_bench_amd import ops
    return ops


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


def _orders(keys):
    """the reference, once per column: the stable argsort of the unsigned and of the signed view"""
    return {False: np.argsort(keys, kind="stable"), True: np.argsort(keys.view(np.int32), kind="stable")}


class Rig:
    """the guarded buffers of the sorts of one (n, bits, fill): keys, tmp and a workspace for the keys-only entry
    points; keys, vals, tmp_keys, tmp_vals and a workspace for the pairs entry points.  Allocated once per pytest case;
    every call starts with the columns it only writes, and the workspace, holding the fill again."""

    def __init__(self, n, bits, fill):
        lib = _lib()
        self.n, self.bits, self.fill = n, bits, fill
        self.wk, self.wp = gt.Watch(fill), gt.Watch(fill)
        self.k_keys, self.k_tmp = self.wk.col(n), self.wk.col(n)
        self.k_bytes = lib.dbhip_radix_sort_workspace_bytes(n, bits)
        self.k_ws = self.wk.ws(self.k_bytes)
        self.p_keys, self.p_vals, self.p_tmp, self.p_tmpv = (self.wp.col(n) for _ in range(4))
        self.p_bytes = lib.dbhip_radix_sort_pairs_workspace_bytes(n, bits)
        self.p_ws = self.wp.ws(self.p_bytes)
        self.k_clean, self.p_clean = self.k_ws.clone(), self.p_ws.clone()  # the fill pattern, byte by byte
        self.word = gt.i32(fill)

    def sort(self, mode, dkeys, dvals, signed):
        """one call -> (status, keys, values or None) as host arrays; the return code and every guard asserted here"""
        lib, n = _lib(), self.n
        if mode == "keys":
            self.k_keys.copy_(dkeys)
            self.k_tmp.fill_(self.word)
            self.k_ws.copy_(self.k_clean)
            fn = lib.dbhip_radix_sort_i32 if signed else lib.dbhip_radix_sort_u32
            rc = fn(ptr(self.k_keys), ptr(self.k_tmp), n, self.bits, ptr(self.k_ws), self.k_bytes, _stream())
            assert rc == 0, rc
            got = _status(self.k_ws), _u32(self.k_keys), None
            self.wk.check()
            return got
        self.p_keys.copy_(dkeys)
        if mode == "pairs":
            self.p_vals.copy_(dvals)
        else:
            self.p_vals.fill_(self.word)  # the argsort writes vals and never reads it
        self.p_tmp.fill_(self.word)
        self.p_tmpv.fill_(self.word)
        self.p_ws.copy_(self.p_clean)
        fn = lib.dbhip_radix_sort_pairs_i32 if signed else lib.dbhip_radix_sort_pairs_u32
        rc = fn(ptr(self.p_keys), ptr(self.p_vals), ptr(self.p_tmp), ptr(self.p_tmpv), n, self.bits, int(mode == "argsort"),
                ptr(self.p_ws), self.p_bytes, _stream())
        assert rc == 0, rc
        got = _status(self.p_ws), _u32(self.p_keys), _u32(self.p_vals)
        self.wp.check()
        return got


def _verdict(got, keys, vals, order, mode):
    """None when the call's result is the reference's, else what differs"""
    status, got_keys, got_vals = got
    wrong = []
    if status != 0:
        wrong.append(f"status {status}")
    if not np.array_equal(got_keys, keys[order]):
        wrong.append("keys")
    if mode == "pairs" and not np.array_equal(got_vals, vals[order]):
        wrong.append("values")
    if mode == "argsort" and not np.array_equal(got_vals, order.astype(np.uint32)):
        wrong.append("row ids")
    return ", ".join(wrong) or None


def run_case(bits, n, part):
    """every sort of one pytest case -> (sorts made, [(pass set, style, base, mode, signed, fill, what differs)]).
    Wrong results are collected, so that one run names every combination that fails; a return code, a guard or an
    exception ends the case at once."""
    rigs = [Rig(n, bits, fill) for fill in FILLS]
    vals = np.random.default_rng(n + bits).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dvals = _dev(vals)
    sorts, failures = 0, []
    for set_mask, style, base, vary_mask, seed in sp.columns(bits, n, part):
        keys = sp.keys_for(vary_mask, n, seed, base)
        dkeys, orders = _dev(keys), _orders(keys)
        for signed in (False, True):
            for mode in MODES:
                for rig in rigs:
                    try:
                        got = rig.sort(mode, dkeys, dvals, signed)
                    except AssertionError as e:
                        raise AssertionError(f"{(bits, n, hex(set_mask), style, hex(base), mode, signed, hex(rig.fill))}: {e}") from None
                    sorts += 1
                    bad = _verdict(got, keys, vals, orders[signed], mode)
                    if bad:
                        failures.append((hex(set_mask), style, hex(base), mode, "signed" if signed else "unsigned",
                                         hex(rig.fill), bad))
    return sorts, failures


@pytest.mark.parametrize("bits,n,part", sp.cases())
def test_every_set_of_executed_passes(bits, n, part):
    sorts, failures = run_case(bits, n, part)
    assert sorts == len(sp.columns(bits, n, part)) * SORTS_PER_COLUMN
    assert not failures, f"{len(failures)} of {sorts} sorts wrong, (pass set, style, base, mode, order, fill, what): {failures[:12]}"


def test_the_cases_walk_every_pass_set_and_the_sizes_reach_their_paths():
    """the arithmetic of radix.hip restated: tiles of 8192 keys, one workgroup up to one tile, the scatter's own prefix
    sum up to 32 chunks (kRsFusedScanChunks), one tile per chunk below the chunk target.  Whoever moves a threshold sees
    this fail and not a path fall out of the cases above."""
    tile, fused = 8192, 32
    for bits, target in ((8, 2048), (4, 1024)):
        tiles = [-(-n // tile) for n in sp.SIZES]
        assert all(t < target for t in tiles)          # q = tiles / target = 0: one tile per chunk, chunks = tiles
        assert tiles == [1, 1, 13, 34]
        assert tiles[2] <= fused < tiles[3]
        assert [sp.geometry(n, bits) for n in sp.SIZES] == [(t, 1, t) for t in tiles]
    assert sp.SIZES[0] < tile == sp.SIZES[1] and all(n % tile and n % 4 for n in sp.SIZES[2:])
    # the workspace the library asks for holds exactly the count matrix of that many chunks (rows padded to four chunks)
    lib = _lib()
    for bits in (4, 8):
        for n in sp.SIZES:
            chunks = sp.geometry(n, bits)[2]
            header_totals_bases = 256 + 4 * 8 * 8 * 256 + 4 * 8 * 256
            want = header_totals_bases + 4 * (1 << bits) * ((chunks + 3) & ~3)
            assert lib.dbhip_radix_sort_workspace_bytes(n, bits) == (want + 255) & ~255, (bits, n)
    per_case = {(b, n, p): len(sp.columns(b, n, p)) * SORTS_PER_COLUMN for b, n, p in sp.cases()}
    assert len(per_case) == 29 and sum(per_case.values()) == 20280
    assert sorted(set(per_case.values())) == [360, 480, 744, 768]
    for bits in (4, 8):
        for n in sp.SIZES:
            walked = [c[0] for p in sp.parts(bits, n) for c in sp.columns(bits, n, p)][::2]
            full = list(range(1, 1 << (32 // bits)))
            assert walked == (list(sp.CHUNKED_SETS_4BIT) if (bits, n) == (4, sp.CHUNKED_SIZE) else full)


# ---- one plan, columns whose executed sets differ ------------------------------------------------------------------------
@pytest.mark.parametrize("n", sp.SIZES)
@pytest.mark.parametrize("bits", [4, 8])
def test_one_plan_over_columns_with_different_executed_passes(bits, n):
    """ops.RadixSort and ops.RadixSortPairs, one plan each for the whole sequence {3}, {0, 2}, {1, 2, 3}, {}, {1}, all
    (bytes; with 4-bit digits both nibbles of a byte).  The workspace is the plan's and nothing clears it between the
    calls: a skip flag, a parity or final_in_tmp left over from the call before must not leak.  The buffers that a call
    only writes (tmp, tmp_keys, tmp_vals, the argsort's permutation) are poisoned before every call."""
    ops = _ops()
    plan, pairs = ops.RadixSort(n, bits), ops.RadixSortPairs(n, bits)
    vals = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    call = 0
    for byte_set, keys in sp.reuse_columns(n):
        orders = _orders(keys)
        for signed in (False, True):
            order = orders[signed]
            for mode in MODES:
                for _ in FILLS:  # every call twice in a row: the second one starts from the first one's header
                    word = gt.i32(FILLS[call % 2])
                    call += 1
                    what = (bits, n, byte_set, mode, signed, call)
                    dkeys = _dev(keys)
                    if mode == "keys":
                        plan.tmp.fill_(word)
                        plan.launch(dkeys, signed)
                        assert ops.workspace_status(plan.ws) == 0, what
                    else:
                        for t in (pairs.tmp_keys, pairs.tmp_vals, pairs.perm):
                            t.fill_(word)
                        got = pairs.launch(dkeys, _dev(vals) if mode == "pairs" else None, signed)
                        assert ops.workspace_status(pairs.ws) == 0, what
                        want = vals[order] if mode == "pairs" else order.astype(np.uint32)
                        assert np.array_equal(_u32(got), want), what
                    assert np.array_equal(_u32(dkeys), keys[order]), what
    assert call == len(sp.REUSE_BYTE_SETS) * SORTS_PER_COLUMN


# ---- the front doors the sort feeds ------------------------------------------------------------------------------------
def test_groupby_sorted_and_topk_on_keys_that_vary_in_one_byte():
    """ops.groupby_sorted = the pairs sort + reduce_by_key, against tests/reduce_by_key_model.py on the stably sorted
    columns; ops.topk orders its selected pairs with the same sort, against tests/topk_model.py.  Keys that vary only in
    the top byte, sign bit included (the only executed pass of the 8-bit sort is the last one, and in signed order all
    of the order rests on the sign flip), and only in byte 1 (one executed pass between skipped ones)."""
    ops = _ops()
    names = ("keys", "counts", "sums", "mins", "maxs")
    for name, keys in sp.front_door_columns():
        n = keys.size
        vals = np.random.default_rng(n + len(name)).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        dk, dv = _dev(keys), _dev(vals)
        for signed_keys in (False, True):
            order = np.argsort(keys.view(np.int32) if signed_keys else keys, kind="stable")
            for signed in (False, True):
                want = rm.reduce_by_key(keys[order], vals[order], signed)
                got = ops.groupby_sorted(dk, dv, signed=signed, signed_keys=signed_keys)
                assert got[0].numel() == 256
                for which, g, w in zip(names, got, want):
                    g = g.cpu().numpy()
                    assert np.array_equal(g.view(np.uint64) if which == "sums" else g.view(np.uint32), w), (name, which, signed, signed_keys)
            for largest in (False, True):
                for srt in (True, False):
                    got_keys, got_rows = ops.topk(dk, 1000, largest=largest, signed=signed_keys, sorted=srt)
                    want_keys, want_rows = tm.topk(keys, 1000, largest, signed_keys, sorted=srt)
                    assert np.array_equal(_u32(got_rows), want_rows), (name, "topk rows", largest, signed_keys, srt)
                    assert np.array_equal(_u32(got_keys), want_keys), (name, "topk keys", largest, signed_keys, srt)
        assert np.array_equal(_u32(dk), keys) and np.array_equal(_u32(dv), vals)  # both doors leave their input alone
