"""Numpy twins of the device-side validators (csrc/check.hip, the check at the end of csrc/join_pairs.hip and the route
check of csrc/partition.hip): one function per validator returns the exact result words the device must produce, and
next to it stands the verdict dwarf_bench_amd/host/hip_dwarfs.cpp draws from those words.  Test infrastructure: it
imports nothing from the library, only the oracle's mix64 (pinned by tests/golden/mix64.json) to vouch for its own.

Columns are numpy uint32 arrays (int32 for the scan), results are lists of Python ints below 2^64.
"""
import json
from pathlib import Path

import numpy as np

from oracle import pyoracle as po
from tests.pjoin_testlib import dest_of, fmix32

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
FP_MUL = 0x9E3779B97F4A7C15  # kFpMul
SORT_SEED = 0x5bd1e995       # the multiset fingerprint's mix64 seed
PICK_SEED = 7                # the join check's pseudo-random id
SENTINEL = 0xFFFFFFFF
CK_THREADS, WAVE, FP_MAX_BLOCKS = 256, 64, 1024


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == np.int32 else np.asarray(a, dtype=np.uint32)


def u64(a):
    return np.asarray(a).astype(np.uint64)


def sum64(a) -> int:
    with np.errstate(over="ignore"):
        return int(np.sum(u64(a), dtype=np.uint64)) & M64


def mix64(seed: int, index):
    """mix64 of csrc/dbhip_common.hpp over an array of 64-bit indices, as uint64"""
    with np.errstate(over="ignore"):
        z = (u64(index) + np.uint64(1)) * np.uint64(FP_MUL) + np.uint64(seed & M64) * np.uint64(0xD1B54A32D192ED03)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def self_check():
    """the model's mix64 against the golden vectors and the oracle's"""
    golden = json.loads((Path(__file__).parent / "golden" / "mix64.json").read_text())["mix64_seed42_i0_2"]
    assert mix64(42, np.arange(3)).tolist() == golden
    idx = [0, 1, 2, 77, (1 << 33) + 5, M64]
    for seed in (0, 7, 42, SORT_SEED, M64):
        assert mix64(seed, np.array(idx, dtype=np.uint64)).tolist() == [po.mix64(seed, i) for i in idx]


def gen_value(seed: int, lo: int, hi: int, index):
    """lo + mix64(seed, index) % (hi - lo + 1), 32-bit wrap-around as the device's unsigned sum"""
    span = np.uint64(hi - lo + 1)
    return ((mix64(seed, index) % span + np.uint64(lo)) & np.uint64(M32)).astype(np.uint32)


# ---- ordered fingerprint (scan) --------------------------------------------------------------------------------------------
def fp_geo(n: int):
    """(blocks, seg) of check.hip's fp_geo: thread t of blocks * 256 walks [t * seg, (t + 1) * seg)"""
    threads_wanted = (n + 63) // 64
    blocks = min(max((threads_wanted + CK_THREADS - 1) // CK_THREADS, 1), FP_MAX_BLOCKS)
    return blocks, max((n + blocks * CK_THREADS - 1) // (blocks * CK_THREADS), 1)


def fingerprint(seq):
    """[sum (x_i + 1) * P^(L-1-i) mod 2^64, L] over a whole sequence"""
    v = (np.asarray(seq).astype(np.int64) & np.int64(M32)).astype(np.uint64) + np.uint64(1)  # int32 or uint32 words
    if v.size == 0:
        return [0, 0]
    with np.errstate(over="ignore"):
        pw = np.ones(v.size, dtype=np.uint64)
        pw[1:] = FP_MUL
        pw = np.multiply.accumulate(pw, dtype=np.uint64)[::-1]
        return [int(np.sum(v * pw, dtype=np.uint64)) & M64, int(v.size)]


def fingerprint_lt(src, filt: int):
    src = np.asarray(src, dtype=np.int32)
    return fingerprint(src[src < filt])


def verdict_scan(count: int, got, want) -> bool:
    """TwoPassScanHip: count == want_len && got == want (got over out[0..min(count, n)) under the same filter)"""
    return count == want[1] and list(got) == list(want)


# ---- sorted ----------------------------------------------------------------------------------------------------------------
def _order(keys, signed):
    return u32(keys) ^ np.uint32(0x80000000 if signed else 0)


def sorted_words(keys, signed=False):
    keys = u32(keys)
    x = _order(keys, signed)
    return [int(np.count_nonzero(x[:-1] > x[1:])), sum64(mix64(SORT_SEED, keys)), sum64(keys)]


def verdict_sort(got, want) -> bool:
    """RadixHip: descents == 0 and both fingerprints those of the input"""
    return got[0] == 0 and got[1] == want[1] and got[2] == want[2]


def sorted_pairs(keys_in, keys_out, ids_out, signed=False):
    keys_in, keys_out, ids = u32(keys_in), u32(keys_out), u32(ids_out)
    n = keys_out.size
    x = _order(keys_out, signed)
    desc = int(np.count_nonzero((x[:-1] > x[1:]) | ((x[:-1] == x[1:]) & (ids[:-1] >= ids[1:]))))
    inside = ids < n
    carried = np.zeros(n, dtype=bool)
    carried[inside] = keys_in[ids[inside]] == keys_out[inside]
    return [desc, int(n - np.count_nonzero(carried))]


def verdict_sort_pairs(got) -> bool:
    return got[0] == 0 and got[1] == 0


# ---- group-by --------------------------------------------------------------------------------------------------------------
def weights(keys):
    """(wt0, wt1) of check.hip as uint64 arrays: fmix32(k) | 1 and fmix32(k ^ 0x9E3779B9) | 1"""
    keys = u32(keys)
    return [fmix32(keys ^ np.uint32(salt)) | np.uint64(1) for salt in (0, 0x9E3779B9)]


def weighted_sum(keys, vals, wts=None):
    """keys None: the index (the dense group-by output); wts: weights(keys) where a caller has them already"""
    vals = u32(vals)
    if wts is None:
        wts = weights(np.arange(vals.size, dtype=np.uint64).astype(np.uint32) if keys is None else keys)
    return [sum64((u64(vals) * wt) & np.uint64(M32)) & M32 for wt in wts]


def verdict_groupby(got, want) -> bool:
    """GroupByHip: the weighted sums over (g, out[g]) equal those over the rows"""
    return list(got) == list(want)


def distinct(keys):
    s = np.sort(u32(keys))
    return [int(np.count_nonzero(s[:-1] >= s[1:]))]


def verdict_groupby_hash(keys, vals, out_keys, out_sums, out_counts, cap=None) -> bool:
    """GroupByHashHip: g <= cap, both weighted sums equal the rows', keys distinct, counts sum to n"""
    n, g = u32(keys).size, u32(out_keys).size
    if cap is not None and g > cap:
        return False
    return (weighted_sum(out_keys, out_sums) == weighted_sum(keys, vals)
            and weighted_sum(out_keys, out_counts) == weighted_sum(keys, np.ones(n, np.uint32))
            and distinct(out_keys) == [0] and sum64(out_counts) == n)


# ---- permutation -----------------------------------------------------------------------------------------------------------
def permutation(ids):
    ids = u32(ids)
    inside = ids[ids < ids.size]
    return [int(ids.size - np.unique(inside).size)]


# ---- one-to-many join ------------------------------------------------------------------------------------------------------
def _key_of(ids, n_build, build_keys, gen):
    """(key carried by each id, whether the id names a row at all)"""
    ids = u32(ids)
    if build_keys is None:
        return gen_value(gen[0], gen[1], gen[2], ids), np.ones(ids.size, dtype=bool)
    ok = ids < n_build
    key = np.zeros(ids.size, dtype=np.uint32)
    key[ok] = u32(build_keys)[ids[ok]]
    return key, ok


def join_picks(cnt):
    """offset inside its range of the pseudo-random id of every probe row (0 where cnt == 0)"""
    cnt = u64(u32(cnt))
    return mix64(PICK_SEED, np.arange(cnt.size, dtype=np.uint64)) % np.maximum(cnt, np.uint64(1))


def join_row_ok(sorted_build, probe, pos, cnt, ids, build_keys=None, gen=(0, 0, 0)):
    """per probe row: count == multiplicity, range inside the id buffer, first / last / picked id carry the key"""
    srt, probe, pos, cnt, ids = (u32(a) for a in (sorted_build, probe, pos, cnt, ids))
    n_build = srt.size
    uniq, times = np.unique(srt, return_counts=True)  # multiplicity of every probe key among the build keys
    at = np.minimum(np.searchsorted(uniq, probe), max(uniq.size - 1, 0))
    mult = np.where(uniq[at] == probe, times[at], 0) if uniq.size else np.zeros(probe.size, dtype=np.int64)
    ok = cnt.astype(np.int64) == mult
    live = ok & (cnt > 0)
    inside = live & (pos.astype(np.int64) + cnt.astype(np.int64) <= n_build)
    ok &= ~live | inside
    rows = np.nonzero(inside)[0]
    if rows.size:
        key, named = _key_of(ids[:n_build], n_build, build_keys, gen)
        p, c = pos[rows].astype(np.int64), cnt[rows].astype(np.int64)
        for at in (p, p + c - 1, p + join_picks(cnt)[rows].astype(np.int64)):
            ok[rows] &= named[at] & (key[at] == probe[rows])
    return ok


def join_runs(sorted_build, ids, build_keys=None, gen=(0, 0, 0)):
    """(neighbours of ids carrying different keys, neighbours of the sorted build column that differ): equal iff every
    key is one run of ids, given that ids is a permutation; an id that names no row differs from every neighbour"""
    srt = u32(sorted_build)
    key, named = _key_of(u32(ids)[:srt.size], srt.size, build_keys, gen)
    up = int(np.count_nonzero((key[:-1] != key[1:]) | ~named[:-1] | ~named[1:]))
    return up, int(np.count_nonzero(srt[:-1] != srt[1:]))


def join(sorted_build, probe, pos, cnt, ids, build_keys=None, gen=(0, 0, 0)):
    """[bad probe rows in the low half | (key runs of ids - distinct neighbours of the build keys) mod 2^32 in the high
    half, sum of counts]; nothing is judged without probe rows"""
    if u32(probe).size == 0:
        return [0, 0]
    bad = int(np.count_nonzero(~join_row_ok(sorted_build, probe, pos, cnt, ids, build_keys, gen)))
    up, down = join_runs(sorted_build, ids, build_keys, gen)
    return [(bad + ((up - down) << 32)) & M64, sum64(u32(cnt))]


def verdict_join(join_words, permutation_words) -> bool:
    """JoinOmnisciHip: no bad row, every key one run, ids a permutation of the build rows"""
    return join_words[0] == 0 and permutation_words[0] == 0


def verdict_probe(join_words, n) -> bool:
    """ProbeHip: no bad row, as many key runs as keys, and the counts sum to n; NO permutation check beside it"""
    return join_words[0] == 0 and join_words[1] == n


def verdict_pjoin_join(join_words) -> bool:
    """the partitioned join's engine adds result[0] to its bad rows; ids (global row ids) get no permutation check"""
    return join_words[0] == 0


# ---- pair table ------------------------------------------------------------------------------------------------------------
def _pair_mix(b, p):
    return mix64(0, (u64(p) << np.uint64(32)) | u64(b))


def join_pairs(build_keys, probe_keys, ids, pos, cnt, out_b, out_p, probe_row_ids=None, left_outer=False):
    """[bad pairs, pairs expected, fingerprint of the pairs given, fingerprint expected]"""
    bk, pk, ids, pos, cnt, ob, op = (u32(a) for a in (build_keys, probe_keys, ids, pos, cnt, out_b, out_p))
    n_build, n_probe = bk.size, pk.size
    p_ok = op < n_probe
    sent = ob == SENTINEL
    b_ok = ob < n_build
    match = np.zeros(ob.size, dtype=bool)
    both = p_ok & b_ok & ~sent
    match[both] = bk[ob[both]] == pk[op[both]]
    good = p_ok & np.where(sent, bool(left_outer), match)
    c = np.where(pos.astype(np.int64) + cnt.astype(np.int64) > n_build, 0, cnt.astype(np.int64))
    rid = np.arange(n_probe, dtype=np.uint32) if probe_row_ids is None else u32(probe_row_ids)
    start = np.cumsum(c) - c
    at = np.repeat(pos.astype(np.int64) - start, c) + np.arange(int(c.sum()))
    want_fp, pairs = sum64(_pair_mix(ids[at], np.repeat(rid, c))), int(c.sum())
    if left_outer:
        empty = c == 0
        want_fp = (want_fp + sum64(_pair_mix(np.full(int(empty.sum()), SENTINEL, np.uint32), rid[empty]))) & M64
        pairs += int(empty.sum())
    return [int(ob.size - np.count_nonzero(good)), pairs, sum64(_pair_mix(ob, op)), want_fp]


def verdict_join_pairs(words, n_pairs) -> bool:
    return words[0] == 0 and words[1] == n_pairs and words[2] == words[3]


# ---- unique-key join -------------------------------------------------------------------------------------------------------
def ujoin(sorted_build, build_vals, probe, probe_vals, out_key, out_bval, out_pval):
    srt, bv, pk, pv, ok_, o1, o2 = (u32(a) for a in (sorted_build, build_vals, probe, probe_vals, out_key, out_bval, out_pval))
    lb = np.searchsorted(srt, pk, "left")
    at = np.minimum(lb, max(srt.size - 1, 0))
    found = (lb < srt.size) & (srt[at] == pk) if srt.size else np.zeros(pk.size, dtype=bool)
    hit_ok = (ok_ == pk) & (o1 == (bv[at] if srt.size else 0)) & (o2 == pv)
    miss_ok = (ok_ == SENTINEL) & (o1 == SENTINEL) & (o2 == SENTINEL)
    return [int(np.count_nonzero(~np.where(found, hit_ok, miss_ok))), int(np.count_nonzero(found))]


def verdict_ujoin(words) -> bool:
    return words[0] == 0


# ---- generator and routing -------------------------------------------------------------------------------------------------
def gen_uniform(values, seed, lo, hi, first_index=0, indices=None):
    values = u32(values)
    idx = (np.arange(values.size, dtype=np.uint64) + np.uint64(first_index)) if indices is None else u64(u32(indices))
    return [int(np.count_nonzero(values != gen_value(seed, lo, hi, idx)))]


def pjoin_route(keys, parts, rank):
    return [int(np.count_nonzero(dest_of(u32(keys), parts) != rank))]


def verdict_zero(words) -> bool:
    """gen_uniform, pjoin_route, distinct, permutation on their own: the one word counts what is wrong"""
    return words[0] == 0
