"""The device-side validators against every kind of wrong result: the words of every dbhip_check_* kernel equal, exactly,
those of the numpy model (tests/validator_model.py, itself judged against brute-force truth in
tests/test_validator_model.py), and the verdict the dwarfs draw from them is the one the catalogue entry is tagged with.

Shapes.  W = compute units * 8 * 256 is the thread count of the capped grid of the grid-stride validators: sizes up to
2W + 3 reach the second and third trip of the stride loop, W - 1 | W is the wrap, and the columns start 0, 4, 8 or 12
bytes past a 16-byte boundary.  The ordered fingerprint has its own decomposition (fp_geo, restated in the model):
thread segments of `seg` elements, 64 segments a wave, 256 a block, `per` blocks a lane of the final kernel.

Positions.  Every neighbour-comparing or per-element kernel is hit at i in {0, 62, 63, 64, 254, 255, 256, W-2, W-1, W,
n-2, n-1} and 32 seeded random places; the fingerprint before and after the first and the last multiple of seg,
64 seg, 256 seg and per * 256 seg.

Tags.  `reject` / `accept`: the verdict must be that.  `blind`: the verdict wrongly accepts, and the entry pins the
words to the model so a change of behaviour is noticed.  The blind list is closed: (a) weighted-sum moves between groups
whose model words coincide, (b) out_pos of a join row without a match.
"""
import numpy as np
import pytest
import torch

from tests import validator_model as vm

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered")]
M32 = vm.M32
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
DEVICE = "cuda"
SIZES = ["0", "1", "2", "63", "64", "65", "255", "256", "257", "W-1", "W", "W+1", "W+257", "2W+3"]


# ---- the device calls, words as lists --------------------------------------------------------------------------------------
def _ops():
    from dwarf_bench_amd import ops
    return ops


def grid_threads() -> int:
    return _ops().device_info()[1] * 8 * 256


def d_fingerprint(src, filt):
    return list(_ops().check_fingerprint_lt(src, filt))


def d_sorted(keys, signed=False):
    return list(_ops().check_sorted(keys, signed))


def d_sorted_pairs(keys_in, keys_out, ids, signed=False):
    return list(_ops().check_sorted_pairs(keys_in, keys_out, ids, signed))


def d_weighted(keys, vals):
    return list(_ops().check_weighted_sum(keys, vals))


def d_distinct(keys):
    return [_ops().check_distinct(keys)]


def d_permutation(ids):
    return [_ops().check_permutation(ids)]


def d_join(srt, probe, pos, cnt, ids, build_keys=None, gen=(0, 0, 0)):
    return list(_ops().check_join(srt, probe, pos, cnt, ids, build_keys=build_keys, gen=gen))


def d_join_pairs(build, probe, ids, pos, cnt, out_b, out_p, left_outer=False):
    return list(_ops().check_join_pairs(build, probe, ids, pos, cnt, out_b, out_p, left_outer=left_outer))


def d_ujoin(*cols):
    return list(_ops().check_ujoin(*cols))


def d_gen(values, seed, lo, hi, first_index=0, indices=None):
    return [_ops().check_gen_uniform(values, seed, lo, hi, first_index=first_index, indices=indices)]


def d_route(keys, parts, rank):
    from dwarf_bench_amd import _capi
    res = torch.empty(1, dtype=torch.int64, device=keys.device)
    _capi.check(_capi.lib().dbhip_check_pjoin_route_u32(keys.data_ptr(), keys.numel(), parts, rank, res.data_ptr(),
                                                        _ops()._stream()), "check_pjoin_route_u32")
    return [int(res.cpu()[0]) & vm.M64]


# ---- columns ---------------------------------------------------------------------------------------------------------------
def dev(a, off=0, tail=None):
    """host column -> int32 device column starting `off` words past a 16-byte boundary (`tail`: words kept behind it)"""
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32)
    extra = np.zeros(0, np.int32) if tail is None else np.ascontiguousarray(tail).view(np.int32)
    base = torch.zeros(off + a.size + extra.size + 4, dtype=torch.int32, device=DEVICE)
    base[off:off + a.size + extra.size] = torch.from_numpy(np.concatenate([a, extra]))
    return base[off:off + a.size]


def size_of(label: str, w: int) -> int:
    """"257" -> 257, "W-1" -> w - 1, "2W+3" -> 2 w + 3"""
    if "W" not in label:
        return int(label)
    factor, rest = label.split("W")
    return int(factor or 1) * w + int(rest or 0)


def positions(n, w, rng, need=1):
    """the seam positions i with i + need <= n, then 32 seeded random ones"""
    fixed = [i for i in (0, 62, 63, 64, 254, 255, 256, w - 2, w - 1, w, n - 2, n - 1) if 0 <= i <= n - need]
    fixed = sorted(set(fixed))
    rand = rng.integers(0, n - need + 1, 32).tolist() if n >= need else []
    return fixed, fixed + sorted(set(rand) - set(fixed))


def batches(places, n):
    """small columns: one place at a time; large ones, where a model call costs, all places in one call (the kernels that
    get batches judge every row on its own, so the count must be the number of places)"""
    return [[i] for i in places] if n <= 4096 else [list(places)]


def poke(col, at, values):
    """write values at positions of a device column; returns what stood there"""
    idx = torch.as_tensor(np.atleast_1d(at), dtype=torch.int64, device=col.device)
    old = col[idx].clone()
    col[idx] = torch.from_numpy(np.atleast_1d(np.asarray(values, dtype=np.uint32)).view(np.int32)).to(col.device)
    return idx, old


class Poked:
    """a device column and its host twin with some words replaced for the length of a `with` block"""

    def __init__(self, col, host, at, values):
        self.col, self.host, self.at = col, host, np.atleast_1d(at)
        self.values = np.atleast_1d(np.asarray(values, dtype=np.uint32))

    def __enter__(self):
        self.idx, self.old = poke(self.col, self.at, self.values)
        self.host_old = self.host[self.at].copy()
        self.host[self.at] = self.values
        return self

    def __exit__(self, *exc):
        self.col[self.idx] = self.old
        self.host[self.at] = self.host_old


# ---- ordered fingerprint ---------------------------------------------------------------------------------------------------
FP_SIZES = [0, 1, 64, 65, 16385, 1048577, (1 << 24) + (1 << 16) + 5]


def fp_seams(n):
    """elements after which a unit of the decomposition ends: first and last multiple of seg, 64 seg, 256 seg and
    per * 256 seg below n (mirrors fp_geo and the final kernel's lane split in check.hip)"""
    blocks, seg = vm.fp_geo(n)
    per = (blocks + vm.WAVE - 1) // vm.WAVE
    out = set()
    for unit in (seg, vm.WAVE * seg, vm.CK_THREADS * seg, per * vm.CK_THREADS * seg):
        if unit < n:
            out |= {unit, (n - 1) // unit * unit}
    return sorted(out)


FP_CASES = [(n, off) for n in FP_SIZES for off in (0, 1, 2, 3)]


@pytest.mark.parametrize("n,off", FP_CASES)
def test_fingerprint_words_and_scan_verdict(n, off):
    """src: 1 in 64 elements passes the filter, so the model stays cheap at 2^24; the elements on both sides of every seam
    (and of 32 random places) pass and differ, and a swap across the seam must change the fingerprint"""
    rng = np.random.default_rng(n + off)
    filt = 1000
    src = rng.integers(filt, INT_MAX, n, endpoint=True).astype(np.int32)
    some = rng.random(n) < 1 / 64
    src[some] = rng.integers(INT_MIN, filt, int(some.sum())).astype(np.int32)
    seams = fp_seams(n)
    rand = sorted({int(m) for m in rng.integers(1, n, 32)} - {m + d for m in seams for d in (-1, 0, 1)}) if n >= 2 else []
    rand = [m for k, m in enumerate(rand) if k == 0 or m - rand[k - 1] > 1]
    for m in seams + rand:
        src[m - 1], src[m] = -5 - m % 7, 7 + m % 11
    col = dev(src, off)
    want = vm.fingerprint_lt(src, filt)
    assert d_fingerprint(col, filt) == want
    assert want[1] == int(np.count_nonzero(src < filt))
    host = src.view(np.uint32)
    for m in seams + rand:  # reject: neighbour swap across the seam
        with Poked(col, host, [m - 1, m], [host[m], host[m - 1]]):
            got = d_fingerprint(col, filt)
            assert got == vm.fingerprint_lt(src, filt), (n, off, m)
            assert not vm.verdict_scan(got[1], got, want), (n, off, m)
    out = src[src < filt]
    few = sorted({0, out.size // 2, out.size - 1} & set(range(out.size)))
    at_seams = [int(np.count_nonzero(src[:m] < filt)) for m in seams[:2] + seams[-2:]]
    for i in sorted(set(few + [j for j in at_seams if 0 < j < out.size])):
        big = np.int32(filt + i)
        for what, bad, count in (("dropped", np.delete(out, i), out.size - 1),
                                 ("duplicated", np.insert(out, i, out[i]), out.size + 1),
                                 ("element >= filter inserted", np.insert(out, i, big), out.size + 1),
                                 ("replaced", np.concatenate([out[:i], [out[i] ^ 1], out[i + 1:]]).astype(np.int32), out.size)):
            got = d_fingerprint(dev(bad, off), filt)
            assert got == vm.fingerprint_lt(bad, filt), (n, off, what, i)
            assert not vm.verdict_scan(count, got, want), (n, off, what, i)
    if out.size:
        got = d_fingerprint(dev(out, off), filt)  # accept: the right answer
        assert got == want and vm.verdict_scan(out.size, got, want)
        got = d_fingerprint(dev(out[:-1], off), filt)  # reject: last element lost
        assert got == vm.fingerprint(out[:-1]) and not vm.verdict_scan(out.size - 1, got, want)


@pytest.mark.parametrize("filt", [INT_MIN, 0, INT_MAX])
def test_fingerprint_at_the_ends_of_the_value_range(filt):
    src = np.array([INT_MAX, INT_MIN, -1, 0, INT_MAX, INT_MIN, INT_MAX - 1, INT_MIN + 1] * 40 + [INT_MIN], dtype=np.int32)
    want = vm.fingerprint_lt(src, filt)
    assert want[1] == {INT_MIN: 0, 0: 161, INT_MAX: 241}[filt]
    assert d_fingerprint(dev(src, 1), filt) == want
    out = src[src < filt]
    assert d_fingerprint(dev(out, 3), filt) == want


# ---- sorted ----------------------------------------------------------------------------------------------------------------
def _sorted_column(n, signed, rng):
    """strictly increasing in the order asked for, gaps of at least 2, from the order's smallest to its largest key"""
    x = np.cumsum(rng.integers(2, 4000, n, dtype=np.uint64)).astype(np.uint32)
    if n:
        x[0] = 0
    if n >= 2:
        x[-1] = M32
    return x ^ np.uint32(0x80000000 if signed else 0)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("label", SIZES)
def test_sorted_words_and_sort_verdict(label, signed):
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + signed)
    keys = _sorted_column(n, signed, rng)
    off = (n + signed) % 4
    col = dev(keys, off)
    want = vm.sorted_words(keys, signed)
    assert want[0] == 0 and d_sorted(col, signed) == want  # accept
    if n >= 2:  # the same column read in the other order: one descent, where the sign flips
        other = vm.sorted_words(keys, not signed)
        assert other[0] == 1 and d_sorted(col, not signed) == other
    fixed, every = positions(n, w, rng, need=2)
    mask = np.uint32(0x80000000 if signed else 0)
    for i in every:  # reject: one descent at i, counted exactly once
        up = ((keys[i + 1] ^ mask) + np.uint32(1)) ^ mask if (keys[i + 1] ^ mask) != M32 else None
        values = [up, keys[i + 1]] if up is not None else [keys[i + 1], keys[i]]
        with Poked(col, keys, [i, i + 1], values):
            got = d_sorted(col, signed)
            model = vm.sorted_words(keys, signed)
            assert got == model and model[0] == 1, (n, signed, i)
            assert not vm.verdict_sort(got, want)
    for i in fixed:
        j = (i + n // 2) % n
        if i != j and n >= 4:  # reject through the hash word: the key sum kept, +1 on one key and -1 on another
            with Poked(col, keys, [i, j], [keys[i] + np.uint32(1), keys[j] - np.uint32(1)]):
                got = d_sorted(col, signed)
                assert got == vm.sorted_words(keys, signed) and got[2] == want[2] and got[1] != want[1], (n, signed, i)
                assert not vm.verdict_sort(got, want)
        with Poked(col, keys, [i], [keys[i + 1]]):  # reject: the multiset changes, the order stands
            got = d_sorted(col, signed)
            assert got == vm.sorted_words(keys, signed) and got[0] == 0, (n, signed, i)
            assert not vm.verdict_sort(got, want)


def test_sorted_at_the_ends_of_the_key_range():
    for keys, signed, descents in (([0x7FFFFFFF, 0x80000000], False, 0), ([0x7FFFFFFF, 0x80000000], True, 1),
                                   ([0x80000000, 0x7FFFFFFF], True, 0), ([0x80000000, 0x7FFFFFFF], False, 1),
                                   ([0, M32], False, 0), ([0, M32], True, 1), ([M32, 0], True, 0), ([M32, 0], False, 1),
                                   ([M32] * 70 + [0] * 70, False, 1), ([0] * 70 + [M32] * 70, False, 0)):
        a = np.array(keys, dtype=np.uint32)
        want = vm.sorted_words(a, signed)
        assert want[0] == descents and d_sorted(dev(a, 1), signed) == want, (keys[:2], signed)


# ---- sorted pairs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("label", SIZES)
def test_sorted_pairs_words_and_verdict(label, signed):
    """sorted keys (i + 2) / 4 spread over the key range: i and i + 1 tie at every seam position (i % 4 != 1)"""
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 10 + signed)
    mask = np.uint32(0x80000000 if signed else 0)
    rank = (np.arange(n, dtype=np.uint64) + 2) // 4
    srt = (rank * (M32 // max(int(rank[-1]) if n else 1, 1))).astype(np.uint32) ^ mask
    keys_in = np.empty(n, dtype=np.uint32)
    keys_in[rng.permutation(n)] = srt
    ids = np.argsort(keys_in ^ mask, kind="stable").astype(np.uint32)
    assert np.array_equal(keys_in[ids], srt)
    d_in, d_out, d_ids = dev(keys_in, 1), dev(srt, 2), dev(ids, 3)
    assert d_sorted_pairs(d_in, d_out, d_ids, signed) == vm.sorted_pairs(keys_in, srt, ids, signed) == [0, 0]  # accept
    fixed, every = positions(n, w, rng, need=2)

    def judged(i, what):
        got = d_sorted_pairs(d_in, d_out, d_ids, signed)
        assert got == vm.sorted_pairs(keys_in, srt, ids, signed), (n, signed, i, what)
        assert not vm.verdict_sort_pairs(got), (n, signed, i, what)
        return got

    for i in every:  # reject: the two ids swapped: a tie broken the wrong way (or, off a tie, ids beside another key)
        with Poked(d_ids, ids, [i, i + 1], [ids[i + 1], ids[i]]):
            got = judged(i, "swap")
            if srt[i] == srt[i + 1]:
                assert got == [1, 0]
    for i in fixed:
        with Poked(d_ids, ids, [i], [n]):  # id == n
            assert judged(i, "id == n")[1] == 1
        other = int(ids[(i + n // 2) % n])
        if keys_in[other] != srt[i]:
            with Poked(d_ids, ids, [i], [other]):  # an id naming a row with another key
                assert judged(i, "other key")[1] == 1
        if srt[i] == srt[i + 1]:
            with Poked(d_ids, ids, [i + 1], [ids[i]]):  # an equal-key pair with equal ids
                assert judged(i, "equal ids") == [1, 0]


# ---- weighted sums and distinct keys: the hash group-by's verdict ------------------------------------------------------------
@pytest.mark.parametrize("label", SIZES)
def test_groupby_hash_words_and_verdict(label):
    """g = the size: output rows (distinct 32-bit keys, sums, counts) of 2 g input rows, two rows a group"""
    w = grid_threads()
    g = size_of(label, w)
    rng = np.random.default_rng(g + 20)
    out_keys = (np.arange(g, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(12345)).astype(np.uint32)  # a bijection
    out_keys = out_keys[rng.permutation(g)]  # accept: rows in a random order
    first = rng.integers(0, M32, g, endpoint=True).astype(np.uint32)
    second = rng.integers(0, M32, g, endpoint=True).astype(np.uint32)
    sums, counts = first + second, np.full(g, 2, dtype=np.uint32)
    rows = rng.permutation(2 * g)
    keys, vals = np.concatenate([out_keys, out_keys])[rows], np.concatenate([first, second])[rows]
    d_keys, d_vals, d_ones = dev(keys, 1), dev(vals, 2), dev(np.ones(2 * g, np.uint32), 3)
    d_ok, d_os, d_oc = dev(out_keys, 3), dev(sums, 1), dev(counts, 2)
    want_s, want_c = vm.weighted_sum(keys, vals), vm.weighted_sum(keys, np.ones(2 * g, np.uint32))
    assert d_weighted(d_keys, d_vals) == want_s and d_weighted(d_keys, d_ones) == want_c
    wts = vm.weights(out_keys)

    def verdict(tag, what, keys_changed=False):
        """the predicate of GroupByHashHip over the device's words, each word the model's"""
        s, c, d = d_weighted(d_ok, d_os), d_weighted(d_ok, d_oc), d_distinct(d_ok)
        w_now = vm.weights(out_keys) if keys_changed else wts
        model_s = vm.weighted_sum(out_keys, sums, w_now) if keys_changed or what[0].startswith("sum") else want_s
        model_c = vm.weighted_sum(out_keys, counts, w_now) if keys_changed or what[0].startswith("count") else want_c
        assert s == model_s and c == model_c, (g, what)
        assert d == (vm.distinct(out_keys) if keys_changed else [0]), (g, what)
        ok = s == want_s and c == want_c and d == [0] and vm.sum64(counts) == 2 * g
        if tag != "blind":
            assert ok == (tag == "accept"), (g, what, tag)
        return ok

    assert vm.weighted_sum(out_keys, sums, wts) == want_s and vm.weighted_sum(out_keys, counts, wts) == want_c
    verdict("accept", ("right answer",))
    fixed, every = positions(g, w, rng)
    for i in every if g <= 4096 else fixed:  # reject: single-group errors are always caught
        with Poked(d_os, sums, [i], [sums[i] + np.uint32(1)]):
            verdict("reject", ("sum + 1", i))
    if g > 4096:  # the random places of a large column in one call: many groups off by one, words that differ by the model
        at = sorted(set(every) - set(fixed))
        with Poked(d_os, sums, at, sums[at] + np.uint32(1)):
            assert vm.weighted_sum(out_keys, sums, wts) != want_s
            verdict("reject", ("sum + 1", at[:3]))
    for i in fixed:
        for d in (1 << 31, int(rng.integers(2, M32))):
            with Poked(d_os, sums, [i], [sums[i] + np.uint32(d)]):
                verdict("reject", ("sum + d", i, d))
        j = (i + g // 2) % g
        if i == j:
            continue
        if (int(sums[i]) - int(sums[j])) % 2:  # reject: two sums swapped, their difference odd
            with Poked(d_os, sums, [i, j], [sums[j], sums[i]]):
                verdict("reject", ("sums swapped", i, j))
        with Poked(d_oc, counts, [i, j], [3, 1]):  # reject: a count moved between groups
            verdict("reject", ("count moved", i, j))
        with Poked(d_os, sums, [i, j], [sums[i] + np.uint32(1 << 31), sums[j] - np.uint32(1 << 31)]):
            assert verdict("blind", ("sum: 2^31 moved", i, j))  # blind (a): both words coincide with the right answer's
    if g >= 2:  # reject through distinct: a key emitted twice with its sum split, on the first and on the last row
        for i, j in ((0, g - 1), (g - 1, 0)):
            half = np.uint32(12345)
            with Poked(d_ok, out_keys, [j], [out_keys[i]]), Poked(d_os, sums, [i, j], [half, sums[i] - half]), \
                    Poked(d_oc, counts, [i, j], [1, 1]):
                assert vm.distinct(out_keys) == [1]
                verdict("reject", ("key twice", i, j), keys_changed=True)


@pytest.mark.parametrize("label", SIZES)
def test_weighted_sum_by_index(label):
    """keys == NULL: the weight comes from the index, all 32 bits of it past the grid's width"""
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 30)
    vals = rng.integers(0, M32, n, endpoint=True).astype(np.uint32)
    col = dev(vals, n % 4)
    want = vm.weighted_sum(None, vals)
    assert d_weighted(None, col) == want
    assert d_weighted(dev(np.arange(n, dtype=np.uint32), 1), col) == want
    for i in positions(n, w, rng)[1]:
        with Poked(col, vals, [i], [vals[i] + np.uint32(1)]):
            got = d_weighted(None, col)
            assert got == vm.weighted_sum(None, vals) and got[0] != want[0] and got[1] != want[1], (n, i)
            assert not vm.verdict_groupby(got, want)


# ---- permutation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SIZES)
def test_permutation_words(label):
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 40)
    ids = rng.permutation(n).astype(np.uint32)
    col = dev(ids, (n + 1) % 4)
    assert d_permutation(col) == vm.permutation(ids) == [0]
    for at in batches(positions(n, w, rng)[1], n):
        for value in (0, n - 1, n, M32):  # an id seen before (0 and n - 1), out of range (n and 2^32 - 1)
            fresh = [i for i in at if ids[i] != value]
            with Poked(col, ids, at, [value] * len(at)):
                assert d_permutation(col) == vm.permutation(ids) == [len(fresh)], (n, at[:3], value)
    if n >= 4:  # exact counts: three ids seen before and two out of range
        with Poked(col, ids, [0, 1, 2, n - 2, n - 1], [ids[3], ids[3], ids[3], n, M32]):
            assert d_permutation(col) == vm.permutation(ids) == [5]
    if n == 1:
        assert d_permutation(dev(np.uint32([1]))) == [1]


# ---- one-to-many join ------------------------------------------------------------------------------------------------------
def _join_case(n_build, n_probe, hi, rng, generated=None):
    """(build, probe, sorted build, pos, cnt, ids): the answer with the key ranges in sorted order, ids row indices, or
    global row ids of gen_uniform(seed, 1..hi) from `first` on when generated = (seed, first)"""
    if generated:
        seed, first = generated
        build = vm.gen_value(seed, 1, hi, np.arange(n_build, dtype=np.uint64) + np.uint64(first))
    else:
        build = rng.integers(1, hi, n_build, endpoint=True).astype(np.uint32)
    probe = rng.integers(1, hi + max(hi // 4, 1), n_probe, endpoint=True).astype(np.uint32)  # a fifth of them miss
    order = np.argsort(build, kind="stable").astype(np.uint32)
    srt = build[order]
    lb = np.searchsorted(srt, probe, "left")
    cnt = (np.searchsorted(srt, probe, "right") - lb).astype(np.uint32)
    pos = np.where(cnt > 0, lb, 0).astype(np.uint32)
    ids = order + np.uint32(generated[1]) if generated else order
    return build, probe, srt, pos, cnt, ids


def _sampled_by(pos, cnt, n_build):
    """(probe row, id position) for every id a probe row reads: the first, the last and the picked one of its range"""
    hit = np.nonzero(cnt > 0)[0]
    p, c = pos[hit].astype(np.int64), cnt[hit].astype(np.int64)
    pick = vm.join_picks(cnt)[hit].astype(np.int64)
    code = np.concatenate([hit, hit, hit]) * np.int64(n_build) + np.concatenate([p, p + c - 1, p + pick])
    code = np.unique(code)
    return code // np.int64(max(n_build, 1)), code % np.int64(max(n_build, 1))


@pytest.mark.parametrize("generated", [False, True])
@pytest.mark.parametrize("label", SIZES)
def test_join_words_and_verdict(label, generated):
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 50 + generated)
    n_build = n if n % 2 else max(n // 2 + 3, 1)  # odd sizes: as many build rows; even ones: about half
    hi = max(n_build // 6, 1)
    gen = (42, 1, hi)
    first = (1 << 20) + 7
    build, probe, srt, pos, cnt, ids = _join_case(n_build, n, hi, rng, (42, first) if generated else None)
    d_build = None if generated else dev(build, 1)
    d_srt, d_probe, d_pos, d_cnt, d_ids = dev(srt, 2), dev(probe, 3), dev(pos, 1), dev(cnt, 2), dev(ids, 3)

    def judged(tag, what, ids_h=None, d_ids_=None):
        ids_h = ids if ids_h is None else ids_h
        got = d_join(d_srt, d_probe, d_pos, d_cnt, d_ids if d_ids_ is None else d_ids_, build_keys=d_build, gen=gen)
        model = vm.join(srt, probe, pos, cnt, ids_h, build_keys=None if generated else build, gen=gen)
        assert got == model, (n, generated, what)
        perm = vm.permutation(ids_h - np.uint32(first) if generated else ids_h)
        if tag != "blind":
            assert vm.verdict_join(got, perm) == (tag == "accept"), (n, generated, what, got)
        return got

    base = judged("accept", "right answer")
    assert base == [0, int(cnt.sum())]
    if n == 0:
        return
    # accept: ids shuffled inside every key's range
    shuffled = ids[np.lexsort((rng.random(n_build), srt))]
    assert judged("accept", "ids shuffled in their ranges", shuffled, dev(shuffled, 1)) == base
    # accept: the key ranges laid out in another order (descending keys), pos adjusted
    flipped = ids[::-1].copy()
    with Poked(d_pos, pos, np.nonzero(cnt)[0], (n_build - pos[cnt > 0].astype(np.int64) - cnt[cnt > 0]).astype(np.uint32)):
        assert judged("accept", "ranges in another order", flipped, dev(flipped, 2)) == base
    fixed, every = positions(n, w, rng)
    for at in batches(every, n):  # reject: a count off by one, up and down; a miss row given a count
        for delta in (1, -1):
            with Poked(d_cnt, cnt, at, cnt[at] + np.uint32(delta & M32)):
                got = judged("reject", ("count", at[:3], delta))
                assert got[0] == len(at) and got[1] == int(cnt.sum()), (n, at[:3], delta, got)
    misses = np.nonzero(cnt == 0)[0]
    at = sorted(set(misses[:4].tolist() + misses[-4:].tolist()))
    if at:  # reject: miss rows given a count, each one a bad row
        with Poked(d_cnt, cnt, at, [1] * len(at)):
            got = judged("reject", ("miss rows given a count", at))
            assert got == [len(at), base[1] + len(at)], (n, at, got)
    at = sorted(set(misses[:4].tolist() + misses[-4:].tolist()))
    if at:
        with Poked(d_pos, pos, at, [n_build - 1] * len(at)):  # blind (b): out_pos of a row without a match is not looked at
            assert judged("blind", ("miss rows with a position", at)) == base
    # a wrong id: the bad rows are exactly the probe rows that read the position, plus what the key runs say
    readers, places = _sampled_by(pos, cnt, n_build)
    up0, down0 = vm.join_runs(srt, ids, None if generated else build, gen)
    assert up0 == down0
    _, id_places = positions(n_build, w, rng)
    key_of = lambda i: build[int(ids[i]) - (first if generated else 0)]
    id_places = [at for at in id_places if key_of((at + n_build // 2) % n_build) != srt[at]]
    for at in batches(id_places, n_build):
        with Poked(d_ids, ids, at, ids[[(i + n_build // 2) % n_build for i in at]]):
            up, down = vm.join_runs(srt, ids, None if generated else build, gen)
            got = judged("reject", ("wrong id", at[:3]))
            bad_rows = np.unique(readers[np.isin(places, at)]).size
            assert got[0] == bad_rows + ((up - down) << 32) and up > down, (n, at[:3], got, bad_rows, up, down)
    # reject: two ids of different keys swapped where no probe row reads them: only the key runs tell
    unread = np.setdiff1d(np.arange(n_build), places)
    if unread.size:
        a = int(unread[0])
        others = unread[srt[unread] != srt[a]]
        if others.size:
            b = int(others[-1])
            with Poked(d_ids, ids, [a, b], [ids[b], ids[a]]):
                assert bool(vm.join_row_ok(srt, probe, pos, cnt, ids, None if generated else build, gen).all())
                assert judged("reject", ("unread ids swapped", a, b))[0] >= 1
    if generated:  # reject: the generated-id mode with a wrong seed
        got = d_join(d_srt, d_probe, d_pos, d_cnt, d_ids, build_keys=None, gen=(41, 1, hi))
        assert got == vm.join(srt, probe, pos, cnt, ids, build_keys=None, gen=(41, 1, hi))
        assert got[0] != 0 or not cnt.any() or hi < 16  # (a span of a few keys can come out alike under two seeds)


def test_join_ranges_that_leave_the_id_buffer():
    """pos + cnt past n_build, with ids a slice of a longer buffer whose tail would make the row pass: an unguarded read
    shows as acceptance, never as a fault"""
    n_build = 301
    build = np.full(n_build, 9, dtype=np.uint32)
    build[:100] = 4
    ids = np.argsort(build, kind="stable").astype(np.uint32)
    srt = build[ids]
    tail = np.full(512, n_build - 1, dtype=np.uint32)  # ids of rows that carry 9
    d_ids = dev(ids, 1, tail=tail)
    d_build, d_srt = dev(build, 2, tail=np.full(512, 9, np.uint32)), dev(srt, 3)
    probe = np.array([9, 4, 9], dtype=np.uint32)
    for pos in (n_build - 1, M32, n_build - 200, 101):
        p, c = np.array([100, 0, pos], dtype=np.uint32), np.array([201, 100, 201], dtype=np.uint32)
        got = d_join(d_srt, dev(probe), dev(p, 1), dev(c, 2), d_ids, build_keys=d_build)
        assert got == vm.join(srt, probe, p, c, ids, build_keys=build) == [1, 502], pos
        assert not vm.verdict_join(got, [0])


def test_join_sum_of_counts_above_32_bits():
    """70 000 probe rows of one key against 70 000 build rows of it: 4.9e9 matches in result[1]"""
    n = 70000
    build = np.full(n, 77, dtype=np.uint32)
    ids = np.arange(n, dtype=np.uint32)
    pos, cnt = np.zeros(n, dtype=np.uint32), np.full(n, n, dtype=np.uint32)
    got = d_join(dev(build, 1), dev(build, 2), dev(pos), dev(cnt, 3), dev(ids, 1), build_keys=dev(build))
    assert got == vm.join(build, build, pos, cnt, ids, build_keys=build) == [0, n * n] and n * n > 1 << 32


def test_join_without_build_rows():
    probe = np.arange(1, 301, dtype=np.uint32)
    zero, none = np.zeros(300, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    d_none = dev(none)
    assert d_join(d_none, dev(probe), dev(zero), dev(zero), d_none, build_keys=d_none) == [0, 0]
    cnt = zero.copy()
    cnt[[0, 299]] = 1
    got = d_join(d_none, dev(probe), dev(zero), dev(cnt), d_none, build_keys=d_none)
    assert got == vm.join(none, probe, zero, cnt, none, build_keys=none) == [2, 2]


# ---- pair table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left_outer", [False, True])
def test_join_pairs_other_orders_and_lost_pairs(left_outer):
    rng = np.random.default_rng(60 + left_outer)
    n_build, n_probe = 3001, 2 * grid_threads() // 256 + 77
    build, probe, srt, pos, cnt, ids = _join_case(n_build, n_probe, 600, rng)
    c = cnt.astype(np.int64)
    rows = np.repeat(np.arange(n_probe), c)
    at = np.repeat(pos.astype(np.int64) - (np.cumsum(c) - c), c) + np.arange(int(c.sum()))
    out_b, out_p = ids[at], rows.astype(np.uint32)
    if left_outer:
        empty = np.nonzero(cnt == 0)[0].astype(np.uint32)
        out_b, out_p = np.concatenate([out_b, np.full(empty.size, M32, np.uint32)]), np.concatenate([out_p, empty])
    order = rng.permutation(out_b.size)  # accept: the pairs in another order, the fingerprint is commutative
    out_b, out_p = out_b[order], out_p[order]
    cols = [dev(a, k % 4) for k, a in enumerate((build, probe, ids, pos, cnt))]
    d_b, d_p = dev(out_b, 1), dev(out_p, 3)

    def judged(accept, what):
        got = d_join_pairs(*cols, d_b, d_p, left_outer=left_outer)
        assert got == vm.join_pairs(build, probe, ids, pos, cnt, out_b, out_p, left_outer=left_outer), what
        assert vm.verdict_join_pairs(got, out_b.size) == accept, (what, got)

    judged(True, "another order")
    real = np.nonzero(out_b != M32)[0]
    for i, j in ((real[0], real[-1]), (real[-1], real[real.size // 2])):  # reject: a pair duplicated, another dropped
        with Poked(d_b, out_b, [i], [out_b[j]]), Poked(d_p, out_p, [i], [out_p[j]]):
            judged(False, ("duplicated and dropped", i, j))
    for i in (real[0], real[-1]):  # reject: a left-outer sentinel on a row that has matches
        with Poked(d_b, out_b, [i], [M32]):
            judged(False, ("sentinel on a matching row", i))


# ---- unique-key join -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SIZES)
def test_ujoin_words_and_verdict(label):
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 70)
    n_build = max(n // 2, 1)
    bk = np.unique(np.concatenate([rng.integers(0, M32, n_build).astype(np.uint32), np.uint32([0, M32 - 1])]))
    bv = rng.integers(0, M32, bk.size).astype(np.uint32)
    pk = rng.integers(0, M32, n, endpoint=True).astype(np.uint32)
    some = rng.random(n) < 0.6
    pk[some] = rng.choice(bk, int(some.sum()))
    if n >= 4:
        pk[[0, 1, n - 1, n - 2]] = [bk[0], M32, bk[-1], M32]  # first and last build key; the sentinel as a probe key
    pv = rng.integers(0, M32, n).astype(np.uint32)
    at = np.minimum(np.searchsorted(bk, pk), bk.size - 1)
    hit = bk[at] == pk
    outs = [np.where(hit, col, np.uint32(M32)).astype(np.uint32) for col in (pk, bv[at], pv)]
    d_in = [dev(a, k % 4) for k, a in enumerate((bk, bv, pk, pv))]
    d_out = [dev(a, (k + 1) % 4) for k, a in enumerate(outs)]
    want = [0, int(hit.sum())]
    assert d_ujoin(*d_in, *d_out) == vm.ujoin(bk, bv, pk, pv, *outs) == want  # accept

    def judged(bad, what):
        got = d_ujoin(*d_in, *d_out)
        assert got == vm.ujoin(bk, bv, pk, pv, *outs) == [bad, want[1]], (n, what)
        assert not vm.verdict_ujoin(got)

    _, every = positions(n, w, rng)
    for at in batches([i for i in every if hit[i]], n):
        for c in range(3):  # each of the three output columns wrong on a hit
            with Poked(d_out[c], outs[c], at, outs[c][at] ^ np.uint32(1)):
                judged(len(at), ("column", c, at[:3]))
        sentinels = [M32] * len(at)
        with Poked(d_out[0], outs[0], at, sentinels), Poked(d_out[1], outs[1], at, sentinels), \
                Poked(d_out[2], outs[2], at, sentinels):
            judged(len(at), ("hit written as a miss", at[:3]))
    for at in batches([i for i in every if not hit[i] and pk[i] != M32], n):
        with Poked(d_out[0], outs[0], at, pk[at]):  # a miss carrying a real key
            judged(len(at), ("miss with its key", at[:3]))


# ---- generator and routing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SIZES)
def test_gen_uniform_and_route_words(label):
    w = grid_threads()
    n = size_of(label, w)
    rng = np.random.default_rng(n + 80)
    _, every = positions(n, w, rng)
    for seed, lo, hi, first in ((42, 1, 10000, 0), (43, 0, M32, (1 << 33) + 12345), (44, 777, 777, 5), (45, 3, 1 << 31, 1 << 40)):
        col = vm.gen_value(seed, lo, hi, np.arange(n, dtype=np.uint64) + np.uint64(first))
        d_col = dev(col, (n + seed) % 4)
        assert d_gen(d_col, seed, lo, hi, first) == vm.gen_uniform(col, seed, lo, hi, first) == [0]
        assert d_gen(d_col, seed + 1, lo, hi, first) == vm.gen_uniform(col, seed + 1, lo, hi, first)
        for at in batches(every, n):
            with Poked(d_col, col, at, col[at] + np.uint32(1)):
                assert d_gen(d_col, seed, lo, hi, first) == vm.gen_uniform(col, seed, lo, hi, first) == [len(at)], (n, seed, at[:3])
    where = rng.permutation(n).astype(np.uint32) + np.uint32(1000)  # the values of given indices, in any order
    col = vm.gen_value(42, 0, n, where)
    d_col, d_where = dev(col, 1), dev(where, 2)
    assert d_gen(d_col, 42, 0, n, indices=d_where) == vm.gen_uniform(col, 42, 0, n, indices=where) == [0]
    for at in batches(every, n):
        with Poked(d_where, where, at, where[at] + np.uint32(1)):
            assert d_gen(d_col, 42, 0, n, indices=d_where) == vm.gen_uniform(col, 42, 0, n, indices=where), (n, at[:3])
    keys = rng.integers(0, M32, n, endpoint=True).astype(np.uint32)
    for parts in (1, 3, 1024):
        dest = vm.dest_of(keys, parts)
        rank = int(dest[0]) if n else 0
        mine = keys[dest == rank]  # what rank `rank` receives: only its own keys
        d_mine = dev(mine, parts % 4)
        assert d_route(d_mine, parts, rank) == vm.pjoin_route(mine, parts, rank) == [0]
        assert d_route(dev(keys, 1), parts, rank) == vm.pjoin_route(keys, parts, rank)
        strangers = keys[dest != rank]
        if parts > 1 and mine.size and strangers.size:
            for i in positions(mine.size, w, rng)[1]:  # one key of another rank at each seam
                with Poked(d_mine, mine, [i], [strangers[i % strangers.size]]):
                    assert d_route(d_mine, parts, rank) == vm.pjoin_route(mine, parts, rank) == [1], (n, parts, i)
