"""The numpy model of the HyperLogLog sketch (tests/hll_model.py) against the format's promises, without a GPU: the sketch is
a function of the SET of key tuples, merge is the build of the union and accumulate is merge, the estimate keeps within four
standard errors of the truth on every key kind the format must not be fooled by, and the empty sketch gives exactly 0.0.

The accuracy condition: |estimate - n| <= 4 * 1.04 / sqrt(m) * n for p in {4, 8, 11, 14}, seeds 0 and 0xDEADBEEF, the key
kinds random, dense 1..n, stride 4096, high bits only (i << 12) and the column pair (i % 1000, i // 1000), and n in
{1, 10, 100, 10^3, 10^4, 10^5, 10^6, 4 * 10^6} (the stride and high-bit kinds up to 2^20: beyond it their 32-bit keys repeat).
The bound is the standard error of the estimator (Flajolet et al. 2007: 1.04 / sqrt(m)) times four; a wrong shift in the
placement or a 32-bit clz breaks it by far more."""
import math

import numpy as np
import pytest

from tests import hll_model as hm

U, W, B = np.uint32, np.uint64, np.uint8
PS = (4, 8, 11, 14)
SEEDS = (0, 0xDEADBEEF)
KINDS = ("random", "dense", "stride", "high bits", "pairs")
COUNTS = (1, 10, 100, 10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6, 4 * 10 ** 6)
CAPPED = 1 << 20


def key_columns(kind, n):
    """the first n rows of a kind: row i depends on i alone, so a smaller n is a prefix"""
    i = np.arange(n, dtype=np.uint64)
    if kind == "random":  # distinct by construction: a bijection of the row number
        return [hm.fmix32(((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(U) ^ U(0x1234567))]
    if kind == "dense":
        return [(i + np.uint64(1)).astype(U)]
    if kind == "stride":
        return [(i * np.uint64(4096)).astype(U)]
    if kind == "high bits":
        return [(i << np.uint64(12)).astype(U)]
    return [(i % np.uint64(1000)).astype(U), (i // np.uint64(1000)).astype(U)]


def test_unmix_inverts_fmix_and_clz_counts():
    x = np.r_[np.array([0, 1, 0x80000000, 0xFFFFFFFF], U), np.random.default_rng(1).integers(0, 1 << 32, 5000, dtype=np.uint64).astype(U)]
    assert np.array_equal(hm.fmix32(hm.unmix32(x)), x) and np.array_equal(hm.unmix32(hm.fmix32(x)), x)
    w = np.array([0, 1, 2, 3, 0xFFFFFFFF, 1 << 32, (1 << 32) - 1, 1 << 63, (1 << 64) - 1, (1 << 53) + 1, (1 << 63) - 1], W)
    assert [int(v) for v in hm.clz64(w)] == [64 - int(v).bit_length() for v in w]
    r = np.random.default_rng(2).integers(0, 1 << 64, 5000, dtype=W) >> np.random.default_rng(3).integers(0, 64, 5000).astype(W)
    assert [int(v) for v in hm.clz64(r)] == [64 - int(v).bit_length() for v in r]


def test_the_sketch_is_a_function_of_the_tuple_set():
    rng = np.random.default_rng(4)
    for p in (4, 11, 14):
        for k in (1, 2, 4):
            base = [rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(U) for _ in range(k)]
            want, hist, st = hm.build(base, p, 9)
            assert st == 0 and int(hist.sum()) == 1 << p and np.array_equal(hist, hm.histogram(want))
            order = rng.permutation(3000)
            again = np.r_[order, rng.integers(0, 3000, 5000)]  # another order, with duplicates
            assert np.array_equal(hm.build([c[again] for c in base], p, 9)[0], want)
            assert np.array_equal(hm.build(base, p, 9, rows=again.astype(U))[0], want)  # through a list: the same set
            assert not np.array_equal(hm.build(base, p, 10)[0], want)                   # the seed matters
            if k > 1:
                assert not np.array_equal(hm.build(base[::-1], p, 9)[0], want)          # and the order of the columns
                assert not np.array_equal(hm.build(base[:-1], p, 9)[0], want)           # and every column
    # one column: distinct keys never share x, so n keys offer n distinct (idx, w) pairs
    keys = np.arange(1 << 16, dtype=U)
    h, g = hm.hash_tuples(keys, 77)
    assert np.unique((h.astype(W) << W(32)) | g.astype(W)).size == keys.size


def test_merge_is_the_build_of_the_union_and_accumulate_is_merge():
    rng = np.random.default_rng(5)
    for p in PS:
        a = [rng.integers(0, 1 << 20, 4000, dtype=np.uint64).astype(U) for _ in range(2)]
        b = [rng.integers(0, 1 << 20, 9000, dtype=np.uint64).astype(U) for _ in range(2)]
        ra, rb = hm.build(a, p, 3)[0], hm.build(b, p, 3)[0]
        union = hm.build([np.r_[x, y] for x, y in zip(a, b)], p, 3)
        merged = hm.merge(ra, rb, p)
        assert merged[2] == 0 and np.array_equal(merged[0], union[0]) and np.array_equal(merged[1], union[1])
        acc = hm.build(b, p, 3, flags=hm.ACCUMULATE, before=ra)
        assert acc[2] == 0 and np.array_equal(acc[0], union[0]) and np.array_equal(acc[1], union[1])
        assert np.array_equal(hm.merge(ra, ra, p)[0], ra) and np.array_equal(hm.build(b, p, 3, before=ra)[0], rb)
        # a stored byte above q+1 counts as q+1 and raises
        spoiled = ra.copy()
        spoiled[[0, 5]] = [64 - p + 2, 255]
        out, hist, st = hm.merge(rb, spoiled, p)
        assert st == hm.KEY_RANGE and out[0] == out[5] == 64 - p + 1 and int(hist.sum()) == 1 << p and not hist[64 - p + 2:].any()
        out, hist, st = hm.build(b, p, 3, flags=hm.ACCUMULATE, before=spoiled)
        assert st == hm.KEY_RANGE and out[5] == 64 - p + 1 and hm.estimate(hist, p) > 0


@pytest.fixture(scope="module")
def hashed():
    """(h, g) of the largest column of every (kind, seed), once"""
    out = {}
    for kind in KINDS:
        cols = key_columns(kind, CAPPED if kind in ("stride", "high bits") else COUNTS[-1])
        if kind != "pairs":
            assert np.unique(cols[0]).size == cols[0].size  # the truth is n
        for seed in SEEDS:
            out[kind, seed] = hm.hash_tuples(cols, seed)
    return out


@pytest.mark.parametrize("p", PS)
def test_the_estimate_keeps_within_four_standard_errors(hashed, p):
    bound = 4 * hm.relative_error(p)
    assert bound == 4 * 1.04 / math.sqrt(1 << p)
    worst = (0.0, None)
    for (kind, seed), (h, g) in hashed.items():
        idx, rank = hm.place(h, g, p)
        registers, done = np.zeros(1 << p, B), 0
        for n in COUNTS:
            if n > h.size:
                continue
            hm.offer(registers, idx[done:n], rank[done:n])  # the rows 0 .. n: a prefix of the kind
            done = n
            e = hm.estimate(hm.histogram(registers), p)
            err = abs(e - n) / n
            worst = max(worst, (err / hm.relative_error(p), (kind, seed, n, e)))
            assert err <= bound, f"p = {p}, {kind}, seed {seed:#x}, n = {n}: estimate {e:.1f}, {err / hm.relative_error(p):.2f} standard errors"
    print(f"p = {p}: the worst case is {worst[0]:.2f} standard errors at {worst[1]}")


def test_the_prefix_walk_is_the_build():
    for kind in KINDS:
        cols = key_columns(kind, 10 ** 4)
        registers = hm.build(cols, 11, 0xDEADBEEF)[0]
        idx, rank = hm.place(*hm.hash_tuples(cols, 0xDEADBEEF), 11)
        assert np.array_equal(hm.offer(np.zeros(1 << 11, B), idx, rank), registers)
        slow = np.zeros(1 << 11, B)
        np.maximum.at(slow, idx, rank)
        assert np.array_equal(slow, registers)


def short_rank(h, p):
    """the classic mistake: a 32-bit clz of what is left of h, the g half ignored"""
    hp = h << U(p)
    return np.where(hp == 0, 32 - p + 1, hm.clz64(hp.astype(W)) - 32 + 1).astype(B)


def test_a_wrong_shift_misses_the_condition_and_a_32_bit_clz_the_built_keys():
    """the checks have teeth: a rank taken from x instead of x << p leaves the condition by far; a 32-bit clz is right on
    all but one ordinary key in 2^(32 - p) and wrong on every key built against the hash (hll_model.keys_ranked_by_g)"""
    p, n = 14, 10 ** 6
    h, g = hm.hash_tuples(key_columns("dense", n), 0)
    idx, rank = hm.place(h, g, p)
    x = (h.astype(W) << W(32)) | g.astype(W)
    unshifted = np.minimum(hm.clz64(x) + 1, 64 - p + 1).astype(B)
    e = hm.estimate(hm.histogram(hm.offer(np.zeros(1 << p, B), idx, unshifted)), p)
    assert abs(e - n) / n > 4 * hm.relative_error(p), e
    assert float((short_rank(h, p) == rank).mean()) > 0.99
    keys = hm.keys_ranked_by_g(5000, p, 7)
    hk, gk = hm.hash_tuples(keys, 7)
    assert not (hk << U(p)).any() and np.unique(keys).size > 4000
    true_rank = hm.place(hk, gk, p)[1]
    assert int(true_rank.min()) >= 32 - p + 1 and np.unique(true_rank).size > 5
    assert (short_rank(hk, p) == 32 - p + 1).all() and float((short_rank(hk, p) == true_rank).mean()) < 0.6


def test_the_empty_sketch_gives_exactly_zero_and_refusals_minus_one():
    for p in range(hm.MIN_P, hm.MAX_P + 1):
        registers, hist, st = hm.build(np.zeros(0, U), p)
        assert st == 0 and not registers.any() and hist[0] == 1 << p
        assert hm.estimate(hist, p) == 0.0
        assert math.isinf(hm.estimate(hm.histogram(np.full(1 << p, 64 - p + 1, B)), p))
        one = hm.build(np.array([5], U), p)[1]
        assert 0.9 < hm.estimate(one, p) < 1.1
        bad = hist.copy()
        bad[0] -= 1
        assert hm.estimate(bad, p) == -1.0
        bad[64 - p + 2] = 1
        assert hm.estimate(bad, p) == -1.0
    assert hm.estimate([16] + [0] * 63, 3) == -1.0 and hm.estimate([1 << 15] + [0] * 63, 15) == -1.0
    assert hm.relative_error(12) == 1.04 / 64
