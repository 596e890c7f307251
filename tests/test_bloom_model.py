"""The numpy model of the Bloom filter (tests/bloom_model.py) against the properties the format promises
(dwarf_bench_amd/host/bloom_filter.hpp): no false negatives on any kind of key, a filter that is a function of the key set,
accumulation, and the false-positive and fill rates of one word and four bits per key.  The rates are conditions on the
model alone; simulated beforehand they came out at 3.3 % (8 bits per key), 0.53 % (16) and a fill of 0.217 (16)."""
import numpy as np
import pytest

from dwarf_bench_amd import bloom_native as bl
from tests import bloom_model as blm
from tests import fuzz_testlib as fz

U = np.uint32
assert (blm.ACCUMULATE, blm.NEGATE) == (bl.ACCUMULATE, bl.NEGATE)  # the model speaks the binding's flags


@pytest.mark.parametrize("kind", range(fz.KEY_KINDS))
def test_no_false_negatives_on_every_kind_of_key(kind):
    rng = np.random.default_rng(100 + kind)
    for n, bits, seed in ((1, 1, 0), (1000, 2, 7), (5000, 8, 12345), (1 << 14, 16, 0xFFFFFFFF)):
        keys = fz.keys(rng, n, kind)
        filt, status = blm.build(keys, blm.words(n, bits), seed)
        assert status == 0 and bool(blm.may_hold(filt, keys, seed).all()), (kind, n, bits)
        rows, count, status = blm.probe(filt, keys, seed)
        assert count == n and status == 0 and np.array_equal(rows, np.arange(n, dtype=U))
        assert blm.probe(filt, keys, seed, flags=blm.NEGATE)[1] == 0


def test_build_does_not_depend_on_order_or_duplicates():
    rng = np.random.default_rng(5)
    keys = fz.keys(rng, 3000, 1)
    want, _ = blm.build(keys, 700, 9)
    assert np.array_equal(blm.build(rng.permutation(keys), 700, 9)[0], want)
    assert np.array_equal(blm.build(np.r_[keys, keys[::3], keys[:17]], 700, 9)[0], want)
    rows = rng.integers(0, keys.size, 20000).astype(U)  # through a list that repeats rows and misses some
    listed, status = blm.build(keys, 700, 9, rows=rows)
    assert status == 0 and np.array_equal(listed, blm.build(keys[np.unique(rows)], 700, 9)[0])
    assert not np.array_equal(blm.build(keys, 700, 10)[0], want)  # the seed is part of the placement


def test_accumulating_two_halves_is_one_build():
    rng = np.random.default_rng(6)
    keys = fz.keys(rng, 4001, 1)
    want, _ = blm.build(keys, 1000, 3)
    first, _ = blm.build(keys[:2000], 1000, 3, before=np.full(1000, 0x5A5A5A5A5A5A5A5A, np.uint64))  # a clearing build
    both, _ = blm.build(keys[2000:], 1000, 3, flags=blm.ACCUMULATE, before=first)
    assert np.array_equal(both, want) and not np.array_equal(first, want)
    # count, a list with ids outside the column, and the status
    got, status = blm.build(keys, 1000, 3, count=2000)
    assert status == 0 and np.array_equal(got, first)
    got, status = blm.build(keys, 1000, 3, rows=np.array([5, 4001, 0xFFFFFFFF, 5, 7], U), count=4)
    assert status == blm.KEY_RANGE and np.array_equal(got, blm.build(keys[5:6], 1000, 3)[0])
    rows, count, status = blm.probe(got, keys, 3, rows=np.array([7, 5, 4001, 5, 6], U), count=4)
    assert status == blm.KEY_RANGE and count == rows.size and [int(r) for r in rows] == [5, 5]


@pytest.mark.parametrize("seed", (0, 12345))
@pytest.mark.parametrize("bits,under", ((8, 0.05), (16, 0.01)))
def test_false_positive_rate(seed, bits, under):
    rng = np.random.default_rng(seed + bits)
    drawn = np.unique(rng.integers(0, 1 << 32, (1 << 16) + (1 << 18) + 4096, dtype=np.uint64).astype(U))
    drawn = rng.permutation(drawn)
    keys, absent = drawn[: 1 << 16], drawn[1 << 16: (1 << 16) + (1 << 18)]
    assert keys.size == 1 << 16 and absent.size == 1 << 18
    filt, _ = blm.build(keys, blm.words(keys.size, bits), seed)
    assert bool(blm.may_hold(filt, keys, seed).all())
    rate = float(blm.may_hold(filt, absent, seed).mean())
    print(f"bits per key {bits}, seed {seed}: false-positive rate {rate:.4%}")
    assert rate < under
    if bits == 16:
        fill = float(np.unpackbits(filt.view(np.uint8)).mean())
        print(f"fill at 16 bits per key: {fill:.4f}")
        assert 0.19 <= fill <= 0.24
