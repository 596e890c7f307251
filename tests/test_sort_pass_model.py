"""The columns of tests/test_gpu_sort_passes.py reach the paths they are named for (CPU only, numpy only).

For every column the GPU test sorts — every (pass set, style, base) of tests/sort_pass_testlib.columns at every (digit
width, size), the reused-plan columns and the front-door columns — the sort's plan restated in numpy
(executed_passes: a pass runs iff its digit of key ^ xor_mask takes more than one value) executes exactly the
intended passes, in either order; the column holds duplicate keys whenever it must, so that the result rests on the
tie order; and where the sign bit varies the signed and the unsigned stable orders differ, so that a sort that drops
the sign flip cannot pass."""
import numpy as np
import pytest

from tests import sort_pass_testlib as sp


def _popcount(x):
    return bin(x).count("1")


def test_vary_masks():
    assert sp.vary_mask_for((0, 1, 2, 3), 8, "whole") == 0xFFFFFFFF == sp.vary_mask_for(range(8), 4, "whole")
    assert sp.vary_mask_for((2,), 8, "whole") == 0x00FF0000 and sp.vary_mask_for((0, 3), 8, "whole") == 0xFF0000FF
    assert sp.vary_mask_for((0, 3), 8, "low bit") == 0x01000001 and sp.vary_mask_for((0, 3), 8, "high bit") == 0x80000080
    assert sp.vary_mask_for((7,), 4, "high bit") == 0x80000000 and sp.vary_mask_for((7,), 4, "low bit") == 0x10000000
    assert sp.vary_mask_for((1, 6), 4, "whole") == 0x0F0000F0 and sp.vary_mask_for((), 4, "whole") == 0
    assert sp.passes_of(0xA5, 4) == (0, 2, 5, 7) and sp.passes_of(0x9, 8) == (0, 3)


def test_bases_have_no_zero_and_no_all_ones_nibble():
    for base in sp.BASES:
        assert all(0 < (base >> s) & 0xF < 0xF for s in range(0, 32, 4)), hex(base)
    assert sp.BASE >> 31 == 0 and sp.BASE_NEG >> 31 == 1
    # a constant nibble beside a varying one of the same byte: both nibbles of every byte differ from 0 and 0xF, so
    # neither a dropped shift nor a whole-byte digit reads the same


def test_keys_for_forces_both_values_of_every_varying_bit():
    for mask in (0, 1, 0x80000000, 0x00F00F00, 0xFFFFFFFF):
        for n in (0, 1, 2, 3, 1000):
            keys = sp.keys_for(mask, n, 5, sp.BASE_NEG)
            assert keys.dtype == np.uint32 and keys.size == n
            assert not np.any((keys ^ np.uint32(sp.BASE_NEG)) & np.uint32(~mask & 0xFFFFFFFF))  # nothing else varies
            if n >= 2:
                assert int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys)) == mask
    assert np.array_equal(sp.keys_for(0xFF00, 100, 7), sp.keys_for(0xFF00, 100, 7))
    assert not np.array_equal(sp.keys_for(0xFF00, 100, 7), sp.keys_for(0xFF00, 100, 8))


def test_executed_passes_on_known_columns():
    full = np.random.default_rng(1).integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    for signed in (False, True):
        assert sp.executed_passes(full, 8, signed) == (0, 1, 2, 3) and sp.executed_passes(full, 4, signed) == tuple(range(8))
        assert sp.executed_passes(np.full(10, 0x80000007, np.uint32), 8, signed) == ()
        assert sp.executed_passes(np.array([5], np.uint32), 4, signed) == ()
        assert sp.executed_passes(np.array([0x00000100, 0x80000100], np.uint32), 8, signed) == (3,)
        assert sp.executed_passes(np.array([0x00000110, 0x00000120], np.uint32), 4, signed) == (1,)
        assert sp.executed_passes(np.array([0x00000110, 0x00000120], np.uint32), 8, signed) == (0,)


def test_the_sizes_restate_the_launch_paths():
    """tiles of 8192 keys, one workgroup up to one tile, the scatter's own prefix sum up to 32 chunks, one tile per chunk
    below the chunk target of either digit width (radix.hip rs_geometry, kRsFusedScanChunks)"""
    for bits in (4, 8):
        chunks = [sp.geometry(n, bits)[2] for n in sp.SIZES]
        assert chunks == [1, 1, 13, 34]
        assert all(sp.geometry(n, bits)[1] == 1 for n in sp.SIZES)
    assert sp.SIZES[0] < sp.TILE == sp.SIZES[1] < sp.SIZES[2]               # one workgroup, ragged and full
    assert 1 < sp.geometry(sp.SIZES[2], 8)[2] <= sp.FUSED_SCAN_CHUNKS < sp.geometry(sp.SIZES[3], 8)[2]
    assert all(n % sp.TILE and n % 4 for n in sp.SIZES[2:])  # a ragged last tile, a ragged last 16-byte vector
    assert sp.CHUNKED_SIZE == sp.SIZES[3]


def test_the_pass_set_lists_are_whole():
    for n in sp.SIZES:
        assert sp.pass_sets(8, n) == tuple(range(1, 16))
    for n in sp.SIZES[:3]:
        assert sp.pass_sets(4, n) == tuple(range(1, 256))
    chunked = sp.pass_sets(4, sp.CHUNKED_SIZE)
    assert len(chunked) >= 20 and len(set(chunked)) == len(chunked)
    assert set(chunked) >= {1 << p for p in range(8)} | {0x55, 0xAA, 0x0F, 0xF0, 0x81, 0x7E, 0xFE, 0x7F, 0xFF, 0x18, 0xC3, 0x24}
    # the parts cover every set once
    for bits in (4, 8):
        for n in sp.SIZES:
            seen = [c[0] for part in sp.parts(bits, n) for c in sp.columns(bits, n, part)]
            assert seen == [s for s in sp.pass_sets(bits, n) for _ in range(2)]
    assert len(sp.cases()) == 4 + 3 * 8 + 1


@pytest.mark.parametrize("bits,n", [(bits, n) for bits in (8, 4) for n in sp.SIZES])
def test_both_one_bit_styles_and_both_bases_at_every_pass_position(bits, n):
    seen = set()
    for part in sp.parts(bits, n):
        cols = sp.columns(bits, n, part)
        for (set_mask, style, base, _, _), (set_mask2, style2, base2, _, _) in zip(cols[::2], cols[1::2]):
            assert set_mask == set_mask2 and style == "whole" and style2 in sp.STYLES[1:] and base != base2
            for p in sp.passes_of(set_mask, bits):
                seen |= {(p, style, base), (p, style2, base2), (p, "one bit", base2)}
    for p in range(32 // bits):
        for base in sp.BASES:
            assert (p, "whole", base) in seen and (p, "one bit", base) in seen, (p, hex(base))
        assert {b for b in sp.BASES if (p, "low bit", b) in seen} and {b for b in sp.BASES if (p, "high bit", b) in seen}, p


def _check_column(keys, want_passes, bits, vary_mask, what):
    n = keys.size
    for signed in (False, True):
        assert sp.executed_passes(keys, bits, signed) == tuple(want_passes), (what, signed)
    if 2 ** _popcount(vary_mask) < n:
        assert np.unique(keys).size < n, what
    assert np.unique(keys).size <= 2 ** _popcount(vary_mask), what
    if vary_mask >> 31:
        unsigned, signed = np.argsort(keys, kind="stable"), np.argsort(keys.view(np.int32), kind="stable")
        assert not np.array_equal(unsigned, signed), what
        assert not np.array_equal(keys[unsigned], keys[signed]), what


@pytest.mark.parametrize("bits,n,part", sp.cases())
def test_every_column_executes_its_pass_set(bits, n, part):
    cols = sp.columns(bits, n, part)
    assert cols
    for set_mask, style, base, vary_mask, seed in cols:
        want = sp.passes_of(set_mask, bits)
        assert vary_mask == sp.vary_mask_for(want, bits, style)
        keys = sp.keys_for(vary_mask, n, seed, base)
        _check_column(keys, want, bits, vary_mask, (bits, n, hex(set_mask), style, hex(base)))
        if style != "whole":  # two values per executed digit: far more rows than distinct keys
            assert np.unique(keys).size == 2 ** len(want) or n < 4 * 2 ** len(want)


def test_the_reused_plan_columns_and_the_front_door_columns():
    for n in sp.SIZES:
        cols = sp.reuse_columns(n)
        assert [s for s, _ in cols] == [(3,), (0, 2), (1, 2, 3), (), (1,), (0, 1, 2, 3)]
        for byte_set, keys in cols:
            mask = sp.vary_mask_for(byte_set, 8, "whole")
            _check_column(keys, byte_set, 8, mask, ("reuse", n, byte_set))
            nibbles = tuple(q for p in byte_set for q in (2 * p, 2 * p + 1))
            _check_column(keys, nibbles, 4, mask, ("reuse, 4-bit", n, byte_set))
    (top_name, top), (low_name, low) = sp.front_door_columns()
    _check_column(top, (3,), 8, 0xFF000000, top_name)
    _check_column(low, (1,), 8, 0x0000FF00, low_name)
    assert top.size == low.size == 100003
