"""tests/bitpack_model.py against a loop that moves one bit at a time: the format (bit positions, little-endian words, the
zero padding to whole 16-byte chunks), the base's wrap-around, the rows that do not fit, the words pack leaves alone, the
take through a list and the range filter.  No GPU, no library."""
import numpy as np
import pytest

from tests import bitpack_model as bm

U = np.uint32
ROWS = (0, 1, 31, 32, 33, 127, 128, 129, 4097)


def slow_words(n, width):
    return (-(-(n * width) // 32) + 3) // 4 * 4


def slow_pack(codes, width):
    words = [0] * slow_words(len(codes), width)
    for i, c in enumerate(codes):
        for k in range(width):
            at = i * width + k
            words[at // 32] |= ((int(c) >> k) & 1) << (at % 32)
    return np.array(words, dtype=np.uint64).astype(U)


def slow_extract(words, i, width):
    return sum(((int(words[(i * width + k) // 32]) >> ((i * width + k) % 32)) & 1) << k for k in range(width))


@pytest.mark.parametrize("width", range(1, 33))
def test_round_trip_of_every_width_at_every_row_count(width):
    rng = np.random.default_rng(width)
    for n in ROWS:
        codes = rng.integers(0, 1 << width, n, dtype=np.uint64).astype(U)
        packed = bm.pack_codes(codes, width)
        assert packed.dtype == U and packed.size == bm.words(n, width) == slow_words(n, width) and packed.size % 4 == 0
        if n <= 129:
            assert np.array_equal(packed, slow_pack(codes, width))
        assert all(slow_extract(packed, i, width) == int(codes[i]) for i in range(0, n, max(1, n // 64)))
        assert np.array_equal(bm.unpack_codes(packed, n, width), codes)
        # every bit from n * width on is zero, so equal rows give equal bytes
        bits = np.unpackbits(packed.view(np.uint8), bitorder="little")
        assert not bits[n * width:].any()
        for ones in (np.zeros(n, U), np.full(n, bm.mask(width), U)):
            again = bm.pack_codes(ones, width)
            assert np.array_equal(bm.unpack_codes(again, n, width), ones)
            assert not np.unpackbits(again.view(np.uint8), bitorder="little")[n * width:].any()


def test_words_query():
    for width in range(1, 33):
        for n in ROWS + ((1 << 32) - 1,):
            assert bm.words(n, width) == slow_words(n, width)
        assert bm.words(1 << 32, width) == 0
    assert bm.words(5, 0) == bm.words(5, 33) == 0 and bm.words(32, 12) == 12 and bm.words(128, 12) == 48
    assert bm.words((1 << 26), 12) * 4 == 96 << 20  # the issue's column: 96 MiB against 256


def test_base_wraps_and_signed_columns_need_nothing_special():
    rng = np.random.default_rng(3)
    col = (rng.integers(-50, 50, 200)).astype(np.int32).view(U)  # int32 values around zero: bit patterns at both ends
    base = int(col.view(np.int32).min()) & 0xFFFFFFFF
    packed, status = bm.pack(col, 7, base)
    assert status == 0 and np.array_equal(bm.decode(packed, 200, 7, base), col)
    assert np.array_equal(bm.unpack_codes(packed, 200, 7), col - U(base))
    # a base above the values: v - base wraps to codes that fit only at width 32
    packed, status = bm.pack(np.array([5, 6, 7], U), 32, 0xFFFFFFF0)
    assert status == 0 and np.array_equal(bm.unpack_codes(packed, 3, 32), np.array([21, 22, 23], U))
    assert np.array_equal(bm.decode(packed, 3, 32, 0xFFFFFFF0), np.array([5, 6, 7], U))
    packed, status = bm.pack(np.array([0xFFFFFFF5, 2], U), 5, 0xFFFFFFF0)  # 5 and 18 (wrapped) fit in five bits
    assert status == 0 and np.array_equal(bm.decode(packed, 2, 5, 0xFFFFFFF0), np.array([0xFFFFFFF5, 2], U))


def test_a_row_that_does_not_fit_keeps_its_low_bits_and_raises():
    col = np.array([1, 2, 300, 4, 0xFFFFFFFF], U)  # the last one: DBENCH_DICT_MISS
    packed, status = bm.pack(col, 8)
    assert status == bm.KEY_RANGE and np.array_equal(bm.unpack_codes(packed, 5, 8), np.array([1, 2, 300 & 255, 4, 255], U))
    assert bm.pack(col[:2], 8)[1] == 0 and bm.pack(col, 32)[1] == 0


def test_pack_writes_exactly_the_words_of_its_count():
    rng = np.random.default_rng(9)
    col = rng.integers(0, 1 << 12, 1000, dtype=np.uint64).astype(U)
    before = np.full(bm.words(1000, 12), 0x5A5A5A5A, U)
    for count, m in ((None, 1000), (0, 0), (1, 1), (333, 333), (1000, 1000), (1 << 40, 1000)):
        out, status = bm.pack(col, 12, count=count, before=before)
        w = bm.words(m, 12)
        assert status == 0 and np.array_equal(out[:w], bm.pack_codes(col[:m], 12)) and (out[w:] == 0x5A5A5A5A).all()


def test_take_through_a_list_and_the_filter():
    rng = np.random.default_rng(5)
    n, width, base = 500, 9, 1000
    col = (rng.integers(0, 1 << width, n, dtype=np.uint64) + base).astype(U)
    packed, _ = bm.pack(col, width, base)
    rows = np.r_[rng.integers(0, n, 50), [n, bm.NO_ROW, 0]].astype(U)
    out, status = bm.unpack(packed, n, width, base, rows=rows, fill=77)
    assert status == bm.KEY_RANGE and np.array_equal(out[:50], col[rows[:50]]) and list(out[50:]) == [77, 77, col[0]]
    assert bm.unpack(packed, n, width, base, rows=rows[51:], flags=bm.OUTER, fill=77)[1] == 0
    out, status = bm.unpack(packed, n, width, base, rows=rows, count=10, before=np.full(53, 9, U))
    assert status == 0 and np.array_equal(out[:10], col[rows[:10]]) and (out[10:] == 9).all()
    assert np.array_equal(bm.unpack(packed, n, width, base)[0], col)
    got, status = bm.select_range(packed, n, width, base, 1100, 1200)
    assert status == 0 and np.array_equal(got, np.nonzero((col >= 1100) & (col <= 1200))[0])
    got, status = bm.select_range(packed, n, width, base, 1100, 1200, flags=bm.NEGATE)
    assert np.array_equal(got, np.nonzero(~((col >= 1100) & (col <= 1200)))[0])
    got, status = bm.select_range(packed, n, width, base, 1100, 1200, rows=rows)
    want = [r for r in rows if r < n and 1100 <= col[r] <= 1200]
    assert status == bm.KEY_RANGE and list(got) == want
    assert bm.select_range(packed, n, width, base, 5, 4)[0].size == 0
    signed = np.array([-3, -1, 0, 2], np.int32).view(U)
    sp, _ = bm.pack(signed, 3, 0xFFFFFFFD)
    assert list(bm.select_range(sp, 4, 3, 0xFFFFFFFD, -2 & 0xFFFFFFFF, 1, flags=bm.SIGNED)[0]) == [1, 2]
    assert list(bm.select_range(sp, 4, 3, 0xFFFFFFFD, 0, 0xFFFFFFFE)[0]) == [0, 2, 3]  # unsigned: -3 is 0xFFFFFFFD
