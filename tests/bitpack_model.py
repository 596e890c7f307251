"""Test-only numpy model of the bit-packed column (dwarf_bench_amd/host/bitpack.hpp): the format as
np.packbits(..., bitorder='little') over the code bits viewed as little-endian uint32 words, padded with zero bits to whole
16-byte chunks; pack with its clamped length, the rows that do not fit and the words it leaves alone; unpack, dense and
through a row-id list; and the range filter on the decoded values.  Never imported by the product."""
import numpy as np

SIGNED, NEGATE, OUTER = 1, 2, 4
NO_ROW = 0xFFFFFFFF
KEY_RANGE = 2  # DBHIP_DEV_KEY_RANGE
SEGMENT_ROWS, TILE_ROWS = 4096, 2048
M64 = (1 << 64) - 1
U = np.uint32


def words(n_rows, width):
    """the uint32 words of a packed column: ceil(n_rows * width / 32) rounded up to a multiple of 4; 0 = no such column"""
    if not 1 <= width <= 32 or not 0 <= n_rows < (1 << 32):
        return 0
    return (-(-(n_rows * width) // 32) + 3) // 4 * 4


def mask(width):
    return (1 << width) - 1


def length(count, capacity):
    """m = min(*count, capacity); count None: the capacity.  count is any uint64"""
    return int(capacity) if count is None else min(int(count) & M64, int(capacity))


def pack_codes(codes, width):
    """codes (each < 2^width) -> the packed words, padding bits zero"""
    codes = np.asarray(codes).view(U)
    bits = ((codes[:, None] >> np.arange(width, dtype=U)) & U(1)).astype(np.uint8).reshape(-1)
    stream = np.zeros(32 * words(codes.size, width), np.uint8)
    stream[: bits.size] = bits
    return np.packbits(stream, bitorder="little").view("<u4").astype(U)


def unpack_codes(packed, n_rows, width):
    """the first n_rows codes of the packed words"""
    bits = np.unpackbits(np.asarray(packed).view(U).astype("<u4").view(np.uint8), bitorder="little")[: n_rows * width]
    weights = (np.uint64(1) << np.arange(width, dtype=np.uint64))
    return (bits.reshape(n_rows, width).astype(np.uint64) * weights).sum(axis=1).astype(U)


def pack(col, width, base=0, count=None, before=None):
    """col: the column (its size is the capacity); before: what out_packed held (at least words(capacity) words; None:
    zeros) -> (out_packed afterwards, the status word).  Exactly words(m) words are written."""
    col = np.asarray(col).view(U)
    m = length(count, col.size)
    codes = col[:m] - U(base & 0xFFFFFFFF)  # mod 2^32
    status = KEY_RANGE if bool((codes.astype(np.uint64) >> np.uint64(width)).any()) else 0
    out = np.zeros(words(col.size, width), U) if before is None else np.asarray(before).view(U).copy()
    out[: words(m, width)] = pack_codes(codes & U(mask(width)), width)
    return out, status


def decode(packed, n_rows, width, base=0):
    """every row's value: (base + code) mod 2^32"""
    return unpack_codes(packed, n_rows, width) + U(base & 0xFFFFFFFF)


def unpack(packed, n_rows, width, base=0, rows=None, count=None, flags=0, fill=0, before=None):
    """-> (out afterwards, the status word); rows None: the dense decode; otherwise the take of dbench_take_u32"""
    assert not flags & ~OUTER
    values = decode(packed, n_rows, width, base)
    if rows is None:
        assert count is None
        return values, 0
    e = np.asarray(rows).view(U)
    m = length(count, e.size)
    e = e[:m]
    inside = e.astype(np.uint64) < np.uint64(n_rows)
    excused = (e == U(NO_ROW)) if flags & OUTER else np.zeros(m, bool)
    out = np.zeros(np.asarray(rows).size, U) if before is None else np.asarray(before).view(U).copy()
    got = np.full(m, fill & 0xFFFFFFFF, U)
    got[inside] = values[e[inside]]
    out[:m] = got
    return out, (KEY_RANGE if bool((~inside & ~excused).any()) else 0)


def keep(values, lo, hi, flags=0):
    """the predicate of select_range on uint32 values; lo, hi: 32-bit patterns"""
    v = np.asarray(values).view(U)
    if flags & SIGNED:
        v, lo, hi = v.view(np.int32).astype(np.int64), int(np.array([lo & 0xFFFFFFFF], U).view(np.int32)[0]), \
            int(np.array([hi & 0xFFFFFFFF], U).view(np.int32)[0])
    else:
        v, lo, hi = v.astype(np.int64), lo & 0xFFFFFFFF, hi & 0xFFFFFFFF
    inside = (v >= lo) & (v <= hi)
    return ~inside if flags & NEGATE else inside


def select_range(packed, n_rows, width, base, lo, hi, rows=None, count=None, flags=0):
    """-> (the kept row ids in candidate order, the status word)"""
    assert not flags & ~(SIGNED | NEGATE)
    values = decode(packed, n_rows, width, base)
    if rows is None:
        assert count is None
        return np.nonzero(keep(values, lo, hi, flags))[0].astype(U), 0
    e = np.asarray(rows).view(U)
    e = e[: length(count, e.size)]
    inside = e.astype(np.uint64) < np.uint64(n_rows)
    kept = inside.copy()
    kept[inside] = keep(values[e[inside]], lo, hi, flags)
    return e[kept], (KEY_RANGE if bool((~inside).any()) else 0)
