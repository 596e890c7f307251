"""numpy model of the dictionary-encoding entry points (dwarf_bench_amd/host/dict_encode.hpp): what build, encode and
combine must leave, bit for bit, including the length rule m = min(*count, n), both key orders, the overflow of the
capacity and the overflow of the composite code.  Also the stated hash and slot count (dict_layout.hpp), so that tests can
build keys against them.  Test-only; never imported by the product."""
import numpy as np

U = np.uint32
SIGNED = 1
MISS = 0xFFFFFFFF
TABLE_FULL, KEY_RANGE = 4, 2  # DBHIP_DEV_TABLE_FULL, DBHIP_DEV_KEY_RANGE


def length(count, n):
    """m = min(*count, n); count None: all n"""
    return n if count is None else min(int(count), n)


def hash32(keys):
    """dict_hash: Murmur3's 32-bit finaliser, on a uint32 array"""
    h = np.asarray(keys, dtype=U).copy()
    h ^= h >> U(16)
    h *= U(0x85EBCA6B)
    h ^= h >> U(13)
    h *= U(0xC2B2AE35)
    h ^= h >> U(16)
    return h


def slots(capacity):
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


def ordered(keys, flags=0):
    """distinct values ascending: as uint32, or as int32 with SIGNED; uint32 bits either way"""
    keys = np.asarray(keys, dtype=U)
    if flags & SIGNED:
        return np.unique(keys.view(np.int32)).view(U)
    return np.unique(keys)


def build(col, capacity, count=None, flags=0):
    """-> (keys: the d distinct values of col[:m] in order, status).  More than `capacity` of them: no keys at all,
    TABLE_FULL, and the dictionary answers MISS for everything until the next build."""
    assert 1 <= capacity < 1 << 31
    col = np.asarray(col, dtype=U)
    keys = ordered(col[: length(count, col.size)], flags)
    if keys.size > capacity:
        return np.zeros(0, U), TABLE_FULL
    return keys, 0


def encode(keys, col, count=None, flags=0):
    """keys: what build returned (ordered by the same flags) -> (codes of col[:m], the number of misses)"""
    col = np.asarray(col, dtype=U)[: length(count, np.asarray(col).size)]
    keys = np.asarray(keys, dtype=U)
    if keys.size == 0:
        return np.full(col.size, MISS, U), int(col.size)
    a, b = (keys.view(np.int32), col.view(np.int32)) if flags & SIGNED else (keys, col)
    at = np.searchsorted(a, b)
    found = (at < keys.size) & (a[np.minimum(at, keys.size - 1)] == b)
    return np.where(found, at, MISS).astype(U), int((~found).sum())


def combine(outer, inner, outer_card, inner_card, count=None):
    """-> (out[:m], status): outer * inner_card + inner, MISS where either is; a product of the cardinalities above
    0xFFFFFFFF: every entry MISS and KEY_RANGE"""
    outer, inner = np.asarray(outer, dtype=U), np.asarray(inner, dtype=U)
    m = length(count, outer.size)
    o, i = outer[:m].astype(np.uint64), inner[:m].astype(np.uint64)
    if int(outer_card) * int(inner_card) > 0xFFFFFFFF:
        return np.full(m, MISS, U), KEY_RANGE
    code = (o * np.uint64(int(inner_card) & 0xFFFFFFFF) + i) & np.uint64(0xFFFFFFFF)
    return np.where((o == MISS) | (i == MISS), MISS, code).astype(U), 0


def colliding_keys(capacity, home, how_many, start=0):
    """the first `how_many` uint32 values from `start` on whose home slot in the table of `capacity` is `home`"""
    mask = U(slots(capacity) - 1)
    out, at = [], start
    while len(out) < how_many:
        block = np.arange(at, at + 65536, dtype=np.uint64).astype(U)
        out += [int(k) for k in block[(hash32(block) & mask) == U(home)]]
        at += 65536
    return np.array(out[:how_many], dtype=U)
