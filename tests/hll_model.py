"""Test-only numpy model of the HyperLogLog sketch (dwarf_bench_amd/host/hll_sketch.hpp, hll_layout.hpp): the two hash chains
of a key tuple, the register and the rank of a hash, build with its clamped length, its row-id list, the ids that do not
count, the registers it started from and the status word, merge, the histogram, and Ertl's estimator in double.  Never
imported by the product."""
import math

import numpy as np

ACCUMULATE = 1
KEY_RANGE = 2  # DBHIP_DEV_KEY_RANGE
GOLDEN = 0x9E3779B9
MIN_P, MAX_P, MAX_COLS, HIST_WORDS = 4, 14, 4, 64
M64 = (1 << 64) - 1
U, W, B = np.uint32, np.uint64, np.uint8


def fmix32(h):
    """csrc/dbhip_common.hpp's fmix32 (murmur3's finaliser) on a uint32 array"""
    h = np.asarray(h, dtype=U).copy()
    h ^= h >> U(16)
    h *= U(0x85EBCA6B)
    h ^= h >> U(13)
    h *= U(0xC2B2AE35)
    h ^= h >> U(16)
    return h


def unmix32(h):
    """the inverse of fmix32: every step of it is a bijection of the 32-bit words"""
    h = np.asarray(h, dtype=U).copy()
    h ^= h >> U(16)
    h *= U(0x7ED1B41D)  # the inverse of 0xC2B2AE35 modulo 2^32
    h ^= (h >> U(13)) ^ (h >> U(26))
    h *= U(0xA5CB9243)  # the inverse of 0x85EBCA6B modulo 2^32
    h ^= h >> U(16)
    return h


def as_u32(col):
    k = np.atleast_1d(np.asarray(col))
    return k.view(U) if k.dtype.itemsize == 4 else (k.astype(W) & W(0xFFFFFFFF)).astype(U)  # int32 bits, or Python ints


def columns(cols):
    """one column or a sequence of 1 .. 4 -> the list of uint32 arrays"""
    cols = [cols] if isinstance(cols, np.ndarray) else list(cols)
    assert 1 <= len(cols) <= MAX_COLS
    cols = [as_u32(c) for c in cols]
    assert all(c.size == cols[0].size for c in cols)
    return cols


def hash_tuples(cols, seed=0):
    """-> (h, g) of every row of the columns: two uint32 arrays"""
    cols = columns(cols)
    s = U(seed & 0xFFFFFFFF)
    h, g = fmix32(cols[0] ^ s), fmix32(cols[0] ^ s ^ U(GOLDEN))
    for c in cols[1:]:
        h, g = fmix32(h ^ c), fmix32(g ^ c)
    return h, g


def clz64(w):
    """the leading zeros of every nonzero uint64 of w (64 for zero)"""
    w = np.asarray(w, dtype=W)
    hi, lo = (w >> W(32)).astype(np.float64), (w & W(0xFFFFFFFF)).astype(np.float64)  # a double holds 32 bits exactly
    bits_hi, bits_lo = np.frexp(hi)[1], np.frexp(lo)[1]  # the bit length of each half; 0 for zero
    return np.where(hi > 0, 32 - bits_hi, 64 - bits_lo).astype(np.int64)


def place(h, g, p):
    """-> (idx, rank) of every hash: the register and the rank it offers, 1 .. 64 - p + 1"""
    assert MIN_P <= p <= MAX_P
    x = (np.asarray(h, dtype=U).astype(W) << W(32)) | np.asarray(g, dtype=U).astype(W)
    w = x << W(p)
    rank = np.where(w == 0, 64 - p + 1, clz64(w) + 1)
    return (x >> W(64 - p)).astype(U), rank.astype(B)


def length(count, capacity):
    """m = min(*count, capacity); count None: the capacity.  count is any uint64"""
    return int(capacity) if count is None else min(int(count) & M64, int(capacity))


def insert(registers, cols, p, seed=0):
    """registers = max(registers, the ranks of the rows), in place"""
    return offer(registers, *place(*hash_tuples(cols, seed), p))


def offer(registers, idx, rank):
    """registers[idx] = max(registers[idx], rank) for every pair, in place: which (register, rank) pairs occur at all, then
    the highest rank of each register"""
    m = registers.size
    seen = np.bincount(idx.astype(np.int64) * 64 + rank, minlength=m * 64).reshape(m, 64) > 0
    registers[:] = np.maximum(registers, (seen * np.arange(64, dtype=B)).max(axis=1))
    return registers


def clamp(registers, p):
    """-> (the bytes with those above q+1 lowered to it, the status that raises)"""
    r = np.asarray(registers).view(B)
    top = 64 - p + 1
    return np.minimum(r, B(top)), (KEY_RANGE if bool((r > top).any()) else 0)


def histogram(registers):
    return np.bincount(np.asarray(registers).view(B), minlength=HIST_WORDS).astype(U)


def build(cols, p, seed=0, rows=None, count=None, flags=0, before=None):
    """-> (the registers afterwards, their histogram, the status word).  before: what the registers held (None: anything — a
    build that does not accumulate)"""
    assert not flags & ~ACCUMULATE
    cols = columns(cols)
    n_col = cols[0].size
    status = 0
    if flags & ACCUMULATE:
        registers, status = clamp(np.zeros(1 << p, B) if before is None else before, p)
        registers = registers.copy()
    else:
        registers = np.zeros(1 << p, B)
    if rows is None:
        m = length(count, n_col)
        keys = [c[:m] for c in cols]
    else:
        e = np.asarray(rows).view(U)
        e = e[: length(count, e.size)]
        inside = e.astype(W) < W(n_col)
        status |= KEY_RANGE if bool((~inside).any()) else 0
        keys = [c[e[inside]] for c in cols]
    insert(registers, keys, p, seed)
    return registers, histogram(registers), status


def merge(dst, src, p):
    """-> (max(dst, src) after the clamp of both, its histogram, the status word)"""
    d, sd = clamp(dst, p)
    s, ss = clamp(src, p)
    out = np.maximum(d, s)
    return out, histogram(out), sd | ss


def sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        before = z
        z += x * y
        y += y
        if z == before:
            return z


def tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        before = z
        y *= 0.5
        z -= (1.0 - x) * (1.0 - x) * y
        if z == before:
            return z / 3.0


def estimate(hist, p):
    """Ertl's improved raw estimator on the histogram, in double.  -1.0: p out of range, a count above q+1, or counts that
    do not sum to m"""
    if not MIN_P <= p <= MAX_P or len(hist) != HIST_WORDS:
        return -1.0
    hist = [int(v) for v in hist]
    q, m = 64 - p, 1 << p
    if any(hist[q + 2:]) or sum(hist) != m or min(hist) < 0:
        return -1.0
    dm = float(m)
    z = dm * tau(1.0 - float(hist[q + 1]) / dm)
    for k in range(q, 0, -1):
        z = (z + float(hist[k])) * 0.5
    z += dm * sigma(float(hist[0]) / dm)
    if z == 0.0:
        return math.inf
    return dm * dm / (2.0 * math.log(2.0) * z)


def relative_error(p):
    return 1.04 / math.sqrt(1 << p)


def keys_ranked_by_g(n, p, seed=0, rng=None, front=()):
    """n keys built against the hash (fmix32 is invertible): the LAST column of n key tuples whose h has its low 32 - p bits
    zero, so that w = x << p has bits only in its g half and the rank (33 - p + clz32(g), or q+1 for g == 0) comes from g
    alone.  front: the columns in front of it (none: a single-column key).  Their registers spread over all of 2^p"""
    rng = rng or np.random.default_rng(5)
    h = (rng.integers(0, 1 << p, n, dtype=np.uint64) << np.uint64(32 - p)).astype(U)
    if not len(front):
        return unmix32(h) ^ U(seed & 0xFFFFFFFF)
    return unmix32(h) ^ hash_tuples(front, seed)[0]
