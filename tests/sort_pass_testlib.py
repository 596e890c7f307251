"""Key columns on which the LSD radix sort (csrc/radix.hip) executes a CHOSEN set of passes, and that plan restated in
numpy.  Test infrastructure, numpy only: never imported by the product.

The sort skips pass p when digit p of (key ^ xor_mask) is constant over the input (rs_plan_kernel from the histogram,
the one-workgroup kernels from an OR / AND of the keys).  keys_for(vary_mask, ...) = base ^ (random & vary_mask) with
rows 0 and 1 forced to base and base ^ vary_mask: every bit of vary_mask takes both values, every other bit is the
base's, so a correct sort executes exactly the digits that vary_mask intersects.  Both bases hold a nibble that is
neither 0 nor 0xF in every position: a constant digit is then neither zero nor the padding key 0xFFFFFFFF of a ragged
tile, and BASE_NEG has the top bit set (a constant top digit on either side of the sign flip).

This module also owns the lists that tests/test_sort_pass_model.py (CPU) and tests/test_gpu_sort_passes.py (GPU) walk,
so the model test proves the paths of exactly the columns the GPU test sorts."""
import numpy as np

BASE = 0x5A3CA5C3      # nibbles 5 A 3 C A 5 C 3
BASE_NEG = 0xA5C35A3C  # nibbles A 5 C 3 5 A 3 C: the top bit set
BASES = (BASE, BASE_NEG)
STYLES = ("whole", "low bit", "high bit")

TILE = 8192            # radix.hip kRsTile
FUSED_SCAN_CHUNKS = 32  # kRsFusedScanChunks: up to this many chunks the scatter sums its own prefix
TARGET_CHUNKS = 2048   # kRsTargetChunks (8-bit digits; 4-bit digits aim at half as many)
# one workgroup; one workgroup, full tile; 13 chunks (the fused scan); 34 chunks (rs_chunk_scan), ragged tile and vector
SIZES = (5000, 8192, 100003, 33 * 8192 + 5)
CHUNKED_SIZE = SIZES[3]
# the 4-bit pass sets at CHUNKED_SIZE, as bit masks over the passes: the 8 single passes, every other pass from either
# end, the lower and the upper half, the two ends, all but the ends, all but pass 0, all but pass 7, all, two neighbours
# in the middle, both ends doubled, two passes with a gap on every side
CHUNKED_SETS_4BIT = tuple(1 << p for p in range(8)) + (0x55, 0xAA, 0x0F, 0xF0, 0x81, 0x7E, 0xFE, 0x7F, 0xFF, 0x18, 0xC3, 0x24)
PART = 32              # pass sets per pytest case of the GPU test where all 255 are walked


def passes_of(set_mask, bits):
    """a set of passes given as a bit mask (bit p = pass p) -> the tuple of passes"""
    return tuple(p for p in range(32 // bits) if set_mask >> p & 1)


def vary_mask_for(pass_set, bits, style):
    """the key bits that vary so that exactly the passes of pass_set execute: all bits of each chosen digit ("whole"),
    its lowest ("low bit") or its highest bit ("high bit": with the top pass chosen, the sign bit)"""
    assert style in STYLES and 32 % bits == 0
    digit = {"whole": (1 << bits) - 1, "low bit": 1, "high bit": 1 << (bits - 1)}[style]
    mask = 0
    for p in pass_set:
        assert 0 <= p < 32 // bits
        mask |= digit << (p * bits)
    return mask


def keys_for(vary_mask, n, seed, base=BASE):
    """base ^ (random_u32 & vary_mask) as uint32; rows 0 and 1 are base and base ^ vary_mask, so for n >= 2 every bit of
    vary_mask really varies"""
    rng = np.random.default_rng(seed)
    keys = np.uint32(base) ^ (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(vary_mask))
    if n >= 1:
        keys[0] = base
    if n >= 2:
        keys[1] = base ^ vary_mask
    return keys


def executed_passes(keys, bits, signed):
    """the sort's plan in numpy: pass p runs iff more than one value of ((key ^ xor_mask) >> shift) & (radix - 1) occurs"""
    x = np.ascontiguousarray(keys).view(np.uint32) ^ np.uint32(0x80000000 if signed else 0)
    ran = []
    for p in range(32 // bits):
        digit = (x >> np.uint32(p * bits)) & np.uint32((1 << bits) - 1)
        if digit.size and digit.min() != digit.max():  # more than one value
            ran.append(p)
    return tuple(ran)


def geometry(n, bits):
    """(tiles, tiles per chunk, chunks) of radix.hip rs_geometry, for sizes below the chunk target (one tile per chunk)"""
    tiles = -(-n // TILE)
    assert tiles < (TARGET_CHUNKS // 2 if bits == 4 else TARGET_CHUNKS)
    return tiles, 1, max(tiles, 1)


def pass_sets(bits, n):
    """the pass sets (bit masks) walked at (bits, n), in the order that fixes each one's index"""
    if bits == 8:
        return tuple(range(1, 16))
    assert bits == 4
    return CHUNKED_SETS_4BIT if n == CHUNKED_SIZE else tuple(range(1, 256))


def parts(bits, n):
    """the pytest cases of (bits, n): slices of pass_sets(bits, n) of at most PART sets"""
    return tuple(range(-(-len(pass_sets(bits, n)) // PART)))


def columns(bits, n, part):
    """the columns of one pytest case -> [(set_mask, style, base, vary_mask, seed)].  Every pass set comes in the style
    "whole" and in ONE of the one-bit styles, alternating with the parity of the bits of the set's index in its list (the
    plain index would give every set with pass 0 the same style in the lists that count 1, 2, 3, ...); the base
    alternates with the bits of index // 2, and the one-bit column takes the other base than the whole-digit one.
    tests/test_sort_pass_model.py checks what this is for: at every pass position both one-bit styles occur, and both
    bases in either kind of style."""
    sets = pass_sets(bits, n)
    out = []
    for index in range(part * PART, min((part + 1) * PART, len(sets))):
        set_mask = sets[index]
        for style in ("whole", STYLES[1 + bin(index).count("1") % 2]):
            base = BASES[(bin(index >> 1).count("1") + (style != "whole")) % 2]
            seed = (bits * 1000003 + n) * 1024 + index * 4 + STYLES.index(style)
            out.append((set_mask, style, base, vary_mask_for(passes_of(set_mask, bits), bits, style), seed))
    return out


def cases():
    """every (bits, n, part) of the GPU test"""
    return [(bits, n, part) for bits in (8, 4) for n in SIZES for part in parts(bits, n)]


# ---- the other columns of the GPU test ------------------------------------------------------------------------------------
# one plan reused over columns whose executed sets differ (8-bit passes; with 4-bit digits pass p is nibbles 2p, 2p + 1)
REUSE_BYTE_SETS = ((3,), (0, 2), (1, 2, 3), (), (1,), (0, 1, 2, 3))


def reuse_columns(n):
    """-> [(byte set, keys)]: whole bytes vary; the empty set is a column of equal keys"""
    return [(s, keys_for(vary_mask_for(s, 8, "whole"), n, 700 + i, BASES[i % 2])) for i, s in enumerate(REUSE_BYTE_SETS)]


FRONT_DOOR_N = 100003


def front_door_columns():
    """-> [(name, keys)]: keys that vary only in the top byte, sign bit included, and only in byte 1"""
    return [("top byte", keys_for(0xFF000000, FRONT_DOOR_N, 801, BASE)), ("byte 1", keys_for(0x0000FF00, FRONT_DOOR_N, 802, BASE_NEG))]
