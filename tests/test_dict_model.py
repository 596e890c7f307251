"""The numpy model of dictionary encoding (tests/dict_model.py) on hand-written cases: the four values at the ends of
both number lines in both orders, the empty column, d = capacity against d = capacity + 1, the length rule, and combine
with its overflow rule.  The GPU tests compare the kernels with this model, so it is checked by hand here."""
import numpy as np

from dwarf_bench_amd import dict_native as dn
from tests import dict_model as dm

U = np.uint32
EDGES = np.array([0xFFFFFFFF, 0, 0x80000000, 0x7FFFFFFF, 0, 0xFFFFFFFF], U)


def test_constants_are_the_bindings():
    assert (dm.SIGNED, dm.MISS) == (dn.SIGNED, dn.MISS)
    from dwarf_bench_amd import ops
    assert (dm.TABLE_FULL, dm.KEY_RANGE) == (ops.DEV_TABLE_FULL, ops.DEV_KEY_RANGE)
    for c in (1, 2, 3, 4, 5, 4096, 4097, (1 << 31) - 1):
        assert dm.slots(c) == dn.slots(c) >= 2 * c and dm.slots(c) & (dm.slots(c) - 1) == 0
    assert dm.slots(1) == 2 and dm.slots(4096) == dn.LDS_SLOTS and dm.slots(4097) == 2 * dn.LDS_SLOTS


def test_the_four_boundary_values_in_both_orders():
    keys, st = dm.build(EDGES, 4)
    assert st == 0 and keys.tolist() == [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    codes, misses = dm.encode(keys, EDGES)
    assert codes.tolist() == [3, 0, 2, 1, 0, 3] and misses == 0
    keys, st = dm.build(EDGES, 4, flags=dm.SIGNED)
    assert st == 0 and keys.tolist() == [0x80000000, 0xFFFFFFFF, 0, 0x7FFFFFFF]  # INT32_MIN, -1, 0, INT32_MAX
    codes, misses = dm.encode(keys, EDGES, flags=dm.SIGNED)
    assert codes.tolist() == [1, 2, 0, 3, 2, 1] and misses == 0
    # decode is a gather through the keys
    assert np.array_equal(keys[codes], EDGES)


def test_the_empty_column_and_absent_values():
    keys, st = dm.build(np.zeros(0, U), 1)
    assert keys.size == 0 and st == 0
    codes, misses = dm.encode(keys, np.array([0, 5, 0xFFFFFFFF], U))
    assert codes.tolist() == [dm.MISS] * 3 and misses == 3
    assert dm.encode(keys, np.zeros(0, U))[0].size == 0
    keys, _ = dm.build(np.array([10, 30, 20, 10], U), 3)
    codes, misses = dm.encode(keys, np.array([5, 10, 15, 20, 25, 30, 35, 0xFFFFFFFF, 0], U))
    assert codes.tolist() == [dm.MISS, 0, dm.MISS, 1, dm.MISS, 2, dm.MISS, dm.MISS, dm.MISS] and misses == 6


def test_capacity_reached_and_passed():
    col = np.array([7, 7, 3, 9, 3, 1], U)  # d = 4
    keys, st = dm.build(col, 4)
    assert st == 0 and keys.tolist() == [1, 3, 7, 9]
    keys, st = dm.build(col, 3)  # d = capacity + 1
    assert st == dm.TABLE_FULL and keys.size == 0
    codes, misses = dm.encode(keys, col)  # unusable: every row misses
    assert codes.tolist() == [dm.MISS] * 6 and misses == 6
    for flags in (0, dm.SIGNED):
        assert dm.build(col, 1, flags=flags)[1] == dm.TABLE_FULL and dm.build(col, 1 << 20, flags=flags)[1] == 0


def test_the_length_is_min_of_count_and_n():
    col = np.array([7, 7, 3, 9, 3, 1], U)
    assert [dm.length(c, 6) for c in (None, 0, 5, 6, 7, (1 << 64) - 1)] == [6, 0, 5, 6, 6, 6]
    assert dm.build(col, 2, count=3)[0].tolist() == [3, 7] and dm.build(col, 2, count=4)[1] == dm.TABLE_FULL
    assert dm.build(col, 2, count=0)[0].size == 0
    keys, _ = dm.build(col, 4)
    codes, misses = dm.encode(keys, np.array([9, 2, 1, 1], U), count=2)
    assert codes.tolist() == [3, dm.MISS] and misses == 1
    assert dm.encode(keys, col, count=1 << 40)[0].size == 6
    assert dm.combine([1, 2, 3], [0, 1, 2], 4, 3, count=2)[0].tolist() == [3, 7]


def test_combine_orders_pairs_lexicographically_and_carries_misses():
    outer, inner = np.array([0, 0, 1, 2, dm.MISS, 1], U), np.array([0, 2, 1, dm.MISS, 1, 0], U)
    out, st = dm.combine(outer, inner, 3, 3)
    assert st == 0 and out.tolist() == [0, 2, 4, dm.MISS, dm.MISS, 3]
    a, b = np.array([5, 1, 5, 1, 3], U), np.array([9, 9, 2, 2, 9], U)
    ka, kb = dm.build(a, 8)[0], dm.build(b, 8)[0]
    code, _ = dm.combine(dm.encode(ka, a)[0], dm.encode(kb, b)[0], ka.size, kb.size)
    pairs = sorted(set(zip(a.tolist(), b.tolist())))
    assert [pairs.index(p) for p in zip(a.tolist(), b.tolist())] == np.unique(code, return_inverse=True)[1].tolist()
    assert all((code[i] < code[j]) == ((a[i], b[i]) < (a[j], b[j])) for i in range(5) for j in range(5))


def test_combine_overflow_rule():
    top = np.array([65536, 0, dm.MISS], U)
    # 65537 x 65535 = 0xFFFFFFFF exactly: legal, the largest composite is 0xFFFFFFFE
    out, st = dm.combine(top, np.array([65534, 7, 1], U), 65537, 65535)
    assert st == 0 and out.tolist() == [0xFFFFFFFE, 7, dm.MISS]
    out, st = dm.combine(top, np.array([65535, 7, 1], U), 65536, 65536)  # 2^32
    assert st == dm.KEY_RANGE and out.tolist() == [dm.MISS] * 3
    assert dm.combine(top, top, 1 << 40, 1 << 40)[1] == dm.KEY_RANGE and dm.combine(top, top, 0, 1 << 63)[1] == 0
    out, st = dm.combine(top, top, 1 << 33, 1, count=1)
    assert out.tolist() == [dm.MISS] and st == dm.KEY_RANGE


def test_the_hash_is_murmur3s_finaliser_and_colliding_keys_collide():
    assert dm.hash32([0, 1, 0xFFFFFFFF]).tolist() == [0, 0x514E28B7, 0x81F16F39]
    keys = dm.colliding_keys(8, 13, 9)
    assert np.unique(keys).size == 9 and ((dm.hash32(keys) & U(15)) == 13).all()
