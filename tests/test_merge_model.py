"""The numpy model of the merge-path entry points (tests/merge_model.py) against numpy itself: the merge is the stable
argsort of the concatenation applied to it, the set operations are union1d, intersect1d and setdiff1d, on every size
and pattern the GPU tests use (tests/merge_testlib.py).  No GPU."""
import numpy as np
import pytest

from dwarf_bench_amd import merge_native as mn
from tests import merge_model as mm
from tests import merge_testlib as ml

T = mn.TILE_ROWS


@pytest.mark.parametrize("signed", (False, True))
def test_merge_is_the_stable_argsort_of_the_concatenation(signed):
    rng = np.random.default_rng(1)
    flags = mm.SIGNED if signed else 0
    for na, nb in ml.sizes(T):
        for name, a, b in ml.key_patterns(na, nb, rng, signed):
            assert (np.diff(mm.order(a, signed)) >= 0).all() and (np.diff(mm.order(b, signed)) >= 0).all(), name
            both = np.concatenate([a, b])
            perm = np.argsort(mm.order(both, signed), kind="stable")
            keys, vals, count, status = mm.merge(a, b, flags)
            assert (count, status, vals) == (na + nb, 0, None) and np.array_equal(keys, both[perm]), name
            _, ids, _, _ = mm.merge(a, b, flags | mm.ROW_IDS)
            assert np.array_equal(ids, perm.astype(np.uint32)), name  # full columns: the ids ARE the argsort
            av, bv = rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32), np.arange(nb, dtype=np.uint32)
            _, carried, _, _ = mm.merge(a, b, flags, a_vals=av, b_vals=bv)
            assert np.array_equal(carried, np.concatenate([av, bv])[perm]), name
            # A first among equal keys, input order inside a source
            from_b = ids >= na
            for side in (ids[~from_b], ids[from_b]):
                assert (np.diff(side.astype(np.int64)) > 0).all(), name
            ties = np.flatnonzero(keys[1:] == keys[:-1])
            assert not (from_b[ties] & ~from_b[ties + 1]).any(), name


def test_merge_counts_are_clamped_and_row_ids_keep_the_capacity_offset():
    rng = np.random.default_rng(2)
    a, b = np.sort(rng.integers(0, 100, 50)).astype(np.uint32), np.sort(rng.integers(0, 100, 70)).astype(np.uint32)
    for ca, cb in ((0, 0), (0, 70), (50, 0), (10, 20), (50, 70), (51, 1 << 40), (None, 3), (7, None)):
        keys, ids, count, _ = mm.merge(a, b, mm.ROW_IDS, a_count=ca, b_count=cb)
        na, nb = (50 if ca is None else min(ca, 50)), (70 if cb is None else min(cb, 70))
        assert count == na + nb == keys.size
        assert np.array_equal(np.sort(ids), np.concatenate([np.arange(na), 50 + np.arange(nb)]))
        assert np.array_equal(np.concatenate([a, b])[ids], keys)  # the ids index the two buffers laid end to end
        assert np.array_equal(keys, np.sort(np.concatenate([a[:na], b[:nb]])))


def test_set_operations_are_numpys():
    rng = np.random.default_rng(3)
    for n in (0, 1, 5, T + 7, 20011):
        for name, a, b in ml.set_cases(max(n, 1), rng):
            if n == 0:
                a, b = a[:0], b[:0]
            assert (np.diff(a.astype(np.int64)) > 0).all() and (np.diff(b.astype(np.int64)) > 0).all(), name
            for op, ref in ((mm.UNION, np.union1d), (mm.INTERSECT, np.intersect1d), (mm.DIFFERENCE, np.setdiff1d)):
                out, count, status = mm.setop(op, a, b)
                assert (count, status) == (out.size, 0) and np.array_equal(out, ref(a, b)), (name, op)
                assert count <= mn.set_bound(op, a.size, b.size)
    a, b = np.arange(0, 40, 2, dtype=np.uint32), np.arange(0, 40, 3, dtype=np.uint32)
    for ca, cb in ((0, 5), (5, 0), (3, 100), (None, 4)):
        out, _, _ = mm.setop(mm.INTERSECT, a, b, ca, cb)
        assert np.array_equal(out, np.intersect1d(a[:ca], b[:min(cb, b.size)]))


def test_the_constructed_lists_put_partner_pairs_across_tile_edges():
    a, b = ml.straddling(T)
    assert (np.diff(a.astype(np.int64)) > 0).all() and (np.diff(b.astype(np.int64)) > 0).all()
    assert ml.pairs_on_tile_edges(a, b, T) == [1, 2, 3]
    assert np.intersect1d(a, b).size == 3
    na, nb = ml.second_round(T)
    assert na + nb == 1025 * T + 3
