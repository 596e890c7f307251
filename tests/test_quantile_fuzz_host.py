"""The quantile select's seeded sweep on the CPU (tests/quantile_fuzz_testlib.py; tests/test_gpu_quantile_fuzz.py runs the same
draws on the GPU): the draws hold every category of every dimension, the intact twin — the select level by level, as the
kernels run it — agrees with tests/quantile_model.py, which sorts, and each one-defect twin is rejected by some draw: so a
kernel with that defect would fail the GPU sweep.

The first draw that rejects each defect (seed 2605, 96 draws), and how many draws reject it:
    rank off by one                                  draw  0   58 draws
    < for <= in the bin pick                         draw  0   60 draws
    last n & 3 keys dropped                          draw  0   59 draws
    sign flip ignored                                draw  2    9 draws
    count not clamped                                draw  3   21 draws
    invalid ids counted in m                         draw  9   10 draws
    another slot's remainder                         draw 17   11 draws
    level-2 digit 11 bits wide                       draw 17    6 draws
"""
import numpy as np
import pytest

from tests import fuzz_testlib as fz
from tests import quantile_fuzz_testlib as qf
from tests import quantile_model as qm

FIRST = {"rank off by one": (0, 58), "< for <= in the bin pick": (0, 60), "last n & 3 keys dropped": (0, 59),
         "sign flip ignored": (2, 9), "count not clamped": (3, 21), "invalid ids counted in m": (9, 10),
         "another slot's remainder": (17, 11), "level-2 digit 11 bits wide": (17, 6)}


@pytest.fixture(scope="module")
def sweep():
    cases = qf.cases()
    return cases, [qf.model(c) for c in cases]


def rejected(case, want, result):
    try:
        fz.same(case, result, want)
    except AssertionError:
        return True
    return False


def test_the_draws_hold_every_category(sweep):
    cases, _ = sweep
    assert 90 <= len(cases) <= 200 and [c["draw"] for c in cases] == list(range(len(cases)))
    assert max(c["size"] for c in cases) <= 1 << 17
    sizes = {c["size"] for c in cases}
    assert {0, 1, 63, 64, 65, qf.ROUND - 1, qf.ROUND, qf.ROUND + 1, 2 * qf.ROUND - 1, 2 * qf.ROUND, 2 * qf.ROUND + 1} <= sizes
    for listed in (False, True):
        mine = [c for c in cases if (c["rows"] is not None) == listed]
        assert len(mine) >= 30
        assert set(fz.COUNT_KINDS) <= {fz.count_kind(c["count"], c["size"]) for c in mine}, listed
        assert {c["signed"] for c in mine} == {False, True}
        assert {1, 4, 5, 16} <= {len(c["num"]) for c in mine}  # every slot capacity, and both sides of each threshold
    assert set(qf.RANK_KINDS) == {k for c in cases for k in c["rank_kinds"]}
    assert {c["offs"]["col"] for c in cases} == {0, 1, 2, 3} == {c["offs"]["rows"] for c in cases if c["rows"] is not None}
    assert {o for c in cases for o in c["offs"]["out"]} == {0, 1, 2, 3}
    assert {c["fill"] for c in cases} == set(fz.FILLS) and len({c["stale_status"] for c in cases}) >= 3
    assert any(c["rows"] is not None and (c["rows"][: fz.counted(c["count"], c["size"])] >= c["col"].size).any() for c in cases)
    assert any(c["col"].size == 0 for c in cases)
    # ranks of one call that share a level-0 bin, a level-1 bin too, and ranks that share a value
    shared = {0: 0, 1: 0, 2: 0}
    for c, want in zip(*sweep):
        live = want["equal"] > 0
        x = want["values"][live] ^ np.uint32(0x80000000 if c["signed"] else 0)
        for level, shift in enumerate((21, 10, 0)):
            shared[level] += int(live.sum()) > len(set((x >> np.uint32(shift)).tolist())) > 1
    assert all(shared[level] >= 3 for level in shared), shared


def test_the_intact_twin_is_the_sorting_model(sweep):
    for case, want in zip(*sweep):
        values, below, equal, st = qm.select(case["col"], case["num"], case["den"], case["flags"], case["rows"], case["count"])
        assert st == want["status"] and np.array_equal(values, want["values"]), case["draw"]
        assert np.array_equal(below, want["below"]) and np.array_equal(equal, want["equal"]), case["draw"]


@pytest.mark.parametrize("defect", qf.DEFECTS)
def test_every_defect_is_rejected_by_some_draw(sweep, defect):
    cases, wants = sweep
    hits = [c["draw"] for c, want in zip(cases, wants) if rejected(c, want, qf.model(c, defect))]
    assert hits, f"no draw rejects a call with '{defect}'"
    assert (hits[0], len(hits)) == FIRST[defect], (defect, hits[0], len(hits))
    assert f"{defect:<48} draw {hits[0]:>2}   {len(hits):>2} draws" in __doc__


def test_the_table_names_every_defect():
    assert set(FIRST) == set(qf.DEFECTS) and len(qf.DEFECTS) == 8
