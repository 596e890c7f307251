"""The Bloom filter's seeded sweep on the CPU (tests/bloom_fuzz_testlib.py; tests/test_gpu_bloom_fuzz.py runs the same draws
on the GPU): the draws hold every category of every dimension, the intact model agrees with tests/bloom_model.py, and each
one-defect model is rejected by some draw — so a kernel with that defect would fail the GPU sweep.

The first draw that rejects each defect (seed 2036, 60 draws), and how many draws reject it:
    count ignored                                    draw  5   17 draws
    count not clamped                                draw  1    8 draws
    negate ignored                                   draw  3   18 draws
    accumulate ignored                               draw  5    9 draws
    filter not cleared                               draw  0   10 draws
    1u << b instead of 1ull << b                     draw  0   35 draws
    word = h % n_words                               draw  0   28 draws
    seed ignored                                     draw  0   28 draws
    last candidate of a ragged segment dropped       draw  0   30 draws
    first element of an unaligned column dropped     draw  4   18 draws
    bad row id read as row 0                         draw 10    4 draws
    status not raised                                draw  3   10 draws
    status not cleared                               draw  0   39 draws
    one entry behind the count written               draw  2   23 draws
"""
import numpy as np
import pytest

from tests import bloom_fuzz_testlib as bf
from tests import bloom_model as blm
from tests import fuzz_testlib as fz

FIRST = {"count ignored": (5, 17), "count not clamped": (1, 8), "negate ignored": (3, 18), "accumulate ignored": (5, 9),
         "filter not cleared": (0, 10), "1u << b instead of 1ull << b": (0, 35), "word = h % n_words": (0, 28),
         "seed ignored": (0, 28), "last candidate of a ragged segment dropped": (0, 30),
         "first element of an unaligned column dropped": (4, 18), "bad row id read as row 0": (10, 4),
         "status not raised": (3, 10), "status not cleared": (0, 39), "one entry behind the count written": (2, 23)}


@pytest.fixture(scope="module")
def sweep():
    cases = bf.cases()
    return cases, [bf.model(c) for c in cases]


def rejected(case, want, result):
    try:
        fz.same(case, result, want)
    except AssertionError:
        return True
    return False


def test_the_draws_hold_every_category(sweep):
    cases, _ = sweep
    assert 55 <= len(cases) <= 65 and [c["draw"] for c in cases] == list(range(len(cases)))
    assert max(c["size"] for c in cases) <= 1 << 17 and max(c["n_words"] for c in cases) <= 1 << 17
    sizes = {c["size"] for c in cases}
    assert {0, 1, 63, 64, 65, bf.SEG - 1, bf.SEG, bf.SEG + 1, 2 * bf.SEG - 1, 2 * bf.SEG, 2 * bf.SEG + 1} <= sizes
    for what in ("build", "probe"):
        mine = [c for c in cases if c["what"] == what]
        assert {c["rows"] is not None for c in mine} == {False, True}, what
        kinds = {fz.count_kind(c["count"], c["size"]) for c in mine if c["rows"] is not None or what == "build"}
        assert set(fz.COUNT_KINDS) <= kinds, (what, kinds)
        assert {c["offs"]["col"] for c in mine} == {c["offs"]["rows"] for c in mine} == {0, 1, 2, 3}, what
        assert {c["fill"] for c in mine} == set(fz.FILLS) and len({c["seed"] for c in mine}) > 3 and 0 in {c["seed"] for c in mine}
        assert any(c["rows"] is not None and (c["rows"][: fz.counted(c["count"], c["size"])] >= c["col"].size).any() for c in mine), what
        assert len({c["stale_status"] for c in mine}) >= 3
    assert {c["accumulate"] for c in cases if c["what"] == "build"} == {False, True}
    probes = [c for c in cases if c["what"] == "probe"]
    assert {c["negate"] for c in probes} == {False, True} == {c["count_only"] for c in probes}
    assert any(not c["filter"].any() for c in probes) and any(c["n_words"] == 1 for c in cases) and any(c["col"].size == 0 for c in cases)


def test_the_intact_model_is_bloom_models(sweep):
    for case, want in zip(*sweep):
        if case["what"] == "build":
            filt, st = blm.build(case["col"], case["n_words"], case["seed"], case["rows"], case["count"], case["flags"], case["before"])
            assert st == want["status"] and np.array_equal(filt, want["filter"]), case["draw"]
        else:
            rows, count, st = blm.probe(case["filter"], case["col"], case["seed"], case["rows"], case["count"], case["flags"])
            assert (count, st) == (want["count"], want["status"]), case["draw"]
            if not case["count_only"]:
                assert np.array_equal(rows, want["out"][:count]), case["draw"]
            assert (want["out"][0 if case["count_only"] else count:] == case["fill"]).all()


@pytest.mark.parametrize("defect", bf.DEFECTS)
def test_every_defect_is_rejected_by_some_draw(sweep, defect):
    cases, wants = sweep
    hits = [c["draw"] for c, want in zip(cases, wants) if rejected(c, want, bf.model(c, defect))]
    assert hits, f"no draw rejects a call with '{defect}'"
    assert (hits[0], len(hits)) == FIRST[defect], (defect, hits[0], len(hits))
    assert f"{defect:<48} draw {hits[0]:>2}   {len(hits):>2} draws" in __doc__


def test_the_table_names_every_defect():
    assert set(FIRST) == set(bf.DEFECTS) and len(bf.DEFECTS) == 14
