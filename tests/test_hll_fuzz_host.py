"""The HyperLogLog sketch's seeded sweep on the CPU (tests/hll_fuzz_testlib.py; tests/test_gpu_hll_fuzz.py runs the same draws on
the GPU): the draws hold every category of every dimension, the intact model agrees with tests/hll_model.py, and each
one-defect model is rejected by some draw — so a kernel with that defect would fail the GPU sweep.

The first draw that rejects each defect (seed 2041, 60 draws), and how many draws reject it:
    count ignored                                    draw  6   16 draws
    count not clamped                                draw  8    6 draws
    accumulate ignored                               draw  0   18 draws
    registers not cleared                            draw  2   20 draws
    seed ignored                                     draw  3   24 draws
    second column ignored                            draw  2   29 draws
    columns hashed in the wrong order                draw  2   30 draws
    idx taken from the low bits                      draw  2   34 draws
    rank off by one                                  draw  2   33 draws
    32-bit clz, the g half ignored                   draw 10    7 draws
    last writer wins instead of max                  draw  1   19 draws
    histogram not recounted on merge                 draw 21    4 draws
    stored byte above q+1 not clamped                draw  0   16 draws
    last element of a ragged segment dropped         draw  2   19 draws
    first element of an unaligned column dropped     draw  2   14 draws
    bad row id read as row 0                         draw 12    1 draws
    status not raised                                draw  0   23 draws
    status not cleared                               draw  2   36 draws
"""
import numpy as np
import pytest

from tests import fuzz_testlib as fz
from tests import hll_fuzz_testlib as hf
from tests import hll_model as hm

FIRST = {"count ignored": (6, 16), "count not clamped": (8, 6), "accumulate ignored": (0, 18),
         "registers not cleared": (2, 20), "seed ignored": (3, 24), "second column ignored": (2, 29),
         "columns hashed in the wrong order": (2, 30), "idx taken from the low bits": (2, 34), "rank off by one": (2, 33),
         "32-bit clz, the g half ignored": (10, 7), "last writer wins instead of max": (1, 19),
         "histogram not recounted on merge": (21, 4), "stored byte above q+1 not clamped": (0, 16),
         "last element of a ragged segment dropped": (2, 19), "first element of an unaligned column dropped": (2, 14),
         "bad row id read as row 0": (12, 1), "status not raised": (0, 23), "status not cleared": (2, 36)}


@pytest.fixture(scope="module")
def sweep():
    cases = hf.cases()
    return cases, [hf.model(c) for c in cases]


def rejected(case, want, result):
    try:
        fz.same(case, result, want)
    except AssertionError:
        return True
    return False


def test_the_draws_hold_every_category(sweep):
    cases, _ = sweep
    assert 55 <= len(cases) <= 65 and [c["draw"] for c in cases] == list(range(len(cases)))
    assert max(c["size"] for c in cases) <= 1 << 17
    sizes = {c["size"] for c in cases}
    assert {0, 1, 63, 64, 65, hf.SEG - 1, hf.SEG, hf.SEG + 1, 2 * hf.SEG - 1, 2 * hf.SEG, 2 * hf.SEG + 1} <= sizes
    builds = [c for c in cases if c["what"] == "build"]
    merges = [c for c in cases if c["what"] == "merge"]
    assert len(merges) >= 5 and len(builds) >= 40
    assert set(hf.PS) <= {c["p"] for c in builds} and {4, 14} <= {c["p"] for c in merges} | {c["p"] for c in builds}
    assert {len(c["cols"]) for c in builds} == {1, 2, 3, 4}
    for listed in (False, True):
        mine = [c for c in builds if (c["rows"] is not None) == listed]
        assert set(fz.COUNT_KINDS) <= {fz.count_kind(c["count"], c["size"]) for c in mine}, listed
        assert {c["accumulate"] for c in mine} == {False, True}
        assert any(c["built"] for c in mine) and any(not c["built"] for c in mine)
    assert {o for c in builds for o in c["offs"]["cols"]} == {0, 1, 2, 3} == {c["offs"]["rows"] for c in builds if c["rows"] is not None}
    assert any(len(set(c["offs"]["cols"])) > 1 for c in builds)  # columns of one call at different offsets
    assert {c["fill"] for c in builds} == set(fz.FILLS) and len({c["seed"] for c in builds}) > 3 and 0 in {c["seed"] for c in builds}
    assert any(c["rows"] is not None and (c["rows"][: fz.counted(c["count"], c["size"])] >= c["cols"][0].size).any() for c in builds)
    assert any(c["cols"][0].size == 0 for c in builds)
    assert {c["held"] for c in builds if c["accumulate"]} == set(hf.BEFORE) == {c["held"] for c in builds if not c["accumulate"]}
    assert len({c["stale_status"] for c in cases}) >= 3
    assert {c["same_buffer"] for c in merges} == {False, True}
    assert {"sketch", "spoiled"} <= {c["held"] for c in merges} and {"sketch", "spoiled"} <= {c["src_held"] for c in merges}


def test_the_intact_model_is_hll_models(sweep):
    for case, want in zip(*sweep):
        if case["what"] == "build":
            regs, hist, st = hm.build(case["cols"], case["p"], case["seed"], case["rows"], case["count"], case["flags"], case["before"])
        else:
            regs, hist, st = hm.merge(case["dst"], case["src"], case["p"])
        assert st == want["status"] and np.array_equal(regs, want["registers"]) and np.array_equal(hist, want["hist"]), case["draw"]
        assert int(want["hist"].sum()) == 1 << case["p"] and int(want["registers"].max()) <= 64 - case["p"] + 1


@pytest.mark.parametrize("defect", hf.DEFECTS)
def test_every_defect_is_rejected_by_some_draw(sweep, defect):
    cases, wants = sweep
    hits = [c["draw"] for c, want in zip(cases, wants) if rejected(c, want, hf.model(c, defect))]
    assert hits, f"no draw rejects a call with '{defect}'"
    assert (hits[0], len(hits)) == FIRST[defect], (defect, hits[0], len(hits))
    assert f"{defect:<48} draw {hits[0]:>2}   {len(hits):>2} draws" in __doc__


def test_the_32_bit_clz_is_rejected_only_by_keys_built_against_the_hash(sweep):
    cases, wants = sweep
    hits = [c for c, want in zip(cases, wants) if rejected(c, want, hf.model(c, "32-bit clz, the g half ignored"))]
    assert hits and all(c["what"] == "build" and c["built"] for c in hits)


def test_the_table_names_every_defect():
    assert set(FIRST) == set(hf.DEFECTS) and len(hf.DEFECTS) == 18
