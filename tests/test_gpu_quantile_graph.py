"""The quantile select under hipGraph capture: select_range on an attribute column -> Quantiles.launch on a value column through
that list and its device count, and a second plan over all rows of the value column, captured once and replayed over other
data: the rows that pass, and with them m and every answer, change on the device from replay to replay (one replay selects no
row, one every row), while the ranks — host values — stay what the capture froze.  Every replay is compared with the numpy
model (tests/quantile_model.py).  A second test runs the same family in a fresh process with no eager call of the family in
front of the capture, as tests/test_gpu_graph_first_capture.py does for the other families.  Helpers of tests/graph_testlib.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import graph_testlib as gt
from tests import quantile_model as qm

pytestmark = pytest.mark.gpu

N = 2 * 8192 + 617  # three rounds of the histogram kernel, the last one ragged
LO, HI = 100, 1 << 30  # the filter on the attribute
QS = [(1, 2), (1, 10), (9, 10), 0, 5000, (1, 1)]  # five ranks resolved against m, and an absolute one that may name no row
ALL = [(i, 10) for i in range(1, 10)]
U = np.uint32


def make():
    sel, listed, dense = ops.SelectRows(N), ops.Quantiles(len(QS)), ops.Quantiles(len(ALL))
    attr = torch.zeros(N, dtype=torch.int32, device="cuda")
    vals = torch.zeros(N, dtype=torch.int32, device="cuda")

    def run():
        sel.launch(attr, LO, HI)
        rows, kept = sel.output()
        listed.launch(vals, QS, rows=rows, count=kept, signed=True)
        dense.launch(vals, ALL)

    def read():
        torch.cuda.synchronize()
        _, kept = sel.output()
        return {"count": np.array([int(kept.item())]), "listed": gt.u32(listed.out).copy(), "dense": gt.u32(dense.out).copy()}

    workspaces = [sel.ws, listed.ws, dense.ws]
    return gt.Buffers([attr, vals], [sel.rows[0], sel.rows[1], sel.counts, listed.out, dense.out], workspaces, workspaces, run, read)


def one_input(rng, name, attr_lo=0, attr_hi=1 << 31, kind="random"):
    attr = rng.integers(attr_lo, attr_hi, N, dtype=np.uint64).astype(U)
    vals = (rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(U) if kind == "random" else
            rng.integers(1, 10001, N).astype(U) if kind == "reference" else np.full(N, 0x80000001, U))
    return gt.Input([attr, vals], status=0, name=name)


def inputs():
    rng = np.random.default_rng(83)
    return [one_input(rng, "half the rows pass"), one_input(rng, "every row passes", LO, HI + 1, "reference"),
            one_input(rng, "no row passes: no rank names a row", 0, LO), one_input(rng, "half again, all keys equal", kind="equal"),
            one_input(rng, "every row again", LO, LO + 1)]


def expected(inp):
    attr, vals = inp.cols
    rows = np.flatnonzero((attr >= LO) & (attr <= HI)).astype(U)
    num, den = ops._quantile_ranks(QS)
    listed = qm.select(vals, num, den, qm.SIGNED, rows=rows)
    num, den = ops._quantile_ranks(ALL)
    return rows, listed, qm.select(vals, num, den)


def check(inp, got):
    rows, listed, dense = expected(inp)
    assert got["count"][0] == rows.size
    assert np.array_equal(got["listed"], np.stack(listed[:3])), (got["listed"], listed)
    assert np.array_equal(got["dense"], np.stack(dense[:3])), (got["dense"], dense)


def test_chain_replays_follow_the_data_and_the_device_count():
    ins = inputs()
    kept = [expected(inp)[0].size for inp in ins]
    assert kept[1] == N == kept[4] and kept[2] == 0 and 0 < kept[0] < N and 0 < kept[3] < N  # the replays differ in m
    answers = [expected(inp)[1] for inp in ins]
    assert not answers[2][2].any() and answers[1][2].all() and answers[4][2].all()  # no rank names a row; every rank does
    assert len({tuple(a[0].tolist()) for a in answers}) == len(ins)  # every replay has answers of its own
    seen = gt.run_family(make, ins, check)
    assert all(st == (0, 0, 0) for st in seen)


def test_first_capture_of_a_process():
    """the capture is the first call of the family in a fresh process: no warm-up run in front of it.  A child that hangs,
    aborts or faults ends the whole session, as in tests/test_gpu_graph_first_capture.py: after a fault or a hang on the GPU
    nothing more is started on it"""
    prog = ("import torch\n"
            "from dwarf_bench_amd import ops\n"
            "ops.reduce_sum(ops.gen_uniform_u32(1024, 1, 0, 9)); torch.cuda.synchronize()  # loads the code object\n"
            "from tests import graph_testlib as gl\n"
            "from tests import test_gpu_quantile_graph as t\n"
            "gl.FIRST_CAPTURE = True\n"
            "t.test_chain_replays_follow_the_data_and_the_device_count()\n"
            "print('ok quantile')\n")
    try:
        r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(__file__)))
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child (quantile) hung: {e}", returncode=3)
    if r.returncode in (-6, -11, 134, 139):  # an abort or a fault on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child (quantile) died with {r.returncode}: {r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0 and "ok quantile" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
