"""The HyperLogLog sketch under hipGraph capture: select_range on an attribute column -> HyperLogLog.build of two key columns
through that list and its device count -> a second sketch built from another column -> merge of the first into it, captured
once and replayed over other data (the rows that count, and with them the first sketch, travel on the device: one replay
selects no row, one every row).  Every replay is compared bit for bit with the numpy model (tests/hll_model.py).  A second
test runs the same family in a fresh process with no eager call of the family in front of the capture, as
tests/test_gpu_graph_first_capture.py does for the other families.  Helpers of tests/graph_testlib.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import graph_testlib as gt
from tests import hll_model as hm

pytestmark = pytest.mark.gpu

N = 9001          # three segments of the select and of the build, the last one ragged
P, SEED = 11, 12345
LO, HI = 100, 1 << 30  # the filter on the attribute
U, B = np.uint32, np.uint8


def make():
    sel, first, second = ops.SelectRows(N), ops.HyperLogLog(P, SEED), ops.HyperLogLog(P, SEED)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    attr, key_a, key_b, other = i32(N), i32(N), i32(N), i32(N)

    def run():
        sel.launch(attr, LO, HI)
        rows, kept = sel.output()
        first.build([key_a, key_b], rows=rows, count=kept)
        second.build(other)
        second.merge(first)

    def read():
        torch.cuda.synchronize()
        rows, kept = sel.output()
        k = int(kept.item())
        tail = gt.u32(rows[k:N])
        return {"count": np.array([k]), "rows": gt.u32(rows[:k]).copy(),
                "first": first.registers.cpu().numpy().copy(), "first hist": gt.u32(first.hist).copy(),
                "second": second.registers.cpu().numpy().copy(), "second hist": gt.u32(second.hist).copy(),
                "estimate": np.array([second.estimate()]),
                "tail untouched": np.array([tail.size == 0 or (bool((tail == tail[0]).all()) and int(tail[0]) in gt.FILLS)])}

    workspaces = [sel.ws, first.ws, second.ws]
    outputs = [sel.rows[0], sel.rows[1], sel.counts, first.registers.view(torch.int32), first.hist,
               second.registers.view(torch.int32), second.hist]
    return gt.Buffers([attr, key_a, key_b, other], outputs, workspaces, workspaces, run, read)


def one_input(rng, name, attr_lo=0, attr_hi=1 << 31, distinct=2000):
    attr = rng.integers(attr_lo, attr_hi, N, dtype=np.uint64).astype(U)
    key_a = rng.integers(0, distinct, N).astype(U)
    key_b = rng.integers(0, 3, N).astype(U)
    other = rng.integers(0, 1 << 32, N // 2, dtype=np.uint64).astype(U)[rng.integers(0, N // 2, N)]
    return gt.Input([attr, key_a, key_b, other], status=0, name=name)


def inputs():
    rng = np.random.default_rng(79)
    return [one_input(rng, "half the rows pass"), one_input(rng, "every row passes", LO, HI + 1, distinct=1 << 20),
            one_input(rng, "no row passes: the first sketch is empty", 0, LO), one_input(rng, "few distinct tuples", distinct=5),
            one_input(rng, "every row again", LO, LO + 1)]


def expected(inp):
    attr, key_a, key_b, other = inp.cols
    rows = np.flatnonzero((attr >= LO) & (attr <= HI)).astype(U)
    first = hm.build([key_a, key_b], P, SEED, rows=rows)
    second = hm.merge(hm.build(other, P, SEED)[0], first[0], P)
    return rows, first, second


def check(inp, got):
    rows, first, second = expected(inp)
    assert got["tail untouched"].all()
    assert got["count"][0] == rows.size and np.array_equal(got["rows"], rows)
    assert np.array_equal(got["first"], first[0]) and np.array_equal(got["first hist"], first[1])
    assert np.array_equal(got["second"], second[0]) and np.array_equal(got["second hist"], second[1])
    assert got["estimate"][0] == hm.estimate(second[1], P)


def test_chain_replays_follow_the_data_and_the_device_count():
    ins = inputs()
    kept = [expected(inp)[0].size for inp in ins]
    assert kept[1] == N == kept[4] and kept[2] == 0 and 0 < kept[0] < N and 0 < kept[3] < N  # the replays differ
    assert not expected(ins[2])[1][0].any() and expected(ins[2])[2][0].any()
    truth = np.unique(np.r_[ins[1].cols[1].astype(np.uint64) * 4 + ins[1].cols[2], (1 << 40) + ins[1].cols[3].astype(np.uint64)]).size
    e = hm.estimate(expected(ins[1])[2][1], P)
    assert abs(e - truth) <= 8 * hm.relative_error(P) * truth  # (tuples and single keys hash apart: about the union's size)
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
            "from tests import test_gpu_hll_graph as t\n"
            "gl.FIRST_CAPTURE = True\n"
            "t.test_chain_replays_follow_the_data_and_the_device_count()\n"
            "print('ok hll')\n")
    try:
        r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(__file__)))
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child (hll) hung: {e}", returncode=3)
    if r.returncode in (-6, -11, 134, 139):  # an abort or a fault on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child (hll) died with {r.returncode}: {r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0 and "ok hll" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
