"""The merge-path entry points under hipGraph capture: a merge captured once and replayed with device counts that differ
by orders of magnitude, and the chain select -> select -> union captured once and replayed with one side empty, both
sides full and both sides sparse.  The counts travel on the device, so the one captured sequence must follow them.
Helpers of tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import merge_native as mn
from dwarf_bench_amd import ops
from tests import graph_testlib as gt
from tests import merge_model as mm

pytestmark = pytest.mark.gpu

T = mn.TILE_ROWS
NA, NB = 40 * T + 3, 25 * T - 1
N = 100003
BOUNDS = (100, 199)  # frozen into the graph; the data decides what passes


def count_words(value):
    """a device count as the two 32-bit words graph_testlib.fill copies into an int32 tensor"""
    return np.array([value], dtype=np.uint64).view(np.uint32)


def make_merge():
    plan = ops.MergeSorted(NA, NB)
    a, b = (torch.zeros(n, dtype=torch.int32, device="cuda") for n in (NA, NB))
    counts = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2)]  # each one int64

    def run():
        plan.launch(a, b, a_count=counts[0].view(torch.int64), b_count=counts[1].view(torch.int64), row_ids=True)

    def read():
        m = plan.count()
        return {"keys": gt.u32(plan.out_keys[:m]).copy(), "ids": gt.u32(plan.out_vals[:m]).copy(), "count": np.array([m])}

    return gt.Buffers([a, b] + counts, [plan.out_keys, plan.out_vals, plan.out_count], [plan.ws], [plan.ws], run, read)


def merge_inputs():
    rng = np.random.default_rng(23)
    shapes = [("a tenth of each", NA // 10, NB // 10), ("both full", NA, NB), ("nothing", 0, 0), ("three rows against all", 3, NB),
              ("all against one row", NA, 1), ("counts above the capacities", 1 << 40, NB + 1), ("one tile", T // 2, T // 2)]
    out = []
    for name, ca, cb in shapes:
        a = np.sort(rng.integers(0, 1 << 20, NA, dtype=np.uint64)).astype(np.uint32)
        b = np.sort(rng.integers(0, 1 << 20, NB, dtype=np.uint64)).astype(np.uint32)
        out.append(gt.Input([a, b, count_words(ca), count_words(cb)], name=name, counts=(ca, cb)))
    return out


def check_merge(inp, got):
    ca, cb = inp.facts["counts"]
    keys, ids, count, _ = mm.merge(inp.cols[0], inp.cols[1], mm.ROW_IDS, a_count=ca, b_count=cb)
    assert got["count"][0] == count and np.array_equal(got["keys"], keys) and np.array_equal(got["ids"], ids)


def test_merge_replays_follow_the_device_counts():
    ins = merge_inputs()
    sizes = [min(i.facts["counts"][0], NA) + min(i.facts["counts"][1], NB) for i in ins]
    assert 0 in sizes and NA + NB in sizes and 0 < min(s for s in sizes if s) * 10 < NA + NB  # orders of magnitude apart
    seen = gt.run_family(make_merge, ins, check_merge)
    assert all(st == (0,) for st in seen)


def make_chain():
    first, second, sets = ops.SelectRows(N), ops.SelectRows(N), ops.RowSets(N, N)
    cols = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]

    def run():
        first.launch(cols[0], *BOUNDS)
        second.launch(cols[1], *BOUNDS)
        (rows_a, count_a), (rows_b, count_b) = first.output(), second.output()  # nothing is read back
        sets.launch("union", rows_a, rows_b, count_a, count_b)

    def read():
        return {"rows": gt.u32(sets.rows[: sets.count()]).copy(), "count": np.array([sets.count()])}

    outputs = first.rows + [first.counts] + second.rows + [second.counts, sets.rows, sets.out_count]
    work = [first.ws, second.ws, sets.ws]
    return gt.Buffers(cols, outputs, work, work, run, read)


def column(rng, share):
    """values in [100, 199] in about `share` of the rows, elsewhere outside"""
    inside = rng.integers(100, 200, N, dtype=np.uint64)
    outside = np.where(rng.integers(0, 2, N) == 1, rng.integers(0, 100, N, dtype=np.uint64),
                       rng.integers(200, 1 << 32, N, dtype=np.uint64))
    return np.where(rng.random(N) < share, inside, outside).astype(np.uint32)


def chain_inputs():
    rng = np.random.default_rng(29)
    shares = [("half and half", (0.5, 0.5)), ("the first side empty", (0.0, 0.5)), ("both sides full", (1.0, 1.0)),
              ("both sides sparse", (0.001, 0.001)), ("the second side empty", (1.0, 0.0)), ("both empty", (0.0, 0.0))]
    return [gt.Input([column(rng, s) for s in share], name=name) for name, share in shares]


def check_chain(inp, got):
    ka, kb = ((c >= BOUNDS[0]) & (c <= BOUNDS[1]) for c in inp.cols)
    want = np.flatnonzero(ka | kb)
    assert got["count"][0] == want.size and np.array_equal(got["rows"], want)
    assert np.array_equal(want, mm.setop(mm.UNION, np.flatnonzero(ka), np.flatnonzero(kb))[0])


def test_chain_select_select_union_replays_follow_the_device_counts():
    ins = chain_inputs()
    sizes = [int(((c >= 100) & (c <= 199)).sum()) for i in ins for c in i.cols]
    assert 0 in sizes and N in sizes and 0 < min(s for s in sizes if s) * 100 < N
    seen = gt.run_family(make_chain, ins, check_chain)
    assert all(st == (0, 0, 0) for st in seen)


def test_chain_captured_on_a_stream_of_the_callers_choice():
    ins = chain_inputs()
    bufs = make_chain()
    bufs.twin = make_chain()
    bufs.prepare(ins[0], gt.FILLS[0], "zeros")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        bufs.run()  # warm-up on that stream
    stream.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        bufs.run()
    seen = gt.replay_sequence(graph, bufs, ins[1:] + ins[:1], check_chain)
    assert all(st == (0, 0, 0) for st in seen)
