"""The selection vectors under hipGraph capture: select_range -> refine -> refine captured once and replayed over columns
whose intermediate counts differ by orders of magnitude (an empty intermediate list, every row surviving).  The counts
travel on the device, so the one captured sequence must follow them.  Helpers of tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import graph_testlib as gt
from tests import select_model as sm

pytestmark = pytest.mark.gpu

N = 100003
BOUNDS = [(100, 199), (100, 199), (100, 199)]  # frozen into the graph; the data decides what passes


def make():
    plan = ops.SelectRows(N)
    cols = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(3)]

    def run():
        plan.launch(cols[0], *BOUNDS[0])
        plan.refine(cols[1], *BOUNDS[1])
        plan.refine(cols[2], *BOUNDS[2])

    def read():
        return {"rows": plan.result(strict=False).cpu().numpy().view(np.uint32).copy(),
                "count": np.array([plan.count()])}

    return gt.Buffers(cols, plan.rows + [plan.counts], [plan.ws], [plan.ws], run, read)


def column(rng, share):
    """values in [100, 199] in about `share` of the rows, elsewhere outside"""
    inside = rng.integers(100, 200, N, dtype=np.uint64)
    outside = np.where(rng.integers(0, 2, N) == 1, rng.integers(0, 100, N, dtype=np.uint64),
                       rng.integers(200, 1 << 32, N, dtype=np.uint64))
    return np.where(rng.random(N) < share, inside, outside).astype(np.uint32)


def inputs():
    rng = np.random.default_rng(17)
    shares = [("half, a thousandth, half", (0.5, 0.001, 0.5)), ("every row survives", (1.0, 1.0, 1.0)),
              ("an empty intermediate list", (0.5, 0.0, 1.0)), ("nothing from the start", (0.0, 1.0, 1.0)),
              ("all, all, a thousandth", (1.0, 1.0, 0.001)), ("a thousandth, all, all", (0.001, 1.0, 1.0))]
    return [gt.Input([column(rng, s) for s in share], name=name) for name, share in shares]


def check(inp, got):
    want = sm.chain(inp.cols, BOUNDS)
    assert got["count"][0] == want.size and np.array_equal(got["rows"], want)
    inside = [(c >= 100) & (c <= 199) for c in inp.cols]
    assert np.array_equal(want, np.flatnonzero(inside[0] & inside[1] & inside[2]))


def test_chain_replays_follow_the_device_counts():
    ins = inputs()
    sizes = [sm.chain(i.cols[:2], BOUNDS[:2]).size for i in ins]
    assert 0 in sizes and N in sizes and 0 < min(s for s in sizes if s) * 100 < N  # orders of magnitude apart
    seen = gt.run_family(make, ins, check)
    assert all(st == (0,) for st in seen)


def test_chain_captured_on_a_stream_of_the_callers_choice():
    ins = inputs()
    bufs = make()
    bufs.twin = make()
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
    seen = gt.replay_sequence(graph, bufs, ins[1:] + ins[:1], check)
    assert all(st == (0,) for st in seen)
