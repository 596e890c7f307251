"""Late materialisation under hipGraph capture: select_range -> refine -> take of two columns -> aggregate of a third
captured once and replayed over columns whose surviving counts differ by orders of magnitude (no row, every row).  The
counts travel on the device, so the one captured sequence must follow them.  Helpers of tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import graph_testlib as gt
from tests import select_model as sm
from tests import take_model as tm

pytestmark = pytest.mark.gpu

N = 100003
BOUNDS = [(100, 199), (100, 199)]  # frozen into the graph; the data decides what passes


def make():
    sel, taker, agg = ops.SelectRows(N), ops.TakeRows(N, 2), ops.AggregateRows(N)
    cols = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(5)]  # two filter columns, three payloads

    def run():
        sel.launch(cols[0], *BOUNDS[0])
        sel.refine(cols[1], *BOUNDS[1])
        rows, count = sel.output()
        taker.launch([cols[2], cols[3]], rows, count)
        agg.launch(cols[4], rows, count, signed=True)

    def read():
        torch.cuda.synchronize()
        m = sel.count()
        tails = [gt.u32(o[m:]) for o in taker.outs]  # behind the count: still the guard word replay_sequence put there
        return {"count": np.array([m]), "rows": gt.u32(sel.result(strict=False)).copy(),
                "taken 0": gt.u32(taker.outs[0][:m]).copy(), "taken 1": gt.u32(taker.outs[1][:m]).copy(),
                "tails untouched": np.array([t.size == 0 or (bool((t == t[0]).all()) and int(t[0]) in gt.FILLS) for t in tails]),
                "aggregate": agg.out.cpu().numpy().view(np.uint64).copy()}

    workspaces = [sel.ws, taker.ws, agg.ws]
    return gt.Buffers(cols, sel.rows + [sel.counts] + taker.outs + [agg.out], workspaces, workspaces, run, read)


def column(rng, share):
    """values in [100, 199] in about `share` of the rows, elsewhere outside"""
    inside = rng.integers(100, 200, N, dtype=np.uint64)
    outside = np.where(rng.integers(0, 2, N) == 1, rng.integers(0, 100, N, dtype=np.uint64),
                       rng.integers(200, 1 << 32, N, dtype=np.uint64))
    return np.where(rng.random(N) < share, inside, outside).astype(np.uint32)


def inputs():
    rng = np.random.default_rng(19)
    shares = [("half, a thousandth", (0.5, 0.001)), ("every row survives", (1.0, 1.0)), ("no row survives", (0.5, 0.0)),
              ("nothing from the start", (0.0, 1.0)), ("all, a hundredth", (1.0, 0.01)), ("a thousandth, all", (0.001, 1.0))]
    payload = lambda: rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    return [gt.Input([column(rng, s) for s in share] + [payload(), payload(), payload()], name=name) for name, share in shares]


def check(inp, got):
    want = sm.chain(inp.cols[:2], BOUNDS)
    assert got["count"][0] == want.size and np.array_equal(got["rows"], want)
    assert np.array_equal(got["taken 0"], inp.cols[2][want]) and np.array_equal(got["taken 1"], inp.cols[3][want])
    assert got["tails untouched"].all()
    words, status = tm.aggregate(inp.cols[4], want.astype(np.uint32), flags=tm.SIGNED)
    assert status == 0 and tuple(int(w) for w in got["aggregate"]) == words


def test_chain_replays_follow_the_device_counts():
    ins = inputs()
    sizes = [sm.chain(i.cols[:2], BOUNDS).size for i in ins]
    assert 0 in sizes and N in sizes and 0 < min(s for s in sizes if s) * 100 < N  # orders of magnitude apart
    seen = gt.run_family(make, ins, check)
    assert all(st == (0, 0, 0) for st in seen)


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
    assert all(st == (0, 0, 0) for st in seen)
