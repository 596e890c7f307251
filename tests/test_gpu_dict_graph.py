"""Dictionary encoding under hipGraph capture: take of two columns through a row-id list -> build of a dictionary on each
-> encode of both -> combine -> encode of another column through the first dictionary, captured once and replayed over
lists of other lengths (the count travels on the device) and over inputs that take the first dictionary from OK to
TABLE_FULL and back.  Every replay is compared with the numpy model.  Helpers of tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import dict_model as dm
from tests import graph_testlib as gt

pytestmark = pytest.mark.gpu

ROWS, N, CAP = 5003, 20011, 60  # rows of the table, entries of the list, the capacity of both dictionaries
U = np.uint32


def make():
    taker, dict_a, dict_b = ops.TakeRows(N, 2), ops.Dictionary(N, CAP), ops.Dictionary(N, CAP)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    src_a, src_b, other, rows, count32 = i32(ROWS), i32(ROWS), i32(N), i32(N), i32(2)
    count = count32.view(torch.int64)  # one device uint64, refilled as two words
    codes_a, codes_b, composite, codes_other = i32(N), i32(N), i32(N), i32(N)
    misses = torch.zeros(1, dtype=torch.int64, device="cuda")
    combine_ws = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def run():
        taker.launch([src_a, src_b], rows, count)
        (a, b), _ = taker.output()
        dict_a.build(a, count)
        dict_b.build(b, count, signed=True)
        dict_a.encode(a, count, out=codes_a)
        dict_b.encode(b, count, out=codes_b)
        ops.dict_combine(codes_a, codes_b, dict_a.count_dev, dict_b.count_dev, count, out=composite, ws=combine_ws)
        dict_a.encode(other, out=codes_other, misses=misses)

    def read():
        torch.cuda.synchronize()
        m = min(int(count.item()), N)
        da, db = int(dict_a.count_dev.item()), int(dict_b.count_dev.item())
        tails = [gt.u32(t[m:]) for t in (codes_a, codes_b, composite)]  # behind the count: still the guard word
        return {"count": np.array([m]), "keys a": gt.u32(dict_a.keys[:da]).copy(), "keys b": gt.u32(dict_b.keys[:db]).copy(),
                "codes a": gt.u32(codes_a[:m]).copy(), "codes b": gt.u32(codes_b[:m]).copy(),
                "composite": gt.u32(composite[:m]).copy(), "codes other": gt.u32(codes_other).copy(),
                "misses": misses.cpu().numpy().copy(),
                "tails untouched": np.array([t.size == 0 or (bool((t == t[0]).all()) and int(t[0]) in gt.FILLS) for t in tails])}

    workspaces = [taker.ws, dict_a.ws, dict_b.ws, combine_ws]
    outputs = taker.outs + [dict_a.keys, dict_b.keys, dict_a.count_dev, dict_b.count_dev, codes_a, codes_b, composite, codes_other,
                            misses]
    return gt.Buffers([src_a, src_b, other, rows, count32], outputs, workspaces, workspaces, run, read)


def one_input(rng, name, distinct_a, distinct_b, count):
    """a table whose columns hold distinct_a and distinct_b values, a list over all of it, `count` entries of which count"""
    values_a = rng.permutation(np.unique(np.r_[np.array([0, 0xFFFFFFFF], U), rng.integers(0, 1 << 32, distinct_a + 4, dtype=np.uint64)
                                               .astype(U)]))[:distinct_a]
    values_b = rng.permutation(np.unique(np.r_[np.array([0x80000000, 0x7FFFFFFF], U), rng.integers(0, 1 << 32, distinct_b + 4,
                                                                                                   dtype=np.uint64).astype(U)]))[:distinct_b]
    src_a = values_a[np.arange(ROWS) % distinct_a]  # every value occurs
    src_b = values_b[rng.integers(0, distinct_b, ROWS)]
    rows = np.r_[np.arange(ROWS), rng.integers(0, ROWS, N - ROWS)].astype(U)  # the first ROWS entries reach every row
    other = np.where(rng.integers(0, 3, N) == 0, rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(U), values_a[rng.integers(0, distinct_a, N)])
    m = min(count, N)
    seen_a = np.unique(src_a[rows[:m]]).size
    full = dm.TABLE_FULL if seen_a > CAP else 0
    words = np.array([count & 0xFFFFFFFF, count >> 32], U)
    return gt.Input([src_a, src_b, other, rows, words], status=(0, full, 0, 0), name=name, count=count)


def inputs():
    rng = np.random.default_rng(41)
    return [one_input(rng, "half the list", 40, 7, N // 2), one_input(rng, "the whole list, the capacity exactly", CAP, 3, N),
            one_input(rng, "one value too many", CAP + 1, 5, N), one_input(rng, "a count beyond the list", 12, CAP, (1 << 40) + 5),
            one_input(rng, "too many again, a short list", 300, 9, 1500), one_input(rng, "no entry counts", 33, 4, 0),
            one_input(rng, "too many values but few counted", 5000, 2, 45), one_input(rng, "one entry", 50, 50, 1)]


def check(inp, got):
    src_a, src_b, other, rows, _ = inp.cols
    m = min(inp.facts["count"], N)
    assert got["count"][0] == m and got["tails untouched"].all()
    a, b = src_a[rows[:m]], src_b[rows[:m]]
    keys_a, st_a = dm.build(a, CAP)
    keys_b, st_b = dm.build(b, CAP, flags=dm.SIGNED)
    assert (0, st_a, st_b, 0) == tuple(inp.status)
    assert np.array_equal(got["keys a"], keys_a) and np.array_equal(got["keys b"], keys_b)
    codes_a, codes_b = dm.encode(keys_a, a)[0], dm.encode(keys_b, b, flags=dm.SIGNED)[0]
    assert np.array_equal(got["codes a"], codes_a) and np.array_equal(got["codes b"], codes_b)
    composite, st = dm.combine(codes_a, codes_b, keys_a.size, keys_b.size)
    assert st == 0 and np.array_equal(got["composite"], composite)
    codes_other, misses = dm.encode(keys_a, other)
    assert np.array_equal(got["codes other"], codes_other) and int(got["misses"][0]) == misses


def test_chain_replays_follow_the_device_counts_and_the_overflow():
    ins = inputs()
    assert [i.status[1] for i in ins].count(dm.TABLE_FULL) == 2 and ins[0].status[1] == 0 and ins[-1].status[1] == 0
    seen = gt.run_family(make, ins, check)
    assert [st[1] for st in seen] == [i.status[1] for i in ins + ins[:1]]


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
    assert [st[1] for st in seen] == [i.status[1] for i in ins[1:] + ins[:1]]
