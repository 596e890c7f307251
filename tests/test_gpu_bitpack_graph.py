"""Bit-packed columns under hipGraph capture: build of a dictionary -> encode -> pack at the dictionary's width ->
select_range on the packed codes over a row-id list -> refine on a plain column -> unpack through the resulting list,
captured once and replayed over other data and other device-side counts (the rows that count, and with them the length
of every list down the chain, travel on the device).  Every replay is compared with numpy.  Helpers of
tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import bitpack_model as bm
from tests import graph_testlib as gt

pytestmark = pytest.mark.gpu

N, CAP = 9001, 200  # rows (three segments of the filter, five tiles of pack), the dictionary's capacity: eight bits
LO, HI = 20, 150    # the filter on the codes
OTHER_HI = 1 << 31  # and on the plain column
U = np.uint32


def make():
    d, sel = ops.Dictionary(N, CAP), ops.SelectRows(N)
    packer = ops.BitPack(N, d.packed_width())
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    src, other, iota, count32 = i32(N), i32(N), i32(N), i32(2)
    count = count32.view(torch.int64)  # one device uint64, refilled as two words
    codes, values = i32(N), i32(N)
    unpack_ws = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def run():
        d.build(src, count)
        d.encode(src, count, out=codes)
        packer.launch(codes, count)
        pc = packer.output()
        sel.launch(pc, LO, HI, rows=iota, count=count)
        sel.refine(other, 0, OTHER_HI)
        rows, kept = sel.output()
        ops.unpack(pc, rows, count=kept, out=values, ws=unpack_ws)

    def read():
        torch.cuda.synchronize()
        m = min(int(count.item()), N)
        rows, kept = sel.output()
        k = int(kept.item())
        words = bm.words(m, packer.width)
        tails = [gt.u32(codes[m:]), gt.u32(packer.packed[words:]), gt.u32(values[k:]), gt.u32(rows[k:])]
        return {"count": np.array([m, k]), "codes": gt.u32(codes[:m]).copy(), "packed": gt.u32(packer.packed[:words]).copy(),
                "rows": gt.u32(rows[:k]).copy(), "values": gt.u32(values[:k]).copy(),
                "tails untouched": np.array([t.size == 0 or (bool((t == t[0]).all()) and int(t[0]) in gt.FILLS) for t in tails])}

    workspaces = [d.ws, packer.ws, sel.ws, unpack_ws]
    outputs = [d.keys, d.count_dev, codes, packer.packed, sel.rows[0], sel.rows[1], sel.counts, values]
    return gt.Buffers([src, other, iota, count32], outputs, workspaces, workspaces, run, read)


def one_input(rng, name, distinct, count):
    keys = rng.permutation(np.unique(np.r_[np.array([0, 0xFFFFFFFF], U), rng.integers(0, 1 << 32, distinct + 4, dtype=np.uint64)
                                           .astype(U)]))[:distinct]
    src = keys[rng.integers(0, distinct, N)]
    other = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(U)
    words = np.array([count & 0xFFFFFFFF, count >> 32], U)
    return gt.Input([src, other, np.arange(N, dtype=U), words], status=0, name=name, count=count)


def inputs():
    rng = np.random.default_rng(77)
    return [one_input(rng, "half the rows", CAP, N // 2), one_input(rng, "all rows", 180, N),
            one_input(rng, "a count beyond the column", CAP, (1 << 40) + 9), one_input(rng, "no row counts", 50, 0),
            one_input(rng, "one row", CAP, 1), one_input(rng, "few values: nothing passes the first filter", 15, 4097),
            one_input(rng, "a segment and a bit", 190, 4096 + 31)]


def check(inp, got):
    src, other, _, _ = inp.cols
    m = min(inp.facts["count"], N)
    keys, codes = np.unique(src[:m], return_inverse=True)
    codes = codes.astype(U)
    assert got["count"][0] == m and got["tails untouched"].all()
    assert np.array_equal(got["codes"], codes)
    assert np.array_equal(got["packed"], bm.pack_codes(codes, 8))
    keep = (codes >= LO) & (codes <= HI) & (other[:m] <= OTHER_HI)
    assert got["count"][1] == keep.sum() and np.array_equal(got["rows"], np.nonzero(keep)[0])
    assert np.array_equal(got["values"], codes[keep])


def test_chain_replays_follow_the_data_and_the_device_counts():
    ins = inputs()
    kept = []
    for inp in ins:
        m = min(inp.facts["count"], N)
        codes = np.unique(inp.cols[0][:m], return_inverse=True)[1]
        kept.append(int(((codes >= LO) & (codes <= HI)).sum()))
    assert kept[0] > 0 and kept[1] > 0 and kept[3] == 0 and kept[5] == 0 and len(set(kept)) >= 5  # the replays differ
    seen = gt.run_family(make, ins, check)
    assert all(st == (0, 0, 0, 0) for st in seen)
