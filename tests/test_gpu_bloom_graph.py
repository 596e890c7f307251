"""The Bloom filter under hipGraph capture: select_range on a dimension column -> BloomFilter.build through that list and its
device count -> SelectRows.launch_in on a fact column -> refine on a plain column -> take, captured once and replayed over
other data and other device-side counts (the dimension rows that count, and with them the filter and the length of every
list down the chain, travel on the device).  Every replay is compared with the numpy model (tests/bloom_model.py).  Helpers
of tests/graph_testlib.py."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import ops
from tests import bloom_model as blm
from tests import graph_testlib as gt

pytestmark = pytest.mark.gpu

ND, NF = 5003, 9001   # dimension rows (two segments of the select and of the build), fact rows (three segments of the probe)
WORDS, SEED = 101, 12345  # few bits per key: false positives are part of every answer
LO, HI = 100, 1 << 30  # the filter on the dimension's attribute
OTHER_HI = 3 << 30     # and on the fact table's plain column
U, W = np.uint32, np.uint64


def make():
    dim_sel, fact_sel, bloom, taker = ops.SelectRows(ND), ops.SelectRows(NF), ops.BloomFilter(WORDS, SEED), ops.TakeRows(NF)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    dim_key, dim_attr, iota, fact_key, fact_other, fact_val, count32 = i32(ND), i32(ND), i32(ND), i32(NF), i32(NF), i32(NF), i32(2)
    count = count32.view(torch.int64)  # one device uint64, refilled as two words

    def run():
        dim_sel.launch(dim_attr, LO, HI, rows=iota, count=count)
        rows, kept = dim_sel.output()
        bloom.build(dim_key, rows=rows, count=kept)
        fact_sel.launch_in(bloom, fact_key)
        fact_sel.refine(fact_other, 0, OTHER_HI)
        rows, kept = fact_sel.output()
        taker.launch(fact_val, rows, count=kept)

    def read():
        torch.cuda.synchronize()
        d_rows, d_kept = dim_sel.output()
        rows, kept = fact_sel.output()
        d, k = int(d_kept.item()), int(kept.item())
        values = taker.outs[0]
        tails = [gt.u32(d_rows[d:]), gt.u32(rows[k:]), gt.u32(values[k:NF])]
        return {"count": np.array([d, k]), "dimension rows": gt.u32(d_rows[:d]).copy(), "filter": bloom.filter.cpu().numpy().view(W).copy(),
                "rows": gt.u32(rows[:k]).copy(), "values": gt.u32(values[:k]).copy(),
                "tails untouched": np.array([t.size == 0 or (bool((t == t[0]).all()) and int(t[0]) in gt.FILLS) for t in tails])}

    workspaces = [dim_sel.ws, bloom.ws, fact_sel.ws, taker.ws]
    outputs = [dim_sel.rows[0], dim_sel.rows[1], dim_sel.counts, bloom.filter, fact_sel.rows[0], fact_sel.rows[1], fact_sel.counts,
               taker.outs[0]]
    return gt.Buffers([dim_key, dim_attr, iota, fact_key, fact_other, fact_val, count32], outputs, workspaces, workspaces, run, read)


def one_input(rng, name, count, attr_hi=1 << 31, share=0.5):
    dim_key = rng.permutation(1 << 20)[:ND].astype(U) * U(4099)  # distinct keys
    dim_attr = rng.integers(0, attr_hi, ND, dtype=np.uint64).astype(U)
    if attr_hi > LO:
        dim_attr[0] = LO + 1  # row 0 passes: a count of one keeps one row
    strangers = rng.integers(0, 1 << 32, NF, dtype=np.uint64).astype(U)
    fact_key = np.where(rng.random(NF) < share, dim_key[rng.integers(0, ND, NF)], strangers)
    fact_other = rng.integers(0, 1 << 32, NF, dtype=np.uint64).astype(U)
    fact_val = rng.integers(0, 1 << 32, NF, dtype=np.uint64).astype(U)
    words = np.array([count & 0xFFFFFFFF, count >> 32], U)
    return gt.Input([dim_key, dim_attr, np.arange(ND, dtype=U), fact_key, fact_other, fact_val, words], status=0, name=name, count=count)


def inputs():
    rng = np.random.default_rng(78)
    return [one_input(rng, "half the dimension", ND // 2), one_input(rng, "all of it", ND),
            one_input(rng, "a count beyond the column", (1 << 40) + 9, share=0.9), one_input(rng, "no row counts: an empty filter", 0),
            one_input(rng, "one row", 1), one_input(rng, "nothing passes the dimension's filter", ND, attr_hi=LO),
            one_input(rng, "a segment and a bit", 4096 + 31, share=0.1)]


def expected(inp):
    dim_key, dim_attr, _, fact_key, fact_other, fact_val, _ = inp.cols
    m = min(inp.facts["count"], ND)
    dims = np.flatnonzero((dim_attr[:m] >= LO) & (dim_attr[:m] <= HI)).astype(U)
    filt, _ = blm.build(dim_key, WORDS, SEED, rows=dims)
    keep = blm.may_hold(filt, fact_key, SEED) & (fact_other <= OTHER_HI)
    return dims, filt, np.flatnonzero(keep).astype(U), fact_val[keep]


def check(inp, got):
    dims, filt, rows, values = expected(inp)
    assert got["tails untouched"].all()
    assert got["count"][0] == dims.size and np.array_equal(got["dimension rows"], dims)
    assert np.array_equal(got["filter"], filt)
    assert got["count"][1] == rows.size and np.array_equal(got["rows"], rows)
    assert np.array_equal(got["values"], values)


def test_chain_replays_follow_the_data_and_the_device_counts():
    ins = inputs()
    sizes = [(expected(inp)[0].size, expected(inp)[2].size) for inp in ins]
    assert sizes[3] == (0, 0) and sizes[5] == (0, 0) and sizes[4][0] == 1 and len(set(sizes)) >= 6  # the replays differ
    assert sizes[1][0] > sizes[0][0] > 0 and sizes[0][1] > 0
    inp = ins[0]  # false positives are part of the answer: more fact rows pass the filter than have a partner
    dims, filt = expected(inp)[:2]
    assert int(blm.may_hold(filt, inp.cols[3], SEED).sum()) > int(np.isin(inp.cols[3], inp.cols[0][dims]).sum())
    seen = gt.run_family(make, ins, check)
    assert all(st == (0, 0, 0, 0) for st in seen)
