"""The Bloom filter's seeded sweep on the GPU: the sixty draws of tests/bloom_fuzz_testlib.py through the raw entry points
on guarded buffers (tests/guard_testlib.py) — every buffer at its drawn offset, inputs frozen, the case's fill word in
every output, a workspace of random bytes whose status word holds the drawn stale value — each compared in full with the
model: the whole filter, or the whole row-id buffer with the entries behind the count, the count and the status word.
tests/test_bloom_fuzz_host.py shows on the CPU which draw rejects which defect."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import bloom_native as bl
from dwarf_bench_amd import ops
from tests import bloom_fuzz_testlib as bf
from tests.guard_testlib import Watch, ptr

pytestmark = pytest.mark.gpu

U, W = np.uint32, np.uint64
PARTS = 4


def stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return ptr(t) if t is not None else None


def run(case):
    w = Watch(case["fill"])
    col, rows, size, offs = case["col"], case["rows"], case["size"], case["offs"]
    d_col = w.col(col.size, offs["col"], data=col, freeze=True)
    d_rows = w.col(size, offs["rows"], data=rows, freeze=True) if rows is not None else None
    d_count = None
    if case["count"] is not None:
        d_count = w.u64(1)
        d_count.fill_(int(case["count"]))
        w.freeze(d_count)
    d_filter = w.u64(case["n_words"])
    build = case["what"] == "build"
    d_filter.copy_(torch.from_numpy((case["before"] if build else case["filter"]).view(np.int64)))
    nbytes = bl.workspace_bytes(0 if build else size)
    ws = w.ws(nbytes)
    ws.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda"))
    ws[:4].copy_(torch.from_numpy(np.array([case["stale_status"]], U).view(np.uint8)))
    col_ptr = ptr(d_col) if col.size else None
    if build:
        rc = bl.build(col_ptr, col.size, _p(d_rows), _p(d_count), size if rows is not None else 0, case["seed"], case["flags"],
                      ptr(d_filter), case["n_words"], ptr(ws), nbytes, stream())
    else:
        w.freeze(d_filter)
        d_out, d_total = w.col(size, offs["out"]), w.u64(1)
        rc = bl.probe(ptr(d_filter), case["n_words"], case["seed"], col_ptr, col.size, _p(d_rows), _p(d_count),
                      size if rows is not None else 0, case["flags"], None if case["count_only"] else ptr(d_out), ptr(d_total),
                      ptr(ws), nbytes, stream())
    assert rc == 0, (case["draw"], rc)
    torch.cuda.synchronize()
    status = ops.workspace_status(ws)
    w.check()
    if build:
        return dict(filter=d_filter.cpu().numpy().view(W).copy(), status=status)
    return dict(out=d_out.cpu().numpy().view(U).copy(), count=int(d_total.item()), status=status)


@pytest.mark.parametrize("part", range(PARTS))
def test_sweep(part):
    torch.manual_seed(part)
    cases = bf.cases()
    assert len(cases) >= 55
    for case in cases[part::PARTS]:
        try:
            bf.check(case, run(case))
        except AssertionError as e:
            what = {k: case[k] for k in ("draw", "what", "size", "n_words", "seed", "count", "flags", "offs")}
            raise AssertionError(f"{what}, list: {case['rows'] is not None}, column of {case['col'].size}: {e}") from e
