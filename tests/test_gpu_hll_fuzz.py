"""The HyperLogLog sketch's seeded sweep on the GPU: the sixty draws of tests/hll_fuzz_testlib.py through the raw entry points
on guarded buffers (tests/guard_testlib.py) — every column and the list at its drawn offset, inputs frozen, the registers
holding what the draw says they held, the case's fill word in the histogram, a workspace of random bytes whose status word
holds the drawn stale value — each compared in full with the model: all registers, all 64 histogram words and the status
word.  tests/test_hll_fuzz_host.py shows on the CPU which draw rejects which defect."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import hll_native as hl
from dwarf_bench_amd import ops
from tests import hll_fuzz_testlib as hf
from tests.guard_testlib import Watch, ptr

pytestmark = pytest.mark.gpu

U, B = np.uint32, np.uint8
PARTS = 4


def stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return ptr(t) if t is not None else None


def registers(w, held):
    regs = w.ws(held.size)
    regs.copy_(torch.from_numpy(np.ascontiguousarray(held)))
    return regs


def run(case):
    w = Watch(case["fill"])
    p = case["p"]
    d_hist = w.u64(hl.HIST_WORDS // 2)
    nbytes = hl.workspace_bytes(p)
    ws = w.ws(nbytes)
    ws.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda"))
    ws[:4].copy_(torch.from_numpy(np.array([case["stale_status"]], U).view(np.uint8)))
    if case["what"] == "build":
        cols, rows, size, offs = case["cols"], case["rows"], case["size"], case["offs"]
        n_col = cols[0].size
        d_cols = [w.col(n_col, off, data=c, freeze=True) for c, off in zip(cols, offs["cols"])]
        d_rows = w.col(size, offs["rows"], data=rows, freeze=True) if rows is not None else None
        d_count = None
        if case["count"] is not None:
            d_count = w.u64(1)
            d_count.fill_(int(case["count"]))
            w.freeze(d_count)
        d_regs = registers(w, case["before"])
        rc = hl.build([ptr(c) if n_col else None for c in d_cols], n_col, _p(d_rows), _p(d_count), size if rows is not None else 0,
                      case["seed"], case["flags"], p, ptr(d_regs), ptr(d_hist), ptr(ws), nbytes, stream())
    else:
        d_regs = registers(w, case["dst"])
        d_src = d_regs
        if not case["same_buffer"]:
            d_src = registers(w, case["src"])
            w.freeze(d_src)
        rc = hl.merge(ptr(d_regs), ptr(d_src), p, ptr(d_hist), ptr(ws), nbytes, stream())
    assert rc == 0, (case["draw"], rc)
    torch.cuda.synchronize()
    status = ops.workspace_status(ws)
    w.check()
    return dict(registers=d_regs.cpu().numpy().copy(), hist=d_hist.cpu().numpy().view(U).copy(), status=status)


@pytest.mark.parametrize("part", range(PARTS))
def test_sweep(part):
    torch.manual_seed(part)
    cases = hf.cases()
    assert len(cases) >= 55
    for case in cases[part::PARTS]:
        try:
            hf.check(case, run(case))
        except AssertionError as e:
            what = {k: case.get(k) for k in ("draw", "what", "size", "p", "seed", "count", "flags", "offs", "held")}
            raise AssertionError(f"{what}: {e}") from e
