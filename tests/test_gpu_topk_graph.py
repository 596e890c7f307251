"""The top-k under graph capture (tests/graph_testlib.run_family): one captured TopK.launch per (signedness, largest,
sorted), replayed on inputs whose select takes other device-side paths — another number of levels before the bin is
taken whole, another threshold, ties cut by a chunk boundary — and the first input again.  Before every replay the
workspace is poisoned and the outputs hold a guard word; every replay is compared with numpy and, bitwise, with an eager
run of the same plan shape.  The validator is captured behind a captured top-k: accept, reject a poked table, accept.

COVERAGE is for the entry points of include/dbhip_topk.h what the table in tests/graph_testlib.py is for those of
include/dbhip.h; tests/test_capi_headers.py holds it to the header."""
import numpy as np
import pytest
import torch

from tests import graph_testlib as gl
from tests import topk_model as tm
from tests.graph_testlib import Buffers, Input, run_family, u32

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF

COVERAGE = {
    "dbhip_topk_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_topk_u32": "test_topk_replays_change_the_select_path",
    "dbhip_topk_i32": "test_topk_replays_change_the_select_path",
    "dbhip_check_topk_u32": "test_validator_behind_a_captured_topk",
}


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _inputs(n, k, chunk):
    rng = np.random.default_rng(n + k)
    uniform = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    equal = np.full(n, 0x80000000, dtype=np.uint32)
    # the first level settles it: the best top byte of each of the four orders (0x00, 0xFF, 0x80, 0x7F) is carried by
    # exactly k rows, every other row by a top byte in [0x20, 0x5F]; the bin of the k-th key is taken whole
    first = ((np.uint32(0x20) + (uniform >> np.uint32(26))) << np.uint32(24)) | (uniform & np.uint32(0x00FFFFFF))
    rows = rng.permutation(n)[:4 * k]
    for j, top in enumerate((0x00, 0xFF, 0x80, 0x7F)):
        mine = rows[j * k:(j + 1) * k]
        first[mine] = np.uint32(top << 24) | (uniform[mine] & np.uint32(0x00FFFFFF))
    # only the last level settles it: every key shares the upper three bytes
    last = np.uint32(0x5A5A5A00) | (uniform & np.uint32(0xFF))
    # ties of the threshold key on both sides of a chunk boundary (or of the column's middle, where it is shorter),
    # everything else worse or better in equal parts
    cut = chunk if n > chunk + 2 else n // 2
    ties = np.where(uniform & np.uint32(1), np.uint32(0x10), np.uint32(0xF0000000)) | (uniform & np.uint32(0xF00))
    ties[cut - 2: cut + 3] = 0x80000000
    cols = [("uniform", uniform), ("all keys equal", equal), ("settled at the first level", first),
            ("settled at the last level", last), ("ties across a chunk cut", ties)]
    return [Input([c], name=name) for name, c in cols]


@pytest.mark.parametrize("srt", [True, False])
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n,k", [(5000, 1), (5000, 1000), ((1 << 20) + 5, 1), ((1 << 20) + 5, 1000)])
def test_topk_replays_change_the_select_path(n, k, signed, largest, srt):
    ops = _ops()

    def make():
        plan = ops.TopK(n, k)
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        return Buffers([keys], [plan.out_keys, plan.out_rows], [plan.ws], [plan.ws],
                       lambda: plan.launch(keys, largest=largest, signed=signed, sorted=srt),
                       lambda: {"keys": u32(plan.out_keys[:plan.m]), "rows": u32(plan.out_rows[:plan.m])})

    def check(inp, got):
        want_keys, want_rows = tm.topk(inp.cols[0], k, largest, signed, sorted=srt)
        assert np.array_equal(got["rows"], want_rows) and np.array_equal(got["keys"], want_keys)
    run_family(make, _inputs(n, k, ops.TOPK_CHUNK_ROWS), check)


@pytest.mark.parametrize("n,k", [(5000, 1000), ((1 << 20) + 5, 1000)])
def test_validator_behind_a_captured_topk(n, k):
    ops = _ops()
    from dwarf_bench_amd import _capi
    plan = ops.TopK(n, k)
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    poked = torch.zeros(1, dtype=torch.int32, device="cuda")  # XORed into one row id between the two captured calls
    res = torch.empty(2, dtype=torch.int64, device="cuda")
    at = k // 2

    def run():
        plan.launch(keys, largest=True, signed=True)
        plan.out_rows[at] ^= poked[0]
        _capi.check(_capi.lib().dbhip_check_topk_u32(keys.data_ptr(), n, plan.out_keys.data_ptr(), plan.out_rows.data_ptr(),
                                                     k, 1, 1, res.data_ptr(), torch.cuda.current_stream().cuda_stream),
                    "check_topk_u32")
    rng = np.random.default_rng(7)
    gl.fill(keys, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    g = gl.capture(run)
    for seed, poke in ((1, 0), (2, 1), (3, 0)):
        host = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        gl.fill(keys, host)
        poked.fill_(poke)
        res.fill_(-1)
        gl.poison(plan.ws, gl.POISONS[seed % 3])
        g.replay()
        torch.cuda.synchronize()
        words = tuple(int(x) for x in res.cpu().tolist())
        assert gl.status(plan.ws) == 0
        assert words == tm.check_words(host, u32(plan.out_keys[:k]), u32(plan.out_rows[:k]), True, True)
        assert tm.verdict(words, k, n) == (poke == 0), (seed, words)
