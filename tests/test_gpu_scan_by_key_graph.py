"""The scan by key under graph capture (tests/graph_testlib.run_family): one captured ScanByKey.launch per vals_signed,
replayed on inputs that take the other paths of the kernels — uniform runs, one single run (every step head-free), all
distinct rows (every step all heads), a run across a chunk cut, long runs — and the first input again; both sizes end in a
ragged segment.  Before every replay the workspace is poisoned and the outputs hold a guard word; every replay is compared
with numpy and, bitwise, with an eager run of the same plan shape.  The validator is captured behind a captured call:
accept, reject a poked table, accept.

COVERAGE is for the entry points of include/dbhip_scan_by_key.h what the table in tests/graph_testlib.py is for those of
include/dbhip.h; tests/test_capi_headers.py holds it to the header."""
import numpy as np
import pytest
import torch

from tests import graph_testlib as gl
from tests import scan_by_key_model as sm
from tests.graph_testlib import Buffers, Input, run_family, u32
from tests.test_gpu_scan_by_key import run_keys, uniform

pytestmark = pytest.mark.gpu
NAMES = sm.NAMES
M64 = (1 << 64) - 1

COVERAGE = {
    "dbhip_scan_by_key_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_check_scan_by_key_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_scan_by_key_u32": "test_replays_change_where_the_runs_lie",
    "dbhip_check_scan_by_key_u32": "test_validator_behind_a_captured_call",
}


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _inputs(n, chunk):
    vals = uniform(n, n + 1)
    cut = chunk if n > chunk + 2 else n // 2
    across = np.arange(n, dtype=np.uint32) // np.uint32(max(n // 50, 1))  # fifty long runs ...
    across[cut - 3: cut + 3] = 0xFFFFFFF0  # ... and one across the chunk cut (or the column's middle)
    cols = [("uniform runs", run_keys(n, 40, n)), ("one single run", np.full(n, 3, dtype=np.uint32)),
            ("all distinct", np.arange(n, dtype=np.uint32) * np.uint32(2654435761)),
            ("a run across a chunk cut", across), ("short runs", run_keys(n, 1.5, n + 2))]
    return [Input([keys, vals if i % 2 == 0 else uniform(n, n + 3 + i)], name=name) for i, (name, keys) in enumerate(cols)]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_replays_change_where_the_runs_lie(n, signed):
    ops = _ops()

    def make():
        plan = ops.ScanByKey(n)
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        vals = torch.empty(n, dtype=torch.int32, device="cuda")
        outs = [getattr(plan, name) for name in NAMES]

        def read():
            return {name: (t.cpu().numpy().view(np.uint64) if name == "sums" else u32(t)) for name, t in zip(NAMES, outs)}
        return Buffers([keys, vals], outs, [plan.ws], [plan.ws], lambda: plan.launch(keys, vals, signed), read)

    def check(inp, got):
        for name, w in zip(NAMES, sm.scan_by_key(inp.cols[0], inp.cols[1], signed)):
            assert np.array_equal(got[name], w), name
    run_family(make, _inputs(n, ops.SCAN_BY_KEY_CHUNK_ROWS), check)


@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_validator_behind_a_captured_call(n):
    ops = _ops()
    from dwarf_bench_amd import _capi
    lib = _capi.lib()
    plan = ops.ScanByKey(n)
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    poked = torch.zeros(1, dtype=torch.int64, device="cuda")  # XORed into one sum between the two captured calls
    res = torch.empty(4, dtype=torch.int64, device="cuda")
    cws = ops._ws(lib.dbhip_check_scan_by_key_workspace_bytes(n), "cuda")
    at = n // 2

    def run():
        plan.launch(keys, vals, True)
        plan.sums[at] ^= poked[0]
        _capi.check(lib.dbhip_check_scan_by_key_u32(keys.data_ptr(), vals.data_ptr(), n, 1, plan.run_ids.data_ptr(),
                                                    plan.row_numbers.data_ptr(), plan.sums.data_ptr(), plan.mins.data_ptr(),
                                                    plan.maxs.data_ptr(), res.data_ptr(), cws.data_ptr(), cws.numel(),
                                                    torch.cuda.current_stream().cuda_stream), "check_scan_by_key_u32")
    shapes = [run_keys(n, 40, 1), np.full(n, 8, dtype=np.uint32), np.arange(n, dtype=np.uint32) + np.uint32(3)]
    gl.fill(keys, shapes[0])
    gl.fill(vals, uniform(n, 11))
    g = gl.capture(run)
    for seed, poke in ((1, 0), (2, 1), (3, 0)):
        host_keys, host_vals = shapes[seed % 3], uniform(n, 20 + seed)  # other runs, other values
        gl.fill(keys, host_keys)
        gl.fill(vals, host_vals)
        poked.fill_(poke)
        res.fill_(-1)
        gl.poison(plan.ws, gl.POISONS[seed % 3])
        gl.poison(cws, gl.POISONS[(seed + 1) % 3])
        g.replay()
        torch.cuda.synchronize()
        words = tuple(int(x) & M64 for x in res.cpu().tolist())
        assert gl.status(plan.ws) == 0 and gl.status(cws) == 0
        table = [u32(plan.run_ids), u32(plan.row_numbers), plan.sums.cpu().numpy().view(np.uint64), u32(plan.mins),
                 u32(plan.maxs)]
        assert words == sm.check_words(host_keys, host_vals, *table, signed=True)
        assert sm.verdict(words, host_keys) == (poke == 0), (seed, words)
        if poke:
            assert words[1] == at
