"""The reduce by key under graph capture (tests/graph_testlib.run_family): one captured ReduceByKey.launch per vals_signed,
replayed on inputs whose runs lie elsewhere — uniform runs, one single run, all distinct rows, a run across a chunk cut, a
run count above the capacity — and the first input again.  Before every replay the workspace is poisoned and the outputs
hold a guard word; every replay is compared with numpy and, bitwise, with an eager run of the same plan shape.  The
validator is captured behind a captured call: accept, reject a poked table, accept.

COVERAGE is for the entry points of include/dbhip_reduce_by_key.h what the table in tests/graph_testlib.py is for those of
include/dbhip.h; tests/test_capi_headers.py holds it to the header."""
import numpy as np
import pytest
import torch

from tests import graph_testlib as gl
from tests import reduce_by_key_model as rm
from tests.graph_testlib import Buffers, Input, run_family, u32
from tests.test_gpu_reduce_by_key import run_keys, uniform

pytestmark = pytest.mark.gpu
TABLE_FULL = 4
NAMES = ("keys", "counts", "sums", "mins", "maxs")

COVERAGE = {
    "dbhip_reduce_by_key_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_check_reduce_by_key_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_reduce_by_key_u32": "test_replays_change_where_the_runs_lie",
    "dbhip_check_reduce_by_key_u32": "test_validator_behind_a_captured_call",
}


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _inputs(n, capacity, chunk):
    vals = uniform(n, n + 1)
    cut = chunk if n > chunk + 2 else n // 2
    across = np.arange(n, dtype=np.uint32) // np.uint32(max(n // (capacity // 2), 1))  # capacity / 2 long runs ...
    across[cut - 3: cut + 3] = 0xFFFFFFF0  # ... and one across the chunk cut (or the column's middle)
    cols = [("uniform runs", run_keys(n, 40, n), 0), ("one single run", np.full(n, 3, dtype=np.uint32), 0),
            ("all distinct", np.arange(n, dtype=np.uint32) * np.uint32(2654435761), TABLE_FULL if n > capacity else 0),
            ("a run across a chunk cut", across, 0),
            ("more runs than the capacity", run_keys(n, 1.5, n + 2), TABLE_FULL)]
    return [Input([keys, vals if i % 2 == 0 else uniform(n, n + 3 + i)], status=st, name=name)
            for i, (name, keys, st) in enumerate(cols)]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_replays_change_where_the_runs_lie(n, signed):
    ops = _ops()
    capacity = n // 20  # above the runs of mean 40 (n / 40), below those of mean 1.5

    def make():
        plan = ops.ReduceByKey(n, capacity)
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        vals = torch.empty(n, dtype=torch.int32, device="cuda")
        outs = [plan.keys, plan.counts, plan.sums, plan.mins, plan.maxs]

        def read():
            r = min(int(plan.runs.item()), capacity)
            host = {name: (t.cpu().numpy().view(np.uint64) if name == "sums" else u32(t)) for name, t in zip(NAMES, outs)}
            got = {name: h[:r] for name, h in host.items()}
            got["runs"] = np.array([int(plan.runs.item())])
            # the entries behind the last run that was written: one value, the guard word of this replay
            got["untouched"] = np.array([np.unique(h[r:]).size <= 1 for h in host.values()])
            return got
        return Buffers([keys, vals], outs + [plan.runs], [plan.ws], [plan.ws], lambda: plan.launch(keys, vals, signed), read)

    def check(inp, got):
        want = rm.reduce_by_key(inp.cols[0], inp.cols[1], signed)
        R = want[0].size
        assert int(got["runs"][0]) == R and (R > capacity) == (inp.status == TABLE_FULL), (R, capacity)
        r = min(R, capacity)
        for name, w in zip(NAMES, want):
            assert np.array_equal(got[name], w[:r]), name
        assert got["untouched"].all(), f"entries behind run {r} were written"
    run_family(make, _inputs(n, capacity, ops.REDUCE_BY_KEY_CHUNK_ROWS), check)


@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_validator_behind_a_captured_call(n):
    ops = _ops()
    from dwarf_bench_amd import _capi
    lib = _capi.lib()
    capacity = n // 20
    plan = ops.ReduceByKey(n, capacity)
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    vals = torch.empty(n, dtype=torch.int32, device="cuda")
    poked = torch.zeros(1, dtype=torch.int32, device="cuda")  # XORed into one count between the two captured calls
    res = torch.empty(4, dtype=torch.int64, device="cuda")
    base_keys, base_vals = run_keys(n, 40, 1), uniform(n, 11)
    R = rm.reduce_by_key(base_keys, base_vals, True)[0].size  # a host value of the captured validator call
    assert R <= capacity
    cws = ops._ws(lib.dbhip_check_reduce_by_key_workspace_bytes(n, R), "cuda")
    at = R // 2

    def run():
        plan.launch(keys, vals, True)
        plan.counts[at] ^= poked[0]
        _capi.check(lib.dbhip_check_reduce_by_key_u32(keys.data_ptr(), vals.data_ptr(), n, 1, plan.keys.data_ptr(),
                                                      plan.counts.data_ptr(), plan.sums.data_ptr(), plan.mins.data_ptr(),
                                                      plan.maxs.data_ptr(), R, res.data_ptr(), cws.data_ptr(), cws.numel(),
                                                      torch.cuda.current_stream().cuda_stream), "check_reduce_by_key_u32")
    gl.fill(keys, base_keys)
    gl.fill(vals, base_vals)
    g = gl.capture(run)
    for seed, poke in ((1, 0), (2, 1), (3, 0)):
        host_vals = uniform(n, 20 + seed)  # the same runs, other values
        gl.fill(keys, base_keys)
        gl.fill(vals, host_vals)
        poked.fill_(poke)
        res.fill_(-1)
        gl.poison(plan.ws, gl.POISONS[seed % 3])
        gl.poison(cws, gl.POISONS[(seed + 1) % 3])
        g.replay()
        torch.cuda.synchronize()
        words = tuple(int(x) & ((1 << 64) - 1) for x in res.cpu().tolist())
        assert gl.status(plan.ws) == 0
        table = [u32(plan.keys[:R]), u32(plan.counts[:R]), plan.sums[:R].cpu().numpy().view(np.uint64), u32(plan.mins[:R]),
                 u32(plan.maxs[:R])]
        assert words == rm.check_words(base_keys, host_vals, *table, True)
        assert rm.verdict(words) == (poke == 0), (seed, words)
