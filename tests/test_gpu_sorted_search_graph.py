"""The sorted search under graph capture (tests/graph_testlib.run_family): index build + search + dbhip_join_pairs_u32
captured once, then replayed onto other columns of the same sizes whose runs lie elsewhere — all distinct, one single value,
long runs, a run over the ragged last blocks — so that the replays end other levels' blocks in other places, and the first
input again.  Before every replay the workspaces are poisoned and the outputs hold a guard word; every replay is compared
with numpy and, bitwise, with an eager run of the same plan shape.  The validator is captured behind a captured search:
accept, reject a poked answer, accept.

COVERAGE is for the entry points of include/dbhip_sorted_search.h what the table in tests/graph_testlib.py is for those of
include/dbhip.h; tests/test_capi_headers.py holds it to the header."""
import numpy as np
import pytest
import torch

from tests import graph_testlib as gl
from tests import sorted_search_model as sm
from tests.graph_testlib import Buffers, Input, run_family, u32

pytestmark = pytest.mark.gpu
U32 = np.uint32
M64 = (1 << 64) - 1
N = 5003

COVERAGE = {
    "dbhip_sorted_index_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_check_sorted_search_workspace_bytes": gl.NO_STREAM_WORK,
    "dbhip_sorted_index_build_u32": "test_replays_change_where_the_runs_lie",
    "dbhip_sorted_search_u32": "test_replays_change_where_the_runs_lie",
    "dbhip_check_sorted_search_u32": "test_validator_behind_a_captured_search",
}


def _ops():
    from dwarf_bench_amd import ops
    return ops


def _columns(m, signed):
    """ascending columns of m entries with other run structures, flipped back from the x domain"""
    i = np.arange(m, dtype=np.uint64)
    tail = i.copy() * np.uint64(5)
    tail[m - m % 64 - 70:] = tail[m - m % 64 - 70]  # one run over the last whole block and the ragged one behind it
    xs = [("all distinct", i * np.uint64(0xFFFFFFFF // m)), ("one single value", np.full(m, 0x80000001, dtype=np.uint64)),
          ("runs of 1000", (i // np.uint64(1000)) * np.uint64(100000)), ("a run over the ragged end", tail),
          ("runs of 3", (i // np.uint64(3)) * np.uint64(11))]
    sign = U32(0x80000000) if signed else U32(0)
    return [(name, x.astype(U32) ^ sign) for name, x in xs]


def _inputs(m, signed):
    rng = np.random.default_rng(m)
    out = []
    for k, (name, col) in enumerate(_columns(m, signed)):
        ids = rng.permutation(m).astype(U32)
        lo = rng.choice(np.concatenate([col, col + U32(1)]), N)
        if name == "one single value":
            lo[3:] += U32(1)  # three rows match the whole column, the others nothing
        hi = lo + rng.integers(0, 4, N).astype(U32) * U32(k)
        out.append(Input([col, ids, lo, hi], name=name))
    return out


def _pairs(inp, signed):
    col, ids, lo, hi = inp.cols
    pos, cnt = sm.search(col, lo, hi, signed)
    rows = np.repeat(np.arange(N, dtype=np.int64), cnt.astype(np.int64))
    first = np.cumsum(cnt.astype(np.int64)) - cnt
    k = np.arange(rows.size, dtype=np.int64) - first[rows]
    return pos, cnt, ids[pos.astype(np.int64)[rows] + k], rows.astype(U32)


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("m,top", [(262145, 64), (4097 + 64, 64), ((1 << 20) + 1, 0)])
def test_replays_change_where_the_runs_lie(m, top, signed):
    ops = _ops()
    inputs = _inputs(m, signed)
    capacity = max(int(_pairs(inp, signed)[1].sum()) for inp in inputs)

    def make():
        search = ops.SortedSearch(m, N, top=top)
        pairs = ops.JoinPairs(N, capacity)
        col, ids = (torch.empty(m, dtype=torch.int32, device="cuda") for _ in range(2))
        lo, hi = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2))

        def run():
            search.index(col, signed)
            search.search(lo, hi)
            pairs.launch(ids, search.pos, search.cnt)

        def read():
            total = int(pairs.total.item())
            return {"pos": u32(search.pos), "cnt": u32(search.cnt), "total": np.array([total]),
                    "build_rows": u32(pairs.build_rows[:total]), "probe_rows": u32(pairs.probe_rows[:total])}
        return Buffers([col, ids, lo, hi], [search.pos, search.cnt, pairs.build_rows, pairs.probe_rows, pairs.total],
                       [search.ws, pairs.ws], [search.ws, pairs.ws], run, read)

    def check(inp, got):
        pos, cnt, build_rows, probe_rows = _pairs(inp, signed)
        assert np.array_equal(got["pos"], pos) and np.array_equal(got["cnt"], cnt)
        assert int(got["total"][0]) == int(cnt.sum())
        assert np.array_equal(got["build_rows"], build_rows) and np.array_equal(got["probe_rows"], probe_rows)
    run_family(make, inputs, check)


@pytest.mark.parametrize("m,top", [(262145, 64), ((1 << 18) + 1, 0)])
def test_validator_behind_a_captured_search(m, top):
    ops = _ops()
    from dwarf_bench_amd import _capi
    lib = _capi.lib()
    signed = True
    plan = ops.SortedSearch(m, N, top=top)
    col = torch.empty(m, dtype=torch.int32, device="cuda")
    lo, hi = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2))
    poked = torch.zeros(1, dtype=torch.int32, device="cuda")  # XORed into one count between the two captured calls
    res = torch.empty(4, dtype=torch.int64, device="cuda")
    cws = ops._ws(lib.dbhip_check_sorted_search_workspace_bytes(N), "cuda")
    at = N // 2

    def run():
        plan.index(col, signed)
        plan.search(lo, hi)
        plan.cnt[at] ^= poked[0]
        _capi.check(lib.dbhip_check_sorted_search_u32(col.data_ptr(), m, 1, lo.data_ptr(), hi.data_ptr(), N,
                                                      plan.pos.data_ptr(), plan.cnt.data_ptr(), res.data_ptr(), cws.data_ptr(),
                                                      cws.numel(), torch.cuda.current_stream().cuda_stream),
                    "check_sorted_search_u32")
    inputs = _inputs(m, signed)
    for t, host in zip((col, lo, hi), (inputs[0].cols[0],) + tuple(inputs[0].cols[2:])):
        gl.fill(t, host)
    g = gl.capture(run)
    for seed, poke in ((1, 0), (2, 1), (3, 0)):
        host_col, _, host_lo, host_hi = inputs[seed].cols
        for t, host in zip((col, lo, hi), (host_col, host_lo, host_hi)):
            gl.fill(t, host)
        poked.fill_(poke)
        res.fill_(-1)
        gl.poison(plan.ws, gl.POISONS[seed % 3])
        gl.poison(cws, gl.POISONS[(seed + 1) % 3])
        g.replay()
        torch.cuda.synchronize()
        words = tuple(int(x) & M64 for x in res.cpu().tolist())
        assert gl.status(plan.ws) == 0 and gl.status(cws) == 0
        assert words == sm.check(host_col, host_lo, host_hi, u32(plan.pos), u32(plan.cnt), signed)
        assert (words[0] == 0) == (poke == 0), (seed, words)
        if poke:
            assert words[:2] == (1, at)
