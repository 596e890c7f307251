"""Test-only helpers for the hipGraph tests: one capture helper, one replay loop, and the table that says which test
captures which entry point of include/dbhip.h.  Never imported by the product.

A graph freezes every host-side decision and every kernel argument of the captured calls; only what the kernels decide
from the data may change between replays.  replay_sequence() therefore runs one captured sequence over inputs that take
different device-side paths, and before every replay it takes away everything a stale result could hide behind: the
output buffers get a guard word, the workspace one of three poisons."""
import numpy as np
import torch

from tests.guard_testlib import FILLS, i32, i64

POISONS = ("zeros", "0xff", "random")  # tests/test_gpu_workspace_reuse.py


def fill(t, host):
    """a host column of 4-byte words -> the int32 device tensor t (same bits)"""
    t.copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.int32)))


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def poison(ws, how):
    """None leaves the workspace as it is"""
    if how is None:
        return
    if how == "zeros":
        ws.zero_()
    elif how == "0xff":
        ws.fill_(0xFF)
    else:
        g = torch.Generator(device=ws.device)
        g.manual_seed(1234)
        ws.copy_(torch.randint(0, 256, ws.shape, dtype=torch.uint8, device=ws.device, generator=g))


def capture(fn, warm=True):
    """fn() captured on torch's capture stream as one linear sequence (no second stream, no branch inside the
    capture).  warm: one eager run first on a side stream (lazy module loads, attribute calls); warm=False captures
    fn() as the first call of its kind, which is what the fresh-process tests are for."""
    if warm:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def status(ws):
    from dwarf_bench_amd import ops
    return ops.workspace_status(ws)


class Input:
    """one replay: the host columns (in the order of Buffers.inputs), the status word it must leave, and whatever the
    family's check wants to know about it"""

    def __init__(self, cols, status=0, name="", **facts):
        self.cols, self.status, self.name, self.facts = cols, status, name, facts


class Buffers:
    """the device buffers of one instance of a call sequence.
      inputs      int32 tensors the captured calls read (refilled before every replay)
      outputs     tensors (int32 or int64) the captured calls write (guard-filled before every replay)
      workspaces  uint8 workspaces the header says may hold anything when the sequence starts (poisoned)
      status_ws   the workspaces whose status word is read after the replay, in order
      run         the call sequence itself, on the current stream
      read        -> {name: numpy array} of the results, after a synchronisation
      twin        a second, independent instance: replay_sequence runs it eagerly on the same input"""

    def __init__(self, inputs, outputs, workspaces, status_ws, run, read, twin=None):
        self.inputs, self.outputs, self.workspaces = list(inputs), list(outputs), list(workspaces)
        self.status_ws, self.run, self.read, self.twin = list(status_ws), run, read, twin

    def prepare(self, inp, word, how):
        for t in self.outputs:
            t.fill_(i64(word) if t.dtype == torch.int64 else i32(word))
        for ws in self.workspaces:
            poison(ws, how)
        assert len(inp.cols) == len(self.inputs)
        for t, host in zip(self.inputs, inp.cols):
            fill(t, host)


def same(got, want, what, canon=None):
    """every named result of the replay against the eager run's: bitwise, after `canon` where the header leaves an
    order open"""
    if canon is not None:
        got, want = canon(got), canon(want)
    assert got.keys() == want.keys()
    for k in got:
        assert np.array_equal(got[k], want[k]), f"{what}: '{k}' of the replay differs from the eager run's"


def replay_sequence(graph, plan_buffers, inputs, check, canon=None, eager_after=False):
    """Replays `graph` (captured over plan_buffers.run) once per input.  Before each replay: the guard word into every
    output, a poison into every workspace (or nothing: see below), the input into the input buffers.  After it: the status word(s) against the
    input's, check(input, results) against the oracle, and the results against an eager run of the same calls in the
    twin buffers (bitwise; through `canon` where the header leaves an order open).  eager_after: the eager runs come
    after the last replay, so that no eager call of the family precedes any replay.  -> the status words seen."""
    seen, kept = [], []
    twin = plan_buffers.twin

    def eager(i, inp, got, want, what):
        twin.prepare(inp, FILLS[(i + 1) % len(FILLS)], POISONS[(i + 1) % len(POISONS)])
        twin.run()
        torch.cuda.synchronize()
        assert tuple(status(ws) for ws in twin.status_ws) == tuple(want), f"{what}: the eager run's status"
        same(got, twin.read(), what, canon)

    for i, inp in enumerate(inputs):
        what = f"replay {i} ({inp.name})"
        # every other replay, and every replay after a flagged one, inherits the workspace as the replay before left it
        # (stale but plausible state: a spill directory, a pool cursor, a status word); the others get a poison
        keep = i > 0 and (i % 2 == 1 or inputs[i - 1].status not in (0, (0,) * len(plan_buffers.status_ws)))
        plan_buffers.prepare(inp, FILLS[i % len(FILLS)], None if keep else POISONS[(i // 2) % len(POISONS)])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = inp.status if isinstance(inp.status, (tuple, list)) else (inp.status,) * len(plan_buffers.status_ws)
        st = tuple(status(ws) for ws in plan_buffers.status_ws)
        seen.append(st)
        assert st == tuple(want), f"{what}: status {st}, expected {tuple(want)}; so far {seen}"
        got = plan_buffers.read()
        try:
            check(inp, got)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from e
        if twin is not None and eager_after:
            kept.append((i, inp, got, want, what))
        elif twin is not None:
            eager(i, inp, got, want, what)
    for args in kept:
        eager(*args)
    return seen


# set by the child processes of tests/test_gpu_graph_first_capture.py: the capture is then the first call of its
# family in the process (no warm-up), and the eager twin runs only after the last replay
FIRST_CAPTURE = False


def run_family(make, inputs, check, canon=None):
    """make() -> Buffers, twice (the captured instance and its eager twin); capture on inputs[0], replay inputs[1:] and
    inputs[0] again: a flagged or spilling replay is always followed by a clean one"""
    bufs = make()
    bufs.twin = make()
    bufs.prepare(inputs[0], FILLS[0], "zeros")
    graph = capture(bufs.run, warm=not FIRST_CAPTURE)
    return replay_sequence(graph, bufs, list(inputs) + [inputs[0]], check, canon, eager_after=FIRST_CAPTURE)


# ---- which test captures which entry point ----------------------------------------------------------------------------
PATHS = "tests/test_gpu_graph_paths.py"
NO_STREAM_WORK = "does no stream work"


def _paths(test):
    return (PATHS, test)


COVERAGE = {
    # entry point: (test file, test function) that captures it, or a one-line reason why it cannot be captured
    "dbhip_version": NO_STREAM_WORK,
    "dbhip_device_info": NO_STREAM_WORK,
    "dbhip_radix_sort_rank_mode": NO_STREAM_WORK,
    "dbhip_workspace_status": "synchronises the stream by contract",
    "dbhip_radix_sort_prepare": "refused during capture (DBHIP_EINVAL): test_sort_prepare_is_refused_inside_a_capture",
    **{name: NO_STREAM_WORK for name in (
        "dbhip_copy_if_lt_i32_workspace_bytes", "dbhip_radix_sort_workspace_bytes",
        "dbhip_radix_sort_pairs_workspace_bytes", "dbhip_groupby_sum_u32_workspace_bytes",
        "dbhip_groupby_hash_workspace_bytes", "dbhip_join_workspace_bytes", "dbhip_join_radix_workspace_bytes",
        "dbhip_join_pairs_workspace_bytes", "dbhip_ujoin_workspace_bytes", "dbhip_bitmask_table_workspace_bytes",
        "dbhip_cuckoo_table_workspace_bytes", "dbhip_slab_table_workspace_bytes",
        "dbhip_pjoin_partition_workspace_bytes", "dbhip_exclusive_scan_u32_workspace_bytes",
        "dbhip_check_fingerprint_workspace_bytes", "dbhip_check_permutation_workspace_bytes",
        "dbhip_check_distinct_workspace_bytes")},
    "dbhip_gen_uniform_u32": _paths("test_generators_in_front_of_a_dwarf"),
    "dbhip_gen_uniform_at_u32": _paths("test_generators_in_front_of_a_dwarf"),
    "dbhip_gen_unique_sorted_u32": _paths("test_generators_in_front_of_a_dwarf"),
    "dbhip_copy_if_lt_i32": _paths("test_scan_replays_change_the_selectivity"),
    "dbhip_copy_if_lt_dense_i32": _paths("test_scan_replays_change_the_selectivity"),
    "dbhip_exclusive_scan_u32": _paths("test_exclusive_scan_three_launch_path"),
    "dbhip_radix_sort_u32": _paths("test_sort_replays_change_the_executed_passes"),
    "dbhip_radix_sort_i32": _paths("test_sort_replays_change_the_executed_passes"),
    "dbhip_radix_sort_pairs_u32": _paths("test_sort_replays_change_the_executed_passes"),
    "dbhip_radix_sort_pairs_i32": _paths("test_sort_replays_change_the_executed_passes"),
    "dbhip_groupby_sum_u32": _paths("test_dense_groupby_replays"),
    "dbhip_groupby_partial_u32": _paths("test_dense_groupby_replays"),
    "dbhip_groupby_merge_u32": _paths("test_dense_groupby_replays"),
    "dbhip_groupby_hash_u32": _paths("test_hash_groupby_replays"),
    "dbhip_join_build_u32": _paths("test_hash_join_replays"),
    "dbhip_join_build_pairs_u32": _paths("test_hash_join_replays"),
    "dbhip_join_probe_u32": _paths("test_hash_join_replays"),
    "dbhip_join_answers_u32": _paths("test_hash_join_replays"),
    "dbhip_join_radix_partition_u32": _paths("test_radix_join_replays"),
    "dbhip_join_radix_match_u32": _paths("test_radix_join_replays"),
    "dbhip_join_radix_u32": _paths("test_radix_join_replays"),
    "dbhip_join_pairs_u32": _paths("test_join_pairs_behind_a_captured_join"),
    "dbhip_ujoin_build_u32": _paths("test_unique_join_replays"),
    "dbhip_ujoin_probe_u32": _paths("test_unique_join_replays"),
    "dbhip_bitmask_table_reset": _paths("test_bitmask_table_life_in_one_graph"),
    "dbhip_bitmask_table_insert_u32": _paths("test_bitmask_table_life_in_one_graph"),
    "dbhip_bitmask_table_lookup_u32": _paths("test_bitmask_table_life_in_one_graph"),
    "dbhip_cuckoo_table_reset": _paths("test_cuckoo_table_life_in_one_graph"),
    "dbhip_cuckoo_table_insert_u32": _paths("test_cuckoo_table_life_in_one_graph"),
    "dbhip_cuckoo_table_lookup_u32": _paths("test_cuckoo_table_life_in_one_graph"),
    "dbhip_cuckoo_table_export_u32": _paths("test_cuckoo_table_life_in_one_graph"),
    "dbhip_slab_table_reset": _paths("test_slab_table_life_in_one_graph"),
    "dbhip_slab_table_insert_u32": _paths("test_slab_table_life_in_one_graph"),
    "dbhip_slab_table_lookup_u32": _paths("test_slab_table_life_in_one_graph"),
    "dbhip_slab_table_join_probe_u32": _paths("test_slab_table_life_in_one_graph"),
    "dbhip_slab_table_export_u32": _paths("test_slab_table_life_in_one_graph"),
    "dbhip_pjoin_partition_u32": _paths("test_small_calls_replay"),
    "dbhip_gather_u32": _paths("test_small_calls_replay"),
    "dbhip_reduce_sum_i32": _paths("test_small_calls_replay"),
    "dbhip_nested_join_u32": _paths("test_small_calls_replay"),
    "dbhip_check_pjoin_route_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_fingerprint_lt_i32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_sorted_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_weighted_sum_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_permutation_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_join_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_ujoin_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_distinct_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_sorted_pairs_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_join_pairs_u32": _paths("test_validators_accept_reject_accept"),
    "dbhip_check_gen_uniform_u32": _paths("test_validators_accept_reject_accept"),
}
