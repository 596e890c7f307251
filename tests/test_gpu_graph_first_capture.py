"""The first call of a family in a process, captured.  partition.hip, join_lds.hip, groupby.hip and groupby_hash.hip set
function attributes and ask for occupancies on first use (partition.hpp jl_resident_per_cu caches the answer per host
thread); the warm-up run in front of every other capture of this suite hides whether those calls are legal inside a capture and size the same grid
there.  Each test starts a fresh child process, loads the code object with one reduce, and runs one family of
tests/test_gpu_graph_paths.py with graph_testlib.FIRST_CAPTURE set: no eager call of the family before the capture, every
replay checked against the oracle, and the eager twin runs only after the last replay.  One child per family, one after
the other: a failure names the family, and never more than one process has the GPU open."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

FAMILIES = {
    "hash join, 2^18 + 5": "t.test_hash_join_replays((1 << 18) + 5, False)",
    "hash join, 2^22": "t.test_hash_join_replays(1 << 22, True)",
    "radix join, 2^18": "t.test_radix_join_replays(1 << 18, 'steps', False)",
    "unique join, 2^16": "t.test_unique_join_replays(1 << 16)",
    "dense group-by, 65536 groups": "t.test_dense_groupby_replays(None, 65536)",
    "hash group-by, lds": "t.test_hash_groupby_replays('lds', True)",
    "hash group-by, part": "t.test_hash_groupby_replays('part', True)",
    "slab table": "t.test_slab_table_life_in_one_graph()",
    "cuckoo table": "t.test_cuckoo_table_life_in_one_graph(2, 0)",
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_first_capture_of_a_process(family):
    """A child that hangs, aborts or faults ends the whole session (pytest.exit, return code 3), as in
    test_groupby_packed_and_wide_tables_pinned: after a fault or a hang on the GPU nothing more is started on it."""
    prog = ("import torch\n"
            "from dwarf_bench_amd import ops\n"
            "ops.reduce_sum(ops.gen_uniform_u32(1024, 1, 0, 9)); torch.cuda.synchronize()  # loads the code object\n"
            "from tests import graph_testlib as gl\n"
            "from tests import test_gpu_graph_paths as t\n"
            "gl.FIRST_CAPTURE = True\n"
            f"{FAMILIES[family]}\n"
            f"print('ok', {family!r})\n")
    try:
        r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=600,
                           cwd=os.path.dirname(os.path.dirname(__file__)))
    except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child ({family}) hung: {e}", returncode=3)
    if r.returncode in (-6, -11, 134, 139):  # an abort or a fault on the GPU: nothing more is started on it
        pytest.exit(f"the first-capture child ({family}) died with {r.returncode}: {r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0 and f"ok {family}" in r.stdout, (family, r.stdout[-2000:], r.stderr[-3000:])
