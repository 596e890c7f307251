"""dbhip_groupby_hash_u32 on the GPU against numpy (np.unique + np.add.at + bincount), every path, the bound, the
0xFFFFFFFF key, reused and poisoned workspaces, graph replay, the device validator and the CLI dwarf."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from dwarf_bench_amd import _capi, ops  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
LDS_MAX = 4096  # the LDS path's bound (groupby_hash.hip kGbhLdsMaxGroups)
M32 = 0xFFFFFFFF


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _expect(keys: np.ndarray, vals: np.ndarray):
    u, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(u), dtype=np.uint32)
    np.add.at(sums, inv, vals.astype(np.uint32))
    return u.astype(np.uint32), sums, np.bincount(inv, minlength=len(u)).astype(np.uint32)


def _sorted(k, s, c):
    k = k.cpu().numpy().view(np.uint32)
    o = np.argsort(k, kind="stable")
    return k[o], s.cpu().numpy().view(np.uint32)[o], (None if c is None else c.cpu().numpy().view(np.uint32)[o])


def _agree(keys, vals, max_groups=None, counts=True):
    got = _sorted(*ops.groupby_hash(_dev(keys), _dev(vals), max_groups, counts=counts))
    want = _expect(keys, vals)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if counts:
        assert np.array_equal(got[2], want[2])
    else:
        assert got[2] is None


def _keys(rng, n, distinct):
    pool = rng.choice(1 << 32, size=distinct, replace=False).astype(np.uint32) if distinct < (1 << 24) else \
        np.unique(rng.integers(0, 1 << 32, size=distinct, dtype=np.uint64).astype(np.uint32))
    return pool[rng.integers(0, len(pool), size=n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 10**6 + 3, 1 << 24])
def test_sizes(n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    _agree(keys, vals)
    if n:
        small = _keys(rng, n, min(n, 100))
        _agree(small, vals, max_groups=100)


@pytest.mark.parametrize("distinct", [1, 2, 100, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, 10**5, "all"])
def test_distinct_key_counts(distinct):
    n = 1 << 20
    rng = np.random.default_rng(7)
    if distinct == "all":
        keys = rng.permutation(np.arange(n, dtype=np.uint64) * 4093 + 17).astype(np.uint32)
        d = n
    else:
        keys, d = _keys(rng, n, distinct), distinct
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    _agree(keys, vals, max_groups=d)  # the caller's exact bound: LDS path up to 4096, partitions above
    _agree(keys, vals)  # no bound: max_groups = n


def test_extreme_keys():
    rng = np.random.default_rng(3)
    n = 300000
    keys = _keys(rng, n, 1000)
    keys[::7] = 0
    keys[1::11] = 0xFFFFFFFE
    keys[2::13] = M32
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    _agree(keys, vals, max_groups=1003)
    _agree(keys, vals)
    only = np.full(1000, M32, dtype=np.uint32)
    _agree(only, np.arange(1000, dtype=np.uint32), max_groups=1)


@pytest.mark.parametrize("key", [12345, M32])
def test_one_key_on_every_row_wraps(key):
    n = 1 << 22
    keys = np.full(n, key, dtype=np.uint32)
    vals = (np.uint32(M32) - np.arange(n, dtype=np.uint32) % 1000).astype(np.uint32)
    _agree(keys, vals, max_groups=1)
    _agree(keys, vals)


def test_hot_key_half_the_rows():
    n = 1 << 24
    rng = np.random.default_rng(11)
    keys = rng.permutation(np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    keys[rng.random(n) < 0.5] = 777  # half the rows on one key, the rest distinct: giant partition slices
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    _agree(keys, vals)


def test_counts_off():
    rng = np.random.default_rng(5)
    keys = _keys(rng, 100000, 5000)
    vals = rng.integers(0, 1 << 16, size=100000).astype(np.uint32)
    _agree(keys, vals, counts=False)
    _agree(_keys(rng, 100000, 50), vals, 50, counts=False)


def test_dense_keys_agree_with_groupby_sum():
    n, groups = 1 << 22, 1 << 16
    keys = ops.gen_uniform_u32(n, 42, 0, groups - 1)
    vals = ops.gen_uniform_u32(n, 43, 1, 10000)
    dense = ops.groupby_sum(keys, vals, groups).cpu().numpy().view(np.uint32)
    k, s, c = ops.groupby_hash(keys, vals, groups)
    scat = np.zeros(groups, dtype=np.uint32)
    scat[k.cpu().numpy().view(np.uint32)] = s.cpu().numpy().view(np.uint32)
    assert np.array_equal(scat, dense) and int(c.sum()) == n


_CHILD = r"""
import numpy as np, torch, sys
from dwarf_bench_amd import ops
rng = np.random.default_rng(9)
out = {}
for name, n, d, mg in (("few", 1 << 20, 64, 64), ("mid", 1 << 20, 20000, 20000), ("all", 1 << 20, 0, 0),
                       ("hot", 1 << 22, 0, 0), ("ff", 100000, 300, 301)):
    if d:
        pool = rng.choice(1 << 32, size=d, replace=False).astype(np.uint32)
        keys = pool[rng.integers(0, d, size=n)]
    else:
        keys = rng.permutation(np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    if name == "hot":
        keys[rng.random(n) < 0.5] = 5
    if name == "ff":
        keys[::3] = 0xFFFFFFFF
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k, s, c = ops.groupby_hash(torch.from_numpy(keys.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda(), mg)
    k = k.cpu().numpy().view(np.uint32); o = np.argsort(k)
    u, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(u), dtype=np.uint32); np.add.at(sums, inv, vals)
    ok = np.array_equal(k[o], u) and np.array_equal(s.cpu().numpy().view(np.uint32)[o], sums) and \
        np.array_equal(c.cpu().numpy().view(np.uint32)[o], np.bincount(inv).astype(np.uint32))
    out[name] = bool(ok)
print("RESULT", out)
sys.exit(0 if all(out.values()) else 1)
"""


@pytest.mark.parametrize("path", ["lds", "part", "global"])
def test_every_path_on_the_same_inputs(path):
    """DBHIP_GBH_PATH pins a path (read once: a fresh process per value)"""
    r = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DBHIP_GBH_PATH": path}, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("distinct,bound", [(101, 100), (5000, 4096), (4097, 4096), (300000, 1000), (300000, 200000)])
def test_more_keys_than_the_bound(distinct, bound):
    n = 1 << 20
    rng = np.random.default_rng(distinct)
    keys = _keys(rng, n, distinct)
    vals = np.ones(n, dtype=np.uint32)
    plan = ops.GroupByHash(n, bound)
    guard = 0x5A5A5A5A
    cap = bound
    # guard words behind each output column: plan columns re-made with room behind them
    for name in ("keys", "sums", "counts"):
        t = torch.full((cap + 64,), guard, dtype=torch.int32, device="cuda")
        setattr(plan, name, t)
    kd, vd = _dev(keys), _dev(vals)
    real = len(np.unique(keys))
    plan.launch(kd, vd)
    torch.cuda.synchronize()
    st = ops.workspace_status(plan.ws)
    if real > bound:
        assert st & ops.DEV_TABLE_FULL
        assert int(plan.groups.item()) == bound
    for name in ("keys", "sums", "counts"):
        tail = getattr(plan, name)[cap:].cpu().numpy()
        assert (tail == guard).all(), name


def test_plan_reuse_and_poisoned_workspace():
    rng = np.random.default_rng(21)
    for mg in (64, 0):
        n = 1 << 20
        plan = ops.GroupByHash(n, mg)
        for trial in range(3):
            keys = _keys(rng, n, 64 if mg else 50000)
            vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            if trial == 1:
                plan.ws.fill_(-1)  # 0xFF bytes
            if trial == 2:
                plan.ws.copy_(torch.randint(-128, 127, plan.ws.shape, dtype=torch.int8, device="cuda").view(torch.uint8))
            plan.launch(_dev(keys), _dev(vals))
            got = _sorted(*plan.result())
            want = _expect(keys, vals)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (mg, trial)


def test_graph_capture_and_replay():
    n = 1 << 20
    rng = np.random.default_rng(31)
    for mg in (64, 0):
        keys = _dev(_keys(rng, n, 64 if mg else 100000))
        vals = _dev(rng.integers(0, 1 << 16, size=n).astype(np.uint32))
        plan = ops.GroupByHash(n, mg)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            plan.launch(keys, vals)  # warm-up outside the capture (function attributes, code objects)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.launch(keys, vals)
        want = _expect(keys.cpu().numpy().view(np.uint32), vals.cpu().numpy().view(np.uint32))
        for _ in range(3):
            plan.ws.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            got = _sorted(*plan.result())
            assert all(np.array_equal(a, b) for a, b in zip(got, want))


def _validate(keys, vals, ok, os_, oc):
    n = keys.numel()
    ones = torch.ones(n, dtype=torch.int32, device="cuda")
    return (ops.check_weighted_sum(ok, os_) == ops.check_weighted_sum(keys, vals)
            and ops.check_weighted_sum(ok, oc) == ops.check_weighted_sum(keys, ones)
            and int(oc.to(torch.int64).sum()) == n and ops.check_distinct(ok) == 0)


def test_device_validator_accepts_and_rejects():
    n = 1 << 20
    keys = ops.gen_uniform_u32(n, 1, 0, M32)
    keys[::2] = keys[1::2]  # about n / 2 distinct keys
    vals = ops.gen_uniform_u32(n, 2, 0, M32)
    k, s, c = ops.groupby_hash(keys, vals)
    assert _validate(keys, vals, k, s, c)
    # a key emitted twice with its sum split: the weighted sums still agree, the distinct-key check does not
    k2 = torch.cat([k, k[:1]])
    half = (s[:1].to(torch.int64) & 0xFFFF).to(torch.int32)
    s2 = torch.cat([s[:1] - half, s[1:], half])
    c2 = torch.cat([c[:1] - 1, c[1:], torch.ones(1, dtype=torch.int32, device="cuda")])
    assert ops.check_weighted_sum(k2, s2) == ops.check_weighted_sum(keys, vals)
    assert ops.check_distinct(k2) == 1 and not _validate(keys, vals, k2, s2, c2)
    s3 = s.clone()
    s3[5] += 1  # a changed sum
    assert not _validate(keys, vals, k, s3, c)
    assert not _validate(keys, vals, k[1:], s[1:], c[1:])  # a dropped group


CLI = ROOT / "dwarf_bench_amd" / "_lib" / "dwarf_bench_groupby_hash"


@pytest.mark.parametrize("groups", [64, 10**6])
def test_cli_dwarf(groups, tmp_path):
    rep = tmp_path / "r.csv"
    sizes = ["1", "1000", "100000", str(1 << 24)]
    r = subprocess.run([str(CLI), "GroupByHashHip", "--device=hip", "--iterations", "3", f"--report_path={rep}",
                        "--groups_count", str(groups), "--input_size"] + sizes, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ncorrect results" not in r.stderr and "Caught exception" not in r.stderr, r.stderr
    assert len(rep.read_text().splitlines()) == 1 + 3 * len(sizes)  # a header and one row per run


def test_cli_dwarf_validator_catches_an_injected_fault():
    r = subprocess.run([str(CLI), "GroupByHashHip", "--device=hip", "--iterations", "2", "--input_size", "100000",
                        "--groups_count", "1000"], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "DWARF_BENCH_INJECT_FAULT": "1"})
    assert r.returncode == 0 and r.stderr.count("ncorrect results") == 2, r.stderr
