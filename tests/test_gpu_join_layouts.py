"""The joins on columns that do not start on a 16-byte boundary, at every histogram variant of the partition step
(partition.hip jl_partition_side: one level, plain, fused, fused16, the digit column), at every forced tile shape, at
the geometry of the 2^30 join, and in the engine's sub-joins, which start at arbitrary row counts.

Every input and output column is a view `offset` words past a 16-byte boundary with guard words around it
(join_testlib.guarded): an offset of 1-3 sends the fused histograms to their scalar loops and the match kernel's
16-byte stores of rid / pos / cnt and the build's id stores to unaligned addresses.  Outputs are checked exactly
against numpy up to 2^24 rows and against torch on the GPU above; guards intact and input columns unchanged always.
Which variant and tile shape each case takes is asserted through join_testlib.side_plan, itself checked against the
compiled header by tests/test_capi_symbols.py."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from dwarf_bench_amd import ops  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import join_testlib as jt  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

FILL = 0x5A5A5A5A
ALIGNED, ONES, MIXED = (0,) * 8, (1,) * 8, (1, 2, 3, 1, 2, 3, 1, 2)  # words: bkeys brids pkeys prids | ids rid pos cnt
NUMPY_MAX = (1 << 24) + 5  # up to here the references are numpy's, above torch's on the GPU
FIRST_B, FIRST_P = (1 << 31) - 4097, 12345  # caller row ids: first + row (the build's cross the int32 sign)
M32 = 0xFFFFFFFF


def _offsets(n):
    return [ALIGNED, ONES, MIXED] if n <= NUMPY_MAX else [ALIGNED, MIXED]


def _name(offs):
    return {ALIGNED: "aligned", ONES: "ones", MIXED: "mixed"}[offs]


def _fits(n, m, ws, words_per_row=16):
    """skip when the workspace, the columns and their copies and the torch reference's int64 temporaries (about
    `words_per_row` 4-byte words per row of either side) do not fit the free device memory"""
    need = ws + 4 * words_per_row * (n + m) + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if need > free:
        pytest.skip(f"{n} x {m} rows need {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free")


@functools.lru_cache(maxsize=1)
def _inputs(n, m):
    """uniform build keys in [0, n - 1], probe keys likewise; numpy copies and counts where numpy checks"""
    torch.cuda.empty_cache()
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(m, 43, 0, n - 1)
    if n > NUMPY_MAX:
        return build, probe, None, None, None
    hb, hp = build.cpu().numpy().view(np.uint32), probe.cpu().numpy().view(np.uint32)
    return build, probe, hb, hp, po.join_counts_fast(hb, hp)


def _row_ids(first, n):
    return torch.arange(first, first + n, dtype=torch.int64, device="cuda").to(torch.int32)


class _Columns:
    """guarded copies of the inputs and guarded output columns; check() asserts every guard word and every input word"""

    def __init__(self):
        self.ins, self.outs = [], []

    def input(self, src, off):
        base, view = jt.guarded(src.numel(), off, FILL)
        view.copy_(src)
        self.ins.append((base, view, src))
        return view

    def output(self, n, off):
        base, view = jt.guarded(n, off, FILL)
        self.outs.append((base, view))
        return view

    def check(self):
        torch.cuda.synchronize()
        for base, view, src in self.ins:
            jt.assert_guards(base, view, FILL)
            assert torch.equal(view, src), "an input column changed"
        for base, view in self.outs:
            jt.assert_guards(base, view, FILL)


def _u64(t):
    return t.to(torch.int64) & M32


def _permutation(x, n):
    """x (int64) holds every value of 0..n-1 exactly once"""
    assert int(x.min()) >= 0 and int(x.max()) < n
    c = torch.bincount(x, minlength=n)
    assert c.numel() == n and bool((c == 1).all())


def _torch_check(build, probe, rows, pos, cnt, ids, first_b=0, first_p=0):
    """the 2^28 test's reference on the GPU, for either join: rows = probe row of every output row (None: the probe's
    order); counts per probe row from a bincount of the build keys; ids a permutation of first_b + build rows in which
    every key is one run; every hit's range starts and ends on its key"""
    n, m = build.numel(), probe.numel()
    b64, p64 = _u64(build), _u64(probe)
    if rows is None:
        rows = torch.arange(m, device="cuda")
    else:
        rows = (_u64(rows) - first_p) & M32
        _permutation(rows, m)
    keys_of_rows = p64[rows]
    per_key = torch.bincount(b64, minlength=max(int(b64.max()), int(p64.max())) + 1)
    assert torch.equal(_u64(cnt), per_key[keys_of_rows])
    del per_key
    ids64 = (_u64(ids) - first_b) & M32
    _permutation(ids64, n)
    in_order = b64[ids64]
    assert int((in_order[1:] != in_order[:-1]).sum()) + 1 == torch.unique(b64).numel()
    del in_order
    cnt64, pos64 = _u64(cnt), _u64(pos)
    hit = cnt64 > 0
    assert torch.equal(b64[ids64[pos64[hit]]], keys_of_rows[hit])
    assert torch.equal(b64[ids64[pos64[hit] + cnt64[hit] - 1]], keys_of_rows[hit])


def _radix(n, m, offs, with_rids, build=None, probe=None):
    """the radix join of guarded columns at offsets `offs`; -> the result views (rid, pos, cnt, ids)"""
    cols = _Columns()
    bk = cols.input(build, offs[0])
    br = cols.input(_row_ids(FIRST_B, n), offs[1]) if with_rids else None
    pk = cols.input(probe, offs[2])
    pr = cols.input(_row_ids(FIRST_P, m), offs[3]) if with_rids else None
    plan = ops.RadixJoin(n, m)
    plan.ids, plan.rid = cols.output(n, offs[4]), cols.output(m, offs[5])
    plan.pos, plan.cnt = cols.output(m, offs[6]), cols.output(m, offs[7])
    plan.partition_build(bk, br)
    plan.partition_probe(pk, pr)
    plan.match()
    res = plan.result()
    cols.check()
    return res


def _hash(n, m, offs, pairs, build, probe):
    """the row-ordered join of guarded columns (build rows through dbhip_join_build_pairs_u32 when `pairs`)"""
    cols = _Columns()
    bk = cols.input(build, offs[0])
    br = cols.input(_row_ids(FIRST_B, n), offs[1]) if pairs else None
    pk = cols.input(probe, offs[2])
    plan = ops.HashJoin(n, m)
    plan.ids, plan.pos, plan.cnt = cols.output(n, offs[4]), cols.output(m, offs[6]), cols.output(m, offs[7])
    plan.build(bk, br)
    plan.probe(pk)
    res = plan.result()
    cols.check()
    return res


# ---- B. every histogram variant x column offsets -----------------------------------------------------------------------
def _radix_cases():
    out = []
    for n, radix, _ in jt.LAYOUT_TABLE:
        large, small = jt.radix_probe_sizes(n)
        for offs in _offsets(n):
            for rids in (False, True):
                out.append(pytest.param(n, large, offs, rids, id=f"{radix[3]}-{n}-large-{_name(offs)}-{'rids' if rids else 'index'}"))
        out.append(pytest.param(n, small, MIXED, True, id=f"{radix[3]}-{n}-small-mixed-rids"))
    return out


@pytest.mark.parametrize("n,m,offs,with_rids", _radix_cases())
def test_radix_join_on_unaligned_columns(n, m, offs, with_rids):
    """the radix join with every column at `offs`, without and with caller row ids; the large probe side takes the
    build side's histogram variant, the small one the plain histograms where the build side's are fused"""
    plan_b = jt.side_plan(n, n, jt.JR_ROWS_PER_PART)
    assert plan_b == next(r for k, r, _ in jt.LAYOUT_TABLE if k == n)
    plan_p = jt.side_plan(m, n, jt.JR_ROWS_PER_PART)
    large, _ = jt.radix_probe_sizes(n)
    assert plan_p[3] == (plan_b[3] if m == large or plan_b[3] in ("one level", "plain", "digits") else "plain")
    _fits(n, m, ops._capi.lib().dbhip_join_radix_workspace_bytes(n, m))
    build, probe, hb, hp, counts = _inputs(n, jt.radix_probe_sizes(n)[0])
    probe = probe[:m]  # the small probe side: a prefix of the large one
    fb, fp = (FIRST_B, FIRST_P) if with_rids else (0, 0)
    res = _radix(n, m, offs, with_rids, build, probe)
    if hb is not None:
        jt.check_radix_result(hb, hp[:m], res, fb, fp, counts if m == hp.size else None)
    else:
        rid, pos, cnt, ids = res
        _torch_check(build, probe, rid, pos, cnt, ids, fb, fp)


def _hash_cases():
    return [pytest.param(n, offs, pairs, id=f"{hashed[3]}-{n}-{_name(offs)}-{'pairs' if pairs else 'keys'}")
            for n, _, hashed in jt.LAYOUT_TABLE for offs in _offsets(n) for pairs in (False, True)]


@pytest.mark.parametrize("n,offs,pairs", _hash_cases())
def test_hash_join_on_unaligned_columns(n, offs, pairs):
    """the row-ordered join with every column at `offs`, its build through dbhip_join_build_u32 and through
    dbhip_join_build_pairs_u32 (caller row ids); the probe side is the radix cases' large one"""
    assert jt.side_plan(n, n, jt.JL_ROWS_PER_PART) == next(h for k, _, h in jt.LAYOUT_TABLE if k == n)
    m = jt.radix_probe_sizes(n)[0]
    _fits(n, m, ops._capi.lib().dbhip_join_workspace_bytes(n))
    build, probe, hb, hp, counts = _inputs(n, m)
    first = FIRST_B if pairs else 0
    res = _hash(n, m, offs, pairs, build, probe)
    if hb is not None:
        jt.check_grouped_result(hb, hp, res, first, counts)
    else:
        pos, cnt, ids = res
        _torch_check(build, probe, None, pos, cnt, ids, first)


@functools.lru_cache(maxsize=1)
def _unique_inputs(n):
    ak = po.gen_unique_sorted_u32(n, 11)
    np.random.default_rng(3).shuffle(ak)
    m = n // 2 + 13
    bk = po.gen_unique_sorted_u32(m, 12)
    av, bv = po.gen_uniform_u32(n, 13, 0, 2**32 - 2), po.gen_uniform_u32(m, 14, 0, 2**32 - 2)
    return ak, av, bk, bv, po.ujoin(ak, av, bk, bv)


@pytest.mark.parametrize("offs", [ALIGNED, ONES, MIXED], ids=_name)
def test_unique_join_on_unaligned_columns(offs):
    """the unique-key join at the fused size: distinct shuffled build keys, its payload riding in the row-id column;
    all seven columns at `offs` (build keys, build values, probe keys, probe values | key, build value, probe value)"""
    n = (1 << 24) + 5
    assert jt.side_plan(n, n, jt.JL_ROWS_PER_PART)[3] == "fused"
    ak, av, bk, bv, want = _unique_inputs(n)
    m = bk.size
    cols = _Columns()
    ins = [cols.input(jt.dev(a), o) for a, o in zip((ak, av, bk, bv), offs[:4])]
    plan = ops.UniqueJoin(n, m)
    plan.out_key, plan.out_bval, plan.out_pval = (cols.output(m, o) for o in offs[4:7])
    plan.build(ins[0], ins[1])
    plan.probe(ins[2], ins[3])
    got = [t.cpu().numpy().view(np.uint32) for t in plan.result()]
    cols.check()
    for g, w, name in zip(got, want, ("key", "build value", "probe value")):
        assert np.array_equal(g, w), name
    assert 0 < int((got[0] != M32).sum()) < m


def test_fused16_carries_on_the_scalar_path():
    """jl_hist_fused16_kernel's scalar loop (keys one word past a 16-byte boundary) on skewed keys: every other build row
    holds one key, so a workgroup's share of that key's partition (2^19 rows) wraps its 16-bit counter: the carries
    settled in the global accumulators, as test_join_2_27_rows_skewed_keys_through_the_packed_histogram does aligned"""
    n = (1 << 26) + 5
    m = jt.radix_probe_sizes(n)[0]
    assert jt.side_plan(n, n, jt.JL_ROWS_PER_PART)[3] == "fused16"
    _fits(n, m, ops._capi.lib().dbhip_join_workspace_bytes(n))
    _inputs.cache_clear()
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    build[::2] = 123456789
    probe = ops.gen_uniform_u32(m, 43, 0, n - 1)
    probe[::1000] = 123456789
    pos, cnt, ids = _hash(n, m, ONES, False, build, probe)
    assert int(cnt[0].item()) == (n + 1) // 2
    _torch_check(build, probe, None, pos, cnt, ids)


# ---- C. every forced tile shape, in a fresh process each (the knobs are read once) --------------------------------------
_SHAPES = r"""
import sys
import numpy as np, torch
from dwarf_bench_amd import ops
from oracle import pyoracle as po
from tests import join_testlib as jt, groupby_hash_testlib as gl
from tests import test_gpu_join_layouts as L
t0, t1 = int(sys.argv[1]), int(sys.argv[2])
done = []
for n in (1 << 20, (1 << 21) + 3, (1 << 24) + 5):
    assert jt.side_plan(n, n, jt.JR_ROWS_PER_PART, t0, t1)[4:] == (t0, min(t1, 1))
    m = jt.radix_probe_sizes(n)[0]
    build, probe, hb, hp, counts = L._inputs(n, m)
    jt.check_radix_result(hb, hp, L._radix(n, m, L.ONES, True, build, probe), L.FIRST_B, L.FIRST_P, counts)
    jt.check_radix_result(hb, hp, L._radix(n, m, L.ALIGNED, False, build, probe), counts=counts)
    jt.check_grouped_result(hb, hp, L._hash(n, m, L.MIXED, True, build, probe), L.FIRST_B, counts)
    ak = po.gen_unique_sorted_u32(n, 11)
    np.random.default_rng(3).shuffle(ak)
    bk = po.gen_unique_sorted_u32(n // 2 + 13, 12)
    av, bv = po.gen_uniform_u32(n, 13, 0, 2**32 - 2), po.gen_uniform_u32(bk.size, 14, 0, 2**32 - 2)
    plan = ops.UniqueJoin(n, bk.size)
    plan.build(jt.dev(ak), jt.dev(av))
    plan.probe(jt.dev(bk), jt.dev(bv))
    got = [t.cpu().numpy().view(np.uint32) for t in plan.result()]
    assert all(np.array_equal(g, w) for g, w in zip(got, po.ujoin(ak, av, bk, bv))), "unique join"
    if n > 1 << 20:  # path b of the group-by: two scatter levels
        keys, vals, want = gl.pool_input(n, n)
        k, s, c = (t.cpu().numpy().view(np.uint32) for t in ops.groupby_hash(jt.dev(keys), jt.dev(vals)))
        o = np.argsort(k, kind="stable")
        assert all(np.array_equal(a, b) for a, b in zip((k[o], s[o], c[o]), want)), "group-by"
    done.append(n)
print("SHAPES OK", t0, t1, done)
"""


@pytest.mark.parametrize("t0,t1", [(t0, t1) for t0 in (0, 1, 2) for t1 in (0, 1)], ids=lambda t: str(t))
def test_every_forced_tile_shape(t0, t1):
    """DBHIP_JL_T0 / DBHIP_JL_T1 forced (read once per process: a child each, one after another): the radix join with
    every column one word off and with aligned ones, the hash join at mixed offsets, the unique join and the group-by's
    path b, against numpy, at one level, plain and fused sizes.  Level-0 shape 1 is selected by no default."""
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, "-c", _SHAPES, str(t0), str(t1)], capture_output=True, text=True, timeout=900,
                       env={**os.environ, "DBHIP_JL_T0": str(t0), "DBHIP_JL_T1": str(t1)}, cwd=str(ROOT))
    assert r.returncode == 0 and f"SHAPES OK {t0} {t1}" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- D. the geometry of the 2^30 join at its natural size --------------------------------------------------------------
def test_headline_geometry_at_its_natural_size():
    """(1 << 29) + 12345 build rows: 586 x 512 partitions for the radix join and 513 x 512 for the row-ordered one —
    16384-row level-0 tiles and, only from 2^29 rows, 1024 x 8 level-1 tiles (t1 = 1), whose rows also set the level-0
    tile starts.  Against torch, as the 2^28 test; output columns at mixed offsets behind guards."""
    n, m = jt.HEADLINE_BUILD, jt.HEADLINE_PROBE
    assert (jt.side_plan(n, n, jt.JR_ROWS_PER_PART), jt.side_plan(n, n, jt.JL_ROWS_PER_PART)) == jt.HEADLINE_PLANS
    assert jt.side_plan(m, n, jt.JR_ROWS_PER_PART)[3:] == ("digits", 2, 1)
    _fits(n, m, ops._capi.lib().dbhip_join_radix_workspace_bytes(n, m))
    _inputs.cache_clear()
    torch.cuda.empty_cache()
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(m, 43, 0, n - 1)
    offs = (0, 0, 0, 0, 1, 2, 3, 1)
    rid, pos, cnt, ids = _radix(n, m, offs, False, build, probe)
    _torch_check(build, probe, rid, pos, cnt, ids)
    del rid, pos, cnt, ids
    torch.cuda.empty_cache()
    pos, cnt, ids = _hash(n, m, offs, False, build, probe)
    _torch_check(build, probe, None, pos, cnt, ids)
