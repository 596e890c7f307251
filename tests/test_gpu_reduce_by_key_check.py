"""dbhip_check_reduce_by_key_u32 on the device against its numpy restatement (tests/reduce_by_key_model.py): the four words
agree bit for bit on right tables and on every kind of poke, and the verdict drawn from them accepts the right tables
only.  Guarded buffers throughout: the input columns and the table frozen, a workspace of exactly the queried size,
poisoned before the call, four result words between guards."""
import numpy as np
import pytest
import torch

from tests import reduce_by_key_model as rm
from tests.guard_testlib import FILLS, Watch, ptr
from tests.test_gpu_reduce_by_key import key_shapes, run_keys, uniform

pytestmark = pytest.mark.gpu
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


def _lib():
    from dwarf_bench_amd import _capi
    return _capi.lib()


def device_words(keys, vals, table, signed, fill=FILLS[0], poison=0xFF):
    """one guarded validator call -> the four words"""
    lib = _lib()
    w = Watch(fill)
    n, runs = keys.size, table[0].size
    dk, dv = w.col(n, data=keys, freeze=True), w.col(n, data=vals, freeze=True)
    cols = [w.col(runs, data=table[0], freeze=True), w.col(runs, data=table[1], freeze=True), w.u64(runs),
            w.col(runs, data=table[3], freeze=True), w.col(runs, data=table[4], freeze=True)]
    cols[2].copy_(torch.from_numpy(np.ascontiguousarray(table[2]).view(np.int64)))
    w.freeze(cols[2])
    res = w.u64(4)
    ws_bytes = lib.dbhip_check_reduce_by_key_workspace_bytes(n, runs)
    ws = w.ws(ws_bytes)
    ws.fill_(poison)
    rc = lib.dbhip_check_reduce_by_key_u32(ptr(dk), ptr(dv), n, int(signed), *(ptr(c) for c in cols), runs, ptr(res), ptr(ws),
                                           ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    w.check()
    return tuple(int(x) & M64 for x in res.cpu().tolist())


def judge(keys, vals, table, signed, **kw):
    words = device_words(keys, vals, table, signed, **kw)
    assert words == rm.check_words(keys, vals, *table, signed), (words, signed)
    return rm.verdict(words)


@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
def test_right_tables_are_accepted(n):
    vals = uniform(n, n + 1)
    for i, (what, keys) in enumerate(key_shapes(n, seed=n)):
        for signed in (False, True):
            table = rm.reduce_by_key(keys, vals, signed)
            assert judge(keys, vals, table, signed, fill=FILLS[i % 2], poison=(0xFF, 0x00)[i % 2]), (what, signed)


def pokes(keys, vals, table, signed):
    """(what, table) of every kind of damage, each at a run in the middle of the table"""
    runs = table[0].size
    r = runs // 2

    def copy():
        return [c.copy() for c in table]

    t = copy()
    t[1][r] -= 1
    t[1][r + 1] += 1
    yield "a count moved to the next run", t
    t = copy()
    t[0][r] ^= np.uint32(0x10000)
    yield "a key changed", t
    for col, step, what in ((3, -1, "min lowered by one"), (4, 1, "max raised by one")):
        t = copy()
        t[col][r] = np.uint32((int(t[col][r]) + step) & M32)
        yield what, t
    for step in (1, -1):
        t = copy()
        t[2][r] = np.uint64((int(t[2][r]) + step) & M64)
        yield f"a sum {step:+d}", t
    starts = np.r_[0, np.cumsum(table[1].astype(np.int64))]
    lo, mid, hi = int(starts[r]), int(starts[r + 1]), int(starts[r + 2])
    merged = rm.reduce_by_key(np.full(hi - lo, keys[lo], dtype=np.uint32), vals[lo:hi], signed)
    yield "two runs merged", [np.r_[c[:r], m, c[r + 2:]].astype(c.dtype) for c, m in zip(table, merged)]
    long_run = int(np.argmax(table[1]))
    lo, hi = int(starts[long_run]), int(starts[long_run + 1])
    if hi - lo >= 2:
        cut = lo + (hi - lo) // 2
        a, b = rm.reduce_by_key(keys[lo:cut], vals[lo:cut], signed), rm.reduce_by_key(keys[cut:hi], vals[cut:hi], signed)
        yield "a run split", [np.r_[c[:long_run], x, y, c[long_run + 1:]].astype(c.dtype) for c, x, y in zip(table, a, b)]
    t = copy()
    t[1][-1] += 1
    yield "a count total above n", t
    yield "a count total below n", [c[:-1] for c in table]


@pytest.mark.parametrize("n", [5000, (1 << 20) + 5])
@pytest.mark.parametrize("signed", [False, True])
def test_every_kind_of_poke_is_rejected(n, signed):
    keys, vals = run_keys(n, 40, n + 7), uniform(n, n + 8)
    table = rm.reduce_by_key(keys, vals, signed)
    assert judge(keys, vals, table, signed)
    seen = []
    for what, t in pokes(keys, vals, table, signed):
        assert not judge(keys, vals, t, signed), what
        seen.append(what)
    assert len(seen) == 10, seen


def test_tables_that_point_outside_the_arrays_are_read_inside_them():
    n = 5000
    keys, vals = run_keys(n, 40, 3), uniform(n, 4)
    table = rm.reduce_by_key(keys, vals)
    for count in (0xFFFFFFFF, 0x80000000, n):
        t = [c.copy() for c in table]
        t[1][1] = count  # the starts behind it lie outside the column, or wrap
        assert not judge(keys, vals, t, False)
    empty = [c[:0] for c in table]
    assert not judge(keys, vals, empty, False)  # no runs: every row is behind the table
    none = np.zeros(0, dtype=np.uint32)
    assert judge(none, none, empty, False)  # no rows and no runs
