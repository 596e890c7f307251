"""Test-only seeded draws for the randomised sweep of the HyperLogLog sketch (tests/test_gpu_hll_fuzz.py on the GPU,
tests/test_hll_fuzz_host.py on the CPU), built from the dimensions of tests/fuzz_testlib.py: draws(rng) yields about sixty
cases, model(case) is what a correct call leaves behind, and model(case, defect) what a call with exactly one of DEFECTS
would leave behind — the host twin proves that every such defect is rejected by some draw.

A case is a dict of host numpy inputs and parameters; nothing here touches torch or the GPU.  Every dimension (build or
merge, size, list or dense, the number of columns, their size and keys — a quarter of them built against the hash, so that
the rank comes from the g half — p and the seed, the device count, the flag, ids outside the columns, what the registers and
the workspace's status word held before, the placement of every buffer) is drawn on its own.  A result holds every output IN
FULL: all registers, all 64 histogram words and the status word.  Never imported by the product."""
import numpy as np

from dwarf_bench_amd import hll_native as hl
from dwarf_bench_amd import select_native as sn
from tests import fuzz_testlib as fz
from tests import hll_model as hm

U, W, B = np.uint32, np.uint64, np.uint8
SEG = sn.SEGMENT_ROWS  # a workgroup's candidates per step of the build
SEAMS = (64, SEG, 2 * SEG)
SEED = 2041  # a draw set that holds every category (tests/test_hll_fuzz_host.py asserts it)
PS = (4, 5, 11, 14)
BEFORE = ("fill", "zeros", "sketch", "spoiled")
DEFECTS = ("count ignored", "count not clamped", "accumulate ignored", "registers not cleared", "seed ignored",
           "second column ignored", "columns hashed in the wrong order", "idx taken from the low bits", "rank off by one",
           "32-bit clz, the g half ignored", "last writer wins instead of max", "histogram not recounted on merge",
           "stored byte above q+1 not clamped", "last element of a ragged segment dropped",
           "first element of an unaligned column dropped", "bad row id read as row 0", "status not raised",
           "status not cleared")


def held_before(rng, kind, p, fill):
    """what a register buffer holds before a call"""
    m = 1 << p
    if kind == "fill":
        return np.full(m, fill & 0xFF, B)  # both fills repeat one byte, and both lie above every q+1
    if kind == "zeros":
        return np.zeros(m, B)
    regs = hm.build(rng.integers(0, 1 << 32, int(2 ** rng.uniform(0, 16)), dtype=np.uint64).astype(U), p, 1)[0]
    if kind == "spoiled":
        at = rng.integers(0, m, max(m // 16, 1))
        regs[at] = rng.choice(np.array([64 - p + 2, 64 - p + 3, 0x7F, 0x80, 0xFF], B), at.size)
    return regs


def draws(rng, log_uniform=49):
    for i, size in enumerate(fz.sizes(rng, log_uniform, SEAMS, hi_log2=17)):
        what = "merge" if rng.integers(0, 6) == 0 else "build"
        p = int(PS[int(rng.integers(0, 4))] if rng.integers(0, 3) else rng.integers(hm.MIN_P, hm.MAX_P + 1))
        fill = fz.FILLS[i % 2]
        case = dict(what=what, size=size, p=p, draw=i, fill=fill, stale_status=int(rng.choice([0, 2, 0xFFFFFFFF, 0x5A5A5A5A])))
        if what == "merge":
            kinds = [BEFORE[int(rng.integers(1, 4))] for _ in range(2)]
            same_buffer = bool(rng.integers(0, 4) == 0)
            dst = held_before(rng, kinds[0], p, fill)
            yield dict(case, dst=dst, src=dst if same_buffer else held_before(rng, kinds[1], p, fill), same_buffer=same_buffer,
                       held=kinds[0], src_held=kinds[0] if same_buffer else kinds[1])
            continue
        listed = bool(rng.integers(0, 2))
        n_cols = int(rng.integers(1, hm.MAX_COLS + 1))
        n_col = size if not listed else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 16)))
        cols = [fz.keys(rng, n_col, int(rng.integers(0, fz.KEY_KINDS))) for _ in range(n_cols)]
        seed = int(rng.choice([0, 12345, int(rng.integers(1, 1 << 32))]))
        built = bool(rng.integers(0, 4) == 0)
        if built:  # the last column against the hash of those in front: every rank comes from the g half
            cols[-1] = hm.keys_ranked_by_g(n_col, p, seed, rng, cols[:-1])
        rows = None
        if listed:
            rows = fz.row_list(rng, size, n_col, bool(rng.integers(0, 2)))
            count = fz.device_count(rng, size)
            fz.spoil_tail(rng, rows, count, n_col)
        else:
            count = fz.device_count(rng, size)  # a dense build takes a count as well
        accumulate = bool(rng.integers(0, 2))
        held = BEFORE[int(rng.integers(0, 4))]
        yield dict(case, cols=cols, rows=rows, count=count, seed=seed, built=built, accumulate=accumulate,
                   flags=hl.ACCUMULATE if accumulate else 0, held=held, before=held_before(rng, held, p, fill),
                   offs=dict(cols=[fz.offset(rng) for _ in range(n_cols)], rows=fz.offset(rng)))


def cases(seed=SEED):
    return list(draws(np.random.default_rng(seed)))


# ---- the model, intact or with one defect ---------------------------------------------------------------------------------
def _place(cols, p, seed, defect):
    if defect == "seed ignored":
        seed = 0
    if defect == "second column ignored" and len(cols) > 1:
        cols = cols[:1] + cols[2:]
    if defect == "columns hashed in the wrong order":
        cols = cols[::-1]
    h, g = hm.hash_tuples(cols, seed)
    idx, rank = hm.place(h, g, p)
    if defect == "idx taken from the low bits":
        idx = g & U((1 << p) - 1)
    if defect == "rank off by one":
        rank = rank - B(1)
    if defect == "32-bit clz, the g half ignored":
        hp = h << U(p)
        rank = np.where(hp == 0, 32 - p + 1, hm.clz64(hp.astype(W)) - 32 + 1).astype(B)
    return idx, rank


def _entries(case, defect):
    """-> (the key tuples that count, column by column; the ids that do not count) of a build, in candidate order"""
    cols, rows, count, size, fill = case["cols"], case["rows"], case["count"], case["size"], case["fill"]
    n_col = cols[0].size
    if defect == "count ignored":
        count = None
    m = hm.length(count, size)
    over = 0
    if defect == "count not clamped" and count is not None and count > size:
        over = min(count - size, 64)  # reads on into the guard words behind the buffer
    if rows is None:
        lo, hi = 0, m
        if defect == "last element of a ragged segment dropped" and m and (case["offs"]["cols"][0] + m) % SEG:
            hi -= 1
        if defect == "first element of an unaligned column dropped" and m and case["offs"]["cols"][0] and hi > lo:
            lo += 1
        return [np.r_[c[lo:hi], np.full(over, fill, U)] for c in cols], np.zeros(0, U)
    e = np.r_[rows[:m], np.full(over, fill, U)]
    if defect == "last element of a ragged segment dropped" and e.size and (case["offs"]["rows"] + e.size) % SEG:
        e = e[:-1]
    if defect == "first element of an unaligned column dropped" and e.size and case["offs"]["rows"]:
        e = e[1:]
    inside = e.astype(W) < W(n_col)
    if defect == "bad row id read as row 0" and n_col:
        return [c[np.where(inside, e, 0)] for c in cols], e[~inside]
    return [c[e[inside]] for c in cols], e[~inside]


def _join(held, p, defect):
    """the bytes a call joins with: clamped to q+1, raising the status -> (bytes, status)"""
    if defect == "stored byte above q+1 not clamped":
        return np.asarray(held).copy(), hm.clamp(held, p)[1]
    clamped, st = hm.clamp(held, p)
    return clamped.copy(), st


def _hist(registers):
    return np.bincount(registers, minlength=hm.HIST_WORDS).astype(U)[: hm.HIST_WORDS]


def _status(case, st, defect):
    if defect == "status not raised":
        st = 0
    return st | case["stale_status"] if defect == "status not cleared" else st


def model(case, defect=None):
    assert defect is None or defect in DEFECTS
    p = case["p"]
    if case["what"] == "merge":
        dst, s1 = _join(case["dst"], p, defect)
        src, s2 = _join(case["src"], p, defect)
        out = np.maximum(dst, src)
        hist = _hist(dst) if defect == "histogram not recounted on merge" else _hist(out)
        return dict(registers=out, hist=hist, status=_status(case, s1 | s2, defect))
    keys, bad = _entries(case, defect)
    st = hm.KEY_RANGE if bad.size else 0
    accumulate = (case["accumulate"] and defect != "accumulate ignored") or defect == "registers not cleared"
    if accumulate:
        registers, s0 = _join(case["before"], p, defect)
        st |= s0 if case["accumulate"] else 0
    else:
        registers = np.zeros(1 << p, B)
    idx, rank = _place(keys, p, case["seed"], defect)
    if defect == "last writer wins instead of max":
        registers[idx] = rank
    else:
        np.maximum.at(registers, idx, rank)
    return dict(registers=registers, hist=_hist(registers), status=_status(case, st, defect))


def check(case, result):
    fz.same(case, result, model(case))
