"""Test-only seeded draws for the randomised sweep of the Bloom filter (tests/test_gpu_bloom_fuzz.py on the GPU,
tests/test_bloom_fuzz_host.py on the CPU), built from the dimensions of tests/fuzz_testlib.py: draws(rng) yields about
sixty cases, model(case) is what a correct call leaves behind, and model(case, defect) what a call with exactly one of
DEFECTS would leave behind — the host twin proves that every such defect is rejected by some draw.

A case is a dict of host numpy inputs and parameters; nothing here touches torch or the GPU.  Every dimension (build or
probe, size, list or dense, the column's size and keys, the filter's size and seed, the device count, each flag, ids
outside the column, what the filter and the workspace's status word held before, the placement of every buffer) is drawn
on its own.  A result holds every output IN FULL: the whole filter, or the whole row-id buffer with the entries behind the
count, the device count and the status word.  Never imported by the product."""
import numpy as np

from dwarf_bench_amd import bloom_native as bl
from dwarf_bench_amd import select_native as sn
from tests import bloom_model as blm
from tests import fuzz_testlib as fz

U, W = np.uint32, np.uint64
SEG = sn.SEGMENT_ROWS  # a wave's keys in build and probe
SEAMS = (64, SEG, 2 * SEG)
SEED = 2036  # a draw set that holds every category (tests/test_bloom_fuzz_host.py asserts it)
N_WORDS = (1, 2, 3, 64, 1000, 65537)
DEFECTS = ("count ignored", "count not clamped", "negate ignored", "accumulate ignored", "filter not cleared",
           "1u << b instead of 1ull << b", "word = h % n_words", "seed ignored", "last candidate of a ragged segment dropped",
           "first element of an unaligned column dropped", "bad row id read as row 0", "status not raised",
           "status not cleared", "one entry behind the count written")


def draws(rng, log_uniform=49):
    for i, size in enumerate(fz.sizes(rng, log_uniform, SEAMS, hi_log2=17)):
        what = ("build", "probe")[int(rng.integers(0, 2))]
        listed = bool(rng.integers(0, 2))
        n_col = size if not listed else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 16)))
        col = fz.keys(rng, n_col, int(rng.integers(0, fz.KEY_KINDS)))
        n_words = int(N_WORDS[int(rng.integers(0, len(N_WORDS)))] if rng.integers(0, 4) else rng.integers(1, 1 << 17))
        seed = int(rng.choice([0, 12345, int(rng.integers(1, 1 << 32))]))
        rows = count = None
        if listed:
            rows = fz.row_list(rng, size, n_col, bool(rng.integers(0, 2)))
            count = fz.device_count(rng, size)
            fz.spoil_tail(rng, rows, count, n_col)
        elif what == "build":
            count = fz.device_count(rng, size)  # a dense build takes a count as well
        case = dict(what=what, size=size, col=col, rows=rows, count=count, n_words=n_words, seed=seed, draw=i,
                    fill=fz.FILLS[i % 2], stale_status=int(rng.choice([0, 2, 0xFFFFFFFF, 0x5A5A5A5A])),
                    offs=dict(col=fz.offset(rng), rows=fz.offset(rng), out=fz.offset(rng)))
        if what == "build":
            accumulate = bool(rng.integers(0, 2))
            before = rng.integers(0, 1 << 64, n_words, dtype=W) & rng.integers(0, 1 << 64, n_words, dtype=W)  # a quarter set
            yield dict(case, accumulate=accumulate, flags=bl.ACCUMULATE if accumulate else 0, before=before)
        else:
            held = col[rng.random(n_col) < float(rng.choice([0.0, 0.1, 0.5, 1.0]))]
            bits = int(rng.choice([1, 2, 4, 16]))
            n_words = blm.words(held.size, bits) if rng.integers(0, 2) else n_words
            negate = bool(rng.integers(0, 2))
            yield dict(case, n_words=n_words, filter=blm.build(held, n_words, seed)[0], negate=negate,
                       flags=bl.NEGATE if negate else 0, count_only=bool(rng.integers(0, 5) == 0))


def cases(seed=SEED):
    return list(draws(np.random.default_rng(seed)))


# ---- the model, intact or with one defect ---------------------------------------------------------------------------------
def _place(keys, n_words, seed, defect):
    if defect == "seed ignored":
        seed = 0
    k = np.asarray(keys).view(U)
    h = blm.fmix32(k ^ U(seed))
    word = ((h.astype(W) * W(n_words)) >> W(32)).astype(U) if defect != "word = h % n_words" else h % U(n_words)
    g = blm.fmix32(h ^ U(blm.GOLDEN))
    mask = np.zeros(k.size, W)
    for j in range(4):
        b = (g >> U(6 * j)) & U(63)
        if defect == "1u << b instead of 1ull << b":
            b = b & U(31)  # what a 32-bit shift gives on this hardware: the count modulo 32
        mask |= W(1) << b.astype(W)
    return word, mask


def _entries(case, defect):
    """-> (the keys that count, the row id of each, the ids that do not count) of a case, in candidate order"""
    col, rows, count, size, fill = case["col"], case["rows"], case["count"], case["size"], case["fill"]
    src = col if rows is None else rows
    off = case["offs"]["col" if rows is None else "rows"]
    if defect == "count ignored":
        count = None
    m = blm.length(count, size)
    if defect == "count not clamped" and count is not None and count > size:
        src = np.r_[src, np.full(min(count - size, 64), fill, U)]  # reads on into the guard words behind the buffer
        m = src.size
    e = src[:m]
    ids = np.arange(m, dtype=U)
    if defect == "last candidate of a ragged segment dropped" and m and (off + m) % SEG:
        e, ids = e[:-1], ids[:-1]
    if defect == "first element of an unaligned column dropped" and m and off and e.size:
        e, ids = e[1:], ids[1:]
    if rows is None:
        return e, ids, np.zeros(0, U)
    inside = e.astype(W) < W(col.size)
    if defect == "bad row id read as row 0" and col.size:
        return col[np.where(inside, e, 0)], e, e[~inside]
    return col[e[inside]], e[inside], e[~inside]


def _status(case, bad, defect):
    st = blm.KEY_RANGE if bad.size and defect != "status not raised" else 0
    return st | case["stale_status"] if defect == "status not cleared" else st


def model(case, defect=None):
    assert defect is None or defect in DEFECTS
    keys, ids, bad = _entries(case, defect)
    n_words, seed = case["n_words"], case["seed"]
    if case["what"] == "build":
        accumulate = (case["accumulate"] and defect != "accumulate ignored") or defect == "filter not cleared"
        filt = case["before"].copy() if accumulate else np.zeros(n_words, W)
        word, mask = _place(keys, n_words, seed, defect)
        np.bitwise_or.at(filt, word, mask)
        return dict(filter=filt, status=_status(case, bad, defect))
    word, mask = _place(keys, n_words, seed, defect)
    hit = (case["filter"][word] & mask) == mask
    keep = ~hit if case["negate"] and defect != "negate ignored" else hit
    kept = ids[keep]
    out = np.full(case["size"], case["fill"], U)
    if not case["count_only"]:
        out[: kept.size] = kept
        if defect == "one entry behind the count written" and kept.size < out.size:
            out[kept.size] = 0
    return dict(out=out, count=int(kept.size), status=_status(case, bad, defect))


def check(case, result):
    fz.same(case, result, model(case))
