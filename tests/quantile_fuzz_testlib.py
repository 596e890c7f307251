"""Test-only seeded draws for the randomised sweep of the quantile select (tests/test_gpu_quantile_fuzz.py on the GPU,
tests/test_quantile_fuzz_host.py on the CPU), built from the dimensions of tests/fuzz_testlib.py: draws(rng) yields about a
hundred cases of at most 2^17 rows, model(case) is what a correct call leaves behind, and model(case, defect) what a call with
exactly one of DEFECTS would leave behind — the host twin proves that every such defect is rejected by some draw.

The twin is the select as the kernels run it — three levels over 11 / 11 / 10-bit digits, the slots of distinct prefixes, per
rank the bin, the remainder and the running count below — so that a defect can sit where it would sit in a kernel; without a
defect it must agree with tests/quantile_model.py, which sorts.

A case is a dict of host numpy inputs and parameters; nothing here touches torch or the GPU.  Every dimension (size, list or
all rows, the column's size and keys, the device count, ids outside the column, the order, the number of ranks and each
rank's kind, the stale status word, the placement of every buffer) is drawn on its own.  A result holds the three output
columns IN FULL and the status word.  Never imported by the product."""
import numpy as np

from tests import fuzz_testlib as fz
from tests import quantile_model as qm

U, W = np.uint32, np.uint64
ROUND = 8192  # positions of one round of a histogram workgroup
SEAMS = (64, ROUND, 2 * ROUND)
SEED = 2605  # a draw set that holds every category (tests/test_quantile_fuzz_host.py asserts it)
TOP = (1 << 32) - 1
RANK_KINDS = ("absolute inside", "absolute m", "absolute 2^32 - 1", "fraction", "zero", "one", "half", "repeat")
N_QS = (1, 2, 4, 5, 9, 16)
DEFECTS = ("rank off by one", "< for <= in the bin pick", "last n & 3 keys dropped", "sign flip ignored",
           "count not clamped", "invalid ids counted in m", "another slot's remainder", "level-2 digit 11 bits wide")


def _ranks(rng, n_q, m):
    """n_q ranks of drawn kinds for a call of about m candidates -> (q_num, q_den, kinds)"""
    num, den, kinds = [], [], []
    for j in range(n_q):
        kind = RANK_KINDS[int(rng.integers(0, len(RANK_KINDS)))]
        if kind == "repeat" and not num:
            kind = "half"
        if kind == "absolute inside":
            q = (int(rng.integers(0, max(m, 1))), 0)
        elif kind == "absolute m":
            q = (m, 0)
        elif kind == "absolute 2^32 - 1":
            q = (TOP, 0)
        elif kind == "fraction":
            d = int(rng.choice([3, 10, 100, 10 ** 9, TOP, int(rng.integers(1, 1 << 32))]))
            q = (int(rng.integers(0, d + 1)), d)
        elif kind == "repeat":
            at = int(rng.integers(0, len(num)))
            q = (num[at], den[at])
        else:
            q = {"zero": (0, 1), "one": (1, 1), "half": (1, 2)}[kind]
        num.append(q[0])
        den.append(q[1])
        kinds.append(kind)
    return num, den, kinds


def draws(rng, log_uniform=85):
    for i, size in enumerate(fz.sizes(rng, log_uniform, SEAMS, hi_log2=17)):
        listed = bool(rng.integers(0, 2))
        n_col = size if not listed else (0 if rng.integers(0, 12) == 0 else int(2 ** rng.uniform(0, 16)))
        col = fz.keys(rng, n_col, int(rng.integers(0, fz.KEY_KINDS)))
        rows = None
        if listed:
            rows = fz.row_list(rng, size, n_col, bool(rng.integers(0, 2)))
            count = fz.device_count(rng, size)
            fz.spoil_tail(rng, rows, count, n_col)
        else:
            count = fz.device_count(rng, size)  # a call over all rows takes a count as well
        signed = bool(rng.integers(0, 2))
        n_q = int(N_QS[int(rng.integers(0, len(N_QS)))] if rng.integers(0, 3) else rng.integers(1, qm.MAX_RANKS + 1))
        m = fz.counted(count, size)
        num, den, kinds = _ranks(rng, n_q, m)
        yield dict(what="quantile", size=size, draw=i, fill=fz.FILLS[i % 2], col=col, rows=rows, count=count, signed=signed,
                   flags=qm.SIGNED if signed else 0, num=num, den=den, rank_kinds=kinds,
                   stale_status=int(rng.choice([0, 2, 0xFFFFFFFF, 0x5A5A5A5A])),
                   offs=dict(col=fz.offset(rng), rows=fz.offset(rng), out=[fz.offset(rng) for _ in range(3)]))


def cases(seed=SEED):
    return list(draws(np.random.default_rng(seed)))


# ---- the twin: the select level by level, intact or with one defect -----------------------------------------------------------
def _candidates(case, defect):
    """-> (the keys that count, the ids that do not) in candidate order"""
    col, rows, count, size, fill = case["col"], case["rows"], case["count"], case["size"], case["fill"]
    m = qm.length(count, size)
    over = 0
    if defect == "count not clamped" and count is not None and count > size:
        over = min(count - size, 64)  # reads on into the guard words behind the buffer
    if defect == "last n & 3 keys dropped":
        m -= m & 3
    if rows is None:
        return np.r_[col[:m], np.full(over, fill, U)], np.zeros(0, U)
    e = np.r_[rows[:m], np.full(over, fill, U)]
    inside = e.astype(W) < W(col.size)
    return col[e[inside]], e[~inside]


def _histogram(x, prefix, level, width):
    """the counts per digit (2^width bins) of the x whose bits above the level's digit equal the prefix's"""
    shift = qm.SHIFTS[level]
    above = shift + width  # a digit counted too wide also narrows the compare with the prefix: the bits overlap
    under = x if above == 32 else x[(x >> U(above)) == (prefix >> above)]
    return np.bincount(((under >> U(shift)) & U((1 << width) - 1)).astype(np.int64), minlength=1 << width)


def model(case, defect=None):
    assert defect is None or defect in DEFECTS
    keys, bad = _candidates(case, defect)
    flip = U(0x80000000 if case["signed"] and defect != "sign flip ignored" else 0)
    x = keys ^ flip
    m = int(x.size) + (int(bad.size) if defect == "invalid ids counted in m" else 0)
    n_q = len(case["num"])
    slot, rem, below = [None] * n_q, [0] * n_q, [0] * n_q
    for j, (num, den) in enumerate(zip(case["num"], case["den"])):
        r = qm.rank(num, den, m)
        if r is not None and defect == "rank off by one" and den:
            r = r + 1 if r + 1 < m else None
        if r is not None:
            slot[j], rem[j] = 0, r
    prefixes, equal = [0], [0] * n_q
    for level in range(3):
        width = 11 if (level == 2 and defect == "level-2 digit 11 bits wide") else qm.WIDTHS[level]
        hists = [_histogram(x, p, level, width) for p in prefixes]
        nxt = []
        for j in range(n_q):
            if slot[j] is None:
                continue
            mine = rem[j]
            if defect == "another slot's remainder" and level > 0:  # the remainder kept per slot: the slot's first rank's
                mine = rem[min(k for k in range(n_q) if slot[k] == slot[j])]
            h = hists[slot[j]]
            ends = np.cumsum(h)
            digit, before, count = 0, 0, 0  # what a pick that finds no bin leaves behind
            for d in np.flatnonzero(h):
                b = int(ends[d] - h[d])
                holds = (b < mine if defect == "< for <= in the bin pick" else b <= mine) and mine - b < int(h[d])
                if holds:
                    digit, before, count = int(d), b, int(h[d])
            prefix = prefixes[slot[j]] | ((digit << qm.SHIFTS[level]) & TOP)
            if prefix not in nxt:
                nxt.append(prefix)
            slot[j], rem[j], below[j], equal[j] = nxt.index(prefix), (mine - before) & TOP, (below[j] + before) & TOP, count
        prefixes = nxt
    values = np.array([(prefixes[slot[j]] ^ int(flip)) if slot[j] is not None else 0 for j in range(n_q)], U)
    below = np.array([below[j] if slot[j] is not None else m & TOP for j in range(n_q)], U)
    equal = np.array([equal[j] if slot[j] is not None else 0 for j in range(n_q)], U)
    return dict(values=values, below=below, equal=equal, status=qm.KEY_RANGE if bad.size else 0)


def check(case, result):
    fz.same(case, result, model(case))
