"""The validators' numpy model (tests/validator_model.py) against brute-force truth, without a GPU.

The GPU suite (tests/test_gpu_validators.py) only shows that the device produces the model's words.  That the WORDS decide
rightly is shown here, on cases small enough to state the truth outright: over seeded sets of mutated outputs the verdict
drawn from the words equals "this output is a right answer", with two families of exceptions, the closed blind list:

  (a) the group-by's weighted sums cannot see an error spread over several groups when both weighted differences vanish
      (a single group's error is always seen; 2^31 moved between two groups never is);
  (b) the join check does not look at out_pos of a probe row without a match (the contract is 0).

Truth for the one-to-many join is the output contract of both join paths: ids is a permutation of the build rows in
which every key is one run, and every probe row's (pos, cnt) is that run (0 / 0 without a match).
"""
import numpy as np
import pytest

from tests import validator_model as vm

pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered")  # uint32 columns wrap on purpose
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
M32 = vm.M32


def test_model_mix64_is_the_oracles_and_the_golden_one():
    vm.self_check()


def test_fingerprint_is_the_sequential_definition():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 65, 1000):
        seq = rng.integers(INT_MIN, INT_MAX, n, endpoint=True).astype(np.int32)
        h = 0
        for x in seq:
            h = (h * vm.FP_MUL + (int(np.uint32(x)) + 1)) & vm.M64
        assert vm.fingerprint(seq) == [h, n]
    assert vm.fp_geo(0) == (1, 1) and vm.fp_geo(16385) == (2, 33) and vm.fp_geo(1048577) == (65, 64)
    assert vm.fp_geo((1 << 24) + (1 << 16) + 5) == (1024, 65)


# ---- scan ------------------------------------------------------------------------------------------------------------------
def _mutate_seq(rng, seq, pool):
    """one random edit of a sequence (possibly none): what a wrong compaction could leave behind"""
    out = list(seq)
    op = rng.integers(0, 7)
    if op == 1 and len(out) >= 2:
        i, j = rng.choice(len(out), 2, replace=False)
        out[i], out[j] = out[j], out[i]
    elif op == 2 and out:
        del out[rng.integers(len(out))]
    elif op == 3 and out:
        i = rng.integers(len(out))
        out.insert(i, out[i])
    elif op == 4:
        out.insert(rng.integers(len(out) + 1), int(rng.choice(pool)))
    elif op == 5 and out:
        out[rng.integers(len(out))] = int(rng.choice(pool))
    elif op == 6 and out:
        out.pop()
    return out


def test_scan_verdict_is_the_truth():
    rng = np.random.default_rng(2)
    pool = np.array([INT_MIN, INT_MIN + 1, -2, -1, 0, 1, 2, 3, INT_MAX - 1, INT_MAX], dtype=np.int64)
    seen = {True: 0, False: 0}
    for _ in range(4000):
        n = int(rng.integers(0, 13))
        src = rng.choice(pool, n).astype(np.int32)
        filt = int(rng.choice([INT_MIN, -1, 0, 2, INT_MAX]))
        right = src[src < filt].tolist()
        out = _mutate_seq(rng, right, pool)
        if len(out) > n:
            continue
        truth = out == right
        want = vm.fingerprint_lt(src, filt)
        got = vm.fingerprint_lt(np.array(out, dtype=np.int32), filt)
        assert vm.verdict_scan(len(out), got, want) == truth, (src, filt, out)
        seen[truth] += 1
    assert min(seen.values()) > 300


# ---- sort ------------------------------------------------------------------------------------------------------------------
KEY_POOL = np.array([0, 1, 2, 3, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def _sort(keys, signed):
    return keys[np.argsort(keys.view(np.int32) if signed else keys, kind="stable")]


@pytest.mark.parametrize("signed", [False, True])
def test_sort_verdict_is_the_truth(signed):
    rng = np.random.default_rng(3 + signed)
    seen = {True: 0, False: 0}
    for _ in range(4000):
        n = int(rng.integers(0, 13))
        keys = rng.choice(KEY_POOL, n)
        right = _sort(keys, signed)
        out = right.copy()
        op = rng.integers(0, 5)
        if op == 1 and n >= 2:
            i, j = rng.choice(n, 2, replace=False)
            out[[i, j]] = out[[j, i]]
        elif op == 2 and n >= 2:  # the key sum kept: +1 here, -1 there
            i, j = rng.choice(n, 2, replace=False)
            out[i] += np.uint32(1)
            out[j] -= np.uint32(1)
        elif op == 3 and n:
            out[rng.integers(n)] = rng.choice(KEY_POOL)
        elif op == 4 and n >= 2:  # a multiset change that keeps the order
            out[rng.integers(1, n)] = out[0]
            out = _sort(out, signed)
        truth = np.array_equal(out, right)
        assert vm.verdict_sort(vm.sorted_words(out, signed), vm.sorted_words(keys, signed)) == truth, (keys, out)
        seen[truth] += 1
    assert min(seen.values()) > 300


@pytest.mark.parametrize("signed", [False, True])
def test_sort_pairs_verdict_is_the_truth(signed):
    rng = np.random.default_rng(5 + signed)
    seen = {True: 0, False: 0}
    for _ in range(4000):
        n = int(rng.integers(0, 13))
        keys = rng.choice(KEY_POOL[::3], n)
        perm = np.argsort(keys.view(np.int32) if signed else keys, kind="stable").astype(np.uint32)
        out_k, out_i = keys[perm].copy(), perm.copy()
        op = rng.integers(0, 6)
        if op == 1 and n >= 2:
            i = rng.integers(n - 1)
            out_i[[i, i + 1]] = out_i[[i + 1, i]]  # a tie broken the wrong way, or an id beside another key
        elif op == 2 and n:
            out_i[rng.integers(n)] = rng.choice([n, M32])
        elif op == 3 and n:
            out_i[rng.integers(n)] = rng.integers(n)
        elif op == 4 and n >= 2:
            i = rng.integers(n - 1)
            out_i[i + 1] = out_i[i]
        elif op == 5 and n >= 2:
            i, j = rng.choice(n, 2, replace=False)
            out_k[[i, j]], out_i[[i, j]] = out_k[[j, i]], out_i[[j, i]]
        truth = np.array_equal(out_k, keys[perm]) and np.array_equal(out_i, perm)
        assert vm.verdict_sort_pairs(vm.sorted_pairs(keys, out_k, out_i, signed)) == truth, (keys, out_k, out_i)
        seen[truth] += 1
    assert min(seen.values()) > 300


# ---- hash group-by ---------------------------------------------------------------------------------------------------------
def _groupby_rows(keys, vals):
    uk, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    sums = np.zeros(uk.size, dtype=np.uint64)
    np.add.at(sums, inv, vals.astype(np.uint64))
    return uk.astype(np.uint32), (sums & np.uint64(M32)).astype(np.uint32), counts.astype(np.uint32)


def _rows(k, s, c):
    return sorted(zip(k.tolist(), s.tolist(), c.tolist()))


def test_groupby_hash_verdict_is_the_truth_but_for_cross_group_moves():
    rng = np.random.default_rng(7)
    seen = {"right": 0, "caught": 0, "blind": 0}
    for trial in range(3000):
        n = int(rng.integers(1, 13))
        pool = rng.integers(0, M32, int(rng.integers(1, 5)), endpoint=True).astype(np.uint32)
        keys, vals = rng.choice(pool, n), rng.integers(0, M32, n, endpoint=True).astype(np.uint32)
        k, s, c = _groupby_rows(keys, vals)
        g = k.size
        order = rng.permutation(g)  # any row order is a right answer
        k, s, c = k[order], s[order], c[order]
        want = _rows(k, s, c)
        op = rng.integers(0, 8)
        if op == 1:
            s[rng.integers(g)] += np.uint32(rng.choice([1, 1 << 31, int(rng.integers(1, M32))]))
        elif op == 2 and g >= 2:  # a value moved from one group's sum to another's
            i, j = rng.choice(g, 2, replace=False)
            d = np.uint32(rng.choice([1, 1 << 31, 1 << 30, int(rng.integers(1, M32))]))
            s[i] += d
            s[j] -= d
        elif op == 3 and g >= 2:
            i, j = rng.choice(g, 2, replace=False)
            s[[i, j]] = s[[j, i]]
        elif op == 4:  # a key emitted twice, its sum and count split
            i = rng.integers(g)
            half = np.uint32(rng.integers(0, M32))
            k, s, c = np.append(k, k[i]), np.append(s, s[i] - half), np.append(c, np.uint32(0))
            s[i] = half
        elif op == 5 and g >= 2:  # a count moved between groups
            i, j = rng.choice(g, 2, replace=False)
            c[i] += np.uint32(1)
            c[j] -= np.uint32(1)
        elif op == 6 and g >= 2:
            k, s, c = k[:-1], s[:-1], c[:-1]
        elif op == 7:
            c[rng.integers(g)] += np.uint32(1)
        truth = _rows(k, s, c) == want
        verdict = vm.verdict_groupby_hash(keys, vals, k, s, c)
        if truth:
            assert verdict, (trial, op)
            seen["right"] += 1
        elif verdict:  # family (a), and nothing else: the keys stand, several groups' sums or counts are off
            got = dict((a, (b, cc)) for a, b, cc in _rows(k, s, c))
            assert len(got) == len(want) and sorted(got) == [w[0] for w in want], (trial, op)
            assert sum(got[a] != (b, cc) for a, b, cc in want) >= 2, (trial, op)
            assert op in (2, 3), (trial, op)
            seen["blind"] += 1
        else:
            seen["caught"] += 1
    assert seen["right"] > 300 and seen["caught"] > 1000 and seen["blind"] > 20


def test_weighted_sum_single_group_errors_are_always_caught_and_a_2p31_move_never():
    """what the arithmetic guarantees: w odd makes v -> v * w a bijection mod 2^32, so one group's error d != 0 shows as
    d * w != 0 in BOTH words; w(g1) - w(g2) is even, so 2^31 * (w(g1) - w(g2)) = 0 mod 2^32 in both"""
    rng = np.random.default_rng(8)
    groups = 1000
    sums = rng.integers(0, M32, groups, endpoint=True).astype(np.uint32)
    base = vm.weighted_sum(None, sums)
    w0, w1 = vm.weights(np.arange(groups, dtype=np.uint32))
    assert bool(np.all(w0 & np.uint64(1))) and bool(np.all(w1 & np.uint64(1)))
    for d in [1, 2, 1 << 24, 1 << 30, 1 << 31, M32] + rng.integers(1, M32, 200).tolist():
        g = int(rng.integers(groups))
        bad = sums.copy()
        bad[g] += np.uint32(d)
        got = vm.weighted_sum(None, bad)
        assert got[0] != base[0] and got[1] != base[1], (d, g)
    for _ in range(200):
        i, j = rng.choice(groups, 2, replace=False)
        bad = sums.copy()
        bad[i] += np.uint32(1 << 31)
        bad[j] -= np.uint32(1 << 31)
        assert vm.weighted_sum(None, bad) == base, (i, j)


def weighted_sum_miss_rate(t: int, moves: int = 200_000, groups: int = 1000, seed: int = 9) -> float:
    """share of random moves d between two random groups of 0..groups-1 that both words miss, d a random non-zero
    multiple of 2^t below 2^32"""
    rng = np.random.default_rng(seed)
    w0, w1 = vm.weights(np.arange(groups, dtype=np.uint32))
    i = rng.integers(0, groups, moves)
    j = (i + rng.integers(1, groups, moves)) % groups
    d = (rng.integers(1, 1 << (32 - t), moves).astype(np.uint64) << np.uint64(t))
    with np.errstate(over="ignore"):
        m0 = (d * (w0[i] - w0[j])) & np.uint64(M32)
        m1 = (d * (w1[i] - w1[j])) & np.uint64(M32)
    return float(np.mean((m0 == 0) & (m1 == 0)))


def join_unsampled_share(n: int, hi: int) -> float:
    """share of the id positions inside probed ranges that no probe row's first / last / picked id reads, on
    gen_uniform(42, 1..hi) joined with gen_uniform(43, 1..hi), n rows each"""
    idx = np.arange(n, dtype=np.uint64)
    build, probe = vm.gen_value(42, 1, hi, idx), vm.gen_value(43, 1, hi, idx)
    srt = np.sort(build)
    lb, ub = np.searchsorted(srt, probe, "left"), np.searchsorted(srt, probe, "right")
    cnt = (ub - lb).astype(np.uint32)
    hit = cnt > 0
    probed = np.zeros(n + 1, dtype=np.int64)
    ulb, first = np.unique(lb[hit], return_index=True)
    np.add.at(probed, ulb, 1)
    np.add.at(probed, ub[hit][first], -1)
    probed = np.cumsum(probed)[:n] > 0
    read = np.zeros(n, dtype=bool)
    pick = vm.join_picks(cnt).astype(np.int64)
    for at in (lb[hit], ub[hit] - 1, lb[hit] + pick[hit]):
        read[at] = True
    return float(np.count_nonzero(probed & ~read) / np.count_nonzero(probed))


def test_the_measured_blind_spot_rates():
    """the figures DESIGN.md quotes, computed with the model and printed; asserted: only that the gaps are real and
    ordered as the arithmetic says (more trailing zero bits, more misses; 31 of them, all missed)"""
    rates = {t: weighted_sum_miss_rate(t) for t in (0, 24, 28, 30, 31)}
    shares = {(n, hi): join_unsampled_share(n, hi) for n, hi in ((1 << 16, 10000), (1 << 20, 10000), (1 << 16, 1 << 16))}
    print("weighted-sum miss rates by trailing zero bits:", rates)
    print("join id positions unread:", shares)
    assert rates[31] == 1.0 and rates[0] <= rates[24] <= rates[28] <= rates[30] < 1.0
    assert all(0.0 < s < 1.0 for s in shares.values())


# ---- one-to-many join ------------------------------------------------------------------------------------------------------
def _join_answer(rng, build, probe, shuffle):
    """a right (pos, cnt, ids): key ranges in a random order, ids in a random order inside a range when asked"""
    uk = np.unique(build)
    if shuffle:
        uk = rng.permutation(uk)
    ids, start = [], {}
    for key in uk:
        rows = np.nonzero(build == key)[0]
        start[int(key)] = len(ids)
        ids += (rng.permutation(rows) if shuffle else rows).tolist()
    cnt = np.array([np.count_nonzero(build == p) for p in probe], dtype=np.uint32)
    pos = np.array([start[int(p)] if c else 0 for p, c in zip(probe, cnt)], dtype=np.uint32)
    return pos, cnt, np.array(ids, dtype=np.uint32)


def _join_truth(build, probe, pos, cnt, ids, miss_pos_matters=True):
    n = build.size
    if sorted(ids.tolist()) != list(range(n)):
        return False
    carried = build[ids]
    if np.count_nonzero(carried[:-1] != carried[1:]) != max(np.unique(build).size - 1, 0):
        return False
    for p, at, c in zip(probe.tolist(), pos.tolist(), cnt.tolist()):
        rows = np.nonzero(build == p)[0].tolist()
        if c != len(rows):
            return False
        if c == 0 and at != 0 and miss_pos_matters:
            return False
        if c and (at + c > n or sorted(ids[at:at + c].tolist()) != rows):
            return False
    return True


def _join_verdict(build, probe, pos, cnt, ids):
    words = vm.join(np.sort(build), probe, pos, cnt, ids, build_keys=build)
    return vm.verdict_join(words, vm.permutation(ids))


def test_join_verdict_is_the_truth_but_for_the_position_of_a_miss():
    rng = np.random.default_rng(10)
    seen = {"right": 0, "caught": 0, "blind": 0}
    for trial in range(4000):
        nb, npr = int(rng.integers(1, 11)), int(rng.integers(1, 9))
        pool = rng.choice(np.array([1, 2, 3, 5, 8, 0xFFFFFFFE], dtype=np.uint32), int(rng.integers(1, 5)), replace=False)
        build = rng.choice(pool, nb)
        probe = rng.choice(np.append(pool, np.uint32([4, 9])), npr)
        pos, cnt, ids = _join_answer(rng, build, probe, shuffle=bool(rng.integers(2)))
        op = rng.integers(0, 9)
        i = int(rng.integers(npr))
        if op == 1 and nb >= 2:  # two ids swapped: inside a key's run (still right) or across keys, sampled or not
            a, b = rng.choice(nb, 2, replace=False)
            ids[[a, b]] = ids[[b, a]]
        elif op == 2:
            cnt[i] += np.uint32(rng.choice([1, M32]))
        elif op == 3:
            ids[rng.integers(nb)] = rng.choice([int(rng.integers(nb)), nb, M32])
        elif op == 4:
            pos[i] += np.uint32(rng.choice([1, M32, nb, M32 - 1]))
        elif op == 5:
            pos[i] = rng.choice([nb - 1, M32, 0])
        elif op == 6 and nb >= 3:  # a run cut in two by a rotation of the id buffer
            ids = np.roll(ids, int(rng.integers(1, nb)))
        elif op == 7:
            cnt[i] = 0
        elif op == 8:
            cnt[i], pos[i] = rng.integers(0, nb + 1), rng.integers(0, nb)
        truth = _join_truth(build, probe, pos, cnt, ids)
        verdict = _join_verdict(build, probe, pos, cnt, ids)
        if truth:
            assert verdict, (trial, op, build, probe, pos, cnt, ids)
            seen["right"] += 1
        elif verdict:  # family (b), and nothing else
            assert _join_truth(build, probe, pos, cnt, ids, miss_pos_matters=False), (trial, op, build, probe, pos, cnt, ids)
            seen["blind"] += 1
        else:
            seen["caught"] += 1
    assert seen["right"] > 300 and seen["caught"] > 1000 and seen["blind"] > 20


def test_join_word_alone_never_passes_a_bad_row():
    """ProbeHip and the partitioned join judge result[0] WITHOUT a permutation check on ids: the count of key runs must
    not be able to cancel a bad row, whatever ids holds.  Over ids that are no permutation (ids duplicated, lost, out of
    range, whole stretches overwritten) the word is 0 only if every per-row check passes and ids has as many key runs as
    the build column has keys; in ProbeHip's own shape (unique sorted keys, pos = row, cnt = 1) the verdict is the truth."""
    rng = np.random.default_rng(11)
    seen = {"bad rows": 0, "runs only": 0, "clean": 0}
    for trial in range(4000):
        nb, npr = int(rng.integers(2, 11)), int(rng.integers(1, 9))
        pool = rng.choice(np.array([1, 2, 3, 5, 8, 0xFFFFFFFE], dtype=np.uint32), int(rng.integers(1, 5)), replace=False)
        build = rng.choice(pool, nb)
        probe = rng.choice(np.append(pool, np.uint32([4, 9])), npr)
        pos, cnt, ids = _join_answer(rng, build, probe, shuffle=bool(rng.integers(2)))
        for _ in range(int(rng.integers(0, 4))):  # ids stops being a permutation
            op = rng.integers(0, 4)
            a = int(rng.integers(nb))
            if op == 0:
                ids[a] = ids[int(rng.integers(nb))]  # one id twice, one lost
            elif op == 1:
                ids[a] = rng.choice([nb, M32])
            elif op == 2:
                ids[a:] = ids[a]
            else:
                ids[:a] = ids[int(rng.integers(nb))]
        srt = np.sort(build)
        words = vm.join(srt, probe, pos, cnt, ids, build_keys=build)
        bad = int(np.count_nonzero(~vm.join_row_ok(srt, probe, pos, cnt, ids, build_keys=build)))
        up, down = vm.join_runs(srt, ids, build_keys=build)
        assert words[0] & M32 == bad and words[0] >> 32 == (up - down) % (1 << 32), (trial, words, bad, up, down)
        assert vm.verdict_pjoin_join(words) == (bad == 0 and up == down), (trial, build, probe, pos, cnt, ids)
        seen["bad rows" if bad else "runs only" if up != down else "clean"] += 1
    assert min(seen.values()) > 200, seen
    for n in (2, 5, 12):  # ProbeHip: every key probes itself
        keys = np.cumsum(rng.integers(1, 9, n)).astype(np.uint32)
        pos, cnt = np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.uint32)
        for trial in range(300):
            ids = np.arange(n, dtype=np.uint32)
            if trial:
                a, b = rng.integers(n, size=2)
                ids[a] = rng.choice([int(ids[b]), n, M32])
            words = vm.join(keys, keys, pos, cnt, ids, build_keys=keys)
            assert vm.verdict_probe(words, n) == np.array_equal(ids, np.arange(n)), (n, ids, words)
    # a duplicated id with the row that reads it: one bad row, one key run fewer; they must not cancel
    keys = np.arange(10, 18, dtype=np.uint32)
    ids = np.arange(8, dtype=np.uint32)
    ids[4] = ids[3]
    words = vm.join(keys, keys, np.arange(8, dtype=np.uint32), np.ones(8, np.uint32), ids, build_keys=keys)
    assert words == [1 + (((1 << 32) - 1) << 32), 8] and not vm.verdict_probe(words, 8) and not vm.verdict_pjoin_join(words)


def test_join_rows_alone_miss_what_the_runs_term_catches():
    """finding 1 restated on the model: two unsampled ids of different keys swapped pass every per-row check, the
    permutation check too, and only the count of key runs tells"""
    n, hi = 1 << 12, 100
    idx = np.arange(n, dtype=np.uint64)
    build, probe = vm.gen_value(42, 1, hi, idx), vm.gen_value(43, 1, hi, idx)
    ids = np.argsort(build, kind="stable").astype(np.uint32)
    srt = build[ids]
    lb = np.searchsorted(srt, probe, "left")
    cnt = (np.searchsorted(srt, probe, "right") - lb).astype(np.uint32)
    pos = np.where(cnt > 0, lb, 0).astype(np.uint32)
    read = np.zeros(n, dtype=bool)
    pick = vm.join_picks(cnt).astype(np.int64)
    for at in (lb, lb + cnt - 1, lb + pick):
        read[at[cnt > 0]] = True
    unread = np.nonzero(~read)[0]
    a = int(unread[0])
    b = int(unread[srt[unread] != srt[a]][0])
    bad = ids.copy()
    bad[[a, b]] = bad[[b, a]]
    assert vm.join(srt, probe, pos, cnt, ids, build_keys=build)[0] == 0
    assert bool(vm.join_row_ok(srt, probe, pos, cnt, bad, build_keys=build).all()) and vm.permutation(bad) == [0]
    up, down = vm.join_runs(srt, bad, build_keys=build)
    assert up > down and vm.join(srt, probe, pos, cnt, bad, build_keys=build)[0] == (up - down) << 32


# ---- pair table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left_outer", [False, True])
def test_join_pairs_verdict_is_the_truth(left_outer):
    rng = np.random.default_rng(12 + left_outer)
    seen = {True: 0, False: 0}
    for trial in range(3000):
        nb, npr = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        build = rng.choice(np.uint32([1, 2, 3]), nb)
        probe = rng.choice(np.uint32([1, 2, 3, 4]), npr)
        pos, cnt, ids = _join_answer(rng, build, probe, shuffle=True)
        want = [(int(ids[pos[p] + j]), p) for p in range(npr) for j in range(int(cnt[p]))]
        if left_outer:
            want += [(vm.SENTINEL, p) for p in range(npr) if cnt[p] == 0]
        out = [want[j] for j in rng.permutation(len(want))]  # any order is a right answer
        op = rng.integers(0, 6)
        if op == 1 and len(out) >= 2:  # a pair duplicated while another is dropped
            i, j = rng.choice(len(out), 2, replace=False)
            out[i] = out[j]
        elif op == 2 and out:
            out[rng.integers(len(out))] = (vm.SENTINEL, int(rng.integers(npr)))
        elif op == 3 and out:
            out[rng.integers(len(out))] = (int(rng.integers(nb)), int(rng.integers(npr)))
        elif op == 4 and out:
            out.pop()
        elif op == 5 and out:
            out[rng.integers(len(out))] = (int(rng.choice([nb, 0])), int(rng.choice([npr, M32])))
        ob = np.array([b for b, _ in out], dtype=np.uint32)
        op_ = np.array([p for _, p in out], dtype=np.uint32)
        truth = sorted(out) == sorted(want)
        words = vm.join_pairs(build, probe, ids, pos, cnt, ob, op_, left_outer=left_outer)
        assert vm.verdict_join_pairs(words, len(out)) == truth, (trial, op, out, want)
        seen[truth] += 1
    assert min(seen.values()) > 300


# ---- unique join, generator, routing, permutation, distinct ----------------------------------------------------------------
def test_ujoin_verdict_is_the_truth():
    rng = np.random.default_rng(14)
    seen = {True: 0, False: 0}
    for _ in range(3000):
        nb, npr = int(rng.integers(0, 9)), int(rng.integers(1, 9))
        bk = np.sort(rng.choice(np.uint32([0, 1, 5, 7, 9, 100, 0xFFFFFFFE, 0xFFFFFFFF]), nb, replace=False))
        bv = rng.integers(0, M32, nb).astype(np.uint32)
        pk = rng.choice(np.uint32([0, 1, 2, 5, 9, 0xFFFFFFFE, 0xFFFFFFFF]), npr)
        pv = rng.integers(0, M32, npr).astype(np.uint32)
        where = {int(k): j for j, k in enumerate(bk)}
        right = [(int(k), int(bv[where[int(k)]]), int(v)) if int(k) in where else (M32,) * 3 for k, v in zip(pk, pv)]
        out = [list(r) for r in right]
        if rng.integers(3):
            i = int(rng.integers(npr))
            op = rng.integers(0, 3)
            if op == 0:
                out[i][rng.integers(3)] ^= int(rng.choice([1, 1 << 31]))
            elif op == 1:
                out[i] = [M32] * 3
            else:
                out[i] = [int(pk[i]), 0, int(pv[i])]
        truth = [tuple(r) for r in out] == right
        cols = [np.array([r[c] for r in out], dtype=np.uint32) for c in range(3)]
        assert vm.verdict_ujoin(vm.ujoin(bk, bv, pk, pv, *cols)) == truth
        seen[truth] += 1
    assert min(seen.values()) > 300


def test_gen_route_permutation_and_distinct_count_exactly_what_is_wrong():
    rng = np.random.default_rng(15)
    from oracle import pyoracle as po
    for n, seed, lo, hi, first in ((0, 1, 0, 0, 0), (1, 2, 5, 5, 7), (300, 42, 1, 10000, (1 << 33) + 11), (300, 43, 0, M32, 5)):
        col = po.gen_uniform_u32(n, seed, lo, hi, first)
        assert vm.gen_uniform(col, seed, lo, hi, first) == [0]
        where = rng.permutation(n).astype(np.uint32)
        if first == 5:
            assert vm.gen_uniform(col[where], seed, lo, hi, indices=where + np.uint32(5)) == [0]
        if n > 1:
            bad = col.copy()
            at = rng.choice(n, 7, replace=False)
            bad[at] += np.uint32(1)
            assert vm.gen_uniform(bad, seed, lo, hi, first) == [7]
    keys = rng.integers(0, M32, 500).astype(np.uint32)
    for parts in (1, 3, 1024):
        dest = vm.dest_of(keys, parts)
        assert dest.min() >= 0 and dest.max() < parts
        assert sum(vm.pjoin_route(keys, parts, r)[0] for r in range(parts)) == keys.size * (parts - 1)
    for _ in range(300):
        n = int(rng.integers(1, 13))
        ids = rng.permutation(n).astype(np.uint32)
        if rng.integers(2):
            ids[rng.integers(n)] = rng.choice([int(rng.integers(n)), n, M32])
        assert vm.verdict_zero(vm.permutation(ids)) == (sorted(ids.tolist()) == list(range(n)))
        col = rng.choice(KEY_POOL, n)
        assert vm.verdict_zero(vm.distinct(col)) == (np.unique(col).size == n)
    assert vm.permutation(np.uint32([0, 0, 0, 5])) == [3]
