"""Test-only inputs for the merge-path tests (tests/test_merge_model.py on the CPU, tests/test_gpu_merge.py on the GPU):
the (na, nb) sizes at the kernels' edges, the key patterns, and the pairs of strictly ascending lists for the set
operations.  Sizes come from T = DBENCH_MERGE_TILE_ROWS.  Never imported by the product."""
import numpy as np

from tests import merge_model as mm


def sizes(T):
    """nothing and one, a tile on one side, a tile split every way, just over, many ragged tiles against one row"""
    return [(0, 0), (0, 1), (1, 0), (1, 1), (0, T), (T, 0), (T - 1, 1), (T // 2, T // 2), (T, T), (T + 1, T - 1),
            (3 * T + 5, 1), (1, 3 * T + 5), (100003, 50021)]


def second_round(T):
    """1025 T + 3 merged rows: 1026 tiles, the scan kernel's 256 threads take 1024 counts a round"""
    return (513 * T + 3, 512 * T)


def sort_as(keys, signed):
    return keys[np.argsort(mm.order(keys, signed), kind="stable")]


EDGES = np.array([0, 0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000000, 0x80000001, 0xFFFFFFFE,
                  0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)


def key_patterns(na, nb, rng, signed=False):
    """name, a_keys, b_keys: ascending in the order of `signed`"""
    def u32(x):
        return np.asarray(x, dtype=np.uint64).astype(np.uint32)

    def asc(x):
        return sort_as(u32(x), signed)

    yield "uniform", asc(rng.integers(0, 1 << 32, na, dtype=np.uint64)), asc(rng.integers(0, 1 << 32, nb, dtype=np.uint64))
    # as unsigned values below 2^31, where both orders agree
    yield "a below b", u32(np.arange(na)), u32(na + np.arange(nb))
    yield "b below a", u32(nb + np.arange(na)), u32(np.arange(nb))
    yield "interleaved", u32(2 * np.arange(na)), u32(2 * np.arange(nb) + 1)
    yield "all equal", np.full(na, 7, dtype=np.uint32), np.full(nb, 7, dtype=np.uint32)
    yield "long runs", u32(np.arange(na) // 1000), u32(np.arange(nb) // 1000)
    yield "one a key inside b", np.full(na, nb // 2, dtype=np.uint32), u32(np.arange(nb))
    edges_a = EDGES[rng.integers(0, EDGES.size, na)] if na else EDGES[:0]
    edges_b = EDGES[rng.integers(0, EDGES.size, nb)] if nb else EDGES[:0]
    yield "edges of both orders", asc(edges_a), asc(edges_b)


def straddling(T, k_tiles=3):
    """two strictly ascending lists whose partner pairs (equal values, A's then B's) fall on merged positions k T - 1 and
    k T for k = 1 .. k_tiles: in front of every such pair an odd number of unpartnered elements.  -> a, b"""
    a, b, value, merged = [], [], 0, 0
    for k in range(1, k_tiles + 1):
        while merged < k * T - 1:  # singles, alternating sides, up to position k T - 2
            (a if (value % 3) else b).append(value)
            value += 1
            merged += 1
        a.append(value), b.append(value)  # positions k T - 1 (A's) and k T (B's)
        value += 1
        merged += 2
    for _ in range(T // 3):
        (a if (value % 2) else b).append(value)
        value += 1
    return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)


def pairs_on_tile_edges(a, b, T):
    """the k for which the merged order of a and b has a partner pair on positions k T - 1 and k T"""
    keys, _, _, _ = mm.merge(a, b)
    same = np.flatnonzero(keys[1:] == keys[:-1])  # position of the pair's first element
    return [int(p + 1) // T for p in same if (p + 1) % T == 0]


def set_cases(n, rng):
    """name, a, b: strictly ascending uint32 lists of about n entries"""
    def pick(universe, k):
        return np.sort(rng.choice(universe, k, replace=False)).astype(np.uint32)

    base = pick(4 * n + 8, n)
    yield "a equals b", base, base.copy()
    yield "disjoint interleaved", (2 * np.arange(n)).astype(np.uint32), (2 * np.arange(n) + 1).astype(np.uint32)
    yield "disjoint ranges", np.arange(n, dtype=np.uint32), (n + np.arange(n)).astype(np.uint32)
    yield "a inside b", base[rng.random(n) < 0.3], base
    yield "b inside a", base, base[rng.random(n) < 0.3]
    yield "a empty", base[:0], base
    yield "b empty", base, base[:0]
    for share in (0.01, 0.5, 0.99):
        common = base[rng.random(n) < share]
        rest = np.setdiff1d(np.arange(4 * n + 8, 8 * n + 16, dtype=np.uint32), base)
        own_a, own_b = pick(rest[: rest.size // 2], n - common.size), pick(rest[rest.size // 2:], n - common.size)
        yield f"{share:.0%} overlap", np.union1d(common, own_a).astype(np.uint32), np.union1d(common, own_b).astype(np.uint32)
    top = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    yield "ends of the range", top[[0, 2, 3, 5]], top[[1, 2, 3, 4, 5]]
