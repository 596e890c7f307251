"""Python model of the reference's slab table (common/dpcpp/slab_hash.hpp) run sequentially: the slab, slot and chain
layout that a serial insert (dbhip_slab_table_insert_u32 with serial != 0) must reproduce, and find()'s answers.

Node b < buckets is bucket b's root slab (the reference allocates it lazily from the heap, :144-152); overflow nodes
are taken from the pool in order.  Insert (:154-175, :224-262): the first empty slot, in ascending slot order, of the
first slab of the chain that has one; a new slab at the chain's end when all are full.  Find (:177-196, :264-294): the
first slot in chain and slot order that holds the key."""
from __future__ import annotations

import numpy as np

EMPTY_KEY = 0xFFFFFFFF
NONE = 0xFFFFFFFF
SLAB = 32
U64 = (1 << 64) - 1


def slab_hash(k: int, a: int, b: int, p: int, buckets: int) -> int:
    """DefaultHasher<A, B, P> (slab_hash.hpp:60-64) in exact integer arithmetic"""
    return ((a * k + b) % p) % buckets


def barrett_constant(d: int) -> int:
    """the multiplier csrc/slab.hip computes on the host for x % d: floor((2^64 - 1) / d)"""
    return U64 // d


def barrett_rem(x: int, d: int) -> int:
    """csrc/slab.hip sl_rem, step by step in 64-bit arithmetic: q = mulhi(x, m), r = x - q*d, two conditional
    subtractions"""
    m = barrett_constant(d)
    q = (x * m) >> 64
    r = (x - q * d) & U64
    if r >= d:
        r -= d
    if r >= d:
        r -= d
    return r


def device_hash(k: int, a: int, b: int, p: int, buckets: int) -> int:
    """the kernel's bucket: sl_rem(sl_rem(a*k + b, p), buckets) with a*k + b in 64 bits"""
    x = (a * k + b) & U64
    return barrett_rem(barrett_rem(x, p), buckets)


def barrett_rem_np(x: np.ndarray, d: int) -> np.ndarray:
    """barrett_rem over a uint64 array (mulhi by 32-bit halves, as __umul64hi does)"""
    x = x.astype(np.uint64)
    m = np.uint64(barrett_constant(d))
    lo32 = np.uint64(0xFFFFFFFF)
    x_lo, x_hi = x & lo32, x >> np.uint64(32)
    m_lo, m_hi = m & lo32, m >> np.uint64(32)
    t = x_lo * m_lo
    mid1 = x_hi * m_lo + (t >> np.uint64(32))
    mid2 = x_lo * m_hi + (mid1 & lo32)
    q = x_hi * m_hi + (mid1 >> np.uint64(32)) + (mid2 >> np.uint64(32))
    r = x - q * np.uint64(d)
    dd = np.uint64(d)
    r = np.where(r >= dd, r - dd, r)
    return np.where(r >= dd, r - dd, r)


class SlabModel:
    def __init__(self, buckets: int, pool_nodes: int, hasher):
        self.buckets, self.pool = buckets, pool_nodes
        self.a, self.b, self.p = hasher
        nodes = buckets + pool_nodes
        self.keys = [[EMPTY_KEY] * SLAB for _ in range(nodes)]
        self.vals = [[0] * SLAB for _ in range(nodes)]
        self.next = [NONE] * nodes
        self.used = 0

    def bucket(self, k: int) -> int:
        return slab_hash(k, self.a, self.b, self.p, self.buckets)

    def insert(self, k: int, v: int) -> bool:
        if k == EMPTY_KEY:
            return False
        node = self.bucket(k)
        while True:
            row = self.keys[node]
            if EMPTY_KEY in row:
                s = row.index(EMPTY_KEY)
                row[s], self.vals[node][s] = k, v
                return True
            if self.next[node] == NONE:
                if self.used >= self.pool:
                    return False  # the pool is exhausted: the row is not stored
                self.next[node] = self.buckets + self.used
                self.used += 1
            node = self.next[node]

    def find(self, k: int):
        """(value, True) of the first slot in chain order holding k, else (None, False)"""
        if k == EMPTY_KEY:
            return None, False
        node = self.bucket(k)
        while node != NONE:
            if k in self.keys[node]:
                return self.vals[node][self.keys[node].index(k)], True
            node = self.next[node]
        return None, False

    def chain(self, bucket: int):
        out, node = [], bucket
        while node != NONE:
            out.append(node)
            node = self.next[node]
        return out

    def export(self):
        """(keys [nodes, 32], vals [nodes, 32], next [nodes], pool_used) as uint32 arrays, the layout of
        dbhip_slab_table_export_u32"""
        return (np.array(self.keys, dtype=np.uint32), np.array(self.vals, dtype=np.uint32),
                np.array(self.next, dtype=np.uint32), self.used)

    def root_layout(self):
        """{bucket: [[slot, key, value], ...]} of the filled slots of every root slab"""
        return {b: [[s, self.keys[b][s], self.vals[b][s]] for s in range(SLAB) if self.keys[b][s] != EMPTY_KEY]
                for b in range(self.buckets) if self.keys[b][0] != EMPTY_KEY}
