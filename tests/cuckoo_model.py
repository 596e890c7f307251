"""Test-only model of the reference's cuckoo table (common/dpcpp/cuckoo_hashtable.hpp of dwarf_bench): insert() and
at() restated in Python, one work-item, input order.  tests/test_cuckoo_host.py pins it to the reference tests' own
assertions (tests/golden/cuckoo_kats.json); tests/test_gpu_cuckoo.py compares the device's serial mode with it.  Never
imported by the product."""
EMPTY_KEY = 0xFFFFFFFF


class CuckooModel:
    def __init__(self, size: int, hash_kind: int, seeds, murmur=None):
        """hash_kind 0: (k % size + seed) % size; 1: murmur(k, seed) % size (pass po.murmur3_x86_32);
        2: (mix64(seed, k) >> 32) % size"""
        self.size, self.kind, self.seeds, self.murmur = size, hash_kind, tuple(seeds), murmur
        self.keys = [EMPTY_KEY] * size
        self.vals = [0] * size

    def _h(self, k: int, seed: int) -> int:
        if self.kind == 0:
            return (k % self.size + seed) % self.size
        if self.kind == 1:
            return self.murmur(k, seed) % self.size
        return int(mix64_np(seed, [k])[0] >> 32) % self.size

    def h1(self, k: int) -> int:
        return self._h(k, self.seeds[0])

    def h2(self, k: int) -> int:
        return self._h(k, self.seeds[1])

    def insert(self, key: int, val: int, max_iter: int) -> bool:
        """cuckoo_hashtable.hpp:43-63 (the lock and unlock do nothing on one work-item)"""
        pos = self.h1(key)
        for _ in range(max_iter):
            if self.keys[pos] == EMPTY_KEY:
                self.keys[pos], self.vals[pos] = key, val
                return True
            key, self.keys[pos] = self.keys[pos], key
            val, self.vals[pos] = self.vals[pos], val
            pos = self.h2(key) if pos == self.h1(key) else self.h1(key)
        return False

    def at(self, key: int):
        """cuckoo_hashtable.hpp:29-37: (value, True) from the h1 slot, else from the h2 slot, else (None, False)"""
        for p in (self.h1(key), self.h2(key)):
            if self.keys[p] == key:
                return self.vals[p], True
        return None, False

    def layout(self) -> dict:
        return {i: (k, v) for i, (k, v) in enumerate(zip(self.keys, self.vals)) if k != EMPTY_KEY}


def murmur3_x86_32_np(keys, seed: int):
    """MurmurHash3_x86_32 of 4-byte keys (hashfunctions.hpp:64-130, _len = 4), vectorised over a numpy uint32 array;
    tests/test_cuckoo_host.py pins it to the oracle's scalar po.murmur3_x86_32"""
    import numpy as np
    m = np.uint64(0xFFFFFFFF)

    def rotl(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m

    k = np.asarray(keys, dtype=np.uint64)
    k = (k * np.uint64(0xcc9e2d51)) & m
    k = (rotl(k, 15) * np.uint64(0x1b873593)) & m
    h = np.uint64(seed & 0xFFFFFFFF) ^ k
    h = (rotl(h, 13) * np.uint64(5) + np.uint64(0xe6546b64)) & m
    h ^= np.uint64(4)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def mix64_np(seed: int, keys):
    """dbhip mix64 (csrc/dbhip_common.hpp, oracle dbo_mix64) over a numpy array of indices, as uint64"""
    import numpy as np
    with np.errstate(over="ignore"):
        z = (np.asarray(keys, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) \
            + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def positions_np(keys, hash_kind: int, seed: int, size: int):
    """h(k) of the device's hasher `hash_kind` (1 or 2) over a numpy uint32 array"""
    import numpy as np
    if hash_kind == 1:
        return (murmur3_x86_32_np(keys, seed) % np.uint32(size)).astype(np.int64)
    return ((mix64_np(seed, keys) >> np.uint64(32)) % np.uint64(size)).astype(np.int64)
