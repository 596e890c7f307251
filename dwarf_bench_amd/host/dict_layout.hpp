// dict_layout.hpp — the pieces of the dictionary (dict_encode.hpp, dict_encode.cpp) that compute an index or a size from
// data: the hash, the slot count, the regions of the workspace, and the two probe loops over a table of 8-byte slots.
// Plain functions for host and device behind one qualifier macro, templated on the table type (anything with
// operator[] that yields a DictSlot): the kernels run them on global and LDS pointers, tests/cpp/dict_layout_check.cpp
// runs the same text on the host over arrays that check every index.
//
// Table.  Open addressing, linear probing, a power-of-two number of slots of at least twice the capacity.  A slot is
// (key, code).  The CODE word says whether a slot is used, so all 2^32 key values are legal: DBENCH_DICT_EMPTY in an
// empty slot, DBENCH_DICT_PENDING from the insert until the key's rank is known, then the rank, which is below the
// capacity and so below 2^31.  A slot goes from empty to used once and its key never changes afterwards.
//
// Nothing here relies on the table's contents for the RANGE of what it returns: every index formed is (home + step) &
// mask with step < slots, whatever the slots hold, and every loop ends after `slots` steps.
#ifndef DBENCH_DICT_LAYOUT_HPP
#define DBENCH_DICT_LAYOUT_HPP

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBENCH_DICT_FN __host__ __device__ inline
#else
#define DBENCH_DICT_FN inline
#endif

#include "dict_encode.hpp" /* DBENCH_DICT_MISS, DBENCH_DICT_LDS_SLOTS */

#define DBENCH_DICT_EMPTY 0xFFFFFFFFu   /* code word of an empty slot */
#define DBENCH_DICT_PENDING 0xFFFFFFFEu /* code word of a used slot whose rank is not known yet */

struct alignas(8) DictSlot {
  uint32_t key, code;
};

// Murmur3's 32-bit finaliser; the home slot of a key is dict_hash(key) & (slots - 1)
DBENCH_DICT_FN uint32_t dict_hash(uint32_t key) {
  uint32_t h = key;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// the number of slots for a capacity in [1, 2^31): the smallest power of two >= 2 * capacity, so 2 .. 2^32
DBENCH_DICT_FN uint64_t dict_slots(uint64_t capacity) {
  uint64_t s = 2;
  while (s < 2 * capacity) s <<= 1;
  return s;
}

// the regions of the workspace, byte offsets from its start, each a multiple of 256.  sort_bytes is
// dbhip_radix_sort_workspace_bytes(capacity, 8): the inner sort's own workspace, whose first word is its status word.
//   [0, 256)        header (DictHeader of dict_encode.cpp: word 0 = status)
//   [table, keys)   8-byte slots
//   [keys, tmp)     capacity words: the distinct keys, padded, where the sort orders them
//   [tmp, sort)     capacity words: the sort's other column
//   [sort, total)   the sort's workspace
struct DictLayout {
  uint64_t slots, table, keys, tmp, sort, total;
};

DBENCH_DICT_FN uint64_t dict_align256(uint64_t x) { return (x + 255u) & ~static_cast<uint64_t>(255u); }

DBENCH_DICT_FN DictLayout dict_layout(uint64_t capacity, uint64_t sort_bytes) {
  DictLayout l;
  l.slots = dict_slots(capacity);
  l.table = 256;
  l.keys = l.table + dict_align256(8 * l.slots);
  l.tmp = l.keys + dict_align256(4 * capacity);
  l.sort = l.tmp + dict_align256(4 * capacity);
  l.total = l.sort + dict_align256(sort_bytes);
  return l;
}

// Lookup.  -> the code word of key's slot, or DBENCH_DICT_EMPTY if the key is not in the table (an empty slot ends the
// chain; so does a whole round of a full table).  Reads table[(home + step) & mask] for step < mask + 1 only.
// `home` is table[dict_hash(key) & mask] as the caller loaded it: a lane issues the home loads of all its keys before it
// looks at the first.
template <class Table>
DBENCH_DICT_FN uint32_t dict_find_after(const Table &table, uint32_t mask, uint32_t key, DictSlot home) {
  uint32_t s = dict_hash(key) & mask;
  DictSlot e = home;
  for (uint64_t step = 0;;) {
    if (e.code == DBENCH_DICT_EMPTY) return DBENCH_DICT_EMPTY;
    if (e.key == key) return e.code;
    if (++step > mask) return DBENCH_DICT_EMPTY;
    s = (s + 1) & mask;
    e = table[s];
  }
}

template <class Table>
DBENCH_DICT_FN uint32_t dict_find(const Table &table, uint32_t mask, uint32_t key) {
  return dict_find_after(table, mask, key, table[dict_hash(key) & mask]);
}

// -> the slot that holds key, or -1
template <class Table>
DBENCH_DICT_FN int64_t dict_find_slot(const Table &table, uint32_t mask, uint32_t key) {
  uint32_t s = dict_hash(key) & mask;
  for (uint64_t step = 0; step <= mask; ++step) {
    const DictSlot e = table[s];
    if (e.code == DBENCH_DICT_EMPTY) return -1;
    if (e.key == key) return static_cast<int64_t>(s);
    s = (s + 1) & mask;
  }
  return -1;
}

// Insert.  claim(s, key) tries to turn the empty slot s into (key, DBENCH_DICT_PENDING) and returns the slot as it was
// in front of the attempt: empty if this call claimed it, otherwise what another insert put there (a compare-and-swap on
// the device, a plain store on the host).  The slot is read before any claim, so a key that is already there costs one
// load.  -> 1 this call inserted the key, 0 it was there already, -1 the table is full and does not hold it.
template <class Table, class Claim>
DBENCH_DICT_FN int dict_insert(const Table &table, uint32_t mask, uint32_t key, Claim &&claim) {
  uint32_t s = dict_hash(key) & mask;
  for (uint64_t step = 0; step <= mask; ++step) {
    DictSlot e = table[s];
    if (e.code == DBENCH_DICT_EMPTY) {
      e = claim(s, key);
      if (e.code == DBENCH_DICT_EMPTY) return 1;
    }
    if (e.key == key) return 0;
    s = (s + 1) & mask;
  }
  return -1;
}

#endif
