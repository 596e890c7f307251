// bloom_layout.hpp — the pieces of the Bloom filter (bloom_filter.hpp, bloom_filter.cpp) that compute a size, a word index
// or a bit mask from integers: the sizing query and the placement of a key.  Plain functions for host and device behind one
// qualifier macro: the kernels run them on the GPU, tests/cpp/bloom_layout_check.cpp runs the same text on the host and
// prints what it gives, tests/bloom_model.py is the numpy form of it.
//
// Format.  A filter is n_words little-endian uint64 words, 1 <= n_words < 2^32, any n_words (no power of two needed).  A key
// k (any 32-bit pattern) owns ONE word and up to four bits in it:
//   h    = fmix32(k ^ seed)                       (csrc/dbhip_common.hpp)
//   word = (uint64(h) * n_words) >> 32            the high half of a 32 x 32 bit product: < n_words, no division
//   g    = fmix32(h ^ 0x9E3779B9)
//   mask = OR over j = 0..3 of 1ull << ((g >> 6 j) & 63)        positions may coincide
// Every shift of a bit is a 64-bit shift: positions 32 .. 63 are as likely as 0 .. 31.
#ifndef DBENCH_BLOOM_LAYOUT_HPP
#define DBENCH_BLOOM_LAYOUT_HPP

#include <stddef.h>
#include <stdint.h>

#include "dbhip_common.hpp" /* fmix32 */

#define DBENCH_BLOOM_FN __host__ __device__ inline

// the words of a filter for n_keys keys at bits_per_key bits each: max(1, ceil(n_keys * bits_per_key / 64)); 0 for
// bits_per_key outside 1 .. 64 or a result of 2^32 or more (no such filter)
DBENCH_BLOOM_FN uint64_t bloom_words(uint64_t n_keys, unsigned bits_per_key) {
  if (bits_per_key < 1 || bits_per_key > 64) return 0;
  if (n_keys >= (1ull << 38)) return 0;  // at one bit per key already 2^32 words; below it the product stays under 2^44
  const uint64_t words = (n_keys * bits_per_key + 63) >> 6;
  if (words >= (1ull << 32)) return 0;
  return words ? words : 1;
}

DBENCH_BLOOM_FN uint32_t bloom_hash(uint32_t key, uint32_t seed) { return dbhip::fmix32(key ^ seed); }

// the word of a key with hash h: < n_words for every h
DBENCH_BLOOM_FN uint32_t bloom_word(uint32_t h, uint32_t n_words) {
  return static_cast<uint32_t>((static_cast<uint64_t>(h) * n_words) >> 32);
}

// its up to four bits
DBENCH_BLOOM_FN uint64_t bloom_mask(uint32_t h) {
  const uint32_t g = dbhip::fmix32(h ^ 0x9E3779B9u);
  uint64_t mask = 0;
  for (int j = 0; j < 4; ++j) mask |= 1ull << ((g >> (6 * j)) & 63u);
  return mask;
}

struct BloomPlace {
  uint32_t word;
  uint64_t mask;
};

DBENCH_BLOOM_FN BloomPlace bloom_place(uint32_t key, uint32_t seed, uint32_t n_words) {
  const uint32_t h = bloom_hash(key, seed);
  return BloomPlace{bloom_word(h, n_words), bloom_mask(h)};
}

#endif
