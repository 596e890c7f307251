// bloom_layout_check.cpp — dwarf_bench_amd/host/bloom_layout.hpp on the host, the text the kernels of bloom_filter.cpp run:
// it prints the word and the mask of a fixed set of keys (0, 1, the seed, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF and a seeded
// thousand) at n_words in {1, 2, 3, 64, 1000, 65537, 2^32 - 1} for two seeds, and bloom_words over a grid that includes the
// refusals; tests/test_bloom_layout_cpp.py compares every line with tests/bloom_model.py.  It checks on its own that every
// word lies inside the filter, that a mask has one to four bits, and that masks reach above bit 31.  Built with hipcc
// (dbhip_common.hpp holds fmix32); it makes no HIP call and needs no GPU.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "bloom_layout.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

int main() {
  const uint32_t seeds[] = {0u, 12345u};
  const uint64_t sizes[] = {1, 2, 3, 64, 1000, 65537, (1ull << 32) - 1};
  long high = 0, lines = 0;
  for (const uint32_t seed : seeds) {
    std::vector<uint32_t> keys = {0u, 1u, seed, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    std::mt19937 rng(seed + 7);
    for (int i = 0; i < 1000; ++i) keys.push_back(static_cast<uint32_t>(rng()));
    for (const uint64_t n_words : sizes) {
      for (const uint32_t k : keys) {
        const BloomPlace p = bloom_place(k, seed, static_cast<uint32_t>(n_words));
        REQUIRE(p.word < n_words);
        const int bits = __builtin_popcountll(p.mask);
        REQUIRE(bits >= 1 && bits <= 4);
        REQUIRE(p.word == bloom_word(bloom_hash(k, seed), static_cast<uint32_t>(n_words)) && p.mask == bloom_mask(bloom_hash(k, seed)));
        high += (p.mask >> 32) != 0;
        std::printf("P %" PRIu32 " %" PRIu64 " %" PRIu32 " %" PRIu32 " %" PRIu64 "\n", seed, n_words, k, p.word, p.mask);
        ++lines;
      }
    }
  }
  REQUIRE(high > lines / 2);  // (about 15 of 16 masks hold a bit above bit 31)
  const uint64_t counts[] = {0, 1, 3, 4, 5, 63, 64, 65, 1000, 1ull << 16, 1ull << 24, (1ull << 26) - 1, 1ull << 26, (1ull << 26) + 1,
                             (1ull << 32) - 1, 1ull << 32, (1ull << 35) - 1, 1ull << 35, (1ull << 38) - 1, 1ull << 38,
                             (1ull << 38) + 1, 1ull << 40, 1ull << 58, 1ull << 63, ~0ull};
  const unsigned bits[] = {0, 1, 2, 7, 8, 12, 16, 24, 63, 64, 65, 128, 1u << 16, ~0u};
  for (const uint64_t n : counts)
    for (const unsigned b : bits) std::printf("W %" PRIu64 " %u %" PRIu64 "\n", n, b, bloom_words(n, b));
  std::printf("bloom layout ok: %ld places\n", lines);
  return 0;
}
