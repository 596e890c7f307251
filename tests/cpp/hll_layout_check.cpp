// hll_layout_check.cpp — dwarf_bench_amd/host/hll_layout.hpp on the host, the text the kernels of hll_sketch.cpp run: it prints
// the two hashes (h, g) of key tuples of 1 .. 4 columns (0, 1, the seed, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF and a seeded two
// hundred per column count) for two seeds, the register and the rank of given (h, g) at p in {4, 5, 11, 14} — w == 0, w with
// only its lowest valid bit set, w with bits only in its g half, the top bit set, and seeded words — and the estimate of a
// few histograms; tests/test_hll_layout_cpp.py compares every line with tests/hll_model.py.  It checks on its own that every
// register lies inside the sketch and every rank in 1 .. q+1.  Built with hipcc (dbhip_common.hpp holds fmix32); it makes no
// HIP call and needs no GPU.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hll_layout.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

int main() {
  const uint32_t seeds[] = {0u, 0xDEADBEEFu};
  long lines = 0;
  for (const uint32_t seed : seeds) {
    const uint32_t fixed[] = {0u, 1u, seed, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    std::mt19937 rng(seed + 7);
    for (int k = 1; k <= DBENCH_HLL_MAX_COLS; ++k) {
      for (int i = 0; i < 206; ++i) {
        uint32_t c[DBENCH_HLL_MAX_COLS] = {0, 0, 0, 0};
        for (int j = 0; j < k; ++j) c[j] = i < 6 ? fixed[(i + j) % 6] : static_cast<uint32_t>(rng());
        const HllHash s = hll_hash(c, k, seed);
        HllHash t = hll_hash_first(c[0], seed);
        for (int j = 1; j < k; ++j) t = hll_hash_next(t, c[j]);
        REQUIRE(s.h == t.h && s.g == t.g);
        std::printf("H %" PRIu32 " %d %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", seed, k, c[0],
                    c[1], c[2], c[3], s.h, s.g);
        ++lines;
      }
    }
  }
  const unsigned ps[] = {4, 5, 11, 14};
  for (const unsigned p : ps) {
    const unsigned q = 64 - p;
    std::vector<uint64_t> xs = {0ull, 1ull, 2ull, 0x80000000ull, 0xFFFFFFFFull, 1ull << 32, 1ull << (q - 1), 1ull << q,
                                (1ull << q) - 1, ~0ull, ~0ull << q, (~0ull << q) | 1ull, 0x00000001FFFFFFFFull};
    for (unsigned b = 0; b < 64; ++b) xs.push_back(1ull << b);
    std::mt19937_64 rng(p);
    for (int i = 0; i < 300; ++i) xs.push_back(rng() >> (rng() & 63));
    for (const uint64_t x : xs) {
      const uint32_t h = static_cast<uint32_t>(x >> 32), g = static_cast<uint32_t>(x);
      const HllPlace at = hll_place(h, g, p);
      REQUIRE(at.idx < (1u << p) && at.rank >= 1 && at.rank <= q + 1);
      std::printf("P %u %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", p, h, g, at.idx, at.rank);
      ++lines;
    }
  }
  // the estimate: the empty sketch, every register saturated, every register 1, a spread, and two refusals
  for (const unsigned p : ps) {
    const uint32_t m = 1u << p, q = 64 - p;
    uint32_t hist[DBENCH_HLL_HIST_WORDS] = {};
    hist[0] = m;
    REQUIRE(hll_estimate(hist, p) == 0.0);
    std::printf("E %u empty %.17g\n", p, hll_estimate(hist, p));
    hist[0] = 0, hist[q + 1] = m;
    std::printf("E %u saturated %.17g\n", p, hll_estimate(hist, p));
    hist[q + 1] = 0, hist[1] = m;
    std::printf("E %u ones %.17g\n", p, hll_estimate(hist, p));
    hist[1] = m / 2, hist[2] = m / 4, hist[0] = m / 8, hist[7] = m / 8;
    std::printf("E %u spread %.17g\n", p, hll_estimate(hist, p));
    hist[7] += 1;
    REQUIRE(hll_estimate(hist, p) == -1.0);
    hist[7] -= 1, hist[0] -= 1, hist[q + 2] = 1;
    REQUIRE(hll_estimate(hist, p) == -1.0);
  }
  uint32_t hist[DBENCH_HLL_HIST_WORDS] = {8};
  REQUIRE(hll_estimate(hist, 3) == -1.0 && hll_estimate(hist, 15) == -1.0 && hll_estimate(nullptr, 4) == -1.0);
  std::printf("hll layout ok: %ld lines\n", lines);
  return 0;
}
