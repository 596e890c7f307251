// quantile_layout_check.cpp — dwarf_bench_amd/host/quantile_layout.hpp on the host, the text qs_pick of quantile_select.cpp
// runs: it prints the rank every (q_num, q_den) names among m candidates (m in {0, 1, 2, 3, 2^32 - 1} and a few more; the
// fractions 0/1, 1/1, 1/2, 1/3, 999999999/10^9, a denominator of 2^32 - 1; the absolute ranks 0, m - 1, m, 2^32 - 1), the
// digits of a few words at every level, and for a handful of histograms — empty bins in front of, between and behind the
// hit — the bin that holds each rank; tests/test_quantile_layout_cpp.py compares every line with tests/quantile_model.py.
// It checks on its own that exactly one bin holds a rank inside the histogram and none a rank behind it.  Plain g++; no GPU.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "quantile_layout.hpp"

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

int main() {
  long lines = 0;
  const uint32_t top = 0xFFFFFFFFu;
  const uint32_t ms[] = {0u, 1u, 2u, 3u, 4u, 7u, 10u, 1000u, 65537u, 0x80000000u, top};
  const uint32_t fractions[][2] = {{0, 1}, {1, 1}, {1, 2}, {1, 3}, {2, 3}, {999999999u, 1000000000u}, {1, 1000000000u},
                                   {1, top}, {top - 1, top}, {top, top}, {0x80000000u, top}, {0, top}, {1, 10}, {9, 10}};
  for (const uint32_t m : ms) {
    for (const auto &f : fractions) {
      uint32_t r = 0;
      const bool live = qs_resolve_rank(f[0], f[1], m, &r);
      REQUIRE(!live || r < m);
      std::printf("R %" PRIu32 " %" PRIu32 " %" PRIu32 " %d %" PRIu32 "\n", f[0], f[1], m, live ? 1 : 0, live ? r : 0u);
      ++lines;
    }
    const uint32_t absolute[] = {0u, 1u, m - 1u, m, m + 1u, top};
    for (const uint32_t k : absolute) {
      uint32_t r = 0;
      const bool live = qs_resolve_rank(k, 0u, m, &r);
      REQUIRE(live == (k < m) && r == k);
      std::printf("R %" PRIu32 " 0 %" PRIu32 " %d %" PRIu32 "\n", k, m, live ? 1 : 0, live ? r : 0u);
      ++lines;
    }
  }
  const uint32_t words[] = {0u, 1u, 0x3FFu, 0x400u, 0x1FFFFFu, 0x200000u, 0x7FFFFFFFu, 0x80000000u, 0xDEADBEEFu, top};
  for (const uint32_t x : words) {
    uint32_t again = 0;
    for (int level = 0; level < DBENCH_QUANTILE_LEVELS; ++level) {
      const uint32_t d = qs_digit(x, level);
      REQUIRE(d < qs_radix(level) && qs_radix(level) <= DBENCH_QUANTILE_RADIX);
      REQUIRE((again & ~qs_high_mask(level)) == 0);  // the digits found so far are the bits above this one
      again |= d << qs_shift(level);
      std::printf("D %" PRIu32 " %d %" PRIu32 " %d %d %" PRIu32 "\n", x, level, d, qs_shift(level), qs_width(level),
                  qs_high_mask(level));
      ++lines;
    }
    REQUIRE(again == x);
  }
  // histograms: empty bins in front of, between and behind the bins that hold something
  const std::vector<std::vector<uint32_t>> hists = {
      {5}, {0, 0, 3, 0, 0, 0, 4, 1, 0, 0}, {1, 1, 1, 1}, {0, 0, 0, 0}, {0, 7}, {7, 0}, {2, 0, 0, 0, 0, 0, 0, 2},
      {0, 0, 0, top}, {0x80000000u, 0, 0x7FFFFFFFu, 0}, {0, 1, 0, 1, 0, 1, 0}};
  for (size_t h = 0; h < hists.size(); ++h) {
    const auto &bins = hists[h];
    uint64_t total = 0;
    std::printf("G %zu", h);
    for (const uint32_t c : bins) {
      std::printf(" %" PRIu32, c);
      total += c;
    }
    std::printf("\n");
    ++lines;
    std::vector<uint64_t> rems = {0, 1, 2, 3, 4, 5, 6, 7, 8, total / 2, total - 1, total, total + 1, 0x7FFFFFFFull, 0x80000000ull,
                                  0xFFFFFFFEull, 0xFFFFFFFFull};
    for (const uint64_t rem64 : rems) {
      if (rem64 > top) continue;
      const uint32_t rem = static_cast<uint32_t>(rem64);
      uint32_t before = 0;
      int hits = 0;
      long bin = -1;
      uint32_t at = 0;
      for (size_t d = 0; d < bins.size(); ++d) {
        if (qs_bin_holds(before, bins[d], rem)) {
          ++hits;
          bin = static_cast<long>(d);
          at = before;
        }
        before += bins[d];  // (the totals here stay below 2^32)
      }
      REQUIRE(hits == (rem < total ? 1 : 0));
      std::printf("B %zu %" PRIu32 " %ld %" PRIu32 "\n", h, rem, bin, at);
      ++lines;
    }
  }
  std::printf("quantile layout ok: %ld lines\n", lines);
  return 0;
}
