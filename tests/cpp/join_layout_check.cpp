// CPU check of the join's partition geometry (dwarf_bench_amd/csrc/partition.hpp, join_common.hpp): every row count
// must give a geometry the kernels can run — at most 1024 level-0 buckets, a power-of-two level-1 fan-out of at most
// 1024, partitions that hold their expected rows, giant lists that fit the kernels' LDS list — and a meta array whose
// parts follow one another without overlap and fill exactly meta_bytes.  Built with hipcc (the header pulls in the HIP
// runtime header), runs without a GPU.  With arguments "n_side:n_build" (or "n" for n:n) it prints instead, per pair
// and rows per partition (the build's, then the radix join's), one line
//   n_side n_build rows parts k1 k2 variant t0 t1 counts0 cursors0 starts0 tile_starts0 counts1 starts1 cursors1 words
// — the geometry of n_build rows, the compiled plan (jl_side_plan) of a side of n_side rows partitioned by it, and the
// word offsets of its meta array — for the tests' restatement to be compared with.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "join_common.hpp"

using namespace dbhip;

static int bad = 0;
#define CHECK(c)                                                                                   \
  do {                                                                                             \
    if (!(c)) {                                                                                    \
      if (bad < 20) std::printf("FAILED %s at n = %zu rows_per_part = %zu\n", #c, n, rows);         \
      ++bad;                                                                                       \
    }                                                                                              \
  } while (0)

static void check(size_t n, size_t rows) {
  const JlLayout L = jl_layout(n, rows);
  CHECK(L.k1 >= 1 && L.k1 <= 1024);
  CHECK(L.k2 >= 1 && L.k2 <= 1024 && (L.k2 & (L.k2 - 1)) == 0 && L.k2 == (1u << L.log2_k2));
  CHECK(L.parts == L.k1 * L.k2 && L.parts <= (1u << 20) + 1024);
  CHECK(static_cast<size_t>(L.parts) * rows >= n || L.parts >= (1u << 20));  // a partition expects at most `rows` rows
  const size_t want = (n + rows - 1) / rows;
  CHECK(L.parts < 2 * (want ? want : 1) + 1024);                              // ... and not far fewer
  CHECK(L.k2 == 1 || L.parts > 1024);                                          // one level up to 1024 partitions
  CHECK(L.max_giants == jl_max_giants(n) && L.max_giants < kJlMaxGiantList);
  CHECK(L.total >= L.giant_off + jl_giant_bytes(L.max_giants) && L.giant_off >= L.meta_off + L.meta_bytes);
  // the meta array: seven arrays, each of the size the kernels index it with, one behind the other, meta_bytes in all
  const JlMeta m = jl_meta(L);
  const size_t g = static_cast<size_t>(kJlGroups) * L.k1;
  CHECK(m.counts0 == 0 && m.cursors0 == m.counts0 + g && m.starts0 == m.cursors0 + g);
  CHECK(m.tile_starts0 == m.starts0 + L.k1 + 1 && m.counts1 == m.tile_starts0 + L.k1 + 1);
  CHECK(m.starts1 == m.counts1 + L.parts && m.cursors1 == m.starts1 + L.parts + 1 && m.words == m.cursors1 + L.parts);
  CHECK(m.counts0 < m.cursors0 && m.cursors0 < m.starts0 && m.starts0 < m.tile_starts0 && m.tile_starts0 < m.counts1 &&
        m.counts1 < m.starts1 && m.starts1 < m.cursors1 && m.cursors1 < m.words);
  CHECK(m.bytes() == L.meta_bytes && m.bytes() == 8 * m.words);
  CHECK(jl_meta_starts(L) == (L.k2 > 1 ? m.starts1 : m.starts0));
  // level 0 alone (the stand-alone partitioner): the same first four arrays and nothing behind them
  const JlMeta m0 = jl_meta(L.k1, 0);
  CHECK(m0.cursors0 == m.cursors0 && m0.starts0 == m.starts0 && m0.tile_starts0 == m.tile_starts0 && m0.words == m.counts1);
}

static const char *variant_name(JlHist h) {
  switch (h) {
    case kJlHistOneLevel: return "one_level";
    case kJlHistPlain: return "plain";
    case kJlHistFused: return "fused";
    case kJlHistFused16: return "fused16";
    case kJlHistDigits: return "digits";
  }
  return "?";
}

int main(int argc, char **argv) {
  const size_t rows_options[2] = {kJlRowsPerPart, kJrRowsPerPart};
  if (argc > 1) {
    for (int i = 1; i < argc; ++i) {
      const size_t n_side = std::strtoull(argv[i], nullptr, 10);
      const char *colon = std::strchr(argv[i], ':');
      const size_t n_build = colon ? std::strtoull(colon + 1, nullptr, 10) : n_side;
      for (size_t rows : rows_options) {
        const JlLayout L = jl_layout(n_build, rows);
        const JlSidePlan plan = jl_side_plan(n_side, L);
        const JlMeta m = jl_meta(L);
        std::printf("%zu %zu %zu %u %u %u %s %d %d %zu %zu %zu %zu %zu %zu %zu %zu\n", n_side, n_build, rows, L.parts, L.k1, L.k2,
                    variant_name(plan.hist), plan.t0, plan.t1, m.counts0, m.cursors0, m.starts0, m.tile_starts0, m.counts1,
                    m.starts1, m.cursors1, m.words);
      }
    }
    return 0;
  }
  for (size_t rows : rows_options) {
    for (size_t n = 0; n < 70000; n += 17) check(n, rows);
    for (unsigned lg = 10; lg <= 31; ++lg)
      for (long d = -3; d <= 3; ++d)
        for (size_t mul : {2u, 3u, 5u, 7u}) {
          const size_t base = (static_cast<size_t>(mul) << lg) / 2;
          const size_t n = base + d > kJlMaxRows ? kJlMaxRows : base + d;
          check(n, rows);
        }
    unsigned long long x = 88172645463325252ull;  // xorshift: arbitrary sizes up to 2^31
    for (int i = 0; i < 200000; ++i) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      check(static_cast<size_t>(x % (kJlMaxRows + 1)), rows);
    }
  }
  for (unsigned a = 10; a <= 31; ++a)
    for (unsigned b = 10; b <= 31; ++b) {
      const size_t n = static_cast<size_t>(1) << a, rows = static_cast<size_t>(1) << b;
      CHECK(jr_max_giants(n, rows) < kJlMaxGiantList);
    }
  std::printf(bad ? "join layout: %d violations\n" : "join layout ok\n", bad);
  return bad ? 1 : 0;
}
