// merge_path_check.cpp — dwarf_bench_amd/host/merge_path.hpp on the host, the text the kernels of merge_sorted.cpp run:
// every pair of sizes in [0, 9] x [0, 9] with a tile of 4 and threads of 3 items, random sizes against std::merge, and
// shuffled (unsorted) inputs.  Every column is a Checked array that aborts on an index outside it; on every tile the
// extents must lie inside the inputs and add up to the tile, and of sorted inputs the tiles laid end to end must be
// std::merge's output with A first on ties.  No GPU, no HIP: plain C++ (built by tests/test_merge_path_cpp.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "merge_path.hpp"

namespace {

long g_reads = 0;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// a column that sees every index used on it.  The storage is exactly n words, so an index that slipped past the
// check would also be a heap overflow for a sanitizer to see
struct Checked {
  std::vector<uint32_t> data;
  unsigned first = 0, n = 0;  // the window [first, first + n) an accessor is entitled to (a tile's part in LDS)
  Checked window(unsigned from, unsigned count) const {
    REQUIRE(from <= n && count <= n - from);
    Checked w;
    w.data.assign(data.begin() + first + from, data.begin() + first + from + count);
    w.n = count;
    return w;
  }
  uint32_t operator[](unsigned i) const {
    REQUIRE(i < n);
    ++g_reads;
    return data[first + i];
  }
};

Checked column(const std::vector<uint32_t> &v) {
  Checked c;
  c.data = v;
  c.n = static_cast<unsigned>(v.size());
  return c;
}

struct Tagged {
  uint32_t key;
  int source;  // 0 = A, 1 = B
  unsigned row;
  bool operator==(const Tagged &o) const { return key == o.key && source == o.source && row == o.row; }
};

// the kernels' path on the host: partition points per tile boundary, clamped extents, a window per tile (the LDS
// image), a diagonal search and a serial merge of kItems per thread.  -> the merged elements in output order
template <int kItems>
std::vector<Tagged> run(const std::vector<uint32_t> &va, const std::vector<uint32_t> &vb, unsigned tile, unsigned flip,
                        bool sorted) {
  const Checked a = column(va), b = column(vb);
  const unsigned na = a.n, nb = b.n, total = na + nb;
  const unsigned tiles = (total + tile - 1) / tile;
  std::vector<unsigned> part(tiles + 1);
  for (unsigned i = 0; i <= tiles; ++i) {
    const unsigned d = std::min(i * tile, total);
    part[i] = mp_diagonal(a, na, b, nb, d, flip);
    REQUIRE(part[i] <= std::min(d, na) && d - part[i] <= nb);
    if (sorted && i) REQUIRE(part[i] >= part[i - 1] && part[i] - part[i - 1] <= tile);
  }
  std::vector<Tagged> out;
  for (unsigned t = 0; t < tiles; ++t) {
    const unsigned d0 = t * tile, d1 = std::min(d0 + tile, total);
    const MpTile e = mp_tile_extents(part[t], part[t + 1], d0, d1, na, nb);
    REQUIRE(e.a0 <= na && e.an <= na - e.a0);
    REQUIRE(e.b0 <= nb && e.bn <= nb - e.b0);
    REQUIRE(e.an + e.bn == d1 - d0);  // the extents sum to the tile
    if (sorted) REQUIRE(e.a0 == part[t] && e.an == part[t + 1] - part[t] && e.b0 == d0 - part[t]);
    const Checked sa = a.window(e.a0, e.an), sb = b.window(e.b0, e.bn);
    const unsigned count = d1 - d0;
    unsigned emitted = 0;
    for (unsigned first = 0; first < std::max(count, 1u); first += kItems) {  // one "thread" per kItems positions
      const unsigned d = std::min(first, count), items = std::min<unsigned>(kItems, count - d);
      const unsigned ai = mp_diagonal(sa, e.an, sb, e.bn, d, flip);
      REQUIRE(ai <= e.an && d - ai <= e.bn);
      unsigned next = 0;
      mp_serial_merge<kItems>(sa, ai, e.an, sb, d - ai, e.bn, flip, items,
                              [&](int k, bool from_a, unsigned i, unsigned j, uint32_t key) {
                                REQUIRE(static_cast<unsigned>(k) == next && next < items);
                                ++next;
                                REQUIRE(from_a ? i < e.an : j < e.bn);
                                REQUIRE(i <= e.an && j <= e.bn);  // the cursors the set operations index the halo with
                                REQUIRE(key == (from_a ? sa.data[i] : sb.data[j]));
                                out.push_back({key, from_a ? 0 : 1, from_a ? e.a0 + i : e.b0 + j});
                              });
      if (sorted) REQUIRE(next == items);
      REQUIRE(next <= items);
      emitted += next;
    }
    REQUIRE(emitted <= count);
    if (sorted) REQUIRE(emitted == count);
  }
  REQUIRE(out.size() <= total);
  return out;
}

std::vector<Tagged> expected(const std::vector<uint32_t> &va, const std::vector<uint32_t> &vb, unsigned flip) {
  std::vector<Tagged> ta, tb, out;
  for (unsigned i = 0; i < va.size(); ++i) ta.push_back({va[i], 0, i});
  for (unsigned i = 0; i < vb.size(); ++i) tb.push_back({vb[i], 1, i});
  // std::merge is stable: of equivalent elements those of the first range come first
  std::merge(ta.begin(), ta.end(), tb.begin(), tb.end(), std::back_inserter(out),
             [flip](const Tagged &x, const Tagged &y) { return (x.key ^ flip) < (y.key ^ flip); });
  return out;
}

std::vector<uint32_t> draw(std::mt19937 &rng, unsigned n, uint32_t span, unsigned flip, bool sorted) {
  std::vector<uint32_t> v(n);
  for (auto &x : v) x = span ? static_cast<uint32_t>(rng() % span) : static_cast<uint32_t>(rng());
  if (sorted) std::sort(v.begin(), v.end(), [flip](uint32_t x, uint32_t y) { return (x ^ flip) < (y ^ flip); });
  return v;
}

template <int kItems>
void both_ways(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, unsigned tile, unsigned flip, bool sorted) {
  const std::vector<Tagged> got = run<kItems>(a, b, tile, flip, sorted);
  if (sorted) REQUIRE(got == expected(a, b, flip));
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  long cases = 0;
  // every pair of sizes in [0, 9] x [0, 9], tile 4, over key spans that give no, some and only ties
  for (unsigned na = 0; na <= 9; ++na)
    for (unsigned nb = 0; nb <= 9; ++nb)
      for (uint32_t span : {1u, 3u, 1000u, 0u})
        for (unsigned flip : {0u, 0x80000000u})
          for (int rep = 0; rep < 4; ++rep)
            for (bool sorted : {true, false}) {
              const auto a = draw(rng, na, span, flip, sorted), b = draw(rng, nb, span, flip, sorted);
              both_ways<3>(a, b, 4, flip, sorted);
              both_ways<1>(a, b, 4, flip, sorted);
              both_ways<8>(a, b, 4, flip, sorted);  // more items than the tile has
              ++cases;
            }
  // random sizes against std::merge, tiles of several sizes; and shuffled inputs
  for (int rep = 0; rep < 300; ++rep) {
    const unsigned na = rng() % 700, nb = rep % 7 == 0 ? rng() % 5 : rng() % 700;
    const uint32_t span = (rep % 3 == 0) ? 0u : (rep % 3 == 1 ? 50u : 5000u);
    const unsigned flip = (rep & 1) ? 0x80000000u : 0u;
    const unsigned tile = std::vector<unsigned>{4, 16, 64, 256}[rep % 4];
    for (bool sorted : {true, false}) {
      const auto a = draw(rng, na, span, flip, sorted), b = draw(rng, nb, span, flip, sorted);
      both_ways<8>(a, b, tile, flip, sorted);
      both_ways<3>(b, a, tile, flip, sorted);
      ++cases;
    }
  }
  // stored partition points that are anything at all: the extents still lie inside and sum to the tile
  for (int rep = 0; rep < 200000; ++rep) {
    const unsigned na = rng() % 40, nb = rng() % 40, total = na + nb;
    const unsigned d0 = static_cast<unsigned>(rng() % (total + 1));
    const unsigned d1 = std::min(total, d0 + static_cast<unsigned>(rng() % 9));
    const unsigned lo = rep % 5 == 0 ? static_cast<unsigned>(rng()) : rng() % 50, hi = rep % 7 == 0 ? static_cast<unsigned>(rng()) : rng() % 50;
    const MpTile e = mp_tile_extents(lo, hi, d0, d1, na, nb);
    REQUIRE(e.a0 <= na && e.an <= na - e.a0 && e.b0 <= nb && e.bn <= nb - e.b0 && e.an + e.bn == d1 - d0);
  }
  std::printf("merge path ok: %ld cases, %ld checked reads\n", cases, g_reads);
  return 0;
}
