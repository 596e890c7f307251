// bitpack_layout_check.cpp — dwarf_bench_amd/host/bitpack_layout.hpp on the host, the text the kernels of bitpack.cpp run:
// the word count, the bit position, the insert of groups of 32 codes and the extract of every row, for every width 1..32
// and every row count 0..300, against a reference that moves one bit at a time; the extract on a fake column of up to
// 2^32 - 1 rows whose words are a function of their index (64-bit bit positions; the last word read lies inside
// ceil(n_rows * width / 32)); the extract through an origin, as the kernels use it on a staged piece; and the workspace
// regions.  The file named on the command line (optional) lists answers of the exported queries — "W n_rows width words"
// and "S capacity bytes" lines, written by tests/test_bitpack_layout_cpp.py — which must equal this header's.  Every
// array aborts on an index outside it and is stored at exactly its stated size.  No GPU, no HIP: plain C++.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "bitpack_layout.hpp"

namespace {

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

long g_reads = 0;

// words that see every index used on them; the storage is exactly the stated size
struct Checked {
  std::vector<uint32_t> *data;
  uint32_t operator[](uint64_t w) const {
    REQUIRE(w < data->size());
    ++g_reads;
    return (*data)[w];
  }
};

struct CheckedOut {
  std::vector<uint32_t> *data;
  uint32_t &operator[](uint64_t w) {
    REQUIRE(w < data->size());
    return (*data)[w];
  }
};

// a group's 32 codes out of a column of n codes: rows behind the last are the zero tail
struct GroupCodes {
  const std::vector<uint32_t> *codes;
  uint64_t first;
  uint32_t operator[](unsigned r) const {
    REQUIRE(r < 32);
    ++g_reads;
    return first + r < codes->size() ? (*codes)[first + r] : 0u;
  }
};

uint64_t plain_words(uint64_t n, unsigned width) { return ((n * width + 31) / 32 + 3) / 4 * 4; }

// one bit at a time: code i's bit k is bit i * width + k of the stream
std::vector<uint32_t> reference_pack(const std::vector<uint32_t> &codes, unsigned width) {
  std::vector<uint32_t> words(plain_words(codes.size(), width), 0u);
  for (uint64_t i = 0; i < codes.size(); ++i) {
    for (unsigned k = 0; k < width; ++k) {
      const uint64_t at = i * width + k;
      if ((codes[i] >> k) & 1u) words[at / 32] |= 1u << (at % 32);
    }
  }
  return words;
}

template <class Bit>
uint32_t reference_extract(Bit &&bit, uint64_t row, unsigned width) {
  uint32_t c = 0;
  for (unsigned k = 0; k < width; ++k) c |= static_cast<uint32_t>(bit(row * width + k)) << k;
  return c;
}

void check_small_columns() {
  std::mt19937 rng(11);
  for (unsigned width = 1; width <= 32; ++width) {
    REQUIRE(bitpack_mask(width) == static_cast<uint32_t>((1ull << width) - 1));
    for (uint64_t n = 0; n <= 300; ++n) {
      REQUIRE(bitpack_words(n, width) == plain_words(n, width));
      std::vector<uint32_t> codes(n);
      const int kind = static_cast<int>((n + width) % 3);  // random, all zero, all ones
      for (auto &c : codes) c = kind == 0 ? (rng() & bitpack_mask(width)) : kind == 1 ? 0u : bitpack_mask(width);
      const std::vector<uint32_t> want = reference_pack(codes, width);
      // the insert, a group at a time, as the pack kernel forms its words; the words behind the column's are zero
      std::vector<uint32_t> got(want.size(), 0xDEADBEEFu);
      for (uint64_t w = 0; w < got.size(); ++w)  // word by word, as the pack kernel forms them: padding words included
        got[w] = bitpack_group_word(GroupCodes{&codes, 32 * (w / width)}, static_cast<unsigned>(w % width), width);
      REQUIRE(got == want);
      for (uint64_t g = 0; g * 32 < n; ++g) {  // a group at a time; the words of the last group behind the column's are zero
        std::vector<uint32_t> group(width, 0xDEADBEEFu);
        CheckedOut out{&group};
        bitpack_insert_group(GroupCodes{&codes, 32 * g}, width, out);
        for (unsigned t = 0; t < width; ++t) REQUIRE(group[t] == (g * width + t < want.size() ? want[g * width + t] : 0u));
      }
      // every bit from n * width on is zero
      for (uint64_t at = n * width; at < 32 * want.size(); ++at) REQUIRE(((want[at / 32] >> (at % 32)) & 1u) == 0u);
      // the extract of every row, on words cut to what the rows need
      std::vector<uint32_t> exact(want.begin(), want.begin() + (n * width + 31) / 32);
      for (uint64_t i = 0; i < n; ++i) {
        REQUIRE(bitpack_bit(i, width) == i * width);
        REQUIRE(bitpack_extract(Checked{&exact}, i, width) == codes[i]);
        REQUIRE(reference_extract([&](uint64_t at) { return (want[at / 32] >> (at % 32)) & 1u; }, i, width) == codes[i]);
      }
      // through an origin: the words from a group boundary on, as a kernel stages them
      for (uint64_t g = 0; g * 32 < n; g += 3) {
        const uint64_t origin = g * width;
        std::vector<uint32_t> piece(exact.begin() + origin, exact.end());
        for (uint64_t i = 32 * g; i < n; i += 7) REQUIRE(bitpack_extract(Checked{&piece}, i, width, origin) == codes[i]);
        // the staged form: rows counted from the piece's first, both words read always, one word of padding (of any
        // content) behind the piece
        piece.push_back(0xDEADBEEFu);
        for (uint64_t i = 32 * g; i < n; i += 5)
          REQUIRE(bitpack_extract_staged(Checked{&piece}, static_cast<uint32_t>(i - 32 * g), width) == codes[i]);
      }
    }
  }
}

uint32_t word_of(uint64_t w) {
  uint64_t x = (w + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return static_cast<uint32_t>(x);
}

// a column too large to store: word w is word_of(w); indices at or past `size` abort
struct Fake {
  uint64_t size;
  uint64_t *last;
  uint32_t operator[](uint64_t w) const {
    REQUIRE(w < size);
    if (w > *last) *last = w;
    ++g_reads;
    return word_of(w);
  }
};

void check_large_rows() {
  const uint64_t counts[] = {1, 4097, 65537, (1ull << 20) + 1, (1ull << 27) + 3, (1ull << 31) - 1, 1ull << 31,
                             (1ull << 31) + 1, (1ull << 32) - 2, (1ull << 32) - 1};
  for (unsigned width = 1; width <= 32; ++width) {
    REQUIRE(bitpack_words(1ull << 32, width) == 0 && bitpack_words((1ull << 32) + 5, width) == 0);
    for (const uint64_t n : counts) {
      const uint64_t stated = (n * width + 31) / 32;  // the words the rows need, in front of the padding
      REQUIRE(bitpack_words(n, width) == plain_words(n, width) && bitpack_words(n, width) - stated < 4);
      uint64_t last = 0;
      const Fake column{stated, &last};
      const uint64_t rows[] = {0, 1, 31, 32, 33, n / 3, n / 2, (1ull << 27) - 1, 1ull << 27, (1ull << 31) - 1, 1ull << 31,
                               n - 2, n - 1};
      for (const uint64_t r : rows) {
        if (r >= n) continue;
        REQUIRE(bitpack_bit(r, width) == r * width);
        const uint32_t want = reference_extract([](uint64_t at) { return (word_of(at / 32) >> (at % 32)) & 1u; }, r, width);
        REQUIRE(bitpack_extract(column, r, width) == want);
      }
      REQUIRE(last == stated - 1);  // row n - 1 ends in the last word, and nothing behind it was asked for
    }
  }
  REQUIRE(bitpack_words(5, 0) == 0 && bitpack_words(5, 33) == 0 && bitpack_words(0, 7) == 0);
  REQUIRE(bitpack_bit((1ull << 32) - 1, 32) == ((1ull << 32) - 1) * 32);  // 2^37 - 32: 64-bit
}

void check_funnel() {
  std::mt19937 rng(13);
  for (unsigned width = 1; width <= 32; ++width) {
    for (unsigned bit = 0; bit < 32; ++bit) {
      const uint32_t lo = rng(), hi = rng();
      const uint32_t want = reference_extract(
          [&](uint64_t at) { return at < 32 ? (lo >> at) & 1u : at < 64 ? (hi >> (at - 32)) & 1u : 0u; }, 0, 32) ;
      REQUIRE(want == lo);
      uint32_t code = 0;
      for (unsigned k = 0; k < width; ++k) {
        const unsigned at = bit + k;
        code |= (at < 32 ? (lo >> at) & 1u : (hi >> (at - 32)) & 1u) << k;
      }
      REQUIRE(bitpack_funnel(lo, hi, bit, width) == code);
      if (bit + width <= 32) REQUIRE(bitpack_funnel(lo, ~hi, bit, width) == code);  // nothing comes from hi
    }
  }
}

void check_layout() {
  uint64_t before = 0;
  const uint64_t caps[] = {0, 1, 4095, 4096, 4097, 8192, 100003, 1ull << 20, (1ull << 22) + 1, 1ull << 26, (1ull << 32) - 1};
  for (const uint64_t c : caps) {
    const BitpackLayout l = bitpack_layout(c);
    REQUIRE(l.segments == (c + DBENCH_BITPACK_SEGMENT_ROWS - 1) / DBENCH_BITPACK_SEGMENT_ROWS);
    REQUIRE(l.cnt == 256 && l.cnt % 256 == 0 && l.pos % 256 == 0 && l.masks % 256 == 0 && l.total % 256 == 0);
    REQUIRE(l.pos >= l.cnt + 4 * l.segments && l.masks >= l.pos + 4 * l.segments && l.total >= l.masks + 512 * l.segments);
    REQUIRE(l.total >= before && l.total <= 1536 + c / 7);
    before = l.total;
  }
  REQUIRE(bitpack_layout(0).total == 256);
}

void check_against(const char *path) {
  std::FILE *f = std::fopen(path, "r");
  REQUIRE(f != nullptr);
  char kind;
  uint64_t a, b, c;
  long lines = 0;
  while (std::fscanf(f, " %c %" SCNu64 " %" SCNu64, &kind, &a, &b) == 3) {
    if (kind == 'W') {
      REQUIRE(std::fscanf(f, " %" SCNu64, &c) == 1);
      REQUIRE(bitpack_words(a, static_cast<unsigned>(b)) == c);
    } else {
      REQUIRE(kind == 'S');
      REQUIRE((a >= (1ull << 32) ? 0 : bitpack_layout(a).total) == b);
    }
    ++lines;
  }
  std::fclose(f);
  REQUIRE(lines > 0);
}

}  // namespace

int main(int argc, char **argv) {
  check_small_columns();
  check_large_rows();
  check_funnel();
  check_layout();
  if (argc > 1) check_against(argv[1]);
  std::printf("bitpack layout ok: %ld reads\n", g_reads);
  return 0;
}
