// bitpack_layout.hpp — the pieces of the bit-packed column (bitpack.hpp, bitpack.cpp) that compute an index or a size from
// integers: the word count, the bit position of a row, the extract of one code, the insert of a group of 32 codes into its
// `width` words, and the regions of the workspace.  Plain functions for host and device behind one qualifier macro,
// templated on the "words" type (anything with operator[] that yields a uint32_t): the kernels run them on global and LDS
// pointers, tests/cpp/bitpack_layout_check.cpp runs the same text on the host over arrays that check every index.
//
// Format.  Code i occupies bits [i * width, i * width + width) of a little-endian bit stream over uint32 words, least
// significant bit first: its first word is (i * width) >> 5, its first bit (i * width) & 31, and it may straddle two words.
// 32 rows are exactly `width` words (a group), 128 rows `width` 16-byte chunks.  i * width needs 64 bits (up to 2^37), and
// no shift here is ever by 32: a code that starts at bit 0 is taken from one word, whatever its width.
//
// bitpack_extract reads no word it does not need: it touches the second word only when the code straddles, so the last
// word read for row n_rows - 1 is inside ceil(n_rows * width / 32).  bitpack_extract_staged, for a piece staged in LDS with
// a word of padding behind it, reads both words always.
#ifndef DBENCH_BITPACK_LAYOUT_HPP
#define DBENCH_BITPACK_LAYOUT_HPP

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBENCH_BITPACK_FN __host__ __device__ inline
#else
#define DBENCH_BITPACK_FN inline
#endif

#include "bitpack.hpp" /* DBENCH_BITPACK_SEGMENT_ROWS */

// the words of a column of n_rows codes: ceil(n_rows * width / 32) rounded up to whole 16-byte chunks; 0 for a width
// outside 1 .. 32 or n_rows >= 2^32 (no such column)
DBENCH_BITPACK_FN uint64_t bitpack_words(uint64_t n_rows, unsigned width) {
  if (width < 1 || width > 32 || n_rows >= (1ull << 32)) return 0;
  const uint64_t words = (n_rows * width + 31) >> 5;
  return (words + 3) & ~static_cast<uint64_t>(3);
}

// the position of row's first bit in the stream
DBENCH_BITPACK_FN uint64_t bitpack_bit(uint64_t row, unsigned width) { return row * width; }

// the `width` low bits set; width 32 does not shift by 32
DBENCH_BITPACK_FN uint32_t bitpack_mask(unsigned width) { return width >= 32 ? 0xFFFFFFFFu : (1u << width) - 1u; }

// the `width` bits from bit `bit` (0 .. 31) on of the 64-bit word hi:lo: one funnel shift, never by 32 or more.  A code
// that does not straddle (bit + width <= 32) takes nothing from hi, whatever hi holds.
DBENCH_BITPACK_FN uint32_t bitpack_funnel(uint32_t lo, uint32_t hi, unsigned bit, unsigned width) {
  const uint64_t both = (static_cast<uint64_t>(hi) << 32) | lo;
  return static_cast<uint32_t>(both >> (bit & 31u)) & bitpack_mask(width);
}

// the code of `row`.  words[0] is word `origin` of the stream (0 for the column itself, the first staged word for a
// piece of it in LDS); reads words[w - origin] and, only if the code straddles, words[w - origin + 1], w = bit >> 5
template <class Words>
DBENCH_BITPACK_FN uint32_t bitpack_extract(const Words &words, uint64_t row, unsigned width, uint64_t origin = 0) {
  const uint64_t at = bitpack_bit(row, width);
  const uint64_t w = (at >> 5) - origin;
  const unsigned bit = static_cast<unsigned>(at & 31u);
  const uint32_t lo = words[w];
  const uint32_t hi = bit + width <= 32 ? 0u : words[w + 1];
  return bitpack_funnel(lo, hi, bit, width);
}

// the same for row `local` of a piece that starts at a group boundary (bit 0 of words[0]) and is followed by one word of
// padding: 32-bit arithmetic (local * width < 2^32: a piece of at most 2^27 rows) and both words read unconditionally, so
// the two reads are one instruction on LDS.  Reads words[w] and words[w + 1], w = (local * width) >> 5.
template <class Words>
DBENCH_BITPACK_FN uint32_t bitpack_extract_staged(const Words &words, uint32_t local, unsigned width) {
  const uint32_t at = local * width;
  const uint32_t w = at >> 5;
  return bitpack_funnel(words[w], words[w + 1], at & 31u, width);
}

// word t (0 .. width - 1) of the `width` words that hold a group of 32 codes c[0 .. 32), every code below 2^width: the
// tail of the code that started in the word before, then every code that starts inside this one.  Reads c[r] for
// r < 32 only.
template <class Codes>
DBENCH_BITPACK_FN uint32_t bitpack_group_word(const Codes &c, unsigned t, unsigned width) {
  const unsigned first_bit = 32 * t;
  unsigned r = first_bit / width;  // the row whose bits reach first_bit
  unsigned start = r * width;      // <= first_bit
  uint32_t w = 0;
  if (start < first_bit) {  // its tail: a shift by 1 .. 31
    w = c[r] >> (first_bit - start);
    ++r;
    start += width;
  }
  for (; start < first_bit + 32; ++r, start += width) w |= c[r] << (start - first_bit);  // shifts by 0 .. 31
  return w;
}

// the insert of a group of 32 codes into its `width` words
template <class Codes, class Words>
DBENCH_BITPACK_FN void bitpack_insert_group(const Codes &c, unsigned width, Words &out) {
  for (unsigned t = 0; t < width; ++t) out[t] = bitpack_group_word(c, t, width);
}

// the regions of the workspace, byte offsets from its start, each a multiple of 256; S = capacity /
// DBENCH_BITPACK_SEGMENT_ROWS rounded up, A = 4 S rounded up to 256:
//   [0, 256)               header, word 0 = status
//   [cnt, cnt + A)         S x uint32 matches per segment
//   [pos, pos + A)         S x uint32 first output position per segment
//   [masks, total)         S x 64 x uint64 match masks: one bit per candidate
struct BitpackLayout {
  uint64_t segments, cnt, pos, masks, total;
};

DBENCH_BITPACK_FN uint64_t bitpack_align256(uint64_t x) { return (x + 255u) & ~static_cast<uint64_t>(255u); }

DBENCH_BITPACK_FN BitpackLayout bitpack_layout(uint64_t capacity) {
  BitpackLayout l;
  l.segments = (capacity + DBENCH_BITPACK_SEGMENT_ROWS - 1) / DBENCH_BITPACK_SEGMENT_ROWS;
  const uint64_t a = bitpack_align256(4 * l.segments);
  l.cnt = 256;
  l.pos = l.cnt + a;
  l.masks = l.pos + a;
  l.total = bitpack_align256(l.masks + 512 * l.segments);
  return l;
}

#endif
