// quantile_layout.hpp — the pieces of the quantile select (quantile_select.hpp, quantile_select.cpp) that are plain integer
// arithmetic: the digits of the three levels, the rank a (q_num, q_den) pair names among m candidates, and the test that says
// whether a histogram bin holds a rank.  Plain functions for host and device behind one qualifier macro: qs_pick runs them on
// the GPU, tests/cpp/quantile_layout_check.cpp runs the same text on the host and prints what it gives,
// tests/quantile_model.py is the Python form of it.
//
// Digits.  x = key ^ flip (flip = 0x80000000 under DBENCH_QUANTILE_SIGNED) is cut into 11 / 11 / 10 bits from the top:
//   level 0: x >> 21            level 1: (x >> 10) & 0x7FF            level 2: x & 0x3FF
// Ranks.  q_den == 0: the absolute 0-based rank r = q_num.  q_den > 0 (q_num <= q_den): r = 0 for q_num == 0, otherwise
//   r = ceil(q_num * m / q_den) - 1 (PERCENTILE_DISC: 1/2 is the lower median, 1/1 the maximum), in 64-bit integers: with
//   m, q_num, q_den < 2^32 neither the product nor the rounding term overflows.  A rank exists iff r < m.
// Bins.  Of the candidates counted into a histogram, `before` lie in the bins in front of a bin and `count` in it: the bin
//   holds the candidate of 0-based rank rem (counted inside the histogram) iff before <= rem < before + count.  An empty bin
//   holds nothing, so exactly one bin of a histogram of more than rem candidates does.
#ifndef DBENCH_QUANTILE_LAYOUT_HPP
#define DBENCH_QUANTILE_LAYOUT_HPP

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBENCH_QUANTILE_FN __host__ __device__ inline
#else
#define DBENCH_QUANTILE_FN inline
#endif

#define DBENCH_QUANTILE_LEVELS 3
#define DBENCH_QUANTILE_RADIX 2048 /* bins of the widest level */
#define DBENCH_QUANTILE_NO_SLOT 0xFFFFFFFFu /* the slot of a rank that names no row */

// the shift and the width in bits of a level's digit
DBENCH_QUANTILE_FN int qs_shift(int level) { return level == 0 ? 21 : (level == 1 ? 10 : 0); }
DBENCH_QUANTILE_FN int qs_width(int level) { return level == 2 ? 10 : 11; }
DBENCH_QUANTILE_FN uint32_t qs_radix(int level) { return 1u << qs_width(level); }
DBENCH_QUANTILE_FN uint32_t qs_digit(uint32_t x, int level) { return (x >> qs_shift(level)) & (qs_radix(level) - 1u); }
// the bits above a level's digit: what a candidate shares with a prefix found so far
DBENCH_QUANTILE_FN uint32_t qs_high_mask(int level) { return level == 0 ? 0u : ~((1u << (qs_shift(level) + qs_width(level))) - 1u); }

// (q_num, q_den) among m candidates -> the 0-based rank in *r; false: no such row (m == 0, or an absolute rank >= m)
DBENCH_QUANTILE_FN bool qs_resolve_rank(uint32_t q_num, uint32_t q_den, uint32_t m, uint32_t *r) {
  uint64_t rank = q_num;
  if (q_den != 0) {
    const uint64_t product = static_cast<uint64_t>(q_num) * m;
    rank = product == 0 ? 0 : (product + q_den - 1) / q_den - 1;
  }
  *r = static_cast<uint32_t>(rank);
  return rank < m;
}

// does the bin with `before` candidates in front of it and `count` in it hold the candidate of rank rem
DBENCH_QUANTILE_FN bool qs_bin_holds(uint32_t before, uint32_t count, uint32_t rem) {
  return before <= rem && rem - before < count;
}

#endif
