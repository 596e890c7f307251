// call_checks.hpp — the argument checks the dbench_* entry points share (select_rows, merge_sorted, take_rows,
// dict_encode, bitpack), in plain C++: no HIP, so that tests/cpp/call_checks_check.cpp runs this text on the host.
//   addr, words_past_16, fits_32      an address as a number, its phase inside a 16-byte vector, a 32-bit size
//   Range, overlap, outputs_overlap   do two buffers share a byte; does an output touch an input or another output
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dbhip {

inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// the 32-bit words of p behind the 16-byte boundary in front of it: 0..3 (p is 4-byte aligned)
inline unsigned words_past_16(const void *p) { return static_cast<unsigned>((addr(p) >> 2) & 3u); }

// row ids, positions and counts are 32 bits wide
inline bool fits_32(size_t n) { return n < (1ull << 32); }

struct Range {
  const void *p;
  size_t bytes;
};

// a null pointer or an empty range overlaps nothing.  The distance between the two starts is compared, never an end:
// a range that ends at the top of the address space has no end that could wrap
inline bool overlap(const Range &x, const Range &y) {
  if (!x.p || !y.p || !x.bytes || !y.bytes) return false;
  const uintptr_t a = addr(x.p), b = addr(y.p);
  return a < b ? b - a < x.bytes : a - b < y.bytes;
}

inline bool overlap(const void *p, size_t p_bytes, const void *q, size_t q_bytes) {
  return overlap(Range{p, p_bytes}, Range{q, q_bytes});
}

// an output overlapping an input or another output
inline bool outputs_overlap(const Range *outs, int n_outs, const Range *ins, int n_ins) {
  for (int i = 0; i < n_outs; ++i) {
    for (int j = 0; j < n_ins; ++j)
      if (overlap(outs[i], ins[j])) return true;
    for (int j = i + 1; j < n_outs; ++j)
      if (overlap(outs[i], outs[j])) return true;
  }
  return false;
}

}  // namespace dbhip
