// call_checks_check.cpp — dwarf_bench_amd/host/call_checks.hpp on the host, the text every dbench_* entry point of the
// row-id operators runs on its arguments: overlap (null and empty ranges, touching ranges and ranges one byte short of
// touching in both argument orders, ranges that end at the top of the address space), outputs_overlap (an output
// against an input and against another output, found at the first and at the last index), words_past_16 over the 16 byte
// offsets that are multiples of 4, and fits_32 around 2^32.  The addresses are numbers; nothing is read through them.
// No GPU, no HIP: plain C++.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "call_checks.hpp"

namespace {

using namespace dbhip;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }

// both overloads, both argument orders
void expect(uintptr_t p, size_t p_bytes, uintptr_t q, size_t q_bytes, bool want) {
  REQUIRE(overlap(at(p), p_bytes, at(q), q_bytes) == want);
  REQUIRE(overlap(at(q), q_bytes, at(p), p_bytes) == want);
  REQUIRE(overlap(Range{at(p), p_bytes}, Range{at(q), q_bytes}) == want);
  REQUIRE(overlap(Range{at(q), q_bytes}, Range{at(p), p_bytes}) == want);
}

void check_overlap() {
  const uintptr_t p = 0x10000;
  // null pointers and zero sizes never overlap, not even with themselves
  expect(0, 64, 0, 64, false);
  expect(0, 64, p, 64, false);
  expect(p, 0, p, 64, false);
  expect(p, 0, p, 0, false);
  expect(p, 64, p + 8, 0, false);  // an empty range inside another
  // a range and itself, a range inside another
  expect(p, 64, p, 64, true);
  expect(p, 64, p + 8, 4, true);
  expect(p, 1, p, 1, true);
  for (size_t n : {size_t{1}, size_t{4}, size_t{64}, size_t{4096}}) {
    expect(p, n, p + n, 64, false);         // touching: [p, p+n) against [p+n, ...)
    expect(p, n + 1, p + n, 64, true);      // one byte short of touching
    expect(p, n, p + n - 1, 64, true);
    expect(p, n, p + n + 1, 64, false);     // a gap of one byte
  }
  // ranges that end at the top of the address space: p + bytes == 2^N wraps to 0 as a number, the answer stays right
  const uintptr_t top = ~uintptr_t{0};  // the last byte's address
  expect(top - 63, 64, top - 63, 64, true);
  expect(top - 63, 64, top, 1, true);
  expect(top - 63, 64, top - 127, 64, false);  // touching below it
  expect(top - 63, 64, top - 127, 65, true);
  expect(top - 63, 64, p, 64, false);          // far away: no wrap into a hit
  expect(top - 63, 64, 1, 64, false);
  expect(top, 1, top - 1, 1, false);
  expect(top, 1, top - 1, 2, true);
}

void check_outputs_overlap() {
  const uintptr_t base = 0x40000;
  // four outputs and five inputs, 64 bytes each, 256 bytes apart: disjoint
  Range outs[4], ins[5];
  auto fresh = [&]() {
    for (int i = 0; i < 4; ++i) outs[i] = Range{at(base + 256 * i), 64};
    for (int j = 0; j < 5; ++j) ins[j] = Range{at(base + 0x1000 + 256 * j), 64};
  };
  fresh();
  REQUIRE(!outputs_overlap(outs, 4, ins, 5));
  REQUIRE(!outputs_overlap(outs, 0, ins, 5) && !outputs_overlap(outs, 4, ins, 0) && !outputs_overlap(outs, 1, ins, 0));
  // an output against an input: every pair, the first and the last index of either among them
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 5; ++j) {
      fresh();
      ins[j] = Range{at(base + 256 * i + 63), 2};  // the output's last byte
      REQUIRE(outputs_overlap(outs, 4, ins, 5));
      ins[j] = Range{at(base + 256 * i + 64), 2};  // touching
      REQUIRE(!outputs_overlap(outs, 4, ins, 5));
      ins[j] = Range{nullptr, 64};                 // an absent input
      REQUIRE(!outputs_overlap(outs, 4, ins, 5));
    }
  }
  // an output against another output: every pair
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 4; ++k) {
      if (i == k) continue;
      fresh();
      outs[k] = Range{at(base + 256 * i + 32), 64};
      REQUIRE(outputs_overlap(outs, 4, ins, 5));
      REQUIRE(outputs_overlap(outs, 4, ins, 0));
      outs[k] = Range{at(base + 256 * i + 64), 64};  // touching
      REQUIRE(!outputs_overlap(outs, 4, ins, 5));
    }
  }
  // inputs may overlap each other
  fresh();
  ins[4] = ins[0];
  REQUIRE(!outputs_overlap(outs, 4, ins, 5));
}

void check_words_and_sizes() {
  for (uintptr_t base : {uintptr_t{0}, uintptr_t{0x7f00}, ~uintptr_t{0} - 15}) {  // 16-byte aligned
    for (unsigned off = 0; off < 16; off += 4) {
      REQUIRE(words_past_16(at(base + off)) == off / 4);
      REQUIRE(addr(at(base + off)) == base + off);
    }
  }
  const unsigned long long two32 = 1ull << 32;
  REQUIRE(fits_32(0) && fits_32(1) && fits_32(static_cast<size_t>(two32 - 1)));
  REQUIRE(!fits_32(static_cast<size_t>(two32)) && !fits_32(static_cast<size_t>(two32 + 1)));
  REQUIRE(!fits_32(~size_t{0}));
}

}  // namespace

int main() {
  static_assert(sizeof(size_t) == 8 && sizeof(uintptr_t) == 8, "64-bit sizes and addresses");
  check_overlap();
  check_outputs_overlap();
  check_words_and_sizes();
  std::printf("call checks ok\n");
  return 0;
}
