// hll_layout.hpp — the pieces of the HyperLogLog sketch (hll_sketch.hpp, hll_sketch.cpp) that compute a hash, a register
// index, a rank or the estimate from integers.  Plain functions for host and device behind one qualifier macro: the kernels
// run them on the GPU, tests/cpp/hll_layout_check.cpp runs the same text on the host and prints what it gives,
// tests/hll_model.py is the numpy form of it.
//
// Format.  A sketch is (registers, p, seed): p in 4 .. 14, m = 2^p registers of one byte each, q = 64 - p, every byte in
// 0 .. q+1.  A row's key is the tuple of its values in k = 1 .. 4 32-bit columns c_0 .. c_{k-1} (any bit pattern):
//   h = fmix32(c_0 ^ seed)            g = fmix32(c_0 ^ seed ^ 0x9E3779B9)          (csrc/dbhip_common.hpp)
//   for j = 1 .. k-1:  h = fmix32(h ^ c_j)    g = fmix32(g ^ c_j)
//   x    = uint64(h) << 32 | g
//   idx  = x >> (64 - p)
//   w    = x << p                     a 64-bit shift: the low 32 - p bits of h, then all of g
//   rank = w ? clz64(w) + 1 : q + 1   1 .. q+1
//   insert: registers[idx] = max(registers[idx], rank)
// With one column both chains are bijections of the key: distinct keys never share x.
// The estimate is a host function of the histogram of the registers alone (Ertl's improved raw estimator, in double).
#ifndef DBENCH_HLL_LAYOUT_HPP
#define DBENCH_HLL_LAYOUT_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "dbhip_common.hpp" /* fmix32 */

#define DBENCH_HLL_FN __host__ __device__ inline

#define DBENCH_HLL_MIN_P 4
#define DBENCH_HLL_MAX_P 14
#define DBENCH_HLL_MAX_COLS 4
#define DBENCH_HLL_HIST_WORDS 64
#define DBENCH_HLL_GOLDEN 0x9E3779B9u

struct HllHash {
  uint32_t h, g;
};

struct HllPlace {
  uint32_t idx, rank;
};

DBENCH_HLL_FN bool hll_p_ok(unsigned p) { return p >= DBENCH_HLL_MIN_P && p <= DBENCH_HLL_MAX_P; }

// the two chains after the first column, and after one more
DBENCH_HLL_FN HllHash hll_hash_first(uint32_t c0, uint32_t seed) {
  return HllHash{dbhip::fmix32(c0 ^ seed), dbhip::fmix32(c0 ^ seed ^ DBENCH_HLL_GOLDEN)};
}

DBENCH_HLL_FN HllHash hll_hash_next(HllHash s, uint32_t c) { return HllHash{dbhip::fmix32(s.h ^ c), dbhip::fmix32(s.g ^ c)}; }

// the hash of the tuple c[0 .. k), k >= 1
DBENCH_HLL_FN HllHash hll_hash(const uint32_t *c, int k, uint32_t seed) {
  HllHash s = hll_hash_first(c[0], seed);
  for (int j = 1; j < k; ++j) s = hll_hash_next(s, c[j]);
  return s;
}

// the register of a hash and the rank it offers: idx < 2^p, 1 <= rank <= 64 - p + 1
DBENCH_HLL_FN HllPlace hll_place(uint32_t h, uint32_t g, unsigned p) {
  const uint64_t x = (static_cast<uint64_t>(h) << 32) | g;
  const uint64_t w = x << p;
  const uint32_t rank = w ? static_cast<uint32_t>(__builtin_clzll(w)) + 1u : 64u - p + 1u;
  return HllPlace{static_cast<uint32_t>(x >> (64u - p)), rank};
}

// ---- the estimate: host only, double --------------------------------------------------------------------------------------
// sigma(x) = x + sum over k >= 1 of x^(2^k) 2^(k-1), tau(x) = (1 - x - sum over k >= 1 of (1 - x^(2^-k))^2 2^-k) / 3, both
// iterated until the double stops changing (Ertl, "New cardinality estimation algorithms for HyperLogLog sketches", 2017)
inline double hll_sigma(double x) {
  if (x == 1.0) return INFINITY;
  double y = 1.0, z = x;
  for (;;) {
    x *= x;
    const double before = z;
    z += x * y;
    y += y;
    if (z == before) return z;
  }
}

inline double hll_tau(double x) {
  if (x == 0.0 || x == 1.0) return 0.0;
  double y = 1.0, z = 1.0 - x;
  for (;;) {
    x = sqrt(x);
    const double before = z;
    y *= 0.5;
    z -= (1.0 - x) * (1.0 - x) * y;
    if (z == before) return z / 3.0;
  }
}

// hist[v] = the registers equal to v.  -1.0: p out of range, a count above q+1, or counts that do not sum to m.  0.0 for the
// empty sketch, +infinity for the one whose registers are all saturated
inline double hll_estimate(const uint32_t *hist, unsigned p) {
  if (!hist || !hll_p_ok(p)) return -1.0;
  const unsigned q = 64u - p;
  const uint64_t m = 1ull << p;
  uint64_t sum = 0;
  for (unsigned v = 0; v < DBENCH_HLL_HIST_WORDS; ++v) {
    if (v > q + 1 && hist[v]) return -1.0;
    sum += hist[v];
  }
  if (sum != m) return -1.0;
  const double dm = static_cast<double>(m);
  double z = dm * hll_tau(1.0 - static_cast<double>(hist[q + 1]) / dm);
  for (unsigned k = q; k >= 1; --k) z = (z + static_cast<double>(hist[k])) * 0.5;
  z += dm * hll_sigma(static_cast<double>(hist[0]) / dm);
  if (z == 0.0) return INFINITY;
  return dm * dm / (2.0 * log(2.0) * z);
}

#endif
