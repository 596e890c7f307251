// bloom_filter.cpp — a Bloom filter over 32-bit keys on gfx950 (bloom_filter.hpp holds the contract, bloom_layout.hpp the
// placement of a key, which the kernels below and the host check run as the same text): build from a column or through a
// row-id list, and the probe that feeds the selection vectors.
//
// One word per key: an inserted key costs one 8-byte read and at most one no-return 64-bit atomic OR, a probed key one
// 8-byte gather.  Both kernels walk their keys as sel_mark_kernel walks its candidates (select_rows.cpp): a wave owns a
// segment of 4096 positions counted from the 16-byte boundary in front of the column (or the list), a lane holds four
// consecutive entries per group of 256 (one aligned 16-byte load; in list mode then four 4-byte gathers, row 0 standing in
// for an entry that does not count), four groups in flight in a whole segment, the ragged ends word by word (load_ragged).
//   build  per key: place, a plain load of the filter word, and the atomic OR only where a bit of the mask is missing.  With
//          few distinct keys (the reference's [1, 10000]) almost every key finds its bits set and the kernel is a stream
//          of reads; a stale read costs a redundant atomic, never a wrong filter, since bits are only ever added.
//   probe  mark: the sixteen keys of four groups, then their sixteen 8-byte filter gathers, then the ballots — select's
//          mask layout, so that scan (launch_rowlist_scan) and write (sel_write_kernel, select_write.hpp) are select's.
//          The gather of an entry that does not count uses key 0: every key's word lies inside the filter.
#include "bloom_filter.hpp"

#include "bloom_layout.hpp"
#include "rowlist.hpp"
#include "select_write.hpp"

namespace {
using namespace dbhip;

// the lane's four entries e (bit q of `valid`: entry q exists) -> the keys x and the entries `ok` that count; in list mode
// through the column, and `bad` collects a row id >= n_col.  sel_mark_kernel's fetch.
template <bool kList>
__device__ __forceinline__ void bloom_fetch(const unsigned *__restrict__ col, unsigned n_col, const u32x4 e, unsigned valid,
                                            unsigned (&x)[4], unsigned &ok, bool &bad) {
  const unsigned w[4] = {e.x, e.y, e.z, e.w};
  ok = valid;
#pragma unroll
  for (int q = 0; q < 4; ++q) x[q] = w[q];
  if (kList) {
    unsigned row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool inside = w[q] < n_col;
      bad = bad || (((valid >> q) & 1u) && !inside);
      if (!inside) ok &= ~(1u << q);
      row[q] = ((ok >> q) & 1u) ? w[q] : 0u;
      x[q] = 0u;
    }
    if (n_col) {  // uniform; an empty column has no row 0, and no entry that counts
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = col[row[q]];
    }
  }
}

#ifdef DBENCH_BLOOM_ALWAYS_SET /* measurement only (tools/ab.py bloom): a build without test-before-set */
constexpr bool kBuildTests = false;
#else
constexpr bool kBuildTests = true;
#endif

// the bits of each key's mask that its filter word lacks: 0 = the filter may hold the key.  Unconditional loads, each inside
// the filter whatever x holds.  !kTest: the whole mask, without the load
template <bool kTest = true>
__device__ __forceinline__ void bloom_missing(const u64 *filter, unsigned n_words, unsigned seed, const unsigned (&x)[4],
                                              unsigned (&word)[4], u64 (&miss)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const BloomPlace p = bloom_place(x[q], seed, n_words);
    word[q] = p.word;
    miss[q] = kTest ? p.mask & ~filter[p.word] : p.mask;
  }
}

// ---------------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------------
// kList: `src` is the row-id list (gathered through into col), otherwise the column itself.  m_host entries at most;
// *count (nullable) lowers it on the device.
template <bool kList>
__global__ __launch_bounds__(kSelThreads) void bloom_build_kernel(const unsigned *__restrict__ col, unsigned n_col,
                                                                  const unsigned *__restrict__ src, size_t m_host,
                                                                  const u64 *count, unsigned a, unsigned seed, u64 *filter,
                                                                  unsigned n_words, unsigned *status, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSelWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const size_t m = clamped_count(count, m_host);
  const size_t vfirst = seg * kSelSegment, vend = a + m;  // positions [a, vend) hold entries
  if (vfirst >= vend) return;                              // a segment behind the last key
  bool bad = false;

  auto set = [&](const unsigned (&word)[4], const u64 (&miss)[4], unsigned ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (((ok >> q) & 1u) && miss[q] != 0)  // the result is not used: a no-return atomic
        __hip_atomic_fetch_or(filter + word[q], miss[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  if (vfirst >= a && vfirst + kSelSegment <= vend) {  // a whole segment: 16 aligned 16-byte loads per lane
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (vfirst - a)) + lane;
#pragma unroll 1
    for (int g = 0; g < kSelGroups; g += 4) {  // four loads in flight, then sixteen gathers (list), then sixteen filter words
      const u32x4 v0 = s4[g * kWave], v1 = s4[(g + 1) * kWave], v2 = s4[(g + 2) * kWave], v3 = s4[(g + 3) * kWave];
      unsigned x0[4], x1[4], x2[4], x3[4], ok0, ok1, ok2, ok3;
      bloom_fetch<kList>(col, n_col, v0, 0xfu, x0, ok0, bad);
      bloom_fetch<kList>(col, n_col, v1, 0xfu, x1, ok1, bad);
      bloom_fetch<kList>(col, n_col, v2, 0xfu, x2, ok2, bad);
      bloom_fetch<kList>(col, n_col, v3, 0xfu, x3, ok3, bad);
      unsigned w0[4], w1[4], w2[4], w3[4];
      u64 m0[4], m1[4], m2[4], m3[4];
      bloom_missing<kBuildTests>(filter, n_words, seed, x0, w0, m0);
      bloom_missing<kBuildTests>(filter, n_words, seed, x1, w1, m1);
      bloom_missing<kBuildTests>(filter, n_words, seed, x2, w2, m2);
      bloom_missing<kBuildTests>(filter, n_words, seed, x3, w3, m3);
      set(w0, m0, ok0);
      set(w1, m1, ok1);
      set(w2, m2, ok2);
      set(w3, m3, ok3);
    }
  } else {  // the first segment of an array that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
    for (int g = 0; g < kSelGroups; ++g) {
      const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
      unsigned valid, x[4], ok, word[4];
      u64 miss[4];
      const u32x4 e = load_ragged(src, a, v0, vend, valid);
      bloom_fetch<kList>(col, n_col, e, valid, x, ok, bad);
      bloom_missing<kBuildTests>(filter, n_words, seed, x, word, miss);
      set(word, miss, ok);
    }
  }
  if (kList && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
}

// ---------------------------------------------------------------------------------------------
// probe
// ---------------------------------------------------------------------------------------------
template <bool kList>
__global__ __launch_bounds__(kSelThreads) void bloom_mark_kernel(const u64 *__restrict__ filter, unsigned n_words, unsigned seed,
                                                                 const unsigned *__restrict__ col, unsigned n_col,
                                                                 const unsigned *__restrict__ src, size_t m_host,
                                                                 const u64 *in_count, unsigned a, bool negate,
                                                                 unsigned *status, unsigned *__restrict__ cnt,
                                                                 u64 *__restrict__ masks, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSelWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const size_t m = kList ? clamped_count(in_count, m_host) : m_host;
  const size_t vfirst = seg * kSelSegment, vend = a + m;  // positions [a, vend) hold candidates
  u64 mine = 0;        // mask word `lane` of the segment
  unsigned total = 0;  // matches of the segment (wave-uniform)
  bool bad = false;    // a row id >= n_col among this lane's candidates

  auto vote = [&](int g, const u64 (&miss)[4], unsigned ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u64 b = __ballot(((ok >> q) & 1u) && ((miss[q] == 0) != negate));
      total += static_cast<unsigned>(__popcll(b));
      if (lane == static_cast<unsigned>(4 * g + q)) mine = b;
    }
  };

  if (vfirst >= vend) {
    // a segment behind the last candidate (the list is shorter than its capacity): zero count, zero masks
  } else if (vfirst >= a && vfirst + kSelSegment <= vend) {  // a whole segment: 16 aligned 16-byte loads per lane
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (vfirst - a)) + lane;
#pragma unroll 1
    for (int g = 0; g < kSelGroups; g += 4) {  // four loads in flight, in list mode then sixteen gathers, then sixteen filter words
      const u32x4 v0 = s4[g * kWave], v1 = s4[(g + 1) * kWave], v2 = s4[(g + 2) * kWave], v3 = s4[(g + 3) * kWave];
      unsigned x0[4], x1[4], x2[4], x3[4], ok0, ok1, ok2, ok3;
      bloom_fetch<kList>(col, n_col, v0, 0xfu, x0, ok0, bad);
      bloom_fetch<kList>(col, n_col, v1, 0xfu, x1, ok1, bad);
      bloom_fetch<kList>(col, n_col, v2, 0xfu, x2, ok2, bad);
      bloom_fetch<kList>(col, n_col, v3, 0xfu, x3, ok3, bad);
      unsigned w[4];
      u64 m0[4], m1[4], m2[4], m3[4];
      bloom_missing(filter, n_words, seed, x0, w, m0);
      bloom_missing(filter, n_words, seed, x1, w, m1);
      bloom_missing(filter, n_words, seed, x2, w, m2);
      bloom_missing(filter, n_words, seed, x3, w, m3);
      vote(g, m0, ok0);
      vote(g + 1, m1, ok1);
      vote(g + 2, m2, ok2);
      vote(g + 3, m3, ok3);
    }
  } else {  // the first segment of an array that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
    for (int g = 0; g < kSelGroups; ++g) {
      const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
      unsigned valid, x[4], ok, w[4];
      u64 miss[4];
      const u32x4 e = load_ragged(src, a, v0, vend, valid);
      bloom_fetch<kList>(col, n_col, e, valid, x, ok, bad);
      bloom_missing(filter, n_words, seed, x, w, miss);
      vote(g, miss, ok);
    }
  }
  masks[seg * kSelWords + lane] = mine;
  if (lane == 0) cnt[seg] = total;
  if (kList && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
}

bool words_ok(size_t n_words) { return n_words >= 1 && fits_32(n_words); }

}  // namespace

extern "C" size_t dbench_bloom_words(size_t n_keys, unsigned bits_per_key) {
  return static_cast<size_t>(bloom_words(n_keys, bits_per_key));
}

extern "C" size_t dbench_bloom_workspace_bytes(size_t candidates) {
  if (!fits_32(candidates)) return 0;
  return sel_layout(candidates).total;
}

extern "C" int dbench_bloom_build_u32(const uint32_t *col, size_t n_col, const uint32_t *rows, const uint64_t *count,
                                      size_t capacity, uint32_t seed, int flags, uint64_t *filter, size_t n_words,
                                      void *workspace, size_t workspace_bytes, void *stream) {
  if (flags & ~DBENCH_BLOOM_ACCUMULATE) return DBHIP_EINVAL;
  if (!words_ok(n_words) || !fits_32(n_col) || !fits_32(capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  if (!filter || (n_col && !col)) return DBHIP_EINVAL;
  if ((addr(filter) & 7u) || ((addr(col) | addr(rows)) & 3u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  const bool list = rows != nullptr;
  const size_t entries = list ? capacity : n_col;
  const size_t filter_bytes = 8 * n_words;
  if (overlap(filter, filter_bytes, col, 4 * n_col) || overlap(filter, filter_bytes, rows, 4 * capacity) ||
      overlap(filter, filter_bytes, count, 8))
    return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, kWsHeader, s);
  if (rc != DBHIP_OK) return rc;
  if (!(flags & DBENCH_BLOOM_ACCUMULATE)) {
    const hipError_t e = fill_async(filter, 0, filter_bytes, s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (!entries) return launch_status();
  const unsigned a = words_past_16(list ? rows : col);
  const size_t segments = (entries + a + kSelSegment - 1) / kSelSegment;
  const unsigned grid = static_cast<unsigned>((segments + kSelWaves - 1) / kSelWaves);
  unsigned *status = static_cast<unsigned *>(workspace);
  u64 *f = reinterpret_cast<u64 *>(filter);
  const u64 *c = reinterpret_cast<const u64 *>(count);
  if (list)
    hipLaunchKernelGGL((bloom_build_kernel<true>), dim3(grid), dim3(kSelThreads), 0, s, col, static_cast<unsigned>(n_col), rows,
                       capacity, c, a, seed, f, static_cast<unsigned>(n_words), status, segments);
  else
    hipLaunchKernelGGL((bloom_build_kernel<false>), dim3(grid), dim3(kSelThreads), 0, s, col, static_cast<unsigned>(n_col), col,
                       n_col, c, a, seed, f, static_cast<unsigned>(n_words), status, segments);
  return launch_status();
}

extern "C" int dbench_bloom_probe_u32(const uint64_t *filter, size_t n_words, uint32_t seed, const uint32_t *col, size_t n_col,
                                      const uint32_t *in_rows, const uint64_t *in_count, size_t in_capacity, int flags,
                                      uint32_t *out_rows, uint64_t *out_count, void *workspace, size_t workspace_bytes,
                                      void *stream) {
  if (flags & ~DBENCH_BLOOM_NEGATE) return DBHIP_EINVAL;
  if (!words_ok(n_words) || !fits_32(n_col) || !fits_32(in_capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  if (!filter || (n_col && !col) || !out_count || (in_count && !in_rows)) return DBHIP_EINVAL;
  if ((addr(filter) & 7u) || ((addr(col) | addr(in_rows) | addr(out_rows)) & 3u) || ((addr(in_count) | addr(out_count)) & 7u))
    return DBHIP_EINVAL;
  const bool list = in_rows != nullptr;
  const size_t candidates = list ? in_capacity : n_col;
  if (overlap(out_rows, 4 * candidates, filter, 8 * n_words) || overlap(out_rows, 4 * candidates, col, 4 * n_col) ||
      overlap(out_rows, 4 * candidates, in_rows, 4 * in_capacity))
    return DBHIP_EINVAL;
  const SelLayout l = sel_layout(candidates);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, l.total, s);
  if (rc != DBHIP_OK) return rc;

  char *base = static_cast<char *>(workspace);
  unsigned *status = reinterpret_cast<unsigned *>(base);
  unsigned *cnt = reinterpret_cast<unsigned *>(base + l.cnt);
  unsigned *pos = reinterpret_cast<unsigned *>(base + l.pos);
  u64 *masks = reinterpret_cast<u64 *>(base + l.masks);
  const u64 *f = reinterpret_cast<const u64 *>(filter);

  const unsigned a = candidates ? words_past_16(list ? in_rows : col) : 0u;
  const size_t segments = candidates ? (candidates + a + kSelSegment - 1) / kSelSegment : 0;  // <= l.segments
  const unsigned grid = static_cast<unsigned>((segments + kSelWaves - 1) / kSelWaves);
  const bool negate = (flags & DBENCH_BLOOM_NEGATE) != 0;
  if (segments) {
    if (list)
      hipLaunchKernelGGL((bloom_mark_kernel<true>), dim3(grid), dim3(kSelThreads), 0, s, f, static_cast<unsigned>(n_words), seed,
                         col, static_cast<unsigned>(n_col), in_rows, in_capacity, reinterpret_cast<const u64 *>(in_count), a,
                         negate, status, cnt, masks, segments);
    else
      hipLaunchKernelGGL((bloom_mark_kernel<false>), dim3(grid), dim3(kSelThreads), 0, s, f, static_cast<unsigned>(n_words), seed,
                         col, static_cast<unsigned>(n_col), col, n_col, static_cast<const u64 *>(nullptr), a, negate, status, cnt,
                         masks, segments);
  }
  launch_rowlist_scan(cnt, pos, segments, candidates, reinterpret_cast<u64 *>(out_count), s);
  if (segments && out_rows) {
    if (list)
      hipLaunchKernelGGL((sel_write_kernel<true>), dim3(grid), dim3(kSelThreads), 0, s, in_rows, in_capacity, a, cnt, pos, masks,
                         segments, out_rows, candidates);
    else
      hipLaunchKernelGGL((sel_write_kernel<false>), dim3(grid), dim3(kSelThreads), 0, s, static_cast<const unsigned *>(nullptr),
                         n_col, a, cnt, pos, masks, segments, out_rows, candidates);
  }
  return launch_status();
}
