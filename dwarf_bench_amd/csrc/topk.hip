// topk.hip — ORDER BY key LIMIT k for gfx950: a radix select that returns keys and row ids (include/dbhip_topk.h).
//
// No reference counterpart.  Row a precedes row b when its key is better (smaller; larger with `largest`) or the keys are
// equal and a < b; the answer is the first m = min(k, n) rows in that order.  Everything works on x = key ^ mask, for
// which better means smaller as unsigned: mask 0 (_u32), 0x80000000 (_i32), ~0 (_u32 largest), 0x7FFFFFFF (_i32 largest).
//
// All dependent launches, no workgroup ever waits on another (DESIGN.md finding 8), every loop bounded by n:
//   1. threshold   MSD radix select over 11/11/10-bit digits (tk_bits below has the A/B against 8-bit digits), per level
//        tk_hist    one streaming read of the column (16-byte loads, four in flight per lane): LDS histogram of the
//                   level's digit over the keys whose higher bits equal the prefix found so far (read from the header),
//                   in copies and with the shortcut for a digit shared by the whole wave as in rs_histogram_kernel;
//                   a wave none of whose keys matches the prefix — nearly all of them from the second level on —
//                   touches no LDS.  One flush per workgroup into one of eight copies of the level's global bins.
//        tk_pick    one workgroup: sums the copies, finds the bin that holds the k-th key, appends its digit to the
//                   prefix and leaves k' = k - (keys in better bins).  When the bin is selected whole (k' == its count)
//                   the select is over: the remaining levels return at once on the header's `done` flag.
//      What is left in the header: the rows to take are those with x < lo, and the first r rows, in row order, with
//      lo <= x <= hi (lo == hi == the k-th key unless a level finished early; then r is the whole bin).
//   2. gather, in row order, per 4096-row SEGMENT (one wave's rows; a workgroup takes eight: a 32768-row chunk)
//        tk_count   one read: rows with x < lo and rows in [lo, hi] of every segment
//        tk_scan    one workgroup: per segment its first output position and the rows in [lo, hi] in front of it
//        tk_write   a wave re-reads its segment — only if the segment holds a selected row — ranks the rows with a wave
//                   scan and writes (x, row) at its rank among the selected rows: ascending row order, no atomics
//   3. order       sorted: dbhip_radix_sort_pairs_u32 (8-bit, stable: equal keys stay in row order) on the m pairs, in
//                   buffers and a sub-workspace carved from this workspace
//        tk_finish  removes the mask, writes out_keys / out_rows, folds the sort's status word into this one
//
// workspace: header | bins[8 copies][levels][radix] | cnt[segments] | pos[segments] | sel_keys[m] | sel_rows[m] |
//            tmp_keys[m] | tmp_rows[m] | the sort's workspace; every part at a 256-byte offset
#include <cstdlib>

#include "../../include/dbhip_topk.h"
#include "dbhip_common.hpp"

namespace dbhip {
namespace {

constexpr int kTkThreads = 512;
constexpr int kTkWaves = kTkThreads / kWave;
constexpr size_t kTkSegment = DBHIP_TOPK_SEGMENT_ROWS;  // rows of one wave in tk_count / tk_write
constexpr size_t kTkChunk = DBHIP_TOPK_CHUNK_ROWS;      // rows of one workgroup there
static_assert(kTkChunk == kTkSegment * kTkWaves, "a chunk is one segment per wave");
static_assert(kTkChunk % 8192 == 0, "a chunk is a whole number of the sort's tiles");
constexpr int kTkBinCopies = 8;  // copies of the global bins (radix.hip: what one copy costs)
constexpr int kTkMaxRadix = 2048;
constexpr int kTkPickThreads = 1024;
constexpr int kTkSortBits = 8;

struct TkHeader {
  unsigned status;
  unsigned prefix;  // the digits found so far, in place
  unsigned krem;    // rows still to take inside the prefix's bin
  unsigned done;    // lo, hi and r are final
  unsigned lo, hi;  // rows with x < lo are taken; of the rows with lo <= x <= hi ...
  unsigned r;       // ... the first r in row order
  unsigned pad[64 - 7];
};
static_assert(sizeof(TkHeader) == kWsHeader, "workspace header size");

// Digit width of the select: 11 (11/11/10 bits, three levels: three reads of the column) or 8 (four levels, four reads).
// Measured on uniform full-range keys, sorted output, both in the same visit (profiles/r12_topk.txt): at 2^26 rows the wide
// digits save the fourth read — k = 1: 227-230 us against 266-274, k = 1024: 249-253 against 289-292, k = 2^20: 377-382
// against 416-419, k = 2^16: 319-323 against 318-319 —, at 2^24 rows, where the column stays in the Infinity Cache, the
// two are within 5 % of each other either way.  DBHIP_TOPK_BITS=8 selects the narrow digits for measurements; the
// workspace is sized for either.
int tk_bits() {
  static const int bits = [] {
    const char *e = std::getenv("DBHIP_TOPK_BITS");
    return e && std::atoi(e) == 8 ? 8 : 11;
  }();
  return bits;
}
struct TkLevel {
  int shift, width;
};
inline int tk_levels(int bits) { return bits == 8 ? 4 : 3; }
inline TkLevel tk_level(int bits, int level) {
  if (bits == 8) return TkLevel{24 - 8 * level, 8};
  return level == 0 ? TkLevel{21, 11} : (level == 1 ? TkLevel{10, 11} : TkLevel{0, 10});
}

struct TkLayout {
  size_t segments, m;
  size_t bins, cnt, pos, sel_keys, sel_rows, tmp_keys, tmp_rows, sort_ws, sort_bytes, total;
};
inline TkLayout tk_layout(size_t n, size_t k) {
  TkLayout l;
  l.m = k < n ? k : n;
  l.segments = (n + kTkSegment - 1) / kTkSegment;
  l.bins = kWsHeader;
  l.cnt = l.bins + sizeof(unsigned) * kTkBinCopies * 3 * kTkMaxRadix;  // 11-bit digits: 3 x 2048; 8-bit: 4 x 256
  l.pos = l.cnt + align_up(l.segments * sizeof(u32x2), kWsAlign);
  l.sel_keys = l.pos + align_up(l.segments * sizeof(u32x2), kWsAlign);
  const size_t col = align_up(l.m * sizeof(unsigned), kWsAlign);
  l.sel_rows = l.sel_keys + col;
  l.tmp_keys = l.sel_rows + col;
  l.tmp_rows = l.tmp_keys + col;
  l.sort_ws = l.tmp_rows + col;
  l.sort_bytes = dbhip_radix_sort_pairs_workspace_bytes(l.m, kTkSortBits);
  l.total = align_up(l.sort_ws + l.sort_bytes, kWsAlign);
  return l;
}

// ---- 1. threshold ------------------------------------------------------------------------------------------------------
// LDS histogram in kCopies copies, lane l adding into copy l % kCopies, copy c lying c words further (radix.hip,
// rs_hist_copies: keys that crowd into a few digits otherwise queue on one LDS word)
template <int BITS>
__global__ __launch_bounds__(kTkThreads) void tk_hist_kernel(const unsigned *__restrict__ keys, size_t n, unsigned mask,
                                                             const TkHeader *hdr, int shift, unsigned digit_mask,
                                                             unsigned high_mask, unsigned *__restrict__ bins) {
  constexpr int kRadix = 1 << BITS;
  constexpr int kCopies = BITS == 8 ? 8 : 4, kStride = kRadix + 1;
  __shared__ unsigned s_hist[kCopies * kStride];
  if (hdr->done) return;  // uniform over the grid
  const unsigned prefix = hdr->prefix;
  for (int i = threadIdx.x; i < kCopies * kStride; i += kTkThreads) s_hist[i] = 0;
  __syncthreads();
  unsigned *hist = s_hist + (threadIdx.x & (kCopies - 1)) * kStride;
  // the digit of a key inside the prefix's bin, kRadix for a key outside it
  auto digit = [&](unsigned key) {
    const unsigned x = key ^ mask;
    return ((x ^ prefix) & high_mask) == 0 ? (x >> shift) & digit_mask : static_cast<unsigned>(kRadix);
  };
  auto count4 = [&](const u32x4 v) {
    const unsigned d[4] = {digit(v.x), digit(v.y), digit(v.z), digit(v.w)};
    const bool any = d[0] != kRadix || d[1] != kRadix || d[2] != kRadix || d[3] != kRadix;
    const unsigned long long active = __ballot(true);
    if (__ballot(any) == 0) return;  // no key of the wave in the bin
    // one digit in the whole wave (all keys equal, the upper bytes of keys in [1, 10000]): one lane adds the lot
    const unsigned first = __builtin_amdgcn_readfirstlane(d[0]);
    const bool same = d[0] == first && d[1] == first && d[2] == first && d[3] == first;
    if (first != kRadix && __ballot(same) == active) {
      if (lane_id() == static_cast<unsigned>(__builtin_ctzll(active)))
        atomicAdd(&hist[first], 4u * static_cast<unsigned>(__builtin_popcountll(active)));
      return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (d[c] != kRadix) atomicAdd(&hist[d[c]], 1u);
  };
  const size_t n4 = n / 4;
  const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys);  // 16-byte aligned (checked on the host)
  constexpr size_t kRound = 4 * kTkThreads;
  for (size_t base = static_cast<size_t>(blockIdx.x) * kRound; base < n4; base += static_cast<size_t>(gridDim.x) * kRound) {
    const size_t i = base + threadIdx.x;
    if (base + kRound <= n4) {  // four loads in flight per lane
      const u32x4 v0 = k4[i], v1 = k4[i + kTkThreads], v2 = k4[i + 2 * kTkThreads], v3 = k4[i + 3 * kTkThreads];
      count4(v0);
      count4(v1);
      count4(v2);
      count4(v3);
    } else {
      for (size_t j = i; j < n4; j += kTkThreads) count4(k4[j]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // the last one to three keys
    const unsigned d = digit(keys[n4 * 4 + threadIdx.x]);
    if (d != kRadix) atomicAdd(&hist[d], 1u);
  }
  __syncthreads();
  unsigned *copy = bins + static_cast<size_t>(blockIdx.x % kTkBinCopies) * kRadix;
  for (int d = threadIdx.x; d < kRadix; d += kTkThreads) {
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < kCopies; ++q) c += s_hist[q * kStride + d];
    if (c) atomicAdd(&copy[d], c);
  }
}

// one workgroup: the bin of this level that holds the k-th key
template <int BITS>
__global__ __launch_bounds__(kTkPickThreads) void tk_pick_kernel(TkHeader *hdr, const unsigned *__restrict__ bins, unsigned k,
                                                                 int first_level, int last_level, int shift) {
  constexpr int kRadix = 1 << BITS;
  constexpr int kPer = kRadix > kTkPickThreads ? kRadix / kTkPickThreads : 1;
  __shared__ unsigned s_wsum[kTkPickThreads / kWave];
  if (hdr->done) return;
  const unsigned need = first_level ? k : hdr->krem;  // 1 <= need <= the keys counted at this level
  const unsigned prefix = first_level ? 0u : hdr->prefix;
  unsigned c[kPer], mine = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const unsigned d = threadIdx.x * kPer + j;
    c[j] = 0;
    if (d < kRadix)
#pragma unroll
      for (int q = 0; q < kTkBinCopies; ++q) c[j] += bins[q * kRadix + d];
    mine += c[j];
  }
  unsigned total;
  unsigned run = block_exclusive_scan<kTkPickThreads>(mine, s_wsum, total);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (run < need && need - run <= c[j]) {  // exactly one bin of the workgroup
      const unsigned d = threadIdx.x * kPer + j;
      const unsigned p = prefix | (d << shift), left = need - run;
      hdr->prefix = p;
      hdr->krem = left;
      if (last_level || left == c[j]) {  // the k-th key itself, or a bin that is taken whole
        hdr->lo = p;
        hdr->hi = p | (shift ? (1u << shift) - 1u : 0u);
        hdr->r = left;
        hdr->done = 1u;
      }
    }
    run += c[j];
  }
}

// ---- 2. gather ---------------------------------------------------------------------------------------------------------
// rows with x < lo and rows with lo <= x <= hi of every segment; one wave per segment
__global__ __launch_bounds__(kTkThreads) void tk_count_kernel(const unsigned *__restrict__ keys, size_t n, unsigned mask,
                                                              const TkHeader *hdr, u32x2 *__restrict__ cnt,
                                                              size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kTkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const unsigned lo = hdr->lo, hi = hdr->hi;
  const size_t first = seg * kTkSegment;
  unsigned better = 0, equal = 0;
  auto count1 = [&](unsigned key) {
    const unsigned x = key ^ mask;
    better += x < lo ? 1u : 0u;
    equal += (x >= lo && x <= hi) ? 1u : 0u;
  };
  auto count4 = [&](const u32x4 v) {
    count1(v.x);
    count1(v.y);
    count1(v.z);
    count1(v.w);
  };
  if (first + kTkSegment <= n) {  // a whole segment: 16 loads of 16 bytes per lane, four in flight
    const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys + first) + lane;
#pragma unroll 1
    for (int i = 0; i < static_cast<int>(kTkSegment / 4 / kWave); i += 4) {
      const u32x4 v0 = k4[i * kWave], v1 = k4[(i + 1) * kWave], v2 = k4[(i + 2) * kWave], v3 = k4[(i + 3) * kWave];
      count4(v0);
      count4(v1);
      count4(v2);
      count4(v3);
    }
  } else {  // the ragged last segment
    for (size_t i = first + lane; i < n; i += kWave) count1(keys[i]);
  }
  better = wave_reduce_add(better);
  equal = wave_reduce_add(equal);
  if (lane == 0) cnt[seg] = u32x2{better, equal};
}

// one workgroup: cnt[segment] -> pos[segment] = {first output position, rows in [lo, hi] in front of the segment}
__global__ __launch_bounds__(kTkPickThreads) void tk_scan_kernel(const TkHeader *hdr, const u32x2 *__restrict__ cnt,
                                                                 u32x2 *__restrict__ pos, size_t segments) {
  __shared__ unsigned s_wsum[kTkPickThreads / kWave];
  const unsigned r = hdr->r;
  unsigned out_run = 0, eq_run = 0;  // totals of the rounds so far (the same in every thread)
  for (size_t base = 0; base < segments; base += kTkPickThreads) {
    const size_t seg = base + threadIdx.x;
    const u32x2 c = seg < segments ? cnt[seg] : u32x2{0u, 0u};
    unsigned eq_total, out_total;
    const unsigned eq_before = eq_run + block_exclusive_scan<kTkPickThreads>(c.y, s_wsum, eq_total);
    const unsigned room = eq_before < r ? r - eq_before : 0u;  // rows in [lo, hi] still to take from here on
    const unsigned take = c.x + (c.y < room ? c.y : room);
    const unsigned out_first = out_run + block_exclusive_scan<kTkPickThreads>(take, s_wsum, out_total);
    if (seg < segments) pos[seg] = u32x2{out_first, eq_before};
    eq_run += eq_total;
    out_run += out_total;
  }
}

// a wave writes its segment's selected rows, in row order, from pos[segment].x on
__global__ __launch_bounds__(kTkThreads) void tk_write_kernel(const unsigned *__restrict__ keys, size_t n, unsigned mask,
                                                              const TkHeader *hdr, const u32x2 *__restrict__ cnt,
                                                              const u32x2 *__restrict__ pos, size_t segments,
                                                              unsigned *__restrict__ sel_keys,
                                                              unsigned *__restrict__ sel_rows, size_t m) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kTkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const unsigned lo = hdr->lo, hi = hdr->hi, r = hdr->r;
  const u32x2 c = cnt[seg], p = pos[seg];
  const unsigned room = p.y < r ? r - p.y : 0u;
  const unsigned take = c.x + (c.y < room ? c.y : room);
  if (take == 0) return;  // nothing of the answer in this segment: it is not read again
  const size_t out_end = static_cast<size_t>(p.x) + take;
  if (out_end > m) return;  // cannot happen with counts of this column; nothing is ever written past the m entries
  size_t out = p.x;     // next output position (wave-uniform)
  unsigned eq_run = p.y;  // rows in [lo, hi] in front of the rows in hand (wave-uniform)
  const size_t first = seg * kTkSegment;
  const size_t last = first + kTkSegment < n ? first + kTkSegment : n;
  for (size_t base = first; base < last && out < out_end; base += 4 * kWave) {
    const size_t row0 = base + 4 * lane;  // this lane's four consecutive rows
    unsigned x[4];
    bool valid[4];
    if (row0 + 4 <= last) {
      const u32x4 v = *reinterpret_cast<const u32x4 *>(keys + row0);  // segment starts are multiples of 4096 rows
      x[0] = v.x ^ mask, x[1] = v.y ^ mask, x[2] = v.z ^ mask, x[3] = v.w ^ mask;
      valid[0] = valid[1] = valid[2] = valid[3] = true;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        valid[q] = row0 + q < last;
        x[q] = valid[q] ? keys[row0 + q] ^ mask : 0u;
      }
    }
    bool sel[4], eq[4];
    unsigned n_eq = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sel[q] = valid[q] && x[q] < lo;
      eq[q] = valid[q] && x[q] >= lo && x[q] <= hi;
      n_eq += eq[q] ? 1u : 0u;
    }
    if (__ballot(n_eq != 0) != 0) {  // rows in [lo, hi]: taken while their rank among all such rows is below r
      const unsigned incl = wave_inclusive_scan(n_eq);
      unsigned rank = eq_run + incl - n_eq;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (eq[q]) {
          sel[q] = rank < r;
          ++rank;
        }
      }
      eq_run += __builtin_amdgcn_readlane(incl, kWave - 1);
    }
    const unsigned n_sel = (sel[0] ? 1u : 0u) + (sel[1] ? 1u : 0u) + (sel[2] ? 1u : 0u) + (sel[3] ? 1u : 0u);
    if (__ballot(n_sel != 0) == 0) continue;
    const unsigned incl = wave_inclusive_scan(n_sel);
    size_t at = out + incl - n_sel;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (sel[q] && at < out_end) {
        sel_keys[at] = x[q];
        sel_rows[at] = static_cast<unsigned>(row0 + q);
        ++at;
      }
    }
    out += __builtin_amdgcn_readlane(incl, kWave - 1);
  }
}

// ---- 3. the outputs ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTkThreads) void tk_finish_kernel(const unsigned *__restrict__ sel_keys,
                                                               const unsigned *__restrict__ sel_rows, size_t m, unsigned mask,
                                                               unsigned *__restrict__ out_keys, unsigned *__restrict__ out_rows,
                                                               TkHeader *hdr, const unsigned *sort_status) {
  if (sort_status && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned st = *sort_status;
    if (st) atomicOr(&hdr->status, st);
  }
  const size_t stride = static_cast<size_t>(gridDim.x) * kTkThreads;
  const size_t first = static_cast<size_t>(blockIdx.x) * kTkThreads + threadIdx.x;
  const size_t m4 = m / 4;  // all four columns are 16-byte aligned
  const u32x4 *k4 = reinterpret_cast<const u32x4 *>(sel_keys), *r4 = reinterpret_cast<const u32x4 *>(sel_rows);
  u32x4 *ok4 = reinterpret_cast<u32x4 *>(out_keys), *or4 = reinterpret_cast<u32x4 *>(out_rows);
  for (size_t i = first; i < m4; i += stride) {
    const u32x4 v = k4[i];
    ok4[i] = u32x4{v.x ^ mask, v.y ^ mask, v.z ^ mask, v.w ^ mask};
    or4[i] = r4[i];
  }
  if (blockIdx.x == 0 && threadIdx.x < (m & 3)) {
    out_keys[m4 * 4 + threadIdx.x] = sel_keys[m4 * 4 + threadIdx.x] ^ mask;
    out_rows[m4 * 4 + threadIdx.x] = sel_rows[m4 * 4 + threadIdx.x];
  }
}

template <int BITS>
int topk_impl(const unsigned *keys, size_t n, size_t m, unsigned mask, int sorted, unsigned *out_keys, unsigned *out_rows,
              void *workspace, const TkLayout &l, hipStream_t s, const DeviceInfo &dev) {
  constexpr int kRadix = 1 << BITS;
  char *base = static_cast<char *>(workspace);
  TkHeader *hdr = reinterpret_cast<TkHeader *>(base);
  unsigned *bins = reinterpret_cast<unsigned *>(base + l.bins);
  u32x2 *cnt = reinterpret_cast<u32x2 *>(base + l.cnt);
  u32x2 *pos = reinterpret_cast<u32x2 *>(base + l.pos);
  unsigned *sel_keys = reinterpret_cast<unsigned *>(base + l.sel_keys);
  unsigned *sel_rows = reinterpret_cast<unsigned *>(base + l.sel_rows);
  const int levels = tk_levels(BITS);
  const size_t level_bins = static_cast<size_t>(kTkBinCopies) * kRadix;  // words of one level's bins, all copies
  const hipError_t e = fill_async(workspace, 0, kWsHeader + sizeof(unsigned) * level_bins * levels, s);
  if (e != hipSuccess) return static_cast<int>(e);

  const unsigned hist_grid = capped_grid(n / 4, 4 * kTkThreads, dev, 4);
  for (int lv = 0; lv < levels; ++lv) {
    const TkLevel t = tk_level(BITS, lv);
    const unsigned digit_mask = (1u << t.width) - 1u;
    const unsigned high_mask = t.shift + t.width >= 32 ? 0u : ~0u << (t.shift + t.width);
    hipLaunchKernelGGL((tk_hist_kernel<BITS>), dim3(hist_grid), dim3(kTkThreads), 0, s, keys, n, mask, hdr, t.shift,
                       digit_mask, high_mask, bins + level_bins * lv);
    hipLaunchKernelGGL((tk_pick_kernel<BITS>), dim3(1), dim3(kTkPickThreads), 0, s, hdr, bins + level_bins * lv,
                       static_cast<unsigned>(m), lv == 0 ? 1 : 0, lv == levels - 1 ? 1 : 0, t.shift);
  }
  const unsigned seg_grid = static_cast<unsigned>((l.segments + kTkWaves - 1) / kTkWaves);
  hipLaunchKernelGGL(tk_count_kernel, dim3(seg_grid), dim3(kTkThreads), 0, s, keys, n, mask, hdr, cnt, l.segments);
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(kTkPickThreads), 0, s, hdr, cnt, pos, l.segments);
  hipLaunchKernelGGL(tk_write_kernel, dim3(seg_grid), dim3(kTkThreads), 0, s, keys, n, mask, hdr, cnt, pos, l.segments,
                     sel_keys, sel_rows, m);
  const unsigned *sort_status = nullptr;
  if (sorted) {
    const int rc = dbhip_radix_sort_pairs_u32(sel_keys, sel_rows, reinterpret_cast<unsigned *>(base + l.tmp_keys),
                                              reinterpret_cast<unsigned *>(base + l.tmp_rows), m, kTkSortBits, 0,
                                              base + l.sort_ws, l.sort_bytes, s);
    if (rc != DBHIP_OK) return rc;
    sort_status = reinterpret_cast<const unsigned *>(base + l.sort_ws);
  }
  hipLaunchKernelGGL(tk_finish_kernel, dim3(capped_grid(m / 4, kTkThreads, dev, 4)), dim3(kTkThreads), 0, s, sel_keys, sel_rows, m, mask, out_keys, out_rows,
                     hdr, sort_status);
  return launch_status();
}

int topk_entry(const unsigned *keys, size_t n, size_t k, unsigned mask, int sorted, unsigned *out_keys, unsigned *out_rows,
               void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  if (n >= (1ull << 32)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  const size_t m = k < n ? k : n;
  if (n && !keys) return DBHIP_EINVAL;
  if (m && (!out_keys || !out_rows)) return DBHIP_EINVAL;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(out_keys) |
                         reinterpret_cast<uintptr_t>(out_rows);
  if (addr & 15u) return DBHIP_EINVAL;  // dbhip_topk.h: 16-byte aligned
  if (m == 0) {  // nothing to select; a workspace that was passed still gets a clean status word
    if (!workspace) return DBHIP_OK;
    if (!ws_ok(workspace, workspace_bytes, kWsHeader)) return DBHIP_EWORKSPACE;
    return static_cast<int>(fill_async(workspace, 0, kWsHeader, as_stream(stream)));
  }
  const TkLayout l = tk_layout(n, k);
  if (!ws_ok(workspace, workspace_bytes, l.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  return tk_bits() == 8
             ? topk_impl<8>(keys, n, m, mask, sorted, out_keys, out_rows, workspace, l, as_stream(stream), dev)
             : topk_impl<11>(keys, n, m, mask, sorted, out_keys, out_rows, workspace, l, as_stream(stream), dev);
}

// ---- the validator -----------------------------------------------------------------------------------------------------
constexpr int kTkCheckThreads = 256;

__device__ __forceinline__ bool tk_precedes(unsigned xa, unsigned ra, unsigned xb, unsigned rb) {
  return xa < xb || (xa == xb && ra < rb);
}

__global__ __launch_bounds__(kTkCheckThreads) void tk_check_kernel(const unsigned *__restrict__ keys, size_t n,
                                                                   const unsigned *__restrict__ out_keys,
                                                                   const unsigned *__restrict__ out_rows, size_t m,
                                                                   unsigned mask, unsigned long long *result) {
  __shared__ unsigned long long s_part[2][kTkCheckThreads / kWave];
  const size_t stride = static_cast<size_t>(gridDim.x) * kTkCheckThreads;
  const size_t first = static_cast<size_t>(blockIdx.x) * kTkCheckThreads + threadIdx.x;
  unsigned long long wrong = 0, before = 0;
  for (size_t i = first; i < m; i += stride) {
    const unsigned k = out_keys[i], row = out_rows[i];
    bool bad = row >= n || keys[row] != k;
    if (i > 0) bad = bad || !tk_precedes(out_keys[i - 1] ^ mask, out_rows[i - 1], k ^ mask, row);
    wrong += bad ? 1u : 0u;
  }
  const unsigned last_x = out_keys[m - 1] ^ mask, last_row = out_rows[m - 1];  // two values: the row is not dereferenced
  for (size_t i = first; i < n; i += stride)
    before += tk_precedes(keys[i] ^ mask, static_cast<unsigned>(i), last_x, last_row) ? 1u : 0u;
  wrong = wave_reduce_add_u64(wrong);
  before = wave_reduce_add_u64(before);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_part[0][threadIdx.x / kWave] = wrong;
    s_part[1][threadIdx.x / kWave] = before;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kTkCheckThreads / kWave; ++w) sum += s_part[threadIdx.x][w];
    if (sum) atomicAdd(result + threadIdx.x, sum);
  }
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_topk_workspace_bytes(size_t n, size_t k) {
  if (n >= (1ull << 32)) return 0;
  return tk_layout(n, k).total;
}

extern "C" int dbhip_topk_u32(const uint32_t *keys, size_t n, size_t k, int largest, int sorted, uint32_t *out_keys,
                              uint32_t *out_rows, void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  return topk_entry(keys, n, k, largest ? 0xFFFFFFFFu : 0u, sorted, out_keys, out_rows, workspace, workspace_bytes, stream);
}

extern "C" int dbhip_topk_i32(const int32_t *keys, size_t n, size_t k, int largest, int sorted, int32_t *out_keys,
                              uint32_t *out_rows, void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  // signed order = unsigned order with the sign bit flipped (radix.hip)
  return topk_entry(reinterpret_cast<const unsigned *>(keys), n, k, largest ? 0x7FFFFFFFu : 0x80000000u, sorted,
                    reinterpret_cast<unsigned *>(out_keys), out_rows, workspace, workspace_bytes, stream);
}

extern "C" int dbhip_check_topk_u32(const uint32_t *keys, size_t n, const uint32_t *out_keys, const uint32_t *out_rows,
                                    size_t k, int largest, int is_signed, uint64_t *result, dbhip_stream_t stream) {
  if (!result || n >= (1ull << 32) || (n && !keys)) return DBHIP_EINVAL;
  const size_t m = k < n ? k : n;
  if (m && (!out_keys || !out_rows)) return DBHIP_EINVAL;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  const hipError_t e = fill_async(result, 0, 2 * sizeof(uint64_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  if (m == 0) return DBHIP_OK;
  const unsigned grid = capped_grid(n, kTkCheckThreads, dev);  // m <= n
  const unsigned mask = (is_signed ? 0x80000000u : 0u) ^ (largest ? 0xFFFFFFFFu : 0u);
  hipLaunchKernelGGL(tk_check_kernel, dim3(grid), dim3(kTkCheckThreads), 0, s, keys, n, out_keys, out_rows, m, mask,
                     reinterpret_cast<unsigned long long *>(result));
  return launch_status();
}
