// join_pairs.hip — materialise the (build row, probe row) pairs of a one-to-many join answer (no reference counterpart:
// the reference stops at OmniSci::HashTable::lookup's {pointer, size} record, common/dpcpp/omnisci_hashtable.hpp:12-17).
//
// Input: (ids, pos, cnt [, probe_row_ids]) of dbhip_join_probe_u32 or dbhip_join_radix_match_u32.  With e[i] = cnt[i]
// (inner) or max(cnt[i], 1) (left outer) and off = the 64-bit exclusive prefix sum of e, pair number off[i] + k is
// (ids[pos[i] + k], rid(i)); see include/dbhip.h.  Four dependent launches, no workgroup waits on another:
//   jp_sums     one workgroup per chunk of probe rows: the chunk's sum of e (64 bits); a row whose id range leaves the id
//               buffer counts as empty and raises DBHIP_DEV_KEY_RANGE
//   jp_offsets  one workgroup: exclusive scan of the <= 4096 chunk sums; the total goes to the workspace header and to
//               *out_pairs, DBHIP_DEV_TABLE_FULL when it exceeds the capacity.  A count-only call ends here.
//   jp_scan     one workgroup per chunk: off[i] (64 bits) into the workspace
//   jp_expand   a fixed grid, partitioned by OUTPUT.  The unit of work is an item: every probe row is one item, followed by
//               one item per pair of that row, so row i's item has number i + off[i] (strictly increasing) and there are
//               n_probe + written items.  Each workgroup takes an equal, contiguous run of 2048-item chunks.  A chunk
//               therefore holds at most 2048 pairs AND touches at most 2049 rows whatever the counts are: a row with
//               2^26 matches is spread over 2^15 chunks, a million rows without a match cost 512 chunks of staging and no
//               loop each, and the rows of a chunk always fit in LDS (a partition by pair number alone would have to
//               walk an unbounded run of empty rows between two pairs).  Per chunk: the number of row items below the
//               chunk's end by a 256-ary search in off[] (all 256 lanes probe at once: three rounds for 2^24 rows from
//               nothing, two from the previous chunk's answer), the covered rows' (first pair, id position, row id)
//               staged in LDS, and then every lane takes four consecutive pair numbers, finds their rows by binary
//               search in LDS and writes both columns with one 16-byte store each when the columns allow it (4-byte
//               stores, still in pair order, otherwise).  ids is read at consecutive positions inside a row's range.
// HBM bytes per call, P pairs written, n probe rows: 8 P written + 4 P ids read + 8 n (cnt, pos: jp_sums) + 8 n + 8 n
// written (jp_scan) + 8 n + 12 n read (off, pos, cnt, row ids: jp_expand) = 12 P + 44 n (40 n without a row id column).
#include "dbhip_common.hpp"

namespace dbhip {
namespace {

typedef unsigned long long u64;

constexpr int kJpThreads = 256;
constexpr int kJpWaves = kJpThreads / kWave;
constexpr size_t kJpTile = static_cast<size_t>(kJpThreads) * 4;  // rows per workgroup step of the scan kernels
constexpr size_t kJpMaxChunks = 4096;
#ifndef DBHIP_JP_ITEMS
#define DBHIP_JP_ITEMS 2048  // tools/build_variant.sh: other chunk sizes for A/B runs
#endif
constexpr unsigned kJpItems = DBHIP_JP_ITEMS;  // items (rows + pairs) per expansion chunk
constexpr unsigned kJpLdsBytes = 3 * (kJpItems + 1) * sizeof(unsigned);
constexpr unsigned kJpPerCu = 160 * 1024 / kJpLdsBytes < 8 ? 160 * 1024 / kJpLdsBytes : 8;  // resident workgroups per CU
constexpr unsigned kJpSentinel = 0xFFFFFFFFu;

struct JpHeader {
  unsigned status, pad0;
  u64 total;    // sum of e
  u64 written;  // min(total, capacity)
  unsigned pad[58];
};
static_assert(sizeof(JpHeader) == kWsHeader, "workspace header size");

struct JpLayout {
  size_t chunk_rows, chunks, off_at, total;
};
inline JpLayout jp_layout(size_t n) {
  JpLayout L;
  size_t per = (n + kJpMaxChunks - 1) / kJpMaxChunks;
  per = (per + kJpTile - 1) / kJpTile * kJpTile;
  L.chunk_rows = per ? per : kJpTile;
  L.chunks = (n + L.chunk_rows - 1) / L.chunk_rows;
  L.off_at = kWsHeader + align_up(kJpMaxChunks * sizeof(u64), kWsAlign);
  L.total = align_up(L.off_at + (n ? n : 1) * sizeof(u64), kWsAlign);
  return L;
}

__device__ __forceinline__ u64 wave_inclusive_scan_u64(u64 v, unsigned lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const u64 up = __shfl_up(v, d, kWave);
    v += lane >= static_cast<unsigned>(d) ? up : 0ull;
  }
  return v;
}

// e of four consecutive rows from `first` on (rows at or above hi: 0).  A row whose range leaves ids[0..n_build) is empty.
__device__ __forceinline__ void jp_load4(const unsigned *__restrict__ pos, const unsigned *__restrict__ cnt, size_t first,
                                         size_t hi, u64 n_build, bool left_outer, bool aligned, unsigned e[4], bool &bad) {
  u32x4 p = u32x4{0, 0, 0, 0}, c = u32x4{0, 0, 0, 0};
  if (aligned && first + 4 <= hi) {
    p = *reinterpret_cast<const u32x4 *>(pos + first);
    c = *reinterpret_cast<const u32x4 *>(cnt + first);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (first + j < hi) {
        p[j] = pos[first + j];
        c[j] = cnt[first + j];
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = first + j < hi;
    const bool ok = static_cast<u64>(p[j]) + c[j] <= n_build;
    bad |= in && !ok;
    const unsigned ce = ok ? c[j] : 0u;
    e[j] = in ? (left_outer && ce == 0 ? 1u : ce) : 0u;
  }
}

__global__ __launch_bounds__(kJpThreads) void jp_sums_kernel(const unsigned *__restrict__ pos,
                                                             const unsigned *__restrict__ cnt, size_t n, size_t chunk_rows,
                                                             u64 n_build, int left_outer, int aligned,
                                                             u64 *__restrict__ sums, JpHeader *hdr) {
  __shared__ u64 s_w[kJpWaves];
  __shared__ unsigned s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const size_t lo = static_cast<size_t>(blockIdx.x) * chunk_rows;
  size_t hi = lo + chunk_rows;
  hi = hi < n ? hi : n;
  u64 acc = 0;
  bool bad = false;
  for (size_t r = lo + static_cast<size_t>(threadIdx.x) * 4; r < hi; r += kJpTile) {
    unsigned e[4];
    jp_load4(pos, cnt, r, hi, n_build, left_outer != 0, aligned != 0, e, bad);
    acc += static_cast<u64>(e[0]) + e[1] + e[2] + e[3];
  }
  acc = wave_reduce_add_u64(acc);
  if (bad) s_bad = 1;
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 s = 0;
#pragma unroll
    for (int w = 0; w < kJpWaves; ++w) s += s_w[w];
    sums[blockIdx.x] = s;
    if (s_bad) atomicOr(&hdr->status, DBHIP_DEV_KEY_RANGE);
  }
}

// exclusive scan of the chunk sums in place; total, written and the capacity verdict
__global__ __launch_bounds__(1024) void jp_offsets_kernel(u64 *sums, unsigned chunks, u64 capacity, int count_only,
                                                          JpHeader *hdr, u64 *out_pairs) {
  __shared__ u64 s_w[1024 / kWave];
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  u64 c[4], mine = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned i = tid * 4 + j;
    c[j] = i < chunks ? sums[i] : 0ull;
    mine += c[j];
  }
  const u64 incl = wave_inclusive_scan_u64(mine, lane);
  if (lane == kWave - 1) s_w[wave] = incl;
  __syncthreads();
  u64 run = incl - mine, total = 0;
  for (unsigned w = 0; w < 1024 / kWave; ++w) {
    const u64 t = s_w[w];
    run += w < wave ? t : 0ull;
    total += t;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned i = tid * 4 + j;
    if (i < chunks) sums[i] = run;
    run += c[j];
  }
  if (tid == 0) {
    hdr->total = total;
    hdr->written = total < capacity ? total : capacity;
    *out_pairs = total;
    if (total > capacity && !count_only) atomicOr(&hdr->status, DBHIP_DEV_TABLE_FULL);
  }
}

__global__ __launch_bounds__(kJpThreads) void jp_scan_kernel(const unsigned *__restrict__ pos,
                                                             const unsigned *__restrict__ cnt, size_t n, size_t chunk_rows,
                                                             u64 n_build, int left_outer, int aligned,
                                                             const u64 *__restrict__ bases, u64 *__restrict__ off) {
  __shared__ u64 s_w[2][kJpWaves];
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t lo = static_cast<size_t>(blockIdx.x) * chunk_rows;
  size_t hi = lo + chunk_rows;
  hi = hi < n ? hi : n;
  u64 running = bases[blockIdx.x];
  unsigned par = 0;
  bool bad = false;
  for (size_t base = lo; base < hi; base += kJpTile, par ^= 1u) {
    const size_t r = base + static_cast<size_t>(tid) * 4;
    unsigned e[4];
    jp_load4(pos, cnt, r, hi, n_build, left_outer != 0, aligned != 0, e, bad);
    const u64 mine = static_cast<u64>(e[0]) + e[1] + e[2] + e[3];
    const u64 incl = wave_inclusive_scan_u64(mine, lane);
    if (lane == kWave - 1) s_w[par][wave] = incl;
    __syncthreads();  // two slots alternate with the tile parity: one barrier per tile
    u64 excl = running + incl - mine, tile_total = 0;
#pragma unroll
    for (int w = 0; w < kJpWaves; ++w) {
      const u64 t = s_w[par][w];
      excl += w < static_cast<int>(wave) ? t : 0ull;
      tile_total += t;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (r + j < hi) off[r + j] = excl;
      excl += e[j];
    }
    running += tile_total;
  }
}

// Number of rows i in [lo, hi) with i + off[i] < d, plus lo: every row below lo is known to satisfy it, every row from hi
// on not to.  All 256 lanes probe the ends of 256 equal pieces at once, so a round divides the range by 256.  Uniform.
__device__ __forceinline__ size_t jp_rows_below(const u64 *__restrict__ off, size_t lo, size_t hi, u64 d) {
  while (lo < hi) {  // uniform
    const size_t step = (hi - lo + kJpThreads - 1) / kJpThreads;
    const size_t idx = lo + (static_cast<size_t>(threadIdx.x) + 1) * step - 1;
    const int below = idx < hi && idx + off[idx] < d;
    const size_t c = static_cast<size_t>(__syncthreads_count(below));  // the predicate is monotone: a prefix of the lanes
    lo += c * step;
    const size_t cap = lo + step - 1;  // the probe that failed, or the end of the range
    hi = cap < hi ? cap : hi;
  }
  return lo;
}

__global__ __launch_bounds__(kJpThreads) void jp_expand_kernel(const unsigned *__restrict__ ids,
                                                               const unsigned *__restrict__ rid_in,
                                                               const unsigned *__restrict__ pos,
                                                               const unsigned *__restrict__ cnt, size_t n, u64 n_build,
                                                               int left_outer, const JpHeader *__restrict__ hdr,
                                                               const u64 *__restrict__ off, unsigned *__restrict__ out_b,
                                                               unsigned *__restrict__ out_p, int phase) {
  __shared__ unsigned s_rel[kJpItems + 1], s_src[kJpItems + 1], s_rid[kJpItems + 1];
  const u64 written = hdr->written;
  if (written == 0) return;
  const u64 items = n + written;
  const u64 num_chunks = (items + kJpItems - 1) / kJpItems;
  const u64 per_wg = (num_chunks + gridDim.x - 1) / gridDim.x;
  u64 chunk = per_wg * blockIdx.x;
  u64 chunk_end = chunk + per_wg;
  chunk_end = chunk_end < num_chunks ? chunk_end : num_chunks;
  if (chunk >= chunk_end) return;
  size_t q0 = jp_rows_below(off, 0, n, chunk * kJpItems);  // row items in front of this workgroup's first chunk
  for (; chunk < chunk_end; ++chunk) {
    const u64 d0 = chunk * kJpItems;
    u64 d1 = d0 + kJpItems;
    d1 = d1 < items ? d1 : items;
    const size_t reach = q0 + kJpItems;  // a chunk holds at most kJpItems row items
    const size_t q1 = jp_rows_below(off, q0, reach < n ? reach : n, d1);
    const u64 k0 = d0 - q0;  // pair items in front of the chunk
    if (k0 >= written) return;  // uniform; k0 only grows
    u64 k1 = d1 - q1;
    k1 = k1 < written ? k1 : written;
    // the chunk's pairs belong to rows q0 - 1 (a row that began in front of the chunk) .. q1 - 1
    const size_t ra = q0 ? q0 - 1 : 0;
    const unsigned nr = static_cast<unsigned>(q1 - ra);  // <= kJpItems + 1
    if (k1 > k0 && nr) {
      for (unsigned j = threadIdx.x; j < nr; j += kJpThreads) {
        const size_t r = ra + j;
        const u64 o = off[r];
        const unsigned p = pos[r], c = cnt[r];
        const bool ok = static_cast<u64>(p) + c <= n_build;
        const bool sentinel = !ok || c == 0;  // only reached by a pair number in left-outer mode
        // only the first staged row can begin in front of the chunk: it is entered at the pair the chunk begins with
        s_rel[j] = o >= k0 ? static_cast<unsigned>(o - k0) : 0u;
        s_src[j] = sentinel ? kJpSentinel : (o >= k0 ? p : p + static_cast<unsigned>(k0 - o));
        s_rid[j] = rid_in ? rid_in[r] : static_cast<unsigned>(r);
      }
      __syncthreads();
      const unsigned m = static_cast<unsigned>(k1 - k0);  // pairs of this chunk, <= kJpItems
      // groups of four pair numbers that start where both columns are 16-byte aligned (phase < 4), else anywhere
      const unsigned lead = phase < 4 ? static_cast<unsigned>((k0 + phase) & 3u) : 0u;
      for (unsigned g = threadIdx.x * 4; g < m + lead; g += kJpThreads * 4) {
        unsigned b[4], pr[4];
        unsigned j = 0;
        bool have = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned xi = g + u;
          b[u] = 0;
          pr[u] = 0;
          if (xi >= lead && xi - lead < m) {
            const unsigned x = xi - lead;
            if (!have || (j + 1 < nr && s_rel[j + 1] <= x)) {  // not the row of the pair before: largest j, s_rel[j] <= x
              unsigned lo = have ? j + 1 : 0, len = nr - lo;
              while (len > 1) {
                const unsigned half = len >> 1;
                const bool right = s_rel[lo + half] <= x;
                lo += right ? half : 0u;
                len -= half;
              }
              j = lo;
              have = true;
            }
            const unsigned src = s_src[j];
            b[u] = src == kJpSentinel ? kJpSentinel : ids[src + (x - s_rel[j])];
            pr[u] = s_rid[j];
          }
        }
        const bool full = g >= lead && g - lead + 4 <= m;
        const u64 k = k0 + g - lead;  // pair number of the group's first member (meaningful for g >= lead)
        if (phase < 4 && full) {
          *reinterpret_cast<u32x4 *>(out_b + k) = u32x4{b[0], b[1], b[2], b[3]};
          *reinterpret_cast<u32x4 *>(out_p + k) = u32x4{pr[0], pr[1], pr[2], pr[3]};
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const unsigned xi = g + u;
            if (xi >= lead && xi - lead < m) {
              out_b[k0 + (xi - lead)] = b[u];
              out_p[k0 + (xi - lead)] = pr[u];
            }
          }
        }
      }
      __syncthreads();  // the staged rows are no longer read
    }
    q0 = q1;
  }
}

__global__ void jp_zero_kernel(u64 *out_pairs) { *out_pairs = 0; }

// ---- validator ---------------------------------------------------------------------------------------------------
constexpr int kJpCkThreads = 256;

__device__ __forceinline__ u64 jp_mix(unsigned b, unsigned p) { return mix64(0, (static_cast<u64>(p) << 32) | b); }

__device__ __forceinline__ void jp_add(u64 *dst, u64 v) {
  v = wave_reduce_add_u64(v);
  if (lane_id() == 0 && v) atomicAdd(reinterpret_cast<u64 *>(dst), v);
}

// the pairs given: result[0] += bad pairs, result[2] += fingerprint
__global__ __launch_bounds__(kJpCkThreads) void jp_check_given_kernel(const unsigned *__restrict__ build_keys, u64 n_build,
                                                                      const unsigned *__restrict__ probe_keys, u64 n_probe,
                                                                      int left_outer, const unsigned *__restrict__ out_b,
                                                                      const unsigned *__restrict__ out_p, u64 n_pairs,
                                                                      u64 *result) {
  u64 bad = 0, fp = 0;
  const u64 stride = static_cast<u64>(gridDim.x) * kJpCkThreads;
  for (u64 k = static_cast<u64>(blockIdx.x) * kJpCkThreads + threadIdx.x; k < n_pairs; k += stride) {
    const unsigned b = out_b[k], p = out_p[k];
    fp += jp_mix(b, p);
    if (p >= n_probe)
      ++bad;
    else if (b == kJpSentinel)
      bad += left_outer ? 0 : 1;
    else if (b >= n_build || build_keys[b] != probe_keys[p])
      ++bad;
  }
  jp_add(result + 0, bad);
  jp_add(result + 2, fp);
}

// the pairs expected: one thread walks one probe row's id range.  result[1] += pairs, result[3] += fingerprint
__global__ __launch_bounds__(kJpCkThreads) void jp_check_expected_kernel(const unsigned *__restrict__ ids, u64 n_build,
                                                                         const unsigned *__restrict__ rid_in,
                                                                         const unsigned *__restrict__ pos,
                                                                         const unsigned *__restrict__ cnt, u64 n_probe,
                                                                         int left_outer, u64 *result) {
  u64 pairs = 0, fp = 0;
  const u64 stride = static_cast<u64>(gridDim.x) * kJpCkThreads;
  for (u64 i = static_cast<u64>(blockIdx.x) * kJpCkThreads + threadIdx.x; i < n_probe; i += stride) {
    const unsigned p = pos[i];
    unsigned c = cnt[i];
    if (static_cast<u64>(p) + c > n_build) c = 0;
    const unsigned rid = rid_in ? rid_in[i] : static_cast<unsigned>(i);
    for (unsigned k = 0; k < c; ++k) fp += jp_mix(ids[p + k], rid);
    pairs += c;
    if (c == 0 && left_outer) {
      fp += jp_mix(kJpSentinel, rid);
      ++pairs;
    }
  }
  jp_add(result + 1, pairs);
  jp_add(result + 3, fp);
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_join_pairs_workspace_bytes(size_t n_probe) {
  if (static_cast<u64>(n_probe) >= (1ull << 32)) return 0;
  return jp_layout(n_probe).total;
}

extern "C" int dbhip_join_pairs_u32(const uint32_t *ids, size_t n_build, const uint32_t *probe_row_ids, const uint32_t *pos,
                                    const uint32_t *cnt, size_t n_probe, int left_outer, uint64_t capacity,
                                    uint32_t *out_build_rows, uint32_t *out_probe_rows, uint64_t *out_pairs, void *workspace,
                                    size_t workspace_bytes, dbhip_stream_t stream) {
  if (static_cast<u64>(n_probe) >= (1ull << 32) || static_cast<u64>(n_build) > (1ull << 31)) return DBHIP_EINVAL;
  if (capacity && (!out_build_rows || !out_probe_rows)) return DBHIP_EINVAL;
  if (n_probe && ((n_build && !ids) || !pos || !cnt || !out_pairs || !workspace)) return DBHIP_EINVAL;
  if ((n_probe || workspace) && !ws_ok(workspace, workspace_bytes, dbhip_join_pairs_workspace_bytes(n_probe)))
    return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  if (workspace) {
    const hipError_t e = fill_async(workspace, 0, kWsHeader, s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (n_probe == 0) {
    if (out_pairs) hipLaunchKernelGGL(jp_zero_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<u64 *>(out_pairs));
    return launch_status();
  }
  const JpLayout L = jp_layout(n_probe);
  char *base = static_cast<char *>(workspace);
  JpHeader *hdr = reinterpret_cast<JpHeader *>(base);
  u64 *sums = reinterpret_cast<u64 *>(base + kWsHeader);
  u64 *off = reinterpret_cast<u64 *>(base + L.off_at);
  const int aligned = ((reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(cnt)) & 15u) == 0;
  const int count_only = capacity == 0 && !out_build_rows && !out_probe_rows;
  const unsigned chunks = static_cast<unsigned>(L.chunks);
  hipLaunchKernelGGL(jp_sums_kernel, dim3(chunks), dim3(kJpThreads), 0, s, pos, cnt, n_probe, L.chunk_rows,
                     static_cast<u64>(n_build), left_outer, aligned, sums, hdr);
  hipLaunchKernelGGL(jp_offsets_kernel, dim3(1), dim3(1024), 0, s, sums, chunks, static_cast<u64>(capacity), count_only, hdr,
                     reinterpret_cast<u64 *>(out_pairs));
  if (capacity == 0) return launch_status();  // nothing can be written
  hipLaunchKernelGGL(jp_scan_kernel, dim3(chunks), dim3(kJpThreads), 0, s, pos, cnt, n_probe, L.chunk_rows,
                     static_cast<u64>(n_build), left_outer, aligned, sums, off);
  // 16-byte stores when both columns sit at the same distance from a 16-byte boundary: phase = that distance in words
  const unsigned pb = static_cast<unsigned>(reinterpret_cast<uintptr_t>(out_build_rows) >> 2) & 3u;
  const unsigned pp = static_cast<unsigned>(reinterpret_cast<uintptr_t>(out_probe_rows) >> 2) & 3u;
  const int phase = pb == pp ? static_cast<int>(pb) : 4;
  const u64 cap_items = capacity < (1ull << 62) ? capacity : (1ull << 62);
  const u64 max_chunks = (static_cast<u64>(n_probe) + cap_items + kJpItems - 1) / kJpItems;
  const u64 resident = static_cast<u64>(dev.cus) * kJpPerCu;  // as many as the staged rows in LDS admit
  const unsigned grid = static_cast<unsigned>(max_chunks < resident ? max_chunks : resident);
  hipLaunchKernelGGL(jp_expand_kernel, dim3(grid), dim3(kJpThreads), 0, s, ids, probe_row_ids, pos, cnt, n_probe,
                     static_cast<u64>(n_build), left_outer, hdr, off, out_build_rows, out_probe_rows, phase);
  return launch_status();
}

extern "C" int dbhip_check_join_pairs_u32(const uint32_t *build_keys, size_t n_build, const uint32_t *probe_keys,
                                          size_t n_probe, const uint32_t *ids, const uint32_t *probe_row_ids,
                                          const uint32_t *pos, const uint32_t *cnt, int left_outer,
                                          const uint32_t *out_build_rows, const uint32_t *out_probe_rows, uint64_t n_pairs,
                                          uint64_t *result, dbhip_stream_t stream) {
  if (!result || (n_probe && (!probe_keys || !pos || !cnt)) || (n_build && (!build_keys || !ids)) ||
      (n_pairs && (!out_build_rows || !out_probe_rows)))
    return DBHIP_EINVAL;
  if (static_cast<u64>(n_probe) >= (1ull << 32) || static_cast<u64>(n_build) > (1ull << 31)) return DBHIP_EINVAL;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  const hipError_t e = fill_async(result, 0, 4 * sizeof(uint64_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  const u64 cap = static_cast<u64>(dev.cus) * 8;
  if (n_pairs) {
    const u64 want = (n_pairs + kJpCkThreads - 1) / kJpCkThreads;
    hipLaunchKernelGGL(jp_check_given_kernel, dim3(static_cast<unsigned>(want < cap ? want : cap)), dim3(kJpCkThreads), 0, s,
                       build_keys, static_cast<u64>(n_build), probe_keys, static_cast<u64>(n_probe), left_outer,
                       out_build_rows, out_probe_rows, static_cast<u64>(n_pairs), reinterpret_cast<u64 *>(result));
  }
  if (n_probe) {
    const u64 want = (static_cast<u64>(n_probe) + kJpCkThreads - 1) / kJpCkThreads;
    hipLaunchKernelGGL(jp_check_expected_kernel, dim3(static_cast<unsigned>(want < cap ? want : cap)), dim3(kJpCkThreads), 0,
                       s, ids, static_cast<u64>(n_build), probe_row_ids, pos, cnt, static_cast<u64>(n_probe), left_outer,
                       reinterpret_cast<u64 *>(result));
  }
  return launch_status();
}
