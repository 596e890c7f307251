// reduce_by_key.hip — one output row per run of equal adjacent keys for gfx950: COUNT, exact 64-bit SUM, MIN, MAX
// (include/dbhip_reduce_by_key.h).  Behind the stable pairs sort this is GROUP BY key ORDER BY key.
//
// No reference counterpart.  HEAD, run, the x domain, SEGMENT, chunk and step are defined in by_key.hpp, which also holds
// the open run's aggregate (BkAgg) and its segmented wave scan.
//
// All dependent launches, no workgroup ever waits on another (DESIGN.md findings 8 and 9), no CAS loop, every loop bounded
// by n:
//   fill        clears the header
//   rk_count    one streaming read of the keys: the heads of every segment (the left neighbour of a segment's first row
//               is read from memory)
//   rk_scan     one workgroup: the first output row of every segment, *out_runs, DBHIP_DEV_TABLE_FULL
//   rk_reduce   one read of keys and vals, 256 rows of the segment at a time, four consecutive rows per lane.  The open
//               run's aggregate travels as (position of the last head, sum, min, max); a segmented wave scan over the
//               lanes' aggregates (DPP, six steps) gives every lane what is open in front of it.  A head row writes its
//               own key, and the run that ended in front of it: to its output row when that run began in this segment,
//               to the segment's LEAD record when it did not.  256 rows without a head are added lane by lane and reduced
//               over the wave only when the next head (or the segment's end) comes.  What is open at the segment's end is
//               its TAIL record — or, in a segment without a head, a lead record that is the whole segment.
//   rk_stitch   one workgroup: a segmented scan over the segments' records (element = tail where the segment has a head,
//               lead where not) gives the run open at the end of every segment; a segment with a head closes the run open
//               in front of it (that aggregate + its lead) at the output row in front of its first head, the last run
//               closes at the column's end.  A scan, not a walk: a column that is one run is n / 4096 records behind one head.
//
// workspace: header | cnt[segments] | pos[segments] | rec[segments] (48 bytes); every part at a 256-byte offset
#include "by_key.hpp"

namespace dbhip {
namespace {

constexpr int kRkThreads = 512;
constexpr int kRkWaves = kRkThreads / kWave;
constexpr size_t kRkSegment = DBHIP_REDUCE_BY_KEY_SEGMENT_ROWS;  // rows of one wave
constexpr size_t kRkChunk = DBHIP_REDUCE_BY_KEY_CHUNK_ROWS;      // rows of one workgroup
static_assert(kRkChunk == kRkSegment * kRkWaves, "a chunk is one segment per wave");
constexpr size_t kRkStep = 4 * kWave;  // rows a wave takes at a time: four consecutive rows per lane
static_assert(kRkSegment % (2 * kRkStep) == 0, "a segment is a whole number of steps");
constexpr int kRkScanThreads = 1024;

// what a segment leaves for rk_stitch; mn and mx in the x domain
struct RkPart {
  u64 sum;
  unsigned cnt, mn, mx;
  unsigned flag;  // inside rk_stitch's scan: the range holds a head
};
struct RkRec {
  RkPart lead, tail;
};
static_assert(sizeof(RkRec) == 48, "record size (dbhip_reduce_by_key.h states the workspace bound)");

struct RkLayout {
  size_t segments, cnt, pos, rec, total;
};
inline RkLayout rk_layout(size_t n) {
  RkLayout l;
  l.segments = (n + kRkSegment - 1) / kRkSegment;
  l.cnt = kWsHeader;
  l.pos = l.cnt + align_up(l.segments * sizeof(unsigned), kWsAlign);
  l.rec = l.pos + align_up(l.segments * sizeof(unsigned), kWsAlign);
  l.total = l.rec + align_up(l.segments * sizeof(RkRec), kWsAlign);
  return l;
}

struct RkOut {
  unsigned *keys, *counts;
  u64 *sums;
  unsigned *mins, *maxs;
  u64 capacity;
};

// ---- count -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRkThreads) void rk_count_kernel(const unsigned *__restrict__ keys, size_t n,
                                                              unsigned *__restrict__ cnt, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kRkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const size_t first = seg * kRkSegment;
  unsigned heads = 0;
  if (first + kRkSegment <= n) {  // a whole segment: 16 loads of 16 bytes per lane, four in flight
    unsigned left = first ? keys[first - 1] : ~keys[0];  // row 0 is a head
    const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys + first) + lane;
    auto count4 = [&](const u32x4 v) {
      unsigned prev = __builtin_amdgcn_update_dpp(0u, v.w, 0x138, 0xf, 0xf, false);  // wave_shr:1
      if (lane == 0) prev = left;
      heads += (v.x != prev ? 1u : 0u) + (v.y != v.x ? 1u : 0u) + (v.z != v.y ? 1u : 0u) + (v.w != v.z ? 1u : 0u);
      left = __builtin_amdgcn_readlane(v.w, kWave - 1);
    };
#pragma unroll 1
    for (int i = 0; i < static_cast<int>(kRkSegment / kRkStep); i += 4) {
      const u32x4 v0 = __builtin_nontemporal_load(k4 + i * kWave), v1 = __builtin_nontemporal_load(k4 + (i + 1) * kWave),
                  v2 = __builtin_nontemporal_load(k4 + (i + 2) * kWave), v3 = __builtin_nontemporal_load(k4 + (i + 3) * kWave);
      count4(v0);
      count4(v1);
      count4(v2);
      count4(v3);
    }
  } else {  // the ragged last segment
    for (size_t i = first + lane; i < n; i += kWave) heads += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
  }
  heads = wave_reduce_add(heads);
  if (lane == 0) cnt[seg] = heads;
}

// ---- scan: one workgroup -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRkScanThreads) void rk_scan_kernel(WsStatusHeader *hdr, const unsigned *__restrict__ cnt,
                                                                 unsigned *__restrict__ pos, size_t segments, u64 capacity,
                                                                 int count_only, u64 *out_runs) {
  __shared__ unsigned s_wsum[kRkScanThreads / kWave];
  unsigned run = 0;  // heads of the rounds so far (the same in every thread); at most n < 2^32
  for (size_t base = 0; base < segments; base += kRkScanThreads) {
    const size_t seg = base + threadIdx.x;
    const unsigned c = seg < segments ? cnt[seg] : 0u;
    unsigned total;
    const unsigned before = block_exclusive_scan<kRkScanThreads>(c, s_wsum, total);
    if (seg < segments) pos[seg] = run + before;
    run += total;
  }
  if (threadIdx.x == 0) {
    *out_runs = run;
    if (!count_only && run > capacity) atomicOr(&hdr->status, DBHIP_DEV_TABLE_FULL);
  }
}

// ---- reduce ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rk_write_run(const RkOut &out, u64 r, unsigned count, u64 sum, unsigned mn, unsigned mx,
                                             unsigned sign) {
  if (r >= out.capacity) return;
  if (out.counts) out.counts[r] = count;
  if (out.sums) out.sums[r] = sum;
  if (out.mins) out.mins[r] = mn ^ sign;
  if (out.maxs) out.maxs[r] = mx ^ sign;
}

__global__ __launch_bounds__(kRkThreads) void rk_reduce_kernel(const unsigned *__restrict__ keys,
                                                               const unsigned *__restrict__ vals, size_t n, unsigned sign,
                                                               const unsigned *__restrict__ pos, RkRec *__restrict__ rec,
                                                               size_t segments, RkOut out) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kRkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const bool is_signed = sign != 0;
  const size_t first = seg * kRkSegment;
  const size_t last = first + kRkSegment < n ? first + kRkSegment : n;
  const bool full = last - first == kRkSegment;
  const u64 base_run = pos[seg];
  unsigned left = first ? keys[first - 1] : 0u;  // key of the row in front of the rows in hand (wave-uniform)
  BkAgg carry = bk_none();  // what is open in front of the rows in hand (wave-uniform) ...
  BkAgg acc = bk_none();    // ... together with these per-lane sums of steps that had no head (lh unused)
  bool acc_used = false;
  unsigned heads_before = 0;  // heads of the segment in front of the rows in hand (wave-uniform)

  // bk_load on this segment.  Through a lambda, as the loads were before by_key.hpp: called directly the kernel is
  // the same instructions with two VGPR names exchanged.
  auto load = [&](size_t row0, u32x4 &k, u32x4 &v) { bk_load(keys, vals, full, row0, last, k, v); };
  auto fold_acc = [&]() {  // the per-lane sums into the carry
    if (!acc_used) return;
    carry.sum += wave_reduce_add_u64(acc.sum);
    carry.mn = bk_min(carry.mn, wave_reduce_min(acc.mn));
    carry.mx = bk_max(carry.mx, wave_reduce_max(acc.mx));
    acc = bk_none();
    acc_used = false;
  };

  u32x4 k4, v4;
  load(first + 4 * lane, k4, v4);
  for (size_t base = first; base < last; base += kRkStep) {
    const size_t row0 = base + 4 * lane;  // this lane's four consecutive rows
    const unsigned rel0 = static_cast<unsigned>(row0 - first);
    const u32x4 k = k4, v = v4;
    if (base + kRkStep < last) load(row0 + kRkStep, k4, v4);  // in flight over this step
    // the previous key and the loop over the lane's rows are those of sk_scan_kernel (scan_by_key.hip)
    bool valid[4], head[4];
    unsigned x[4];
    unsigned prev = __builtin_amdgcn_update_dpp(0u, k[3], 0x138, 0xf, 0xf, false);  // wave_shr:1
    if (lane == 0) prev = left;
    left = __builtin_amdgcn_readlane(k[3], kWave - 1);
    unsigned n_heads = 0;
    BkAgg a = bk_none();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      valid[q] = full || row0 + q < last;
      x[q] = v[q] ^ sign;
      head[q] = valid[q] && (q ? k[q] != k[q - 1] : (row0 == 0 || k[0] != prev));
      n_heads += head[q] ? 1u : 0u;
      if (head[q]) a = BkAgg{rel0 + q + 1, 0xFFFFFFFFu, 0u, 0ull};
      if (valid[q]) {
        a.sum += bk_ext(v[q], is_signed);
        a.mn = bk_min(a.mn, x[q]);
        a.mx = bk_max(a.mx, x[q]);
      }
    }
    if (__ballot(n_heads != 0) == 0) {  // no head in the wave's rows: a plain sum, reduced over the wave later
      acc.sum += a.sum;
      acc.mn = bk_min(acc.mn, a.mn);
      acc.mx = bk_max(acc.mx, a.mx);
      acc_used = true;
      continue;
    }
    fold_acc();
    const unsigned h_incl = wave_inclusive_scan(n_heads);
    unsigned h_before = heads_before + h_incl - n_heads;  // heads of the segment in front of this lane's rows
    heads_before += __builtin_amdgcn_readlane(h_incl, kWave - 1);
    BkAgg incl = a;
    bk_wave_scan<true>(incl);
    BkAgg open = bk_dpp<0x138, 0xf>(incl);  // wave_shr:1: what the lanes in front of this one leave open
    bk_prepend<true>(open, carry);
    BkAgg total;  // the last lane's; down to `carry = total` as in sk_scan_kernel
    total.lh = __builtin_amdgcn_readlane(incl.lh, kWave - 1);
    total.mn = __builtin_amdgcn_readlane(incl.mn, kWave - 1);
    total.mx = __builtin_amdgcn_readlane(incl.mx, kWave - 1);
    const unsigned total_hi = __builtin_amdgcn_readlane(static_cast<unsigned>(incl.sum >> 32), kWave - 1);
    const unsigned total_lo = __builtin_amdgcn_readlane(static_cast<unsigned>(incl.sum), kWave - 1);  // (readlane gives an int)
    total.sum = (static_cast<u64>(total_hi) << 32) | total_lo;
    bk_prepend<true>(total, carry);
    carry = total;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (head[q]) {
        const u64 r = base_run + h_before;  // the run that starts here
        if (out.keys && r < out.capacity) out.keys[r] = k[q];
        if (open.lh == 0) {  // the rows in front of the segment's first head: part of a run that began earlier
          rec[seg].lead = RkPart{open.sum, rel0 + q, open.mn, open.mx, 0u};
        } else {  // a run that began in this segment and ends in front of this row
          rk_write_run(out, r - 1, rel0 + q - (open.lh - 1), open.sum, open.mn, open.mx, sign);
        }
        ++h_before;
        open = BkAgg{rel0 + q + 1, 0xFFFFFFFFu, 0u, 0ull};
      }
      if (valid[q]) {
        open.sum += bk_ext(v[q], is_signed);
        open.mn = bk_min(open.mn, x[q]);
        open.mx = bk_max(open.mx, x[q]);
      }
    }
  }
  fold_acc();
  if (lane == 0) {
    const unsigned rows = static_cast<unsigned>(last - first);
    if (carry.lh == 0)  // no head in the segment: all of it belongs to a run that began earlier
      rec[seg].lead = RkPart{carry.sum, rows, carry.mn, carry.mx, 0u};
    else
      rec[seg].tail = RkPart{carry.sum, rows - (carry.lh - 1), carry.mn, carry.mx, 0u};
  }
}

// ---- stitch: one workgroup -----------------------------------------------------------------------------------------------
__device__ __forceinline__ RkPart rk_part_none() { return RkPart{0ull, 0u, 0xFFFFFFFFu, 0u, 0u}; }
// a = l (+) a over segments: a range with a head keeps what is open behind its last head
__device__ __forceinline__ void rk_part_prepend(RkPart &a, const RkPart &l) {
  if (!a.flag) {
    a.sum += l.sum;
    a.cnt += l.cnt;
    a.mn = bk_min(a.mn, l.mn);
    a.mx = bk_max(a.mx, l.mx);
    a.flag = l.flag;
  }
}
__device__ __forceinline__ RkPart rk_part_shfl_up(const RkPart &a, unsigned d, unsigned lane) {
  RkPart l;
  l.sum = __shfl_up(a.sum, d, kWave);
  l.cnt = __shfl_up(a.cnt, d, kWave);
  l.mn = __shfl_up(a.mn, d, kWave);
  l.mx = __shfl_up(a.mx, d, kWave);
  l.flag = __shfl_up(a.flag, d, kWave);
  return lane >= d ? l : rk_part_none();
}

__global__ __launch_bounds__(kRkScanThreads) void rk_stitch_kernel(const unsigned *__restrict__ cnt,
                                                                   const unsigned *__restrict__ pos,
                                                                   const RkRec *__restrict__ rec, size_t segments,
                                                                   RkOut out, unsigned sign) {
  constexpr int kWaves = kRkScanThreads / kWave;
  __shared__ RkPart s_wave[kWaves];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  RkPart carry = rk_part_none();  // the run open at the end of the rounds so far (the same in every thread)
  // a round's loads are all independent (the tail is read whether or not it is used) and the next round's are in flight
  // over this round's scan: the rounds would otherwise each pay three dependent trips to memory
  struct Round {
    unsigned cnt, pos;
    RkPart lead, tail;
  };
  auto fetch = [&](size_t seg) {
    Round in{0u, 0u, rk_part_none(), rk_part_none()};
    if (seg < segments) {
      in.cnt = cnt[seg];
      in.pos = pos[seg];
      in.lead = rec[seg].lead;
      in.tail = rec[seg].tail;
    }
    return in;
  };
  Round next = fetch(threadIdx.x);
  for (size_t base = 0; base < segments; base += kRkScanThreads) {
    const size_t seg = base + threadIdx.x;
    const Round in = next;
    if (base + kRkScanThreads < segments) next = fetch(seg + kRkScanThreads);
    const bool has_head = seg < segments && in.cnt != 0;
    RkPart lead = in.lead;
    lead.flag = 0u;
    RkPart incl = lead;
    if (has_head) {
      incl = in.tail;
      incl.flag = 1u;
    }
#pragma unroll
    for (unsigned d = 1; d < kWave; d <<= 1) {
      const RkPart l = rk_part_shfl_up(incl, d, lane);
      rk_part_prepend(incl, l);
    }
    RkPart open = rk_part_shfl_up(incl, 1, lane);  // open at the end of the segment in front of this one
    wg_barrier_lds_only();  // s_wave may still be read from the round before; the loads in flight stay in flight
    if (lane == kWave - 1) s_wave[wave] = incl;
    wg_barrier_lds_only();
    RkPart before = carry, all = carry;
#pragma unroll 1
    for (int w = 0; w < kWaves; ++w) {
      RkPart p = s_wave[w];
      RkPart q = p;
      rk_part_prepend(p, all);
      all = p;
      if (static_cast<unsigned>(w) < wave) {
        rk_part_prepend(q, before);
        before = q;
      }
    }
    rk_part_prepend(open, before);
    if (has_head && seg > 0) {  // closes the run that was open in front of it, at the row in front of its first head
      rk_part_prepend(lead, open);
      rk_write_run(out, static_cast<u64>(in.pos) - 1, lead.cnt, lead.sum, lead.mn, lead.mx, sign);
    }
    carry = all;
  }
  if (threadIdx.x == 0 && segments)  // the last run ends with the column
    rk_write_run(out, static_cast<u64>(pos[segments - 1]) + cnt[segments - 1] - 1, carry.cnt, carry.sum, carry.mn, carry.mx,
                 sign);
}

// ---- the validator -------------------------------------------------------------------------------------------------------
constexpr int kRkCheckThreads = 256;
constexpr u64 kRkWeightSeed = 0x72626Bull;

struct RkCheckHeader {
  u64 total;  // the exact sum of out_counts
  u64 pad[31];
};
static_assert(sizeof(RkCheckHeader) == kWsHeader, "validator header size");

struct RkCheckLayout {
  size_t flags, starts, scan_ws, scan_bytes, total;
};
inline RkCheckLayout rk_check_layout(size_t runs) {
  RkCheckLayout l;
  const size_t col = align_up((runs ? runs : 1) * sizeof(unsigned), kWsAlign);
  l.flags = kWsHeader;
  l.starts = l.flags + col;
  l.scan_ws = l.starts + col;
  l.scan_bytes = dbhip_exclusive_scan_u32_workspace_bytes(runs);
  l.total = align_up(l.scan_ws + l.scan_bytes, kWsAlign);
  return l;
}

__device__ __forceinline__ u64 rk_weight(u64 run) { return mix64(kRkWeightSeed, run) | 1ull; }

// adds the workgroup's sums of a and b to result[ia] and result[ib]
__device__ __forceinline__ void rk_check_flush(u64 a, u64 b, u64 *result, int ia, int ib, u64 (*s_part)[kRkCheckThreads / kWave]) {
  a = wave_reduce_add_u64(a);
  b = wave_reduce_add_u64(b);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_part[0][threadIdx.x / kWave] = a;
    s_part[1][threadIdx.x / kWave] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    u64 sum = 0;
#pragma unroll
    for (int w = 0; w < kRkCheckThreads / kWave; ++w) sum += s_part[threadIdx.x][w];
    if (sum) atomicAdd(result + (threadIdx.x ? ib : ia), sum);
  }
  __syncthreads();
}

// per run: the count's share of T, empty runs, runs that continue their predecessor's key, the sums' fingerprint
__global__ __launch_bounds__(kRkCheckThreads) void rk_check_runs_kernel(const unsigned *__restrict__ keys, size_t n,
                                                                        const unsigned *__restrict__ out_keys,
                                                                        const unsigned *__restrict__ out_counts,
                                                                        const u64 *__restrict__ out_sums,
                                                                        const unsigned *__restrict__ starts, size_t runs,
                                                                        RkCheckHeader *hdr, u64 *result) {
  __shared__ u64 s_part[2][kRkCheckThreads / kWave];
  const size_t stride = static_cast<size_t>(gridDim.x) * kRkCheckThreads;
  u64 faults = 0, wsum = 0, rows = 0;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kRkCheckThreads + threadIdx.x; r < runs; r += stride) {
    const unsigned c = out_counts[r], s = starts[r];
    rows += c;
    faults += c == 0 ? 1u : 0u;
    if (r > 0 && s >= 1 && s <= n && keys[s - 1] == out_keys[r]) ++faults;  // not maximal
    wsum += out_sums[r] * rk_weight(r);
  }
  rk_check_flush(faults, wsum, result, 0, 3, s_part);
  rk_check_flush(rows, 0, &hdr->total, 0, 0, s_part);
}

// per input row: its run by bisection in starts
__global__ __launch_bounds__(kRkCheckThreads) void rk_check_rows_kernel(
    const unsigned *__restrict__ keys, const unsigned *__restrict__ vals, size_t n, unsigned sign,
    const unsigned *__restrict__ out_keys, const unsigned *__restrict__ out_mins, const unsigned *__restrict__ out_maxs,
    const unsigned *__restrict__ starts, size_t runs, const RkCheckHeader *hdr, unsigned *flags, u64 *result) {
  __shared__ u64 s_part[2][kRkCheckThreads / kWave];
  const size_t stride = static_cast<size_t>(gridDim.x) * kRkCheckThreads;
  const u64 total = hdr->total;
  u64 faults = 0, wsum = 0;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kRkCheckThreads + threadIdx.x; i < n; i += stride) {
    if (i >= total || runs == 0) {  // a row behind the table
      ++faults;
      continue;
    }
    size_t lo = 0, hi = runs;  // starts[0] == 0 <= i
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      if (starts[mid] <= i) lo = mid;
      else hi = mid;
    }
    const unsigned v = vals[i], x = v ^ sign;
    const unsigned mn = out_mins[lo] ^ sign, mx = out_maxs[lo] ^ sign;
    faults += keys[i] != out_keys[lo] ? 1u : 0u;
    faults += (x < mn || x > mx) ? 1u : 0u;
    unsigned seen = (x == mn ? 1u : 0u) | (x == mx ? 2u : 0u);
    if (seen) seen &= ~flags[lo];  // set only when not yet set
    if (seen) atomicOr(&flags[lo], seen);
    wsum += bk_ext(v, sign != 0) * rk_weight(lo);
  }
  rk_check_flush(faults, wsum, result, 0, 2, s_part);
}

// the runs whose min or max no row carried; T against n
__global__ __launch_bounds__(kRkCheckThreads) void rk_check_final_kernel(const unsigned *__restrict__ flags, size_t runs,
                                                                         size_t n, const RkCheckHeader *hdr, u64 *result) {
  __shared__ u64 s_part[2][kRkCheckThreads / kWave];
  const size_t stride = static_cast<size_t>(gridDim.x) * kRkCheckThreads;
  u64 unseen = 0;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kRkCheckThreads + threadIdx.x; r < runs; r += stride) {
    const unsigned f = flags[r];
    unseen += (f & 1u ? 0u : 1u) + (f & 2u ? 0u : 1u);
  }
  const u64 wrong_total = (blockIdx.x == 0 && threadIdx.x == 0 && hdr->total != n) ? 1u : 0u;
  rk_check_flush(wrong_total, unseen, result, 0, 1, s_part);
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_reduce_by_key_workspace_bytes(size_t n) {
  if (n >= (1ull << 32)) return 0;
  return rk_layout(n).total;
}

extern "C" int dbhip_reduce_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                       uint32_t *out_keys, uint32_t *out_counts, uint64_t *out_sums, uint32_t *out_mins,
                                       uint32_t *out_maxs, size_t capacity, uint64_t *out_runs, void *workspace,
                                       size_t workspace_bytes, dbhip_stream_t stream) {
  if (n >= (1ull << 32)) return DBHIP_EINVAL;  // 32-bit counts and run numbers
  if (n && (!keys || !out_runs)) return DBHIP_EINVAL;
  const bool any_column = out_keys || out_counts || out_sums || out_mins || out_maxs;
  if ((capacity == 0) == any_column) return DBHIP_EINVAL;  // columns without room, or room without a column
  if (!vals && (out_sums || out_mins || out_maxs)) return DBHIP_EINVAL;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(vals) |
                         reinterpret_cast<uintptr_t>(out_keys) | reinterpret_cast<uintptr_t>(out_counts) |
                         reinterpret_cast<uintptr_t>(out_sums) | reinterpret_cast<uintptr_t>(out_mins) |
                         reinterpret_cast<uintptr_t>(out_maxs);
  if (addr & 15u) return DBHIP_EINVAL;  // dbhip_reduce_by_key.h: 16-byte aligned
  if (reinterpret_cast<uintptr_t>(out_runs) & 7u) return DBHIP_EINVAL;
  hipStream_t s = as_stream(stream);
  if (n == 0) {  // no rows, no runs; a workspace that was passed still gets a clean status word
    if (workspace && !ws_ok(workspace, workspace_bytes, kWsHeader)) return DBHIP_EWORKSPACE;
    if (workspace) {
      const hipError_t e = fill_async(workspace, 0, kWsHeader, s);
      if (e != hipSuccess) return static_cast<int>(e);
    }
    if (out_runs) return static_cast<int>(fill_async(out_runs, 0, sizeof(uint64_t), s));
    return DBHIP_OK;
  }
  const RkLayout l = rk_layout(n);
  if (!ws_ok(workspace, workspace_bytes, l.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  char *base = static_cast<char *>(workspace);
  WsStatusHeader *hdr = reinterpret_cast<WsStatusHeader *>(base);
  unsigned *cnt = reinterpret_cast<unsigned *>(base + l.cnt);
  unsigned *pos = reinterpret_cast<unsigned *>(base + l.pos);
  RkRec *rec = reinterpret_cast<RkRec *>(base + l.rec);
  const hipError_t e = fill_async(workspace, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  const unsigned seg_grid = static_cast<unsigned>((l.segments + kRkWaves - 1) / kRkWaves);
  hipLaunchKernelGGL(rk_count_kernel, dim3(seg_grid), dim3(kRkThreads), 0, s, keys, n, cnt, l.segments);
  hipLaunchKernelGGL(rk_scan_kernel, dim3(1), dim3(kRkScanThreads), 0, s, hdr, cnt, pos, l.segments,
                     static_cast<u64>(capacity), any_column ? 0 : 1, reinterpret_cast<u64 *>(out_runs));
  if (any_column) {
    const RkOut out{out_keys, out_counts, reinterpret_cast<u64 *>(out_sums), out_mins, out_maxs, static_cast<u64>(capacity)};
    const unsigned sign = vals_signed ? 0x80000000u : 0u;
    hipLaunchKernelGGL(rk_reduce_kernel, dim3(seg_grid), dim3(kRkThreads), 0, s, keys, vals, n, sign, pos, rec, l.segments,
                       out);
    hipLaunchKernelGGL(rk_stitch_kernel, dim3(1), dim3(kRkScanThreads), 0, s, cnt, pos, rec, l.segments, out, sign);
  }
  return launch_status();
}

extern "C" size_t dbhip_check_reduce_by_key_workspace_bytes(size_t n, size_t runs) {
  if (n >= (1ull << 32) || runs >= (1ull << 32)) return 0;
  return rk_check_layout(runs).total;
}

extern "C" int dbhip_check_reduce_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                             const uint32_t *out_keys, const uint32_t *out_counts,
                                             const uint64_t *out_sums, const uint32_t *out_mins, const uint32_t *out_maxs,
                                             size_t runs, uint64_t *result, void *workspace, size_t workspace_bytes,
                                             dbhip_stream_t stream) {
  if (!result || n >= (1ull << 32) || runs >= (1ull << 32)) return DBHIP_EINVAL;
  if (n && (!keys || !vals)) return DBHIP_EINVAL;
  if (runs && (!out_keys || !out_counts || !out_sums || !out_mins || !out_maxs)) return DBHIP_EINVAL;
  const RkCheckLayout l = rk_check_layout(runs);
  if (!ws_ok(workspace, workspace_bytes, l.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  char *base = static_cast<char *>(workspace);
  RkCheckHeader *hdr = reinterpret_cast<RkCheckHeader *>(base);
  unsigned *flags = reinterpret_cast<unsigned *>(base + l.flags);
  unsigned *starts = reinterpret_cast<unsigned *>(base + l.starts);
  u64 *res = reinterpret_cast<u64 *>(result);
  hipError_t e = fill_async(result, 0, 4 * sizeof(uint64_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  e = fill_async(workspace, 0, l.starts, s);  // the header and the flags
  if (e != hipSuccess) return static_cast<int>(e);
  if (runs) {
    const int rc = dbhip_exclusive_scan_u32(out_counts, runs, 0u, starts, base + l.scan_ws, l.scan_bytes, stream);
    if (rc != DBHIP_OK) return rc;
    hipLaunchKernelGGL(rk_check_runs_kernel, dim3(capped_grid(runs, kRkCheckThreads, dev)), dim3(kRkCheckThreads), 0, s,
                       keys, n, out_keys, out_counts, reinterpret_cast<const u64 *>(out_sums), starts, runs, hdr, res);
  }
  if (n)
    hipLaunchKernelGGL(rk_check_rows_kernel, dim3(capped_grid(n, kRkCheckThreads, dev)), dim3(kRkCheckThreads), 0, s, keys,
                       vals, n, vals_signed ? 0x80000000u : 0u, out_keys, out_mins, out_maxs, starts, runs, hdr, flags, res);
  hipLaunchKernelGGL(rk_check_final_kernel, dim3(capped_grid(runs, kRkCheckThreads, dev)), dim3(kRkCheckThreads), 0, s,
                     flags, runs, n, hdr, res);
  return launch_status();
}
