// scan_by_key.hip — one output row per input row over runs of equal adjacent keys for gfx950: the run number, the running
// COUNT, exact 64-bit SUM, MIN and MAX (include/dbhip_scan_by_key.h).  Behind the stable pairs sort these are the window
// functions over PARTITION BY key ... ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW.
//
// No reference counterpart.  HEAD, run, the x domain, SEGMENT, chunk and step are defined in by_key.hpp, which also holds
// the open run's aggregate (BkAgg) and its segmented wave scan; the run number is the run's row in reduce_by_key.hip's table.
//
// All dependent launches, no workgroup ever waits on another (DESIGN.md findings 8 and 9), no CAS loop, every loop bounded
// by n:
//   fill      clears the header
//   sk_tail   one streaming read of keys and vals, 256 rows of the segment at a time, four consecutive rows per lane.  Per
//             segment one RECORD: its heads, and the aggregate (count, sum, min, max) of the rows from its last head to its
//             end — of all its rows if it has no head.  No scan: a ballot of the head flags gives the step's last head, the
//             per-lane accumulators start again there, and they are reduced over the wave once, at the segment's end.
//   sk_carry  one workgroup, one round at any n: an exclusive segmented scan over the records.  Each of the 1024 threads
//             combines a contiguous block of ceil(segments / 1024) records in registers, one
//             workgroup scan runs over the 1024 block aggregates, and each thread walks its block again and writes every
//             segment's CARRY: the heads in front of it and the aggregate of the run still open in front of it.
//   sk_scan   the second read of keys and vals: every lane scans its four rows, the lane aggregates go through the
//             segmented wave scan seeded with what is open in front of the step (at first the segment's carry), and every
//             requested column is written with 16-byte stores.  A step without a head takes the same ladder without its
//             selects.  The ragged last segment loads and stores row by row.
//
// workspace: header | rec[segments] (32 bytes) | carry[segments] (32 bytes); every part at a 256-byte offset
#include "by_key.hpp"

namespace dbhip {
namespace {

constexpr int kSkThreads = 512;
constexpr int kSkWaves = kSkThreads / kWave;
constexpr size_t kSkSegment = DBHIP_SCAN_BY_KEY_SEGMENT_ROWS;  // rows of one wave
constexpr size_t kSkChunk = DBHIP_SCAN_BY_KEY_CHUNK_ROWS;      // rows of one workgroup
static_assert(kSkChunk == kSkSegment * kSkWaves, "a chunk is one segment per wave");
constexpr size_t kSkStep = 4 * kWave;  // rows a wave takes at a time: four consecutive rows per lane
static_assert(kSkSegment % kSkStep == 0, "a segment is a whole number of steps");
constexpr int kSkCarryThreads = 1024;

// A range of rows as the scans over segments see it: heads = its number of heads; cnt, sum, mn, mx (x domain) over the rows
// from its last head on, or over all of it when heads == 0.  sk_tail writes one per segment (the record); sk_carry writes
// one per segment for the rows in front of it (the carry: heads = the segment's first run number, the rest = the open run).
struct SkPart {
  u64 sum;
  unsigned heads, cnt, mn, mx;
  unsigned pad[2];
};
static_assert(sizeof(SkPart) == 32, "record and carry size (dbhip_scan_by_key.h states the workspace bound)");

struct SkLayout {
  size_t segments, rec, carry, total;
};
inline SkLayout sk_layout(size_t n) {
  SkLayout l;
  l.segments = (n + kSkSegment - 1) / kSkSegment;
  l.rec = kWsHeader;
  l.carry = l.rec + align_up(l.segments * sizeof(SkPart), kWsAlign);
  l.total = l.carry + align_up(l.segments * sizeof(SkPart), kWsAlign);
  return l;
}

struct SkOut {
  unsigned *run_ids, *row_numbers;
  u64 *sums;
  unsigned *mins, *maxs;
};

// ---- tail --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSkThreads) void sk_tail_kernel(const unsigned *__restrict__ keys,
                                                             const unsigned *__restrict__ vals, size_t n, unsigned sign,
                                                             SkPart *__restrict__ rec, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const bool is_signed = sign != 0;
  const size_t first = seg * kSkSegment;
  const size_t last = first + kSkSegment < n ? first + kSkSegment : n;
  const bool full = last - first == kSkSegment;
  unsigned left = first ? keys[first - 1] : 0u;  // key of the row in front of the rows in hand (wave-uniform)
  // per lane, over the rows of this lane since the segment's last head so far
  u64 acc_sum = 0;
  unsigned acc_cnt = 0, acc_mn = 0xFFFFFFFFu, acc_mx = 0u, heads = 0;

  u32x4 k4, v4;
  bk_load(keys, vals, full, first + 4 * lane, last, k4, v4);
  for (size_t base = first; base < last; base += kSkStep) {
    const size_t row0 = base + 4 * lane;
    const u32x4 k = k4, v = v4;
    if (base + kSkStep < last) bk_load(keys, vals, full, row0 + kSkStep, last, k4, v4);  // in flight over this step
    unsigned prev = __builtin_amdgcn_update_dpp(0u, k[3], 0x138, 0xf, 0xf, false);  // wave_shr:1
    if (lane == 0) prev = left;
    left = __builtin_amdgcn_readlane(k[3], kWave - 1);
    // this lane's rows from its own last head on (all four when it has none): the loop of sk_scan_kernel and
    // rk_reduce_kernel, counting rows instead of keeping the head's position
    u64 a_sum = 0;
    unsigned a_cnt = 0, a_mn = 0xFFFFFFFFu, a_mx = 0u, n_heads = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool valid = full || row0 + q < last;
      const bool head = valid && (q ? k[q] != k[q - 1] : (row0 == 0 || k[0] != prev));
      if (head) {
        ++n_heads;
        a_sum = 0;
        a_cnt = 0;
        a_mn = 0xFFFFFFFFu;
        a_mx = 0u;
      }
      if (valid) {
        const unsigned x = v[q] ^ sign;
        a_sum += bk_ext(v[q], is_signed);
        ++a_cnt;
        a_mn = bk_min(a_mn, x);
        a_mx = bk_max(a_mx, x);
      }
    }
    heads += n_heads;
    const u64 mask = __ballot(n_heads != 0);
    if (mask == 0) {  // the open run goes on
      acc_sum += a_sum;
      acc_cnt += a_cnt;
      acc_mn = bk_min(acc_mn, a_mn);
      acc_mx = bk_max(acc_mx, a_mx);
    } else {  // only the rows at or behind the step's last head count
      const unsigned last_lane = 63u - static_cast<unsigned>(__builtin_clzll(mask));
      const bool keep = lane >= last_lane;
      acc_sum = keep ? a_sum : 0ull;
      acc_cnt = keep ? a_cnt : 0u;
      acc_mn = keep ? a_mn : 0xFFFFFFFFu;
      acc_mx = keep ? a_mx : 0u;
    }
  }
  acc_sum = wave_reduce_add_u64(acc_sum);
  acc_cnt = wave_reduce_add(acc_cnt);
  acc_mn = wave_reduce_min(acc_mn);
  acc_mx = wave_reduce_max(acc_mx);
  heads = wave_reduce_add(heads);
  if (lane == 0) rec[seg] = SkPart{acc_sum, heads, acc_cnt, acc_mn, acc_mx, {0u, 0u}};
}

// ---- carry: one workgroup ------------------------------------------------------------------------------------------------
__device__ __forceinline__ SkPart sk_part_none() { return SkPart{0ull, 0u, 0u, 0xFFFFFFFFu, 0u, {0u, 0u}}; }
// a = l (+) a: the rows of l directly in front of the rows of a
__device__ __forceinline__ void sk_part_prepend(SkPart &a, const SkPart &l) {
  if (a.heads == 0) {
    a.sum += l.sum;
    a.cnt += l.cnt;
    a.mn = bk_min(a.mn, l.mn);
    a.mx = bk_max(a.mx, l.mx);
  }
  a.heads += l.heads;
}
// a = a (+) r: the rows of r directly behind the rows of a
__device__ __forceinline__ void sk_part_append(SkPart &a, const SkPart &r) {
  const unsigned heads = a.heads + r.heads;
  if (r.heads != 0) {
    a = r;
  } else {
    a.sum += r.sum;
    a.cnt += r.cnt;
    a.mn = bk_min(a.mn, r.mn);
    a.mx = bk_max(a.mx, r.mx);
  }
  a.heads = heads;
}
__device__ __forceinline__ SkPart sk_part_shfl_up(const SkPart &a, unsigned d, unsigned lane) {
  SkPart l = sk_part_none();
  l.sum = __shfl_up(a.sum, d, kWave);
  l.heads = __shfl_up(a.heads, d, kWave);
  l.cnt = __shfl_up(a.cnt, d, kWave);
  l.mn = __shfl_up(a.mn, d, kWave);
  l.mx = __shfl_up(a.mx, d, kWave);
  return lane >= d ? l : sk_part_none();
}

__global__ __launch_bounds__(kSkCarryThreads) void sk_carry_kernel(const SkPart *__restrict__ rec,
                                                                   SkPart *__restrict__ carry, size_t segments) {
  constexpr int kWaves = kSkCarryThreads / kWave;
  __shared__ SkPart s_wave[kWaves];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t per = (segments + kSkCarryThreads - 1) / kSkCarryThreads;  // records of one thread
  const size_t lo = per * threadIdx.x < segments ? per * threadIdx.x : segments;
  const size_t hi = lo + per < segments ? lo + per : segments;
  SkPart block = sk_part_none();  // this thread's records, combined
  for (size_t s = lo; s < hi; ++s) sk_part_append(block, rec[s]);
  SkPart incl = block;
#pragma unroll
  for (unsigned d = 1; d < kWave; d <<= 1) {
    const SkPart l = sk_part_shfl_up(incl, d, lane);
    sk_part_prepend(incl, l);
  }
  SkPart open = sk_part_shfl_up(incl, 1, lane);  // the blocks of this wave in front of this thread's
  if (lane == kWave - 1) s_wave[wave] = incl;
  __syncthreads();
  SkPart before = sk_part_none();  // the waves in front of this one
  for (unsigned w = 0; w < wave; ++w) sk_part_append(before, s_wave[w]);
  sk_part_prepend(open, before);
  for (size_t s = lo; s < hi; ++s) {  // the second walk: what is in front of every segment
    carry[s] = open;
    sk_part_append(open, rec[s]);
  }
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sk_store4(unsigned *col, size_t row0, size_t last, bool full, const u32x4 w) {
  if (full) {
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4 *>(col + row0));
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row0 + q < last) col[row0 + q] = w[q];
  }
}

__global__ __launch_bounds__(kSkThreads) void sk_scan_kernel(const unsigned *__restrict__ keys,
                                                             const unsigned *__restrict__ vals, size_t n, unsigned sign,
                                                             const SkPart *__restrict__ carries, size_t segments, SkOut out) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSkWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const bool is_signed = sign != 0;
  const size_t first = seg * kSkSegment;
  const size_t last = first + kSkSegment < n ? first + kSkSegment : n;
  const bool full = last - first == kSkSegment;
  const SkPart in = carries[seg];
  const unsigned run_base = in.heads;  // heads in front of the segment
  const unsigned cnt_base = in.cnt;    // rows of the run that is open in front of the segment
  unsigned left = first ? keys[first - 1] : 0u;  // key of the row in front of the rows in hand (wave-uniform)
  BkAgg carry{0u, in.mn, in.mx, in.sum};  // what is open in front of the rows in hand (wave-uniform)
  unsigned heads_before = 0;              // heads of the segment in front of the rows in hand (wave-uniform)

  u32x4 k4, v4;
  bk_load(keys, vals, full, first + 4 * lane, last, k4, v4);
  for (size_t base = first; base < last; base += kSkStep) {
    const size_t row0 = base + 4 * lane;  // this lane's four consecutive rows
    const unsigned rel0 = static_cast<unsigned>(row0 - first);
    const u32x4 k = k4, v = v4;
    if (base + kSkStep < last) bk_load(keys, vals, full, row0 + kSkStep, last, k4, v4);  // in flight over this step
    // the previous key and the loop over the lane's rows are those of rk_reduce_kernel (reduce_by_key.hip)
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
    BkAgg incl = a;
    unsigned h_before = heads_before;  // heads of the segment in front of this lane's rows
    if (__ballot(n_heads != 0) == 0) {  // no head in the wave's rows: plain sums, minima and maxima
      bk_wave_scan<false>(incl);
    } else {
      bk_wave_scan<true>(incl);
      const unsigned h_incl = wave_inclusive_scan(n_heads);
      h_before += h_incl - n_heads;
      heads_before += __builtin_amdgcn_readlane(h_incl, kWave - 1);
    }
    BkAgg open = bk_dpp<0x138, 0xf>(incl);  // wave_shr:1: what the lanes in front of this one leave open
    bk_prepend<true>(open, carry);
    BkAgg total;  // the last lane's; down to `carry = total` as in rk_reduce_kernel
    total.lh = __builtin_amdgcn_readlane(incl.lh, kWave - 1);
    total.mn = __builtin_amdgcn_readlane(incl.mn, kWave - 1);
    total.mx = __builtin_amdgcn_readlane(incl.mx, kWave - 1);
    const unsigned total_hi = __builtin_amdgcn_readlane(static_cast<unsigned>(incl.sum >> 32), kWave - 1);
    const unsigned total_lo = __builtin_amdgcn_readlane(static_cast<unsigned>(incl.sum), kWave - 1);
    total.sum = (static_cast<u64>(total_hi) << 32) | total_lo;
    bk_prepend<true>(total, carry);
    carry = total;

    u32x4 w_run, w_num, w_mn, w_mx;
    u64 w_sum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (head[q]) {
        ++h_before;
        open = BkAgg{rel0 + q + 1, 0xFFFFFFFFu, 0u, 0ull};
      }
      open.sum += bk_ext(v[q], is_signed);  // (rows behind `last` are never stored)
      open.mn = bk_min(open.mn, x[q]);
      open.mx = bk_max(open.mx, x[q]);
      w_run[q] = run_base + h_before - 1u;
      w_num[q] = open.lh ? rel0 + q + 2u - open.lh : cnt_base + rel0 + q + 1u;
      w_sum[q] = open.sum;
      w_mn[q] = open.mn ^ sign;
      w_mx[q] = open.mx ^ sign;
    }
    if (out.run_ids) sk_store4(out.run_ids, row0, last, full, w_run);
    if (out.row_numbers) sk_store4(out.row_numbers, row0, last, full, w_num);
    if (out.mins) sk_store4(out.mins, row0, last, full, w_mn);
    if (out.maxs) sk_store4(out.maxs, row0, last, full, w_mx);
    if (out.sums) {
      if (full) {
        u64x2 *p = reinterpret_cast<u64x2 *>(out.sums + row0);
        __builtin_nontemporal_store(u64x2{w_sum[0], w_sum[1]}, p);
        __builtin_nontemporal_store(u64x2{w_sum[2], w_sum[3]}, p + 1);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (row0 + q < last) out.sums[row0 + q] = w_sum[q];
      }
    }
  }
}

// ---- the validator -------------------------------------------------------------------------------------------------------
constexpr int kSkCheckThreads = 256;

__global__ __launch_bounds__(kSkCheckThreads) void sk_check_kernel(const unsigned *__restrict__ keys,
                                                                   const unsigned *__restrict__ vals, size_t n, unsigned sign,
                                                                   const unsigned *__restrict__ run_ids,
                                                                   const unsigned *__restrict__ row_numbers,
                                                                   const u64 *__restrict__ sums,
                                                                   const unsigned *__restrict__ mins,
                                                                   const unsigned *__restrict__ maxs, u64 *result) {
  const bool is_signed = sign != 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kSkCheckThreads;
  u64 faults = 0, heads = 0, lowest = ~0ull;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kSkCheckThreads + threadIdx.x; i < n; i += stride) {
    const bool head = i == 0 || keys[i] != keys[i - 1];
    const unsigned v = vals ? vals[i] : 0u;
    unsigned bad = 0;
    if (head) {
      ++heads;
      if (run_ids) bad += run_ids[i] != (i ? run_ids[i - 1] + 1u : 0u) ? 1u : 0u;
      if (row_numbers) bad += row_numbers[i] != 1u ? 1u : 0u;
      if (sums) bad += sums[i] != bk_ext(v, is_signed) ? 1u : 0u;
      if (mins) bad += mins[i] != v ? 1u : 0u;
      if (maxs) bad += maxs[i] != v ? 1u : 0u;
    } else {
      if (run_ids) bad += run_ids[i] != run_ids[i - 1] ? 1u : 0u;
      if (row_numbers) bad += row_numbers[i] != row_numbers[i - 1] + 1u ? 1u : 0u;
      if (sums) bad += sums[i] != sums[i - 1] + bk_ext(v, is_signed) ? 1u : 0u;
      if (mins) bad += (mins[i] ^ sign) != bk_min(mins[i - 1] ^ sign, v ^ sign) ? 1u : 0u;
      if (maxs) bad += (maxs[i] ^ sign) != bk_max(maxs[i - 1] ^ sign, v ^ sign) ? 1u : 0u;
    }
    faults += bad;
    if (bad && i < lowest) lowest = i;
  }
  faults = wave_reduce_add_u64(faults);
  heads = wave_reduce_add_u64(heads);
  if (faults) {  // uniform over the wave: faults is the wave's sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 other = __shfl_xor(lowest, off, kWave);
      lowest = other < lowest ? other : lowest;
    }
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (faults) {
      atomicAdd(result + 0, faults);
      atomicMin(result + 1, lowest);
    }
    if (heads) atomicAdd(result + 2, heads);
  }
}

inline bool sk_args_bad(const uint32_t *keys, const uint32_t *vals, size_t n, const void *c0, const void *c1, const void *c2,
                        const void *c3, const void *c4) {
  if (n >= (1ull << 32)) return true;  // 32-bit row numbers and run numbers
  if (n && !keys) return true;
  if (n && !c0 && !c1 && !c2 && !c3 && !c4) return true;
  if (!vals && (c2 || c3 || c4)) return true;
  return false;
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_scan_by_key_workspace_bytes(size_t n) {
  if (n >= (1ull << 32)) return 0;
  return sk_layout(n).total;
}

extern "C" int dbhip_scan_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                     uint32_t *out_run_ids, uint32_t *out_row_numbers, uint64_t *out_sums, uint32_t *out_mins,
                                     uint32_t *out_maxs, void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  if (sk_args_bad(keys, vals, n, out_run_ids, out_row_numbers, out_sums, out_mins, out_maxs)) return DBHIP_EINVAL;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(vals) |
                         reinterpret_cast<uintptr_t>(out_run_ids) | reinterpret_cast<uintptr_t>(out_row_numbers) |
                         reinterpret_cast<uintptr_t>(out_sums) | reinterpret_cast<uintptr_t>(out_mins) |
                         reinterpret_cast<uintptr_t>(out_maxs);
  if (addr & 15u) return DBHIP_EINVAL;  // dbhip_scan_by_key.h: 16-byte aligned
  hipStream_t s = as_stream(stream);
  if (n == 0) {  // no rows; a workspace that was passed still gets a clean status word
    if (workspace && !ws_ok(workspace, workspace_bytes, kWsHeader)) return DBHIP_EWORKSPACE;
    if (workspace) return static_cast<int>(fill_async(workspace, 0, kWsHeader, s));
    return DBHIP_OK;
  }
  const SkLayout l = sk_layout(n);
  if (!ws_ok(workspace, workspace_bytes, l.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  char *base = static_cast<char *>(workspace);
  SkPart *rec = reinterpret_cast<SkPart *>(base + l.rec);
  SkPart *carry = reinterpret_cast<SkPart *>(base + l.carry);
  const hipError_t e = fill_async(workspace, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  const bool with_vals = out_sums || out_mins || out_maxs;
  const unsigned *v = with_vals ? vals : nullptr;  // without a value column the values are not read
  const unsigned sign = vals_signed ? 0x80000000u : 0u;
  const unsigned seg_grid = static_cast<unsigned>((l.segments + kSkWaves - 1) / kSkWaves);
  const SkOut out{out_run_ids, out_row_numbers, reinterpret_cast<u64 *>(out_sums), out_mins, out_maxs};
  hipLaunchKernelGGL(sk_tail_kernel, dim3(seg_grid), dim3(kSkThreads), 0, s, keys, v, n, sign, rec, l.segments);
  hipLaunchKernelGGL(sk_carry_kernel, dim3(1), dim3(kSkCarryThreads), 0, s, rec, carry, l.segments);
  hipLaunchKernelGGL(sk_scan_kernel, dim3(seg_grid), dim3(kSkThreads), 0, s, keys, v, n, sign, carry, l.segments, out);
  return launch_status();
}

extern "C" size_t dbhip_check_scan_by_key_workspace_bytes(size_t n) {
  if (n >= (1ull << 32)) return 0;
  return kWsHeader;
}

extern "C" int dbhip_check_scan_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                           const uint32_t *run_ids, const uint32_t *row_numbers, const uint64_t *sums,
                                           const uint32_t *mins, const uint32_t *maxs, uint64_t *result, void *workspace,
                                           size_t workspace_bytes, dbhip_stream_t stream) {
  if (!result || (reinterpret_cast<uintptr_t>(result) & 7u)) return DBHIP_EINVAL;
  if (sk_args_bad(keys, vals, n, run_ids, row_numbers, sums, mins, maxs)) return DBHIP_EINVAL;
  if (!ws_ok(workspace, workspace_bytes, kWsHeader)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  hipError_t e = fill_async(workspace, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  e = fill_async(result, 0, 4 * sizeof(uint64_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  e = fill_async(result + 1, 0xFF, sizeof(uint64_t), s);  // no violating row yet
  if (e != hipSuccess) return static_cast<int>(e);
  if (n) {
    hipLaunchKernelGGL(sk_check_kernel, dim3(capped_grid(n, kSkCheckThreads, dev)), dim3(kSkCheckThreads), 0, s,
                       keys, vals, n, vals_signed ? 0x80000000u : 0u, run_ids, row_numbers,
                       reinterpret_cast<const u64 *>(sums), mins, maxs, reinterpret_cast<u64 *>(result));
  }
  return launch_status();
}
