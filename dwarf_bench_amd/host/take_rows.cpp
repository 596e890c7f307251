// take_rows.cpp — late materialisation on gfx950 (take_rows.hpp holds the contract and the workspace layout): the gather
// of up to four 32-bit columns through a row-id list, and COUNT / 64-bit SUM / MIN / MAX of a column over a row-id list or
// over all its rows.
//
// The load shape is that of sel_mark_kernel<list> (select_rows.cpp), its shared text is rowlist.hpp's.  Positions are
// counted from the 16-byte boundary in front of the list: entry i sits at v = i + a, a = 0..3 words, so every 16-byte load
// of row ids is aligned whatever the pointer's alignment.  A wave owns one segment of 1024 positions at a time, a lane
// four consecutive entries per group of 256; each entry is bounds-checked, and the gathers are unconditional (row 0
// stands in for an entry that does not count), so they are independent of each other and all issued before the first
// use.  The two segments that straddle the ends of the list are handled word by word; nothing outside the arrays is
// touched.
//   take       one launch, a wave per segment.  An output is written in position order: a lane stores its four words
//              per column with one 16-byte store where the output has the list's phase (the same words past a 16-byte
//              boundary); where it has not, the lanes pass the words that belong to their right neighbour's aligned
//              vector on, and the two ends of a group of 256 are written word by word.
//   aggregate  a grid-stride launch over the segments, at most one workgroup per partial record of the workspace; a lane
//              keeps a count, a 64-bit sum, a min and a max, a wave reduces them, a workgroup writes one record.  A second
//              dependent launch of one workgroup folds the records into out[4].  No workgroup waits for another.
#include "take_rows.hpp"

#include "rowlist.hpp"

namespace {
using namespace dbhip;

constexpr unsigned kTakeSegment = DBENCH_TAKE_SEGMENT_ROWS;
constexpr int kTakeMaxCols = DBENCH_TAKE_MAX_COLS;
// segments of a workgroup.  Neither take kernel uses LDS or a barrier, so the number only decides how a short list
// spreads over the compute units: two, as the selection vectors found for lists of 2^20 rows
constexpr int kTakeWaves = 2;
constexpr int kTakeThreads = kTakeWaves * kWave;
constexpr int kTakeGroups = kTakeSegment / (4 * kWave);  // groups of 256 positions: four per lane
constexpr int kAggWaves = 4;
constexpr int kAggThreads = kAggWaves * kWave;
constexpr size_t kAggMaxParts = 2048;  // partial records, one per workgroup: eight workgroups on each of 256 compute units
constexpr int kAggFoldThreads = 256;
static_assert(kTakeGroups >= 1 && kTakeGroups * 4 * kWave == static_cast<int>(kTakeSegment), "whole groups per segment");

struct AggRecord {
  u64 count, sum, mn, mx;  // mn, mx in the x domain: value ^ flip, compared as unsigned
};
static_assert(sizeof(AggRecord) == 32, "partial record size");

struct TakeLayout {
  size_t parts, total;
};

TakeLayout take_layout(size_t capacity) {
  const size_t segments = (capacity + kTakeSegment - 1) / kTakeSegment + 1;  // + 1: the up to three words in front
  TakeLayout l;
  l.parts = (segments + kAggWaves - 1) / kAggWaves;
  if (l.parts > kAggMaxParts) l.parts = kAggMaxParts;
  l.total = kWsHeader + align_up(sizeof(AggRecord) * l.parts, kWsAlign);
  return l;
}

// the columns of one take call, by value in the kernel arguments
struct TakeCols {
  const unsigned *col[kTakeMaxCols];
  unsigned *out[kTakeMaxCols];
  unsigned shift[kTakeMaxCols];  // (words of out[c] past a 16-byte boundary - those of the list) mod 4
};

// the bounds check of a lane's four row ids: -> bit q of the result: entry q is valid and names a row of the column;
// row[q] = the row to gather (row 0 for an entry that does not count); bad: a valid entry that is neither a row nor,
// under `outer`, the "no row" id
__device__ __forceinline__ unsigned check_rows(const u32x4 e, unsigned valid, unsigned n_rows, bool outer, unsigned (&row)[4],
                                               bool &bad) {
  unsigned ok = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned w = e[q];
    const bool here = (valid >> q) & 1u, inside = w < n_rows;
    bad = bad || (here && !inside && !(outer && w == 0xFFFFFFFFu));
    if (here && inside) ok |= 1u << q;
    row[q] = inside ? w : 0u;
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------
// take
// ---------------------------------------------------------------------------------------------
// a lane's four consecutive words x of one output, `o` = the address of the first.  kShift = 0: o is 16-byte aligned.
// Otherwise the aligned vector that ends inside this lane's words starts kShift words in front of o, in the left
// neighbour's: lanes 1..63 store that vector, lane 0 its first 4 - kShift words and lane 63 its last kShift words one by
// one.  All 64 lanes call (the neighbour's words come by a wave shuffle) and all their words are entries of the list.
template <int kShift>
__device__ __forceinline__ void store_four(unsigned *__restrict__ o, unsigned lane, const unsigned (&x)[4]) {
  if constexpr (kShift == 0) {
    *reinterpret_cast<u32x4 *>(o) = u32x4{x[0], x[1], x[2], x[3]};
  } else {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < kShift; ++j) w[j] = __shfl_up(x[4 - kShift + j], 1, kWave);  // the left neighbour's last words
#pragma unroll
    for (int j = kShift; j < 4; ++j) w[j] = x[j - kShift];
    if (lane != 0) {
      *reinterpret_cast<u32x4 *>(o - kShift) = u32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4 - kShift; ++j) o[j] = x[j];
    }
    if (lane == kWave - 1) {
#pragma unroll
      for (int j = 4 - kShift; j < 4; ++j) o[j] = x[j];
    }
  }
}

template <int kCols>
__global__ __launch_bounds__(kTakeThreads) void take_kernel(const TakeCols t, unsigned n_rows, const unsigned *__restrict__ rows,
                                                            size_t capacity, const u64 *count, unsigned a, bool outer,
                                                            unsigned fill, unsigned *status, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kTakeWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const size_t m = clamped_count(count, capacity);
  const size_t vfirst = seg * kTakeSegment, vend = a + m;  // positions [a, vend) hold entries
  if (vfirst >= vend) return;  // a segment behind the last entry (the list is shorter than its capacity)
  bool bad = false;

  // the values of a lane's four entries in every column: the 4 x kCols gathers are unconditional and independent
  auto gather = [&](const u32x4 e, unsigned valid, unsigned (&x)[kCols][4]) {
    unsigned row[4];
    const unsigned ok = check_rows(e, valid, n_rows, outer, row, bad);
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
#pragma unroll
      for (int q = 0; q < 4; ++q) x[c][q] = fill;
    }
    if (n_rows) {  // uniform; an empty column has no row 0, and every entry is filled
      unsigned got[kCols][4];
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) got[c][q] = t.col[c][row[q]];
      }
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[c][q] = ((ok >> q) & 1u) ? got[c][q] : fill;
      }
    }
  };

  if (vfirst >= a && vfirst + kTakeSegment <= vend) {  // a whole segment: aligned 16-byte loads, all entries valid
    constexpr int kStep = kCols <= 2 ? 4 : 2;  // groups whose gathers are in flight together: 16 .. 32 per lane
    static_assert(kTakeGroups % kStep == 0, "whole steps per segment");
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(rows + (vfirst - a)) + lane;
#pragma unroll 1
    for (int g = 0; g < kTakeGroups; g += kStep) {
      u32x4 e[kStep];
      unsigned x[kStep][kCols][4];
#pragma unroll
      for (int j = 0; j < kStep; ++j) e[j] = s4[(g + j) * kWave];
#pragma unroll
      for (int j = 0; j < kStep; ++j) gather(e[j], 0xfu, x[j]);
#pragma unroll
      for (int j = 0; j < kStep; ++j) {
        const size_t i0 = vfirst - a + static_cast<size_t>(g + j) * (4 * kWave) + 4 * lane;
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
          unsigned *o = t.out[c] + i0;
          switch (t.shift[c]) {  // uniform
            case 0: store_four<0>(o, lane, x[j][c]); break;
            case 1: store_four<1>(o, lane, x[j][c]); break;
            case 2: store_four<2>(o, lane, x[j][c]); break;
            default: store_four<3>(o, lane, x[j][c]); break;
          }
        }
      }
    }
  } else {  // the first segment of a list that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
    for (int g = 0; g < kTakeGroups; ++g) {
      const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
      unsigned valid;
      const u32x4 e = load_ragged(rows, a, v0, vend, valid);
      unsigned x[kCols][4];
      gather(e, valid, x);
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if ((valid >> q) & 1u) t.out[c][v0 + q - a] = x[c][q];
        }
      }
    }
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
}

// ---------------------------------------------------------------------------------------------
// aggregate
// ---------------------------------------------------------------------------------------------
struct AggLane {
  u64 count, sum;
  unsigned mn, mx;  // x domain
};

// kList: `src` is the row-id list (gathered through into col), otherwise the column itself (m_host = n_rows, no count).
// flip = 0x80000000 for int32 values: MIN and MAX compare value ^ flip as unsigned, the SUM sign-extends.
template <bool kList>
__global__ __launch_bounds__(kAggThreads) void agg_kernel(const unsigned *__restrict__ col, unsigned n_rows,
                                                          const unsigned *__restrict__ src, size_t m_host, const u64 *count,
                                                          unsigned a, unsigned flip, bool outer, unsigned *status,
                                                          AggRecord *__restrict__ parts, size_t segments) {
  __shared__ AggRecord s_wave[kAggWaves];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t m = kList ? clamped_count(count, m_host) : m_host;
  const size_t vend = a + m;  // positions [a, vend) hold candidates
  AggLane acc{0ull, 0ull, 0xFFFFFFFFu, 0u};
  bool bad = false;

  auto add = [&](unsigned v, bool counts) {
    const unsigned x = v ^ flip;
    const u64 wide = flip ? static_cast<u64>(static_cast<long long>(static_cast<int>(v))) : static_cast<u64>(v);
    acc.count += counts ? 1ull : 0ull;
    acc.sum += counts ? wide : 0ull;
    acc.mn = (counts && x < acc.mn) ? x : acc.mn;
    acc.mx = (counts && x > acc.mx) ? x : acc.mx;
  };
  // fetch: a lane's four entries -> the values and the candidates `ok` that count; list mode gathers unconditionally
  auto fetch = [&](const u32x4 e, unsigned valid, unsigned (&x)[4], unsigned &ok) {
    ok = valid;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = e[q];
    if (kList) {
      unsigned row[4];
      ok = check_rows(e, valid, n_rows, outer, row, bad);
      if (n_rows) {  // uniform; an empty column has no row 0, and no candidate that counts
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = col[row[q]];
      }
    }
  };

  const size_t stride = static_cast<size_t>(gridDim.x) * kAggWaves;
#pragma unroll 1
  for (size_t seg = static_cast<size_t>(blockIdx.x) * kAggWaves + wave; seg < segments; seg += stride) {
    const size_t vfirst = seg * kTakeSegment;
    if (vfirst >= vend) break;  // behind the last candidate, and so is every later segment of this wave
    if (vfirst >= a && vfirst + kTakeSegment <= vend) {  // a whole segment: every load issued before the first use
      const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (vfirst - a)) + lane;
      u32x4 e[kTakeGroups];
      unsigned x[kTakeGroups][4], ok[kTakeGroups];
#pragma unroll
      for (int g = 0; g < kTakeGroups; ++g) e[g] = kList ? s4[g * kWave] : __builtin_nontemporal_load(s4 + g * kWave);
#pragma unroll
      for (int g = 0; g < kTakeGroups; ++g) fetch(e[g], 0xfu, x[g], ok[g]);
#pragma unroll
      for (int g = 0; g < kTakeGroups; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) add(x[g][q], (ok[g] >> q) & 1u);
      }
    } else {
#pragma unroll 1
      for (int g = 0; g < kTakeGroups; ++g) {
        const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
        unsigned valid, x[4], ok;
        const u32x4 e = load_ragged(src, a, v0, vend, valid);
        fetch(e, valid, x, ok);
#pragma unroll
        for (int q = 0; q < 4; ++q) add(x[q], (ok >> q) & 1u);
      }
    }
  }
  if (kList && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);

  const AggRecord mine{wave_reduce_add_u64(acc.count), wave_reduce_add_u64(acc.sum), wave_reduce_min(acc.mn),
                       wave_reduce_max(acc.mx)};
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    AggRecord r = s_wave[0];
#pragma unroll
    for (int w = 1; w < kAggWaves; ++w) {
      r.count += s_wave[w].count;
      r.sum += s_wave[w].sum;
      r.mn = r.mn < s_wave[w].mn ? r.mn : s_wave[w].mn;
      r.mx = r.mx > s_wave[w].mx ? r.mx : s_wave[w].mx;
    }
    parts[blockIdx.x] = r;
  }
}

// one workgroup: the n_parts partial records -> out[4], MIN and MAX back from the x domain and extended to 64 bits
__global__ __launch_bounds__(kAggFoldThreads) void agg_fold_kernel(const AggRecord *__restrict__ parts, unsigned n_parts,
                                                                   unsigned flip, u64 *__restrict__ out) {
  __shared__ AggRecord s_wave[kAggFoldThreads / kWave];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  AggRecord r{0ull, 0ull, 0xFFFFFFFFull, 0ull};
  for (unsigned i = threadIdx.x; i < n_parts; i += kAggFoldThreads) {
    const AggRecord p = parts[i];
    r.count += p.count;
    r.sum += p.sum;
    r.mn = r.mn < p.mn ? r.mn : p.mn;
    r.mx = r.mx > p.mx ? r.mx : p.mx;
  }
  const AggRecord mine{wave_reduce_add_u64(r.count), wave_reduce_add_u64(r.sum),
                       wave_reduce_min(static_cast<unsigned>(r.mn)), wave_reduce_max(static_cast<unsigned>(r.mx))};
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    AggRecord all = s_wave[0];
#pragma unroll
    for (int w = 1; w < kAggFoldThreads / kWave; ++w) {
      all.count += s_wave[w].count;
      all.sum += s_wave[w].sum;
      all.mn = all.mn < s_wave[w].mn ? all.mn : s_wave[w].mn;
      all.mx = all.mx > s_wave[w].mx ? all.mx : s_wave[w].mx;
    }
    const unsigned mn = static_cast<unsigned>(all.mn) ^ flip, mx = static_cast<unsigned>(all.mx) ^ flip;
    out[0] = all.count;
    out[1] = all.sum;
    out[2] = flip ? static_cast<u64>(static_cast<long long>(static_cast<int>(mn))) : static_cast<u64>(mn);
    out[3] = flip ? static_cast<u64>(static_cast<long long>(static_cast<int>(mx))) : static_cast<u64>(mx);
  }
}

template <int kCols>
void launch_take(unsigned grid, hipStream_t s, const TakeCols &t, unsigned n_rows, const unsigned *rows, size_t capacity,
                 const u64 *count, unsigned a, bool outer, unsigned fill, unsigned *status, size_t segments) {
  hipLaunchKernelGGL((take_kernel<kCols>), dim3(grid), dim3(kTakeThreads), 0, s, t, n_rows, rows, capacity, count, a, outer,
                     fill, status, segments);
}

}  // namespace

extern "C" size_t dbench_take_workspace_bytes(size_t capacity) {
  if (!fits_32(capacity)) return 0;
  return take_layout(capacity).total;
}

extern "C" int dbench_take_u32(const uint32_t *const *cols, size_t n_cols, size_t n_rows, const uint32_t *rows,
                               const uint64_t *count, size_t capacity, int flags, uint32_t fill, uint32_t *const *outs,
                               void *workspace, size_t workspace_bytes, void *stream) {
  if (flags & ~DBENCH_TAKE_OUTER) return DBHIP_EINVAL;  // unknown bits, and DBENCH_TAKE_SIGNED: take moves bit patterns
  if (n_cols < 1 || n_cols > DBENCH_TAKE_MAX_COLS || !cols || !outs) return DBHIP_EINVAL;
  if (!fits_32(n_rows) || !fits_32(capacity)) return DBHIP_EINVAL;  // 32-bit row ids and positions
  if ((capacity && !rows) || (count && !rows)) return DBHIP_EINVAL;
  uintptr_t words = addr(rows);
  for (size_t c = 0; c < n_cols; ++c) {
    if ((n_rows && capacity && !cols[c]) || !outs[c]) return DBHIP_EINVAL;
    words |= addr(cols[c]) | addr(outs[c]);
  }
  if ((words & 3u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  for (size_t c = 0; c < n_cols; ++c) {
    if (overlap(outs[c], 4 * capacity, rows, 4 * capacity) || overlap(outs[c], 4 * capacity, count, 8)) return DBHIP_EINVAL;
    for (size_t k = 0; k < n_cols; ++k) {
      if (overlap(outs[c], 4 * capacity, cols[k], 4 * n_rows)) return DBHIP_EINVAL;
      if (k < c && overlap(outs[c], 4 * capacity, outs[k], 4 * capacity)) return DBHIP_EINVAL;
    }
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, take_layout(capacity).total, s);
  if (rc != DBHIP_OK) return rc;
  if (!capacity) return launch_status();

  unsigned *status = static_cast<unsigned *>(workspace);

  const unsigned a = words_past_16(rows);
  const size_t segments = (capacity + a + kTakeSegment - 1) / kTakeSegment;
  const unsigned grid = static_cast<unsigned>((segments + kTakeWaves - 1) / kTakeWaves);
  TakeCols t{};
  for (size_t c = 0; c < n_cols; ++c) {
    t.col[c] = cols[c];
    t.out[c] = outs[c];
    t.shift[c] = (words_past_16(outs[c]) - a) & 3u;
  }
  const bool outer = (flags & DBENCH_TAKE_OUTER) != 0;
  const u64 *cnt = reinterpret_cast<const u64 *>(count);
  const unsigned n = static_cast<unsigned>(n_rows);
  switch (n_cols) {
    case 1: launch_take<1>(grid, s, t, n, rows, capacity, cnt, a, outer, fill, status, segments); break;
    case 2: launch_take<2>(grid, s, t, n, rows, capacity, cnt, a, outer, fill, status, segments); break;
    case 3: launch_take<3>(grid, s, t, n, rows, capacity, cnt, a, outer, fill, status, segments); break;
    default: launch_take<4>(grid, s, t, n, rows, capacity, cnt, a, outer, fill, status, segments); break;
  }
  return launch_status();
}

extern "C" int dbench_aggregate_rows_u32(const uint32_t *col, size_t n_rows, const uint32_t *rows, const uint64_t *count,
                                         size_t capacity, int flags, uint64_t *out, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  if (flags & ~(DBENCH_TAKE_OUTER | DBENCH_TAKE_SIGNED)) return DBHIP_EINVAL;
  if (!fits_32(n_rows) || !fits_32(capacity)) return DBHIP_EINVAL;  // 32-bit row ids and positions
  const bool list = rows != nullptr;
  if ((n_rows && (list ? capacity != 0 : true) && !col) || (count && !rows) || !out) return DBHIP_EINVAL;
  if (((addr(col) | addr(rows)) & 3u) || ((addr(count) | addr(out)) & 7u)) return DBHIP_EINVAL;
  const size_t candidates = list ? capacity : n_rows;
  if (overlap(out, 32, col, 4 * n_rows) || overlap(out, 32, rows, 4 * capacity) || overlap(out, 32, count, 8))
    return DBHIP_EINVAL;
  // the aggregate over all rows asks for the smallest workspace and takes the partial records the given one holds
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, take_layout(list ? capacity : 0).total, s);
  if (rc != DBHIP_OK) return rc;

  unsigned *status = static_cast<unsigned *>(workspace);
  AggRecord *parts = reinterpret_cast<AggRecord *>(static_cast<char *>(workspace) + kWsHeader);

  const unsigned a = candidates ? words_past_16(list ? rows : col) : 0u;
  const size_t segments = candidates ? (candidates + a + kTakeSegment - 1) / kTakeSegment : 0;
  size_t room = (workspace_bytes - kWsHeader) / sizeof(AggRecord);
  if (room > kAggMaxParts) room = kAggMaxParts;
  size_t grid = (segments + kAggWaves - 1) / kAggWaves;
  if (grid > room) grid = room;
  const unsigned flip = (flags & DBENCH_TAKE_SIGNED) ? 0x80000000u : 0u;
  const bool outer = (flags & DBENCH_TAKE_OUTER) != 0;
  if (grid) {
    if (list)
      hipLaunchKernelGGL((agg_kernel<true>), dim3(static_cast<unsigned>(grid)), dim3(kAggThreads), 0, s, col,
                         static_cast<unsigned>(n_rows), rows, capacity, reinterpret_cast<const u64 *>(count), a, flip, outer,
                         status, parts, segments);
    else
      hipLaunchKernelGGL((agg_kernel<false>), dim3(static_cast<unsigned>(grid)), dim3(kAggThreads), 0, s, col,
                         static_cast<unsigned>(n_rows), col, n_rows, static_cast<const u64 *>(nullptr), a, flip, false, status,
                         parts, segments);
  }
  hipLaunchKernelGGL(agg_fold_kernel, dim3(1), dim3(kAggFoldThreads), 0, s, parts, static_cast<unsigned>(grid), flip,
                     reinterpret_cast<u64 *>(out));
  return launch_status();
}
