// bitpack.cpp — bit-packed columns on gfx950 (bitpack.hpp holds the contract and the workspace layout, bitpack_layout.hpp
// the index arithmetic, which the kernels below run on global and LDS pointers): pack, unpack (dense, or take through a
// row-id list) and the range filter on packed codes that feeds the selection vectors.
//
// Which lane holds which rows.  A segment of 4096 rows is 128 groups of 32 rows, 128 x width words, a run of aligned
// 16-byte chunks.  Were a lane to own a group, it would walk its own `width` words and the 64 lanes of a load would touch
// 64 places `width` words apart; so the WAVE owns the run: it reads the chunks once with coalesced 16-byte loads (lane l
// chunk l, l + 64, ...) into a wave-private piece of LDS, and then lane l extracts row 64 j + l of the segment in step
// j: two LDS words and a funnel shift.  Neighbouring lanes read the same or neighbouring LDS words (width / 32 words
// apart), the 64 ballots of a segment are its match mask in row order, and an output column is stored 256 bytes per
// step.  Rows are counted from the segment's first, so the bit position is a 32-bit product, and a chunk of padding behind
// the piece lets both words of a code be read always (bitpack_extract_staged).  The LDS piece is dynamic, 512 x width + 16
// bytes per wave, so a narrow column keeps more waves on a compute unit.
// No barrier: a wave reads only what it staged itself (a wavefront fence and wave barrier order the two).
//   pack    a wave owns a tile of 2048 rows = 64 groups = 64 x width output words.  It loads the rows coalesced, subtracts
//           the base, checks and masks the codes and leaves them in LDS (33 words per group of 32: lanes 32 rows apart
//           fall on different banks); then lane l builds the output chunks l, l + 64, ... of the tile, each word from the
//           codes that reach into it (bitpack_group_word), and stores 16 bytes.  One lane per output word, no atomics.
//   unpack  dense: stage, extract, add the base, store.  Through a list: a lane loads its row id, bounds-checks it and
//           gathers the one or two words of the code from global memory (row 0 stands in for an id that does not count).
//   select  mark / scan / write as in select_rows.cpp, with the mask layout above; the predicate and the scan are the
//           same text (rowlist.hpp).  The dense mark kernel is the only reader of the packed column; the decoded column
//           never exists.
#include "bitpack.hpp"

#include <type_traits>

#include "bitpack_layout.hpp"
#include "rowlist.hpp"

namespace {
using namespace dbhip;

constexpr unsigned kBpSegment = DBENCH_BITPACK_SEGMENT_ROWS;
constexpr unsigned kBpTile = DBENCH_BITPACK_TILE_ROWS;
constexpr int kBpWaves = 2;  // segments of a workgroup, as in select_rows.cpp: a short list spreads over more compute units
constexpr int kBpThreads = kBpWaves * kWave;
constexpr int kBpSteps = kBpSegment / kWave;       // ballots (mask words) of a segment, one per lane
constexpr unsigned kBpSegGroups = kBpSegment / 32;  // x width = the packed words of a whole segment
constexpr unsigned kBpPad = 4;  // words behind a wave's staged piece: bitpack_extract_staged reads one word past the code's first
constexpr int kPackWaves = 4;
constexpr int kPackThreads = kPackWaves * kWave;
constexpr int kPackLoads = kBpTile / kWave;          // rows of a lane
constexpr unsigned kPackGroups = kBpTile / 32;       // groups of a tile: x width = its output words
constexpr unsigned kPackStride = 33;                 // LDS words per group of 32 codes
constexpr int kBpAhead = 8;  // steps of the mark kernels whose loads are in flight together
static_assert(kBpSteps == kWave && kBpSteps % kBpAhead == 0, "a lane keeps one mask word of its wave's segment");
static_assert(kBpSegGroups % 4 == 0 && kPackGroups % 4 == 0, "segments and tiles start on a 16-byte chunk at any width");

// what one wave wrote to its piece of LDS is visible to all its lanes behind this
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the packed words of segment `seg` that exist, a multiple of 4: all 128 x width of them, or what the column's last
// segment holds
__device__ __forceinline__ unsigned segment_words(size_t seg, unsigned n_rows, unsigned width) {
  const u64 first = static_cast<u64>(seg) * kBpSegGroups * width, all = bitpack_words(n_rows, width);
  const u64 whole = static_cast<u64>(kBpSegGroups) * width;
  return static_cast<unsigned>(all - first < whole ? all - first : whole);
}

// words [first, first + n_words) of the column -> s[0 .. n_words), 16 bytes per lane and load, four loads in flight
__device__ __forceinline__ void stage_words(const unsigned *__restrict__ packed, u64 first, unsigned n_words, unsigned *s,
                                            unsigned lane) {
  const u32x4 *g = reinterpret_cast<const u32x4 *>(packed + first);
  u32x4 *d = reinterpret_cast<u32x4 *>(s);
  const unsigned chunks = n_words >> 2;
#pragma unroll 1
  for (unsigned c = lane; c < chunks; c += 4 * kWave) {
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c + j * kWave < chunks) v[j] = __builtin_nontemporal_load(g + c + j * kWave);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c + j * kWave < chunks) d[c + j * kWave] = v[j];
    }
  }
  wave_lds_sync();
}

// ---------------------------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPackThreads) void bp_pack_kernel(const unsigned *__restrict__ col, size_t capacity,
                                                               const u64 *count, unsigned width, unsigned base,
                                                               unsigned *__restrict__ out, unsigned *status, size_t tiles) {
  __shared__ unsigned s_codes[kPackWaves][kPackGroups * kPackStride];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t tile = static_cast<size_t>(blockIdx.x) * kPackWaves + wave;
  if (tile >= tiles) return;  // uniform over the wave; no workgroup barrier below
  const size_t m = clamped_count(count, capacity);
  const size_t first = tile * kBpTile;
  if (first >= m) return;  // a tile behind the last row: the words of the column end inside an earlier tile
  const unsigned here = m - first < kBpTile ? static_cast<unsigned>(m - first) : kBpTile;
  const unsigned mask = bitpack_mask(width);
  unsigned *s = s_codes[wave];
  bool bad = false;
#pragma unroll 8
  for (int k = 0; k < kPackLoads; ++k) {
    const unsigned i = k * kWave + lane;
    unsigned code = 0;  // rows behind m: the zero tail of the last group
    if (i < here) {
      const unsigned c = col[first + i] - base;
      bad = bad || (c & ~mask) != 0;
      code = c & mask;
    }
    s[i + (i >> 5)] = code;  // kPackStride words per group
  }
  wave_lds_sync();
  if (__ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);

  const u64 first_word = static_cast<u64>(tile) * kPackGroups * width;  // a multiple of 4
  const u64 left = bitpack_words(m, width) - first_word, whole = static_cast<u64>(kPackGroups) * width;
  const unsigned chunks = static_cast<unsigned>(left < whole ? left : whole) >> 2;
  u32x4 *o4 = reinterpret_cast<u32x4 *>(out + first_word);
#pragma unroll 1
  for (unsigned c = lane; c < chunks; c += kWave) {
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned o = 4 * c + q, g = o / width, t = o - g * width;  // word t of group g of the tile
      const unsigned *codes = s + g * kPackStride;
      w[q] = bitpack_group_word(codes, t, width);
    }
    o4[c] = u32x4{w[0], w[1], w[2], w[3]};
  }
}

// ---------------------------------------------------------------------------------------------
// unpack
// ---------------------------------------------------------------------------------------------
// kList: out[i] = decode(rows[i]) for i < m = min(*count, m_host); otherwise out[i] = decode(i) for i < m_host = n_rows
template <bool kList>
__global__ __launch_bounds__(kBpThreads) void bp_unpack_kernel(const unsigned *__restrict__ packed, unsigned n_rows,
                                                               unsigned width, unsigned base,
                                                               const unsigned *__restrict__ rows, size_t m_host,
                                                               const u64 *count, bool outer, unsigned fill,
                                                               unsigned *__restrict__ out, unsigned *status, size_t segments) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kBpWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no workgroup barrier below
  const size_t m = kList ? clamped_count(count, m_host) : m_host;
  const size_t first = seg * kBpSegment;
  if (first >= m) return;
  const unsigned here = m - first < kBpSegment ? static_cast<unsigned>(m - first) : kBpSegment;
  const int steps = static_cast<int>((here + kWave - 1) / kWave);
  if (!kList) {
    unsigned *s = s_dyn + wave * (kBpSegGroups * width + kBpPad);
    const u64 origin = static_cast<u64>(seg) * kBpSegGroups * width;
    stage_words(packed, origin, segment_words(seg, n_rows, width), s, lane);
#pragma unroll 8
    for (int j = 0; j < steps; ++j) {  // the segment starts at a group boundary: row i of it is row i of the staged piece
      const unsigned i = j * kWave + lane;
      if (i < here) out[first + i] = base + bitpack_extract_staged(s, i, width);
    }
  } else {
    bool bad = false;
#pragma unroll 4
    for (int j = 0; j < steps; ++j) {
      const unsigned i = j * kWave + lane;
      const bool valid = i < here;
      const unsigned r = rows[first + (valid ? i : 0u)];  // entry `first` exists
      const bool inside = r < n_rows;
      bad = bad || (valid && !inside && !(outer && r == 0xFFFFFFFFu));
      unsigned x = fill;
      if (n_rows) {  // uniform; an empty column has no row 0, and every entry is filled
        const unsigned v = base + bitpack_extract(packed, inside ? r : 0u, width);
        x = inside ? v : fill;
      }
      if (valid) out[first + i] = x;
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
  }
}

// ---------------------------------------------------------------------------------------------
// select_range
// ---------------------------------------------------------------------------------------------
// kList: the candidates are rows[0 .. m), m = min(*in_count, m_host); otherwise rows 0 .. m_host - 1 = n_rows - 1
template <bool kList>
__global__ __launch_bounds__(kBpThreads) void bp_mark_kernel(const unsigned *__restrict__ packed, unsigned n_rows,
                                                             unsigned width, unsigned base,
                                                             const unsigned *__restrict__ rows, size_t m_host,
                                                             const u64 *in_count, RangePred p, unsigned *status,
                                                             unsigned *__restrict__ cnt, u64 *__restrict__ masks,
                                                             size_t segments) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kBpWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no workgroup barrier below
  const size_t m = kList ? clamped_count(in_count, m_host) : m_host;
  const size_t first = seg * kBpSegment;
  u64 mine = 0;        // mask word `lane` of the segment
  unsigned total = 0;  // matches of the segment (wave-uniform)
  if (first < m) {     // otherwise a segment behind the last candidate: zero count, zero masks
    const unsigned here = m - first < kBpSegment ? static_cast<unsigned>(m - first) : kBpSegment;
    const int steps = static_cast<int>((here + kWave - 1) / kWave);
    if (!kList) {
      unsigned *s = s_dyn + wave * (kBpSegGroups * width + kBpPad);
      const u64 origin = static_cast<u64>(seg) * kBpSegGroups * width;
      stage_words(packed, origin, segment_words(seg, n_rows, width), s, lane);
      // whole rounds (a ballot is not unrolled with a remainder); the segment starts at a group boundary, so row i of it
      // is row i of the staged piece.  A whole segment votes without a bounds check; in the column's last one the steps
      // behind the last row vote no (their reads stay inside the wave's piece of LDS, what they return is not used)
      auto round = [&](int j0, auto whole) {
        unsigned x[kBpAhead];
#pragma unroll
        for (int k = 0; k < kBpAhead; ++k) x[k] = base + bitpack_extract_staged(s, (j0 + k) * kWave + lane, width);
#pragma unroll
        for (int k = 0; k < kBpAhead; ++k) {
          const bool valid = decltype(whole)::value || (j0 + k) * kWave + lane < here;
          const u64 b = __ballot(valid && range_keep(x[k], p));
          total += static_cast<unsigned>(__popcll(b));
          if (lane == static_cast<unsigned>(j0 + k)) mine = b;
        }
      };
      if (here == kBpSegment) {
#pragma unroll 1
        for (int j0 = 0; j0 < kBpSteps; j0 += kBpAhead) round(j0, std::true_type{});
      } else {
#pragma unroll 1
        for (int j0 = 0; j0 < steps; j0 += kBpAhead) round(j0, std::false_type{});
      }
    } else {
      bool bad = false;
#pragma unroll 1
      for (int j0 = 0; j0 < steps; j0 += kBpAhead) {
        unsigned r[kBpAhead], x[kBpAhead];
#pragma unroll
        for (int k = 0; k < kBpAhead; ++k) {
          const unsigned i = (j0 + k) * kWave + lane;
          r[k] = rows[first + (i < here ? i : 0u)];  // entry `first` exists
        }
#pragma unroll
        for (int k = 0; k < kBpAhead; ++k) {  // the gathers are unconditional: row 0 stands in for an id that does not count
          x[k] = 0;
          if (n_rows) x[k] = base + bitpack_extract(packed, r[k] < n_rows ? r[k] : 0u, width);  // uniform branch
        }
#pragma unroll
        for (int k = 0; k < kBpAhead; ++k) {
          const unsigned i = (j0 + k) * kWave + lane;
          const bool valid = i < here, inside = r[k] < n_rows;
          bad = bad || (valid && !inside);
          const u64 b = __ballot(valid && inside && range_keep(x[k], p));
          total += static_cast<unsigned>(__popcll(b));
          if (lane == static_cast<unsigned>(j0 + k)) mine = b;
        }
      }
      if (__ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
    }
  }
  masks[seg * kBpSteps + lane] = mine;
  if (lane == 0) cnt[seg] = total;
}

// a wave writes its segment's kept row ids, in candidate order, from pos[segment] on
template <bool kList>
__global__ __launch_bounds__(kBpThreads) void bp_write_kernel(const unsigned *__restrict__ rows,
                                                              const unsigned *__restrict__ cnt,
                                                              const unsigned *__restrict__ pos,
                                                              const u64 *__restrict__ masks, size_t segments,
                                                              unsigned *__restrict__ out, size_t out_capacity) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kBpWaves + wave;
  if (seg >= segments) return;  // uniform over the wave
  const unsigned c = cnt[seg];
  if (c == 0) return;  // nothing kept in this segment: neither its masks nor its row ids are read
  size_t run = pos[seg];  // next output position (wave-uniform)
  const size_t end = run + c;
  if (end > out_capacity) return;  // cannot happen with this call's own counts; nothing is ever written past the buffer
  const u64 mine = masks[seg * kBpSteps + lane];
  const unsigned mine_lo = static_cast<unsigned>(mine), mine_hi = static_cast<unsigned>(mine >> 32);
  const size_t first = seg * kBpSegment;
#pragma unroll 1
  for (int j = 0; j < kBpSteps; ++j) {
    // (the builtin returns int: through unsigned, or the low half's sign bit would fill the high half)
    const unsigned b_lo = __builtin_amdgcn_readlane(mine_lo, j), b_hi = __builtin_amdgcn_readlane(mine_hi, j);
    const u64 b = b_lo | static_cast<u64>(b_hi) << 32;
    if (b == 0) continue;  // uniform
    if ((b >> lane) & 1ull) {
      const size_t i = first + static_cast<size_t>(j) * kWave + lane;  // a kept candidate: below m, so inside the list
      const size_t at = run + mbcnt(b);
      const unsigned id = kList ? rows[i] : static_cast<unsigned>(i);
      if (at < end) out[at] = id;
    }
    run += static_cast<unsigned>(__popcll(b));
  }
}

bool width_ok(unsigned width) { return width >= 1 && width <= 32; }
size_t lds_bytes(unsigned width) { return sizeof(unsigned) * kBpWaves * (kBpSegGroups * width + kBpPad); }  // at most 32 KiB + 32

}  // namespace

extern "C" size_t dbench_bitpack_words(size_t n_rows, unsigned width) {
  return static_cast<size_t>(bitpack_words(n_rows, width));
}

extern "C" size_t dbench_bitpack_workspace_bytes(size_t capacity) {
  if (!fits_32(capacity)) return 0;
  return static_cast<size_t>(bitpack_layout(capacity).total);
}

extern "C" int dbench_bitpack_pack_u32(const uint32_t *col, size_t capacity, const uint64_t *count, unsigned width,
                                       uint32_t base, uint32_t *out_packed, void *workspace, size_t workspace_bytes,
                                       void *stream) {
  if (!width_ok(width) || !fits_32(capacity)) return DBHIP_EINVAL;
  if (capacity && (!col || !out_packed)) return DBHIP_EINVAL;
  if ((addr(col) & 3u) || (addr(out_packed) & 15u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  const size_t out_bytes = 4 * static_cast<size_t>(bitpack_words(capacity, width));
  if (overlap(out_packed, out_bytes, col, 4 * capacity) || overlap(out_packed, out_bytes, count, 8)) return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, static_cast<size_t>(bitpack_layout(0).total), s);
  if (rc != DBHIP_OK) return rc;
  if (!capacity) return launch_status();
  const size_t tiles = (capacity + kBpTile - 1) / kBpTile;
  const unsigned grid = static_cast<unsigned>((tiles + kPackWaves - 1) / kPackWaves);
  hipLaunchKernelGGL(bp_pack_kernel, dim3(grid), dim3(kPackThreads), 0, s, col, capacity,
                     reinterpret_cast<const u64 *>(count), width, base, out_packed, static_cast<unsigned *>(workspace), tiles);
  return launch_status();
}

extern "C" int dbench_bitpack_unpack_u32(const uint32_t *packed, size_t n_rows, unsigned width, uint32_t base,
                                         const uint32_t *rows, const uint64_t *count, size_t capacity, int flags,
                                         uint32_t fill, uint32_t *out, void *workspace, size_t workspace_bytes,
                                         void *stream) {
  if (!width_ok(width) || (flags & ~DBENCH_BITPACK_OUTER)) return DBHIP_EINVAL;
  const bool list = rows != nullptr;
  if (!fits_32(n_rows) || (list && !fits_32(capacity))) return DBHIP_EINVAL;  // 32-bit row ids and positions
  if (count && !rows) return DBHIP_EINVAL;
  const size_t entries = list ? capacity : n_rows;
  if ((n_rows && entries && !packed) || (entries && !out)) return DBHIP_EINVAL;
  if ((addr(packed) & 15u) || ((addr(rows) | addr(out)) & 3u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  const size_t packed_bytes = 4 * static_cast<size_t>(bitpack_words(n_rows, width));
  if (overlap(out, 4 * entries, packed, packed_bytes) || overlap(out, 4 * entries, rows, 4 * entries) ||
      overlap(out, 4 * entries, count, 8))
    return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, static_cast<size_t>(bitpack_layout(0).total), s);
  if (rc != DBHIP_OK) return rc;
  if (!entries) return launch_status();
  unsigned *status = static_cast<unsigned *>(workspace);
  const size_t segments = (entries + kBpSegment - 1) / kBpSegment;
  const unsigned grid = static_cast<unsigned>((segments + kBpWaves - 1) / kBpWaves);
  const unsigned n = static_cast<unsigned>(n_rows);
  if (list)
    hipLaunchKernelGGL((bp_unpack_kernel<true>), dim3(grid), dim3(kBpThreads), 0, s, packed, n, width, base, rows, capacity,
                       reinterpret_cast<const u64 *>(count), (flags & DBENCH_BITPACK_OUTER) != 0, fill, out, status, segments);
  else
    hipLaunchKernelGGL((bp_unpack_kernel<false>), dim3(grid), dim3(kBpThreads), lds_bytes(width), s, packed, n, width, base,
                       static_cast<const unsigned *>(nullptr), n_rows, static_cast<const u64 *>(nullptr), false, fill, out,
                       status, segments);
  return launch_status();
}

extern "C" int dbench_bitpack_select_range_u32(const uint32_t *packed, size_t n_rows, unsigned width, uint32_t base,
                                               const uint32_t *in_rows, const uint64_t *in_count, size_t in_capacity,
                                               uint32_t lo, uint32_t hi, int flags, uint32_t *out_rows, uint64_t *out_count,
                                               void *workspace, size_t workspace_bytes, void *stream) {
  if (!width_ok(width) || (flags & ~(DBENCH_BITPACK_SIGNED | DBENCH_BITPACK_NEGATE))) return DBHIP_EINVAL;
  if (!fits_32(n_rows) || !fits_32(in_capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  if ((n_rows && !packed) || !out_count || (in_count && !in_rows)) return DBHIP_EINVAL;
  if ((addr(packed) & 15u) || ((addr(in_rows) | addr(out_rows)) & 3u) || ((addr(in_count) | addr(out_count)) & 7u))
    return DBHIP_EINVAL;
  const bool list = in_rows != nullptr;
  const size_t candidates = list ? in_capacity : n_rows;
  const size_t packed_bytes = 4 * static_cast<size_t>(bitpack_words(n_rows, width));
  if (overlap(out_rows, 4 * candidates, packed, packed_bytes) || overlap(out_rows, 4 * candidates, in_rows, 4 * in_capacity))
    return DBHIP_EINVAL;
  const BitpackLayout l = bitpack_layout(candidates);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, static_cast<size_t>(l.total), s);
  if (rc != DBHIP_OK) return rc;

  char *ws = static_cast<char *>(workspace);
  unsigned *status = reinterpret_cast<unsigned *>(ws);
  unsigned *cnt = reinterpret_cast<unsigned *>(ws + l.cnt);
  unsigned *pos = reinterpret_cast<unsigned *>(ws + l.pos);
  u64 *masks = reinterpret_cast<u64 *>(ws + l.masks);

  const size_t segments = static_cast<size_t>(l.segments);
  const unsigned grid = static_cast<unsigned>((segments + kBpWaves - 1) / kBpWaves);
  const unsigned flip = (flags & DBENCH_BITPACK_SIGNED) ? 0x80000000u : 0u;
  const RangePred p{flip, lo ^ flip, hi ^ flip, (flags & DBENCH_BITPACK_NEGATE) != 0};
  const unsigned n = static_cast<unsigned>(n_rows);
  if (segments) {
    if (list)
      hipLaunchKernelGGL((bp_mark_kernel<true>), dim3(grid), dim3(kBpThreads), 0, s, packed, n, width, base, in_rows,
                         in_capacity, reinterpret_cast<const u64 *>(in_count), p, status, cnt, masks, segments);
    else
      hipLaunchKernelGGL((bp_mark_kernel<false>), dim3(grid), dim3(kBpThreads), lds_bytes(width), s, packed, n, width, base,
                         static_cast<const unsigned *>(nullptr), n_rows, static_cast<const u64 *>(nullptr), p, status, cnt,
                         masks, segments);
  }
  // (the write kernels stop at `candidates` as well)
  launch_rowlist_scan(cnt, pos, segments, candidates, reinterpret_cast<u64 *>(out_count), s);
  if (segments && out_rows) {
    if (list)
      hipLaunchKernelGGL((bp_write_kernel<true>), dim3(grid), dim3(kBpThreads), 0, s, in_rows, cnt, pos, masks, segments,
                         out_rows, candidates);
    else
      hipLaunchKernelGGL((bp_write_kernel<false>), dim3(grid), dim3(kBpThreads), 0, s, static_cast<const unsigned *>(nullptr),
                         cnt, pos, masks, segments, out_rows, candidates);
  }
  return launch_status();
}
