// hll_sketch.cpp — a HyperLogLog sketch over 1 .. 4 32-bit columns on gfx950 (hll_sketch.hpp holds the contract,
// hll_layout.hpp the hash and the placement, which the kernels below and the host check run as the same text).
//
// build   a persistent grid (at most DBENCH_HLL_MAX_GRID workgroups of eight waves) walks the candidates as
//         bloom_build_kernel walks its keys: positions are counted from the 16-byte boundary in front of column 0 (or the
//         list), a lane holds four consecutive entries per group of 256 (one aligned 16-byte load; the further columns of a
//         dense build sit at their own alignment and are read as 16 bytes at 4-byte alignment; in list mode four 4-byte
//         gathers per column, row 0 standing in for an entry that does not count), the ragged ends word by word
//         (load_ragged).  A segment of 4096 positions belongs to a WORKGROUP here, two groups to each wave, both in flight:
//         the grid is full from 2^22 rows on and a workgroup clears and stores its registers once for all its segments.
//         The m registers live in LDS as one 32-bit word each (64 KiB at p = 14, two workgroups to a CU's 160 KiB): a plain
//         LDS read, and the no-return LDS max only where the rank is larger (a stale read costs a redundant atomic, never
//         a wrong register).  At the end the workgroup packs its registers to bytes into its own slot of the workspace.
// reduce  one workgroup per 256 registers, its four waves sharing the slots of the workgroups that were launched; under
//         accumulate (and in merge) the old bytes join, clamped to q+1.  It writes the bytes and a partial histogram.
// hist    one wave adds the partial histograms.
#include "hll_sketch.hpp"

#include "hll_layout.hpp"
#include "rowlist.hpp"
#include "select_write.hpp"

namespace {
using namespace dbhip;

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // 16-byte access at 4-byte alignment

constexpr int kHllWaves = 8;
constexpr int kHllThreads = kHllWaves * kWave;
constexpr int kHllWaveGroups = kSelGroups / kHllWaves;  // groups of 256 positions a wave takes of each segment
constexpr unsigned kHllMaxM = 1u << DBENCH_HLL_MAX_P;
constexpr unsigned kHllMinSegments = 2;  // segments a workgroup takes at least where there are as many
constexpr int kRedThreads = 256, kRedWaves = kRedThreads / kWave;
constexpr unsigned kRedRegs = 256;                          // registers of one reduce workgroup: four bytes per lane
constexpr unsigned kHllParts = kHllMaxM / kRedRegs;         // reduce workgroups at p = 14
constexpr size_t kHllPartBytes = sizeof(unsigned) * DBENCH_HLL_HIST_WORDS;
constexpr size_t kHllSlotsAt = kWsHeader + kHllParts * kHllPartBytes;
static_assert(kHllWaveGroups == 2 && kHllWaves * kHllWaveGroups == kSelGroups, "two groups of a segment per wave");
static_assert(DBENCH_HLL_HIST_WORDS == kWave, "one lane of the hist kernel's wave per histogram word");

#ifdef DBENCH_HLL_ALWAYS_MAX /* measurement only (tools/ab.py hll): a build without test-before-set */
constexpr bool kBuildTests = false;
#else
constexpr bool kBuildTests = true;
#endif

struct HllCols {
  const unsigned *p[DBENCH_HLL_MAX_COLS];
};

// the lane's four entries e at positions v0 .. v0+3 (bit q of `valid`: entry q exists; entry q of column 0 is row
// v0 + q - a) -> the hashes of the four key tuples and the entries `ok` that count; in list mode through the columns, and
// `bad` collects a row id >= n_col
template <int kCols, bool kList>
__device__ __forceinline__ void hll_fetch(const HllCols &c, unsigned n_col, const u32x4 e, size_t v0, unsigned a,
                                          unsigned valid, unsigned seed, HllHash (&s)[4], unsigned &ok, bool &bad) {
  const unsigned w[4] = {e.x, e.y, e.z, e.w};
  ok = valid;
  unsigned x[kCols][4];
  if (kList) {
    unsigned row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool inside = w[q] < n_col;
      bad = bad || (((valid >> q) & 1u) && !inside);
      if (!inside) ok &= ~(1u << q);
      row[q] = ((ok >> q) & 1u) ? w[q] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) x[j][q] = 0u;
      if (n_col) {  // uniform; an empty column has no row 0, and no entry that counts
#pragma unroll
        for (int q = 0; q < 4; ++q) x[j][q] = c.p[j][row[q]];
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) x[0][q] = w[q];
#pragma unroll
    for (int j = 1; j < kCols; ++j) {
      if (valid == 0xfu) {  // rows v0 - a .. v0 - a + 3 all exist
        const u32x4_a4 t = *reinterpret_cast<const u32x4_a4 *>(c.p[j] + (v0 - a));
        x[j][0] = t.x, x[j][1] = t.y, x[j][2] = t.z, x[j][3] = t.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[j][q] = ((valid >> q) & 1u) ? c.p[j][v0 + q - a] : 0u;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[q] = hll_hash_first(x[0][q], seed);
#pragma unroll
    for (int j = 1; j < kCols; ++j) s[q] = hll_hash_next(s[q], x[j][q]);
  }
}

// ---------------------------------------------------------------------------------------------
// build: the candidates -> one partial sketch per workgroup
// ---------------------------------------------------------------------------------------------
// kList: `src` is the row-id list (gathered through into the columns), otherwise column 0 itself.  m_host entries at most;
// *count (nullable) lowers it on the device.  slots: gridDim.x partial sketches of 2^p bytes
template <int kCols, bool kList>
__global__ __launch_bounds__(kHllThreads) void hll_build_kernel(const HllCols cols, unsigned n_col,
                                                                const unsigned *__restrict__ src, size_t m_host,
                                                                const u64 *count, unsigned a, unsigned seed, unsigned p,
                                                                unsigned *__restrict__ slots, unsigned *status,
                                                                size_t segments) {
  __shared__ unsigned s_reg[kHllMaxM];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned m_regs = 1u << p;
  for (unsigned i = threadIdx.x; i < m_regs; i += kHllThreads) s_reg[i] = 0u;
  __syncthreads();

  const size_t m = clamped_count(count, m_host);
  const size_t vend = a + m;  // positions [a, vend) hold entries
  bool bad = false;

  auto offer = [&](const HllHash (&s)[4], unsigned ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const HllPlace at = hll_place(s[q].h, s[q].g, p);
      if (((ok >> q) & 1u) && (!kBuildTests || s_reg[at.idx] < at.rank))  // the result is not used: a no-return LDS max
        __hip_atomic_fetch_max(&s_reg[at.idx], at.rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };

#pragma unroll 1
  for (size_t seg = blockIdx.x; seg < segments; seg += gridDim.x) {  // uniform over the workgroup; no barrier inside
    const size_t vfirst = seg * kSelSegment;
    if (vfirst >= vend) break;  // this segment and all behind it lie behind the last entry
    const int g0 = static_cast<int>(wave) * kHllWaveGroups;
    if (vfirst >= a && vfirst + kSelSegment <= vend) {  // a whole segment: two aligned 16-byte loads per lane, both in flight
      const size_t v0 = vfirst + static_cast<size_t>(g0) * (4 * kWave) + 4 * lane;
      const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (v0 - a));
      const u32x4 e0 = s4[0], e1 = s4[kWave];
      HllHash h0[4], h1[4];
      unsigned ok0, ok1;
      hll_fetch<kCols, kList>(cols, n_col, e0, v0, a, 0xfu, seed, h0, ok0, bad);
      hll_fetch<kCols, kList>(cols, n_col, e1, v0 + 4 * kWave, a, 0xfu, seed, h1, ok1, bad);
      offer(h0, ok0);
      offer(h1, ok1);
    } else {  // the first segment of an array that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
      for (int g = g0; g < g0 + kHllWaveGroups; ++g) {
        const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
        unsigned valid, ok;
        HllHash h[4];
        const u32x4 e = load_ragged(src, a, v0, vend, valid);
        hll_fetch<kCols, kList>(cols, n_col, e, v0, a, valid, seed, h, ok, bad);
        offer(h, ok);
      }
    }
  }
  if (kList && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);

  __syncthreads();
  unsigned *mine = slots + static_cast<size_t>(blockIdx.x) * (m_regs / 4);  // m_regs >= 16: whole words
  for (unsigned i = threadIdx.x; i < m_regs / 4; i += kHllThreads)
    mine[i] = s_reg[4 * i] | (s_reg[4 * i + 1] << 8) | (s_reg[4 * i + 2] << 16) | (s_reg[4 * i + 3] << 24);
}

// ---------------------------------------------------------------------------------------------
// reduce: the partial sketches (and the old registers) -> the registers and partial histograms
// ---------------------------------------------------------------------------------------------
// slots: n_slots sketches of 2^p bytes each, 4-byte aligned.  kClampSlots: a slot is a caller's sketch (merge), whose bytes
// above q+1 count as q+1 and raise the status like the old registers' do.  old: join the bytes `registers` holds
template <bool kClampSlots>
__global__ __launch_bounds__(kRedThreads) void hll_reduce_kernel(const unsigned *slots, unsigned n_slots, bool old, unsigned p,
                                                                 unsigned *registers, unsigned *__restrict__ parts,
                                                                 unsigned *status) {
  __shared__ unsigned s_max[kRedRegs];
  __shared__ unsigned s_hist[DBENCH_HLL_HIST_WORDS];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned words = (1u << p) / 4;                 // 32-bit words of a sketch
  const unsigned word = blockIdx.x * (kRedRegs / 4) + lane;  // this lane's four registers
  const bool mine = word < words;
  const unsigned top = 64u - p + 1u;
  s_max[threadIdx.x] = 0u;
  if (threadIdx.x < DBENCH_HLL_HIST_WORDS) s_hist[threadIdx.x] = 0u;
  __syncthreads();

  bool bad = false;
  unsigned r[4] = {0u, 0u, 0u, 0u};
  auto join = [&](unsigned packed, bool clamp) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      unsigned v = (packed >> (8 * b)) & 0xffu;
      if (clamp && v > top) {
        v = top;
        bad = true;
      }
      r[b] = r[b] > v ? r[b] : v;
    }
  };
  if (mine) {
    for (unsigned s = wave; s < n_slots; s += kRedWaves) join(slots[static_cast<size_t>(s) * words + word], kClampSlots);
    if (old && wave == 0) join(registers[word], true);
#pragma unroll
    for (int b = 0; b < 4; ++b)  // the result is not used: a no-return LDS max
      __hip_atomic_fetch_max(&s_max[4 * lane + b], r[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (__ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
  __syncthreads();  // every read of `registers` (and of src == dst) lies in front of this barrier, the store behind it
  if (wave == 0 && mine) {
    unsigned packed = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const unsigned v = s_max[4 * lane + b];  // <= q+1 < 64
      packed |= v << (8 * b);
      __hip_atomic_fetch_add(&s_hist[v & (DBENCH_HLL_HIST_WORDS - 1)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    registers[word] = packed;
  }
  __syncthreads();
  if (threadIdx.x < DBENCH_HLL_HIST_WORDS) parts[blockIdx.x * DBENCH_HLL_HIST_WORDS + threadIdx.x] = s_hist[threadIdx.x];
}

__global__ __launch_bounds__(kWave) void hll_hist_kernel(const unsigned *__restrict__ parts, unsigned n_parts,
                                                         unsigned *__restrict__ hist) {
  unsigned sum = 0;
  for (unsigned i = 0; i < n_parts; ++i) sum += parts[i * DBENCH_HLL_HIST_WORDS + threadIdx.x];
  hist[threadIdx.x] = sum;
}

unsigned reduce_parts(unsigned p) { return ((1u << p) + kRedRegs - 1) / kRedRegs; }

// the two launches behind the partial sketches (or behind src, in merge)
template <bool kClampSlots>
void launch_reduce(const unsigned *slots, unsigned n_slots, bool old, unsigned p, uint8_t *registers, uint32_t *hist,
                   void *workspace, hipStream_t s) {
  unsigned *status = static_cast<unsigned *>(workspace);
  unsigned *parts = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + kWsHeader);
  const unsigned n_parts = reduce_parts(p);
  hipLaunchKernelGGL((hll_reduce_kernel<kClampSlots>), dim3(n_parts), dim3(kRedThreads), 0, s, slots, n_slots, old, p,
                     reinterpret_cast<unsigned *>(registers), parts, status);
  hipLaunchKernelGGL(hll_hist_kernel, dim3(1), dim3(kWave), 0, s, parts, n_parts, hist);
}

template <int kCols>
void launch_build(bool list, unsigned grid, hipStream_t s, const HllCols &c, unsigned n_col, const unsigned *src, size_t entries,
                  const u64 *count, unsigned a, unsigned seed, unsigned p, unsigned *slots, unsigned *status, size_t segments) {
  if (list)
    hipLaunchKernelGGL((hll_build_kernel<kCols, true>), dim3(grid), dim3(kHllThreads), 0, s, c, n_col, src, entries, count, a,
                       seed, p, slots, status, segments);
  else
    hipLaunchKernelGGL((hll_build_kernel<kCols, false>), dim3(grid), dim3(kHllThreads), 0, s, c, n_col, src, entries, count, a,
                       seed, p, slots, status, segments);
}

}  // namespace

extern "C" size_t dbench_hll_workspace_bytes(unsigned p) {
  if (!hll_p_ok(p)) return 0;
  return kHllSlotsAt + (static_cast<size_t>(DBENCH_HLL_MAX_GRID) << p);
}

extern "C" int dbench_hll_build_u32(const uint32_t *const *cols, int n_cols, size_t n_col, const uint32_t *rows,
                                    const uint64_t *count, size_t capacity, uint32_t seed, int flags, unsigned p,
                                    uint8_t *registers, uint32_t *hist, void *workspace, size_t workspace_bytes, void *stream) {
  if (flags & ~DBENCH_HLL_ACCUMULATE) return DBHIP_EINVAL;
  if (!hll_p_ok(p) || n_cols < 1 || n_cols > DBENCH_HLL_MAX_COLS) return DBHIP_EINVAL;
  if (!fits_32(n_col) || !fits_32(capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  if (!registers || !hist || !cols) return DBHIP_EINVAL;
  if ((addr(registers) & 3u) || (addr(hist) & 7u) || (addr(rows) & 3u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  const size_t m_regs = static_cast<size_t>(1) << p;
  HllCols c = {};
  Range ins[DBENCH_HLL_MAX_COLS + 2];
  for (int j = 0; j < n_cols; ++j) {
    if ((n_col && !cols[j]) || (addr(cols[j]) & 3u)) return DBHIP_EINVAL;
    c.p[j] = cols[j];
    ins[j] = Range{cols[j], 4 * n_col};
  }
  ins[n_cols] = Range{rows, 4 * capacity};
  ins[n_cols + 1] = Range{count, 8};
  const Range outs[2] = {Range{registers, m_regs}, Range{hist, kHllPartBytes}};
  if (outputs_overlap(outs, 2, ins, n_cols + 2)) return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, dbench_hll_workspace_bytes(p), s);
  if (rc != DBHIP_OK) return rc;

  const bool list = rows != nullptr;
  const size_t entries = list ? capacity : n_col;
  unsigned *status = static_cast<unsigned *>(workspace);
  unsigned *slots = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + kHllSlotsAt);
  unsigned grid = 0;
  if (entries) {
    const unsigned *src = list ? rows : c.p[0];
    const unsigned a = words_past_16(src);
    const size_t segments = (entries + a + kSelSegment - 1) / kSelSegment;
    const size_t wanted = (segments + kHllMinSegments - 1) / kHllMinSegments;
    grid = static_cast<unsigned>(wanted < DBENCH_HLL_MAX_GRID ? wanted : DBENCH_HLL_MAX_GRID);
    const u64 *cnt = reinterpret_cast<const u64 *>(count);
    const unsigned n = static_cast<unsigned>(n_col);
    switch (n_cols) {
      case 1: launch_build<1>(list, grid, s, c, n, src, entries, cnt, a, seed, p, slots, status, segments); break;
      case 2: launch_build<2>(list, grid, s, c, n, src, entries, cnt, a, seed, p, slots, status, segments); break;
      case 3: launch_build<3>(list, grid, s, c, n, src, entries, cnt, a, seed, p, slots, status, segments); break;
      default: launch_build<4>(list, grid, s, c, n, src, entries, cnt, a, seed, p, slots, status, segments); break;
    }
  }
  launch_reduce<false>(slots, grid, (flags & DBENCH_HLL_ACCUMULATE) != 0, p, registers, hist, workspace, s);
  return launch_status();
}

extern "C" int dbench_hll_merge(uint8_t *dst_registers, const uint8_t *src_registers, unsigned p, uint32_t *hist,
                                void *workspace, size_t workspace_bytes, void *stream) {
  if (!hll_p_ok(p) || !dst_registers || !src_registers || !hist) return DBHIP_EINVAL;
  if (((addr(dst_registers) | addr(src_registers)) & 3u) || (addr(hist) & 7u)) return DBHIP_EINVAL;
  const size_t m_regs = static_cast<size_t>(1) << p;
  if (overlap(hist, kHllPartBytes, dst_registers, m_regs) || overlap(hist, kHllPartBytes, src_registers, m_regs))
    return DBHIP_EINVAL;
  if (dst_registers != src_registers && overlap(dst_registers, m_regs, src_registers, m_regs)) return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, kHllSlotsAt, s);
  if (rc != DBHIP_OK) return rc;
  launch_reduce<true>(reinterpret_cast<const unsigned *>(src_registers), 1u, true, p, dst_registers, hist, workspace, s);
  return launch_status();
}

extern "C" double dbench_hll_estimate(const uint32_t *hist, unsigned p) { return hll_estimate(hist, p); }
