// partition.hip — the radix hash partitioner of the joins (join_lds.hip), the hash group-by (groupby_hash.hip) and the
// multi-GPU exchange (pjoin.hip): a column of keys, with row ids or payloads, becomes partition-major (key, row id)
// pairs in one or two levels of <= 1024-way scatter (jl_hist / jl_offsets / jl_scatter: LDS counts, one global
// reservation per bucket per tile, runs of pairs written contiguously; tiles of 4096 rows, of 16384 where a level has
// 512+ buckets; both histograms from ONE read of the keys up to 81920 partitions, above that level 0 leaves every row's
// level-1 bucket as a 16-bit column for the level-1 histogram to read instead of the pairs).  partition.hpp holds what
// callers need: the hashes, the geometry, the layout of `meta`, and the plan (jl_side_plan) that jl_partition_side
// launches.  Of the histograms, jl_hist1 and jl_hist1d stream through jl_stream, and they and jl_hist0 flush through
// jl_hist_flush_add; jl_hist0's stream, jl_hist_fused / fused16 and the two reduces are spelled out ("what the
// histogram kernels share" below).
#include "dbhip_common.hpp"
#include "partition.hpp"

namespace dbhip {
namespace {

#ifndef DBHIP_JL_KPT
#define DBHIP_JL_KPT 8
#endif
constexpr int kJlKpt = DBHIP_JL_KPT;
constexpr int kJlTile = kJlThreads * kJlKpt;  // 4096 rows per scatter tile, 36 KiB of LDS: four 512-thread workgroups
                                              // per CU.  Measured at 2^26 rows (build, us): 512x8 1361, 512x16 1423,
                                              // 1024x8 1390, 512x4 1442, 256x8 1499, 512x32 1687

template <bool RANK>
__device__ __forceinline__ unsigned jl_pid_sel(unsigned key, unsigned parts) {
  return RANK ? jl_rank_of(key, parts) : jl_pid(key, parts);
}

// ---- level 0: histogram per (tile group, bucket) (the kJlGroups tile groups: partition.hpp) -----------
constexpr unsigned kJlHistWgPerGroup = 32;

// rows of a tile group: a whole number of the level-0 scatter's tiles (`tile` rows each — the scatter comes in three
// tile shapes, see partition.hpp), so histogram and scatter agree on which rows are group g's
__host__ __device__ __forceinline__ size_t jl_group_rows(size_t n, unsigned tile) {
  const size_t tiles = (n + tile - 1) / tile;
  return (tiles + kJlGroups - 1) / kJlGroups * tile;
}

// ---- what the histogram kernels share -------------------------------------------------------------------------------
// All five zero an LDS histogram, let workgroup w of a group stride over a row range with several independent loads per
// lane per step, count each row, and flush.  The stream and the flush below are that text once for the kernels that
// compile to the same instructions through them (profiles/r23_partition_isa.txt); jl_hist0's stream, both
// fused kernels and the two reduces come out with a branch or two registers the other way round, and keep their text.

// Workgroup `w` of `wgs` strides over the elements [lo, hi) of `src`: LOADS independent loads per lane per step, all of
// a step issued before the first use, each(element) for every element in range.
template <auto THREADS, int LOADS, class T, class Each>
__device__ __forceinline__ void jl_stream(const T *src, size_t lo, size_t hi, unsigned w, unsigned wgs, Each each) {
  for (size_t i = lo + static_cast<size_t>(w) * LOADS * THREADS + threadIdx.x; i < hi;
       i += static_cast<size_t>(wgs) * LOADS * THREADS) {
    T v[LOADS];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) v[j] = i + j * THREADS < hi ? src[i + j * THREADS] : T{};
#pragma unroll
    for (int j = 0; j < LOADS; ++j)
      if (i + j * THREADS < hi) each(v[j]);
  }
}

// the non-zero counters of the LDS histogram onto the 64-bit global counters dst[0 .. words)
template <auto THREADS>
__device__ __forceinline__ void jl_hist_flush_add(const unsigned *s_hist, unsigned words, unsigned long long *dst) {
  __syncthreads();
  for (unsigned i = threadIdx.x; i < words; i += THREADS)
    if (s_hist[i]) atomicAdd(&dst[i], static_cast<unsigned long long>(s_hist[i]));
}

template <bool RANK>
__global__ __launch_bounds__(kJlThreads) void jl_hist0_kernel(const unsigned *__restrict__ keys, size_t n, size_t group_rows,
                                                              unsigned parts, unsigned k2_shift,
                                                              unsigned k1, unsigned long long *counts_g) {
  extern __shared__ unsigned s_hist[];
  const unsigned group = blockIdx.x / kJlHistWgPerGroup, w = blockIdx.x % kJlHistWgPerGroup;
  const size_t lo = static_cast<size_t>(group) * group_rows;
  size_t hi = lo + group_rows;
  hi = hi < n ? hi : n;
  if (lo >= hi) return;
  for (unsigned i = threadIdx.x; i < k1; i += kJlThreads) s_hist[i] = 0;
  __syncthreads();
  // (jl_stream<kJlThreads, 4>, kept inline: through it the loop steps its index and address differently, 246
  //  instructions for 251)
  for (size_t i = lo + static_cast<size_t>(w) * 4 * kJlThreads + threadIdx.x; i < hi;
       i += static_cast<size_t>(kJlHistWgPerGroup) * 4 * kJlThreads) {  // four independent loads per lane per step
    unsigned k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = i + j * kJlThreads < hi ? keys[i + j * kJlThreads] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j * kJlThreads < hi) atomicAdd(&s_hist[jl_pid_sel<RANK>(k[j], parts) >> k2_shift], 1u);
  }
  jl_hist_flush_add<kJlThreads>(s_hist, k1, counts_g + static_cast<size_t>(group) * k1);
}

// ---- both levels' histograms in ONE read of the keys (parts <= 32768: the counters fit 128 KiB of LDS) --------------
// Workgroup (group g, w) counts the FINAL partition of every row of its share of group g in an LDS histogram of `parts`
// bins and stores it, plainly, as its own row of wgcnt[][]; jl_hist_reduce sums the rows: per (group, level-0 bucket)
// for the level-0 cursors and per partition for level 1.  Replaces jl_hist0 + jl_hist1: the second used to re-read the
// level-0 output (8 bytes per row: 113 us of the 2^26-row build).
constexpr unsigned kJlFusedThreads = 1024;  // kJlGroups x kJlFusedWgPerGroup workgroups (partition.hpp) of these
#ifndef DBHIP_JL_HIST_LOADS
#define DBHIP_JL_HIST_LOADS 4
#endif
constexpr int kJlHistLoads = DBHIP_JL_HIST_LOADS;  // 16-byte key loads in flight per lane of the fused16 histogram

// (Kept whole, as is jl_hist_fused16_kernel: with its zeroing, a stream, the ragged tail or the flush in a function of
//  its own either kernel tests `lo < hi && aligned` or `w == 0` with the opposite branch, or swaps two registers of the
//  store loop.  The two differ in the counter and in the unaligned path: four loads in flight here, one there.)
__global__ __launch_bounds__(kJlFusedThreads) void jl_hist_fused_kernel(const unsigned *__restrict__ keys, size_t n, size_t group_rows,
                                                                        unsigned parts, unsigned *__restrict__ wgcnt) {
  extern __shared__ unsigned s_hist[];
  const unsigned group = blockIdx.x / kJlFusedWgPerGroup, w = blockIdx.x % kJlFusedWgPerGroup;
  for (unsigned i = threadIdx.x; i < parts; i += kJlFusedThreads) s_hist[i] = 0;
  __syncthreads();
  const size_t lo = static_cast<size_t>(group) * group_rows;
  size_t hi = lo + group_rows;
  hi = hi < n ? hi : n;
  if (lo < hi && (reinterpret_cast<uintptr_t>(keys + lo) & 15u) == 0) {
    // 16-byte loads, four in flight per lane (4-byte loads kept 16 KiB per CU in flight: 79 us for 256 MiB of keys)
    const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys + lo);
    const size_t n4 = (hi - lo) / 4;
    for (size_t i = static_cast<size_t>(w) * 4 * kJlFusedThreads + threadIdx.x; i < n4;
         i += static_cast<size_t>(kJlFusedWgPerGroup) * 4 * kJlFusedThreads) {
      u32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = i + j * kJlFusedThreads < n4 ? k4[i + j * kJlFusedThreads] : u32x4{0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j * kJlFusedThreads < n4) {
          atomicAdd(&s_hist[jl_pid(v[j].x, parts)], 1u);
          atomicAdd(&s_hist[jl_pid(v[j].y, parts)], 1u);
          atomicAdd(&s_hist[jl_pid(v[j].z, parts)], 1u);
          atomicAdd(&s_hist[jl_pid(v[j].w, parts)], 1u);
        }
    }
    if (w == 0 && lo + n4 * 4 + threadIdx.x < hi) atomicAdd(&s_hist[jl_pid(keys[lo + n4 * 4 + threadIdx.x], parts)], 1u);
  } else {
    for (size_t i = lo + static_cast<size_t>(w) * 4 * kJlFusedThreads + threadIdx.x; i < hi;
         i += static_cast<size_t>(kJlFusedWgPerGroup) * 4 * kJlFusedThreads) {  // four independent loads per lane per step
      unsigned k[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) k[j] = i + j * kJlFusedThreads < hi ? keys[i + j * kJlFusedThreads] : 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j * kJlFusedThreads < hi) atomicAdd(&s_hist[jl_pid(k[j], parts)], 1u);
    }
  }
  __syncthreads();
  unsigned *mine = wgcnt + static_cast<size_t>(blockIdx.x) * parts;
  for (unsigned i = threadIdx.x; i < parts; i += kJlFusedThreads) mine[i] = s_hist[i];
}

// ---- the same for 32768 < parts <= 65536 (2^27-row shards: what every rank of the 8-GPU join partitions) ----------------
// 65536 32-bit counters do not fit the LDS; 16 bits are enough for a workgroup's share of a partition (2^27 rows / 256
// workgroups / 65536 partitions = 8 rows) unless the input is heavily skewed.  TWO counters per LDS word, fed by
// RETURNING ds_add: from the returned value a lane sees exactly when its increment carried out of the low half (the
// even partition's counter wrapped and the odd one's now holds one too many) or out of bit 31 (the odd one wrapped) and
// settles that in the global accumulators the reduce kernel adds to — correct for any input, and free for every input
// that is not pathological.  The workgroup's row of wgcnt is the LDS image: parts / 2 words.
__global__ __launch_bounds__(kJlFusedThreads) void jl_hist_fused16_kernel(const unsigned *__restrict__ keys, size_t n, size_t group_rows,
                                                                          unsigned parts, unsigned log2_k2, unsigned k1,
                                                                          unsigned *__restrict__ wgcnt,
                                                                          unsigned long long *counts0g,
                                                                          unsigned long long *counts1) {
  extern __shared__ unsigned s_hist[];
  const unsigned group = blockIdx.x / kJlFusedWgPerGroup, w = blockIdx.x % kJlFusedWgPerGroup;
  const unsigned words = parts / 2;
  for (unsigned i = threadIdx.x; i < words; i += kJlFusedThreads) s_hist[i] = 0;
  __syncthreads();
  auto count = [&](unsigned key) {
    const unsigned p = jl_pid(key, parts);
    const unsigned inc = 1u << ((p & 1u) << 4);
    const unsigned old = atomicAdd(&s_hist[p >> 1], inc);
    const bool carry16 = (p & 1u) == 0 && (old & 0xFFFFu) == 0xFFFFu, carry32 = old + inc < old;
    if (carry16 || carry32) {  // (more than 65535 rows of this workgroup's share in one partition)
      const unsigned even = p & ~1u, odd = p | 1u;
      unsigned long long *g0 = counts0g + static_cast<size_t>(group) * k1;
      if (carry16) {
        atomicAdd(&counts1[even], 65536ull);
        atomicAdd(&g0[even >> log2_k2], 65536ull);
        atomicAdd(&counts1[odd], ~0ull);  // minus one: the carry landed in the odd partition's half
        atomicAdd(&g0[odd >> log2_k2], ~0ull);
      }
      if (carry32) {
        atomicAdd(&counts1[odd], 65536ull);
        atomicAdd(&g0[odd >> log2_k2], 65536ull);
      }
    }
  };
  const size_t lo = static_cast<size_t>(group) * group_rows;
  size_t hi = lo + group_rows;
  hi = hi < n ? hi : n;
  if (lo < hi && (reinterpret_cast<uintptr_t>(keys + lo) & 15u) == 0) {
    const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys + lo);
    const size_t n4 = (hi - lo) / 4;
    // (round 4, measured and dropped: the next step's loads in flight while this step's keys are counted, two register
    //  sets as in the group-by — 80.7 -> 99.6 us for the 256 MiB of keys of a 2^26-row side; eight loads per lane in
    //  flight instead of four: partition of one side 572 -> 590 us, two: the same as four)
    for (size_t i = static_cast<size_t>(w) * kJlHistLoads * kJlFusedThreads + threadIdx.x; i < n4;
         i += static_cast<size_t>(kJlFusedWgPerGroup) * kJlHistLoads * kJlFusedThreads) {
      u32x4 v[kJlHistLoads];
#pragma unroll
      for (int j = 0; j < kJlHistLoads; ++j) v[j] = i + j * kJlFusedThreads < n4 ? k4[i + j * kJlFusedThreads] : u32x4{0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < kJlHistLoads; ++j)
        if (i + j * kJlFusedThreads < n4) {
          count(v[j].x);
          count(v[j].y);
          count(v[j].z);
          count(v[j].w);
        }
    }
    if (w == 0 && lo + n4 * 4 + threadIdx.x < hi) count(keys[lo + n4 * 4 + threadIdx.x]);
  } else {
    for (size_t i = lo + static_cast<size_t>(w) * kJlFusedThreads + threadIdx.x; i < hi;
         i += static_cast<size_t>(kJlFusedWgPerGroup) * kJlFusedThreads)
      count(keys[i]);
  }
  __syncthreads();
  unsigned *mine = wgcnt + static_cast<size_t>(blockIdx.x) * words;
  for (unsigned i = threadIdx.x; i < words; i += kJlFusedThreads) mine[i] = s_hist[i];
}

// reduce of the packed rows; ADDS to counts1 / counts0g (zeroed with the metadata, and possibly holding the carries
// the histogram kernel settled): one thread per WORD (two partitions) for the column sums, one wave per (row, bucket)
// for the level-0 counts — the sum of both halves of a bucket's words
// (One kernel with jl_hist_reduce_kernel below but for how a word is read and `+=` against `=`; as one
//  `template <bool kPacked>` body that one kept its text and this one set up `words * 28` and `words * 32` in the
//  other order — as it does when this very body is moved into a function unchanged.  Two kernels stay.)
__global__ __launch_bounds__(256) void jl_hist_reduce16_kernel(const unsigned *__restrict__ wgcnt, unsigned parts, unsigned k1,
                                                               unsigned k2, unsigned long long *counts0g,
                                                               unsigned long long *counts1) {
  constexpr unsigned kRows = kJlGroups * kJlFusedWgPerGroup;
  const unsigned words = parts / 2, col_blocks = (words + 255) / 256;
  if (blockIdx.x < col_blocks) {
    const unsigned wd = blockIdx.x * 256 + threadIdx.x;
    if (wd >= words) return;
    unsigned long long lo = 0, hi = 0;
    for (unsigned r0 = 0; r0 < kRows; r0 += 8) {
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = wgcnt[static_cast<size_t>(r0 + u) * words + wd];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        lo += v[u] & 0xFFFFu;
        hi += v[u] >> 16;
      }
    }
    counts1[2 * wd] += lo;  // (the histogram kernel has finished: no one else touches these words now)
    counts1[2 * wd + 1] += hi;
    return;
  }
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t item = static_cast<size_t>(blockIdx.x - col_blocks) * 4 + wave;  // (row, bucket)
  if (item >= static_cast<size_t>(kRows) * k1) return;
  const unsigned row = static_cast<unsigned>(item / k1), bucket = static_cast<unsigned>(item % k1);
  const unsigned *src = wgcnt + static_cast<size_t>(row) * words + static_cast<size_t>(bucket) * (k2 / 2);
  unsigned mine = 0;
  for (unsigned sub = lane; sub < k2 / 2; sub += kWave) mine += (src[sub] & 0xFFFFu) + (src[sub] >> 16);
  mine = wave_reduce_add(mine);
  if (lane == kWave - 1 && mine)
    atomicAdd(&counts0g[static_cast<size_t>(row / kJlFusedWgPerGroup) * k1 + bucket], static_cast<unsigned long long>(mine));
}

// counts1[p] = rows of partition p (column sums of wgcnt, one thread per partition: the first parts/256 workgroups),
// counts0g[g][b] = rows of group g in level-0 bucket b (one WAVE per (workgroup row, bucket): k2 contiguous counters,
// added to the zeroed counts0g with one atomic per wave: the remaining workgroups)
__global__ __launch_bounds__(256) void jl_hist_reduce_kernel(const unsigned *__restrict__ wgcnt, unsigned parts, unsigned k1,
                                                             unsigned k2, unsigned long long *counts0g,
                                                             unsigned long long *counts1) {
  constexpr unsigned kRows = kJlGroups * kJlFusedWgPerGroup;
  const unsigned col_blocks = (parts + 255) / 256;
  if (blockIdx.x < col_blocks) {
    const unsigned p = blockIdx.x * 256 + threadIdx.x;
    if (p >= parts) return;
    unsigned long long sum = 0;
    for (unsigned r0 = 0; r0 < kRows; r0 += 8) {
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = wgcnt[static_cast<size_t>(r0 + u) * parts + p];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum += v[u];
    }
    counts1[p] = sum;
    return;
  }
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t item = static_cast<size_t>(blockIdx.x - col_blocks) * 4 + wave;  // (row, bucket)
  if (item >= static_cast<size_t>(kRows) * k1) return;
  const unsigned row = static_cast<unsigned>(item / k1), bucket = static_cast<unsigned>(item % k1);
  const unsigned *src = wgcnt + static_cast<size_t>(row) * parts + static_cast<size_t>(bucket) * k2;
  unsigned mine = 0;
  for (unsigned sub = lane; sub < k2; sub += kWave) mine += src[sub];
  mine = wave_reduce_add(mine);
  if (lane == kWave - 1 && mine)
    atomicAdd(&counts0g[static_cast<size_t>(row / kJlFusedWgPerGroup) * k1 + bucket], static_cast<unsigned long long>(mine));
}

// bucket starts, per-group cursors and the tile index of every bucket (for the 1-D grid of level 1).
// One workgroup, thread b owns bucket b (k1 <= 1024).
__global__ __launch_bounds__(1024) void jl_offsets0_kernel(const unsigned long long *__restrict__ counts_g,
                                                           unsigned k1, unsigned tile1, unsigned long long *cursors_g,
                                                           unsigned long long *starts, unsigned long long *tile_starts,
                                                           unsigned long long *totals_out) {
  __shared__ unsigned long long s_tot[1024], s_start[1025], s_tstart[1025];
  __shared__ unsigned long long s_wrow[16], s_wtile[16];
  const unsigned b = threadIdx.x, lane = b & (kWave - 1), wave = b / kWave;
  unsigned long long tot = 0;
  if (b < k1)
    for (unsigned g = 0; g < kJlGroups; ++g) tot += counts_g[static_cast<size_t>(g) * k1 + b];
  s_tot[b] = tot;
  // exclusive prefix over the buckets of rows and of level-1 tiles: wave scans + a 16-entry pass
  const unsigned long long tl = b < k1 ? (tot + tile1 - 1) / tile1 : 0ull;  // tiles of the level-1 scatter (tile1 rows each)
  unsigned long long ir = tot, it = tl;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long pr = __shfl_up(ir, off, kWave), pt = __shfl_up(it, off, kWave);
    if (lane >= static_cast<unsigned>(off)) {
      ir += pr;
      it += pt;
    }
  }
  if (lane == kWave - 1) {
    s_wrow[wave] = ir;
    s_wtile[wave] = it;
  }
  __syncthreads();
  unsigned long long base_r = 0, base_t = 0;
  for (unsigned w = 0; w < wave; ++w) {
    base_r += s_wrow[w];
    base_t += s_wtile[w];
  }
  s_start[b] = base_r + ir - tot;
  s_tstart[b] = base_t + it - tl;
  if (b == 1023) {
    s_start[1024] = base_r + ir;
    s_tstart[1024] = base_t + it;
  }
  __syncthreads();
  if (b < k1) {
    starts[b] = s_start[b];
    tile_starts[b] = s_tstart[b];
    if (totals_out) totals_out[b] = s_tot[b];
    unsigned long long run = s_start[b];
    for (unsigned g = 0; g < kJlGroups; ++g) {
      cursors_g[static_cast<size_t>(g) * k1 + b] = run;
      run += counts_g[static_cast<size_t>(g) * k1 + b];
    }
  }
  if (b == 0) {
    starts[k1] = s_start[k1];
    tile_starts[k1] = s_tstart[k1];
  }
}

// level 1: bucket b's k2 sub-buckets live inside [starts0[b], starts0[b+1]).  One workgroup per bucket.
__global__ __launch_bounds__(kJlThreads) void jl_offsets1_kernel(const unsigned long long *__restrict__ counts1,
                                                                 const unsigned long long *__restrict__ starts0,
                                                                 unsigned k1, unsigned k2, unsigned long long *starts1,
                                                                 unsigned long long *cursors1) {
  __shared__ unsigned s_wsum[kJlThreads / kWave];
  const unsigned b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const unsigned per = (k2 + kJlThreads - 1) / kJlThreads;  // <= 4
  unsigned c[4] = {0, 0, 0, 0}, mine = 0;
#pragma unroll
  for (unsigned u = 0; u < 4; ++u) {
    const unsigned sidx = tid * per + u;
    if (u < per && sidx < k2) c[u] = static_cast<unsigned>(counts1[static_cast<size_t>(b) * k2 + sidx]);
    mine += c[u];
  }
  const unsigned incl = wave_inclusive_scan(mine);
  if (lane == kWave - 1) s_wsum[wave] = incl;
  __syncthreads();
  unsigned long long run = starts0[b] + incl - mine;
  for (unsigned w = 0; w < wave; ++w) run += s_wsum[w];
#pragma unroll
  for (unsigned u = 0; u < 4; ++u) {
    const unsigned sidx = tid * per + u;
    if (u < per && sidx < k2) {
      starts1[static_cast<size_t>(b) * k2 + sidx] = run;
      cursors1[static_cast<size_t>(b) * k2 + sidx] = run;
      run += c[u];
    }
  }
  if (b == k1 - 1 && tid == 0) starts1[static_cast<size_t>(k1) * k2] = starts0[k1];
}

// Scatter of one 4096-row tile into `nb` (<= 1024) buckets, staged through LDS so that the global
// writes are runs: rows are ranked inside their bucket with LDS atomics, the tile is re-ordered by
// bucket in LDS, every bucket's run gets ONE global reservation, and consecutive lanes then write
// consecutive addresses of a run.  LEVEL selects how the bucket is recomputed from the key on the way
// out (0: pid >> arg, 1: pid & arg).  dest[j] == nb marks an invalid (out-of-range) row.
// LDS: cnt[nb] | excl[nb] | base[nb] (u64) | keys[4096] | rids[4096] | 4 wave sums.
constexpr size_t jl_scatter_lds_bytes(unsigned nb, unsigned tile = kJlTile, unsigned threads = kJlThreads) {
  return static_cast<size_t>(nb) * 16 + 2 * static_cast<size_t>(tile) * sizeof(unsigned) + sizeof(unsigned) * (threads / kWave);
}
struct JlNoHook {
  __device__ __forceinline__ void operator()() const {}
};
// before_stores(): called once, right before the tile's global stores are issued (the level-0 kernel waits there for
// the next tile's prefetched keys: see jl_scatter0_kernel)
template <int LEVEL, int THREADS, int KPT, bool RANK = false, bool DIGITS = false, class Hook = JlNoHook>
__device__ __forceinline__ void jl_scatter_tile(const unsigned (&key)[KPT], const unsigned (&rid)[KPT],
                                                const unsigned (&dest)[KPT], unsigned nb, unsigned parts,
                                                unsigned arg, unsigned long long *cursors,
                                                unsigned *__restrict__ out_keys, unsigned *__restrict__ out_rids,
                                                unsigned *s_mem, Hook before_stores = Hook()) {
  unsigned long long *s_base = reinterpret_cast<unsigned long long *>(s_mem);  // 8-byte aligned first
  unsigned *s_cnt = s_mem + 2 * nb;
  unsigned *s_excl = s_cnt + nb;
  unsigned *s_keys = s_excl + nb;
  unsigned *s_rids = s_keys + (THREADS * KPT);
  unsigned *s_wsum = s_rids + (THREADS * KPT);
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  for (unsigned i = tid; i < nb; i += THREADS) s_cnt[i] = 0;
  __syncthreads();
  unsigned rank[KPT];
#pragma unroll
  for (int j = 0; j < KPT; ++j) rank[j] = dest[j] < nb ? atomicAdd(&s_cnt[dest[j]], 1u) : 0u;
  __syncthreads();
  // exclusive scan of the bucket counts (nb <= 1024: up to 4 consecutive buckets per thread)
  const unsigned per = (nb + THREADS - 1) / THREADS;
  unsigned c[4] = {0, 0, 0, 0}, mine = 0;
#pragma unroll
  for (unsigned u = 0; u < 4; ++u) {
    const unsigned b = tid * per + u;
    if (u < per && b < nb) c[u] = s_cnt[b];
    mine += c[u];
  }
  const unsigned incl = wave_inclusive_scan(mine);
  if (lane == kWave - 1) s_wsum[wave] = incl;
  __syncthreads();
  unsigned run = incl - mine;
  for (unsigned w = 0; w < wave; ++w) run += s_wsum[w];
  unsigned total = 0;
#pragma unroll
  for (int w = 0; w < (THREADS / kWave); ++w) total += s_wsum[w];
#pragma unroll
  for (unsigned u = 0; u < 4; ++u) {
    const unsigned b = tid * per + u;
    if (u < per && b < nb) {
      s_excl[b] = run;
      // (one returning global atomic per bucket per tile; replacing them by a precomputed offset in a timing
      //  experiment did not make the kernel faster: the reservations are not what bounds it)
      s_base[b] = c[u] ? atomicAdd(&cursors[b], static_cast<unsigned long long>(c[u])) : 0ull;
      run += c[u];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (dest[j] < nb) {
      const unsigned p = s_excl[dest[j]] + rank[j];
      s_keys[p] = key[j];
      s_rids[p] = rid[j];
    }
  }
  __syncthreads();
  before_stores();
  for (unsigned p = tid; p < total; p += THREADS) {
    const unsigned k = s_keys[p];
    const unsigned pid = jl_pid_sel<RANK>(k, parts);
    const unsigned d = LEVEL == 0 ? pid >> arg : pid & arg;
    const size_t slot = s_base[d] + (p - s_excl[d]);
    if (DIGITS) {  // pairs + the row's level-1 bucket as a 16-bit column of its own (behind `out_rids`): what the level-1
                   // histogram reads instead of the pairs, 2 bytes per row for 8 (jl_hist1d_kernel)
      reinterpret_cast<u32x2 *>(out_keys)[slot] = u32x2{k, s_rids[p]};
      reinterpret_cast<unsigned short *>(out_rids)[slot] = static_cast<unsigned short>(pid & ((1u << arg) - 1u));
    } else if (out_rids) {  // two columns (the rank-level partition: its outputs go into an all-to-all as they are)
      out_keys[slot] = k;
      out_rids[slot] = s_rids[p];
    } else {  // one array of (key, row id) pairs: one 8-byte store per row, a run of r rows is 8r contiguous bytes
      // (plain stores: the runs of neighbouring tiles meet in L2; non-temporal stores here made a partition side of
      //  2^26 rows 778 us instead of 602)
      reinterpret_cast<u32x2 *>(out_keys)[slot] = u32x2{k, s_rids[p]};
    }
  }
  __syncthreads();  // LDS is reused by the next tile
}

// level-0 scatter: (key, row id) pairs bucket-major; row id = index (or row_ids[index] when given)
// THREADS x KPT rows per tile (JlSidePlan); RIDS: row ids come as a column (the received pairs of the multi-GPU join) —
// a template parameter so that the other callers do not carry the prefetched row-id registers
#ifndef DBHIP_JL_SC0_WPE
#define DBHIP_JL_SC0_WPE 6
#endif
template <bool RANK, bool RIDS, int THREADS, int KPT, bool DIGITS = false>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(THREADS == 512 && !RIDS ? DBHIP_JL_SC0_WPE : 1))) void jl_scatter0_kernel(const unsigned *__restrict__ keys,
                                                                 const unsigned *__restrict__ row_ids,
                                                                 unsigned long long first_row, size_t n,
                                                                 unsigned parts, unsigned k2_shift, unsigned k1,
                                                                 unsigned long long *cursors,
                                                                 unsigned *__restrict__ out_keys,
                                                                 unsigned *__restrict__ out_rids) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_mem[];
  const size_t tiles = (n + (THREADS * KPT) - 1) / (THREADS * KPT);
  // XCD-aware tile order (speed only, any order is correct): workgroups are dealt to the 8 XCDs round-robin by
  // blockIdx, so XCD x = blockIdx % 8 takes the tile groups g with g % 8 == x.  A (group, bucket) write frontier is
  // then advanced by ONE XCD, whose L2 merges the partial lines of consecutive runs before they leave for memory
  // (WRITE_SIZE 770 MB for 537 MB stored when every XCD touched every frontier; 338 -> 310 us at 2^26 rows).
  // The same slicing of the level-1 scatter (buckets b % 8 == x per XCD, persistent grid) measured no faster.
  const size_t tpg = jl_group_rows(n, THREADS * KPT) / (THREADS * KPT);
  const unsigned xcd = blockIdx.x % 8u, slot = blockIdx.x / 8u, per_xcd = gridDim.x / 8u;  // host: grid % 8 == 0
  const size_t locals = (kJlGroups / 8) * tpg;
  // tile of the workgroup's `local`-th step, or `tiles` when that step has none (the ragged end of the last group)
  auto tile_of = [&](size_t local, size_t *group) -> size_t {
    *group = (local / tpg) * 8 + xcd;
    const size_t tile = *group * tpg + local % tpg;
    return local < locals && tile < tiles ? tile : tiles;
  };
  auto load_tile = [&](size_t tile, unsigned (&k)[KPT], unsigned (&r)[KPT]) {
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const size_t idx = tile * (THREADS * KPT) + static_cast<size_t>(j) * THREADS + threadIdx.x;
      const bool valid = tile < tiles && idx < n;
      k[j] = valid ? keys[idx] : 0u;
      r[j] = RIDS && valid ? row_ids[idx] : 0u;
    }
  };
  // The next tile's keys are requested before the current tile's LDS work and waited for right before the current
  // tile's stores go out (vmcnt counts a wave's loads and stores in issue order: waiting for loads at the top of the
  // next step would also wait for every store of this one).  They cross the loop in registers moved by a v_mov the
  // compiler cannot see through — a loop-carried register that a load defined is waited for with vmcnt(0) at first use.
  unsigned ckey[KPT], crid[KPT];
  size_t group = 0, tile = tile_of(slot, &group);
  load_tile(tile, ckey, crid);
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    asm volatile("v_mov_b32 %0, %0" : "+v"(ckey[j]));
    if (RIDS) asm volatile("v_mov_b32 %0, %0" : "+v"(crid[j]));
  }
  for (size_t local = slot; local < locals; local += per_xcd) {
    size_t ngroup = 0;
    const size_t ntile = tile_of(local + per_xcd, &ngroup);
    unsigned nkey[KPT], nrid[KPT], mkey[KPT], mrid[KPT];
    load_tile(ntile, nkey, nrid);
    auto wait_next = [&]() {
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        asm volatile("v_mov_b32 %0, %1" : "=v"(mkey[j]) : "v"(nkey[j]));
        if (RIDS) asm volatile("v_mov_b32 %0, %1" : "=v"(mrid[j]) : "v"(nrid[j]));
        else mrid[j] = 0u;
      }
    };
    if (tile < tiles) {  // uniform over the workgroup
      const size_t base = tile * (THREADS * KPT);
      unsigned rid[KPT], dest[KPT];
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const size_t idx = base + static_cast<size_t>(j) * THREADS + threadIdx.x;
        const bool valid = idx < n;
        rid[j] = valid ? (RIDS ? crid[j] : static_cast<unsigned>(first_row + idx)) : 0u;
        dest[j] = valid ? jl_pid_sel<RANK>(ckey[j], parts) >> k2_shift : k1;
      }
      // this tile bumps only its group's cursors
      jl_scatter_tile<0, THREADS, KPT, RANK, DIGITS>(ckey, rid, dest, k1, parts, k2_shift, cursors + group * k1, out_keys, out_rids, s_mem, wait_next);
    } else {
      wait_next();
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      ckey[j] = mkey[j];
      crid[j] = mrid[j];
    }
    tile = ntile;
    group = ngroup;
  }
}

// (bucket, tile-in-bucket) of virtual tile `vt` by binary search over tile_starts[0..k1]
__device__ __forceinline__ bool jl_locate(const unsigned long long *__restrict__ tile_starts, unsigned k1,
                                          unsigned long long vt, unsigned *bucket, unsigned long long *tile) {
  if (vt >= tile_starts[k1]) return false;
  unsigned lo = 0, hi = k1;  // find largest b with tile_starts[b] <= vt
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) / 2;
    if (tile_starts[mid] <= vt) lo = mid; else hi = mid;
  }
  *bucket = lo;
  *tile = vt - tile_starts[lo];
  return true;
}

// level-1 histogram: kJlHist1WgPerBucket workgroups stride over one level-0 bucket (four independent loads per
// lane per step), so a bucket's k2 counters see 16 flushes instead of one per scatter tile
constexpr unsigned kJlHist1WgPerBucket = 16;

__global__ __launch_bounds__(kJlThreads) void jl_hist1_kernel(const u32x2 *__restrict__ rows,
                                                              const unsigned long long *__restrict__ starts0,
                                                              unsigned parts, unsigned k2,
                                                              unsigned long long *counts1) {
  extern __shared__ unsigned s_hist[];
  const unsigned bucket = blockIdx.x / kJlHist1WgPerBucket, w = blockIdx.x % kJlHist1WgPerBucket;
  const size_t lo = starts0[bucket], hi = starts0[bucket + 1];
  if (lo + static_cast<size_t>(w) * 4 * kJlThreads >= hi) return;
  for (unsigned i = threadIdx.x; i < k2; i += kJlThreads) s_hist[i] = 0;
  __syncthreads();
  // the level-0 output is (key, row id) pairs: the histogram reads them whole (8 bytes per row)
  jl_stream<kJlThreads, 4>(rows, lo, hi, w, kJlHist1WgPerBucket,
                           [&](u32x2 row) { atomicAdd(&s_hist[jl_pid(row.x, parts) & (k2 - 1)], 1u); });
  jl_hist_flush_add<kJlThreads>(s_hist, k2, counts1 + static_cast<size_t>(bucket) * k2);
}

// The same histogram from the 16-bit level-1 bucket column the level-0 scatter wrote beside its pairs (jl_scatter_tile
// DIGITS; the 16384-row shape, i.e. 2^28 rows and more): 2 bytes per row instead of 8, and no hash.  Eight digits per
// 16-byte load over the aligned middle of the bucket's range, the ragged ends one digit per lane.
__global__ __launch_bounds__(kJlThreads) void jl_hist1d_kernel(const unsigned short *__restrict__ digits,
                                                               const unsigned long long *__restrict__ starts0, unsigned k2,
                                                               unsigned long long *counts1) {
  extern __shared__ unsigned s_hist[];
  const unsigned bucket = blockIdx.x / kJlHist1WgPerBucket, w = blockIdx.x % kJlHist1WgPerBucket;
  const size_t lo = starts0[bucket], hi = starts0[bucket + 1];
  if (lo >= hi) return;
  for (unsigned i = threadIdx.x; i < k2; i += kJlThreads) s_hist[i] = 0;
  __syncthreads();
  const unsigned mask = k2 - 1;
  // head [lo, a) and tail [b, hi) one digit per lane (first workgroup of the bucket), [a, b) in whole 16-byte vectors
  size_t a = (lo + 7) & ~static_cast<size_t>(7);
  if (a > hi) a = hi;
  size_t b = hi & ~static_cast<size_t>(7);
  if (b < a) b = a;
  if (w == 0) {
    for (size_t i = lo + threadIdx.x; i < a; i += kJlThreads) atomicAdd(&s_hist[digits[i] & mask], 1u);
    for (size_t i = b + threadIdx.x; i < hi; i += kJlThreads) atomicAdd(&s_hist[digits[i] & mask], 1u);
  }
  jl_stream<kJlThreads, 2>(reinterpret_cast<const u32x4 *>(digits), a / 8, b / 8, w, kJlHist1WgPerBucket, [&](u32x4 x) {
    const unsigned word[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      atomicAdd(&s_hist[word[q] & mask], 1u);
      atomicAdd(&s_hist[(word[q] >> 16) & mask], 1u);
    }
  });
  jl_hist_flush_add<kJlThreads>(s_hist, k2, counts1 + static_cast<size_t>(bucket) * k2);
}

// Level-1 scatter: a PERSISTENT grid of the resident workgroups over the "virtual tiles" (every level-0 bucket cut into
// tiles of THREADS x KPT rows; tile_starts[b] = index of bucket b's first tile).  XCD x walks the x-th eighth of the
// virtual tiles, its workgroups interleaved (workgroup j: tiles j, j + per, ...), so the tiles in flight on an XCD
// belong to one or two level-0 buckets, whose k2 write frontiers then meet in ONE L2; a workgroup finds its next tile
// by stepping on from the current one (the bucket changes every few steps: one or two loads), requests its rows
// before the current tile's LDS work and waits for them right before the current tile's stores (the vmcnt rule of
// jl_scatter0_kernel).  Until round 4 this was one tile per workgroup, each starting with a binary search for its
// tile (eight to ten dependent loads) and then its row loads: radix join 2^22 / 2^24 / 2^26 / 2^27 rows 212 / 514 / 1737 /
// 3240 us -> 205 / 496 / 1671 / 3144 (4096-row tiles), 2^30 rows 31.3 -> 26.8 ms (8192-row tiles; 16384-row ones 28.2:
// their 32 prefetched words per lane no longer fit the 128 VGPRs of a 1024-thread workgroup).
template <int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void jl_scatter1p_kernel(const u32x2 *__restrict__ rows,
                                                               const unsigned long long *__restrict__ starts0,
                                                               const unsigned long long *__restrict__ tile_starts,
                                                               unsigned parts, unsigned k1, unsigned k2,
                                                               unsigned long long *cursors1, u32x2 *__restrict__ out_pairs) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_mem[];
  constexpr unsigned kTile = THREADS * KPT;
  const unsigned long long total = tile_starts[k1];
  const unsigned xcd = blockIdx.x % 8u, j = blockIdx.x / 8u, per = gridDim.x / 8u;  // host: gridDim.x % 8 == 0
  const unsigned long long per_xcd = (total + 7) / 8;
  const unsigned long long vend = (xcd + 1) * per_xcd < total ? (xcd + 1) * per_xcd : total;
  unsigned long long vt = xcd * per_xcd + j;
  if (vt >= vend) return;
  unsigned bucket;
  unsigned long long tile;
  if (!jl_locate(tile_starts, k1, vt, &bucket, &tile)) return;
  auto load_tile = [&](unsigned b, unsigned long long t, unsigned (&k)[KPT], unsigned (&r)[KPT]) {
    const size_t lo = starts0[b] + t * kTile, hi = starts0[b + 1];
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const size_t idx = lo + static_cast<size_t>(q) * THREADS + threadIdx.x;
      const u32x2 row = idx < hi ? rows[idx] : u32x2{0u, 0u};  // (idx < lo + kTile by construction)
      k[q] = row.x;
      r[q] = row.y;
    }
  };
  unsigned ckey[KPT], crid[KPT];
  load_tile(bucket, tile, ckey, crid);
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    asm volatile("v_mov_b32 %0, %0" : "+v"(ckey[q]));
    asm volatile("v_mov_b32 %0, %0" : "+v"(crid[q]));
  }
  while (true) {
    // the next tile of this workgroup: step on from the current bucket
    const unsigned long long nvt = vt + per;
    const bool more = nvt < vend;
    unsigned nbucket = bucket;
    if (more)
      while (nbucket + 1 < k1 && nvt >= tile_starts[nbucket + 1]) ++nbucket;
    const unsigned long long ntile = more ? nvt - tile_starts[nbucket] : 0ull;
    unsigned nkey[KPT], nrid[KPT], mkey[KPT], mrid[KPT];
    if (more) {
      load_tile(nbucket, ntile, nkey, nrid);
    } else {
#pragma unroll
      for (int q = 0; q < KPT; ++q) nkey[q] = nrid[q] = 0u;
    }
    auto wait_next = [&]() {
#pragma unroll
      for (int q = 0; q < KPT; ++q) {
        asm volatile("v_mov_b32 %0, %1" : "=v"(mkey[q]) : "v"(nkey[q]));
        asm volatile("v_mov_b32 %0, %1" : "=v"(mrid[q]) : "v"(nrid[q]));
      }
    };
    {
      const size_t lo = starts0[bucket] + tile * kTile, hi = starts0[bucket + 1];
      unsigned dest[KPT];
#pragma unroll
      for (int q = 0; q < KPT; ++q) {
        const size_t idx = lo + static_cast<size_t>(q) * THREADS + threadIdx.x;
        dest[q] = idx < hi ? jl_pid(ckey[q], parts) & (k2 - 1) : k2;
      }
      jl_scatter_tile<1, THREADS, KPT, false>(ckey, crid, dest, k2, parts, k2 - 1, cursors1 + static_cast<size_t>(bucket) * k2,
                                              reinterpret_cast<unsigned *>(out_pairs), nullptr, s_mem, wait_next);
    }
    if (!more) break;
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      ckey[q] = mkey[q];
      crid[q] = mrid[q];
    }
    vt = nvt;
    bucket = nbucket;
    tile = ntile;
  }
}

// grid of the level-0 scatter: a multiple of 8 (one slice of workgroups per XCD)
inline unsigned jl_scatter0_grid(size_t tiles, size_t cap) {
  static const int forced = [] { const char *e = getenv("DBHIP_JL_SC0_WGS"); return e ? atoi(e) : 0; }();  // experiment knob: workgroups per CU
  if (forced >= 1 && forced <= 32) cap = static_cast<size_t>(forced) * 256;  // (knob: per CU of a 256-CU chip)
  size_t g = tiles < cap ? tiles : cap;
  g = (g + 7) / 8 * 8;
  return static_cast<unsigned>(g ? g : 8);
}

template <bool RANK, bool RIDS, int THREADS, int KPT, bool DIGITS>
hipError_t jl_launch_scatter0_shape(const DeviceInfo &dev, hipStream_t s, const unsigned *keys, const unsigned *row_ids,
                                    unsigned long long first_row, size_t n, unsigned parts, unsigned k2_shift, unsigned k1,
                                    unsigned long long *cursors, unsigned *out_keys, unsigned *out_rids) {
  constexpr unsigned kTile = THREADS * KPT;
  const size_t lds = jl_scatter_lds_bytes(k1, kTile, THREADS);
  auto kernel = jl_scatter0_kernel<RANK, RIDS, THREADS, KPT, DIGITS>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return e;
  }
  const size_t tiles = (n + kTile - 1) / kTile;
  // persistent grid of the workgroups that are resident (round 4: the 4096-row shape ran with eight per CU where its
  // registers allowed two; held to 80 VGPRs — amdgpu_waves_per_eu(6) — three are, and a grid of exactly those measured
  // 1.5-2 % of the radix join at 2^26 rows: 1759-1777 -> 1726-1740 us on the same box)
  const size_t per_cu = jl_resident_per_cu(reinterpret_cast<const void *>(kernel), THREADS, lds);
  hipLaunchKernelGGL(kernel, dim3(jl_scatter0_grid(tiles, static_cast<size_t>(dev.cus) * per_cu)), dim3(THREADS), lds, s, keys,
                     row_ids, first_row, n, parts, k2_shift, k1, cursors, out_keys, out_rids);
  return hipSuccess;
}
// the level-0 scatter in tile shape `shape`; `a`: the arguments of jl_launch_scatter0_shape.  RIDS: row ids come as a
// column; DIGITS: pairs into out_keys AND every row's level-1 bucket as a 16-bit column behind out_rids
template <bool RANK, bool RIDS, bool DIGITS, class... Args>
hipError_t jl_launch_scatter0(int shape, Args... a) {
  return shape == 0   ? jl_launch_scatter0_shape<RANK, RIDS, 512, 8, DIGITS>(a...)
         : shape == 1 ? jl_launch_scatter0_shape<RANK, RIDS, 1024, 8, DIGITS>(a...)
                      : jl_launch_scatter0_shape<RANK, RIDS, 1024, 16, DIGITS>(a...);
}

template <int THREADS, int KPT>
hipError_t jl_launch_scatter1_shape(hipStream_t s, size_t n, const u32x2 *rows, const unsigned long long *starts0,
                                    const unsigned long long *tstarts0, unsigned parts, unsigned k1, unsigned k2,
                                    unsigned long long *cursors1, u32x2 *out, const DeviceInfo &dev) {
  constexpr unsigned kTile = THREADS * KPT;
  const size_t lds = jl_scatter_lds_bytes(k2, kTile, THREADS);
  auto kernel = jl_scatter1p_kernel<THREADS, KPT>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return e;
  }
  const size_t blocks = jl_resident_per_cu(reinterpret_cast<const void *>(kernel), THREADS, lds);
  const size_t vtiles = ((n + kTile - 1) / kTile + k1 + 7) / 8 * 8;  // every bucket's last tile may be ragged
  size_t grid = static_cast<size_t>(dev.cus) * blocks / 8 * 8;       // the resident workgroups, a whole number per XCD
  if (grid < 8) grid = 8;
  if (grid > vtiles) grid = vtiles;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(grid)), dim3(THREADS), lds, s, rows, starts0, tstarts0, parts, k1, k2,
                     cursors1, out);
  return hipSuccess;
}
inline hipError_t jl_launch_scatter1(int shape, hipStream_t s, size_t n, const u32x2 *rows, const unsigned long long *starts0,
                                     const unsigned long long *tstarts0, unsigned parts, unsigned k1, unsigned k2,
                                     unsigned long long *cursors1, u32x2 *out, const DeviceInfo &dev) {
  return shape == 0 ? jl_launch_scatter1_shape<512, 8>(s, n, rows, starts0, tstarts0, parts, k1, k2, cursors1, out, dev)
                    : jl_launch_scatter1_shape<1024, 8>(s, n, rows, starts0, tstarts0, parts, k1, k2, cursors1, out, dev);
}

}  // namespace

// The one or two scatter levels shared by all joins (partition.hpp): launches what jl_side_plan(n, g) decides.
int jl_partition_side(const unsigned *keys, const unsigned *row_ids, size_t n, const JlGeometry &g, u32x2 *rows_a,
                      u32x2 *rows_b, unsigned long long *meta, hipStream_t s, const DeviceInfo &dev,
                      const unsigned **out_pairs, const unsigned long long **out_starts) {
  const unsigned parts = g.parts, k1 = g.k1, k2 = g.k2;
  const JlMeta m = jl_meta(g);
  unsigned long long *counts0 = meta + m.counts0, *cursors0 = meta + m.cursors0, *starts0 = meta + m.starts0;
  unsigned long long *tstarts0 = meta + m.tile_starts0, *counts1 = meta + m.counts1, *starts1 = meta + m.starts1;
  unsigned long long *cursors1 = meta + m.cursors1;

  const hipError_t e = fill_async(meta, 0, m.bytes(), s);
  if (e != hipSuccess) return static_cast<int>(e);
  const JlSidePlan plan = jl_side_plan(n, g);
  // scratch of the fused histograms (wgcnt): the level-1 output region, written only later by the level-1 scatter
  unsigned *fused_scratch = reinterpret_cast<unsigned *>(rows_b);

  // both levels write (key, row id) as ONE 8-byte element: a run of r rows is 8r contiguous bytes instead of two
  // runs of 4r (the scatters are bound by partially written lines: level 1 went 330 -> 254 us at 2^26 rows when it
  // switched, level 0 followed once the level-1 histogram read pairs instead of a keys-only column)
  const unsigned k2_shift = g.log2_k2;
  const size_t group_rows = jl_group_rows(n, jl_shape_rows(plan.t0));
  if (plan.hist == kJlHistFused16 || plan.hist == kJlHistFused) {
    // a workgroup per row of wgcnt, `words` words each; the reduce: a thread per word + a wave per (row, bucket)
    const bool packed = plan.hist == kJlHistFused16;
    const unsigned words = packed ? parts / 2 : parts;
    const size_t lds = static_cast<size_t>(words) * sizeof(unsigned);
    const dim3 grid(kJlGroups * kJlFusedWgPerGroup), threads(kJlFusedThreads);
    const hipError_t ea = hipFuncSetAttribute(packed ? reinterpret_cast<const void *>(jl_hist_fused16_kernel)
                                                     : reinterpret_cast<const void *>(jl_hist_fused_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (ea != hipSuccess) return static_cast<int>(ea);
    if (packed)
      hipLaunchKernelGGL(jl_hist_fused16_kernel, grid, threads, lds, s, keys, n, group_rows, parts, g.log2_k2, k1, fused_scratch,
                         counts0, counts1);
    else
      hipLaunchKernelGGL(jl_hist_fused_kernel, grid, threads, lds, s, keys, n, group_rows, parts, fused_scratch);
    const unsigned red_grid = (words + 255) / 256 + (kJlGroups * kJlFusedWgPerGroup * k1 + 3) / 4;
    hipLaunchKernelGGL(packed ? jl_hist_reduce16_kernel : jl_hist_reduce_kernel, dim3(red_grid), dim3(256), 0, s, fused_scratch,
                       parts, k1, k2, counts0, counts1);
  } else {
    hipLaunchKernelGGL(jl_hist0_kernel<false>, dim3(kJlGroups * kJlHistWgPerGroup), dim3(kJlThreads),
                       k1 * sizeof(unsigned), s, keys, n, group_rows, parts, k2_shift, k1, counts0);
  }
  hipLaunchKernelGGL(jl_offsets0_kernel, dim3(1), dim3(1024), 0, s, counts0, k1, jl_shape_rows(plan.t1), cursors0, starts0,
                     tstarts0, static_cast<unsigned long long *>(nullptr));
  {
    const bool digits = plan.hist == kJlHistDigits;
    unsigned *pairs = reinterpret_cast<unsigned *>(rows_a), *column = digits ? reinterpret_cast<unsigned *>(rows_b) : nullptr;
    hipError_t es;
    if (digits)
      es = row_ids ? jl_launch_scatter0<false, true, true>(plan.t0, dev, s, keys, row_ids, 0ull, n, parts, k2_shift, k1, cursors0, pairs, column)
                   : jl_launch_scatter0<false, false, true>(plan.t0, dev, s, keys, row_ids, 0ull, n, parts, k2_shift, k1, cursors0, pairs, column);
    else
      es = row_ids ? jl_launch_scatter0<false, true, false>(plan.t0, dev, s, keys, row_ids, 0ull, n, parts, k2_shift, k1, cursors0, pairs, column)
                   : jl_launch_scatter0<false, false, false>(plan.t0, dev, s, keys, row_ids, 0ull, n, parts, k2_shift, k1, cursors0, pairs, column);
    if (es != hipSuccess) return static_cast<int>(es);
  }
  *out_pairs = reinterpret_cast<const unsigned *>(rows_a);
  *out_starts = starts0;
  if (k2 > 1) {
    if (plan.hist == kJlHistDigits)
      hipLaunchKernelGGL(jl_hist1d_kernel, dim3(k1 * kJlHist1WgPerBucket), dim3(kJlThreads), k2 * sizeof(unsigned), s,
                         reinterpret_cast<const unsigned short *>(rows_b), starts0, k2, counts1);
    else if (plan.hist == kJlHistPlain)
      hipLaunchKernelGGL(jl_hist1_kernel, dim3(k1 * kJlHist1WgPerBucket), dim3(kJlThreads), k2 * sizeof(unsigned), s,
                         rows_a, starts0, parts, k2, counts1);
    hipLaunchKernelGGL(jl_offsets1_kernel, dim3(k1), dim3(kJlThreads), 0, s, counts1, starts0, k1, k2, starts1,
                       cursors1);
    // (one tile per workgroup; a persistent grid with the next tile's rows prefetched — what helps the level-0
    //  scatter — measured the same here: a workgroup that ends after its stores never waits for them.  Round 3: a
    //  precomputed {bucket, tile} map in place of the workgroup's binary search over tile_starts — eight dependent
    //  loads in front of its row loads — measured the same as well (partition of 2^26 rows 610 vs 615 us), and so did
    //  the tile shapes 512x16 / 512x4 / 1024x4 once more (723 / 661 / 699 us against 610).)
    const hipError_t e1 = jl_launch_scatter1(plan.t1, s, n, rows_a, starts0, tstarts0, parts, k1, k2, cursors1, rows_b, dev);
    if (e1 != hipSuccess) return static_cast<int>(e1);
    *out_pairs = reinterpret_cast<const unsigned *>(rows_b);
    *out_starts = starts1;
  }
  return launch_status();
}

// how many of `keys` do NOT belong to bucket `rank` of `parts` under the rank hash (validator of the exchange's routing)
__global__ __launch_bounds__(kJlThreads) void jl_route_check_kernel(const unsigned *__restrict__ keys, size_t n,
                                                                    unsigned parts, unsigned rank,
                                                                    unsigned long long *result) {
  __shared__ unsigned s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const size_t stride = static_cast<size_t>(gridDim.x) * kJlThreads;
  unsigned bad = 0;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kJlThreads + threadIdx.x; i < n; i += stride)
    bad += jl_rank_of(keys[i], parts) != rank;
  bad = wave_reduce_add(bad);
  if ((threadIdx.x & (kWave - 1)) == kWave - 1 && bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0 && s_bad) atomicAdd(result, static_cast<unsigned long long>(s_bad));
}

int jl_route_check(const unsigned *keys, size_t n, unsigned parts, unsigned rank, unsigned long long *result,
                   hipStream_t s, const DeviceInfo &dev) {
  const hipError_t e = fill_async(result, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return static_cast<int>(e);
  if (n == 0) return DBHIP_OK;
  hipLaunchKernelGGL(jl_route_check_kernel, dim3(jl_grid(n, dev, 8)), dim3(kJlThreads), 0, s, keys, n, parts, rank, result);
  return launch_status();
}

// ---- stand-alone level-0 partition (multi-GPU join: bucket = destination rank) ------------------------
// 2^27 rows into 8 buckets: histogram 158 us + scatter 566 us (into 2 buckets: 285 + 700 us — the LDS atomics of a
// wave land on very few addresses).  Counting and ranking by ballot in wave-uniform registers instead (16 unrolled
// bucket tests per key) was measured at 324 + 794 us and dropped.
size_t jl_partition_workspace_bytes(unsigned parts) {
  return align_up(kWsHeader + jl_meta(parts, 0).bytes(), kWsAlign);  // header | meta of level 0 alone
}

int jl_partition(const unsigned *keys, size_t n, unsigned long long first_row, unsigned parts, unsigned *out_keys,
                 unsigned *out_rids, unsigned long long *out_counts, void *workspace, hipStream_t s,
                 const DeviceInfo &dev) {
  char *base = static_cast<char *>(workspace);
  unsigned long long *meta = reinterpret_cast<unsigned long long *>(base + kWsHeader);
  const JlMeta m = jl_meta(parts, 0);
  unsigned long long *counts0 = meta + m.counts0, *cursors0 = meta + m.cursors0, *starts0 = meta + m.starts0;
  unsigned long long *tstarts0 = meta + m.tile_starts0;
  hipError_t e = fill_async(base, 0, jl_partition_workspace_bytes(parts), s);
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(jl_hist0_kernel<true>, dim3(kJlGroups * kJlHistWgPerGroup), dim3(kJlThreads),
                     parts * sizeof(unsigned), s, keys, n, jl_group_rows(n, kJlTile), parts, 0u, parts, counts0);
  hipLaunchKernelGGL(jl_offsets0_kernel, dim3(1), dim3(1024), 0, s, counts0, parts, static_cast<unsigned>(kJlTile), cursors0,
                     starts0, tstarts0, out_counts);
  if (n) {
    // (the rank-level partition numbers its rows itself and writes two columns: its outputs go into an all-to-all as they are)
    e = jl_launch_scatter0<true, false, false>(0, dev, s, keys, static_cast<const unsigned *>(nullptr), first_row, n, parts, 0u,
                                               parts, cursors0, out_keys, out_rids);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return launch_status();
}

}  // namespace dbhip