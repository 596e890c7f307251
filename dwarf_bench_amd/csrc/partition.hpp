// partition.hpp — the radix hash partitioner (partition.hip) as its users see it: the joins (join_lds.hip), the hash
// group-by (groupby_hash.hip) and the multi-GPU exchange (pjoin.hip).  The key-to-partition hashes, the geometry
// (how many partitions, split over how many scatter levels), the layout of the `meta` array the kernels keep their
// counts, cursors and offsets in, and the plan of one side (which histogram, which tile shapes) are each written
// down ONCE, here; everything is a pure function of row counts, so callers agree without reading anything back
// from the device.  The host functions are inline: a program without device code can include this header and ask
// (tests/cpp/join_layout_check.cpp).
#pragma once
#include <stdlib.h>

#include "dbhip_common.hpp"

namespace dbhip {

constexpr unsigned kEmptyKey = 0xFFFFFFFFu;
#ifndef DBHIP_JL_THREADS
#define DBHIP_JL_THREADS 512
#endif
constexpr int kJlThreads = DBHIP_JL_THREADS;  // scatter / histogram / probe workgroups

__device__ __forceinline__ unsigned jl_pid(unsigned key, unsigned parts) {
  return static_cast<unsigned>((static_cast<unsigned long long>(fmix32(key)) * parts) >> 32);
}
// Destination RANK of the multi-GPU partitioner: a second, independent hash.  It must not be the high bits of
// fmix32(key) again: a rank only receives keys of one rank bucket, and its local build (jl_pid above) would then
// find all of them in 1/P of its partitions — P times overfull sub-tables (at P = 8 more keys than slots: the spill path).
__device__ __forceinline__ unsigned jl_rank_of(unsigned key, unsigned parts) {
  return static_cast<unsigned>((static_cast<unsigned long long>(fmix32(key * 0x9E3779B1u + 0x7F4A7C15u)) * parts) >> 32);
}

// ---- geometry ---------------------------------------------------------------------------------------------------------
#ifndef DBHIP_JL_K2_BIAS
#define DBHIP_JL_K2_BIAS 0
#endif
struct JlGeometry {
  unsigned parts, k1, k2, log2_k2;  // parts = k1 * k2: k1 level-0 buckets, each cut into k2 = 2^log2_k2 by level 1
};
inline JlGeometry jl_geometry(size_t n, size_t rows_per_part) {
  JlGeometry L;
  // parts = ceil(n / rows_per_part) rounded up to a multiple of the level-1 fan-out k2 (a power of two: level 1 takes
  // the low bits of the partition id, level 0 the rest — any number k1 <= 1024 of buckets; the partition id itself is a
  // multiply-shift of the hash and takes any range).  Until late in round 3 parts was the next POWER of two: one row
  // more than 2^26 meant 65536 half-empty partitions — build 1245 us against 1029, twice the table.
  size_t want = (n + rows_per_part - 1) / rows_per_part;
  if (want == 0) want = 1;
  if (want > (static_cast<size_t>(1) << 20)) want = static_cast<size_t>(1) << 20;  // 2^20 partitions at most
  unsigned lg = 0;
  while ((static_cast<size_t>(1) << lg) < want) ++lg;
  if (want <= 1024) {  // one scatter level handles up to 1024 buckets
    L.log2_k2 = 0;
  } else {
    // split of the partition bits between the two scatter levels, by floor(log2(parts)): between two powers of two
    // level 0 takes the extra buckets (37504 partitions as 293 x 128: one side of 2^26 rows 615 us; as 147 x 256: 639)
    const unsigned lgs = (static_cast<size_t>(1) << lg) != want ? lg - 1 : lg;
    L.log2_k2 = (lgs + DBHIP_JL_K2_BIAS) / 2;
  }
  L.k2 = 1u << L.log2_k2;
  L.k1 = static_cast<unsigned>((want + L.k2 - 1) / L.k2);
  while (L.k1 > 1024) {  // level 0 (one workgroup of 1024 threads owns the bucket offsets) takes at most 1024 buckets
    ++L.log2_k2;
    L.k2 <<= 1;
    L.k1 = static_cast<unsigned>((want + L.k2 - 1) / L.k2);
  }
  L.parts = L.k1 * L.k2;
  return L;
}

// ---- the meta array ---------------------------------------------------------------------------------------------------
// The column's 4096-row tiles are cut into kJlGroups contiguous groups; every group owns a private slice
// of every bucket (its rows' share), so the scatter's reservations on one cursor come from 1/64 of
// the tiles: 16384 tiles bumping the SAME 128 cursors serialise on the memory-side atomic unit
// (measured: 544 us for a 768 MiB scatter).
constexpr unsigned kJlGroups = 64;
// 8-byte words of a side's `meta`, which the partitioner clears and fills:
//   counts0[G][k1] | cursors0[G][k1] | starts0[k1 + 1] | tile_starts0[k1 + 1] | counts1[parts] | starts1[parts + 1] | cursors1[parts]
// (G = kJlGroups).  parts == 0: level 0 alone, the stand-alone partitioner's array (jl_partition: k1 = its buckets).
struct JlMeta {
  size_t counts0, cursors0, starts0, tile_starts0, counts1, starts1, cursors1, words;
  size_t bytes() const { return words * sizeof(unsigned long long); }
};
inline JlMeta jl_meta(unsigned k1, unsigned parts) {
  JlMeta m;
  m.counts0 = 0;
  m.cursors0 = m.counts0 + static_cast<size_t>(kJlGroups) * k1;
  m.starts0 = m.cursors0 + static_cast<size_t>(kJlGroups) * k1;
  m.tile_starts0 = m.starts0 + k1 + 1;
  m.counts1 = m.tile_starts0 + k1 + 1;
  m.starts1 = m.counts1 + parts;
  m.cursors1 = m.starts1 + (parts ? parts + 1 : 0);
  m.words = m.cursors1 + parts;
  return m;
}
inline JlMeta jl_meta(const JlGeometry &g) { return jl_meta(g.k1, g.parts); }
// the offsets of the partitions a side was cut into (parts + 1 words): level 1's when there are two levels
inline size_t jl_meta_starts(const JlGeometry &g) { return g.k2 > 1 ? jl_meta(g).starts1 : jl_meta(g).starts0; }

// ---- the plan of one side ---------------------------------------------------------------------------------------------
// both levels' histograms in ONE read of the keys: kJlGroups x kJlFusedWgPerGroup workgroups, each with a row of
// `parts` counters (32-bit up to kJlFusedMaxParts partitions, two 16-bit ones per word up to kJlFused16MaxParts) in a
// scratch that lives in the level-1 output region until the level-1 scatter writes it (partition.hip)
constexpr unsigned kJlFusedWgPerGroup = 4;   // 64 groups x 4 = 256 workgroups of 1024 threads: one per CU
#ifndef DBHIP_JL_FUSED_MAX_PARTS
#define DBHIP_JL_FUSED_MAX_PARTS 32768
#endif
constexpr unsigned kJlFusedMaxParts = DBHIP_JL_FUSED_MAX_PARTS;  // 0 disables the fused histogram (A/B timing)
// two 16-bit counters per LDS word (jl_hist_fused16_kernel): as many partitions as the CU's 160 KiB hold — 2^27 rows
// and a quarter more (a rank of the 8-GPU join receives 2^27 rows +- a few thousand: 65537+ partitions)
constexpr unsigned kJlFused16MaxParts = 80 * 1024;

// Tile shapes of the two scatter levels.
// 0: 512 threads x 8 rows = 4096-row tiles (36 KiB + 16 B per bucket of LDS) — the shape every size up to 2^27 rows was
//    tuned on;  1: 1024 x 8 = 8192 rows;  2 (level 0 only): 1024 x 16 = 16384 rows (128 KiB of LDS: one workgroup per CU).
// A tile of T rows into nb buckets writes runs of T / nb rows and takes one returning global atomic per bucket: with the
// 586 x 1024 buckets of a 2^30-row side a 4096-row tile writes 56- and 32-byte runs and one atomic per 7 / 4 rows (level 0
// at 2.8 TB/s, level 1 at 2.6, against 4.0 / 3.9 at 2^26 rows with 293 x 128 buckets).  DBHIP_JL_T0 / DBHIP_JL_T1 force a
// shape (experiments; T1 = 2 reads as 1).
inline unsigned jl_shape_rows(int id) { return id == 0 ? 4096u : id == 1 ? 8192u : 16384u; }
inline int jl_env_shape(const char *name) {
  const char *e = getenv(name);
  return e && e[0] >= '0' && e[0] <= '2' && !e[1] ? e[0] - '0' : -1;
}

// how the rows of a partition are counted before they are scattered
enum JlHist {
  kJlHistOneLevel,  // k2 == 1: jl_hist0 alone
  kJlHistPlain,     // jl_hist0, then jl_hist1 over the level-0 output (8 bytes per row)
  kJlHistFused,     // jl_hist_fused + jl_hist_reduce
  kJlHistFused16,   // jl_hist_fused16 + jl_hist_reduce16
  kJlHistDigits,    // jl_hist0, then jl_hist1d over the 16-bit level-1 bucket column level 0 writes beside its pairs
};
struct JlSidePlan {
  JlHist hist;
  int t0, t1;  // tile shapes of the level-0 and level-1 scatter
};
// What jl_partition_side does with a column of n_side rows and a geometry that may come from ANOTHER column (the radix
// join partitions the probe side by the build side's geometry).
inline JlSidePlan jl_side_plan(size_t n_side, const JlGeometry &g) {
  static const int f0 = jl_env_shape("DBHIP_JL_T0"), f1 = jl_env_shape("DBHIP_JL_T1");
  static const bool digits_on = [] { const char *v = getenv("DBHIP_JL_DIGITS"); return !(v && v[0] == '0'); }();
  JlSidePlan p{kJlHistOneLevel, 0, 0};
  // Measured (radix join, us, t0/t1; same box per size).  Level 1 one tile per workgroup, before it became persistent:
  // 2^26 rows (293 x 128 buckets) 0/0 1838, 1/1 1862, 2/2 2039; 2^27 (293 x 256) 0/0 3406, 1/1 3502, 2/2 3805; 2^28 (586 x 256)
  // 0/0 7776, 1/0 7521, 2/0 7261, 2/1 7425, 2/2 8089; 2^29 (586 x 512) 0/0 16214, 2/0 15225, 1/1 15196, 2/1 14567, 2/2 15836;
  // 2^30 (586 x 1024) 0/0 35256, 2/0 33994, 0/2 33265, 1/2 32852, 2/2 32558.  Persistent level 1: 2^26 x/0 1671, x/1 1703;
  // 2^27 x/0 3144, x/1 3157; 2^28 2/0 6829, 2/1 6769, 0/1 7181, 1/1 7007; 2^30 2/0 29565, 2/1 26830, 1/1 27381, 0/1 27871.
  if (g.k1 >= 512) p.t0 = 2;
  if (g.k2 >= 512) p.t1 = 1;
  if (f0 >= 0) p.t0 = f0;
  if (f1 >= 0) p.t1 = f1 > 1 ? 1 : f1;
  if (g.k2 == 1) return p;
  // scratch of the fused histograms: 256 rows of `parts` counters, in the level-1 output region while it is still unused
  // (it holds 8 n_side bytes; 1 KiB per partition is enough whenever a partition averages >= 128 rows)
  const bool scratch = n_side * 8 >= static_cast<size_t>(kJlGroups) * kJlFusedWgPerGroup * g.parts * sizeof(unsigned);
  // (8192..32768 partitions = 2^24..2^26 rows: below it the two plain histograms are as fast, 2^22 rows: 77 vs 80 us)
  if (g.parts >= 8192 && g.parts <= kJlFusedMaxParts && scratch) {
    p.hist = kJlHistFused;
  } else if (kJlFusedMaxParts != 0 && g.parts > kJlFusedMaxParts && g.parts <= kJlFused16MaxParts && scratch) {
    // 32768 < parts <= 81920 (2^27-row shards and a quarter more): two 16-bit counters per LDS word
    p.hist = kJlHistFused16;
  } else if (digits_on && g.k2 <= 65536 && g.parts > kJlFused16MaxParts) {
    // A level-1 histogram of its own (more partitions than the fused ones count: sides of more than 1.47e8 rows): level 0
    // writes every row's level-1 bucket as a 16-bit column into the level-1 output region — unused until the level-1
    // scatter writes it, like the fused histograms' scratch — and the histogram reads those 2 bytes per row instead of
    // the 8-byte pairs: 2^30 x 2^30 26.7-26.8 -> 25.5-25.6 ms, same box (DBHIP_JL_DIGITS=0: the pairs, for A/B runs).
    // Not below 8192 partitions, where the plain histograms run as well: those sides are a few hundred us as they are.
    p.hist = kJlHistDigits;
  } else {
    p.hist = kJlHistPlain;
  }
  return p;
}

// ---- launch helpers shared by the partitioner and the joins -------------------------------------------------------
inline unsigned jl_grid(size_t items, const DeviceInfo &dev, int per_cu) {
  const size_t want = (items + kJlThreads - 1) / kJlThreads;
  const size_t cap = static_cast<size_t>(dev.cus) * per_cu;
  return static_cast<unsigned>(want < cap ? (want ? want : 1) : cap);
}
// Resident workgroups per CU of a persistent kernel with `lds` bytes of dynamic LDS, as the runtime computes it from the
// kernel's REGISTERS as well as its LDS (round 4: the build kernels were launched with four 512-thread workgroups per CU
// — what their 24 KiB of LDS allow — while their 73-79 VGPRs allow six waves per SIMD, i.e. three: a quarter of the
// statically dealt partitions belonged to workgroups that only started when the first ones had finished).  Asked once per
// (kernel, lds) and host thread, not on every launch.  `env`: experiment knob (workgroups per CU, 1..32) that replaces
// the answer; `fallback`: the answer when the runtime has none.
inline unsigned jl_resident_per_cu(const void *kernel, int threads, size_t lds, const char *env = nullptr,
                                   unsigned fallback = 1u) {
  struct Known {
    const void *kernel;
    size_t lds;
    unsigned blocks;
  };
  constexpr unsigned kKnown = 16;  // (a partition step and a build alternate between three or four kernels)
  thread_local Known known[kKnown] = {};
  thread_local unsigned next = 0;
  for (const Known &k : known)
    if (k.kernel == kernel && k.lds == lds) return k.blocks;
  const char *e = env ? getenv(env) : nullptr;
  int blocks = e ? atoi(e) : 0;
  if (blocks < 1 || blocks > 32) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, threads, lds) != hipSuccess || blocks < 1) {
      (void)hipGetLastError();
      blocks = static_cast<int>(fallback);
    }
  }
  known[next++ % kKnown] = Known{kernel, lds, static_cast<unsigned>(blocks)};
  return static_cast<unsigned>(blocks);
}

// ---- partition.hip ----------------------------------------------------------------------------------------------------
// The partition step of every join, also the group-by's: the (key, row id) pairs of a column of n rows hash-partitioned
// into the g.parts partitions of geometry g; level-0 output in rows_a, level-1 output (g.k2 > 1) in rows_b, offsets in
// `meta` (jl_meta(g).bytes()).  *out_pairs: the partition-major pairs, *out_starts: parts + 1 offsets into them
// (meta + jl_meta_starts(g)).  row_ids == nullptr: the row index.  Any key, 0xFFFFFFFF included, is carried like any other.
int jl_partition_side(const unsigned *keys, const unsigned *row_ids, size_t n, const JlGeometry &g, u32x2 *rows_a,
                      u32x2 *rows_b, unsigned long long *meta, hipStream_t s, const DeviceInfo &dev,
                      const unsigned **out_pairs, const unsigned long long **out_starts);
size_t jl_partition_workspace_bytes(unsigned parts);
int jl_partition(const unsigned *keys, size_t n, unsigned long long first_row, unsigned parts, unsigned *out_keys,
                 unsigned *out_rids, unsigned long long *out_counts, void *workspace, hipStream_t s,
                 const DeviceInfo &dev);
int jl_route_check(const unsigned *keys, size_t n, unsigned parts, unsigned rank, unsigned long long *result,
                   hipStream_t s, const DeviceInfo &dev);

}  // namespace dbhip
