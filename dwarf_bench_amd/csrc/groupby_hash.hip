// groupby_hash.hip — GROUP BY key, SUM(val), COUNT(*) over arbitrary 32-bit keys for gfx950.
//
// The reference's GroupBy (groupby/groupby.cpp:58-93) aggregates through an open-addressing table keyed by the group key;
// dbhip_groupby_sum_u32 (groupby.hip) only takes keys < groups.  This file is the general one: one output row per distinct
// key, in no particular order.  Three paths, chosen on the host from the caller's bound max_groups (no device round trip;
// DBHIP_GBH_PATH=lds|part|global pins one, read once):
//
//   a. LDS (max_groups <= kGbhLdsMaxGroups): a resident grid, one 1024-thread workgroup per CU, streams (key, val) with
//      16-byte loads into a private open-addressing table in LDS (kGbhLdsSlots slots of key | sum | count: plain read of the
//      slot, ds_cmpst on an empty one, ds_add for sum and count).  Rows of one key in kGbhCrowd or more lanes of a wave are
//      summed across the wave and added once (a hot key costs no 64-way queue on one LDS word).  At the end every
//      workgroup inserts its occupied slots into the global table: one global insert per (workgroup, group).  A row that
//      finds no LDS slot within kGbhProbe steps goes to the global table directly: slow, correct.
//   b. PARTITION (more groups): the radix join's partition step (partition.hip jl_partition_side, geometry jl_geometry(n)) hash-partitions
//      the (key, val) pairs — the vals column rides where the join passes row ids — into ~2048-row partitions; one
//      workgroup per partition aggregates it in a kGbhSubSlots-slot LDS sub-table and writes its groups straight to the
//      outputs at an offset taken from a ticket.  A partition of more than kGbhGiantRows rows (a hot key) is listed instead
//      and cut into slices of kGbhGiantRows rows that all workgroups of a second launch aggregate, each slice flushing into
//      the global table.  Keys that find no sub-table slot (a partition with more distinct keys than slots: keys built
//      against the hash) go to the global table too.
//   c. GLOBAL: open addressing in HBM over 2 * max_groups slots (at least 64) of key | sum | count, reset by
//      the call: load the slot's key, CAS only an empty one, memory-side atomic adds for sum and count (two 32-bit adds:
//      a (sum, count) pair added as one 64-bit word would carry a wrapping sum into the count).  A compaction appends the
//      occupied slots behind the rows path b wrote directly.  Pinned, it aggregates every row (tests, A/B timing).
//
// Key 0xFFFFFFFF is the tables' empty marker: its rows are summed on the side (LDS, then two header words) and appended
// as one output row at the end.  More distinct keys than max_groups: the output cursor passes the bound, nothing is
// written past it and DBHIP_DEV_TABLE_FULL is set; every probe loop is bounded by the table size and stops early once
// the status word holds DBHIP_DEV_TABLE_FULL.  AVG follows from SUM and COUNT; MIN / MAX would be one more LDS and one
// more global column with ds_min / ds_max and atomicMin / atomicMax in the same slots.
//
// Geometry and thresholds: see DESIGN.md §4.8 for the measured figures.
#include <cstdlib>

#include "dbhip_common.hpp"
#include "join_common.hpp"

namespace dbhip {
namespace {

constexpr unsigned kEmpty = 0xFFFFFFFFu;
constexpr int kGbhThreads = 1024;            // path a: one 16-wave workgroup per CU
constexpr unsigned kGbhLdsSlots = 8192;      // path a: 96 KiB of key | sum | count
constexpr unsigned kGbhLdsLg = 13;
constexpr uint32_t kGbhLdsMaxGroups = 4096;  // path a up to this bound: the LDS table at most half full
constexpr int kGbhPartThreads = 256;         // path b workgroups
constexpr unsigned kGbhSubSlots = 4096;      // path b sub-table: 48 KiB, partitions of 2048 +- 270 rows at most 0.57 full
constexpr unsigned kGbhSubLg = 12;
constexpr size_t kGbhGiantRows = 32768;      // path b: a partition above this is sliced, a slice is this many rows
constexpr int kGbhProbe = 64;                // LDS probe bound before a row goes to the global table
constexpr int kGbhCrowd = 16;                // lanes of a wave on one key from which they are summed before the add
constexpr int kGbhPartPairs = 4;             // pairs per lane per step of the partition kernel

// header words (kWsHeader bytes, cleared by every call): [0] status, [2..3] output cursor (uint64), [4] sum and [5] count
// of key 0xFFFFFFFF, [6] giant partitions listed
constexpr unsigned kHdrCursor = 2, kHdrFfSum = 4, kHdrFfCnt = 5, kHdrGiants = 6;

struct GbhTable {      // the global table
  unsigned *keys, *sums, *cnts;  // cnts == nullptr: no counting
  unsigned long long slots;      // 64 <= slots <= 2^32
  unsigned *status;
};
struct GbhOut {
  unsigned *keys, *sums, *cnts;  // cnts may be nullptr
  unsigned long long cap;        // max_groups
  unsigned *hdr;
};

__device__ __forceinline__ unsigned gbh_home(unsigned key, unsigned long long slots) {  // multiply-shift range reduction
  return static_cast<unsigned>((static_cast<unsigned long long>(fmix32(key) * 0x9E3779B1u) * slots) >> 32);
}

// insert-or-find `key` in the global table and add (sum, cnt) to its slot; bounded by the table size, and by 32 more
// steps once the status word says the table is full
__device__ void gbh_global_add(const GbhTable &g, unsigned key, unsigned sum, unsigned cnt) {
  unsigned s = gbh_home(key, g.slots);
  for (unsigned long long i = 0; i < g.slots; ++i) {
    const unsigned k = __hip_atomic_load(g.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool hit = k == key;
    if (!hit && k == kEmpty) {
      const unsigned prev = atomicCAS(g.keys + s, kEmpty, key);
      hit = prev == kEmpty || prev == key;
    }
    if (hit) {
      atomicAdd(g.sums + s, sum);
      if (g.cnts) atomicAdd(g.cnts + s, cnt);
      return;
    }
    s = s + 1 == g.slots ? 0u : s + 1;
    if ((i & 31u) == 31u && (__hip_atomic_load(g.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & DBHIP_DEV_TABLE_FULL)) break;
  }
  atomicOr(g.status, DBHIP_DEV_TABLE_FULL);
}

struct GbhLds {  // an LDS table of 2^lg slots: keys | sums | cnts
  unsigned *keys, *sums, *cnts;
  unsigned lg;
};

__device__ __forceinline__ void gbh_lds_clear(const GbhLds &t, unsigned *ff, unsigned tid, unsigned threads) {
  const unsigned slots = 1u << t.lg;
  for (unsigned i = tid; i < slots; i += threads) {
    t.keys[i] = kEmpty;
    t.sums[i] = 0;
    t.cnts[i] = 0;
  }
  if (tid < 2) ff[tid] = 0;
}

// add (sum, cnt) to key's LDS slot, or to the global table when kGbhProbe steps find none
template <bool kLds>
__device__ __forceinline__ void gbh_add(const GbhLds &t, const GbhTable &g, unsigned key, unsigned sum, unsigned cnt) {
  if (kLds) {
    const unsigned mask = (1u << t.lg) - 1u;
    unsigned s = (fmix32(key) * 0x9E3779B1u) >> (32 - t.lg);
    for (int i = 0; i < kGbhProbe; ++i) {
      const unsigned k = t.keys[s];
      bool hit = k == key;
      if (!hit && k == kEmpty) {
        const unsigned prev = atomicCAS(t.keys + s, kEmpty, key);
        hit = prev == kEmpty || prev == key;
      }
      if (hit) {
        atomicAdd(t.sums + s, sum);
        if (g.cnts) atomicAdd(t.cnts + s, cnt);
        return;
      }
      s = (s + 1) & mask;
    }
  }
  gbh_global_add(g, key, sum, cnt);
}

// One row per lane, every lane of the wave present (live = false: no row).  Key 0xFFFFFFFF goes to ff[0] (sum) and
// ff[1] (count); a crowd of kGbhCrowd+ lanes on the first active lane's key is summed across the wave and added once.
template <bool kLds>
__device__ __forceinline__ void gbh_wave_row(const GbhLds &t, const GbhTable &g, unsigned *ff, unsigned key, unsigned val,
                                             bool live) {
  const unsigned lane = lane_id();
  const bool is_ff = live && key == kEmpty;
  const unsigned long long ffm = __ballot(is_ff);
  if (ffm) {
    const unsigned s = wave_reduce_add(is_ff ? val : 0u);
    if (lane == static_cast<unsigned>(__builtin_ctzll(ffm))) {
      atomicAdd(ff, s);
      atomicAdd(ff + 1, static_cast<unsigned>(__builtin_popcountll(ffm)));
    }
  }
  bool act = live && !is_ff;
  const unsigned long long am = __ballot(act);
  if (!am) return;
  const unsigned first = __builtin_amdgcn_readlane(key, __builtin_ctzll(am));
  const bool same = act && key == first;
  const unsigned long long cm = __ballot(same);
  if (__builtin_popcountll(cm) >= kGbhCrowd) {
    const unsigned s = wave_reduce_add(same ? val : 0u);
    if (lane == static_cast<unsigned>(__builtin_ctzll(cm))) gbh_add<kLds>(t, g, first, s, static_cast<unsigned>(__builtin_popcountll(cm)));
    act = act && !same;
  }
  if (act) gbh_add<kLds>(t, g, key, val, 1u);
}

// every occupied slot of an LDS table into the global table, the side sums into the header
__device__ __forceinline__ void gbh_lds_flush(const GbhLds &t, const GbhTable &g, const unsigned *ff, unsigned *hdr,
                                              unsigned tid, unsigned threads) {
  const unsigned slots = 1u << t.lg;
  for (unsigned i = tid; i < slots; i += threads) {
    const unsigned k = t.keys[i];
    if (k != kEmpty) gbh_global_add(g, k, t.sums[i], t.cnts[i]);
  }
  if (tid == 0 && ff[1]) {
    atomicAdd(hdr + kHdrFfSum, ff[0]);
    atomicAdd(hdr + kHdrFfCnt, ff[1]);
  }
}

// ---- path a: resident grid, private LDS tables --------------------------------------------------------------------
__global__ __launch_bounds__(kGbhThreads) void gbh_lds_kernel(const u32x4 *__restrict__ keys4, const u32x4 *__restrict__ vals4,
                                                               const unsigned *__restrict__ keys, const unsigned *__restrict__ vals,
                                                               size_t n, GbhTable g, unsigned *hdr) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_mem[];
  const GbhLds t{s_mem, s_mem + kGbhLdsSlots, s_mem + 2 * kGbhLdsSlots, kGbhLdsLg};
  unsigned *ff = s_mem + 3 * kGbhLdsSlots;
  const unsigned tid = threadIdx.x;
  gbh_lds_clear(t, ff, tid, kGbhThreads);
  __syncthreads();
  const size_t n4 = n / 4;
  const size_t step = static_cast<size_t>(gridDim.x) * kGbhThreads * 2;
  // two 16-byte loads per column in flight per lane; the loop bound is uniform over the workgroup
  for (size_t base = static_cast<size_t>(blockIdx.x) * kGbhThreads * 2; base < n4; base += step) {
    u32x4 k[2], v[2];
    bool live[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kGbhThreads + tid;
      live[u] = i < n4;
      k[u] = live[u] ? __builtin_nontemporal_load(keys4 + i) : u32x4{0u, 0u, 0u, 0u};
      v[u] = live[u] ? __builtin_nontemporal_load(vals4 + i) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      gbh_wave_row<true>(t, g, ff, k[u].x, v[u].x, live[u]);
      gbh_wave_row<true>(t, g, ff, k[u].y, v[u].y, live[u]);
      gbh_wave_row<true>(t, g, ff, k[u].z, v[u].z, live[u]);
      gbh_wave_row<true>(t, g, ff, k[u].w, v[u].w, live[u]);
    }
  }
  if (blockIdx.x == 0 && tid < kWave) {  // the n % 4 tail rows: wave 0 of workgroup 0
    const bool live = tid < (n & 3);
    const size_t i = n4 * 4 + tid;
    gbh_wave_row<true>(t, g, ff, live ? keys[i] : 0u, live ? vals[i] : 0u, live);
  }
  __syncthreads();
  gbh_lds_flush(t, g, ff, hdr, tid, kGbhThreads);
}

// ---- path c pinned: every row into the global table -----------------------------------------------------------------
__global__ __launch_bounds__(256) void gbh_global_kernel(const unsigned *__restrict__ keys, const unsigned *__restrict__ vals,
                                                         size_t n, GbhTable g, unsigned *hdr) {
  const GbhLds none{nullptr, nullptr, nullptr, 0};
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  for (size_t base = static_cast<size_t>(blockIdx.x) * 256; base < n; base += stride) {
    const size_t i = base + threadIdx.x;
    const bool live = i < n;
    gbh_wave_row<false>(none, g, hdr + kHdrFfSum, live ? keys[i] : 0u, live ? vals[i] : 0u, live);
  }
}

// ---- path b: one workgroup per partition ----------------------------------------------------------------------------
// aggregate pairs [lo, hi) into the sub-table (the loop bound is uniform over the workgroup)
__device__ __forceinline__ void gbh_sub_rows(const GbhLds &t, const GbhTable &g, unsigned *ff, const u32x2 *__restrict__ pairs,
                                             size_t lo, size_t hi) {
  const unsigned tid = threadIdx.x;
  for (size_t base = lo; base < hi; base += kGbhPartPairs * kGbhPartThreads) {
    u32x2 p[kGbhPartPairs];
#pragma unroll
    for (int u = 0; u < kGbhPartPairs; ++u) {
      const size_t i = base + static_cast<size_t>(u) * kGbhPartThreads + tid;
      p[u] = i < hi ? pairs[i] : u32x2{0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kGbhPartPairs; ++u)
      gbh_wave_row<true>(t, g, ff, p[u].x, p[u].y, base + static_cast<size_t>(u) * kGbhPartThreads + tid < hi);
  }
}

__global__ __launch_bounds__(kGbhPartThreads) void gbh_part_kernel(const u32x2 *__restrict__ pairs,
                                                                   const unsigned long long *__restrict__ starts, GbhTable g,
                                                                   GbhOut out, unsigned *giants, unsigned max_giants) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_mem[];
  const GbhLds t{s_mem, s_mem + kGbhSubSlots, s_mem + 2 * kGbhSubSlots, kGbhSubLg};
  unsigned *ff = s_mem + 3 * kGbhSubSlots;  // [0] sum, [1] count of key 0xFFFFFFFF, [2] groups, [3] output base
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1);
  const size_t lo = starts[blockIdx.x], hi = starts[blockIdx.x + 1];
  if (hi - lo > kGbhGiantRows) {  // a giant: left to gbh_giant_kernel (fewer than n / kGbhGiantRows of them)
    if (tid == 0) {
      const unsigned at = atomicAdd(out.hdr + kHdrGiants, 1u);
      if (at < max_giants) giants[at] = blockIdx.x;
    }
    return;
  }
  gbh_lds_clear(t, ff, tid, kGbhPartThreads);
  if (tid == 2) ff[2] = 0;
  __syncthreads();
  gbh_sub_rows(t, g, ff, pairs, lo, hi);
  __syncthreads();
  // number the occupied slots (one LDS atomic per wave and slot row), take an output range by ticket, write
  constexpr unsigned kPer = kGbhSubSlots / kGbhPartThreads;
  unsigned idx[kPer];
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j) {
    const bool occ = t.keys[j * kGbhPartThreads + tid] != kEmpty;
    const unsigned long long m = __ballot(occ);
    unsigned base = 0;
    if (m && lane == 0) base = atomicAdd(ff + 2, static_cast<unsigned>(__builtin_popcountll(m)));
    base = __shfl(base, 0, kWave);
    idx[j] = occ ? base + mbcnt(m) : kEmpty;
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long b = atomicAdd(reinterpret_cast<unsigned long long *>(out.hdr + kHdrCursor),
                                           static_cast<unsigned long long>(ff[2]));
    if (b + ff[2] > out.cap) atomicOr(out.hdr, DBHIP_DEV_TABLE_FULL);
    reinterpret_cast<unsigned long long *>(ff + 4)[0] = b;
    if (ff[1]) {
      atomicAdd(out.hdr + kHdrFfSum, ff[0]);
      atomicAdd(out.hdr + kHdrFfCnt, ff[1]);
    }
  }
  __syncthreads();
  const unsigned long long b = reinterpret_cast<const unsigned long long *>(ff + 4)[0];
#pragma unroll
  for (unsigned j = 0; j < kPer; ++j) {
    const unsigned s = j * kGbhPartThreads + tid;
    if (idx[j] != kEmpty && b + idx[j] < out.cap) {
      const unsigned long long o = b + idx[j];
      out.keys[o] = t.keys[s];
      out.sums[o] = t.sums[s];
      if (out.cnts) out.cnts[o] = t.cnts[s];
    }
  }
}

// the giant partitions' slices: slice q of the listed partitions (in list order) goes to workgroup q % gridDim.x
__global__ __launch_bounds__(kGbhPartThreads) void gbh_giant_kernel(const u32x2 *__restrict__ pairs,
                                                                    const unsigned long long *__restrict__ starts, GbhTable g,
                                                                    unsigned *hdr, const unsigned *giants, unsigned max_giants) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_mem[];
  const GbhLds t{s_mem, s_mem + kGbhSubSlots, s_mem + 2 * kGbhSubSlots, kGbhSubLg};
  unsigned *ff = s_mem + 3 * kGbhSubSlots;
  const unsigned tid = threadIdx.x;
  unsigned listed = hdr[kHdrGiants];
  listed = listed < max_giants ? listed : max_giants;
  if (listed == 0) return;
  if (tid < 2) ff[tid] = 0;
  unsigned long long q0 = 0;  // first slice number of the current giant
  for (unsigned j = 0; j < listed; ++j) {
    const unsigned p = giants[j];
    const size_t lo = starts[p], hi = starts[p + 1];
    const unsigned long long slices = (hi - lo + kGbhGiantRows - 1) / kGbhGiantRows;
    unsigned long long q = q0 + (blockIdx.x + gridDim.x - q0 % gridDim.x) % gridDim.x;  // first slice >= q0 of this workgroup
    for (; q < q0 + slices; q += gridDim.x) {
      const size_t a = lo + (q - q0) * kGbhGiantRows;
      const size_t e = a + kGbhGiantRows < hi ? a + kGbhGiantRows : hi;
      const unsigned slots = kGbhSubSlots;
      for (unsigned i = tid; i < slots; i += kGbhPartThreads) {
        t.keys[i] = kEmpty;
        t.sums[i] = 0;
        t.cnts[i] = 0;
      }
      __syncthreads();
      gbh_sub_rows(t, g, ff, pairs, a, e);
      __syncthreads();
      for (unsigned i = tid; i < slots; i += kGbhPartThreads) {
        const unsigned k = t.keys[i];
        if (k != kEmpty) gbh_global_add(g, k, t.sums[i], t.cnts[i]);
      }
      __syncthreads();
    }
    q0 += slices;
  }
  if (tid == 0 && ff[1]) {
    atomicAdd(hdr + kHdrFfSum, ff[0]);
    atomicAdd(hdr + kHdrFfCnt, ff[1]);
  }
}

// ---- the end of every path ------------------------------------------------------------------------------------------
// occupied global slots behind the rows already written (one cursor atomic per wave and step)
__global__ __launch_bounds__(256) void gbh_compact_kernel(GbhTable g, GbhOut out) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const size_t stride = static_cast<size_t>(gridDim.x) * 256;
  bool over = false;
  for (size_t base = static_cast<size_t>(blockIdx.x) * 256; base < g.slots; base += stride) {
    const size_t s = base + threadIdx.x;
    const unsigned k = s < g.slots ? g.keys[s] : kEmpty;
    const bool occ = k != kEmpty;
    const unsigned long long m = __ballot(occ);
    if (!m) continue;
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(reinterpret_cast<unsigned long long *>(out.hdr + kHdrCursor),
                                 static_cast<unsigned long long>(__builtin_popcountll(m)));
    b = __shfl(b, 0, kWave);
    const unsigned long long o = b + mbcnt(m);
    if (occ) {
      if (o < out.cap) {
        out.keys[o] = k;
        out.sums[o] = g.sums[s];
        if (out.cnts) out.cnts[o] = g.cnts[s];
      } else {
        over = true;
      }
    }
  }
  if (over) atomicOr(out.hdr, DBHIP_DEV_TABLE_FULL);
}

// key 0xFFFFFFFF's row, then *out_groups = min(cursor, max_groups)
__global__ void gbh_finish_kernel(GbhOut out, unsigned long long *out_groups) {
  if (threadIdx.x != 0) return;
  unsigned long long *cursor = reinterpret_cast<unsigned long long *>(out.hdr + kHdrCursor);
  unsigned long long c = *cursor;
  const unsigned ff_cnt = out.hdr[kHdrFfCnt];
  if (ff_cnt) {
    if (c < out.cap) {
      out.keys[c] = kEmpty;
      out.sums[c] = out.hdr[kHdrFfSum];
      if (out.cnts) out.cnts[c] = ff_cnt;
    }
    ++c;
    *cursor = c;
  }
  if (c > out.cap) atomicOr(out.hdr, DBHIP_DEV_TABLE_FULL);
  *out_groups = c < out.cap ? c : out.cap;
}

enum GbhPath { kPathLds = 0, kPathPart = 1, kPathGlobal = 2 };

int gbh_forced_path() {  // DBHIP_GBH_PATH=lds|part|global, read once; -1: by max_groups
  static const int p = [] {
    const char *e = getenv("DBHIP_GBH_PATH");
    if (!e) return -1;
    if (e[0] == 'l') return static_cast<int>(kPathLds);
    if (e[0] == 'p') return static_cast<int>(kPathPart);
    if (e[0] == 'g') return static_cast<int>(kPathGlobal);
    return -1;
  }();
  return p;
}

struct GbhLayout {
  int path;
  unsigned long long slots;  // global table
  unsigned max_giants;
  JlGeometry part;  // path b
  size_t giants_off, keys_off, sums_off, cnts_off, pairs_a_off, pairs_b_off, meta_off, total;
};

GbhLayout gbh_layout(size_t n, uint32_t max_groups) {
  GbhLayout L{};
  const unsigned long long bound = max_groups ? static_cast<unsigned long long>(max_groups) : n;
  const unsigned long long groups = bound < n ? bound : n;  // distinct keys never exceed n
  const int forced = gbh_forced_path();
  L.path = forced >= 0 ? forced : (groups <= kGbhLdsMaxGroups ? kPathLds : kPathPart);
  L.slots = 2 * groups > 64 ? 2 * groups : 64;
  const size_t col = align_up(static_cast<size_t>(L.slots) * sizeof(unsigned), kWsAlign);
  size_t off = kWsHeader;
  if (L.path == kPathPart) {
    L.part = jl_geometry(n, kJlRowsPerPart);
    L.max_giants = static_cast<unsigned>(n / kGbhGiantRows + 1);
    L.giants_off = off;
    off += align_up(static_cast<size_t>(L.max_giants) * sizeof(unsigned), kWsAlign);
  }
  L.keys_off = off;
  L.sums_off = L.keys_off + col;
  L.cnts_off = L.sums_off + col;
  off = L.cnts_off + col;
  if (L.path == kPathPart) {
    const size_t pairs = align_up((n ? n : 1) * sizeof(u32x2), kWsAlign);
    L.pairs_a_off = off;
    L.pairs_b_off = off + pairs;
    L.meta_off = L.pairs_b_off + (L.part.k2 > 1 ? pairs : 0);
    off = align_up(L.meta_off + jl_meta(L.part).bytes(), kWsAlign);
  }
  L.total = off;
  return L;
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_groupby_hash_workspace_bytes(size_t n, uint32_t max_groups) {
  if (n > kJlMaxRows) return 0;
  return gbh_layout(n, max_groups).total;
}

extern "C" int dbhip_groupby_hash_u32(const uint32_t *keys, const uint32_t *vals, size_t n, uint32_t max_groups,
                                      uint32_t *out_keys, uint32_t *out_sums, uint32_t *out_counts, uint64_t *out_groups,
                                      void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  if (n > kJlMaxRows || !out_groups) return DBHIP_EINVAL;
  if (n && (!keys || !vals || !out_keys || !out_sums)) return DBHIP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(vals)) & 15u) return DBHIP_EINVAL;
  const GbhLayout L = gbh_layout(n, max_groups);
  if (!ws_ok(workspace, workspace_bytes, L.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  char *base = static_cast<char *>(workspace);
  unsigned *hdr = reinterpret_cast<unsigned *>(base);
  hipError_t e = fill_async(hdr, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  if (n == 0) return static_cast<int>(fill_async(out_groups, 0, sizeof(uint64_t), s));
  const GbhTable g{reinterpret_cast<unsigned *>(base + L.keys_off), reinterpret_cast<unsigned *>(base + L.sums_off),
                   out_counts ? reinterpret_cast<unsigned *>(base + L.cnts_off) : nullptr, L.slots, hdr};
  const GbhOut out{out_keys, out_sums, out_counts, max_groups ? static_cast<unsigned long long>(max_groups) : n, hdr};
  const size_t col = static_cast<size_t>(L.slots) * sizeof(unsigned);
  e = fill_async(g.keys, 0xFF, col, s);
  if (e == hipSuccess) e = fill_async(g.sums, 0, out_counts ? L.cnts_off - L.sums_off + col : col, s);
  if (e != hipSuccess) return static_cast<int>(e);
  const u32x4 *k4 = reinterpret_cast<const u32x4 *>(keys), *v4 = reinterpret_cast<const u32x4 *>(vals);
  if (L.path == kPathLds) {
    const size_t lds = (3 * static_cast<size_t>(kGbhLdsSlots) + 4) * sizeof(unsigned);
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(gbh_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(lds));
    if (e != hipSuccess) return static_cast<int>(e);
    const size_t steps = (n / 4 + 2 * kGbhThreads - 1) / (2 * kGbhThreads);
    const unsigned grid = static_cast<unsigned>(steps < static_cast<size_t>(dev.cus) ? (steps ? steps : 1) : dev.cus);
    hipLaunchKernelGGL(gbh_lds_kernel, dim3(grid), dim3(kGbhThreads), lds, s, k4, v4, keys, vals, n, g, hdr);
  } else if (L.path == kPathGlobal) {
    hipLaunchKernelGGL(gbh_global_kernel, dim3(capped_grid(n, 256, dev)), dim3(256), 0, s, keys, vals, n, g, hdr);
  } else {
    const unsigned *pairs = nullptr;
    const unsigned long long *starts = nullptr;
    const int rc = jl_partition_side(keys, vals, n, L.part, reinterpret_cast<u32x2 *>(base + L.pairs_a_off),
                                     reinterpret_cast<u32x2 *>(base + L.pairs_b_off),
                                     reinterpret_cast<unsigned long long *>(base + L.meta_off), s, dev, &pairs, &starts);
    if (rc != 0) return rc;
    const size_t lds = (3 * static_cast<size_t>(kGbhSubSlots) + 8) * sizeof(unsigned);
    unsigned *giants = reinterpret_cast<unsigned *>(base + L.giants_off);
    hipLaunchKernelGGL(gbh_part_kernel, dim3(L.part.parts), dim3(kGbhPartThreads), lds, s, reinterpret_cast<const u32x2 *>(pairs),
                       starts, g, out, giants, L.max_giants);
    hipLaunchKernelGGL(gbh_giant_kernel, dim3(static_cast<unsigned>(dev.cus) * 4), dim3(kGbhPartThreads), lds, s,
                       reinterpret_cast<const u32x2 *>(pairs), starts, g, hdr, static_cast<const unsigned *>(giants),
                       L.max_giants);
  }
  hipLaunchKernelGGL(gbh_compact_kernel, dim3(capped_grid(L.slots, 256, dev)), dim3(256), 0, s, g, out);
  hipLaunchKernelGGL(gbh_finish_kernel, dim3(1), dim3(kWave), 0, s, out, reinterpret_cast<unsigned long long *>(out_groups));
  return launch_status();
}
