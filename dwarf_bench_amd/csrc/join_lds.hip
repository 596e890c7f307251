// join_lds.hip — dwarf 4a at every size (and dwarf 4b from 2^16 build rows): radix-partitioned build with
// LDS-resident sub-tables, single-gather probe.  OmniSci semantics: distinct-key table, per-key count, exclusive scan -> position, ids grouped by key, probe ->
// {offset, count} (common/dpcpp/omnisci_hashtable.hpp:58-261).
//
// Why: on MI355X a table in HBM costs one memory-side atomic per step (20-27 G/s random, tools/ubench) — three per
// build row — and three 4-byte gathers per probe row (53 G/s).  Random LDS atomics run at ~4,000 G/s chip-wide
// (profiles/r04_ubench.txt).  So:
//   build  1. partition the build column into K = ceil(n / 2048) partitions (partition.hpp jl_geometry) by the mixed hash,
//             in one or two levels of <= 1024-way scatter (partition.hip: jl_hist / jl_offsets / jl_scatter: LDS counts, one global
//             reservation per bucket per tile, runs of (key, row id) pairs written contiguously; tiles of 4096 rows,
//             of 16384 where a level has 512+ buckets: JlSidePlan; both histograms from ONE read of the keys up to 81920
//             partitions, above that level 0 leaves every row's level-1 bucket as a 16-bit column for the level-1
//             histogram to read instead of the pairs);
//          2. persistent workgroups — as many as are RESIDENT, partitions dealt by ticket — walk the partitions
//             (jl_build_kernel): 3072-slot sub-table in LDS (kJlSubSlots) — plain read of the key's slot, ds_cmpst on
//             an empty one, ONE returning ds_add whose old value is the row's rank inside its key group, LDS exclusive
//             scan -> positions, the fill takes slot and rank of each row from registers kept since the claim, then
//             the sub-table is written out as 8-byte slots {key, first id position | count field} — EVERY slot, empty
//             ones included, carries the position the exclusive scan reached there, and positions run on from one
//             sub-table to the next (the global table is the concatenation of the sub-tables plus one sentinel slot
//             {empty, n}), so a key's match count is ALSO first_position[slot + 1] - first_position[slot]; the bits
//             of the position word that n does not need hold min(count - 1, all ones) (join_common.hpp): the table
//             costs 12 bytes per build row;
//   probe  ONE 8-byte gather per probe row whenever the count fits its field (a 16-byte read of slot and neighbour
//          crossed a 64-byte line for every eighth row: one more memory request); the all-ones field sends the row to
//          the right-hand neighbour.  Partition from the high hash bits, linear probing inside the sub-table, outputs
//          written coalesced in row order.
// A partition may hold any number of rows: one far above its expected size — a hot key — is shared by all workgroups
// ("giant partitions" below).  It may hold any number of DISTINCT keys too: 2048 +- 45 per sigma are expected, a
// sub-table has 3072 slots, and a partition that needs more (keys constructed against the hash) is built in a table of
// its own in HBM by one workgroup (jl_spill_partition; until round 4 this raised DBHIP_DEV_TABLE_FULL) — the join
// answers every input the reference's table answers (omnisci_hashtable.hpp:80-108, ht_size = 2 * distinct).
#include "dbhip_common.hpp"
#include "join_common.hpp"

namespace dbhip {
namespace {

#ifndef DBHIP_JL_BUILD_THREADS
#define DBHIP_JL_BUILD_THREADS 512
#endif
constexpr int kJlBuildThreads = DBHIP_JL_BUILD_THREADS;  // per-partition build workgroup; 2^26 rows: 512 -> 1398 us,
                                                        // 256 -> 1514 us, 1024 -> 1465 us (whole build); round 4, resident
                                                        // ticketed grid: build 920 / 938 / 1148 us and the radix join's fused
                                                        // kernel 605 / 700 / 1285 us with 512 / 256 / 1024 threads

// ---- per-partition build in LDS --------------------------------------------------------------------
// A partition's rows come either as two columns (the level-0 output, when one level suffices) or as (key, row id)
// pairs (the level-1 output): prids == nullptr means pkeys points at pairs.
__device__ __forceinline__ u32x2 jl_row(const unsigned *__restrict__ pkeys, const unsigned *__restrict__ prids,
                                        size_t i) {
  (void)prids;  // both scatter levels write (key, row id) pairs
  return reinterpret_cast<const u32x2 *>(pkeys)[i];
}

// Slot of `key` in the LDS key array `lk`: a plain read first — a key that is already there (a duplicate row) and
// every step of a collision chain need no atomic — ds_cmpst only on a slot read as empty.  Returns kJlSubSlots for
// the sentinel key (flagged in the status word) and for a full sub-table — more distinct keys than slots: *full (an LDS
// word of the caller) is set, the caller hands the partition to the spill path.
__device__ __forceinline__ unsigned jl_claim(unsigned *lk, unsigned key, unsigned *status, unsigned *full) {
  if (key == kEmptyKey) {  // the sentinel is not a key (join/join_omnisci.cpp:52): flag it, drop the row
    atomicOr(status, DBHIP_DEV_KEY_RANGE);
    return kJlSubSlots;
  }
  unsigned s = jl_home_slot(fmix32(key));
  for (unsigned tries = 0; tries < kJlSubSlots; ++tries) {
    unsigned k = lk[s];
    if (k == kEmptyKey) k = atomicCAS(&lk[s], kEmptyKey, key);
    if (k == kEmptyKey || k == key) return s;
    s = jl_next_slot(s);
  }
  *full = 1u;
  return kJlSubSlots;
}

// ---- lanes of a wave that meet on one LDS counter -----------------------------------------------------------------
// A hot key is many rows of a wave on one counter of the sub-table, and the LDS serves the lanes of one atomic that hit
// the same word one after the other.  jl_take: every live lane takes the next value of its counter (UP: returns the old
// value, the counter grows; down: returns old - 1, the counter shrinks); when kJlCrowd lanes or more share the first live
// lane's counter, one of them adds for all and the others derive their values from its result.  `id` names the counter
// (lanes with the same id pass the same pointer).  Every lane of the wave must call it together.
constexpr unsigned kJlCrowd = 16;
template <bool UP>
__device__ __forceinline__ unsigned jl_take(unsigned *counter, unsigned id, bool live) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned long long act = __ballot(live);
  if (act == 0) return 0u;  // (uniform)
  const unsigned first = __builtin_amdgcn_readlane(id, __builtin_ctzll(act));
  const bool same = live && id == first;
  const unsigned long long crowd = __ballot(same);
  const unsigned c = static_cast<unsigned>(__builtin_popcountll(crowd));
  if (c >= kJlCrowd) {  // (uniform)
    const unsigned leader = static_cast<unsigned>(__builtin_ctzll(crowd));
    unsigned old = 0;
    if (lane == leader) old = UP ? atomicAdd(counter, c) : atomicSub(counter, c);
    old = __builtin_amdgcn_readlane(old, leader);
    if (same) return UP ? old + mbcnt(crowd) : old - 1u - mbcnt(crowd);
  }
  if (!live) return 0u;
  return UP ? atomicAdd(counter, 1u) : atomicSub(counter, 1u) - 1u;
}

// Barriers of the build kernel order LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait for the
// next partition's prefetched rows and for every id / table store still on its way to memory (DBHIP_JL_FULL_BARRIER=1
// restores it for A/B timing).
#ifdef DBHIP_JL_FULL_BARRIER
#define JL_BUILD_BARRIER() __syncthreads()
#else
#define JL_BUILD_BARRIER() wg_barrier_lds_only()
#endif
// kMatch = false: the build of the one-to-many join (sub-tables published to HBM for a later probe launch).
// kMatch = true: the radix join — the probe side was partitioned with the SAME geometry, so partition p of S meets
// the sub-table of partition p of R while it is still in LDS: no table is written, no random access leaves the CU;
// results go out in S's partition order together with the probe row ids.
struct JlMatchArgs {
  const u32x2 *spairs;               // probe side, partition-major (key, row id) pairs
  const unsigned long long *sstarts; // parts + 1 offsets
  unsigned *out_rid, *out_pos, *out_cnt;
};
// The giant partitions' scratch (join_common.hpp: jl_giant_bytes): max == 0 switches the path off.
struct JlGiants {
  unsigned *base;           // count, pad[3] | part[max] | done[max] | counts[max][kJlSubSlots] | cursors[max][kJlSubSlots] | tables
  unsigned max;
  unsigned long long rows;  // a partition with more rows than this is a giant
  unsigned long long probe_rows;  // radix join: ... or with more probe rows than this
  unsigned with_tables;     // radix join: the giants' sub-tables are in the scratch (kJlSubSlots + 1 slots each), not in `table`
  __host__ __device__ u32x2 *scratch_table(unsigned g) const {
    return reinterpret_cast<u32x2 *>(cursors(max)) + static_cast<size_t>(g) * (kJlSubSlots + 1);
  }
  __host__ __device__ u32x2 *sub_table(u32x2 *table, unsigned g, size_t part) const {
    if (with_tables) return scratch_table(g);
    return table + part * kJlSubSlots;
  }
  __host__ __device__ unsigned *count() const { return base; }
  __host__ __device__ unsigned *part() const { return base + 4; }
  __host__ __device__ unsigned *done() const { return base + 4 + max; }
  __host__ __device__ unsigned *counts(unsigned g) const {
    return base + ((4 + 2 * static_cast<size_t>(max) + 3) & ~static_cast<size_t>(3)) + static_cast<size_t>(g) * kJlSubSlots;
  }
  __host__ __device__ unsigned *cursors(unsigned g) const { return counts(max) + static_cast<size_t>(g) * kJlSubSlots; }
};
// The spilled partitions' scratch (join_common.hpp).
struct JlSpill {
  unsigned *area;  // dir[parts] {first slot + 1 | 0, slots} | list[max_list] | keys[pool] | pos[pool] | cnt[pool]
  unsigned parts, max_list, list_words;
  unsigned long long pool;
  __host__ __device__ u32x2 *dir() const { return reinterpret_cast<u32x2 *>(area); }
  __host__ __device__ unsigned *list() const { return area + 2 * static_cast<size_t>(parts); }
  __host__ __device__ unsigned *keys() const { return list() + list_words; }
  __host__ __device__ unsigned *pos() const { return keys() + pool; }
  __host__ __device__ unsigned *cnt() const { return pos() + pool; }
};
// (a pure function of the build's partition and row counts: the build kernels take only the area's address — their scalar
//  registers are all in use — and derive the rest where the rare path needs it)
__host__ __device__ __forceinline__ JlSpill jl_spill_of(void *area, unsigned parts, size_t n) {
  return JlSpill{static_cast<unsigned *>(area), parts, jl_max_spill(n), static_cast<unsigned>(jl_spill_list_words(n)),
                 static_cast<unsigned long long>(jl_spill_pool_slots(n))};
}
__device__ __forceinline__ unsigned jl_spill_home(unsigned key, unsigned cap) {
  return static_cast<unsigned>((static_cast<unsigned long long>(fmix32(key * 0x9E3779B1u ^ 0x7F4A7C15u)) * cap) >> 32);
}
__device__ __forceinline__ unsigned jl_ld(const unsigned *p) {  // a read that no stale line of this CU's L1 can answer
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// {first id position, count} of `key` in the spilled partition's table [base, base + cap), {0, 0} if it is not there
__device__ __forceinline__ void jl_spill_lookup(const JlSpill &sp, unsigned base, unsigned cap, unsigned key, unsigned *pos_out,
                                                unsigned *cnt_out) {
  *pos_out = *cnt_out = 0;
  if (key == kEmptyKey) return;
  const unsigned *keys = sp.keys() + base;
  unsigned s = jl_spill_home(key, cap);
  for (unsigned tries = 0; tries < cap; ++tries) {
    const unsigned k = jl_ld(&keys[s]);
    if (k == key) {
      *pos_out = jl_ld(&sp.pos()[base + s]);
      *cnt_out = jl_ld(&sp.cnt()[base + s]);
      return;
    }
    if (k == kEmptyKey) return;
    s = s + 1 == cap ? 0u : s + 1;
  }
}
// One workgroup (kJlGiantThreads = kJlBuildThreads threads, all of them call this together) builds the table of partition
// `part` — rows [lo, hi) of the partition-major pairs — in the pool and writes the partition's ids[lo, hi); radix join
// (match.spairs != nullptr): it then answers the partition's probe rows.  Correct for any rows; not written to be fast:
// every step is a memory-side atomic (a hot key of such a partition is served at one atomic per ~11 ns).
// `sub` (one-to-many build, a giant that spilled): the partition's sub-table of the published table, which jl_giant_count
// left half-claimed — it is rewritten as an empty, MARKED one (jl_probe_sub; the build kernel publishes a spilled
// partition of its own that way itself).
__device__ __noinline__ void jl_spill_partition(const JlSpill sp, const u32x2 *__restrict__ rows, size_t lo, size_t hi, unsigned part,
                                                unsigned *__restrict__ ids, unsigned *status, const JlMatchArgs match, size_t slo,
                                                size_t shi, u32x2 *sub, unsigned pos_bits) {
  constexpr unsigned kT = kJlBuildThreads;
  __shared__ unsigned s_base, s_w[kT / kWave];
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const unsigned cap = static_cast<unsigned>(jl_spill_cap(hi - lo));
  __syncthreads();
  if (tid == 0) s_base = atomicAdd(status + kJlHdrSpillPool, cap);
  __syncthreads();
  const unsigned base = s_base;
  if (static_cast<unsigned long long>(base) + cap > sp.pool) {  // (cannot happen: the pool holds every partition that can spill)
    if (tid == 0) atomicOr(status, DBHIP_DEV_TABLE_FULL);
    return;
  }
  unsigned *keys = sp.keys() + base, *pos = sp.pos() + base, *cnt = sp.cnt() + base;
  for (unsigned i = tid; i < cap; i += kT) {
    keys[i] = kEmptyKey;
    cnt[i] = 0;
  }
  __threadfence();
  __syncthreads();
  // 1. distinct keys and their row counts
  for (size_t i = lo + tid; i < hi; i += kT) {
    const unsigned key = rows[i].x;
    if (key == kEmptyKey) {  // the sentinel is not a key (join/join_omnisci.cpp:52): flagged, the row is dropped
      atomicOr(status, DBHIP_DEV_KEY_RANGE);
      continue;
    }
    unsigned s = jl_spill_home(key, cap);
    while (true) {  // (cap > rows >= distinct keys: an empty slot exists)
      const unsigned k = atomicCAS(&keys[s], kEmptyKey, key);
      if (k == kEmptyKey || k == key) break;
      s = s + 1 == cap ? 0u : s + 1;
    }
    atomicAdd(&cnt[s], 1u);
  }
  __threadfence();
  __syncthreads();
  // 2. first id position of every key: exclusive scan of the counts in slot order, from the partition's first position
  unsigned run = static_cast<unsigned>(lo);
  for (unsigned c0 = 0; c0 < cap; c0 += kT) {  // (uniform)
    const unsigned i = c0 + tid;
    const unsigned c = i < cap && jl_ld(&keys[i]) != kEmptyKey ? jl_ld(&cnt[i]) : 0u;
    const unsigned incl = wave_inclusive_scan(c);
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (unsigned w = 0; w < kT / kWave; ++w) {
      before += w < wave ? s_w[w] : 0u;
      total += s_w[w];
    }
    if (i < cap) pos[i] = run + before + incl - c;
    run += total;
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  // 3. ids: every row takes the next place of its key's range (the position word is the cursor; step 4 puts it back)
  for (size_t i = lo + tid; i < hi; i += kT) {
    const u32x2 row = rows[i];
    if (row.x == kEmptyKey) continue;
    unsigned s = jl_spill_home(row.x, cap);
    while (jl_ld(&keys[s]) != row.x) s = s + 1 == cap ? 0u : s + 1;
    ids[atomicAdd(&pos[s], 1u)] = row.y;
  }
  __threadfence();
  __syncthreads();
  for (unsigned i = tid; i < cap; i += kT)
    if (jl_ld(&keys[i]) != kEmptyKey) pos[i] = jl_ld(&pos[i]) - jl_ld(&cnt[i]);
  __threadfence();
  __syncthreads();
  if (tid == 0) sp.dir()[part] = u32x2{base + 1u, cap};
  if (sub != nullptr) {
    const unsigned word = static_cast<unsigned>(lo) | (pos_bits < 32 ? 1u << pos_bits : 0u);
    for (unsigned i = tid; i < kJlSubSlots; i += kT) sub[i] = u32x2{kEmptyKey, word};
  }
  // 4. radix join: the partition's probe rows
  if (match.spairs != nullptr)
    for (size_t j = slo + tid; j < shi; j += kT) {
      const u32x2 row = match.spairs[j];
      unsigned p, c;
      jl_spill_lookup(sp, base, cap, row.x, &p, &c);
      match.out_rid[j] = row.y;
      match.out_pos[j] = p;
      match.out_cnt[j] = c;
    }
  __syncthreads();
}
// a workgroup whose partition does not fit its sub-table lists it for the spill path (thread 0)
__device__ __forceinline__ void jl_spill_list(const JlSpill &sp, unsigned part, unsigned *status) {
  const unsigned g = atomicAdd(status + kJlHdrSpilled, 1u);
  if (g < sp.max_list) sp.list()[g] = part;
  else atomicOr(status, DBHIP_DEV_TABLE_FULL);  // (cannot happen: fewer partitions can spill than the list holds)
}

// kInline: the workgroup that finds its partition overfull builds the spill table itself, at once (small inputs: no
// launch behind this one looks at the list); otherwise it lists the partition for the tail of jl_giant_ids_kernel.
template <bool kMatch, bool kInline>
__global__ __launch_bounds__(kJlBuildThreads) __attribute__((amdgpu_waves_per_eu(kInline ? 4 : 6))) void jl_build_kernel(const unsigned *__restrict__ pkeys,
                                                                   const unsigned *__restrict__ prids,
                                                                   const unsigned long long *__restrict__ starts,
                                                                   u32x2 *__restrict__ table, unsigned parts,
                                                                   unsigned n_rows, unsigned pos_bits,
                                                                   unsigned *__restrict__ ids, unsigned *status,
                                                                   JlMatchArgs match, JlGiants giants, unsigned *spill_area) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_lds[];
  unsigned *lk = s_lds;                // keys
  unsigned *lc = s_lds + kJlSubSlots;  // counts in step 1; the scan turns the same words into positions:
  unsigned *lp = lc;                   // first id position of the slot, bumped to its end by the fill.
  // (two arrays instead of three: 24 KiB per workgroup at 3072 slots)
  __shared__ unsigned s_wsum[kJlBuildThreads / kWave];
  __shared__ unsigned s_end;  // where the last slot's id range ends = first position behind the partition's counted rows
  __shared__ unsigned s_ticket;  // the ticket thread 0 took for the partition after the next one
  __shared__ unsigned s_full;    // a row of this partition found the sub-table full of other keys
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  // Partitions by ticket (round 4).  A static deal (partition p, p + grid, ...) ends when the SLOWEST workgroup has walked
  // its share, and workgroups are not equally fast (CUs share L2 slices and memory channels unevenly): the fused kernel
  // took 669 us for the 37504 partitions of 2^26 rows, 49 per workgroup, and 8903 us / 16 = 556 us per 2^26 rows at 2^30,
  // 781 per workgroup, where the differences average out.  The first partition is blockIdx, every further one comes from
  // a counter in the workspace header (status[32]; status[33] counts the workgroups that have left: the last one zeroes
  // both for the next launch).  The ticket is taken one step ahead of the prefetch, by thread 0, and handed over
  // through LDS where the prefetched rows are waited for — a returning atomic counts in vmcnt like a load.
  unsigned *const ticket_word = status + kJlHdrTicket, *const left_word = status + kJlHdrLeft;
  // a partition holds ~kJlRowsPerPart rows (+ 6 sigma of a Poisson count): rows per thread whose slot and row id
  // stay in registers between steps 1 and 3, and rows per thread loaded one partition ahead
  constexpr unsigned kRowsPerPart = kMatch ? kJrRowsPerPart : kJlRowsPerPart;  // (the radix join partitions for fewer rows)
  constexpr int kJlCached = static_cast<int>((kRowsPerPart + kRowsPerPart / 8 + kJlBuildThreads - 1) / kJlBuildThreads);
  constexpr int kJlPre = kJlCached;  // every cached row comes from the prefetch: a row loaded inside the claim phase made
                                     // the compiler wait (s_waitcnt vmcnt(0)) for the prefetch issued just before it too
  static_assert(static_cast<unsigned>(kJlCached) * kJlBuildThreads <= kJlSubSlots, "a partition without overflow rows fits the id staging area");

  // Persistent workgroups walk the partitions with a stride of the grid; a workgroup is a chain of dependent
  // phases (load, claim, scan, fill, publish), so the NEXT partition's rows are requested before the current
  // partition's LDS work starts and arrive while it runs.
  unsigned part = blockIdx.x;
  if (part >= parts) return;
  unsigned lo = static_cast<unsigned>(starts[part]), hi = static_cast<unsigned>(starts[part + 1]);  // (32-bit: n <= 2^31 rows; the kernel is short of scalar registers)
  unsigned npart = parts;  // the partition after this one
  {
    if (tid == 0) s_ticket = atomicAdd(ticket_word, 1u);
    __syncthreads();
    npart = static_cast<unsigned>(gridDim.x) + s_ticket;
    __syncthreads();
  }
  u32x2 carry[kJlPre];  // the current partition's rows, in registers that no load is pending on
#pragma unroll
  for (int r = 0; r < kJlPre; ++r) {
    const unsigned i = lo + tid + static_cast<unsigned>(r) * kJlBuildThreads;
    carry[r] = i < hi ? jl_row(pkeys, prids, i) : u32x2{0u, 0u};
  }
#pragma unroll
  for (int r = 0; r < kJlPre; ++r) {  // (see below: the loop must not carry a register that a load defined)
    asm volatile("v_mov_b32 %0, %0" : "+v"(carry[r].x));
    asm volatile("v_mov_b32 %0, %0" : "+v"(carry[r].y));
  }
  while (true) {
    // the offsets this step needs, requested together: the next partition's rows and (radix join) this partition's probe rows
    unsigned nlo = 0, nhi = 0, slo = 0, shi = 0;
    unsigned tk = 0;
    if (npart < parts) {
      nlo = static_cast<unsigned>(starts[npart]);
      nhi = static_cast<unsigned>(starts[npart + 1]);
      if (tid == 0) tk = atomicAdd(ticket_word, 1u);  // for the step after the next (consumed below, with the prefetch)
    }
    if (kMatch) {
      slo = static_cast<unsigned>(match.sstarts[part]);
      shi = static_cast<unsigned>(match.sstarts[part + 1]);
    }
    if (giants.max != 0 && (hi - lo > giants.rows || (kMatch && shi - slo > giants.probe_rows))) {  // (uniform)
      // a giant partition (join_common.hpp): listed for the jl_giant_* kernels, which all workgroups share.  Build: it is
      // published here as an EMPTY sub-table — the state their claims of its slots start from.  Radix join: nothing of
      // it is done here, neither side; its sub-table will be one of the scratch tables, emptied here.
      if (tid == 0) s_end = atomicAdd(giants.count(), 1u);
      JL_BUILD_BARRIER();
      const unsigned slot = s_end;
      JL_BUILD_BARRIER();  // (s_end is written again below)
      if (slot < giants.max) {  // always: the list is sized for every partition that can be this large
        if (tid == 0) giants.part()[slot] = static_cast<unsigned>(part);
        unsigned *gc = giants.counts(slot);
        for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) gc[i] = 0;
        if (kMatch) {
          u32x2 *sub = giants.scratch_table(slot);
          for (unsigned i = tid; i < kJlSubSlots + 1; i += kJlBuildThreads) sub[i] = u32x2{kEmptyKey, 0u};
          shi = slo;
        }
        hi = lo;
      }
    }
    for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) {
      lk[i] = kEmptyKey;
      lc[i] = 0;
    }
    if (tid == 0) {
      s_full = 0;
      reinterpret_cast<u32x2 *>(spill_area)[part] = u32x2{0u, 0u};  // "not spilled" (every partition passes here exactly once per build)
    }
    u32x2 cur[kJlPre];
#pragma unroll
    for (int r = 0; r < kJlPre; ++r) cur[r] = carry[r];
    u32x2 pre[kJlPre];  // the next partition's rows, in flight
#pragma unroll
    for (int r = 0; r < kJlPre; ++r) pre[r] = u32x2{0u, 0u};
    if (npart < parts) {
#pragma unroll
      for (int r = 0; r < kJlPre; ++r) {
        const unsigned i = nlo + tid + static_cast<unsigned>(r) * kJlBuildThreads;
        if (i < nhi) pre[r] = jl_row(pkeys, prids, i);
      }
    }
    // radix join: this partition's first probe rows (four consecutive ones per lane) are requested now and arrive
    // while the sub-table is built
    u32x2 srow[4] = {u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}};
    if (kMatch) {
      const unsigned j0 = slo + 4 * static_cast<unsigned>(tid);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (j0 + q < shi) srow[q] = match.spairs[j0 + q];
    }
    JL_BUILD_BARRIER();
    // 1. claim the key's slot and take the row's rank inside its key group.  LDS atomics are what bounds this kernel
    //    (measured with the output stores compiled out: 400 of its 550 us at 2^26 rows), so a row costs two of them,
    //    not three: a plain read of the slot first (a duplicate of an already published key and every step of a
    //    collision chain need no ds_cmpst), ds_cmpst only on a slot read as empty, and ONE returning ds_add whose
    //    old value is the row's rank — the fill then needs no second atomic.  Two attempts at overlapping the LDS round
    //    trips of a lane's rows both measured SLOWER: a loop of rounds (every row one probe step per round: 1583 vs 1186 us
    //    for the 2^26 build) and a staged form (all first reads, then all first ds_cmpst, stragglers one by one, then all
    //    rank atomics: 1194 vs 1110 us; the fused match kernel 940 vs 870 us) — in-kernel stamps put this phase at a
    //    median 3500 of a 6500-cycle partition step with a 12000-cycle 90th percentile: the CU's LDS pipeline, shared
    //    by four workgroups of random-address traffic, is what the rows queue on, not their own dependency chain.
    unsigned c_slot[kJlCached], c_rid[kJlCached], c_rank[kJlCached];
#pragma unroll
    for (int r = 0; r < kJlCached; ++r) {
      const unsigned i = lo + tid + static_cast<unsigned>(r) * kJlBuildThreads;
      c_slot[r] = kJlSubSlots;  // "no row"
      c_rid[r] = 0;
      c_rank[r] = 0;
      if (i < hi) {
        const u32x2 row = r < kJlPre ? cur[r < kJlPre ? r : 0] : jl_row(pkeys, prids, i);
        c_rid[r] = row.y;
        const unsigned s = jl_claim(lk, row.x, status, &s_full);
        if (s < kJlSubSlots) {
          c_slot[r] = s;
          c_rank[r] = atomicAdd(&lc[s], 1u);
        }
      }
    }
    // a partition far above its expected size: the rows beyond the cached ones are counted AFTER every cached row has
    // its rank (so the cached rows of a key hold the ranks 0 .. k-1 and these rows own the ranks behind them)
    const bool overflow = hi - lo > static_cast<unsigned>(kJlCached) * kJlBuildThreads;  // uniform over the workgroup
    if (overflow) {
      // (four rows per lane in flight and crowds of one key added by one lane, round 3: a partition of 2^16 rows of one
      //  key took a workgroup 2.6 ns per row with one load in flight and every lane's atomic on the same word)
      JL_BUILD_BARRIER();
      for (unsigned i0 = lo + static_cast<unsigned>(kJlCached) * kJlBuildThreads; i0 < hi; i0 += 4 * static_cast<unsigned>(kJlBuildThreads)) {
        u32x2 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned i = i0 + static_cast<unsigned>(q) * kJlBuildThreads + tid;
          row[q] = i < hi ? jl_row(pkeys, prids, i) : u32x2{0u, 0u};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool have = i0 + static_cast<unsigned>(q) * kJlBuildThreads + tid < hi;
          const unsigned s = have ? jl_claim(lk, row[q].x, status, &s_full) : kJlSubSlots;
          (void)jl_take<true>(&lc[s < kJlSubSlots ? s : 0u], s, s < kJlSubSlots);
        }
      }
    }
    JL_BUILD_BARRIER();
    const bool spilled = s_full != 0u;
    if (spilled) {  // (uniform) more distinct keys than slots: the spill path builds this partition; here it becomes an
                    // empty one — cleared counters scan to "every position = lo", which is what gets published; the rows'
                    // stale slot / rank registers reach nothing (no counted rows are written out; guards below)
      const JlSpill spill = jl_spill_of(spill_area, parts, n_rows);
      if (kInline) {
        jl_spill_partition(spill, reinterpret_cast<const u32x2 *>(pkeys), lo, hi, static_cast<unsigned>(part), ids, status, match,
                           slo, shi, nullptr, pos_bits);
        if (tid == 0) atomicAdd(status + kJlHdrSpilled, 1u);
      } else if (tid == 0) {
        jl_spill_list(spill, static_cast<unsigned>(part), status);
      }
      // (a build of exactly 2^31 rows has no count field to mark a spilled sub-table with: that one size still fails loudly)
      if (!kMatch && pos_bits >= 32 && tid == 0) atomicOr(status, DBHIP_DEV_TABLE_FULL);
      JL_BUILD_BARRIER();
      for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) {
        lk[i] = kEmptyKey;
        lc[i] = 0;
      }
      JL_BUILD_BARRIER();
    }
    // 2. exclusive scan of the counts -> first id position of every slot
    constexpr unsigned kPer = kJlSubSlots / kJlBuildThreads;
    unsigned c[kPer], mine = 0;
#pragma unroll
    for (unsigned j = 0; j < kPer; ++j) {
      c[j] = lc[tid * kPer + j];
      mine += c[j];
    }
    const unsigned incl = wave_inclusive_scan(mine);
    if (lane == kWave - 1) s_wsum[wave] = incl;
    JL_BUILD_BARRIER();
    unsigned run = static_cast<unsigned>(lo) + incl - mine;
    for (unsigned w = 0; w < wave; ++w) run += s_wsum[w];
    // every thread has its counts in registers (the barrier above): overwrite them with the positions
#pragma unroll
    for (unsigned j = 0; j < kPer; ++j) {
      lp[tid * kPer + j] = run;
      run += c[j];
    }
    if (tid == kJlBuildThreads - 1) s_end = run;
    JL_BUILD_BARRIER();
    // vmcnt counts loads and stores of a wave in issue order: the next partition's rows (requested at the top of this
    // iteration) are waited for HERE, while nothing but those loads is outstanding — at the top of the next iteration
    // the wait would also cover every store issued below, i.e. a full store drain per partition
    // (the rows move on through a v_mov the compiler cannot see through: a loop-carried register that a load defined
    //  is waited for with vmcnt(0) at the loop head whatever happened in between)
    u32x2 nxt[kJlPre];
#pragma unroll
    for (int r = 0; r < kJlPre; ++r) {
      asm volatile("v_mov_b32 %0, %1" : "=v"(nxt[r].x) : "v"(pre[r].x));
      asm volatile("v_mov_b32 %0, %1" : "=v"(nxt[r].y) : "v"(pre[r].y));
    }
    if (tid == 0 && npart < parts) {  // (read by everyone behind the barrier that closes this step)
      unsigned got;
      asm volatile("v_mov_b32 %0, %1" : "=v"(got) : "v"(tk));
      s_ticket = got;
    }
    if (!kMatch) {
    // 3. publish the sub-table: {key, first position | count field} for every slot.  Positions are an exclusive scan
    //    in slot order, so slot i ends where slot i+1 starts (the last one at s_end).  Output stores are what this
    //    kernel waits for (per-instruction issue cost: with the stores compiled out it ran 150 us shorter at 2^26
    //    rows), so every store instruction carries 16 bytes per lane: two slots here, four ids below.  Written once,
    //    read by another launch: non-temporal.
    u32x4 *dst = reinterpret_cast<u32x4 *>(table + static_cast<size_t>(part) * kJlSubSlots);  // 16-byte aligned: kJlSubSlots is even
    const unsigned cnt_esc = pos_bits < 32 ? (1u << (32 - pos_bits)) - 1u : 0u;
    for (unsigned i = tid; i < kJlSubSlots / 2; i += kJlBuildThreads) {
      const unsigned p0 = lp[2 * i], p1 = lp[2 * i + 1], p2 = 2 * i + 2 < kJlSubSlots ? lp[2 * i + 2] : s_end;
      const unsigned c0 = p1 - p0, c1 = p2 - p1;
      unsigned f0 = c0 ? c0 - 1 : 0u, f1 = c1 ? c1 - 1 : 0u;
      f0 = f0 < cnt_esc ? f0 : cnt_esc;
      f1 = f1 < cnt_esc ? f1 : cnt_esc;
      if (spilled) f0 = f1 = 1u;  // (uniform) the mark on a spilled partition's empty slots: see jl_probe_sub
      const unsigned w0 = pos_bits < 32 ? (p0 | (f0 << pos_bits)) : p0, w1 = pos_bits < 32 ? (p1 | (f1 << pos_bits)) : p1;
      __builtin_nontemporal_store(u32x4{lk[2 * i], w0, lk[2 * i + 1], w1}, dst + i);
    }
    if (part + 1 == parts && tid == 0) table[static_cast<size_t>(parts) * kJlSubSlots] = u32x2{kEmptyKey, n_rows};  // sentinel
    } else {
    // 3'. probe: the rows of S's partition `part` against the sub-table in LDS — plain LDS reads; the results
    //     {probe row id, first id position, count} leave coalesced in S's partition order
      //     FOUR consecutive rows per lane: one 16-byte store per output column and lane (4-byte stores made this
      //     kernel store-issue-bound: 914 us at 2^26 x 2^26 rows)
      typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
      const unsigned jfirst = slo + 4 * static_cast<unsigned>(tid);
      if (!spilled)  // (a spilled partition's probe rows are answered by jl_spill_partition)
      for (unsigned j0 = jfirst; j0 < shi; j0 += 4 * static_cast<unsigned>(kJlBuildThreads)) {
        unsigned rid[4], pos[4], cnt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rid[q] = pos[q] = cnt[q] = 0;
          if (j0 + q < shi) {
            const u32x2 row = j0 == jfirst ? srow[q] : match.spairs[j0 + q];
            const unsigned key = row.x;
            rid[q] = row.y;
            unsigned sl = jl_home_slot(fmix32(key));
            for (unsigned tries = 0; tries < kJlSubSlots && key != kEmptyKey; ++tries) {
              const unsigned k = lk[sl];
              if (k == key) {
                pos[q] = lp[sl];
                cnt[q] = (sl + 1 < kJlSubSlots ? lp[sl + 1] : s_end) - pos[q];
                break;
              }
              if (k == kEmptyKey) break;
              sl = jl_next_slot(sl);
            }
          }
        }
        if (j0 + 3 < shi) {
          *reinterpret_cast<u32x4_a4 *>(match.out_rid + j0) = u32x4{rid[0], rid[1], rid[2], rid[3]};
          *reinterpret_cast<u32x4_a4 *>(match.out_pos + j0) = u32x4{pos[0], pos[1], pos[2], pos[3]};
          *reinterpret_cast<u32x4_a4 *>(match.out_cnt + j0) = u32x4{cnt[0], cnt[1], cnt[2], cnt[3]};
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (j0 + q < shi) {
              match.out_rid[j0 + q] = rid[q];
              match.out_pos[j0 + q] = pos[q];
              match.out_cnt[j0 + q] = cnt[q];
            }
        }
      }
    }
    // 4. fill: id position = first position of the slot + rank of the row (slot / rank / row id from the registers of
    //    step 1: a plain LDS read, no atomic).  The partition's ids are ONE contiguous range [lo, s_end): they are
    //    staged in LDS — in the key array, free once it is published — and leave as 16-byte stores.  A partition far
    //    above its expected size (rows beyond the cached ones, `overflow`) stores every id directly instead.
    unsigned c_pos[kJlCached];
#pragma unroll
    for (int r = 0; r < kJlCached; ++r) c_pos[r] = c_slot[r] < kJlSubSlots ? lp[c_slot[r]] + c_rank[r] : 0xFFFFFFFFu;
    if (!overflow) {
      JL_BUILD_BARRIER();  // every key and position word has been read: the key array becomes the staging area
      unsigned *stage = lk;
      const unsigned lo32 = static_cast<unsigned>(lo);
#pragma unroll
      for (int r = 0; r < kJlCached; ++r)
        if (c_pos[r] != 0xFFFFFFFFu) stage[c_pos[r] - lo32] = c_rid[r];  // rows <= cached rows <= kJlSubSlots (static_assert)
      JL_BUILD_BARRIER();
      const unsigned rows = s_end - lo32;  // counted rows of the partition
      unsigned *out = ids + lo;
      const unsigned head0 = ((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(out)) & 15u)) & 15u) / 4u;  // up to the next 16-byte boundary
      const unsigned head = head0 < rows ? head0 : rows;
      if (tid < head) out[tid] = stage[tid];
      const unsigned body = (rows - head) / 4;
      for (unsigned v = tid; v < body; v += kJlBuildThreads) {
        const unsigned at = head + 4 * v;
        __builtin_nontemporal_store(u32x4{stage[at], stage[at + 1], stage[at + 2], stage[at + 3]},
                                    reinterpret_cast<u32x4 *>(out + at));
      }
      const unsigned tail0 = head + 4 * body;
      if (tid < 4 && tail0 + tid < rows) out[tail0 + tid] = stage[tail0 + tid];
    } else if (!spilled) {
#pragma unroll
      for (int r = 0; r < kJlCached; ++r)
        if (c_pos[r] != 0xFFFFFFFFu) ids[c_pos[r]] = c_rid[r];
      // the uncached rows of a key own the ranks behind its cached rows: they take them from the END of the key's id
      // range downwards, decrementing a cursor that starts at the next slot's first position (for the last slot:
      // s_end) — after a barrier: the publish and the cached rows above still needed those words intact
      JL_BUILD_BARRIER();
      for (unsigned i0 = lo + static_cast<unsigned>(kJlCached) * kJlBuildThreads; i0 < hi; i0 += 4 * static_cast<unsigned>(kJlBuildThreads)) {
        u32x2 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned i = i0 + static_cast<unsigned>(q) * kJlBuildThreads + tid;
          row[q] = i < hi ? jl_row(pkeys, prids, i) : u32x2{kEmptyKey, 0u};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned key = row[q].x;
          unsigned s = kJlSubSlots;
          if (key != kEmptyKey) {  // (a missing row reads as the sentinel key)
            s = jl_home_slot(fmix32(key));
            for (unsigned tries = 0; tries < kJlSubSlots && lk[s] != key; ++tries) s = jl_next_slot(s);
            if (lk[s] != key) s = kJlSubSlots;
          }
          const bool live = s < kJlSubSlots;
          unsigned *cursor = live && s + 1 < kJlSubSlots ? &lp[s + 1] : &s_end;
          const unsigned at = jl_take<false>(cursor, s, live);
          if (live) ids[at] = row[q].y;
        }
      }
    }
    if (npart >= parts) break;
    JL_BUILD_BARRIER();  // the LDS arrays and s_wsum are reused by the next partition
    part = npart;
    npart = static_cast<unsigned>(gridDim.x) + s_ticket;
    lo = nlo;
    hi = nhi;
#pragma unroll
    for (int r = 0; r < kJlPre; ++r) carry[r] = nxt[r];
  }
  // every ticket this workgroup asked for has been answered (each was consumed above): the last workgroup to leave
  // resets the two words, so a launch finds them zero without a fill in front of it
  if (tid == 0 && atomicAdd(left_word, 1u) + 1u == gridDim.x) {
    __hip_atomic_store(ticket_word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(left_word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- giant partitions: all workgroups together, slice by slice ----------------------------------------------------
// jl_build_kernel leaves a partition above giants.rows rows out (an empty sub-table in its place) and lists it.  Such a
// partition is a few hot keys — any number of rows, still at most kJlSubSlots distinct keys — and one workgroup walks
// 0.38 G rows/s.  Two launches over slices of kJlSlice rows of the listed partitions:
//   jl_giant_count  a slice's rows are counted per key in an LDS sub-table (as the build does); every distinct key of the
//                   slice then claims its slot of the partition's sub-table IN HBM (atomicCAS on the empty slots the build
//                   published; same home slot, same linear probing: the probe kernel reads it like any other sub-table)
//                   and adds the slice's count to that slot's counter — one memory-side atomic per slice and key, not per
//                   row.  The workgroup that finishes a giant's LAST slice (a counter per giant) scans the slot counters:
//                   first id position of every slot -> the table's position words and the slot cursors.
//   jl_giant_ids    the slices are counted again the same way; per distinct key ONE returning add on the slot's cursor
//                   reserves the slice's share of the key's id range, then every row takes its place inside the share
//                   from an LDS cursor and stores its row id.
// Lanes of a wave that meet on one LDS counter (that is what a hot key is) are added by one lane: jl_take.
// Nothing here waits for another workgroup.
constexpr unsigned kJlSlice = 8192;        // rows of a slice: 16 per thread
constexpr int kJlGiantThreads = 512;
// jl_giant_ids_kernel calls jl_spill_partition, whose loops stride by kJlBuildThreads: with narrower giant workgroups
// they would skip rows, with wider ones walk rows twice
static_assert(kJlGiantThreads == kJlBuildThreads,
              "jl_spill_partition runs in build (kJlBuildThreads) and giant (kJlGiantThreads) workgroups: they must be equally wide");
// the slices of the listed giants as one flat list: s_first[g] = index of giant g's first slice (s_first[ng] = total)
__device__ __forceinline__ unsigned jl_giant_slices(const JlGiants &giants, const unsigned long long *__restrict__ starts,
                                                    unsigned *s_first, unsigned *s_wsum, unsigned *ng_out) {
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (giants.max == 0) {  // (uniform) DBHIP_JL_NO_GIANTS=1: no list, this launch only serves the spilled partitions
    *ng_out = 0;
    return 0u;
  }
  unsigned ng = *giants.count();
  ng = ng < giants.max ? ng : giants.max;
  ng = ng < kJlMaxGiantList - 1 ? ng : kJlMaxGiantList - 1;
  *ng_out = ng;
  if (ng == 0) return 0u;
  unsigned total = 0;
  for (unsigned g0 = 0; g0 < ng; g0 += kJlGiantThreads) {  // (uniform trip count)
    const unsigned g = g0 + tid;
    unsigned mine = 0;
    if (g < ng) {
      const unsigned p = giants.part()[g];
      mine = static_cast<unsigned>((starts[p + 1] - starts[p] + kJlSlice - 1) / kJlSlice);
    }
    const unsigned incl = wave_inclusive_scan(mine);
    if (lane == kWave - 1) s_wsum[wave] = incl;
    __syncthreads();
    unsigned before = total;
    for (unsigned w = 0; w < wave; ++w) before += s_wsum[w];
    if (g < ng) s_first[g] = before + incl - mine;
    for (unsigned w = 0; w < kJlGiantThreads / kWave; ++w) total += s_wsum[w];
    __syncthreads();
  }
  if (tid == 0) s_first[ng] = total;
  __syncthreads();
  return total;
}
// giant of flat slice `item` (largest g with s_first[g] <= item)
__device__ __forceinline__ unsigned jl_giant_of(const unsigned *s_first, unsigned ng, unsigned item) {
  unsigned lo = 0, hi = ng;
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) / 2;
    if (s_first[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}
// count the rows [a, b) per key in the LDS sub-table lk / lc (cleared here)
__device__ __forceinline__ void jl_slice_count(const u32x2 *__restrict__ rows, size_t a, size_t b, unsigned *lk, unsigned *lc,
                                               unsigned *status, unsigned *full) {
  const unsigned tid = threadIdx.x;
  for (unsigned i = tid; i < kJlSubSlots; i += kJlGiantThreads) {
    lk[i] = kEmptyKey;
    lc[i] = 0;
  }
  __syncthreads();
  for (size_t i0 = a; i0 < b; i0 += 4 * static_cast<size_t>(kJlGiantThreads)) {  // (uniform) four rows per lane in flight
    u32x2 r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const size_t i = i0 + static_cast<size_t>(q) * kJlGiantThreads + tid;
      r[q] = i < b ? rows[i] : u32x2{kEmptyKey, 0u};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool have = i0 + static_cast<size_t>(q) * kJlGiantThreads + tid < b;
      const unsigned sl = have ? jl_claim(lk, r[q].x, status, full) : kJlSubSlots;
      (void)jl_take<true>(&lc[sl < kJlSubSlots ? sl : 0u], sl, sl < kJlSubSlots);
    }
  }
  __syncthreads();
}
// slot of `key` in the giant's sub-table in HBM; claim = true: take the first empty slot of its chain if it is not there
// yet.  kJlSubSlots: the sub-table is full of other keys (*full is set: the giant goes to the spill path) / the key is
// not there.
__device__ __forceinline__ unsigned jl_giant_slot(u32x2 *sub, unsigned key, bool claim, unsigned *full) {
  unsigned s = jl_home_slot(fmix32(key));
  for (unsigned tries = 0; tries < kJlSubSlots; ++tries) {
    unsigned *kw = reinterpret_cast<unsigned *>(sub + s);
    unsigned k = __builtin_nontemporal_load(kw);
    if (k == kEmptyKey) {
      if (!claim) return kJlSubSlots;
      k = atomicCAS(kw, kEmptyKey, key);
      if (k == kEmptyKey) return s;
    }
    if (k == key) return s;
    s = jl_next_slot(s);
  }
  if (claim) *full = 1u;
  return kJlSubSlots;
}

__global__ __launch_bounds__(kJlGiantThreads) void jl_giant_count_kernel(const u32x2 *__restrict__ rows,
                                                                         const unsigned long long *__restrict__ starts,
                                                                         u32x2 *table, unsigned pos_bits, JlGiants giants,
                                                                         unsigned *status, JlSpill spill) {
  __shared__ unsigned lk[kJlSubSlots], lc[kJlSubSlots];
  __shared__ unsigned s_first[kJlMaxGiantList], s_wsum[kJlGiantThreads / kWave], s_last, s_full;
  const unsigned tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  unsigned ng;
  const unsigned items = jl_giant_slices(giants, starts, s_first, s_wsum, &ng);
  for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
    const unsigned g = jl_giant_of(s_first, ng, item);
    const unsigned part = giants.part()[g];
    const size_t lo = starts[part], hi = starts[part + 1];
    const size_t a = lo + static_cast<size_t>(item - s_first[g]) * kJlSlice;
    const size_t b = a + kJlSlice < hi ? a + kJlSlice : hi;
    if (tid == 0) s_full = 0;
    jl_slice_count(rows, a, b, lk, lc, status, &s_full);
    u32x2 *sub = giants.sub_table(table, g, part);
    unsigned *gcount = giants.counts(g);
    for (unsigned i = tid; i < kJlSubSlots && !s_full; i += kJlGiantThreads) {
      const unsigned c = lc[i];
      if (c) {
        const unsigned gs = jl_giant_slot(sub, lk[i], true, &s_full);
        if (gs < kJlSubSlots) {
          // (scope and order spelled out: a device-scope read-modify-write performed at the memory side; what orders it
          //  against the tick below is that the lane holds its answer before the barrier)
          const unsigned before = __hip_atomic_fetch_add(&gcount[gs], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          asm volatile("" ::"v"(before));  // the lane waits for the atomic's answer: the add has been performed
        }
      }
    }
    // The last slice of a giant to get here turns the slot counters into positions.  Counter adds, tick and the reads
    // below are all memory-side atomics, every lane has its adds' answers before the barrier, the tick comes after it:
    // no fence.  (With __threadfence() on either side of the tick — a write-back and an invalidation of the XCD's whole
    // L2 each — this kernel took 2.1 ms for 500 giants of 2^16 rows: 9 slices each, every one stalling its XCD twice.)
    __syncthreads();
    // more distinct keys than a sub-table has slots (in this slice, or in the giant as a whole): the giant goes to the spill
    // path, listed once — the directory word doubles as the guard; what the other slices still count is never read
    if (tid == 0 && s_full && atomicCAS(spill.area + 2 * static_cast<size_t>(part), 0u, 0xFFFFFFFFu) == 0u) jl_spill_list(spill, part, status);
    if (tid == 0)
      s_last = __hip_atomic_fetch_add(&giants.done()[g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == s_first[g + 1] - s_first[g] ? 1u : 0u;
    __syncthreads();
    if (s_last) {  // (uniform)
      constexpr unsigned kPer = kJlSubSlots / kJlGiantThreads;
      unsigned c[kPer], mine = 0;
#pragma unroll
      for (unsigned j = 0; j < kPer; ++j) {
        c[j] = __hip_atomic_fetch_add(&gcount[tid * kPer + j], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a read that no stale cache line can answer)
        mine += c[j];
      }
      const unsigned incl = wave_inclusive_scan(mine);
      if (lane == kWave - 1) s_wsum[wave] = incl;
      __syncthreads();
      unsigned run = static_cast<unsigned>(lo) + incl - mine;
      for (unsigned w = 0; w < wave; ++w) run += s_wsum[w];
      const unsigned cnt_esc = pos_bits < 32 ? (1u << (32 - pos_bits)) - 1u : 0u;
      unsigned *cursor = giants.cursors(g);
#pragma unroll
      for (unsigned j = 0; j < kPer; ++j) {
        const unsigned slot = tid * kPer + j;
        unsigned f = c[j] ? c[j] - 1 : 0u;
        f = f < cnt_esc ? f : cnt_esc;
        cursor[slot] = run;
        reinterpret_cast<unsigned *>(sub + slot)[1] = pos_bits < 32 ? (run | (f << pos_bits)) : run;
        run += c[j];
      }
      if (giants.with_tables && tid == kJlGiantThreads - 1) sub[kJlSubSlots] = u32x2{kEmptyKey, run};  // the scratch table's sentinel
    }
    __syncthreads();  // lk / lc / s_wsum / s_last are reused by the next slice
  }
}

__device__ __forceinline__ void jl_probe_sub(unsigned key, unsigned h, const u32x2 *__restrict__ sub, unsigned pos_bits,
                                             unsigned pos_mask, unsigned cnt_esc, unsigned *pos_out, unsigned *cnt_out,
                                             unsigned *marked);
// (radix join, match.spairs != nullptr: the same launch then runs the listed partitions' PROBE rows against their scratch
//  sub-tables, in slices of kJlSlice rows over all workgroups — they need the tables' position words, which
//  jl_giant_count finished, not the ids; one 8-byte gather per row, a hot key's slot one cache line for everybody;
//  results at the row's place in the probe side's partition order, like the fused kernel's)
__global__ __launch_bounds__(kJlGiantThreads) void jl_giant_ids_kernel(const u32x2 *__restrict__ rows,
                                                                        const unsigned long long *__restrict__ starts,
                                                                        u32x2 *table, JlGiants giants,
                                                                        unsigned *__restrict__ ids, unsigned *status,
                                                                        JlMatchArgs match, unsigned pos_bits, JlSpill spill) {
  __shared__ unsigned lk[kJlSubSlots], lc[kJlSubSlots];
  __shared__ unsigned s_first[kJlMaxGiantList], s_wsum[kJlGiantThreads / kWave], s_full;
  const unsigned tid = threadIdx.x;
  unsigned ng;
  const unsigned items = jl_giant_slices(giants, starts, s_first, s_wsum, &ng);
  for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
    const unsigned g = jl_giant_of(s_first, ng, item);
    const unsigned part = giants.part()[g];
    const size_t lo = starts[part], hi = starts[part + 1];
    const size_t a = lo + static_cast<size_t>(item - s_first[g]) * kJlSlice;
    const size_t b = a + kJlSlice < hi ? a + kJlSlice : hi;
    if (spill.dir()[part].x != 0u) continue;  // (uniform) a giant that went to the spill path: built at the end of this kernel
    jl_slice_count(rows, a, b, lk, lc, status, &s_full);
    u32x2 *sub = giants.sub_table(table, g, part);
    unsigned *cursor = giants.cursors(g);
    // the slice's share of every key's id range: lc[i] becomes the first position of the share
    for (unsigned i = tid; i < kJlSubSlots; i += kJlGiantThreads) {
      const unsigned c = lc[i];
      if (c) {
        const unsigned gs = jl_giant_slot(sub, lk[i], false, &s_full);
        lc[i] = gs < kJlSubSlots ? atomicAdd(&cursor[gs], c) : 0xFFFFFFFFu;  // (not there: only behind a full table, flagged)
      }
    }
    __syncthreads();
    for (size_t i0 = a; i0 < b; i0 += 4 * static_cast<size_t>(kJlGiantThreads)) {  // (uniform)
      u32x2 r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t i = i0 + static_cast<size_t>(q) * kJlGiantThreads + tid;
        r[q] = i < b ? rows[i] : u32x2{kEmptyKey, 0u};
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned key = r[q].x;
        unsigned sl = kJlSubSlots;
        if (i0 + static_cast<size_t>(q) * kJlGiantThreads + tid < b && key != kEmptyKey) {
          unsigned t = jl_home_slot(fmix32(key));
          for (unsigned tries = 0; tries < kJlSubSlots; ++tries) {
            const unsigned k = lk[t];
            if (k == key) {
              sl = t;
              break;
            }
            if (k == kEmptyKey) break;
            t = jl_next_slot(t);
          }
        }
        const bool live = sl < kJlSubSlots;
        const unsigned pos = jl_take<true>(&lc[live ? sl : 0u], sl, live);
        if (live && pos - static_cast<unsigned>(lo) < static_cast<unsigned>(hi - lo)) ids[pos] = r[q].y;  // (outside: only behind a full table)
      }
    }
    __syncthreads();  // lk / lc are reused by the next slice
  }
  // the spilled partitions (listed by jl_build_kernel and jl_giant_count_kernel): one workgroup each
  {
    unsigned nsp = status[kJlHdrSpilled];
    nsp = nsp < spill.max_list ? nsp : spill.max_list;
    for (unsigned g = blockIdx.x; g < nsp; g += gridDim.x) {  // (uniform)
      const unsigned part = spill.list()[g];
      const size_t slo = match.spairs ? match.sstarts[part] : 0, shi = match.spairs ? match.sstarts[part + 1] : 0;
      jl_spill_partition(spill, rows, starts[part], starts[part + 1], part, ids, status, match, slo, shi,
                         table != nullptr ? table + static_cast<size_t>(part) * kJlSubSlots : nullptr, pos_bits);
    }
  }
  if (match.spairs == nullptr) return;
  __syncthreads();
  const unsigned pitems = jl_giant_slices(giants, match.sstarts, s_first, s_wsum, &ng);
  const unsigned pos_mask = pos_bits < 32 ? (1u << pos_bits) - 1u : 0xFFFFFFFFu;
  const unsigned cnt_esc = pos_bits < 32 ? (1u << (32 - pos_bits)) - 1u : 0u;
  for (unsigned item = blockIdx.x; item < pitems; item += gridDim.x) {
    const unsigned g = jl_giant_of(s_first, ng, item);
    const unsigned part = giants.part()[g];
    const size_t slo = match.sstarts[part], shi = match.sstarts[part + 1];
    const size_t a = slo + static_cast<size_t>(item - s_first[g]) * kJlSlice;
    const size_t b = a + kJlSlice < shi ? a + kJlSlice : shi;
    if (spill.dir()[part].x != 0u) continue;  // (uniform) spilled: its probe rows were answered by jl_spill_partition
    const u32x2 *sub = giants.scratch_table(g);
    for (size_t j = a + tid; j < b; j += kJlGiantThreads) {
      const u32x2 row = match.spairs[j];
      unsigned pos, cnt;
      unsigned marked = 0;
      jl_probe_sub(row.x, fmix32(row.x), sub, pos_bits, pos_mask, cnt_esc, &pos, &cnt, &marked);
      match.out_rid[j] = row.y;
      match.out_pos[j] = pos;
      match.out_cnt[j] = cnt;
    }
  }
}

// one probe row: slot {key, first position | count field} by linear probing inside the key's sub-table.
// *marked |= the count field of the EMPTY slot a miss ended on: zero in every sub-table the build kernels publish
// normally, non-zero in the sub-table of a partition whose keys live in the spill pool (jl_spill_partition) — the probe
// learns that from the slot it reads anyway (a flag word in the workspace header, read once per wave, made the same
// loop 7-11 % slower: 1557 -> 1670-1730 us at 2^26 rows on the same box, the branch never taken).
__device__ __forceinline__ void jl_probe_sub(unsigned key, unsigned h, const u32x2 *__restrict__ sub, unsigned pos_bits,
                                             unsigned pos_mask, unsigned cnt_esc, unsigned *pos_out, unsigned *cnt_out,
                                             unsigned *marked);
__device__ __forceinline__ void jl_probe_row(unsigned key, const u32x2 *__restrict__ table, unsigned parts, unsigned pos_bits,
                                             unsigned pos_mask, unsigned cnt_esc, unsigned *pos_out, unsigned *cnt_out,
                                             unsigned *marked) {
  const unsigned h = fmix32(key);
  jl_probe_sub(key, h, table + static_cast<size_t>((static_cast<unsigned long long>(h) * parts) >> 32) * kJlSubSlots, pos_bits,
               pos_mask, cnt_esc, pos_out, cnt_out, marked);
}
// the same inside a given sub-table (h = fmix32(key))
__device__ __forceinline__ void jl_probe_sub(unsigned key, unsigned h, const u32x2 *__restrict__ sub, unsigned pos_bits,
                                             unsigned pos_mask, unsigned cnt_esc, unsigned *pos_out, unsigned *cnt_out,
                                             unsigned *marked) {
  unsigned s = jl_home_slot(h), pos = 0, cnt = 0;
  for (unsigned tries = 0; tries < kJlSubSlots && key != kEmptyKey; ++tries) {  // the sentinel never matches
    const u32x2 e = sub[s];
    if (e.x == key) {
      pos = e.y & pos_mask;
      const unsigned field = pos_bits < 32 ? e.y >> pos_bits : 0u;
      // s + 1 may be the first slot of the next sub-table (or the sentinel): positions run on across them
      cnt = field < cnt_esc ? field + 1u : (sub[s + 1].y & pos_mask) - pos;
      break;
    }
    if (e.x == kEmptyKey) {
      *marked |= pos_bits < 32 ? e.y >> pos_bits : 0u;
      break;
    }
    s = jl_next_slot(s);
  }
  *pos_out = pos;
  *cnt_out = cnt;
}

__global__ __launch_bounds__(kJlThreads) void jl_probe_kernel(const unsigned *__restrict__ probe, size_t n,
                                                              const u32x2 *__restrict__ table, unsigned parts,
                                                              unsigned pos_bits, unsigned *__restrict__ out_pos,
                                                              unsigned *__restrict__ out_cnt, JlSpill spill) {
  // The probe is pure memory latency: one random 8-byte gather per row = the slot {key, first position | count
  // field}; the right-hand neighbour is read only when the field holds the escape value.  (The first layout read
  // slot and neighbour with one 16-byte load at 8-byte alignment: every eighth row crossed a 64-byte line, i.e. one
  // more memory request.  A variant with FOUR consecutive rows per lane — one 16-byte key load, four gathers in flight,
  // one 16-byte store per output column — measured SLOWER, 1852 vs 1434 us at 2^26 rows: the random-access path
  // saturates sooner; removed in round 4.)
  const unsigned pos_mask = pos_bits < 32 ? (1u << pos_bits) - 1u : 0xFFFFFFFFu;
  const unsigned cnt_esc = pos_bits < 32 ? (1u << (32 - pos_bits)) - 1u : 0u;
  const size_t stride = static_cast<size_t>(gridDim.x) * kJlThreads;
  unsigned marked = 0;  // some row of this thread ended on an empty slot of a spilled partition's sub-table
  for (size_t i = static_cast<size_t>(blockIdx.x) * kJlThreads + threadIdx.x; i < n; i += stride)
    jl_probe_row(probe[i], table, parts, pos_bits, pos_mask, cnt_esc, out_pos + i, out_cnt + i, &marked);
  // Spilled partitions (never on hashed keys): a sub-table whose EMPTY slots carry a non-zero count field belongs to a
  // partition whose keys are in the spill pool; a thread that met one goes over ITS rows again and answers those of
  // spilled partitions from the pool (a hit cannot happen in such a sub-table: it holds no keys)
  if (marked == 0u) return;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kJlThreads + threadIdx.x; i < n; i += stride) {
    const unsigned key = probe[i];
    const u32x2 d = spill.dir()[jl_pid(key, parts)];
    if (d.x == 0u) continue;
    unsigned p, c;
    jl_spill_lookup(spill, d.x - 1u, d.y, key, &p, &c);
    out_pos[i] = p;
    out_cnt[i] = c;
  }
}

// ---- unique-key payload join (dwarf 4b, join/join.cpp:60-131) over the same partitions -----------------------
// One workgroup per partition: ds_cmpst claims the key's slot, the claimer stores its payload next to it (a
// duplicate build key keeps the first claimer's payload: keys are unique by contract, join/join.cpp:13-16), the
// sub-table goes out as 8-byte slots {key, payload}.  Probe: one 8-byte gather per step.
// A partition of more than kJlSubSlots (unique) keys — keys constructed against the hash — goes to the spill pool as well
// (round 4): the workgroup builds an open-addressing {key -> payload} table for it there (jl_spill_partition's pool and
// directory; the position array holds the payloads), and publishes the sub-table as an empty one whose slots carry
// payload 0 instead of the sentinel: the mark the probe looks for on a miss.
__device__ __noinline__ void jl_uspill_partition(const JlSpill sp, const u32x2 *__restrict__ rows, size_t lo, size_t hi, unsigned part,
                                                 unsigned *status) {
  constexpr unsigned kT = kJlBuildThreads;
  __shared__ unsigned s_base;
  const unsigned tid = threadIdx.x;
  const unsigned cap = static_cast<unsigned>(jl_spill_cap(hi - lo));
  __syncthreads();
  if (tid == 0) s_base = atomicAdd(status + kJlHdrSpillPool, cap);
  __syncthreads();
  const unsigned base = s_base;
  if (static_cast<unsigned long long>(base) + cap > sp.pool) {  // (cannot happen: the pool holds every partition that can spill)
    if (tid == 0) atomicOr(status, DBHIP_DEV_TABLE_FULL);
    return;
  }
  unsigned *keys = sp.keys() + base, *vals = sp.pos() + base;
  for (unsigned i = tid; i < cap; i += kT) keys[i] = kEmptyKey;
  __threadfence();
  __syncthreads();
  for (size_t i = lo + tid; i < hi; i += kT) {
    const u32x2 row = rows[i];
    if (row.x == kEmptyKey) {
      atomicOr(status, DBHIP_DEV_KEY_RANGE);
      continue;
    }
    unsigned sl = jl_spill_home(row.x, cap);
    while (true) {  // (cap > rows: an empty slot exists)
      const unsigned k = atomicCAS(&keys[sl], kEmptyKey, row.x);
      if (k == kEmptyKey) {  // the claimer's payload stays (a duplicate build key keeps the first claimer's: join.cpp:13-16)
        __hip_atomic_store(&vals[sl], row.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (k == row.x) break;
      sl = sl + 1 == cap ? 0u : sl + 1;
    }
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) sp.dir()[part] = u32x2{base + 1u, cap};
}

__global__ __launch_bounds__(kJlBuildThreads) void jl_ubuild_kernel(const unsigned *__restrict__ pkeys,
                                                                    const unsigned *__restrict__ prids,
                                                                    const unsigned long long *__restrict__ starts,
                                                                    u32x2 *__restrict__ table, unsigned *status, JlSpill spill) {
  __shared__ unsigned lk[kJlSubSlots];
  __shared__ unsigned lv[kJlSubSlots];
  __shared__ unsigned s_full;
  const unsigned tid = threadIdx.x;
  const size_t part = blockIdx.x;
  const size_t lo = starts[part], hi = starts[part + 1];
  for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) {
    lk[i] = kEmptyKey;
    lv[i] = kEmptyKey;
  }
  if (tid == 0) {
    s_full = 0;
    spill.dir()[part] = u32x2{0u, 0u};  // "not spilled"
  }
  __syncthreads();
  for (size_t i = lo + tid; i < hi; i += kJlBuildThreads) {
    const u32x2 row = jl_row(pkeys, prids, i);
    const unsigned key = row.x;
    unsigned s = jl_home_slot(fmix32(key));
    if (key == kEmptyKey) {  // the sentinel is not a key: flag it, drop the row
      atomicOr(status, DBHIP_DEV_KEY_RANGE);
      continue;
    }
    for (unsigned tries = 0;; ++tries) {
      const unsigned old = atomicCAS(&lk[s], kEmptyKey, key);
      if (old == kEmptyKey) {
        lv[s] = row.y;
        break;
      }
      if (old == key) break;
      s = jl_next_slot(s);
      if (tries + 1 >= kJlSubSlots) {  // more keys than slots: the partition goes to the spill pool
        s_full = 1u;
        break;
      }
    }
  }
  __syncthreads();
  u32x2 *dst = table + part * kJlSubSlots;
  if (s_full) {  // (uniform)
    jl_uspill_partition(spill, reinterpret_cast<const u32x2 *>(pkeys), lo, hi, static_cast<unsigned>(part), status);
    for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) __builtin_nontemporal_store(u32x2{kEmptyKey, 0u}, dst + i);
    return;
  }
  for (unsigned i = tid; i < kJlSubSlots; i += kJlBuildThreads) __builtin_nontemporal_store(u32x2{lk[i], lv[i]}, dst + i);
}

__global__ __launch_bounds__(kJlThreads) void jl_uprobe_kernel(const unsigned *__restrict__ pkeys,
                                                               const unsigned *__restrict__ pvals, size_t n,
                                                               const u32x2 *__restrict__ table, unsigned parts,
                                                               unsigned *__restrict__ out_key,
                                                               unsigned *__restrict__ out_bval,
                                                               unsigned *__restrict__ out_pval, JlSpill spill) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kJlThreads;
  unsigned marked = 0;  // a miss of this thread ended on an empty slot of a spilled partition's sub-table (payload 0, not the sentinel)
  for (size_t i = static_cast<size_t>(blockIdx.x) * kJlThreads + threadIdx.x; i < n; i += stride) {
    const unsigned key = pkeys[i];
    const unsigned h = fmix32(key);
    const u32x2 *sub = table + static_cast<size_t>((static_cast<unsigned long long>(h) * parts) >> 32) * kJlSubSlots;
    unsigned s = jl_home_slot(h), bval = kEmptyKey;
    bool found = false;
    for (unsigned tries = 0; tries < kJlSubSlots && key != kEmptyKey; ++tries) {
      const u32x2 e = sub[s];
      if (e.x == key) {
        found = true;
        bval = e.y;
        break;
      }
      if (e.x == kEmptyKey) {
        marked |= e.y != kEmptyKey ? 1u : 0u;
        break;
      }
      s = jl_next_slot(s);
    }
    // join.cpp:41-43, :96-101: sentinels where the probe row has no partner
    out_key[i] = found ? key : kEmptyKey;
    out_bval[i] = bval;
    out_pval[i] = found ? pvals[i] : kEmptyKey;
  }
  if (marked == 0u) return;
  // a thread that met a spilled partition goes over ITS rows again and answers those of spilled partitions from the pool
  for (size_t i = static_cast<size_t>(blockIdx.x) * kJlThreads + threadIdx.x; i < n; i += stride) {
    const unsigned key = pkeys[i];
    if (key == kEmptyKey) continue;
    const u32x2 d = spill.dir()[jl_pid(key, parts)];
    if (d.x == 0u) continue;
    const unsigned base = d.x - 1u, cap = d.y;
    unsigned sl = jl_spill_home(key, cap);
    for (unsigned tries = 0; tries < cap; ++tries) {
      const unsigned k = spill.keys()[base + sl];
      if (k == key) {
        out_key[i] = key;
        out_bval[i] = spill.pos()[base + sl];
        out_pval[i] = pvals[i];
        break;
      }
      if (k == kEmptyKey) break;
      sl = sl + 1 == cap ? 0u : sl + 1;
    }
  }
}

// ---- host side (called from join.hip's entry points) ---------------------------------------------------
struct JlPartitioned {
  const unsigned *pairs;                   // partition-major (key, row id) pairs
  const unsigned long long *starts;        // parts + 1 offsets
  u32x2 *table;
  unsigned *status;
};
// the build side of the one-to-many / unique-key joins, laid out by jl_layout(n): fills `out`
int jl_partition_rows(const unsigned *build_keys, const unsigned *row_ids, size_t n, void *workspace, hipStream_t s,
                      const DeviceInfo &dev, const JlLayout &L, JlPartitioned *out) {
  char *base = static_cast<char *>(workspace);
  const hipError_t e = fill_async(base, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  out->table = reinterpret_cast<u32x2 *>(base + L.table_off);
  out->status = reinterpret_cast<unsigned *>(base);
  return jl_partition_side(build_keys, row_ids, n, L, reinterpret_cast<u32x2 *>(base + L.pairs_a_off),
                           reinterpret_cast<u32x2 *>(base + L.pairs_b_off),
                           reinterpret_cast<unsigned long long *>(base + L.meta_off), s, dev, &out->pairs, &out->starts);
}

size_t jl_build_lds_bytes() { return 2 * static_cast<size_t>(kJlSubSlots) * sizeof(unsigned); }
bool jl_no_giants() {  // DBHIP_JL_NO_GIANTS=1: every partition through the per-partition kernel, whatever its size (A/B timing)
  static const bool off = [] { const char *v = getenv("DBHIP_JL_NO_GIANTS"); return v && v[0] == '1'; }();
  return off;
}

// The launches behind the partition step, for the one-to-many build (kMatch = false: sub-tables published to `table`)
// and the radix join's fused build + probe (kMatch = true): the build kernel over every partition by ticket, then — from
// the size where giant partitions are looked for (max_giants != 0, join_common.hpp) — jl_giant_count / jl_giant_ids,
// which all workgroups share and whose tail builds the spilled partitions the build kernel listed; below that size the
// build kernel's workgroup builds a spilled partition itself, at once.  `pairs`, `starts`: the partitioned build side.
template <bool kMatch>
int jl_launch_build(const unsigned *pairs, const unsigned long long *starts, u32x2 *table, unsigned parts, size_t n_build,
                    size_t n_probe, unsigned max_giants, void *giant_area, void *spill_area, unsigned *ids, unsigned *status,
                    const JlMatchArgs &match, hipStream_t s, const DeviceInfo &dev) {
  const size_t build_lds = jl_build_lds_bytes();
  const void *listing = reinterpret_cast<const void *>(jl_build_kernel<kMatch, false>);
  const void *inlined = reinterpret_cast<const void *>(jl_build_kernel<kMatch, true>);
  hipError_t e = hipFuncSetAttribute(listing, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(build_lds));
  if (e == hipSuccess && (kMatch || !max_giants))
    e = hipFuncSetAttribute(inlined, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(build_lds));
  if (e != hipSuccess) return static_cast<int>(e);
  // giant partitions — radix join: a giant build OR probe side — are left out by the build kernel, listed, then counted
  // and filled (radix join: into scratch sub-tables, and probed) by the two launches of their own
  JlGiants giants{nullptr, 0u, ~0ull, ~0ull, 0u};
  if (max_giants && !jl_no_giants()) {
    giants.base = static_cast<unsigned *>(giant_area);
    giants.max = max_giants;
    giants.rows = jl_giant_rows(n_build);
    if (kMatch) giants.probe_rows = jl_giant_rows(n_probe);
    giants.with_tables = kMatch ? 1u : 0u;
    e = fill_async(giants.base, 0, jl_giant_header_bytes(max_giants), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (kMatch) {
    // the spilled-partition list and the pool cursor belong to this match, not to the partitioned sides: a second match
    // on the same sides would list every spilled partition again (two workgroups building one table) and allocate on
    // from the pool.  (The spill directory needs no clear: the build kernel writes every partition's entry.)
    static_assert(kJlHdrSpillPool == kJlHdrSpilled + 1, "header words 34 and 35 are cleared together");
    e = fill_async(status + kJlHdrSpilled, 0, 2 * sizeof(unsigned), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  const JlSpill spill = jl_spill_of(spill_area, parts, n_build);
  const unsigned pos_bits = jl_pos_bits(n_build);
  const unsigned *no_rids = nullptr;  // (the kernels' row-id column parameter: both scatter levels write pairs)
  // as many workgroups as are RESIDENT (DBHIP_JL_BUILD_WGS / DBHIP_JL_MATCH_WGS: experiments)
  const size_t cap = static_cast<size_t>(dev.cus) * jl_resident_per_cu(listing, kJlBuildThreads, build_lds,
                                                                       kMatch ? "DBHIP_JL_MATCH_WGS" : "DBHIP_JL_BUILD_WGS", 3u);
  const unsigned build_grid = static_cast<unsigned>(parts < cap ? parts : cap);
  if (max_giants) {
    hipLaunchKernelGGL((jl_build_kernel<kMatch, false>), dim3(build_grid), dim3(kJlBuildThreads), build_lds, s, pairs, no_rids,
                       starts, table, parts, static_cast<unsigned>(n_build), pos_bits, ids, status, match, giants, spill.area);
    const unsigned grid = static_cast<unsigned>(dev.cus) * (2048 / kJlGiantThreads);
    if (giants.max)
      hipLaunchKernelGGL(jl_giant_count_kernel, dim3(grid), dim3(kJlGiantThreads), 0, s, reinterpret_cast<const u32x2 *>(pairs),
                         starts, table, pos_bits, giants, status, spill);
    hipLaunchKernelGGL(jl_giant_ids_kernel, dim3(grid), dim3(kJlGiantThreads), 0, s, reinterpret_cast<const u32x2 *>(pairs),
                       starts, table, giants, ids, status, match, pos_bits, spill);
  } else {
    hipLaunchKernelGGL((jl_build_kernel<kMatch, true>), dim3(build_grid), dim3(kJlBuildThreads), build_lds, s, pairs, no_rids,
                       starts, table, parts, static_cast<unsigned>(n_build), pos_bits, ids, status, match, giants, spill.area);
  }
  return launch_status();
}
}  // namespace

int join_lds_build(const unsigned *build_keys, const unsigned *row_ids, size_t n, unsigned *ids, void *workspace,
                   hipStream_t s, const DeviceInfo &dev) {
  const JlLayout L = jl_layout(n);
  JlPartitioned p;
  const int rc = jl_partition_rows(build_keys, row_ids, n, workspace, s, dev, L, &p);
  if (rc != 0) return rc;
  char *base = static_cast<char *>(workspace);
  const JlMatchArgs no_match{nullptr, nullptr, nullptr, nullptr, nullptr};
  return jl_launch_build<false>(p.pairs, p.starts, p.table, L.parts, n, 0, L.max_giants, base + L.giant_off, base + L.spill_off,
                                ids, p.status, no_match, s, dev);
}

// ---- radix join: both sides partitioned with the build side's geometry, one fused build + probe launch -----------
// workspace: header | build side: pairs a, pairs b, meta | probe side: pairs a, pairs b, meta
namespace {
struct JrLayout : JlGeometry {
  unsigned max_giants;
  size_t b_a, b_b, b_meta, p_a, p_b, p_meta, giant_off, spill_off, total;
};
JrLayout jr_layout(size_t n_build, size_t n_probe) {
  JrLayout L;
  static_cast<JlGeometry &>(L) = jl_geometry(n_build, kJrRowsPerPart);
  const size_t cb = align_up((n_build ? n_build : 1) * 8, kWsAlign), cp = align_up((n_probe ? n_probe : 1) * 8, kWsAlign);
  const size_t mb = align_up(jl_meta(L).bytes(), kWsAlign);
  L.b_a = kWsHeader;
  L.b_b = L.b_a + cb;
  L.b_meta = L.b_b + (L.k2 > 1 ? cb : 0);
  L.p_a = L.b_meta + mb;
  L.p_b = L.p_a + cp;
  L.p_meta = L.p_b + (L.k2 > 1 ? cp : 0);
  L.max_giants = jr_max_giants(n_build, n_probe);
  L.giant_off = L.p_meta + mb;
  L.spill_off = align_up(L.giant_off + jl_giant_bytes(L.max_giants, true), kWsAlign);
  L.total = L.spill_off + jl_spill_bytes(L.parts, n_build);
  return L;
}
// where a partitioned side ended up is a pure function of the sizes: no state is kept between the calls
void jr_side(const JrLayout &L, char *base, bool probe, const unsigned **pairs, const unsigned long long **starts) {
  const size_t a = probe ? L.p_a : L.b_a, b = probe ? L.p_b : L.b_b, m = probe ? L.p_meta : L.b_meta;
  *pairs = reinterpret_cast<const unsigned *>(base + (L.k2 > 1 ? b : a));
  *starts = reinterpret_cast<const unsigned long long *>(base + m) + jl_meta_starts(L);
}
}  // namespace

size_t join_radix_workspace_bytes(size_t n_build, size_t n_probe) { return jr_layout(n_build, n_probe).total; }

// jl_build_kernel<true, ...> walks a partition's probe rows with 32-bit indices: j0 < shi <= n_probe, then
// j0 += 4 * kJlBuildThreads, which must not wrap past 2^32 - 1
size_t jr_max_probe_rows() { return (static_cast<size_t>(1) << 32) - 4 * static_cast<size_t>(kJlBuildThreads); }

int join_radix_partition(int probe_side, const unsigned *keys, const unsigned *row_ids, size_t n, size_t n_build,
                         size_t n_probe, void *workspace, hipStream_t s, const DeviceInfo &dev) {
  const JrLayout L = jr_layout(n_build, n_probe);
  char *base = static_cast<char *>(workspace);
  if (!probe_side) {  // the build side's call opens a join: it clears the status word
    const hipError_t e = fill_async(base, 0, kWsHeader, s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  const unsigned *pairs;
  const unsigned long long *starts;
  return jl_partition_side(keys, row_ids, n, L, reinterpret_cast<u32x2 *>(base + (probe_side ? L.p_a : L.b_a)),
                           reinterpret_cast<u32x2 *>(base + (probe_side ? L.p_b : L.b_b)),
                           reinterpret_cast<unsigned long long *>(base + (probe_side ? L.p_meta : L.b_meta)), s, dev, &pairs,
                           &starts);
}

int join_radix_match(size_t n_build, size_t n_probe, unsigned *ids, unsigned *out_rid, unsigned *out_pos, unsigned *out_cnt,
                     void *workspace, hipStream_t s, const DeviceInfo &dev) {
  const JrLayout L = jr_layout(n_build, n_probe);
  char *base = static_cast<char *>(workspace);
  const unsigned *bp, *pp;
  const unsigned long long *bs, *ps;
  jr_side(L, base, false, &bp, &bs);
  jr_side(L, base, true, &pp, &ps);
  const JlMatchArgs match{reinterpret_cast<const u32x2 *>(pp), ps, out_rid, out_pos, out_cnt};
  // (no table is published: the giants' sub-tables live in their scratch)
  return jl_launch_build<true>(bp, bs, static_cast<u32x2 *>(nullptr), L.parts, n_build, n_probe, L.max_giants, base + L.giant_off,
                               base + L.spill_off, ids, reinterpret_cast<unsigned *>(base), match, s, dev);
}

// unique-key payload join: `build_vals` ride through the partition in the row-id column
int ujoin_lds_build(const unsigned *build_keys, const unsigned *build_vals, size_t n, void *workspace, hipStream_t s,
                    const DeviceInfo &dev) {
  const JlLayout L = jl_layout(n);
  JlPartitioned p;
  const int rc = jl_partition_rows(build_keys, build_vals, n, workspace, s, dev, L, &p);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(jl_ubuild_kernel, dim3(L.parts), dim3(kJlBuildThreads), 0, s, p.pairs, static_cast<const unsigned *>(nullptr),
                     p.starts, p.table, p.status, jl_spill_of(static_cast<char *>(workspace) + L.spill_off, L.parts, n));
  return launch_status();
}

int ujoin_lds_probe(const unsigned *probe_keys, const unsigned *probe_vals, size_t n_probe, const void *workspace,
                    size_t n_build, unsigned *out_key, unsigned *out_bval, unsigned *out_pval, hipStream_t s,
                    const DeviceInfo &dev) {
  const JlLayout L = jl_layout(n_build);
  const u32x2 *table = reinterpret_cast<const u32x2 *>(static_cast<const char *>(workspace) + L.table_off);
  const int uprobe_wgs = static_cast<int>(jl_resident_per_cu(reinterpret_cast<const void *>(jl_uprobe_kernel), kJlThreads, 0,
                                                             "DBHIP_JL_UPROBE_WGS", 4u));
  hipLaunchKernelGGL(jl_uprobe_kernel, dim3(jl_grid(n_probe, dev, uprobe_wgs)), dim3(kJlThreads), 0, s, probe_keys, probe_vals,
                     n_probe, table, L.parts, out_key, out_bval, out_pval,
                     jl_spill_of(const_cast<char *>(static_cast<const char *>(workspace)) + L.spill_off, L.parts, n_build));
  return launch_status();
}

int join_lds_probe(const unsigned *probe_keys, size_t n_probe, const void *workspace, size_t n_build,
                   unsigned *out_pos, unsigned *out_cnt, hipStream_t s, const DeviceInfo &dev) {
  const JlLayout L = jl_layout(n_build);
  const u32x2 *table = reinterpret_cast<const u32x2 *>(static_cast<const char *>(workspace) + L.table_off);
  // Exactly the workgroups that are resident (four of 512 threads per CU), every thread striding over its rows: with
  // eight per CU — two rounds of workgroups — the kernel's time depended on how the second round happened to fill in
  // (round 4, same box, 2^26 rows: 2 per CU 1767-1838 us, 4: 1553-1572, 6: 1692-1713, 8: 1566 for one build of this
  // kernel and 1708 for another whose loop was the same instructions; 16: 1566 / 1625).  DBHIP_JL_PROBE_WGS: experiments.
  const int wgs_per_cu = static_cast<int>(jl_resident_per_cu(reinterpret_cast<const void *>(jl_probe_kernel), kJlThreads, 0,
                                                             "DBHIP_JL_PROBE_WGS", 4u));
  char *ws = const_cast<char *>(static_cast<const char *>(workspace));
  hipLaunchKernelGGL(jl_probe_kernel, dim3(jl_grid(n_probe, dev, wgs_per_cu)), dim3(kJlThreads), 0, s, probe_keys, n_probe,
                     table, L.parts, jl_pos_bits(n_build), out_pos, out_cnt, jl_spill_of(ws + L.spill_off, L.parts, n_build));
  return launch_status();
}

}  // namespace dbhip
