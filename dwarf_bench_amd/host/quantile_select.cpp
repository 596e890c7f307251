// quantile_select.cpp — exact order statistics at up to 16 ranks by a multi-rank radix select on gfx950
// (quantile_select.hpp holds the contract, quantile_layout.hpp the digits, the rank formula and the bin test, which qs_pick
// below and the host check run as the same text).
//
// Three levels over the 11 / 11 / 10-bit digits of x = key ^ flip, each a histogram launch and a pick launch:
// qs_hist  a persistent grid of workgroups of eight waves (sixteen in the sixteen-slot form, which has its CU to itself)
//          walks rounds of 8192 (16384) positions, counted from the 16-byte boundary
//          in front of the column (or the list) as hll_build_kernel counts them: a lane holds four consecutive entries per
//          16-byte load and four such loads per round, all in flight; the ragged ends word by word (load_ragged); with a
//          list four gathers per load, an entry that does not count reading nothing.  Level 0 is the one-slot form with an
//          empty prefix.  From level 1 on a key belongs to the slot whose prefix its higher bits equal: with one slot one
//          compare, with more a 2048-entry LDS table on the top digit gives the mask of slots to compare against, so nearly
//          every key is rejected by one LDS read.  A wave with no key in any slot touches no histogram word, and a wave
//          whose keys all share one (slot, digit) adds once.  One slot keeps four copies of its bins in LDS (lane l adds
//          into copy l % 4), four slots one copy (32 KiB), sixteen slots one copy of 16 x 2048 words: 128 KiB of static
//          LDS, one workgroup to a CU.  A workgroup flushes once, its non-zero words alone, into one of the copies of the
//          level's global bins.
// qs_pick  one workgroup of sixteen waves per level, a wave per slot: the sum of the copies and a wave scan; per rank the
//          bin that holds it.  Thread 0 then writes the next level's slot table (at most 16 ranks: one thread dedupes the prefixes), or
//          the three output columns behind the last level.
#include "quantile_select.hpp"

#include "quantile_layout.hpp"
#include "rowlist.hpp"

namespace {
using namespace dbhip;

constexpr int kQsMaxRanks = DBENCH_QUANTILE_MAX_RANKS;
// threads of a histogram workgroup: eight waves, sixteen where one workgroup has the CU to itself (its LDS)
constexpr int qs_threads(int slots) { return slots == 16 ? 1024 : 512; }
constexpr int kQsLoads = 4;                                     // 16-byte loads in flight per lane
constexpr size_t qs_round(int slots) { return static_cast<size_t>(kQsLoads) * 4 * qs_threads(slots); }  // positions of a round
constexpr int kQsRadix = DBENCH_QUANTILE_RADIX;
constexpr int kQsPickThreads = 1024;
constexpr int kQsTopCopies = 8;                                 // copies of level 0's global bins
constexpr unsigned kQsNone = 0xFFFFFFFFu;                       // the histogram word of a key that is counted nowhere
static_assert(qs_round(1) == 8192 && qs_round(4) == 8192 && qs_round(16) == 16384, "rounds of 8192 and 16384 positions");
static_assert(kQsPickThreads / kWave == kQsMaxRanks, "qs_pick: a wave per slot");

// what the picks hand on, behind the workspace header: the slots of the level to come and every rank's place in them
struct QsTable {
  unsigned m;                            // valid candidates: the total of level 0's histogram
  unsigned n_slots;                      // distinct prefixes the live ranks have led to
  unsigned pad[14];
  unsigned slot_prefix[kQsMaxRanks];     // x with the digits found so far, the rest zero
  unsigned rank_slot[kQsMaxRanks];       // DBENCH_QUANTILE_NO_SLOT: the rank names no row
  unsigned rank_rem[kQsMaxRanks];        // the rank counted inside its slot
  unsigned rank_below[kQsMaxRanks];      // candidates in front of the slot
  unsigned pad2[128 - 16 - 4 * kQsMaxRanks];
};
static_assert(sizeof(QsTable) == 512, "slot table size");

struct QsRanks {
  unsigned num[kQsMaxRanks], den[kQsMaxRanks];
};

// slot capacity of the histogram kernel for n_q ranks (what the sixteen-slot kernel costs a single rank: tools/ab.py
// quantile measures it with sixteen equal ranks, which stay one slot)
int qs_slots(int n_q) { return n_q <= 1 ? 1 : (n_q <= 4 ? 4 : 16); }
// copies of the global bins of levels 1 and 2: the more slots, the fewer workgroups add to one word
int qs_copies(int slots) { return slots == 1 ? 8 : (slots == 4 ? 4 : 2); }

struct QsLayout {
  size_t table, bins[DBENCH_QUANTILE_LEVELS], total;
};
QsLayout qs_layout(int slots) {
  QsLayout l;
  l.table = kWsHeader;
  l.bins[0] = l.table + sizeof(QsTable);
  l.bins[1] = l.bins[0] + sizeof(unsigned) * kQsTopCopies * qs_radix(0);
  l.bins[2] = l.bins[1] + sizeof(unsigned) * qs_copies(slots) * slots * qs_radix(1);
  l.total = align_up(l.bins[2] + sizeof(unsigned) * qs_copies(slots) * slots * qs_radix(2), kWsAlign);
  return l;
}

// ---------------------------------------------------------------------------------------------
// hist: the candidates -> this level's counts per (slot, digit), added into one copy of the global bins
// ---------------------------------------------------------------------------------------------
// kList: `src` is the row-id list (gathered through into col), otherwise col itself.  entries at most; *count (nullable)
// lowers it on the device.  bins: `copies` copies of SLOTS x radix words
template <int SLOTS, bool kList>
__global__ __launch_bounds__(qs_threads(SLOTS)) void qs_hist(const unsigned *__restrict__ col, unsigned n_col,
                                                      const unsigned *__restrict__ src, size_t entries, const u64 *count,
                                                      unsigned a, unsigned flip, int level, const QsTable *tab,
                                                      unsigned *__restrict__ bins, int copies, unsigned *status,
                                                      size_t rounds) {
  constexpr int kQsThreads = qs_threads(SLOTS);
  constexpr size_t kQsLoadSpan = 4 * kQsThreads, kQsRound = qs_round(SLOTS);  // positions of one load, of a round
  constexpr int kCopies = SLOTS == 1 ? 4 : 1, kStride = SLOTS * kQsRadix + (SLOTS == 1 ? 1 : 0);
  __shared__ unsigned s_hist[kCopies * kStride];
  __shared__ unsigned s_mask[SLOTS == 1 ? 1 : kQsRadix];  // top digit -> the slots whose prefix starts with it
  __shared__ unsigned s_prefix[kQsMaxRanks];
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned n_slots = level == 0 ? 1u : tab->n_slots;  // <= SLOTS
  if (n_slots == 0) return;                                 // no rank names a row (uniform over the grid)
  const int shift = qs_shift(level);
  const unsigned radix = qs_radix(level), high_mask = qs_high_mask(level);
  const unsigned used = SLOTS == 1 ? static_cast<unsigned>(kCopies * kStride) : n_slots * radix;
  for (unsigned i = threadIdx.x; i < used; i += kQsThreads) s_hist[i] = 0;
  if (SLOTS > 1)
    for (unsigned i = threadIdx.x; i < kQsRadix; i += kQsThreads) s_mask[i] = 0;
  if (threadIdx.x < kQsMaxRanks) s_prefix[threadIdx.x] = (level != 0 && threadIdx.x < n_slots) ? tab->slot_prefix[threadIdx.x] : 0u;
  __syncthreads();
  if (SLOTS > 1 && threadIdx.x < n_slots)  // the result is not used: a no-return LDS or
    __hip_atomic_fetch_or(&s_mask[s_prefix[threadIdx.x] >> qs_shift(0)], 1u << threadIdx.x, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  const unsigned prefix0 = s_prefix[0];
  unsigned *hist = s_hist + (SLOTS == 1 ? (threadIdx.x & (kCopies - 1)) * kStride : 0);

  // the histogram word of a key, kQsNone for a key under no slot's prefix
  auto word_of = [&](unsigned key) -> unsigned {
    const unsigned x = key ^ flip;
    const unsigned d = (x >> shift) & (radix - 1u);
    if (SLOTS == 1) return ((x ^ prefix0) & high_mask) == 0 ? d : kQsNone;
    unsigned mk = s_mask[x >> qs_shift(0)], w = kQsNone;
    while (mk) {  // at most n_slots turns; prefixes are distinct: at most one matches
      const unsigned s = static_cast<unsigned>(__builtin_ctz(mk));
      mk &= mk - 1u;
      if (((x ^ s_prefix[s]) & high_mask) == 0) w = s * radix + d;
    }
    return w;
  };
  // four keys of the lane; bit q of ok: key q counts
  auto count4 = [&](const unsigned (&key)[4], unsigned ok) {
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = ((ok >> q) & 1u) ? word_of(key[q]) : kQsNone;
    const bool any = w[0] != kQsNone || w[1] != kQsNone || w[2] != kQsNone || w[3] != kQsNone;
    const unsigned long long active = __ballot(true);
    if (__ballot(any) == 0) return;  // no key of the wave under any slot
    // one word in the whole wave (all keys equal, the upper digits of keys in [1, 10000]): one lane adds the lot
    const unsigned first = __builtin_amdgcn_readfirstlane(w[0]);
    const bool same = w[0] == first && w[1] == first && w[2] == first && w[3] == first;
    if (first != kQsNone && __ballot(same) == active) {
      if (lane_id() == static_cast<unsigned>(__builtin_ctzll(active)))
        atomicAdd(&hist[first], 4u * static_cast<unsigned>(__builtin_popcountll(active)));
      return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (w[q] != kQsNone) atomicAdd(&hist[w[q]], 1u);
  };
  bool bad = false;
  // the lane's four entries e (bit q of valid: entry q exists) -> its four keys and the entries that count
  auto fetch = [&](const u32x4 e, unsigned valid, unsigned (&key)[4]) -> unsigned {
    const unsigned w[4] = {e.x, e.y, e.z, e.w};
    unsigned ok = valid;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (kList) {
        const bool inside = w[q] < n_col;
        bad = bad || (((valid >> q) & 1u) && !inside);
        if (!inside) ok &= ~(1u << q);
        key[q] = ((ok >> q) & 1u) ? col[w[q]] : 0u;
      } else {
        key[q] = w[q];
      }
    }
    return ok;
  };

  const size_t m = clamped_count(count, entries);
  const size_t vend = a + m;  // positions [a, vend) hold entries
#pragma unroll 1
  for (size_t round = blockIdx.x; round < rounds; round += gridDim.x) {  // uniform over the workgroup; no barrier inside
    const size_t vfirst = round * kQsRound;
    if (vfirst >= vend) break;  // this round and all behind it lie behind the last entry
    const size_t v0 = vfirst + 4 * static_cast<size_t>(threadIdx.x);
    if (vfirst >= a && vfirst + kQsRound <= vend) {  // a whole round: four aligned 16-byte loads per lane, all in flight
      const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (v0 - a));
      const u32x4 e0 = s4[0], e1 = s4[kQsThreads], e2 = s4[2 * kQsThreads], e3 = s4[3 * kQsThreads];
      unsigned k0[4], k1[4], k2[4], k3[4];
      const unsigned ok0 = fetch(e0, 0xfu, k0), ok1 = fetch(e1, 0xfu, k1), ok2 = fetch(e2, 0xfu, k2), ok3 = fetch(e3, 0xfu, k3);
      count4(k0, ok0);
      count4(k1, ok1);
      count4(k2, ok2);
      count4(k3, ok3);
    } else {  // the first round of an array that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
      for (int g = 0; g < kQsLoads; ++g) {
        unsigned valid, key[4];
        const u32x4 e = load_ragged(src, a, v0 + g * kQsLoadSpan, vend, valid);
        const unsigned ok = fetch(e, valid, key);
        count4(key, ok);
      }
    }
  }
  if (kList && level == 0 && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);

  __syncthreads();
  unsigned *copy = bins + static_cast<size_t>(blockIdx.x % copies) * (SLOTS * radix);
  for (unsigned i = threadIdx.x; i < n_slots * radix; i += kQsThreads) {
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < kCopies; ++q) c += s_hist[q * kStride + i];
    if (c) atomicAdd(&copy[i], c);  // the result is not used: a no-return global add
  }
}

// ---------------------------------------------------------------------------------------------
// pick: this level's bins -> every rank's bin, and the next level's slots (or the outputs)
// ---------------------------------------------------------------------------------------------
// bins: `copies` copies of slot_cap x radix words.  A wave takes a slot: a lane sums the copies of 32 neighbouring bins (16
// at the last level) with 16-byte loads, one wave scan gives every lane the candidates in front of its bins, and the lane
// whose bins hold a rank looks for the bin.  All slots are under way at once: a pick waits for one round of loads, not
// for one per slot
__global__ __launch_bounds__(kQsPickThreads) void qs_pick(QsTable *tab, const unsigned *__restrict__ bins, int copies,
                                                          int slot_cap, int level, const QsRanks ranks, int n_q, unsigned flip,
                                                          unsigned *out_values, unsigned *out_below, unsigned *out_equal) {
  constexpr int kLaneBins = kQsRadix / kWave;
  __shared__ unsigned s_prefix[kQsMaxRanks], s_slot[kQsMaxRanks], s_rem[kQsMaxRanks], s_below[kQsMaxRanks];
  __shared__ unsigned s_digit[kQsMaxRanks], s_before[kQsMaxRanks], s_count[kQsMaxRanks], s_next[kQsMaxRanks];
  __shared__ unsigned s_m;
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned radix = qs_radix(level), per = radix / kWave;  // bins of a lane
  const int shift = qs_shift(level);
  const unsigned n_slots = level == 0 ? 1u : tab->n_slots;
  if (threadIdx.x < kQsMaxRanks) {
    const unsigned j = threadIdx.x;
    const bool known = level != 0 && static_cast<int>(j) < n_q;
    s_prefix[j] = (level != 0 && j < n_slots) ? tab->slot_prefix[j] : 0u;
    s_slot[j] = known ? tab->rank_slot[j] : DBENCH_QUANTILE_NO_SLOT;  // level 0 decides below, once m is known
    s_rem[j] = known ? tab->rank_rem[j] : 0u;
    s_below[j] = known ? tab->rank_below[j] : 0u;
    s_digit[j] = s_before[j] = s_count[j] = 0u;
  }
  if (threadIdx.x == 0) s_m = level == 0 ? 0u : tab->m;
  __syncthreads();

#pragma unroll 1
  for (unsigned s = wave; s < n_slots; s += kQsPickThreads / kWave) {  // uniform over the wave
    const unsigned *mine = bins + static_cast<size_t>(s) * radix + lane * per;
    unsigned c[kLaneBins], sum = 0;
#pragma unroll
    for (int i = 0; i < kLaneBins; ++i) c[i] = 0;
    for (int q = 0; q < copies; ++q) {
      const u32x4 *v = reinterpret_cast<const u32x4 *>(mine + static_cast<size_t>(q) * slot_cap * radix);  // 64-byte aligned
#pragma unroll
      for (int i = 0; i < kLaneBins / 4; ++i) {
        if (4u * i < per) {
          const u32x4 t = v[i];
          c[4 * i] += t.x, c[4 * i + 1] += t.y, c[4 * i + 2] += t.z, c[4 * i + 3] += t.w;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kLaneBins; ++i) sum += c[i];
    const unsigned incl = wave_inclusive_scan(sum);
    const unsigned run = incl - sum, total = __builtin_amdgcn_readlane(incl, kWave - 1);
    for (int j = 0; j < n_q; ++j) {
      unsigned rem = s_rem[j];
      bool here = s_slot[j] == s;
      if (level == 0) {  // the slot's total is m: every (q_num, q_den) becomes its rank
        here = qs_resolve_rank(ranks.num[j], ranks.den[j], total, &rem);
        if (lane == 0) {
          s_slot[j] = here ? 0u : DBENCH_QUANTILE_NO_SLOT;
          s_rem[j] = rem;
        }
      }
      if (here && qs_bin_holds(run, sum, rem)) {  // exactly one lane of the slot's wave, and exactly one of its bins
        unsigned before = run;
#pragma unroll
        for (int i = 0; i < kLaneBins; ++i) {
          if (static_cast<unsigned>(i) < per && qs_bin_holds(before, c[i], rem)) {
            s_digit[j] = lane * per + i;
            s_before[j] = before;
            s_count[j] = c[i];
          }
          before += c[i];
        }
      }
    }
    if (level == 0 && lane == 0) s_m = total;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;

  const unsigned m = s_m;
  unsigned n_next = 0;
  for (int j = 0; j < n_q; ++j) {
    const bool live = s_slot[j] != DBENCH_QUANTILE_NO_SLOT;
    const unsigned prefix = live ? (s_prefix[s_slot[j]] | (s_digit[j] << shift)) : 0u;
    const unsigned below = s_below[j] + s_before[j];
    if (level == DBENCH_QUANTILE_LEVELS - 1) {
      out_values[j] = live ? prefix ^ flip : 0u;
      out_below[j] = live ? below : m;
      out_equal[j] = live ? s_count[j] : 0u;
      continue;
    }
    unsigned slot = DBENCH_QUANTILE_NO_SLOT;
    if (live) {
      for (unsigned k = 0; k < n_next; ++k)
        if (s_next[k] == prefix) slot = k;
      if (slot == DBENCH_QUANTILE_NO_SLOT) {
        slot = n_next++;
        s_next[slot] = prefix;
      }
    }
    tab->rank_slot[j] = slot;
    tab->rank_rem[j] = s_rem[j] - s_before[j];
    tab->rank_below[j] = below;
  }
  if (level == DBENCH_QUANTILE_LEVELS - 1) return;
  for (unsigned k = 0; k < n_next; ++k) tab->slot_prefix[k] = s_next[k];
  tab->n_slots = n_next;
  tab->m = m;
}

template <int SLOTS>
void launch_hist(bool list, unsigned grid, hipStream_t s, const unsigned *col, unsigned n_col, const unsigned *src, size_t entries,
                 const u64 *count, unsigned a, unsigned flip, int level, const QsTable *tab, unsigned *bins, int copies,
                 unsigned *status, size_t rounds) {
  if (list)
    hipLaunchKernelGGL((qs_hist<SLOTS, true>), dim3(grid), dim3(qs_threads(SLOTS)), 0, s, col, n_col, src, entries, count, a, flip,
                       level, tab, bins, copies, status, rounds);
  else
    hipLaunchKernelGGL((qs_hist<SLOTS, false>), dim3(grid), dim3(qs_threads(SLOTS)), 0, s, col, n_col, src, entries, count, a, flip,
                       level, tab, bins, copies, status, rounds);
}

}  // namespace

extern "C" size_t dbench_quantile_workspace_bytes(int n_q) {
  if (n_q < 1 || n_q > kQsMaxRanks) return 0;
  return qs_layout(qs_slots(n_q)).total;
}

extern "C" int dbench_quantile_select_u32(const uint32_t *col, size_t n_col, const uint32_t *rows, const uint64_t *count,
                                          size_t capacity, const uint32_t *q_num, const uint32_t *q_den, int n_q, int flags,
                                          uint32_t *out_values, uint32_t *out_below, uint32_t *out_equal, void *workspace,
                                          size_t workspace_bytes, void *stream) {
  if (flags & ~DBENCH_QUANTILE_SIGNED) return DBHIP_EINVAL;
  if (n_q < 1 || n_q > kQsMaxRanks) return DBHIP_EINVAL;
  if (!q_num || !q_den || !out_values || !out_below || !out_equal) return DBHIP_EINVAL;
  QsRanks ranks = {};
  for (int j = 0; j < n_q; ++j) {
    if (q_den[j] != 0 && q_num[j] > q_den[j]) return DBHIP_EINVAL;
    ranks.num[j] = q_num[j];
    ranks.den[j] = q_den[j];
  }
  if (!fits_32(n_col) || !fits_32(capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  const bool list = rows != nullptr;
  const size_t entries = list ? capacity : n_col;
  if (!col && n_col) return DBHIP_EINVAL;  // a NULL column with rows to read
  if ((addr(col) & 3u) || (addr(rows) & 3u) || (addr(count) & 7u)) return DBHIP_EINVAL;
  if ((addr(out_values) | addr(out_below) | addr(out_equal)) & 3u) return DBHIP_EINVAL;
  const size_t out_bytes = sizeof(uint32_t) * static_cast<size_t>(n_q);
  const Range ins[3] = {Range{col, 4 * n_col}, Range{rows, 4 * capacity}, Range{count, 8}};
  const Range outs[3] = {Range{out_values, out_bytes}, Range{out_below, out_bytes}, Range{out_equal, out_bytes}};
  if (outputs_overlap(outs, 3, ins, 3)) return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int slots = qs_slots(n_q), copies = qs_copies(slots);
  const QsLayout l = qs_layout(slots);
  int rc = begin_call(workspace, workspace_bytes, l.total, s, false);
  if (rc != DBHIP_OK) return rc;
  rc = static_cast<int>(fill_async(workspace, 0, l.total, s));  // the status word, the slot table and every bin
  if (rc != DBHIP_OK) return rc;

  char *base = static_cast<char *>(workspace);
  unsigned *status = static_cast<unsigned *>(workspace);
  QsTable *tab = reinterpret_cast<QsTable *>(base + l.table);
  const unsigned flip = (flags & DBENCH_QUANTILE_SIGNED) ? 0x80000000u : 0u;
  const unsigned *src = list ? rows : col;
  const unsigned a = words_past_16(src);
  const u64 *cnt = reinterpret_cast<const u64 *>(count);
  const unsigned n = static_cast<unsigned>(n_col);
  const size_t cus = static_cast<size_t>(current_device_info().cus);
  for (int level = 0; level < DBENCH_QUANTILE_LEVELS; ++level) {
    unsigned *bins = reinterpret_cast<unsigned *>(base + l.bins[level]);
    const int level_slots = level == 0 ? 1 : slots, level_copies = level == 0 ? kQsTopCopies : copies;
    if (entries) {
      const size_t rounds = (entries + a + qs_round(level_slots) - 1) / qs_round(level_slots);
      // sixteen slots fill a CU's LDS with one workgroup; the smaller kernels fit two
      const size_t cap = cus * (level_slots == 16 ? 1 : 2);
      const unsigned grid = static_cast<unsigned>(rounds < cap ? rounds : cap);
      if (level_slots == 1)
        launch_hist<1>(list, grid, s, col, n, src, entries, cnt, a, flip, level, tab, bins, level_copies, status, rounds);
      else if (level_slots == 4)
        launch_hist<4>(list, grid, s, col, n, src, entries, cnt, a, flip, level, tab, bins, level_copies, status, rounds);
      else
        launch_hist<16>(list, grid, s, col, n, src, entries, cnt, a, flip, level, tab, bins, level_copies, status, rounds);
    }
    hipLaunchKernelGGL(qs_pick, dim3(1), dim3(kQsPickThreads), 0, s, tab, bins, level_copies, level_slots, level, ranks, n_q,
                       flip, out_values, out_below, out_equal);
  }
  return launch_status();
}
