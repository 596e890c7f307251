// dict_encode.cpp — dictionary encoding on gfx950 (dict_encode.hpp holds the contract, dict_layout.hpp the hash, the
// workspace regions and the two probe loops, which the kernels below run on global and LDS pointers).
//
// The load shape is that of take_rows.cpp (the positions and the device count are rowlist.hpp's).  Positions are
// counted from the 16-byte boundary in front of the column: row i sits at v = i + a, a = 0..3 words, so every 16-byte
// load of rows is aligned whatever the pointer's alignment; a lane holds four consecutive rows, and the groups that
// straddle the ends of the column are handled word by word.  An output that sits at the same distance from a 16-byte
// boundary as the column is written with 16-byte stores, any other word by word.  Nothing outside the arrays is touched.
//   build    clear -> insert -> compact -> dbhip_radix_sort -> finalize, five dependent steps, no workgroup waits for
//            another.  insert: a lane drops a row that repeats the row before it, then asks the workgroup's LDS filter
//            (1024 entries, (valid, key), direct mapped by the key's hash): a key the workgroup has inserted costs one LDS
//            read; an exchange on the filter entry elects one lane among those of a workgroup that arrive with the same
//            new key, and only that lane goes to memory.  There the slot is read before any compare-and-swap.  The
//            column of one key therefore costs one LDS read per row and a handful of loads per workgroup.
//   encode   one kernel of 1024 threads and 64 KiB of LDS: two workgroups and all 32 waves per compute unit whichever
//            body runs.  The body is chosen ON THE DEVICE from the header (encode is not told the capacity): a table of
//            at most DBENCH_DICT_LDS_SLOTS slots is copied into LDS once per workgroup, a larger one is probed in global
//            memory; in both a lane issues the home-slot reads of its four rows before it looks at the first.
//   combine  one streaming kernel, four rows per lane.
#include "dict_encode.hpp"

#include "dict_layout.hpp"
#include "rowlist.hpp"

namespace {
using namespace dbhip;

constexpr unsigned kDictMagic = 0x44494354u;  // "DICT": a header some build of this file wrote
constexpr u64 kEmptySlot = static_cast<u64>(DBENCH_DICT_EMPTY) << 32;  // (key 0, code EMPTY)
constexpr int kBuildThreads = 256;
constexpr unsigned kBuildTile = 4 * kBuildThreads;  // rows (insert) or slots (compact) of a workgroup at a time
constexpr unsigned kSeenEntries = 1024;             // the insert's LDS filter: 8 KiB
constexpr int kEncThreads = 1024;
constexpr unsigned kEncTile = 4 * kEncThreads;
constexpr int kEncPerCu = 2;  // 64 KiB of LDS each
constexpr int kCombThreads = 256;
constexpr unsigned kCombTile = 4 * kCombThreads;
static_assert(sizeof(DictSlot) == 8 && sizeof(u64) == 8, "slot size");
static_assert(DBENCH_DICT_LDS_SLOTS * sizeof(DictSlot) == 64 * 1024, "the LDS body's table");
static_assert((DBENCH_DICT_LDS_SLOTS & (DBENCH_DICT_LDS_SLOTS - 1)) == 0, "a power of two");

struct DictHeader {
  unsigned status;    // DBHIP_DEV_*
  unsigned magic;     // kDictMagic once clear has run
  unsigned mask;      // slots - 1
  unsigned capacity;
  unsigned d;         // the number of keys; 0 until finalize has run, and after a build that overflowed
  unsigned cursor;    // compact: the number of used slots
  unsigned flip;      // 0x80000000 for a dictionary in int32 order
  unsigned pad[57];
};
static_assert(sizeof(DictHeader) == kWsHeader, "workspace header size");

__device__ __forceinline__ DictSlot unpack(u64 w) {
  DictSlot e;
  e.key = static_cast<unsigned>(w);
  e.code = static_cast<unsigned>(w >> 32);
  return e;
}

// a table that no kernel is writing: plain 8-byte loads, global or LDS
struct Slots {
  const u64 *p;
  __device__ __forceinline__ DictSlot operator[](unsigned s) const { return unpack(p[s]); }
};
// the table while inserts run: a slot is read whole, by one 8-byte load that the compiler may not split or keep
struct LiveSlots {
  u64 *p;
  __device__ __forceinline__ DictSlot operator[](unsigned s) const {
    return unpack(__hip_atomic_load(p + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
};

// (valid_four, load_four and store_four are not rowlist.hpp's load_ragged: they carry a `vec` flag, and the validity is
// computed once for a load and a store)
// bit q: position v0 + q holds a row, that is, lies in [a, vend)
__device__ __forceinline__ unsigned valid_four(unsigned a, size_t v0, size_t vend) {
  if (v0 >= a && v0 + 4 <= vend) return 0xfu;
  unsigned valid = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (v0 + q >= a && v0 + q < vend) valid |= 1u << q;
  }
  return valid;
}

// this lane's four words at positions v0 .. v0+3 of a column whose word 0 is position a.  vec: the column is `a` words
// past a 16-byte boundary, so a whole group is one aligned 16-byte load; words that hold no row come back 0
__device__ __forceinline__ u32x4 load_four(const unsigned *__restrict__ p, unsigned a, size_t v0, unsigned valid, bool vec) {
  u32x4 e = {0u, 0u, 0u, 0u};
  if (valid == 0xfu && vec) {
    e = *reinterpret_cast<const u32x4 *>(p + (v0 - a));
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((valid >> q) & 1u) e[q] = p[v0 + q - a];
    }
  }
  return e;
}

__device__ __forceinline__ void store_four(unsigned *__restrict__ p, unsigned a, size_t v0, unsigned valid, bool vec,
                                           const u32x4 x) {
  if (valid == 0xfu && vec) {
    *reinterpret_cast<u32x4 *>(p + (v0 - a)) = x;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((valid >> q) & 1u) p[v0 + q - a] = x[q];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------------
// the header, every slot empty, the key region (all of it, to its 256-byte end) padded with the order's maximum
__global__ __launch_bounds__(kBuildThreads) void dict_clear_kernel(DictHeader *hdr, u32x4 *__restrict__ table, u64 pairs,
                                                                   u32x4 *__restrict__ keys, u64 key_vectors, unsigned mask,
                                                                   unsigned capacity, unsigned flip) {
  const u64 tid = static_cast<u64>(blockIdx.x) * kBuildThreads + threadIdx.x;
  const u64 stride = static_cast<u64>(gridDim.x) * kBuildThreads;
  if (tid < kWsHeader / sizeof(unsigned)) {
    const unsigned words[7] = {0u, kDictMagic, mask, capacity, 0u, 0u, flip};
    reinterpret_cast<unsigned *>(hdr)[tid] = tid < 7 ? words[tid] : 0u;
  }
  const u32x4 empty2 = {0u, DBENCH_DICT_EMPTY, 0u, DBENCH_DICT_EMPTY};
  for (u64 j = tid; j < pairs; j += stride) table[j] = empty2;
  const unsigned top = 0xFFFFFFFFu ^ flip;  // the last key of the order
  const u32x4 pad4 = {top, top, top, top};
  for (u64 j = tid; j < key_vectors; j += stride) keys[j] = pad4;
}

__global__ __launch_bounds__(kBuildThreads) void dict_insert_kernel(const unsigned *__restrict__ col, size_t n, const u64 *count,
                                                                    unsigned a, u64 *table, unsigned mask, unsigned *status,
                                                                    size_t tiles) {
  __shared__ u64 s_seen[kSeenEntries];  // (1 << 32) | key of a key this workgroup has taken charge of; 0: none
  for (unsigned j = threadIdx.x; j < kSeenEntries; j += kBuildThreads) s_seen[j] = 0ull;
  __syncthreads();
  const size_t vend = a + clamped_count(count, n);  // positions [a, vend) hold rows
  const LiveSlots live{table};
  auto claim = [&](unsigned s, unsigned key) {
    return unpack(atomicCAS(table + s, kEmptySlot, (static_cast<u64>(DBENCH_DICT_PENDING) << 32) | key));
  };
  bool full = false;
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t vfirst = tile * kBuildTile;
    if (vfirst >= vend) break;  // behind the last row, and so is every later tile of this workgroup
    const size_t v0 = vfirst + 4 * threadIdx.x;
    const unsigned valid = valid_four(a, v0, vend);
    const u32x4 e = load_four(col, a, v0, valid, true);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned k = e[q];
      bool go = (valid >> q) & 1u;
      if (q > 0) go = go && !(((valid >> (q - 1)) & 1u) && k == e[q - 1]);  // the row before it went
      if (go) {
        const u64 tag = (1ull << 32) | k;
        u64 *seen = s_seen + ((dict_hash(k) >> 16) & (kSeenEntries - 1));
        if (__hip_atomic_load(seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != tag &&
            __hip_atomic_exchange(seen, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != tag) {
          // this lane put the key into the filter: it is the one that inserts it
          if (dict_insert(live, mask, k, claim) < 0) full = true;
        }
      }
    }
  }
  if (full) atomicOr(status, DBHIP_DEV_TABLE_FULL);
}

// the keys of the used slots -> keys[0 .. min(used, capacity)) in any order; *cursor = the number of used slots
__global__ __launch_bounds__(kBuildThreads) void dict_compact_kernel(const u64 *__restrict__ table, u64 slots, unsigned capacity,
                                                                     unsigned *__restrict__ keys, unsigned *cursor) {
  __shared__ unsigned s_wsum[kBuildThreads / kWave];
  __shared__ unsigned s_base;
#pragma unroll 1
  for (u64 t0 = static_cast<u64>(blockIdx.x) * kBuildTile; t0 < slots; t0 += static_cast<u64>(gridDim.x) * kBuildTile) {
    const u64 s0 = t0 + 4 * threadIdx.x;
    u64 w[4] = {kEmptySlot, kEmptySlot, kEmptySlot, kEmptySlot};
    if (s0 + 4 <= slots) {
      const u32x4 lo = *reinterpret_cast<const u32x4 *>(table + s0), hi = *reinterpret_cast<const u32x4 *>(table + s0 + 2);
      w[0] = (static_cast<u64>(lo[1]) << 32) | lo[0];
      w[1] = (static_cast<u64>(lo[3]) << 32) | lo[2];
      w[2] = (static_cast<u64>(hi[1]) << 32) | hi[0];
      w[3] = (static_cast<u64>(hi[3]) << 32) | hi[2];
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (s0 + q < slots) w[q] = table[s0 + q];
      }
    }
    unsigned used = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) used += static_cast<unsigned>(w[q] >> 32) != DBENCH_DICT_EMPTY ? 1u : 0u;
    unsigned total;
    const unsigned before = block_exclusive_scan<kBuildThreads>(used, s_wsum, total);
    if (threadIdx.x == 0) s_base = total ? atomicAdd(cursor, total) : 0u;
    __syncthreads();
    unsigned at = s_base + before;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (static_cast<unsigned>(w[q] >> 32) != DBENCH_DICT_EMPTY) {
        if (at < capacity) keys[at] = static_cast<unsigned>(w[q]);
        ++at;
      }
    }
  }
}

// behind the sort: key i of the order gets rank i in its slot and goes to out_keys; thread 0 leaves d and the status
__global__ __launch_bounds__(kBuildThreads) void dict_finalize_kernel(DictHeader *hdr, u64 *table, unsigned mask, unsigned capacity,
                                                                      const unsigned *__restrict__ keys,
                                                                      const unsigned *__restrict__ sort_status,
                                                                      unsigned *__restrict__ out_keys, u64 *__restrict__ out_count) {
  const unsigned i = blockIdx.x * kBuildThreads + threadIdx.x;  // capacity < 2^31
  const unsigned used = hdr->cursor;
  const bool full = used > capacity;  // (a probe that went round a full table has used == slots > capacity)
  const unsigned d = full ? 0u : used;
  if (i < d) {
    const unsigned key = keys[i];
    const int64_t s = dict_find_slot(Slots{table}, mask, key);
    if (s >= 0) reinterpret_cast<unsigned *>(table)[2 * s + 1] = i;  // the code word; the key word stays
    out_keys[i] = key;
  }
  if (i == 0) {
    hdr->d = d;
    *out_count = d;
    const unsigned bits = (full ? DBHIP_DEV_TABLE_FULL : 0u) | *sort_status;
    if (bits) atomicOr(&hdr->status, bits);
  }
}

// ---------------------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------------------
// the codes of a lane's four rows: the four home slots are read before the first is looked at.  A code of d or more is
// no rank: an empty slot, a slot whose rank was never stored, a table no build finished
template <class Table>
__device__ __forceinline__ u32x4 codes_of_four(const Table &table, unsigned mask, unsigned d, const u32x4 e, unsigned valid,
                                               unsigned &misses) {
  DictSlot home[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) home[q] = table[dict_hash(e[q]) & mask];
  u32x4 code;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned c = dict_find_after(table, mask, e[q], home[q]);
    code[q] = c < d ? c : DBENCH_DICT_MISS;
    misses += (((valid >> q) & 1u) && code[q] == DBENCH_DICT_MISS) ? 1u : 0u;
  }
  return code;
}

template <class Table>
__device__ __forceinline__ unsigned encode_tiles(const Table &table, unsigned mask, unsigned d, const unsigned *__restrict__ col,
                                                 unsigned a, size_t vend, unsigned *__restrict__ out, bool vec_out,
                                                 size_t tiles) {
  unsigned misses = 0;
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t vfirst = tile * kEncTile;
    if (vfirst >= vend) break;
    const size_t v0 = vfirst + 4 * threadIdx.x;
    const unsigned valid = valid_four(a, v0, vend);
    if (!valid) continue;  // (no barrier below)
    const u32x4 e = load_four(col, a, v0, valid, true);
    u32x4 code = {DBENCH_DICT_MISS, DBENCH_DICT_MISS, DBENCH_DICT_MISS, DBENCH_DICT_MISS};
    if (d)  // uniform
      code = codes_of_four(table, mask, d, e, valid, misses);
    else
      misses += __popc(valid);
    store_four(out, a, v0, valid, vec_out, code);
  }
  return misses;
}

__global__ __launch_bounds__(kEncThreads) void dict_encode_kernel(const unsigned *__restrict__ col, size_t n, const u64 *count,
                                                                  unsigned a, unsigned *__restrict__ out, bool vec_out,
                                                                  const DictHeader *hdr, size_t ws_bytes, u64 *misses_out,
                                                                  size_t tiles) {
  __shared__ u64 s_table[DBENCH_DICT_LDS_SLOTS];
  const u64 *table = reinterpret_cast<const u64 *>(reinterpret_cast<const char *>(hdr) + kWsHeader);
  // the header is trusted as far as the bytes this call was given reach
  const unsigned mask = hdr->mask;
  const u64 slots = static_cast<u64>(mask) + 1;
  const bool usable = hdr->magic == kDictMagic && (slots & mask) == 0 && slots >= 2 &&
                      slots <= (ws_bytes - kWsHeader) / sizeof(DictSlot) && hdr->d <= hdr->capacity && hdr->capacity <= slots / 2;
  const unsigned d = usable ? hdr->d : 0u;
  const size_t vend = a + clamped_count(count, n);
  unsigned misses;
  if (d && slots <= DBENCH_DICT_LDS_SLOTS) {  // uniform
    const u32x4 *src = reinterpret_cast<const u32x4 *>(table);
    u32x4 *dst = reinterpret_cast<u32x4 *>(s_table);
    for (unsigned j = threadIdx.x; j < slots / 2; j += kEncThreads) dst[j] = src[j];
    __syncthreads();
    misses = encode_tiles(Slots{s_table}, mask, d, col, a, vend, out, vec_out, tiles);
  } else {
    misses = encode_tiles(Slots{table}, mask, d, col, a, vend, out, vec_out, tiles);
  }
  if (misses_out) {
    const unsigned wave_misses = wave_reduce_add(misses);
    if ((threadIdx.x & (kWave - 1)) == 0 && wave_misses) atomicAdd(misses_out, static_cast<u64>(wave_misses));
  }
}

// ---------------------------------------------------------------------------------------------
// combine
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCombThreads) void dict_combine_kernel(const unsigned *outer, const unsigned *__restrict__ inner,
                                                                    size_t n, const u64 *count, const u64 *__restrict__ outer_card,
                                                                    const u64 *__restrict__ inner_card, unsigned a, unsigned *out,
                                                                    bool vec_inner, bool vec_out, unsigned *status) {
  const u64 oc = *outer_card, ic = *inner_card;
  const bool wide = oc != 0 && ic > 0xFFFFFFFFull / oc;  // oc * ic > 0xFFFFFFFF
  if (wide && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
  const unsigned mul = static_cast<unsigned>(ic);
  const size_t vend = a + clamped_count(count, n);
  const size_t v0 = static_cast<size_t>(blockIdx.x) * kCombTile + 4 * threadIdx.x;
  const unsigned valid = valid_four(a, v0, vend);
  if (!valid) return;
  const u32x4 o = load_four(outer, a, v0, valid, true);
  const u32x4 i = load_four(inner, a, v0, valid, vec_inner);
  u32x4 x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool miss = wide || o[q] == DBENCH_DICT_MISS || i[q] == DBENCH_DICT_MISS;
    x[q] = miss ? DBENCH_DICT_MISS : o[q] * mul + i[q];
  }
  store_four(out, a, v0, valid, vec_out, x);
}

bool capacity_ok(size_t capacity) { return capacity >= 1 && capacity < (1ull << 31); }

DictLayout layout_of(size_t capacity) { return dict_layout(capacity, dbhip_radix_sort_workspace_bytes(capacity, 8)); }

}  // namespace

extern "C" size_t dbench_dict_workspace_bytes(size_t capacity) {
  if (!capacity_ok(capacity)) return 0;
  return static_cast<size_t>(layout_of(capacity).total);
}

extern "C" int dbench_dict_build_u32(const uint32_t *col, size_t n, const uint64_t *count, size_t capacity, int flags,
                                     uint32_t *out_keys, uint64_t *out_count, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  if (flags & ~DBENCH_DICT_SIGNED) return DBHIP_EINVAL;
  if (!capacity_ok(capacity) || !fits_32(n)) return DBHIP_EINVAL;
  if ((n && !col) || !out_keys || !out_count) return DBHIP_EINVAL;
  if (((addr(col) | addr(out_keys)) & 3u) || ((addr(count) | addr(out_count)) & 7u)) return DBHIP_EINVAL;
  if (overlap(out_keys, 4 * capacity, col, 4 * n) || overlap(out_keys, 4 * capacity, count, 8) ||
      overlap(out_count, 8, col, 4 * n) || overlap(out_count, 8, count, 8) || overlap(out_count, 8, out_keys, 4 * capacity))
    return DBHIP_EINVAL;
  const DictLayout l = layout_of(capacity);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ready = begin_call(workspace, workspace_bytes, l.total, s, false);  // dict_clear_kernel writes the header
  if (ready != DBHIP_OK) return ready;
  const DeviceInfo &dev = current_device_info();

  char *ws = static_cast<char *>(workspace);
  DictHeader *hdr = reinterpret_cast<DictHeader *>(ws);
  u64 *table = reinterpret_cast<u64 *>(ws + l.table);
  unsigned *keys = reinterpret_cast<unsigned *>(ws + l.keys), *tmp = reinterpret_cast<unsigned *>(ws + l.tmp);
  void *sort_ws = ws + l.sort;
  const size_t sort_bytes = l.total - l.sort;
  const unsigned mask = static_cast<unsigned>(l.slots - 1), cap = static_cast<unsigned>(capacity);
  const unsigned flip = (flags & DBENCH_DICT_SIGNED) ? 0x80000000u : 0u;

  const u64 pairs = l.slots / 2, key_vectors = (l.tmp - l.keys) / 16;
  hipLaunchKernelGGL(dict_clear_kernel, dim3(capped_grid(pairs + key_vectors, kBuildThreads, dev)), dim3(kBuildThreads), 0, s,
                     hdr, reinterpret_cast<u32x4 *>(table), pairs, reinterpret_cast<u32x4 *>(keys), key_vectors, mask, cap, flip);
  if (n) {
    const unsigned a = words_past_16(col);
    const size_t tiles = (n + a + kBuildTile - 1) / kBuildTile;
    hipLaunchKernelGGL(dict_insert_kernel, dim3(capped_grid(tiles, 1, dev)), dim3(kBuildThreads), 0, s, col, n,
                       reinterpret_cast<const u64 *>(count), a, table, mask, &hdr->status, tiles);
  }
  hipLaunchKernelGGL(dict_compact_kernel, dim3(capped_grid(l.slots, kBuildTile, dev)), dim3(kBuildThreads), 0, s, table,
                     static_cast<u64>(l.slots), cap, keys, &hdr->cursor);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  const int rc = flip ? dbhip_radix_sort_i32(reinterpret_cast<int32_t *>(keys), reinterpret_cast<int32_t *>(tmp), capacity, 8,
                                             sort_ws, sort_bytes, stream)
                      : dbhip_radix_sort_u32(keys, tmp, capacity, 8, sort_ws, sort_bytes, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(dict_finalize_kernel, dim3(static_cast<unsigned>((capacity + kBuildThreads - 1) / kBuildThreads)),
                     dim3(kBuildThreads), 0, s, hdr, table, mask, cap, keys, static_cast<const unsigned *>(sort_ws), out_keys,
                     reinterpret_cast<u64 *>(out_count));
  return launch_status();
}

extern "C" int dbench_dict_encode_u32(const uint32_t *col, size_t n, const uint64_t *count, uint32_t *out_codes,
                                      uint64_t *out_misses, const void *workspace, size_t workspace_bytes, void *stream) {
  if (!fits_32(n)) return DBHIP_EINVAL;
  if (n && (!col || !out_codes)) return DBHIP_EINVAL;
  if (((addr(col) | addr(out_codes)) & 3u) || ((addr(count) | addr(out_misses)) & 7u)) return DBHIP_EINVAL;
  if (overlap(out_codes, 4 * n, col, 4 * n) || overlap(out_codes, 4 * n, count, 8) || overlap(out_codes, 4 * n, out_misses, 8) ||
      overlap(out_misses, 8, col, 4 * n) || overlap(out_misses, 8, count, 8))
    return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (the workspace is the dictionary: read, never cleared)
  const int rc = begin_call(const_cast<void *>(workspace), workspace_bytes, dbench_dict_workspace_bytes(1), s, false);
  if (rc != DBHIP_OK) return rc;
  const DeviceInfo &dev = current_device_info();

  if (out_misses) {
    const hipError_t e = fill_async(out_misses, 0, 8, s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (!n) return launch_status();
  const unsigned a = words_past_16(col);
  const size_t tiles = (n + a + kEncTile - 1) / kEncTile;
  hipLaunchKernelGGL(dict_encode_kernel, dim3(capped_grid(tiles, 1, dev, kEncPerCu)), dim3(kEncThreads), 0, s, col, n,
                     reinterpret_cast<const u64 *>(count), a, out_codes, words_past_16(out_codes) == a,
                     static_cast<const DictHeader *>(workspace), workspace_bytes, reinterpret_cast<u64 *>(out_misses), tiles);
  return launch_status();
}

extern "C" int dbench_dict_combine_u32(const uint32_t *outer, const uint32_t *inner, size_t n, const uint64_t *count,
                                       const uint64_t *outer_card, const uint64_t *inner_card, uint32_t *out, void *workspace,
                                       size_t workspace_bytes, void *stream) {
  if (!fits_32(n)) return DBHIP_EINVAL;
  if ((n && (!outer || !inner || !out)) || !outer_card || !inner_card) return DBHIP_EINVAL;
  if (((addr(outer) | addr(inner) | addr(out)) & 3u) || ((addr(count) | addr(outer_card) | addr(inner_card)) & 7u))
    return DBHIP_EINVAL;
  if ((out != outer && overlap(out, 4 * n, outer, 4 * n)) || overlap(out, 4 * n, inner, 4 * n) || overlap(out, 4 * n, count, 8) ||
      overlap(out, 4 * n, outer_card, 8) || overlap(out, 4 * n, inner_card, 8))
    return DBHIP_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, kWsHeader, s);
  if (rc != DBHIP_OK) return rc;
  const unsigned a = n ? words_past_16(outer) : 0u;
  const size_t tiles = (n + a + kCombTile - 1) / kCombTile;
  // (one workgroup at least: the cardinalities are judged for an empty column too)
  hipLaunchKernelGGL(dict_combine_kernel, dim3(static_cast<unsigned>(tiles ? tiles : 1)), dim3(kCombThreads), 0, s, outer, inner, n,
                     reinterpret_cast<const u64 *>(count), reinterpret_cast<const u64 *>(outer_card),
                     reinterpret_cast<const u64 *>(inner_card), a, out, words_past_16(inner) == a, words_past_16(out) == a,
                     static_cast<unsigned *>(workspace));
  return launch_status();
}
