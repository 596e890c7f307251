// slab.hip — the slab hash table for gfx950: HIP counterpart of SlabHashTable (common/dpcpp/slab_hash.hpp) and the
// table of the reference's SlabHashBuild, SlabProbe and SlabJoin dwarfs.
//
// Every bucket heads a singly linked chain of slabs of 32 (key, value) pairs (SLAB_SIZE = 8 x 4, slab_hash.hpp:20-22);
// duplicate keys take slots of their own (a multimap).  Node b < buckets is bucket b's root slab; overflow nodes
// [buckets, buckets + pool_nodes) come from a pool cursor.  Workspace (all offsets multiples of 128 B):
//   header (256 B: [0] status word, [8] 64-bit pool cursor) | vals[nodes][32] | keys[nodes][32] | meta[nodes]
// A slab is one 128-B line of keys and one 128-B line of values; meta[i] is an 8-byte word {next node, tail hint}
// (next = 0xFFFFFFFF: none; the hint is used in the roots' words only).  Empty = key 0xFFFFFFFF, value 0.
//
// One row is handled by a group of 32 lanes (two rows per wave64), lane s holding slot s: a slab costs one coalesced
// key load and one __ballot gives its 32-slot empty / match mask.  Insert (slab_hash.hpp:144-175, :224-262): CAS the
// key of the lowest empty slot from EMPTY to k (a failed CAS returns the slot's key: the slot is full, try the next
// one), store the value with a plain store; when the slab is full go to `next`, and when there is none take a node
// from the pool and link it with a CAS of next from none.  A group that loses the link CAS keeps its node as a spare
// for its next append and follows the winner's link.  The reference appends under a spin lock (:209-222) that
// deadlocks a wave64 whose lanes contend for it, and never checks the heap's end (:92-97).  Here no lane waits on
// another, and every loop has a bound from the table's geometry: a chain walk at most buckets + pool_nodes steps, a
// slab at most 32 CASes (each failed one means another lane filled a slot).  A bound reached or a link pointing
// outside the table raises DBHIP_DEV_SPIN_TIMEOUT and stops the row; an exhausted pool raises DBHIP_DEV_TABLE_FULL.
// Either way the row is not stored and nothing is written outside the workspace.
//
// Slots never become empty again, so a slab a group saw full stays full, and a chain node reached past full slabs is
// a valid place to start an insert: inserts start at the bucket's tail hint, which they advance with a plain store
// each time they step past a full slab (a stale hint only lengthens the walk).  Lookups start at the root.
#include <stdlib.h>

#include <algorithm>

#include "dbhip_common.hpp"

namespace dbhip {
namespace {

constexpr int kSlThreads = 256;
constexpr int kSlGroup = 32;  // lanes per row = slots per slab
constexpr unsigned kSlEmpty = 0xFFFFFFFFu;
constexpr unsigned kSlNone = 0xFFFFFFFFu;
constexpr size_t kSlCursorOff = 8;  // header byte offset of the 64-bit pool cursor
constexpr unsigned kSlMaxInsertBlocks = DBHIP_SLAB_INSERT_GROUPS / (kSlThreads / kSlGroup);

struct SlabGeom {
  size_t nodes;
  size_t vals_off, keys_off, meta_off, bytes;
};
inline SlabGeom sl_geom(size_t buckets, size_t pool) {
  SlabGeom g;
  g.nodes = buckets + pool;
  g.vals_off = kWsHeader;
  g.keys_off = g.vals_off + g.nodes * kSlGroup * 4;
  g.meta_off = g.keys_off + g.nodes * kSlGroup * 4;
  g.bytes = align_up(g.meta_off + g.nodes * 8, kWsAlign);
  return g;
}
inline bool sl_size_ok(size_t buckets, size_t pool) {
  return buckets != 0 && pool <= 0xFFFFFFFFull && buckets <= 0xFFFFFFFFull - pool;  // node ids < 0xFFFFFFFF (= none)
}

// Exact x % d for x < 2^64 and 1 <= d < 2^32 without a 64-bit division: q = mulhi(x, m) with m = floor((2^64-1) / d)
// is at most two below floor(x / d), so r = x - q*d < 3d and two conditional subtractions finish it.
// m is computed once on the host.
struct SlMod {
  unsigned long long m;
  unsigned d;
};
inline SlMod sl_mod(unsigned long long d) { return SlMod{0xFFFFFFFFFFFFFFFFull / d, static_cast<unsigned>(d)}; }
__device__ __forceinline__ unsigned long long sl_rem(unsigned long long x, SlMod M) {
  unsigned long long r = x - __umul64hi(x, M.m) * M.d;
  if (r >= M.d) r -= M.d;
  if (r >= M.d) r -= M.d;
  return r;
}

// DefaultHasher<A, B, P> (slab_hash.hpp:60-64): ((A*k + B) % P) % buckets in 64 bits; A, B, P < 2^32 keep A*k + B
// below 2^64
struct SlHash {
  unsigned long long a, b;
  SlMod p, buckets;
  __device__ __forceinline__ unsigned operator()(unsigned k) const {
    return static_cast<unsigned>(sl_rem(sl_rem(a * k + b, p), buckets));
  }
};

struct SlTable {
  unsigned *keys, *vals;
  unsigned long long *meta;
  unsigned long long *cursor;
  unsigned *status;
  unsigned buckets, pool, nodes;
};

__device__ __forceinline__ unsigned group_mask(unsigned long long ballot, unsigned half) {
  return static_cast<unsigned>(ballot >> (half * 32));
}

// Insert one row with the 32 lanes of a group (every lane of the group calls it with the same key).  Returns true when
// the pair was stored; `raised` collects status bits; `spare` is the group's unlinked pool node (kSlNone: none).
__device__ bool sl_insert(const SlTable &T, unsigned bucket, unsigned key, unsigned val, unsigned slot, unsigned half,
                          unsigned rot, bool spread_first, bool use_hint, unsigned &spare, unsigned &raised) {
  // Key lines are read with L1-bypassing loads: a stale line costs one failed CAS per slot it shows empty, and the
  // failed CAS drops the line from this XCD's L2, so the next visit reads it fresh.  The root's line is read together
  // with the hint, so a chain that never grew past its root pays no extra latency for the hint.
  unsigned *hint = reinterpret_cast<unsigned *>(&T.meta[bucket]) + 1;
  unsigned node = bucket;
  unsigned k = __hip_atomic_load(&T.keys[static_cast<size_t>(node) * kSlGroup + slot], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  if (use_hint) {
    const unsigned h = *hint;
    if (h < T.nodes && h != bucket) {  // kSlNone (or anything stale outside the table): the root
      node = h;
      k = __hip_atomic_load(&T.keys[static_cast<size_t>(node) * kSlGroup + slot], __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (unsigned step = 0; step < T.nodes; ++step) {
    unsigned *line = T.keys + static_cast<size_t>(node) * kSlGroup;
    unsigned empty = group_mask(__ballot(k == kSlEmpty), half);
    // at most 32 attempts: each failed CAS takes one bit out of `empty`
    for (int tries = 0; empty && tries < kSlGroup; ++tries) {
      unsigned target = __builtin_ctz(empty);
      if (rot && (spread_first || tries)) {  // the (rot mod popcount)-th empty slot: groups on a hot slab spread out
        const unsigned want = rot % __builtin_popcount(empty);
        const bool mine = (empty >> slot) & 1u && __builtin_popcount(empty & ((1u << slot) - 1u)) == want;
        target = __builtin_ctz(group_mask(__ballot(mine), half));
      }
      unsigned old = 0;
      if (slot == target) old = atomicCAS(&line[target], kSlEmpty, key);
      old = __shfl(old, static_cast<int>(half * 32 + target), kWave);
      if (old == kSlEmpty) {
        if (slot == target) T.vals[static_cast<size_t>(node) * kSlGroup + target] = val;
        return true;
      }
      empty &= ~(1u << target);
    }
    // the slab is full: follow next, appending a node when there is none
    unsigned *link = reinterpret_cast<unsigned *>(&T.meta[node]);
    unsigned nxt = *link;
    if (nxt == kSlNone) {  // read it again at the memory side before taking a node: a stale `none` would leak one
      unsigned fresh = 0;
      if (slot == 0) fresh = __hip_atomic_fetch_add(link, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      nxt = __shfl(fresh, static_cast<int>(half * 32), kWave);
    }
    if (nxt == kSlNone) {
      if (spare == kSlNone) {
        unsigned long long got = 0;
        if (slot == 0) got = atomicAdd(T.cursor, 1ull);
        got = __shfl(got, static_cast<int>(half * 32), kWave);
        if (got >= T.pool) {
          raised |= DBHIP_DEV_TABLE_FULL;
          return false;
        }
        spare = T.buckets + static_cast<unsigned>(got);
      }
      unsigned old = 0;
      if (slot == 0) old = atomicCAS(link, kSlNone, spare);
      old = __shfl(old, static_cast<int>(half * 32), kWave);
      if (old == kSlNone) {
        nxt = spare;
        spare = kSlNone;
      } else {
        nxt = old;  // another group linked first: keep the spare, move on to the winner's slab
      }
    }
    if (nxt >= T.nodes) break;  // a link outside the table: not a workspace this table reset
    if (use_hint && slot == 0) *hint = nxt;
    node = nxt;
    k = __hip_atomic_load(&T.keys[static_cast<size_t>(node) * kSlGroup + slot], __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
  }
  raised |= DBHIP_DEV_SPIN_TIMEOUT;
  return false;
}

// opts bit 0: serial, bit 1: tail hint, bit 2: after a failed CAS aim at the (row mod popcount)-th empty slot instead
// of the lowest, bit 3: do so from the first CAS on
__global__ __launch_bounds__(kSlThreads) void sl_insert_kernel(const unsigned *__restrict__ in_keys,
                                                               const unsigned *__restrict__ in_vals, size_t n, SlHash H,
                                                               SlTable T, unsigned *__restrict__ out_inserted,
                                                               unsigned opts) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned slot = lane & (kSlGroup - 1), half = lane >> 5;
  const bool serial = opts & 1u;
  const size_t group = (static_cast<size_t>(blockIdx.x) * kSlThreads + threadIdx.x) / kSlGroup;
  const size_t stride = static_cast<size_t>(gridDim.x) * kSlThreads / kSlGroup;
  if (serial && group != 0) return;  // one group, input order: the reference's sequential layout
  unsigned spare = kSlNone, raised = 0;
  for (size_t i = group; i < n; i += serial ? 1 : stride) {
    const unsigned key = in_keys[i];
    bool ok = false;
    if (key == kSlEmpty) {
      raised |= DBHIP_DEV_KEY_RANGE;  // the empty pattern is not a key
    } else {
      const unsigned rot = (opts & 4u) && !serial ? static_cast<unsigned>(i) | 1u : 0u;
      ok = sl_insert(T, H(key), key, in_vals[i], slot, half, rot, opts & 8u, opts & 2u, spare, raised);
    }
    if (out_inserted && slot == 0) out_inserted[i] = ok ? 1u : 0u;
  }
  if (raised && slot == 0) atomicOr(T.status, raised);
}

// find(), slab_hash.hpp:177-196, :264-294: the first slot in chain and slot order that holds the key.  Every slab but
// a chain's last is full, so a slab with an empty slot ends the walk without reading its link.
// kJoin = false: out0 = value or 0, out1 = found 1 / 0.  kJoin = true, SlabJoin's probe (join/slab_join.cpp:88-111) in
// dbhip_ujoin_probe_u32's convention: out0 = key, out1 = build value, out2 = probe value; all 0xFFFFFFFF on a miss.
template <bool kJoin>
__global__ __launch_bounds__(kSlThreads) void sl_lookup_kernel(const unsigned *__restrict__ q,
                                                               const unsigned *__restrict__ probe_vals, size_t n,
                                                               SlHash H, SlTable T, unsigned *__restrict__ out0,
                                                               unsigned *__restrict__ out1,
                                                               unsigned *__restrict__ out2) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned slot = lane & (kSlGroup - 1), half = lane >> 5;
  const size_t stride = static_cast<size_t>(gridDim.x) * kSlThreads / kSlGroup;
  for (size_t i = (static_cast<size_t>(blockIdx.x) * kSlThreads + threadIdx.x) / kSlGroup; i < n; i += stride) {
    const unsigned key = q[i];
    unsigned val = 0;
    bool found = false;
    if (key != kSlEmpty) {
      unsigned node = H(key);
      for (unsigned step = 0; step < T.nodes; ++step) {
        const unsigned k = T.keys[static_cast<size_t>(node) * kSlGroup + slot];
        const unsigned hit = group_mask(__ballot(k == key), half);
        if (hit) {
          const unsigned s = __builtin_ctz(hit);
          if (slot == s) val = T.vals[static_cast<size_t>(node) * kSlGroup + s];
          val = __shfl(val, static_cast<int>(half * 32 + s), kWave);
          found = true;
          break;
        }
        if (group_mask(__ballot(k == kSlEmpty), half)) break;
        node = static_cast<unsigned>(T.meta[node]);
        if (node >= T.nodes) break;
      }
    }
    if (slot == 0 && kJoin) {
      out0[i] = found ? key : kSlNone;
      out1[i] = found ? val : kSlNone;
      out2[i] = found ? probe_vals[i] : kSlNone;
    } else if (slot == 0) {
      out0[i] = val;
      out1[i] = found ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(kSlThreads) void sl_export_kernel(SlTable T, unsigned *__restrict__ out_keys,
                                                               unsigned *__restrict__ out_vals,
                                                               unsigned *__restrict__ out_next,
                                                               unsigned *__restrict__ out_pool_used) {
  const size_t slots = static_cast<size_t>(T.nodes) * kSlGroup;
  const size_t stride = static_cast<size_t>(gridDim.x) * kSlThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kSlThreads + threadIdx.x; i < slots; i += stride) {
    out_keys[i] = T.keys[i];
    out_vals[i] = T.vals[i];
    if (i < T.nodes) out_next[i] = static_cast<unsigned>(T.meta[i]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long c = *T.cursor;
    *out_pool_used = static_cast<unsigned>(c < T.pool ? c : T.pool);
  }
}

inline unsigned sl_grid(size_t work_items, const DeviceInfo &dev, int per_cu = 8) {
  const size_t want = (work_items + kSlThreads - 1) / kSlThreads;
  const size_t cap = static_cast<size_t>(dev.cus) * per_cu;
  return static_cast<unsigned>(want < cap ? (want ? want : 1) : cap);
}

inline SlTable sl_table(const void *workspace, size_t buckets, size_t pool) {
  char *base = static_cast<char *>(const_cast<void *>(workspace));
  const SlabGeom g = sl_geom(buckets, pool);
  SlTable T;
  T.vals = reinterpret_cast<unsigned *>(base + g.vals_off);
  T.keys = reinterpret_cast<unsigned *>(base + g.keys_off);
  T.meta = reinterpret_cast<unsigned long long *>(base + g.meta_off);
  T.cursor = reinterpret_cast<unsigned long long *>(base + kSlCursorOff);
  T.status = reinterpret_cast<unsigned *>(base);
  T.buckets = static_cast<unsigned>(buckets);
  T.pool = static_cast<unsigned>(pool);
  T.nodes = static_cast<unsigned>(g.nodes);
  return T;
}

inline bool sl_hash_ok(uint64_t a, uint64_t b, uint64_t p) {
  return p != 0 && a <= 0xFFFFFFFFull && b <= 0xFFFFFFFFull && p <= 0xFFFFFFFFull;
}
inline SlHash sl_hash(uint64_t a, uint64_t b, uint64_t p, size_t buckets) { return SlHash{a, b, sl_mod(p), sl_mod(buckets)}; }

// experiment knobs of tools/ab.py slab, read on every call: DBHIP_SLAB_HINT=0 turns the tail hint off;
// DBHIP_SLAB_SPREAD=0 aims every CAS at the lowest empty slot, =1 spreads from the first CAS on (default: the first CAS
// at the lowest empty slot, the later ones spread)
inline bool env_is(const char *name, char v) {
  const char *e = getenv(name);
  return e && e[0] == v;
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_slab_table_workspace_bytes(size_t buckets, size_t pool_nodes) {
  return sl_size_ok(buckets, pool_nodes) ? sl_geom(buckets, pool_nodes).bytes : 0;
}

extern "C" int dbhip_slab_table_reset(void *workspace, size_t workspace_bytes, size_t buckets, size_t pool_nodes,
                                      dbhip_stream_t stream) {
  if (!sl_size_ok(buckets, pool_nodes)) return DBHIP_EINVAL;
  const SlabGeom g = sl_geom(buckets, pool_nodes);
  if (!ws_ok(workspace, workspace_bytes, g.bytes)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  char *base = static_cast<char *>(workspace);
  // header and values to 0, keys and links to 0xFF: every slab empty, every link none, every hint the root
  hipError_t e = fill_async(base, 0, g.keys_off, as_stream(stream));
  if (e == hipSuccess) e = fill_async(base + g.keys_off, 0xFF, g.meta_off + g.nodes * 8 - g.keys_off, as_stream(stream));
  return e == hipSuccess ? launch_status() : static_cast<int>(e);
}

extern "C" int dbhip_slab_table_insert_u32(const uint32_t *keys, const uint32_t *vals, size_t n, void *workspace,
                                           size_t workspace_bytes, size_t buckets, size_t pool_nodes, uint64_t hash_a,
                                           uint64_t hash_b, uint64_t hash_p, int serial, uint32_t *out_inserted,
                                           dbhip_stream_t stream) {
  if (!sl_size_ok(buckets, pool_nodes) || !sl_hash_ok(hash_a, hash_b, hash_p)) return DBHIP_EINVAL;
  if (n && (!keys || !vals)) return DBHIP_EINVAL;
  if (!ws_ok(workspace, workspace_bytes, sl_geom(buckets, pool_nodes).bytes)) return DBHIP_EWORKSPACE;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  const unsigned opts = (serial ? 1u : 0u) | (env_is("DBHIP_SLAB_HINT", '0') ? 0u : 2u) |
                        (env_is("DBHIP_SLAB_SPREAD", '0') ? 0u : 4u) | (env_is("DBHIP_SLAB_SPREAD", '1') ? 8u : 0u);
  // at most DBHIP_SLAB_INSERT_GROUPS groups, each of which may end holding one unlinked pool node
  const unsigned grid = serial ? 1u : std::min(sl_grid(n * kSlGroup, dev), kSlMaxInsertBlocks);
  hipLaunchKernelGGL(sl_insert_kernel, dim3(grid), dim3(kSlThreads), 0, as_stream(stream), keys, vals, n,
                     sl_hash(hash_a, hash_b, hash_p, buckets), sl_table(workspace, buckets, pool_nodes), out_inserted,
                     opts);
  return launch_status();
}

extern "C" int dbhip_slab_table_lookup_u32(const uint32_t *keys, size_t n, const void *workspace, size_t buckets,
                                           size_t pool_nodes, uint64_t hash_a, uint64_t hash_b, uint64_t hash_p,
                                           uint32_t *out_vals, uint32_t *out_found, dbhip_stream_t stream) {
  if (!sl_size_ok(buckets, pool_nodes) || !sl_hash_ok(hash_a, hash_b, hash_p) || !workspace) return DBHIP_EINVAL;
  if (n && (!keys || !out_vals || !out_found)) return DBHIP_EINVAL;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipLaunchKernelGGL(sl_lookup_kernel<false>, dim3(sl_grid(n * kSlGroup, dev)), dim3(kSlThreads), 0,
                     as_stream(stream), keys, nullptr, n, sl_hash(hash_a, hash_b, hash_p, buckets),
                     sl_table(workspace, buckets, pool_nodes), out_vals, out_found, nullptr);
  return launch_status();
}

extern "C" int dbhip_slab_table_join_probe_u32(const uint32_t *probe_keys, const uint32_t *probe_vals, size_t n,
                                               const void *workspace, size_t buckets, size_t pool_nodes,
                                               uint64_t hash_a, uint64_t hash_b, uint64_t hash_p, uint32_t *out_key,
                                               uint32_t *out_build_val, uint32_t *out_probe_val,
                                               dbhip_stream_t stream) {
  if (!sl_size_ok(buckets, pool_nodes) || !sl_hash_ok(hash_a, hash_b, hash_p) || !workspace) return DBHIP_EINVAL;
  if (n && (!probe_keys || !probe_vals || !out_key || !out_build_val || !out_probe_val)) return DBHIP_EINVAL;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipLaunchKernelGGL(sl_lookup_kernel<true>, dim3(sl_grid(n * kSlGroup, dev)), dim3(kSlThreads), 0,
                     as_stream(stream), probe_keys, probe_vals, n, sl_hash(hash_a, hash_b, hash_p, buckets),
                     sl_table(workspace, buckets, pool_nodes), out_key, out_build_val, out_probe_val);
  return launch_status();
}

extern "C" int dbhip_slab_table_export_u32(const void *workspace, size_t buckets, size_t pool_nodes,
                                           uint32_t *out_keys, uint32_t *out_vals, uint32_t *out_next,
                                           uint32_t *out_pool_used, dbhip_stream_t stream) {
  if (!sl_size_ok(buckets, pool_nodes) || !workspace || !out_keys || !out_vals || !out_next || !out_pool_used)
    return DBHIP_EINVAL;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipLaunchKernelGGL(sl_export_kernel, dim3(sl_grid((buckets + pool_nodes) * kSlGroup, dev)), dim3(kSlThreads), 0,
                     as_stream(stream), sl_table(workspace, buckets, pool_nodes), out_keys, out_vals, out_next,
                     out_pool_used);
  return launch_status();
}
