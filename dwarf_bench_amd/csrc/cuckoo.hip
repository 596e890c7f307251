// cuckoo.hip — the two-choice cuckoo hash table for gfx950: HIP counterpart of CuckooHashtable
// (common/dpcpp/cuckoo_hashtable.hpp) and the table of the reference's CuckooHashBuild dwarf (hash/cuckoo_hash_build.cpp).
//
// Layout: workspace header (status word) | slots[table_size], one 8-byte word per slot, key in the low word and value in
// the high word; empty = key 0xFFFFFFFF, value 0 (cuckoo_hashtable.hpp:16).  Key and value share one word so that one
// 64-bit atomic moves both: the reference keeps keys[] and vals[] apart and guards each slot with a spin lock built
// from fetch_or on a bitmask (:65-80), which can livelock lanes of one wave that contend for one lock.  Here an insert
// is a chain of device-scope 64-bit exchanges (global_atomic_swap_x2): the lane swaps the pair it carries into its
// position, and whatever comes back is the next pair to carry, at the reference's next position
// (pos == h1(k) ? h2(k) : h1(k), :43-63).  An empty pair coming back ends the chain.  No lane waits on another, and
// the chain is at most max_iter exchanges long; a lane that reaches it drops the pair it carries, as the reference
// does, and reports the row as not inserted (DBHIP_DEV_TABLE_FULL).  A lookup reads h1(k) and, only if that slot holds
// another key, h2(k) (at(), :29-37: the h1 slot wins).
#include "dbhip_common.hpp"

namespace dbhip {
namespace {

constexpr int kCkThreads = 256;
constexpr unsigned kCkEmptyKey = 0xFFFFFFFFu;
constexpr unsigned long long kCkEmptySlot = 0x00000000FFFFFFFFull;  // key 0xFFFFFFFF, value 0
constexpr unsigned kCkDefaultMaxIter = 100000;                     // cuckoo_hashtable.hpp:19 (max_iter = 1e5)
constexpr unsigned kCkMaxIterLimit = 1u << 20;

inline unsigned ck_grid(size_t n, const DeviceInfo &dev, int per_cu = 8) {
  const size_t want = (n + kCkThreads - 1) / kCkThreads;
  const size_t cap = static_cast<size_t>(dev.cus) * per_cu;
  return static_cast<unsigned>(want < cap ? (want ? want : 1) : cap);
}

inline bool ck_size_ok(size_t table_size) { return table_size != 0 && table_size <= 0xFFFFFFFFull; }
inline size_t ck_workspace_bytes(size_t table_size) {
  return align_up(kWsHeader + table_size * sizeof(unsigned long long), kWsAlign);
}

// hash_kind 0: (k % size + seed) % size (StaticSimpleHasher / StaticSimpleHasherWithOffset, hashfunctions.hpp:33-41,
// seed = the offset); 1: MurmurHash3_x86_32(k, seed) % size (hashfunctions.hpp:64-130); 2: the high word of
// mix64(seed, k) % size.  Kind 1 is the reference's pair and a weak one for cuckoo hashing: Murmur3 of a 4-byte key is
// F(seed ^ f(k)) with bijections F and f, so for every key k the key k' with f(k') = f(k) ^ seed1 ^ seed2 has
// h1(k') = h2(k) and h2(k') = h1(k).  Such pairs are a double edge of the cuckoo graph, and with millions of keys some
// component collects more keys than slots whatever the seeds.  Kind 2 has no such relation.
__device__ __forceinline__ unsigned ck_hash(unsigned key, int kind, unsigned seed, unsigned size) {
  if (kind == 0) {
    const unsigned long long s = static_cast<unsigned long long>(key % size) + seed % size;
    return static_cast<unsigned>(s >= size ? s - size : s);
  }
  if (kind == 1) return murmur3_x86_32_u32(key, seed) % size;
  return static_cast<unsigned>(mix64(seed, key) >> 32) % size;
}
inline bool ck_kind_ok(int hash_kind) { return hash_kind >= 0 && hash_kind <= 2; }

struct CkHash {
  unsigned size;
  int kind;
  unsigned seed1, seed2;
  __device__ __forceinline__ unsigned h1(unsigned k) const { return ck_hash(k, kind, seed1, size); }
  __device__ __forceinline__ unsigned h2(unsigned k) const { return ck_hash(k, kind, seed2, size); }
};

// insert(), cuckoo_hashtable.hpp:43-63, with the lock + test + swap of one slot replaced by one atomic exchange
__device__ __forceinline__ bool ck_insert(unsigned key, unsigned val, const CkHash &H, unsigned max_iter,
                                          unsigned long long *slots) {
  unsigned long long carry = (static_cast<unsigned long long>(val) << 32) | key;
  unsigned pos = H.h1(key);
  for (unsigned it = 0; it < max_iter; ++it) {
    carry = atomicExch(&slots[pos], carry);
    const unsigned k = static_cast<unsigned>(carry);
    if (k == kCkEmptyKey) return true;
    const unsigned p1 = H.h1(k);
    pos = pos == p1 ? H.h2(k) : p1;
  }
  return false;  // the pair in `carry` is dropped, as in the reference
}

__global__ __launch_bounds__(kCkThreads) void ck_insert_kernel(const unsigned *__restrict__ in_keys,
                                                               const unsigned *__restrict__ in_vals, size_t n,
                                                               CkHash H, unsigned max_iter, unsigned long long *slots,
                                                               unsigned *status, unsigned *__restrict__ out_inserted,
                                                               int serial) {
  const size_t first = serial ? 0 : static_cast<size_t>(blockIdx.x) * kCkThreads + threadIdx.x;
  const size_t stride = serial ? 1 : static_cast<size_t>(gridDim.x) * kCkThreads;
  if (serial && (blockIdx.x != 0 || threadIdx.x != 0)) return;  // one work-item, input order: the reference tests' layouts
  unsigned raised = 0;
  for (size_t i = first; i < n; i += stride) {
    const unsigned key = in_keys[i];
    bool ok = false;
    if (key == kCkEmptyKey) {
      raised |= DBHIP_DEV_KEY_RANGE;  // the empty pattern is not a key
    } else {
      ok = ck_insert(key, in_vals[i], H, max_iter, slots);
      if (!ok) raised |= DBHIP_DEV_TABLE_FULL;
    }
    if (out_inserted) out_inserted[i] = ok ? 1u : 0u;
  }
  if (raised) atomicOr(status, raised);
}

// The h2 read is issued only after the h1 slot held another key.  Issuing both reads up front was measured and rejected
// (DESIGN.md §4.6): the lookup is bound by the random-read rate, and the second read of a key found at h1 is wasted.
__global__ __launch_bounds__(kCkThreads) void ck_lookup_kernel(const unsigned *__restrict__ q, size_t n, CkHash H,
                                                               const unsigned long long *__restrict__ slots,
                                                               unsigned *__restrict__ out_vals,
                                                               unsigned *__restrict__ out_found) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kCkThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kCkThreads + threadIdx.x; i < n; i += stride) {
    const unsigned key = q[i];
    unsigned long long s = slots[H.h1(key)];
    if (static_cast<unsigned>(s) != key) s = slots[H.h2(key)];
    const bool found = key != kCkEmptyKey && static_cast<unsigned>(s) == key;
    out_vals[i] = found ? static_cast<unsigned>(s >> 32) : 0u;
    out_found[i] = found ? 1u : 0u;
  }
}

// header cleared and every slot set to the empty pair with 16-byte stores; `tail` is the last slot of an odd table
__global__ __launch_bounds__(kCkThreads) void ck_reset_kernel(u32x4 *base, size_t n_vec, unsigned long long *tail) {
  constexpr size_t kHeaderVecs = kWsHeader / sizeof(u32x4);
  const size_t stride = static_cast<size_t>(gridDim.x) * kCkThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kCkThreads + threadIdx.x; i < n_vec; i += stride)
    base[i] = i < kHeaderVecs ? u32x4{0u, 0u, 0u, 0u} : u32x4{kCkEmptyKey, 0u, kCkEmptyKey, 0u};
  if (tail && blockIdx.x == 0 && threadIdx.x == 0) *tail = kCkEmptySlot;
}

__global__ __launch_bounds__(kCkThreads) void ck_export_kernel(const unsigned long long *__restrict__ slots, size_t n,
                                                               unsigned *__restrict__ out_keys,
                                                               unsigned *__restrict__ out_vals) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kCkThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kCkThreads + threadIdx.x; i < n; i += stride) {
    const unsigned long long s = slots[i];
    out_keys[i] = static_cast<unsigned>(s);
    out_vals[i] = static_cast<unsigned>(s >> 32);
  }
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_cuckoo_table_workspace_bytes(size_t table_size) {
  return table_size ? ck_workspace_bytes(table_size) : 0;
}

extern "C" int dbhip_cuckoo_table_reset(void *workspace, size_t workspace_bytes, size_t table_size,
                                        dbhip_stream_t stream) {
  if (!ck_size_ok(table_size)) return DBHIP_EINVAL;
  if (!ws_ok(workspace, workspace_bytes, ck_workspace_bytes(table_size))) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  char *base = static_cast<char *>(workspace);
  // header + slots as 16-byte vectors; kWsHeader is a multiple of 16, so the vectors end on the last even slot
  const size_t n_vec = (kWsHeader + (table_size / 2) * 16) / 16;
  unsigned long long *tail =
      table_size % 2 ? reinterpret_cast<unsigned long long *>(base + kWsHeader) + (table_size - 1) : nullptr;
  hipLaunchKernelGGL(ck_reset_kernel, dim3(ck_grid(n_vec, dev)), dim3(kCkThreads), 0, as_stream(stream),
                     reinterpret_cast<u32x4 *>(base), n_vec, tail);
  return launch_status();
}

extern "C" int dbhip_cuckoo_table_insert_u32(const uint32_t *keys, const uint32_t *vals, size_t n, void *workspace,
                                             size_t workspace_bytes, size_t table_size, int hash_kind, uint32_t seed1,
                                             uint32_t seed2, uint32_t max_iter, int serial, uint32_t *out_inserted,
                                             dbhip_stream_t stream) {
  if (!ck_size_ok(table_size) || !ck_kind_ok(hash_kind) || max_iter > kCkMaxIterLimit) return DBHIP_EINVAL;
  if (n && (!keys || !vals)) return DBHIP_EINVAL;
  if (!ws_ok(workspace, workspace_bytes, ck_workspace_bytes(table_size))) return DBHIP_EWORKSPACE;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  // cuckoo_hashtable.hpp:45: min(input_size, max_iter) exchanges, input_size = the rows of the build
  const unsigned iters = max_iter ? max_iter : static_cast<unsigned>(n < kCkDefaultMaxIter ? n : kCkDefaultMaxIter);
  char *base = static_cast<char *>(workspace);
  const CkHash H{static_cast<unsigned>(table_size), hash_kind, seed1, seed2};
  hipLaunchKernelGGL(ck_insert_kernel, dim3(serial ? 1 : ck_grid(n, dev)), dim3(kCkThreads), 0, as_stream(stream), keys,
                     vals, n, H, iters, reinterpret_cast<unsigned long long *>(base + kWsHeader),
                     reinterpret_cast<unsigned *>(base), out_inserted, serial);
  return launch_status();
}

extern "C" int dbhip_cuckoo_table_lookup_u32(const uint32_t *keys, size_t n, const void *workspace, size_t table_size,
                                             int hash_kind, uint32_t seed1, uint32_t seed2, uint32_t *out_vals,
                                             uint32_t *out_found, dbhip_stream_t stream) {
  if (!ck_size_ok(table_size) || !ck_kind_ok(hash_kind) || !workspace) return DBHIP_EINVAL;
  if (n && (!keys || !out_vals || !out_found)) return DBHIP_EINVAL;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  const CkHash H{static_cast<unsigned>(table_size), hash_kind, seed1, seed2};
  const unsigned long long *slots =
      reinterpret_cast<const unsigned long long *>(static_cast<const char *>(workspace) + kWsHeader);
  hipLaunchKernelGGL(ck_lookup_kernel, dim3(ck_grid(n, dev)), dim3(kCkThreads), 0, as_stream(stream), keys, n, H, slots,
                     out_vals, out_found);
  return launch_status();
}

extern "C" int dbhip_cuckoo_table_export_u32(const void *workspace, size_t table_size, uint32_t *out_keys,
                                             uint32_t *out_vals, dbhip_stream_t stream) {
  if (!ck_size_ok(table_size) || !workspace || !out_keys || !out_vals) return DBHIP_EINVAL;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipLaunchKernelGGL(ck_export_kernel, dim3(ck_grid(table_size, dev)), dim3(kCkThreads), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long *>(static_cast<const char *>(workspace) + kWsHeader),
                     table_size, out_keys, out_vals);
  return launch_status();
}
