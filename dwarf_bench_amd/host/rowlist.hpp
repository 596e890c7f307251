// rowlist.hpp — what the row-id operators of libdbench.so share (select_rows, merge_sorted, take_rows, dict_encode,
// bitpack), once each; call_checks.hpp holds the part of it that needs no HIP.
//   host:    begin_call (the steps between an entry point's argument checks and its first launch),
//            launch_rowlist_scan (counts -> first output positions and the total, rowlist.cpp)
//   device:  clamped_count, load_ragged, RangePred / range_keep
// Positions of a column or a row-id list are counted from the 16-byte boundary in front of it: entry i sits at
// v = i + a, a = words_past_16(p) = 0..3, so every 16-byte load is aligned whatever the pointer's alignment, and the
// two vectors that straddle the ends of the array are read word by word (load_ragged).
#pragma once
#include "call_checks.hpp"
#include "dbhip_common.hpp"

namespace dbhip {

typedef unsigned long long u64;

// behind an entry point's own argument checks, in this order: the workspace (DBHIP_EWORKSPACE), the device
// (DBHIP_ENODEVICE), and the clear of the workspace header — a launch of its own, in front of the one that can raise the
// status word.  -> DBHIP_OK, or the code to return
inline int begin_call(void *workspace, size_t have, size_t need, hipStream_t s, bool clear_header = true) {
  if (!ws_ok(workspace, have, need)) return DBHIP_EWORKSPACE;
  if (!current_device_info().ok) return DBHIP_ENODEVICE;
  return clear_header ? static_cast<int>(fill_async(workspace, 0, kWsHeader, s)) : DBHIP_OK;
}

// cnt[0 .. n) -> pos[i] = the sum of the counts in front of i; *out_count = min(their total, bound).  One workgroup,
// enqueued on s; cnt and pos are padded to 256 bytes in the workspace
void launch_rowlist_scan(const unsigned *cnt, unsigned *pos, size_t n, u64 bound, u64 *out_count, hipStream_t s);

// m = min(*count, capacity), read on the device
__device__ __forceinline__ size_t clamped_count(const u64 *count, size_t capacity) {
  size_t m = capacity;
  if (count) {
    const u64 given = *count;
    if (given < m) m = static_cast<size_t>(given);
  }
  return m;
}

// this lane's four entries at positions v0 .. v0+3, word by word: bit q of `valid` says that position v0 + q holds an
// entry, that is, lies in [a, vend)
__device__ __forceinline__ u32x4 load_ragged(const unsigned *__restrict__ src, unsigned a, size_t v0, size_t vend,
                                             unsigned &valid) {
  u32x4 e = {0u, 0u, 0u, 0u};
  valid = 0;
  if (v0 >= a && v0 + 4 <= vend) {
    e = *reinterpret_cast<const u32x4 *>(src + (v0 - a));
    valid = 0xfu;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (v0 + q >= a && v0 + q < vend) {
        e[q] = src[v0 + q - a];
        valid |= 1u << q;
      }
    }
  }
  return e;
}

struct RangePred {
  unsigned flip, lo, hi;  // x is inside iff lo <= (x ^ flip) <= hi, lo and hi already flipped (0x80000000 for int32)
  bool negate;
};

__device__ __forceinline__ bool range_keep(unsigned x, const RangePred &p) {
  const unsigned y = x ^ p.flip;
  return (y >= p.lo && y <= p.hi) != p.negate;
}

}  // namespace dbhip
