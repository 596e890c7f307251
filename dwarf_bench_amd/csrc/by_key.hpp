// by_key.hpp — what the by-key kernels share: reduce_by_key.hip (one row per run) and scan_by_key.hip (one row per row).
//
// The terms, for both files:
//   HEAD      row 0, or a row whose key differs from its left neighbour's.
//   run       run r is the rows from the r-th head to the row in front of the next one; scan-by-key's run number is the
//             run's row in reduce-by-key's table.
//   x domain  MIN and MAX work on x = value ^ sign (sign = 0x80000000 with vals_signed), for which smaller means smaller as
//             unsigned; the SUM adds the value itself, zero- or sign-extended to 64 bits (bk_ext).
//   SEGMENT   the 4096 rows of one wave; segment starts are multiples of 4096 rows, so with 16-byte aligned columns a
//             whole segment is read with 16-byte loads.  Only the last segment of a column can be ragged.
//   chunk     the eight segments (32768 rows) of one 512-thread workgroup.
//   step      the 256 rows a wave takes at a time, four consecutive rows per lane; the next step's rows are in flight over
//             this one.
// The open run travels through a segment as a BkAgg: (position of the last head, 64-bit sum, min, max in the x domain).
// bk_wave_scan is the six-step DPP ladder of wave_inclusive_scan over BkAggs, segmented at the heads.
#pragma once
#include "../../include/dbhip_reduce_by_key.h"
#include "../../include/dbhip_scan_by_key.h"
#include "dbhip_common.hpp"

namespace dbhip {

// one geometry for both: scan-by-key's run numbers are reduce-by-key's rows, and the code below is written once
static_assert(DBHIP_REDUCE_BY_KEY_SEGMENT_ROWS == DBHIP_SCAN_BY_KEY_SEGMENT_ROWS, "one segment size for the by-key kernels");
static_assert(DBHIP_REDUCE_BY_KEY_CHUNK_ROWS == DBHIP_SCAN_BY_KEY_CHUNK_ROWS, "one chunk size for the by-key kernels");

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 bk_ext(unsigned v, bool is_signed) {
  return is_signed ? static_cast<u64>(static_cast<long long>(static_cast<int>(v))) : static_cast<u64>(v);
}
__device__ __forceinline__ unsigned bk_min(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned bk_max(unsigned a, unsigned b) { return a > b ? a : b; }

// this lane's four consecutive rows of a step: 16-byte non-temporal loads in a whole segment, row by row and bounded by
// `last` in the ragged one; vals may be null (zeros)
__device__ __forceinline__ void bk_load(const unsigned *__restrict__ keys, const unsigned *__restrict__ vals, bool full,
                                        size_t row0, size_t last, u32x4 &k, u32x4 &v) {
  if (full) {
    k = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(keys + row0));
    v = vals ? __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(vals + row0)) : u32x4{0u, 0u, 0u, 0u};
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      k[q] = row0 + q < last ? keys[row0 + q] : 0u;
      v[q] = (vals && row0 + q < last) ? vals[row0 + q] : 0u;
    }
  }
}

// the rows from the last head (or from the segment's first row) up to some row: lh = 1 + the head's row inside the
// segment, 0 when there is no head yet; sum, mn, mx over the rows behind that point
struct BkAgg {
  unsigned lh, mn, mx;
  u64 sum;
};
__device__ __forceinline__ BkAgg bk_none() { return BkAgg{0u, 0xFFFFFFFFu, 0u, 0ull}; }
// a = l (+) a: the rows of l directly in front of the rows of a; kSeg = false: a is known to hold no head
template <bool kSeg>
__device__ __forceinline__ void bk_prepend(BkAgg &a, const BkAgg &l) {
  if (!kSeg || a.lh == 0) {
    a.lh = l.lh;
    a.sum += l.sum;
    a.mn = bk_min(a.mn, l.mn);
    a.mx = bk_max(a.mx, l.mx);
  }
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ BkAgg bk_dpp(const BkAgg &a) {  // lanes without a source get bk_none()
  BkAgg l;
  l.lh = __builtin_amdgcn_update_dpp(0u, a.lh, kCtrl, kRowMask, 0xf, false);
  l.mn = __builtin_amdgcn_update_dpp(0xFFFFFFFFu, a.mn, kCtrl, kRowMask, 0xf, false);
  l.mx = __builtin_amdgcn_update_dpp(0u, a.mx, kCtrl, kRowMask, 0xf, false);
  const unsigned lo = __builtin_amdgcn_update_dpp(0u, static_cast<unsigned>(a.sum), kCtrl, kRowMask, 0xf, false);
  const unsigned hi = __builtin_amdgcn_update_dpp(0u, static_cast<unsigned>(a.sum >> 32), kCtrl, kRowMask, 0xf, false);
  l.sum = (static_cast<u64>(hi) << 32) | lo;
  return l;
}
template <bool kSeg, int kCtrl, int kRowMask>
__device__ __forceinline__ void bk_scan_step(BkAgg &a) {
  const BkAgg l = bk_dpp<kCtrl, kRowMask>(a);
  bk_prepend<kSeg>(a, l);
}
// inclusive (segmented) scan over the wave's lanes, the DPP ladder of wave_inclusive_scan
template <bool kSeg>
__device__ __forceinline__ void bk_wave_scan(BkAgg &a) {
  bk_scan_step<kSeg, 0x111, 0xf>(a);  // row_shr:1
  bk_scan_step<kSeg, 0x112, 0xf>(a);  // row_shr:2
  bk_scan_step<kSeg, 0x114, 0xf>(a);  // row_shr:4
  bk_scan_step<kSeg, 0x118, 0xf>(a);  // row_shr:8
  bk_scan_step<kSeg, 0x142, 0xa>(a);  // row_bcast:15 -> rows 1,3
  bk_scan_step<kSeg, 0x143, 0xc>(a);  // row_bcast:31 -> rows 2,3
}

}  // namespace dbhip
