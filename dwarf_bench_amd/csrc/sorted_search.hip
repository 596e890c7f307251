// sorted_search.hip — lower and upper bound of every probe row in a sorted 32-bit column for gfx950, over a fence ladder of
// fan-out 64 (include/dbhip_sorted_search.h).  Behind the stable argsort and in front of join_pairs.hip this is the range
// join b.key BETWEEN p.lo AND p.hi, and with lo == NULL the ASOF join.
//
// No reference counterpart.  The x DOMAIN is the key with its sign bit flipped when the column is signed, so that every
// comparison is unsigned (as radix.hip does on load).  LEVEL 0 is the column, level l+1 holds the last entry of every 64-entry
// BLOCK of level l, in the x domain; the ladder stops at the first level T with at most `top` entries.
//
// All dependent launches, no workgroup ever waits on another (DESIGN.md findings 8 and 9), no CAS loop, every loop bounded by
// the sizes:
//   ss_header  writes the 64 words of the workspace header: a clean status word, the magic, m, top, the sign
//   ss_fence   one launch per level 1..T: F_{l+1}[j] = F_l[min(64 j + 63, m_l - 1)]
//   ss_search  persistent workgroups, two per compute unit (the 64 KiB top level in LDS).  The geometry is worked out again
//              from the header's (m, top), which are checked against the call first: nothing of a foreign workspace is
//              trusted.  Per wave 256 rows at a time, four consecutive rows per lane: binary search in LDS, then per level
//              and row one 256-byte block load from a wave-uniform base, a ballot, a population count, a lane select.  Every
//              step is clamped to its level: b <= m_{l+1} blocks in, the count over the lanes inside the level only.
//   ss_check   the validator: four range-checked reads per row, never a search
//
// workspace: header | level 1 | ... | level T; every part at a 256-byte offset
#include "dbhip_common.hpp"

#include "../../include/dbhip_sorted_search.h"

namespace dbhip {
namespace {

typedef unsigned long long u64;

constexpr unsigned kSsFan = DBHIP_SORTED_SEARCH_FANOUT;
static_assert(kSsFan == kWave, "a block of the ladder is one wave's load");
constexpr unsigned kSsTop = DBHIP_SORTED_SEARCH_TOP;
constexpr unsigned kSsMagic = 0x53534C44u;  // a built index
constexpr int kSsMaxLevels = 6;             // top = 64 and m = 2^31: levels 0..5
constexpr u64 kSsMaxM = 1ull << 31;
constexpr int kSsThreads = 512;
constexpr unsigned kSsWaveRows = 4 * kWave;                         // rows a wave takes at a time
constexpr unsigned kSsTileRows = kSsWaveRows * (kSsThreads / kWave);  // rows a workgroup takes at a time
constexpr int kSsUnroll = 4;  // block loads in flight per wave on the way down

struct SsHeader {
  unsigned status, magic, top, sign;
  u64 m;
  unsigned pad[58];
};
static_assert(sizeof(SsHeader) == kWsHeader, "workspace header size");

// the ladder of (m, top): count[l] entries at byte offset off[l] of the workspace for l = 1..T (level 0 is the column)
struct SsGeometry {
  int T;
  unsigned count[kSsMaxLevels];
  u64 off[kSsMaxLevels];
  u64 total;
};
__host__ __device__ inline bool ss_top_ok(unsigned top) { return top >= 64 && top <= kSsTop && (top & (top - 1)) == 0; }
__host__ __device__ inline SsGeometry ss_geometry(u64 m, unsigned top) {
  SsGeometry g;
  g.T = 0;
  g.count[0] = static_cast<unsigned>(m);  // m <= 2^31
  g.off[0] = 0;
  g.total = kWsHeader;
  for (int l = 1; l < kSsMaxLevels; ++l) {
    g.count[l] = 0;
    g.off[l] = 0;
  }
#pragma unroll
  for (int l = 1; l < kSsMaxLevels; ++l) {  // constant indices: the kernel keeps all of this in scalar registers
    if (g.T == l - 1 && g.count[l - 1] > top) {
      const unsigned next = (g.count[l - 1] + kSsFan - 1) / kSsFan;
      g.T = l;
      g.count[l] = next;
      g.off[l] = g.total;
      g.total += (static_cast<u64>(next) * 4 + kWsAlign - 1) / kWsAlign * kWsAlign;
    }
  }
  return g;
}

// ---- the build ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void ss_header_kernel(unsigned *header, u64 m, unsigned top, unsigned sign) {
  const unsigned t = threadIdx.x;
  unsigned w = 0;
  if (t == 1) w = kSsMagic;
  if (t == 2) w = top;
  if (t == 3) w = sign;
  if (t == 4) w = static_cast<unsigned>(m);
  if (t == 5) w = static_cast<unsigned>(m >> 32);
  header[t] = w;
}

__global__ __launch_bounds__(256) void ss_fence_kernel(const unsigned *__restrict__ below, unsigned m_below, unsigned flip,
                                                        unsigned *__restrict__ fence, unsigned m_fence) {
  const unsigned stride = gridDim.x * 256u;
  for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < m_fence; j += stride) {
    const u64 last = static_cast<u64>(j) * kSsFan + (kSsFan - 1);
    fence[j] = below[last < m_below ? last : m_below - 1] ^ flip;
  }
}

// ---- the search ----------------------------------------------------------------------------------------------------------
// the number of entries of s[0..count) below x (kUpper: not above x); s ascending, at most 15 steps
template <bool kUpper>
__device__ __forceinline__ unsigned ss_lds_bound(const unsigned *s, unsigned count, unsigned first_step, unsigned x) {
  unsigned pos = 0;
  for (unsigned step = first_step; step; step >>= 1) {
    const unsigned p = pos + step;
    if (p <= count) {
      const unsigned e = s[p - 1];
      if (kUpper ? e <= x : e < x) pos = p;
    }
  }
  return pos;
}

// One level down for the wave's 64 rows of one of the four row slots: in, the number of this level's blocks in front of the
// row's bound (<= m_next); out, the number of this level's entries in front of it (<= m_level).
template <bool kL, bool kU>
__device__ __forceinline__ void ss_descend(const unsigned *__restrict__ level, unsigned m_level, unsigned m_next, unsigned flip,
                                           unsigned lane, unsigned xl, unsigned xh, unsigned &il, unsigned &iu) {
  unsigned nl = il, nu = iu;
  for (unsigned r0 = 0; r0 < kWave; r0 += kSsUnroll) {
    unsigned bl[kSsUnroll], bu[kSsUnroll], el[kSsUnroll], eu[kSsUnroll];
#pragma unroll
    for (int u = 0; u < kSsUnroll; ++u) {  // the loads of kSsUnroll rows, all in flight
      bl[u] = kL ? __builtin_amdgcn_readlane(il, r0 + u) : 0u;
      bu[u] = kU ? __builtin_amdgcn_readlane(iu, r0 + u) : 0u;
      el[u] = eu[u] = 0u;
      if (kL) {
        const unsigned at = bl[u] * kSsFan + lane;  // bl < m_next <= 2^25 where it is used
        if (bl[u] < m_next && at < m_level) el[u] = level[at] ^ flip;
      }
      if (kU) {
        if (kL && bu[u] == bl[u]) {  // wave-uniform: both bounds in one block, one load
          eu[u] = el[u];
        } else {
          const unsigned at = bu[u] * kSsFan + lane;
          if (bu[u] < m_next && at < m_level) eu[u] = level[at] ^ flip;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSsUnroll; ++u) {
      if (kL) {
        const unsigned x = __builtin_amdgcn_readlane(xl, r0 + u);
        const bool in = bl[u] < m_next && bl[u] * kSsFan + lane < m_level;  // lanes behind the level's end do not vote
        const unsigned below = static_cast<unsigned>(__popcll(__ballot(in && el[u] < x)));
        const unsigned res = bl[u] < m_next ? bl[u] * kSsFan + below : m_level;
        nl = lane == r0 + u ? res : nl;  // (hipcc has no writelane builtin: a select on the lane id)
      }
      if (kU) {
        const unsigned x = __builtin_amdgcn_readlane(xh, r0 + u);
        const bool in = bu[u] < m_next && bu[u] * kSsFan + lane < m_level;
        const unsigned below = static_cast<unsigned>(__popcll(__ballot(in && eu[u] <= x)));
        const unsigned res = bu[u] < m_next ? bu[u] * kSsFan + below : m_level;
        nu = lane == r0 + u ? res : nu;
      }
    }
  }
  il = nl;
  iu = nu;
}

__device__ __forceinline__ void ss_store4(unsigned *col, size_t row0, size_t n, bool full, const u32x4 w) {
  if (full) {
    *reinterpret_cast<u32x4 *>(col + row0) = w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row0 + q < n) col[row0 + q] = w[q];
  }
}
__device__ __forceinline__ u32x4 ss_load4(const unsigned *col, size_t row0, size_t n, bool full) {
  u32x4 w = {0u, 0u, 0u, 0u};
  if (full) {
    w = *reinterpret_cast<const u32x4 *>(col + row0);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (row0 + q < n) w[q] = col[row0 + q];
  }
  return w;
}

// kL: the lower bound of lo is needed (lo given); kU: the upper bound of hi' is needed (out_cnt given)
template <bool kL, bool kU>
__global__ __launch_bounds__(kSsThreads) void ss_search_kernel(const unsigned *__restrict__ sorted, u64 m,
                                                               const unsigned *__restrict__ lo,
                                                               const unsigned *__restrict__ hi, size_t n,
                                                               unsigned *__restrict__ out_pos, unsigned *__restrict__ out_cnt,
                                                               const unsigned char *ws, u64 ws_bytes) {
  __shared__ unsigned s_top[kSsTop];
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const SsHeader *header = reinterpret_cast<const SsHeader *>(ws);
  const unsigned magic = header->magic, top = header->top;
  const u64 m_built = header->m;
  const unsigned sign = header->sign & 0x80000000u;
  bool mine = magic == kSsMagic && m_built == m && ss_top_ok(top);
  SsGeometry g = ss_geometry(m, mine ? top : kSsTop);
  mine = mine && g.total <= ws_bytes;
  if (!mine) {  // uniform over the grid: not an index of this column.  0 / 0 in every row, one status bit, nothing else read
    const size_t stride = static_cast<size_t>(gridDim.x) * kSsThreads;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kSsThreads + threadIdx.x; i < n; i += stride) {
      if (out_pos) out_pos[i] = 0u;
      if (out_cnt) out_cnt[i] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
      atomicOr(const_cast<unsigned *>(&header->status), static_cast<unsigned>(DBHIP_DEV_KEY_RANGE));
    return;
  }
  const int T = g.T;
  unsigned m_top = 0;  // <= top <= kSsTop
  u64 off_top = 0;
#pragma unroll
  for (int k = 0; k < kSsMaxLevels; ++k) {  // (constant indices into g, here and below: no scratch)
    if (k == T) {
      m_top = g.count[k];
      off_top = g.off[k];
    }
  }
  {
    const unsigned *src = T ? reinterpret_cast<const unsigned *>(ws + off_top) : sorted;
    const unsigned flip = T ? 0u : sign;
    for (unsigned i = threadIdx.x; i < m_top; i += kSsThreads) s_top[i] = src[i] ^ flip;
  }
  __syncthreads();
  unsigned first_step = 1;
  while (first_step * 2 <= m_top) first_step *= 2;
  if (m_top == 0) first_step = 0;

  for (size_t tile = static_cast<size_t>(blockIdx.x) * kSsTileRows; tile < n;
       tile += static_cast<size_t>(gridDim.x) * kSsTileRows) {
    const size_t base = tile + static_cast<size_t>(wave) * kSsWaveRows;
    if (base >= n) continue;  // uniform over the wave; no barrier in this loop
    const bool full = base + kSsWaveRows <= n;
    const size_t row0 = base + 4 * lane;
    u32x4 xl = {0u, 0u, 0u, 0u}, xh;
    if (kL) xl = ss_load4(lo, row0, n, full) ^ sign;
    xh = hi ? ss_load4(hi, row0, n, full) ^ sign : xl;
    unsigned il[4], iu[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool valid = full || row0 + q < n;
      // a row behind the column's end stands behind every block of every level: it is never loaded for
      il[q] = kL ? (valid ? ss_lds_bound<false>(s_top, m_top, first_step, xl[q]) : m_top) : 0u;
      iu[q] = kU ? (valid ? ss_lds_bound<true>(s_top, m_top, first_step, xh[q]) : m_top) : 0u;
    }
    for (int l = T - 1; l >= 0; --l) {
      unsigned m_level = 0, m_next = 0;
      u64 off = 0;
#pragma unroll
      for (int k = 0; k + 1 < kSsMaxLevels; ++k) {
        if (k == l) {
          m_level = g.count[k];
          m_next = g.count[k + 1];
          off = g.off[k];
        }
      }
      const unsigned *level = l ? reinterpret_cast<const unsigned *>(ws + off) : sorted;
      const unsigned flip = l ? 0u : sign;
#pragma unroll
      for (int q = 0; q < 4; ++q) ss_descend<kL, kU>(level, m_level, m_next, flip, lane, xl[q], xh[q], il[q], iu[q]);
    }
    u32x4 w_pos, w_cnt;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w_pos[q] = kL ? il[q] : 0u;
      w_cnt[q] = kU ? (iu[q] > w_pos[q] ? iu[q] - w_pos[q] : 0u) : 0u;
    }
    if (out_pos) ss_store4(out_pos, row0, n, full, w_pos);
    if (kU) ss_store4(out_cnt, row0, n, full, w_cnt);
  }
}

// ---- the validator -------------------------------------------------------------------------------------------------------
constexpr int kSsCheckThreads = 256;

__global__ __launch_bounds__(kSsCheckThreads) void ss_check_kernel(const unsigned *__restrict__ sorted, u64 m, unsigned sign,
                                                                   const unsigned *__restrict__ lo,
                                                                   const unsigned *__restrict__ hi, size_t n,
                                                                   const unsigned *__restrict__ pos,
                                                                   const unsigned *__restrict__ cnt, u64 *result) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kSsCheckThreads;
  u64 faults = 0, pairs = 0, lowest = ~0ull;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kSsCheckThreads + threadIdx.x; i < n; i += stride) {
    const unsigned xl = lo ? lo[i] ^ sign : 0u;
    const unsigned xh = hi ? hi[i] ^ sign : xl;
    const u64 p = pos ? pos[i] : 0ull;
    unsigned bad = 0;
    if (pos) {
      bool ok = p <= m;
      if (ok && !lo) ok = p == 0;
      if (ok && lo) ok = (p == 0 || (sorted[p - 1] ^ sign) < xl) && (p == m || (sorted[p] ^ sign) >= xl);
      bad += ok ? 0u : 1u;
    }
    if (cnt) {
      const u64 c = cnt[i], e = p + c;
      pairs += c;
      bool ok = e <= m;
      if (ok && lo && xh < xl) {
        ok = c == 0;
      } else if (ok) {
        ok = (e == 0 || (sorted[e - 1] ^ sign) <= xh) && (e == m || (sorted[e] ^ sign) > xh);
      }
      bad += ok ? 0u : 1u;
    }
    faults += bad;
    if (bad && i < lowest) lowest = i;
  }
  faults = wave_reduce_add_u64(faults);
  pairs = wave_reduce_add_u64(pairs);
  if (faults) {  // uniform over the wave: faults is the wave's sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 other = __shfl_xor(lowest, off, kWave);
      lowest = other < lowest ? other : lowest;
    }
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (faults) {
      atomicAdd(result + 0, faults);
      atomicMin(result + 1, lowest);
    }
    if (pairs) atomicAdd(result + 2, pairs);
  }
}

// the argument rules the search and its validator share, in the header's order (the alignment rule is the search's alone)
inline bool ss_args_bad(const uint32_t *sorted, size_t m, const uint32_t *lo, const uint32_t *hi, size_t n, const void *pos,
                        const void *cnt) {
  if (m > kSsMaxM || n >= (1ull << 32)) return true;
  if (!lo && !hi) return true;
  if (!pos && !cnt) return true;
  if (hi && !cnt) return true;
  return false;
}

}  // namespace
}  // namespace dbhip

using namespace dbhip;

extern "C" size_t dbhip_sorted_index_workspace_bytes(size_t m, uint32_t top_entries) {
  const unsigned top = top_entries ? top_entries : kSsTop;
  if (m > kSsMaxM || !ss_top_ok(top)) return 0;
  return static_cast<size_t>(ss_geometry(m, top).total);
}

extern "C" int dbhip_sorted_index_build_u32(const uint32_t *sorted, size_t m, int keys_signed, uint32_t top_entries,
                                            void *workspace, size_t workspace_bytes, dbhip_stream_t stream) {
  const unsigned top = top_entries ? top_entries : kSsTop;
  if (m > kSsMaxM) return DBHIP_EINVAL;
  if (!ss_top_ok(top)) return DBHIP_EINVAL;
  if (m && !sorted) return DBHIP_EINVAL;
  const SsGeometry g = ss_geometry(m, top);
  if (!ws_ok(workspace, workspace_bytes, g.total)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  const unsigned sign = keys_signed ? 0x80000000u : 0u;
  char *base = static_cast<char *>(workspace);
  hipLaunchKernelGGL(ss_header_kernel, dim3(1), dim3(kWave), 0, s, reinterpret_cast<unsigned *>(base),
                     static_cast<u64>(m), top, sign);
  for (int l = 1; l <= g.T; ++l) {
    const unsigned *below = l == 1 ? sorted : reinterpret_cast<const unsigned *>(base + g.off[l - 1]);
    hipLaunchKernelGGL(ss_fence_kernel, dim3(capped_grid(g.count[l], 256, dev)), dim3(256), 0, s, below, g.count[l - 1],
                       l == 1 ? sign : 0u, reinterpret_cast<unsigned *>(base + g.off[l]), g.count[l]);
  }
  return launch_status();
}

extern "C" int dbhip_sorted_search_u32(const uint32_t *sorted, size_t m, const uint32_t *lo, const uint32_t *hi, size_t n,
                                       uint32_t *out_pos, uint32_t *out_cnt, const void *workspace, size_t workspace_bytes,
                                       dbhip_stream_t stream) {
  if (ss_args_bad(sorted, m, lo, hi, n, out_pos, out_cnt)) return DBHIP_EINVAL;
  if (m && n && !sorted) return DBHIP_EINVAL;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(hi) |
                         reinterpret_cast<uintptr_t>(out_pos) | reinterpret_cast<uintptr_t>(out_cnt);
  if (addr & 15u) return DBHIP_EINVAL;  // dbhip_sorted_search.h: 16-byte aligned
  if (!ws_ok(workspace, workspace_bytes, ss_geometry(m, kSsTop).total)) return DBHIP_EWORKSPACE;
  if (n == 0) return DBHIP_OK;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  const size_t tiles = (n + kSsTileRows - 1) / kSsTileRows;
  const size_t resident = static_cast<size_t>(dev.cus) * 2;  // 64 KiB of LDS each
  const dim3 grid(static_cast<unsigned>(tiles < resident ? tiles : resident)), block(kSsThreads);
  const unsigned char *ws = static_cast<const unsigned char *>(workspace);
  const u64 wsb = workspace_bytes;
  if (lo && out_cnt) {
    hipLaunchKernelGGL((ss_search_kernel<true, true>), grid, block, 0, s, sorted, static_cast<u64>(m), lo, hi, n, out_pos,
                       out_cnt, ws, wsb);
  } else if (lo) {
    hipLaunchKernelGGL((ss_search_kernel<true, false>), grid, block, 0, s, sorted, static_cast<u64>(m), lo, hi, n, out_pos,
                       out_cnt, ws, wsb);
  } else {
    hipLaunchKernelGGL((ss_search_kernel<false, true>), grid, block, 0, s, sorted, static_cast<u64>(m), lo, hi, n, out_pos,
                       out_cnt, ws, wsb);
  }
  return launch_status();
}

extern "C" size_t dbhip_check_sorted_search_workspace_bytes(size_t n) {
  if (n >= (1ull << 32)) return 0;
  return kWsHeader;
}

extern "C" int dbhip_check_sorted_search_u32(const uint32_t *sorted, size_t m, int keys_signed, const uint32_t *lo,
                                             const uint32_t *hi, size_t n, const uint32_t *pos, const uint32_t *cnt,
                                             uint64_t *result, void *workspace, size_t workspace_bytes,
                                             dbhip_stream_t stream) {
  if (!result || (reinterpret_cast<uintptr_t>(result) & 7u)) return DBHIP_EINVAL;
  if (ss_args_bad(sorted, m, lo, hi, n, pos, cnt)) return DBHIP_EINVAL;
  if (!pos && lo && cnt) return DBHIP_EINVAL;
  if (m && n && !sorted) return DBHIP_EINVAL;
  if (!ws_ok(workspace, workspace_bytes, kWsHeader)) return DBHIP_EWORKSPACE;
  const DeviceInfo &dev = current_device_info();
  if (!dev.ok) return DBHIP_ENODEVICE;
  hipStream_t s = as_stream(stream);
  hipError_t e = fill_async(workspace, 0, kWsHeader, s);
  if (e != hipSuccess) return static_cast<int>(e);
  e = fill_async(result, 0, 4 * sizeof(uint64_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  e = fill_async(result + 1, 0xFF, sizeof(uint64_t), s);  // no violating row yet
  if (e != hipSuccess) return static_cast<int>(e);
  if (n) {
    hipLaunchKernelGGL(ss_check_kernel, dim3(capped_grid(n, kSsCheckThreads, dev)), dim3(kSsCheckThreads), 0, s, sorted,
                       static_cast<u64>(m), keys_signed ? 0x80000000u : 0u, lo, hi, n, pos, cnt,
                       reinterpret_cast<u64 *>(result));
  }
  return launch_status();
}
