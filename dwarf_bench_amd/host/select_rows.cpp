// select_rows.cpp — selection vectors on gfx950 (select_rows.hpp holds the contract and the workspace layout): stable
// compaction of row ids under a range predicate on a 32-bit column, over all rows or over a row-id list.
//
// Three dependent launches behind the clear of the workspace header; no workgroup ever waits for another (the shape of
// tk_count_kernel / tk_scan_kernel / tk_write_kernel in csrc/topk.hip):
//   mark   a wave owns one segment of 4096 candidate positions, a workgroup two of them.  A lane holds four
//          consecutive candidates per group of 256 (one 16-byte load of the column, or of the row ids followed by four
//          4-byte gathers), evaluates the predicate and ballots it; the 64 ballots of the segment are its match mask
//          (one coalesced 512-byte store) and their population count is the segment's match count.
//   scan   one workgroup: counts -> first output positions, and *out_count (launch_rowlist_scan).
//   write  a wave whose segment has matches reads the masks back (not the column), ranks every match with mbcnt over
//          the group's four ballots plus the wave's running position, and stores the row ids.
// Positions are counted from the 16-byte boundary in front of the column (or the list): candidate i sits at v = i + a,
// a = 0..3 words, so every 16-byte load is aligned whatever the pointer's alignment; the two vectors that straddle the
// ends of the array are read word by word, and nothing outside the arrays is touched.  The predicate, the ragged load,
// the device count, the scan and the host checks are those of every row-id operator (rowlist.hpp, call_checks.hpp).
#include "select_rows.hpp"

#include "rowlist.hpp"
#include "select_write.hpp"  // the segment shape, the workspace layout, sel_write_kernel

namespace {
using namespace dbhip;

// kList: `src` is the row-id list (gathered through into col), otherwise the column itself.  m_host candidates at
// most (n_col in dense mode); in list mode *in_count (nullable) lowers it on the device.
template <bool kList>
__global__ __launch_bounds__(kSelThreads) void sel_mark_kernel(const unsigned *__restrict__ col, unsigned n_col,
                                                               const unsigned *__restrict__ src, size_t m_host,
                                                               const unsigned long long *in_count, unsigned a, RangePred p,
                                                               unsigned *status, unsigned *__restrict__ cnt,
                                                               unsigned long long *__restrict__ masks, size_t segments) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSelWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const size_t m = kList ? clamped_count(in_count, m_host) : m_host;
  const size_t vfirst = seg * kSelSegment, vend = a + m;  // positions [a, vend) hold candidates
  unsigned long long mine = 0;  // mask word `lane` of the segment
  unsigned total = 0;           // matches of the segment (wave-uniform)
  bool bad = false;             // a row id >= n_col among this lane's candidates

  // a group in two steps, so that a caller can have the gathers of several groups in flight before the first ballot.
  // fetch: the lane's four entries e (bit q of `valid`: entry q is a candidate) -> the values x the predicate sees and
  // the candidates `ok` that count.  List mode: the gather is unconditional — row 0 stands in for an entry that does
  // not count — so the four loads are independent of each other and of the votes in front of them.
  auto fetch = [&](const u32x4 e, unsigned valid, unsigned (&x)[4], unsigned &ok) {
    const unsigned w[4] = {e.x, e.y, e.z, e.w};
    ok = valid;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = w[q];
    if (kList) {
      unsigned row[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool inside = w[q] < n_col;
        bad = bad || (((valid >> q) & 1u) && !inside);
        if (!inside) ok &= ~(1u << q);
        row[q] = ((ok >> q) & 1u) ? w[q] : 0u;
      }
      if (n_col) {  // uniform; an empty column has no row 0, and no candidate that counts
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = col[row[q]];
      }
    }
  };
  auto vote = [&](int g, const unsigned (&x)[4], unsigned ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long b = __ballot(((ok >> q) & 1u) && range_keep(x[q], p));
      total += static_cast<unsigned>(__popcll(b));
      if (lane == static_cast<unsigned>(4 * g + q)) mine = b;
    }
  };
  auto group = [&](int g, const u32x4 e, unsigned valid) {
    unsigned x[4], ok;
    fetch(e, valid, x, ok);
    vote(g, x, ok);
  };

  if (vfirst >= vend) {
    // a segment behind the last candidate (the list is shorter than its capacity): zero count, zero masks
  } else if (vfirst >= a && vfirst + kSelSegment <= vend) {  // a whole segment: 16 aligned 16-byte loads per lane
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src + (vfirst - a)) + lane;
#pragma unroll 1
    for (int g = 0; g < kSelGroups; g += 4) {  // four loads in flight, and in list mode then their sixteen gathers
      const u32x4 v0 = s4[g * kWave], v1 = s4[(g + 1) * kWave], v2 = s4[(g + 2) * kWave], v3 = s4[(g + 3) * kWave];
      unsigned x0[4], x1[4], x2[4], x3[4], ok0, ok1, ok2, ok3;
      fetch(v0, 0xfu, x0, ok0);
      fetch(v1, 0xfu, x1, ok1);
      fetch(v2, 0xfu, x2, ok2);
      fetch(v3, 0xfu, x3, ok3);
      vote(g, x0, ok0);
      vote(g + 1, x1, ok1);
      vote(g + 2, x2, ok2);
      vote(g + 3, x3, ok3);
    }
  } else {  // the first segment of an array that starts off a 16-byte boundary, and the ragged last one
#pragma unroll 1
    for (int g = 0; g < kSelGroups; ++g) {
      const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
      // load_ragged's text (rowlist.hpp), a deliberate copy: through the call sel_mark_kernel<true> comes out with the
      // operands of four s_and_b64 exchanged, and the rule is same instruction text or the parent's body
      u32x4 e = {0u, 0u, 0u, 0u};
      unsigned valid = 0;
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
      group(g, e, valid);
    }
  }
  masks[seg * kSelWords + lane] = mine;
  if (lane == 0) cnt[seg] = total;
  if (kList && __ballot(bad) != 0 && lane == 0) atomicOr(status, DBHIP_DEV_KEY_RANGE);
}

}  // namespace

extern "C" size_t dbench_select_workspace_bytes(size_t candidates) {
  if (!fits_32(candidates)) return 0;
  return sel_layout(candidates).total;
}

extern "C" int dbench_select_range_u32(const uint32_t *col, size_t n_col, const uint32_t *in_rows, const uint64_t *in_count,
                                       size_t in_capacity, uint32_t lo, uint32_t hi, int flags, uint32_t *out_rows,
                                       uint64_t *out_count, void *workspace, size_t workspace_bytes, void *stream) {
  if (flags & ~(DBENCH_SELECT_SIGNED | DBENCH_SELECT_NEGATE)) return DBHIP_EINVAL;
  if (!fits_32(n_col) || !fits_32(in_capacity)) return DBHIP_EINVAL;  // 32-bit row ids and counts
  if ((n_col && !col) || !out_count || (in_count && !in_rows)) return DBHIP_EINVAL;
  if (((addr(col) | addr(in_rows) | addr(out_rows)) & 3u) || ((addr(in_count) | addr(out_count)) & 7u)) return DBHIP_EINVAL;
  const bool list = in_rows != nullptr;
  const size_t candidates = list ? in_capacity : n_col;
  if (overlap(out_rows, 4 * candidates, col, 4 * n_col) || overlap(out_rows, 4 * candidates, in_rows, 4 * in_capacity))
    return DBHIP_EINVAL;
  const SelLayout l = sel_layout(candidates);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, l.total, s);
  if (rc != DBHIP_OK) return rc;

  char *base = static_cast<char *>(workspace);
  unsigned *status = reinterpret_cast<unsigned *>(base);
  unsigned *cnt = reinterpret_cast<unsigned *>(base + l.cnt);
  unsigned *pos = reinterpret_cast<unsigned *>(base + l.pos);
  unsigned long long *masks = reinterpret_cast<unsigned long long *>(base + l.masks);
  unsigned long long *total = reinterpret_cast<unsigned long long *>(out_count);

  const unsigned a = candidates ? words_past_16(list ? in_rows : col) : 0u;
  const size_t segments = candidates ? (candidates + a + kSelSegment - 1) / kSelSegment : 0;  // <= l.segments
  const unsigned grid = static_cast<unsigned>((segments + kSelWaves - 1) / kSelWaves);
  const unsigned flip = (flags & DBENCH_SELECT_SIGNED) ? 0x80000000u : 0u;
  const RangePred p{flip, lo ^ flip, hi ^ flip, (flags & DBENCH_SELECT_NEGATE) != 0};
  if (segments) {
    if (list)
      hipLaunchKernelGGL((sel_mark_kernel<true>), dim3(grid), dim3(kSelThreads), 0, s, col, static_cast<unsigned>(n_col),
                         in_rows, in_capacity, reinterpret_cast<const unsigned long long *>(in_count), a, p, status, cnt,
                         masks, segments);
    else
      hipLaunchKernelGGL((sel_mark_kernel<false>), dim3(grid), dim3(kSelThreads), 0, s, col, static_cast<unsigned>(n_col),
                         col, n_col, static_cast<const unsigned long long *>(nullptr), a, p, status, cnt, masks, segments);
  }
  launch_rowlist_scan(cnt, pos, segments, candidates, total, s);  // the write kernels stop at `candidates` as well
  if (segments && out_rows) {
    if (list)
      hipLaunchKernelGGL((sel_write_kernel<true>), dim3(grid), dim3(kSelThreads), 0, s, in_rows, in_capacity, a, cnt, pos,
                         masks, segments, out_rows, candidates);
    else
      hipLaunchKernelGGL((sel_write_kernel<false>), dim3(grid), dim3(kSelThreads), 0, s,
                         static_cast<const unsigned *>(nullptr), n_col, a, cnt, pos, masks, segments, out_rows, candidates);
  }
  return launch_status();
}
