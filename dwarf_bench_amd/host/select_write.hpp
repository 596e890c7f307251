// select_write.hpp — the segment shape and the write kernel of the selection vectors, for the files that mark candidates in
// select's mask layout (select_rows.hpp): select_rows.cpp (range predicate) and bloom_filter.cpp (Bloom filter test).  Each
// of them instantiates the kernel in its own anonymous namespace; the instruction text in select_rows.cpp is the one it had
// when the kernel lived there (profiles/r24_bloom_isa.txt).
#pragma once
#include "rowlist.hpp"
#include "select_rows.hpp"

namespace {
using namespace dbhip;

constexpr unsigned kSelSegment = DBENCH_SELECT_SEGMENT_ROWS;
// segments of a workgroup.  No kernel here uses LDS or a barrier, so the number only decides how a short list spreads
// over the compute units: lists of 2^20 rows out of 2^26 took 82-91 us with eight and 57-66 us with two, the dense
// stream of 2^26 rows the same 77-82 us with either
constexpr int kSelWaves = 2;
constexpr int kSelThreads = kSelWaves * kWave;
constexpr int kSelGroups = kSelSegment / (4 * kWave);  // groups of 256 candidates: four per lane
constexpr int kSelWords = kSelSegment / kWave;         // mask words of a segment, one per lane
static_assert(kSelWords == kWave && kSelGroups * 4 == kSelWords, "a lane keeps one mask word of its wave's segment");

struct SelLayout {
  size_t segments, cnt, pos, masks, total;
};

inline SelLayout sel_layout(size_t candidates) {
  SelLayout l;
  l.segments = (candidates + kSelSegment - 1) / kSelSegment + 1;  // + 1: the up to three words in front of the first
  const size_t words = align_up(sizeof(unsigned) * l.segments, kWsAlign);
  l.cnt = kWsHeader;
  l.pos = l.cnt + words;
  l.masks = l.pos + words;
  l.total = l.masks + sizeof(unsigned long long) * kSelWords * l.segments;
  return l;
}

// a wave writes its segment's kept row ids, in candidate order, from pos[segment] on
template <bool kList>
__global__ __launch_bounds__(kSelThreads) void sel_write_kernel(const unsigned *__restrict__ rows, size_t capacity, unsigned a,
                                                                const unsigned *__restrict__ cnt,
                                                                const unsigned *__restrict__ pos,
                                                                const unsigned long long *__restrict__ masks,
                                                                size_t segments, unsigned *__restrict__ out,
                                                                size_t out_capacity) {
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const size_t seg = static_cast<size_t>(blockIdx.x) * kSelWaves + wave;
  if (seg >= segments) return;  // uniform over the wave; no barrier below
  const unsigned c = cnt[seg];
  if (c == 0) return;  // nothing kept in this segment: neither its masks nor its row ids are read
  size_t run = pos[seg];  // next output position (wave-uniform)
  const size_t end = run + c;
  if (end > out_capacity) return;  // cannot happen with this call's own counts; nothing is ever written past the buffer
  const unsigned long long mine = masks[seg * kSelWords + lane];
  const unsigned mine_lo = static_cast<unsigned>(mine), mine_hi = static_cast<unsigned>(mine >> 32);
  const size_t vfirst = seg * kSelSegment;
#pragma unroll 1
  for (int g = 0; g < kSelGroups; ++g) {
    unsigned long long b[4];
    unsigned in_group = 0, before = 0, k = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // (the builtin returns int: through unsigned, or the low half's sign bit would fill the high half)
      const unsigned b_lo = __builtin_amdgcn_readlane(mine_lo, 4 * g + q), b_hi = __builtin_amdgcn_readlane(mine_hi, 4 * g + q);
      b[q] = b_lo | static_cast<unsigned long long>(b_hi) << 32;
      in_group += static_cast<unsigned>(__popcll(b[q]));
      before += mbcnt(b[q]);  // lower lanes hold earlier candidates, whatever their q
      k |= static_cast<unsigned>((b[q] >> lane) & 1ull) << q;
    }
    if (in_group == 0) continue;  // uniform
    if (k) {
      const size_t v0 = vfirst + static_cast<size_t>(g) * (4 * kWave) + 4 * lane;
      unsigned id[4];
      if (!kList) {
#pragma unroll
        for (int q = 0; q < 4; ++q) id[q] = static_cast<unsigned>(v0 + q - a);
      } else if (v0 >= a && v0 + 4 - a <= capacity) {
        const u32x4 e = *reinterpret_cast<const u32x4 *>(rows + (v0 - a));
        id[0] = e.x, id[1] = e.y, id[2] = e.z, id[3] = e.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) id[q] = (v0 + q >= a && v0 + q - a < capacity) ? rows[v0 + q - a] : 0u;
      }
      size_t at = run + before;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((k >> q) & 1u) {
          if (at < end) out[at] = id[q];
          ++at;
        }
      }
    }
    run += in_group;
  }
}

}  // namespace
