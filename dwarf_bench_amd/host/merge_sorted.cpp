// merge_sorted.cpp — merge path on gfx950 (merge_sorted.hpp holds the contract and the workspace layout; merge_path.hpp
// the diagonal search, the clamped tile extents and the serial merge, shared with tests/cpp/merge_path_check.cpp): the
// stable merge of two sorted (key, value) columns, and union / intersection / difference of two strictly ascending lists.
//
// Dependent launches behind the clear of the workspace header; no workgroup ever waits for another:
//   partition  one thread per tile boundary i: the number of A elements in front of diagonal i * T of the merged order,
//              by binary search over A and B in global memory, after reading the device counts.
//   tile body  (mp_tile_load + mp_thread_merge) a workgroup owns T merged positions.  It clamps its two partition
//              points to extents that add up to the tile, loads its at most T elements of A and B into LDS (aligned
//              16-byte loads in the body, the ragged ends word by word), and every thread searches its own diagonal
//              in LDS and merges its kItems elements serially in registers.
//   merge      the tile body; keys and source indices go back through LDS so that the global stores are coalesced;
//              values are then gathered by source index (consecutive outputs come from at most two consecutive runs
//              of the inputs), or are the row ids themselves.
//   count / scan / write  the set operations: the tile body with a keep flag per merged element -> kept per tile ->
//              first output position per tile and *out_count (one workgroup, launch_rowlist_scan of rowlist.hpp) -> the
//              tile body again, the kept keys compacted through LDS and stored.
// The keep flag is local to the element because A stands first on ties and the lists are strict: an A element met
// with B's cursor at j has a partner iff j < cb and B[j] equals it; a B element met with A's cursor at i has one iff
// i > 0 and A[i - 1] equals it.  The two neighbours that may lie in another tile (A[a0 - 1] and B[b0 + bn]) are read
// from global memory into two halo words of the LDS image.
#include "merge_sorted.hpp"

#include "merge_path.hpp"
#include "rowlist.hpp"

namespace {
using namespace dbhip;

constexpr unsigned kMpTile = DBENCH_MERGE_TILE_ROWS;
constexpr int kMpThreads = 256;
constexpr int kMpItems = kMpTile / kMpThreads;  // a thread's merged elements
static_assert(kMpItems == 8 && kMpItems * kMpThreads == kMpTile, "a thread stores its items as two 16-byte vectors");
static_assert(kMpTile <= 65536, "source indices inside a tile are 16 bits");

enum { kKeysOnly = 0, kCarried = 1, kRowIds = 2 };

struct MpLayout {
  size_t tiles, part, cnt, pos, total;
};

MpLayout mp_layout(size_t rows) {
  MpLayout l;
  l.tiles = (rows + kMpTile - 1) / kMpTile;
  l.part = kWsHeader;
  l.cnt = l.part + align_up(sizeof(unsigned) * (l.tiles + 1), kWsAlign);
  l.pos = l.cnt + align_up(sizeof(unsigned) * l.tiles, kWsAlign);
  l.total = l.pos + align_up(sizeof(unsigned) * l.tiles, kWsAlign);
  return l;
}

__device__ __forceinline__ unsigned mp_count(const unsigned long long *given, unsigned capacity) {
  return static_cast<unsigned>(clamped_count(given, capacity));
}

__global__ __launch_bounds__(kMpThreads) void mp_partition_kernel(const unsigned *__restrict__ a,
                                                                  const unsigned long long *a_count, unsigned a_capacity,
                                                                  const unsigned *__restrict__ b,
                                                                  const unsigned long long *b_count, unsigned b_capacity,
                                                                  unsigned flip, unsigned *__restrict__ part, unsigned tiles,
                                                                  unsigned long long *merged_count) {
  const unsigned i = blockIdx.x * kMpThreads + threadIdx.x;
  if (i > tiles) return;
  const unsigned ca = mp_count(a_count, a_capacity), cb = mp_count(b_count, b_capacity);
  const unsigned total = ca + cb;  // the capacities add up to less than 2^32
  const unsigned long long d = static_cast<unsigned long long>(i) * kMpTile;
  part[i] = mp_diagonal(a, ca, b, cb, d < total ? static_cast<unsigned>(d) : total, flip);
  if (i == 0 && merged_count) *merged_count = total;
}

// n words from src (any 4-byte alignment) into LDS: vectors counted from the 16-byte boundary in front of src, the
// whole ones by a 16-byte load, the two that straddle the ends word by word; nothing outside src[0, n) is read
__device__ __forceinline__ void mp_load_run(unsigned *dst, const unsigned *__restrict__ src, unsigned n) {
  const unsigned m = static_cast<unsigned>((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
  const unsigned vectors = (m + n + 3) / 4;
  for (unsigned v = threadIdx.x; v < vectors; v += kMpThreads) {
    const unsigned at = 4 * v;  // position of the vector's first word, counted from the boundary: word at - m of src
    if (at >= m && at - m + 4 <= n) {
      const u32x4 e = *reinterpret_cast<const u32x4 *>(src + (at - m));
      dst[at - m] = e.x, dst[at - m + 1] = e.y, dst[at - m + 2] = e.z, dst[at - m + 3] = e.w;
    } else {
#pragma unroll
      for (unsigned q = 0; q < 4; ++q)
        if (at + q >= m && at + q - m < n) dst[at + q - m] = src[at + q - m];
    }
  }
}

struct MpWork {
  unsigned ca, cb, diag0, count;  // the tile's first merged position and its merged elements (1 .. kMpTile)
  MpTile e;
};

// LDS image of a tile: s[0] = A[a0 - 1] (halo), s[1 .. 1 + an) = A's part, s[1 + an .. 1 + count) = B's part,
// s[1 + count] = B[b0 + bn] (halo); a halo that does not exist holds 0 and is never compared.
// -> false (uniform over the workgroup, before any barrier): the tile lies behind the merged count
template <bool kHalo>
__device__ __forceinline__ bool mp_tile_load(const unsigned *__restrict__ a, const unsigned long long *a_count,
                                             unsigned a_capacity, const unsigned *__restrict__ b,
                                             const unsigned long long *b_count, unsigned b_capacity,
                                             const unsigned *__restrict__ part, unsigned *s, MpWork &w) {
  w.ca = mp_count(a_count, a_capacity), w.cb = mp_count(b_count, b_capacity);
  const unsigned total = w.ca + w.cb;
  const unsigned long long d0 = static_cast<unsigned long long>(blockIdx.x) * kMpTile;
  if (d0 >= total) return false;
  w.diag0 = static_cast<unsigned>(d0);
  w.count = total - w.diag0 < kMpTile ? total - w.diag0 : kMpTile;
  w.e = mp_tile_extents(part[blockIdx.x], part[blockIdx.x + 1], w.diag0, w.diag0 + w.count, w.ca, w.cb);
  mp_load_run(s + 1, a + w.e.a0, w.e.an);
  mp_load_run(s + 1 + w.e.an, b + w.e.b0, w.e.bn);
  if (kHalo && threadIdx.x == 0) {
    s[0] = w.e.a0 > 0 ? a[w.e.a0 - 1] : 0u;
    s[1 + w.count] = w.e.b0 + w.e.bn < w.cb ? b[w.e.b0 + w.e.bn] : 0u;
  }
  __syncthreads();
  return true;
}

// the calling thread's part of the tile: emit(k, from_a, i, j, key) as mp_serial_merge gives them, i and j counted
// from the tile's a0 and b0
template <class Emit>
__device__ __forceinline__ void mp_thread_merge(const unsigned *s, const MpWork &w, unsigned flip, Emit &&emit) {
  const unsigned *sa = s + 1, *sb = s + 1 + w.e.an;
  const unsigned first = threadIdx.x * kMpItems;
  const unsigned d = first < w.count ? first : w.count;
  const unsigned items = w.count - d < static_cast<unsigned>(kMpItems) ? w.count - d : kMpItems;
  const unsigned ai = mp_diagonal(sa, w.e.an, sb, w.e.bn, d, flip);
  mp_serial_merge<kMpItems>(sa, ai, w.e.an, sb, d - ai, w.e.bn, flip, items, emit);
}

template <int kMode>
__global__ __launch_bounds__(kMpThreads) void mp_merge_kernel(const unsigned *__restrict__ a_keys,
                                                              const unsigned *__restrict__ a_vals,
                                                              const unsigned long long *a_count, unsigned a_capacity,
                                                              const unsigned *__restrict__ b_keys,
                                                              const unsigned *__restrict__ b_vals,
                                                              const unsigned long long *b_count, unsigned b_capacity,
                                                              unsigned flip, const unsigned *__restrict__ part,
                                                              unsigned *__restrict__ out_keys,
                                                              unsigned *__restrict__ out_vals) {
  __shared__ __attribute__((aligned(16))) unsigned s[kMpTile + 4];
  __shared__ __attribute__((aligned(16))) unsigned short s_src[kMpTile];
  MpWork w;
  if (!mp_tile_load<false>(a_keys, a_count, a_capacity, b_keys, b_count, b_capacity, part, s, w)) return;
  unsigned key[kMpItems];
  unsigned short src[kMpItems];  // below an: A's row a0 + src, otherwise B's row b0 + src - an
#pragma unroll
  for (int k = 0; k < kMpItems; ++k) key[k] = 0u, src[k] = 0;
  const unsigned an = w.e.an;
  mp_thread_merge(s, w, flip, [&](int k, bool from_a, unsigned i, unsigned j, unsigned x) {
    key[k] = x;
    src[k] = static_cast<unsigned short>(from_a ? i : an + j);
  });
  __syncthreads();  // every thread has read its part of the image: the merged tile takes its place
  u32x4 *s4 = reinterpret_cast<u32x4 *>(s) + 2 * threadIdx.x;
  s4[0] = u32x4{key[0], key[1], key[2], key[3]};
  s4[1] = u32x4{key[4], key[5], key[6], key[7]};
  if (kMode != kKeysOnly) {
    reinterpret_cast<u32x4 *>(s_src)[threadIdx.x] =
        u32x4{src[0] | unsigned(src[1]) << 16, src[2] | unsigned(src[3]) << 16, src[4] | unsigned(src[5]) << 16,
              src[6] | unsigned(src[7]) << 16};
  }
  __syncthreads();
  unsigned *ok = out_keys + w.diag0, *ov = out_vals + w.diag0;  // w.diag0 + w.count <= ca + cb
#pragma unroll
  for (int k = 0; k < kMpItems; ++k) {
    const unsigned p = k * kMpThreads + threadIdx.x;
    if (p < w.count) {
      ok[p] = s[p];
      if (kMode != kKeysOnly) {
        const unsigned from = s_src[p];  // from < an + bn, so the rows below are inside [0, ca) and [0, cb)
        const bool from_a = from < an;
        const unsigned row = from_a ? w.e.a0 + from : w.e.b0 + (from - an);
        if (kMode == kRowIds)
          ov[p] = from_a ? row : a_capacity + row;
        else
          ov[p] = from_a ? a_vals[row] : b_vals[row];
      }
    }
  }
}

__device__ __forceinline__ bool mp_keep(int op, bool from_a, bool partner) {
  return op == DBENCH_SETOP_UNION ? (from_a || !partner) : (from_a && partner == (op == DBENCH_SETOP_INTERSECT));
}

// kWrite false: cnt[tile] = kept elements of the tile (0 for a tile behind the merged count).  kWrite true: the kept
// elements to out[pos[tile] ..), never at or behind `bound` (unsorted inputs can count an element in two tiles)
template <bool kWrite>
__global__ __launch_bounds__(kMpThreads) void mp_setop_kernel(int op, const unsigned *__restrict__ a,
                                                              const unsigned long long *a_count, unsigned a_capacity,
                                                              const unsigned *__restrict__ b,
                                                              const unsigned long long *b_count, unsigned b_capacity,
                                                              const unsigned *__restrict__ part, unsigned *__restrict__ cnt,
                                                              const unsigned *__restrict__ pos, unsigned *__restrict__ out,
                                                              unsigned bound) {
  __shared__ __attribute__((aligned(16))) unsigned s[kMpTile + 4];
  __shared__ unsigned s_wsum[kMpThreads / kWave];
  if (kWrite && cnt[blockIdx.x] == 0) return;  // uniform; nothing kept here: the inputs are not read again
  MpWork w;
  if (!mp_tile_load<true>(a, a_count, a_capacity, b, b_count, b_capacity, part, s, w)) {
    if (!kWrite && threadIdx.x == 0) cnt[blockIdx.x] = 0u;
    return;
  }
  unsigned key[kMpItems];
#pragma unroll
  for (int k = 0; k < kMpItems; ++k) key[k] = 0u;
  unsigned kept = 0;  // bit k: the thread's k-th element is kept
  const unsigned an = w.e.an;
  mp_thread_merge(s, w, 0u, [&](int k, bool from_a, unsigned i, unsigned j, unsigned x) {
    // the neighbour on the other side: B[b0 + j] (the halo for j == bn) or A[a0 + i - 1] (the halo for i == 0)
    const unsigned other = s[from_a ? 1 + an + j : i];
    const bool there = from_a ? (w.e.b0 + j < w.cb) : (w.e.a0 + i > 0);
    key[k] = x;
    kept |= static_cast<unsigned>(mp_keep(op, from_a, there && other == x)) << k;
  });
  unsigned tile_kept;
  unsigned at = block_exclusive_scan<kMpThreads>(static_cast<unsigned>(__popc(kept)), s_wsum, tile_kept);
  if (!kWrite) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = tile_kept;
    return;
  }
  // (the scan's barriers are behind every thread's reads of the image: the kept elements take its place)
#pragma unroll
  for (int k = 0; k < kMpItems; ++k)
    if ((kept >> k) & 1u) s[at++] = key[k];  // at < tile_kept <= count <= kMpTile
  __syncthreads();
  const unsigned first = pos[blockIdx.x];
  for (unsigned p = threadIdx.x; p < tile_kept; p += kMpThreads) {
    const unsigned long long to = static_cast<unsigned long long>(first) + p;
    if (to < bound) out[to] = s[p];
  }
}

bool sizes_ok(size_t a_capacity, size_t b_capacity) {
  return fits_32(a_capacity) && fits_32(b_capacity) && fits_32(a_capacity + b_capacity);
}

}  // namespace

extern "C" size_t dbench_merge_workspace_bytes(size_t a_capacity, size_t b_capacity) {
  if (!sizes_ok(a_capacity, b_capacity)) return 0;
  return mp_layout(a_capacity + b_capacity).total;
}

extern "C" int dbench_merge_u32(const uint32_t *a_keys, const uint32_t *a_vals, const uint64_t *a_count, size_t a_capacity,
                                const uint32_t *b_keys, const uint32_t *b_vals, const uint64_t *b_count, size_t b_capacity,
                                int flags, uint32_t *out_keys, uint32_t *out_vals, uint64_t *out_count, void *workspace,
                                size_t workspace_bytes, void *stream) {
  if (flags & ~(DBENCH_MERGE_SIGNED | DBENCH_MERGE_ROW_IDS)) return DBHIP_EINVAL;
  if (!sizes_ok(a_capacity, b_capacity)) return DBHIP_EINVAL;
  const size_t rows = a_capacity + b_capacity;
  if ((a_capacity && !a_keys) || (b_capacity && !b_keys) || (rows && !out_keys) || !out_count) return DBHIP_EINVAL;
  if ((a_count && !a_keys) || (b_count && !b_keys)) return DBHIP_EINVAL;
  const bool row_ids = (flags & DBENCH_MERGE_ROW_IDS) != 0;
  if (!out_vals || row_ids) {  // keys only, or row ids: no value columns; row ids need their output
    if (a_vals || b_vals || (row_ids && !out_vals)) return DBHIP_EINVAL;
  } else if ((a_capacity && !a_vals) || (b_capacity && !b_vals)) {
    return DBHIP_EINVAL;
  }
  const uintptr_t words = addr(a_keys) | addr(a_vals) | addr(b_keys) | addr(b_vals) | addr(out_keys) | addr(out_vals);
  const uintptr_t counts = addr(a_count) | addr(b_count) | addr(out_count);
  if ((words & 3u) || (counts & 7u)) return DBHIP_EINVAL;
  const Range outs[] = {{out_keys, 4 * rows}, {out_vals, 4 * rows}, {out_count, 8}};
  const Range ins[] = {{a_keys, 4 * a_capacity}, {a_vals, 4 * a_capacity}, {a_count, 8},
                       {b_keys, 4 * b_capacity}, {b_vals, 4 * b_capacity}, {b_count, 8}};
  if (outputs_overlap(outs, 3, ins, 6)) return DBHIP_EINVAL;
  const MpLayout l = mp_layout(rows);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, l.total, s);
  if (rc != DBHIP_OK) return rc;

  char *base = static_cast<char *>(workspace);
  unsigned *part = reinterpret_cast<unsigned *>(base + l.part);
  const unsigned long long *na = reinterpret_cast<const unsigned long long *>(a_count);
  const unsigned long long *nb = reinterpret_cast<const unsigned long long *>(b_count);

  const unsigned tiles = static_cast<unsigned>(l.tiles), ac = static_cast<unsigned>(a_capacity),
                 bc = static_cast<unsigned>(b_capacity);
  const unsigned flip = (flags & DBENCH_MERGE_SIGNED) ? 0x80000000u : 0u;
  hipLaunchKernelGGL(mp_partition_kernel, dim3(tiles / kMpThreads + 1), dim3(kMpThreads), 0, s, a_keys, na, ac, b_keys, nb,
                     bc, flip, part, tiles, reinterpret_cast<unsigned long long *>(out_count));
  if (tiles) {
    const int mode = !out_vals ? kKeysOnly : (row_ids ? kRowIds : kCarried);
    auto kernel = mode == kKeysOnly ? mp_merge_kernel<kKeysOnly> : (mode == kRowIds ? mp_merge_kernel<kRowIds> : mp_merge_kernel<kCarried>);
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kMpThreads), 0, s, a_keys, a_vals, na, ac, b_keys, b_vals, nb, bc, flip,
                       part, out_keys, out_vals);
  }
  return launch_status();
}

extern "C" int dbench_setop_u32(int op, const uint32_t *a, const uint64_t *a_count, size_t a_capacity, const uint32_t *b,
                                const uint64_t *b_count, size_t b_capacity, uint32_t *out, uint64_t *out_count,
                                void *workspace, size_t workspace_bytes, void *stream) {
  if (op != DBENCH_SETOP_UNION && op != DBENCH_SETOP_INTERSECT && op != DBENCH_SETOP_DIFFERENCE) return DBHIP_EINVAL;
  if (!sizes_ok(a_capacity, b_capacity)) return DBHIP_EINVAL;
  if ((a_capacity && !a) || (b_capacity && !b) || !out_count) return DBHIP_EINVAL;
  if ((a_count && !a) || (b_count && !b)) return DBHIP_EINVAL;
  if (((addr(a) | addr(b) | addr(out)) & 3u) || ((addr(a_count) | addr(b_count) | addr(out_count)) & 7u)) return DBHIP_EINVAL;
  const size_t rows = a_capacity + b_capacity;
  const size_t bound = op == DBENCH_SETOP_UNION ? rows
                       : op == DBENCH_SETOP_INTERSECT ? (a_capacity < b_capacity ? a_capacity : b_capacity)
                                                      : a_capacity;
  const Range outs[] = {{out, 4 * bound}, {out_count, 8}};
  const Range ins[] = {{a, 4 * a_capacity}, {a_count, 8}, {b, 4 * b_capacity}, {b_count, 8}};
  if (outputs_overlap(outs, 2, ins, 4)) return DBHIP_EINVAL;
  const MpLayout l = mp_layout(rows);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = begin_call(workspace, workspace_bytes, l.total, s);
  if (rc != DBHIP_OK) return rc;

  char *base = static_cast<char *>(workspace);
  unsigned *part = reinterpret_cast<unsigned *>(base + l.part);
  unsigned *cnt = reinterpret_cast<unsigned *>(base + l.cnt);
  unsigned *pos = reinterpret_cast<unsigned *>(base + l.pos);
  const unsigned long long *na = reinterpret_cast<const unsigned long long *>(a_count);
  const unsigned long long *nb = reinterpret_cast<const unsigned long long *>(b_count);

  const unsigned tiles = static_cast<unsigned>(l.tiles), ac = static_cast<unsigned>(a_capacity),
                 bc = static_cast<unsigned>(b_capacity);
  if (tiles) {
    hipLaunchKernelGGL(mp_partition_kernel, dim3(tiles / kMpThreads + 1), dim3(kMpThreads), 0, s, a, na, ac, b, nb, bc, 0u,
                       part, tiles, static_cast<unsigned long long *>(nullptr));
    hipLaunchKernelGGL(mp_setop_kernel<false>, dim3(tiles), dim3(kMpThreads), 0, s, op, a, na, ac, b, nb, bc, part, cnt,
                       static_cast<const unsigned *>(nullptr), static_cast<unsigned *>(nullptr), 0u);
  }
  launch_rowlist_scan(cnt, pos, tiles, bound, reinterpret_cast<unsigned long long *>(out_count), s);
  if (tiles && out)
    hipLaunchKernelGGL(mp_setop_kernel<true>, dim3(tiles), dim3(kMpThreads), 0, s, op, a, na, ac, b, nb, bc, part, cnt, pos,
                       out, static_cast<unsigned>(bound));
  return launch_status();
}
