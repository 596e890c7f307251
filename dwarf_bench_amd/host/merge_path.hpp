// merge_path.hpp — the two pieces of the merge-path kernels (merge_sorted.cpp) that compute an index from data: the
// diagonal search, and the clamped extents of a tile with the serial merge of a thread's items.  Plain functions for
// host and device behind one qualifier macro, templated on the column type (anything with operator[]): the kernels
// run them on global and LDS pointers, tests/cpp/merge_path_check.cpp runs the same text on the host over arrays
// that check every index.
//
// Order.  Keys compare as (x ^ flip) unsigned: flip = 0 for uint32, 0x80000000 for int32.  The merged order is by key,
// and among equal keys every A element stands before every B element (A[i] stands before B[j] iff A[i] <= B[j]).
//
// Nothing here relies on the inputs being sorted for the RANGE of what it returns: every index it forms is inside
// [0, na) or [0, nb) whatever the columns hold, and the extents of a tile always add up to the tile.
#ifndef DBENCH_MERGE_PATH_HPP
#define DBENCH_MERGE_PATH_HPP

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBENCH_MP_FN __host__ __device__ inline
#else
#define DBENCH_MP_FN inline
#endif

// The number of A elements among the first `diag` elements of the merged order, 0 <= diag <= na + nb.
// Returns i with max(0, diag - nb) <= i <= min(diag, na), so that j = diag - i lies in [0, nb].  The search reads
// a[mid] for mid in [0, na) and b[diag - 1 - mid] in [0, nb) only.
template <class KA, class KB>
DBENCH_MP_FN unsigned mp_diagonal(const KA &a, unsigned na, const KB &b, unsigned nb, unsigned diag, unsigned flip) {
  unsigned lo = diag > nb ? diag - nb : 0u;
  unsigned hi = diag < na ? diag : na;
  while (lo < hi) {
    const unsigned mid = lo + (hi - lo) / 2;  // lo <= mid < hi <= min(diag, na): diag - 1 - mid is in [0, nb)
    if ((a[mid] ^ flip) <= (b[diag - 1 - mid] ^ flip))
      lo = mid + 1;  // A[mid] stands before B[diag - 1 - mid]: it is among the first diag
    else
      hi = mid;
  }
  return lo;
}

struct MpTile {
  unsigned a0, an, b0, bn;  // the tile merges a[a0, a0 + an) with b[b0, b0 + bn); an + bn == diag1 - diag0
};

// The extents of the tile between the diagonals diag0 <= diag1 <= na + nb, from the two partition points as they
// were stored (a_lo for diag0, a_hi for diag1).  Of sorted inputs these are mp_diagonal's values and come back
// unchanged.  Partition points of unsorted inputs need not be monotone, and a stored word could be anything, so
// both are clamped: a0 into [diag0 - nb, min(diag0, na)], and the end of the A part into
// [max(a0, diag1 - nb), min(a0 + (diag1 - diag0), na)], which is never empty.  Hence
//   a0 + an <= na,  b0 + bn <= nb,  an + bn == diag1 - diag0   always.
DBENCH_MP_FN MpTile mp_tile_extents(unsigned a_lo, unsigned a_hi, unsigned diag0, unsigned diag1, unsigned na,
                                    unsigned nb) {
  const unsigned count = diag1 - diag0;
  const unsigned a0_least = diag0 > nb ? diag0 - nb : 0u, a0_most = diag0 < na ? diag0 : na;
  const unsigned a0 = a_lo < a0_least ? a0_least : (a_lo > a0_most ? a0_most : a_lo);
  const unsigned reach = diag1 > nb ? diag1 - nb : 0u;
  const unsigned end_least = a0 > reach ? a0 : reach;
  const unsigned end_most = (na - a0) < count ? na : a0 + count;
  const unsigned a_end = a_hi < end_least ? end_least : (a_hi > end_most ? end_most : a_hi);
  MpTile t;
  t.a0 = a0;
  t.an = a_end - a0;
  t.b0 = diag0 - a0;
  t.bn = count - t.an;
  return t;
}

// The serial merge of at most kItems elements from a[ai, a_end) and b[bi, b_end), both ranges inside their arrays:
// emit(k, from_a, ai, bi, key) for the k-th of them, with the two cursors as they stand BEFORE the element is taken
// (the element is a[ai] if from_a, else b[bi]).  It stops after `items` elements or when both ranges are used up.
// Reads a[i] for i in [ai, a_end) and b[j] for j in [bi, b_end) only.
template <int kItems, class KA, class KB, class Emit>
DBENCH_MP_FN void mp_serial_merge(const KA &a, unsigned ai, unsigned a_end, const KB &b, unsigned bi, unsigned b_end,
                                  unsigned flip, unsigned items, Emit &&emit) {
  unsigned ka = ai < a_end ? a[ai] : 0u, kb = bi < b_end ? b[bi] : 0u;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const bool has_a = ai < a_end, has_b = bi < b_end;
    if (static_cast<unsigned>(k) < items && (has_a || has_b)) {  // (no break: the loop unrolls, k is a constant)
      const bool from_a = !has_b || (has_a && (ka ^ flip) <= (kb ^ flip));
      emit(k, from_a, ai, bi, from_a ? ka : kb);
      if (from_a) {
        ++ai;
        if (ai < a_end) ka = a[ai];
      } else {
        ++bi;
        if (bi < b_end) kb = b[bi];
      }
    }
  }
}

#endif
