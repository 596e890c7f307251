/* select_rows.hpp — selection vectors: the row ids of the rows whose 32-bit column value lies inside (or outside) [lo, hi],
 * over all rows of a column or over a given row-id list, in candidate order (stable compaction).  Plain C, exported
 * by libdbench.so; the contract is that of include/dbhip.h (error codes DBHIP_E*, status bits DBHIP_DEV_*): device
 * pointers, a caller-owned 256-byte aligned workspace whose first word is the status word, asynchronous on `stream`,
 * nothing allocates, frees, synchronises or reads back, capturable into a hipGraph, and repeated calls on a workspace
 * that held anything give identical outputs.
 *
 * Candidates.  in_rows == NULL: rows 0 .. n_col-1 in that order (candidates = n_col; in_capacity is not looked at
 *   beyond its range check).  Otherwise in_rows[0 .. m) in list order, m = min(*in_count, in_capacity); in_count is a
 *   device uint64 read ON THE DEVICE (NULL: m = in_capacity), the grid is sized from in_capacity (candidates =
 *   in_capacity): the out_count of one call can be the in_count of the next inside one captured graph.  A list may be
 *   unsorted and may hold a row twice; each occurrence is a candidate of its own.
 * Predicate.  Candidate row r is kept iff r < n_col and (lo <= col[r] && col[r] <= hi) XOR DBENCH_SELECT_NEGATE;
 *   unsigned comparison, or as int32 with DBENCH_SELECT_SIGNED (lo and hi are then the int32 bounds' bit patterns).
 *   lo > hi is the empty interval.
 * Row ids >= n_col are never kept, not even under negate; one of them sets DBHIP_DEV_KEY_RANGE in the status word.
 *   Nothing outside col[0 .. n_col) is read, whatever the list holds.
 * Output.  out_rows[0 .. *out_count) = the kept row ids in candidate order; *out_count is always written (0 for no
 *   candidates); out_rows has room for `candidates` entries, entries from *out_count on are not touched.  out_rows ==
 *   NULL: the count alone.
 * col, in_rows, out_rows: any 4-byte alignment; in_count, out_count: 8-byte aligned.  n_col, in_capacity < 2^32.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits, a size out of range, col NULL with n_col > 0, out_count NULL,
 *   in_count without in_rows, a misaligned pointer, out_rows overlapping col or in_rows.  DBHIP_EWORKSPACE: a NULL, short
 *   or misaligned workspace (argument errors come first).  The device is looked for after both.
 *
 * Workspace of dbench_select_workspace_bytes(c), S = c / 4096 rounded up, plus 1 (candidates are laid out from the
 * 16-byte boundary in front of the column or list, so a list of c entries can touch S segments):
 *   [0, 256)                       header, word 0 = status
 *   [256, 256 + A)                 S x uint32 matches per segment, A = 4 S rounded up to 256
 *   [256 + A, 256 + 2 A)           S x uint32 first output position per segment
 *   [256 + 2 A, 256 + 2 A + 512 S) S x 64 x uint64 match masks: one bit per candidate
 * A multiple of 256, monotone in c, at most 4096 + c / 4, and 0 for c >= 2^32 (no such call).
 * Mask layout: candidate i has the position v = i + a, a = the words between the 16-byte boundary and the first entry
 * (0..3); segment = v / 4096, and inside it group g = v / 256 % 16, lane l = v / 4 % 64, q = v % 4 (a lane holds four
 * consecutive candidates: one 16-byte load); its bit is bit l of mask word 4 g + q of the segment.
 *
 * Three dependent launches behind the header's clear, no workgroup waits for another: mark (one wave per segment:
 * predicate -> ballots -> masks and the segment's count), scan (one workgroup: counts -> positions, *out_count), write
 * (segments with matches only: masks -> ranks -> row ids; the column is not read again).
 */
#ifndef DBENCH_SELECT_ROWS_HPP
#define DBENCH_SELECT_ROWS_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_SELECT_SEGMENT_ROWS 4096 /* one wave's candidates */
#define DBENCH_SELECT_SIGNED 1          /* compare as int32 instead of uint32 */
#define DBENCH_SELECT_NEGATE 2          /* keep the rows OUTSIDE [lo, hi] */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_select_workspace_bytes(size_t candidates);
int dbench_select_range_u32(const uint32_t *col, size_t n_col, const uint32_t *in_rows, const uint64_t *in_count,
                            size_t in_capacity, uint32_t lo, uint32_t hi, int flags, uint32_t *out_rows,
                            uint64_t *out_count, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
