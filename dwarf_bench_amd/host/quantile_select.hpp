/* quantile_select.hpp — exact order statistics of a 32-bit column: the values at up to 16 ranks (MEDIAN, PERCENTILE_DISC,
 * the k-th value, equi-depth bucket bounds) by one multi-rank radix select, over all rows or the rows of a row-id list.
 * Plain C, exported by libdbench.so; the contract is that of hll_sketch.hpp and bloom_filter.hpp (error codes DBHIP_E*,
 * status bits DBHIP_DEV_* of include/dbhip.h): device pointers, a caller-owned 256-byte aligned workspace whose first word
 * is the status word (cleared, with the rest of the workspace, by a launch of its own in front of the first kernel that can
 * raise it), asynchronous on `stream`, nothing allocates, frees, synchronises or reads back, capturable into a hipGraph,
 * and repeated calls on a workspace that held anything give identical outputs.
 *
 * Candidates.  rows == NULL: rows 0 .. min(*count, n_col) of col (capacity is not looked at beyond its range check).
 *   Otherwise rows[i] for i < min(*count, capacity).  count is a device uint64 read ON THE DEVICE (NULL: all) and may hold
 *   any 64-bit value; grids are sized from n_col or capacity, so the out_count of a select can be the count of this call
 *   inside one captured graph.  The list may be unsorted and may repeat rows: a repeated row counts as many times as it
 *   appears.  A row id >= n_col is not a candidate and raises DBHIP_DEV_KEY_RANGE; nothing outside [0, n_col) of the column
 *   is read, whatever the list holds.  m, the number of valid candidates, is known on the device alone.
 * Order.  Unsigned by default, int32 with DBENCH_QUANTILE_SIGNED: the select works on x = key ^ flip.
 * Ranks.  q_num and q_den are HOST arrays of n_q = 1 .. DBENCH_QUANTILE_MAX_RANKS entries, read during the call; the ranks
 *   are resolved on the device against m in exact integer arithmetic (quantile_layout.hpp):
 *     q_den[j] == 0   the absolute 0-based rank r = q_num[j]
 *     q_den[j] >  0   q_num[j] <= q_den[j];  r = 0 for q_num[j] == 0, otherwise r = ceil(q_num[j] * m / q_den[j]) - 1
 *                     (PERCENTILE_DISC: 1/2 is the lower median, 1/1 the maximum)
 *   Ranks may repeat and come in any order.
 * Answer for rank j, v being the r-th smallest candidate in the order:
 *     out_values[j] = v (the key itself, the flip removed)
 *     out_below[j]  = the candidates strictly before v        out_equal[j] = the candidates equal to v
 *   so out_below[j] <= r < out_below[j] + out_equal[j].  No such row (m == 0, or an absolute r >= m): out_values[j] = 0,
 *   out_below[j] = m, out_equal[j] = 0.  All 3 * n_q words are written by every call and nothing else outside the
 *   workspace; the answer is unique.
 * col, rows: any 4-byte alignment; the outputs: 4-byte aligned; count: 8-byte aligned.  n_col, capacity < 2^32.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits, n_q outside 1 .. 16, NULL q_num, q_den or an output,
 *   q_num[j] > q_den[j] > 0, a size of 2^32 or more, a NULL column with rows to read, a misaligned pointer, an output
 *   overlapping the column, the list, the count or another output.  DBHIP_EWORKSPACE: a NULL, short or misaligned
 *   workspace (argument errors come first).  The device is looked for after both.
 *
 * Workspace.  dbench_quantile_workspace_bytes(n_q) = 0 for n_q outside 1 .. 16, otherwise a multiple of 256 that depends on
 *   n_q alone: the 256-byte header, the slot table (512 bytes) and the three levels' global bins in copies.  It holds no
 *   state per row.
 *
 * Launches behind the clear of the workspace, each depending on the one in front; no workgroup waits for another, no grid
 *   barrier, no CAS loop, no atomic that returns a value, every loop bounded by the candidate count.  Three levels over the
 *   11 / 11 / 10-bit digits of x, each a histogram and a pick:
 *   qs_hist  a persistent grid streams the candidates (with a list: gathers col[rows[i]] again at every level).  Level 0
 *            counts the top digit of every valid candidate; levels 1 and 2 count, for the up to S <= n_q distinct prefixes
 *            ("slots") the ranks have led to so far, the next digit of the candidates under each prefix.  One flush per
 *            workgroup into one of the copies of the level's global bins.
 *   qs_pick  one workgroup sums the copies and scans each slot's bins.  At level 0 the total is m, and every (q_num, q_den)
 *            becomes its r; for every rank it finds the bin that holds it, appends the digit to the prefix, and keeps the
 *            candidates below (running) and the rank inside the bin; the new prefixes, duplicates removed, are the next
 *            level's slots.  The last level writes the three output columns.
 */
#ifndef DBENCH_QUANTILE_SELECT_HPP
#define DBENCH_QUANTILE_SELECT_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_QUANTILE_MAX_RANKS 16
#define DBENCH_QUANTILE_SIGNED 1 /* order the keys as int32 */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_quantile_workspace_bytes(int n_q);
int dbench_quantile_select_u32(const uint32_t *col, size_t n_col, const uint32_t *rows, const uint64_t *count, size_t capacity,
                               const uint32_t *q_num, const uint32_t *q_den, int n_q, int flags, uint32_t *out_values,
                               uint32_t *out_below, uint32_t *out_equal, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
