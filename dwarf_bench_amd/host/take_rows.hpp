/* take_rows.hpp — late materialisation: what turns a row-id list back into data.  take gathers up to four 32-bit columns
 * through a row-id list; aggregate computes COUNT, the 64-bit SUM, MIN and MAX of one column over a row-id list, or over
 * the whole column, without materialising it.  Both read the list's length on the device.  Plain C, exported by
 * libdbench.so; the contract is that of include/dbhip.h as select_rows.hpp and merge_sorted.hpp restate it (error codes
 * DBHIP_E*, status bits DBHIP_DEV_*): device pointers, a caller-owned 256-byte aligned workspace whose first word is the
 * status word (cleared by a launch in front of the first kernel that can raise it), asynchronous on `stream`, nothing
 * allocates, frees, synchronises or reads back, capturable into a hipGraph, and repeated calls on a workspace that held
 * anything give identical outputs.
 *
 * Length.  m = min(*count, capacity); count is a device uint64 read ON THE DEVICE (NULL: m = capacity) and may hold any
 *   64-bit value (the total of dbhip_join_pairs_u32 exceeds the capacity on overflow).  Grids are sized from capacity:
 *   the out_count of dbench_select_range_u32 or dbench_setop_u32 can be the count of these calls inside one captured
 *   graph.  capacity < 2^32, n_rows < 2^32.
 * take.  cols and outs are HOST arrays of n_cols (1 .. DBENCH_TAKE_MAX_COLS) device pointers, read during the call and
 *   not retained: they travel by value in the kernel arguments.  All columns have n_rows rows.  For i < m and every
 *   column c: outs[c][i] = cols[c][rows[i]] if rows[i] < n_rows; otherwise outs[c][i] = fill and DBHIP_DEV_KEY_RANGE is
 *   raised in the status word — except that with DBENCH_TAKE_OUTER the id 0xFFFFFFFF ("no row": the build row of a
 *   left-outer join's miss) is filled without raising.  Entries [m, capacity) of every output are not touched.  Nothing
 *   outside cols[c][0 .. n_rows) is ever read, whatever the list holds; with n_rows == 0 every entry is filled.  The
 *   list may be unsorted and may repeat rows.
 * aggregate.  The candidates are rows[0 .. m); with rows == NULL all rows 0 .. n_rows-1 (count must then be NULL,
 *   capacity is ignored).  Candidates >= n_rows are skipped and raise DBHIP_DEV_KEY_RANGE; with DBENCH_TAKE_OUTER
 *   0xFFFFFFFF is skipped silently.  out[0] = the number of rows aggregated, out[1] = their sum mod 2^64 (values
 *   zero-extended, or sign-extended with DBENCH_TAKE_SIGNED), out[2] = the minimum, out[3] = the maximum, extended to
 *   64 bits the same way.  For zero rows the minimum is 0xFFFFFFFF (signed: INT32_MAX) and the maximum 0 (signed:
 *   INT32_MIN).  out is always written in full and need not be zeroed.  Integer arithmetic: the answer does not depend
 *   on the order of the reduction, it is bit-exact and identical from call to call.
 * Columns, list and outputs: any 4-byte alignment; count and out: 8-byte aligned.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits, DBENCH_TAKE_SIGNED on take, n_cols outside 1 .. 4 (or cols or
 *   outs NULL), a size of 2^32 or more, a NULL column with n_rows > 0 and capacity > 0 (aggregate over all rows: with
 *   n_rows > 0), rows NULL with capacity > 0 (take), count without rows, a NULL output, a misaligned pointer, an output
 *   overlapping an input or another output.  DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (argument errors
 *   come first).  The device is looked for after both.
 *
 * Workspace of dbench_take_workspace_bytes(capacity) — one query serves both entry points — with S = capacity /
 * DBENCH_TAKE_SEGMENT_ROWS rounded up, plus 1 (positions are laid out from the 16-byte boundary in front of the list, so
 * a list of `capacity` entries can touch S segments), and P = S / 4 rounded up, at least 1 and at most 2048:
 *   [0, 256)               header, word 0 = status
 *   [256, 256 + 32 P ...)  P partial records of the aggregate, one per workgroup: uint64 count, sum, min, max
 * rounded up to 256: a multiple of 256, monotone in capacity, at most 1024 + capacity / 128 and never more than 65792,
 * and 0 for capacity >= 2^32 (no such call).  take uses the header alone.  The aggregate over all rows (rows == NULL)
 * needs the 512 bytes of capacity 0 and uses as many partial records as the workspace it is given holds, up to 2048: a
 * workspace sized for capacity = n_rows runs it at full width.
 *
 * Launches behind the header's clear, no workgroup waits for another.  take: one launch, a wave per segment, two waves
 * per workgroup; a lane holds four consecutive entries (one 16-byte load of row ids), bounds-checks each, issues its
 * 4 x n_cols gathers before the first use and stores four consecutive words per column.  aggregate: a grid-stride launch
 * of at most P workgroups, each leaving one partial record, then one workgroup that folds the records into out.
 */
#ifndef DBENCH_TAKE_ROWS_HPP
#define DBENCH_TAKE_ROWS_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_TAKE_MAX_COLS 4
#define DBENCH_TAKE_SEGMENT_ROWS 1024 /* one wave's positions at a time */
#define DBENCH_TAKE_OUTER 1  /* row id 0xFFFFFFFF is "no row" (the left-outer join's miss), not an error */
#define DBENCH_TAKE_SIGNED 2 /* aggregate: values are int32 */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_take_workspace_bytes(size_t capacity);
int dbench_take_u32(const uint32_t *const *cols, size_t n_cols, size_t n_rows, const uint32_t *rows, const uint64_t *count,
                    size_t capacity, int flags, uint32_t fill, uint32_t *const *outs, void *workspace,
                    size_t workspace_bytes, void *stream);
int dbench_aggregate_rows_u32(const uint32_t *col, size_t n_rows, const uint32_t *rows, const uint64_t *count,
                              size_t capacity, int flags, uint64_t *out, void *workspace, size_t workspace_bytes,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif
