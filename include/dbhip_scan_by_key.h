/* dbhip_scan_by_key.h — one output row per INPUT row over runs of equal adjacent keys on gfx950 (thrust's
 * inclusive_scan_by_key, cuDF's grouped scans): the run number, the running COUNT (ROW_NUMBER), the exact running 64-bit
 * SUM, the running MIN and MAX, and its device-side validator.  Behind the stable pairs sort of dbhip.h this is
 *   SELECT key, v, ROW_NUMBER() OVER w, SUM(v) OVER w, MIN(v) OVER w, MAX(v) OVER w
 *   FROM t WINDOW w AS (PARTITION BY key ORDER BY <row order> ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)
 * A fourth header next to dbhip.h (whose error codes, status bits and dbhip_stream_t it uses); the contract of dbhip.h holds
 * throughout: plain C ABI, device pointers, caller-owned workspace with a 256-byte header whose first word is the status
 * word, nothing allocates, frees, synchronises or reads back, every call can be captured into a graph.  No reference
 * counterpart.
 *
 * Runs and heads are those of dbhip_reduce_by_key.h: a HEAD is row 0 or a row whose key differs from its left neighbour's,
 * run r is the rows from the r-th head to the row in front of the next one.  Keys are compared for equality only and the
 * input need not be sorted: a key that comes back later starts a new run.
 *
 * Row i of run r whose head is row h:
 *   out_run_ids[i]      r: the row's output row in dbhip_reduce_by_key_u32 (DENSE_RANK - 1 on sorted keys); with
 *                       dbhip_gather_u32 it broadcasts a group total back to the group's rows
 *   out_row_numbers[i]  i - h + 1, the running COUNT
 *   out_sums[i]         the exact 64-bit sum of vals[h..i], zero-extended, or sign-extended when vals_signed is set (cannot
 *                       overflow: fewer than 2^32 rows of 32-bit values)
 *   out_mins[i], out_maxs[i]  the extremes of vals[h..i], as unsigned, or as int32 when vals_signed is set
 * Each of the five output columns may be NULL: it is then neither computed nor written.  vals may be NULL only if out_sums,
 * out_mins and out_maxs are all NULL.  The answer is unique.  The output columns must not overlap keys, vals or one another
 * (the second pass reads the inputs while it writes).  Every column that is passed has n entries; nothing else is written.
 *
 * n == 0: DBHIP_OK, no workspace needed; a workspace that was passed is still checked and gets a clean status word.
 * DBHIP_EINVAL, before any HIP call and in this order: n >= 2^32; keys NULL with n > 0; all five output columns NULL with
 * n > 0; vals NULL with out_sums, out_mins or out_maxs given; keys, vals or any output column that is not NULL and not
 * 16-byte aligned (for n == 0 too).  DBHIP_EWORKSPACE: a NULL, short or misaligned workspace; an argument error comes first.
 * The workspace may hold anything on entry; repeated calls on one workspace give identical outputs.  The status word is
 * cleared and never set: no input makes the call fail on the device.
 *
 * How (all dependent launches, no workgroup ever waits for another, no CAS loop, every loop bounded by n): a wave owns a
 * 4096-row SEGMENT, a workgroup eight of them.  One read of keys (and vals) leaves one record per segment: its number of
 * heads and the aggregate of the rows from its last head on (of all its rows, if it has none).  One workgroup scans the
 * records — every thread combines a contiguous block of them in registers, one workgroup scan joins the 1024 blocks, every
 * thread walks its block again — into every segment's CARRY: the heads in front of it and the aggregate of the run still
 * open there.  A second read of keys and vals scans every segment from its carry with a segmented wave scan and writes the
 * columns with 16-byte stores.  Bytes: 16n read + 24n written for all five columns.
 *
 * Workspace bound: dbhip_scan_by_key_workspace_bytes(n) <= 2048 + n / 64, a multiple of 256, and 0 for n >= 2^32.  (The
 * header and 64 bytes per 4096-row segment — a 32-byte record and a 32-byte carry — in two parts that each start at a
 * 256-byte offset.)                                                                                                      */
#ifndef DBHIP_SCAN_BY_KEY_H
#define DBHIP_SCAN_BY_KEY_H

#include "dbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBHIP_SCAN_BY_KEY_SEGMENT_ROWS 4096 /* one wave's rows in the two streaming kernels */
#define DBHIP_SCAN_BY_KEY_CHUNK_ROWS 32768  /* one workgroup's rows there: eight segments */

size_t dbhip_scan_by_key_workspace_bytes(size_t n); /* 0 for n >= 2^32 */
int dbhip_scan_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed, uint32_t *out_run_ids,
                          uint32_t *out_row_numbers, uint64_t *out_sums, uint32_t *out_mins, uint32_t *out_maxs,
                          void *workspace, size_t workspace_bytes, dbhip_stream_t stream);

/* Validator of the five columns against the input, exact, by an algorithm that never scans: it checks the recurrence row by
 * row.  Row i is a head iff i == 0 or keys[i] != keys[i-1]; v = vals[i], ext(v) its zero- or sign-extension.
 *   a head row must have      row_numbers[i] == 1, sums[i] == ext(v), mins[i] == maxs[i] == v, and
 *                             run_ids[i] == 0 for i == 0, run_ids[i-1] + 1 otherwise
 *   any other row must have   row_numbers[i] == row_numbers[i-1] + 1, sums[i] == sums[i-1] + ext(v),
 *                             mins[i] == min(mins[i-1], v), maxs[i] == max(maxs[i-1], v) (as unsigned, or as int32 when
 *                             vals_signed is set), run_ids[i] == run_ids[i-1]
 * All arithmetic is mod 2^32 or 2^64 on whatever the columns hold, and nothing outside the arrays is read, whatever they
 * hold.  By induction a table without a violating row is the right table.  The four result words are set by the call:
 *   result[0]  the number of (row, column) pairs that violate their rule
 *   result[1]  the lowest violating row, or ~0 when there is none
 *   result[2]  the number of heads seen
 *   result[3]  0
 * A NULL column is skipped.  DBHIP_EINVAL: result NULL or not 8-byte aligned; n >= 2^32; keys NULL with n > 0; all five
 * columns NULL with n > 0; vals NULL with sums, mins or maxs given.  The columns need only their natural alignment.
 * DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (dbhip_check_scan_by_key_workspace_bytes(n): a bare 256-byte
 * header, whose status word the call clears; 0 for n >= 2^32).                                                           */
size_t dbhip_check_scan_by_key_workspace_bytes(size_t n);
int dbhip_check_scan_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                const uint32_t *run_ids, const uint32_t *row_numbers, const uint64_t *sums,
                                const uint32_t *mins, const uint32_t *maxs, uint64_t *result /* 4 words, device */,
                                void *workspace, size_t workspace_bytes, dbhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBHIP_SCAN_BY_KEY_H */
