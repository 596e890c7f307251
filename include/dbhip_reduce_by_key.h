/* dbhip_reduce_by_key.h — one output row per run of equal adjacent keys on gfx950 (thrust's and cuDF's reduce_by_key):
 * COUNT, exact 64-bit SUM, MIN and MAX per run, and its device-side validator.  Behind the stable pairs sort of dbhip.h
 * this is SELECT key, COUNT(*), SUM(v), MIN(v), MAX(v) ... GROUP BY key ORDER BY key; on a column that is already grouped
 * it is the whole group-by.  A third header next to dbhip.h (whose error codes, status bits and dbhip_stream_t it uses);
 * the contract of dbhip.h holds throughout: plain C ABI, device pointers, caller-owned workspace with a 256-byte header
 * whose first word is the status word, nothing allocates, frees or synchronises, every call can be captured into a graph.
 * No reference counterpart.
 *
 * Runs.  A RUN is a maximal range of consecutive rows with equal keys.  Keys are compared for equality only (there is no
 * signed or unsigned variant for keys) and the input need not be sorted: a key that comes back later starts a new run.
 * Runs are numbered in row order; *out_runs (a DEVICE uint64) is always the full number of runs R.
 *
 * Output row r:
 *   out_keys[r]    the key of run r
 *   out_counts[r]  its number of rows (fits 32 bits: n < 2^32)
 *   out_sums[r]    the exact 64-bit sum of its values, zero-extended, or sign-extended when vals_signed is set (cannot
 *                  overflow: fewer than 2^32 rows of 32-bit values)
 *   out_mins[r], out_maxs[r]  the extreme values, as unsigned, or as int32 when vals_signed is set
 * Each of the five output columns may be NULL: that aggregate is then neither computed nor written.  vals may be NULL only
 * if out_sums, out_mins and out_maxs are all NULL (DISTINCT with counts on grouped input).  The answer is unique.
 *
 * capacity is the number of entries of every output column that was passed.  Only runs numbered below it are written,
 * everything else stays untouched; R > capacity sets DBHIP_DEV_TABLE_FULL in the workspace status word and *out_runs still
 * holds R (the dbhip_join_pairs_u32 convention), so a caller can allocate and call again.  The count-only call,
 * capacity == 0 with all five columns NULL, computes R alone and never raises DBHIP_DEV_TABLE_FULL.
 *
 * n == 0: DBHIP_OK, *out_runs = 0 when out_runs is given, a workspace that was passed gets a clean status word.
 * DBHIP_EINVAL, before any HIP call: n >= 2^32; keys NULL with n > 0; out_runs NULL with n > 0; a non-NULL column with
 * capacity 0, or capacity > 0 with every column NULL; vals NULL with out_sums, out_mins or out_maxs given; keys, vals or
 * any output column not 16-byte aligned.  DBHIP_EWORKSPACE: a short or misaligned workspace; an argument error comes first.
 * The workspace may hold anything on entry; repeated calls on one workspace give identical outputs.
 *
 * How (all dependent launches, no workgroup ever waits for another, no CAS loop, every loop bounded by n): a wave owns a
 * 4096-row SEGMENT.  One read of the keys counts every segment's run heads (row 0, or keys[i] != keys[i-1]); one workgroup
 * scans the counts into every segment's first output row, writes *out_runs and compares it with capacity; one read of
 * keys and vals runs a segmented wave scan and writes every run that ends inside the segment where it began, leaving the
 * rows in front of a segment's first head and the rows from its last head on as two partial records; one workgroup joins
 * the records with a segmented scan over the segments and writes the runs that cross a segment boundary.
 * Bytes: 12n + 24 min(R, capacity) for all five aggregates.
 *
 * Workspace bound: dbhip_reduce_by_key_workspace_bytes(n) <= 2048 + n / 64, a multiple of 256, and 0 for n >= 2^32.
 * (The header and 56 bytes per 4096-row segment — head count, first output row, the two partial records — in three parts
 * that each start at a 256-byte offset.)                                                                                 */
#ifndef DBHIP_REDUCE_BY_KEY_H
#define DBHIP_REDUCE_BY_KEY_H

#include "dbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBHIP_REDUCE_BY_KEY_SEGMENT_ROWS 4096 /* one wave's rows in the count and reduce kernels */
#define DBHIP_REDUCE_BY_KEY_CHUNK_ROWS 32768  /* one workgroup's rows there: eight segments */

size_t dbhip_reduce_by_key_workspace_bytes(size_t n); /* 0 for n >= 2^32 */
int dbhip_reduce_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed, uint32_t *out_keys,
                            uint32_t *out_counts, uint64_t *out_sums, uint32_t *out_mins, uint32_t *out_maxs,
                            size_t capacity, uint64_t *out_runs /* device */, void *workspace, size_t workspace_bytes,
                            dbhip_stream_t stream);

/* Validator of a table of `runs` rows (all five columns required) against the input, by an algorithm that does not count
 * heads: starts = the exclusive scan of out_counts (dbhip_exclusive_scan_u32 in the validator's workspace, 32-bit), T = the
 * exact 64-bit sum of out_counts, and every input row i < T finds its run r by binary search in starts (the last r of the
 * bisection with starts[r] <= i).  The four result words are zeroed by the call itself:
 *   result[0]  faults: 1 if T != n; runs with count 0; runs r > 0 with 1 <= starts[r] <= n whose key equals the key of row
 *              starts[r] - 1 (the run is not maximal); rows i < T whose key differs from the key of their run; rows i < T
 *              whose value lies outside [min, max] of their run (as unsigned, or as int32 when vals_signed is set); rows
 *              i >= T (rows behind the table)
 *   result[1]  runs whose min is not the value of any of its rows, plus the same for max
 *   result[2]  sum over rows i < T of value * w(run) mod 2^64 (value zero- or sign-extended to 64 bits)
 *   result[3]  sum over runs of out_sums[r] * w(r) mod 2^64;  w(r) = mix64(0x72626B, r) | 1, an odd 64-bit weight
 * The table is right iff result[0] == 0, result[1] == 0 and result[2] == result[3].  The sum comparison is a fingerprint:
 * a right table always agrees, an error confined to one run's sum never does (an odd weight is a bijection mod 2^64), and
 * errors d_r spread over several runs pass only when sum d_r * w(r) == 0 mod 2^64.  Nothing outside the arrays is read,
 * whatever the table holds.  DBHIP_EINVAL: result NULL, n or runs >= 2^32, keys or vals NULL with n > 0, a column NULL
 * with runs > 0; DBHIP_EWORKSPACE: a short or misaligned workspace (dbhip_check_reduce_by_key_workspace_bytes(n, runs):
 * two words per run, a header, and the scan's own workspace).                                                          */
size_t dbhip_check_reduce_by_key_workspace_bytes(size_t n, size_t runs);
int dbhip_check_reduce_by_key_u32(const uint32_t *keys, const uint32_t *vals, size_t n, int vals_signed,
                                  const uint32_t *out_keys, const uint32_t *out_counts, const uint64_t *out_sums,
                                  const uint32_t *out_mins, const uint32_t *out_maxs, size_t runs,
                                  uint64_t *result /* 4 words, device */, void *workspace, size_t workspace_bytes,
                                  dbhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBHIP_REDUCE_BY_KEY_H */
