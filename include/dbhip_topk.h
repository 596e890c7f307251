/* dbhip_topk.h — ORDER BY key LIMIT k on gfx950: a radix select that returns the keys and the row ids of the first k
 * rows, and its device-side validator.  A second header next to dbhip.h (whose error codes, status bits and
 * dbhip_stream_t it uses); the contract of dbhip.h holds throughout: plain C ABI, device pointers, caller-owned
 * workspace with a 256-byte header whose first word is the status word, nothing allocates, frees or synchronises, every
 * call can be captured into a graph.  No reference counterpart: the reference stops at the sort.
 *
 * Order.  Row a PRECEDES row b when keys[a] is better than keys[b], or when the keys are equal and a < b.  Better means
 * smaller, or larger when `largest` is set; unsigned for _u32, signed for _i32.  The answer is the first
 * m = min(k, n) rows in that order:
 *   sorted != 0   out_keys[i] / out_rows[i] = key and row index of the i-th of them: keys ascending (descending with
 *                 `largest`), ties by ascending row.  With largest == 0 and k >= n this is the stable argsort; with
 *                 `largest` it is NOT its reverse: ties still ascend by row.
 *   sorted == 0   the same rows in ascending row order (what a later gather wants).
 * Either way the answer is unique.  Exactly m entries of each output column are written; entries [m, k) and everything
 * else stay untouched.  n, k, largest and sorted are host values, everything else is decided on the device.
 *
 * DBHIP_EINVAL, before any HIP call: keys NULL with n > 0, an output column NULL with m > 0, n >= 2^32, keys, out_keys or
 * out_rows not 16-byte aligned.  DBHIP_EWORKSPACE: a short or misaligned workspace; an argument error comes first.
 * n == 0 or k == 0: DBHIP_OK, nothing written to the outputs, a workspace that was passed gets a clean status word.
 * The workspace may hold anything on entry.  DBHIP_DEV_RANK_ORDER: raised by the stable pairs sort that orders the
 * selected rows (sorted != 0, dbhip.h) and folded into this workspace's status word by the call's last kernel.
 *
 * How: an MSD radix select over 11/11/10-bit digits finds the k-th key (three streaming reads of the column, 4n bytes
 * each), one more read counts per 4096-row segment the rows better than / equal to it, a scan turns the counts into output
 * positions, and one read of the segments that hold selected rows writes them in row order; rows equal to the k-th key
 * are taken in row order until k is reached.  sorted: dbhip_radix_sort_pairs_u32 on the m selected pairs.  There is no
 * separate route for large k (DESIGN.md 4.9 has the figures).
 *
 * Workspace bound: dbhip_topk_workspace_bytes(n, k) <= 4 MiB + n / 128 + 16 * min(k, n), a multiple of 256, and 0 for
 * n >= 2^32.  (Header and digit bins 193 KiB, 16 bytes per 4096-row segment, four 4-byte columns of m entries — the
 * selected pairs and the sort's ping-pong buffers — and the sort's own workspace, at most 3.1 MiB.)                    */
#ifndef DBHIP_TOPK_H
#define DBHIP_TOPK_H

#include "dbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBHIP_TOPK_SEGMENT_ROWS 4096 /* one wave's rows in the count and write kernels */
#define DBHIP_TOPK_CHUNK_ROWS 32768  /* one workgroup's rows there: eight segments, four 8192-key tiles */

size_t dbhip_topk_workspace_bytes(size_t n, size_t k); /* 0 for n >= 2^32 */
int dbhip_topk_u32(const uint32_t *keys, size_t n, size_t k, int largest, int sorted, uint32_t *out_keys,
                   uint32_t *out_rows, void *workspace, size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_topk_i32(const int32_t *keys, size_t n, size_t k, int largest, int sorted, int32_t *out_keys,
                   uint32_t *out_rows, void *workspace, size_t workspace_bytes, dbhip_stream_t stream);

/* Validator of a SORTED top-k table, m = min(k, n); both result words are zeroed by the call itself:
 *   result[0]  entries i < m that are wrong: out_rows[i] >= n, keys[out_rows[i]] != out_keys[i], or i > 0 and entry i-1
 *              does not strictly precede entry i (as (key, row) pairs, in the order above);
 *   result[1]  input rows that strictly precede the pair (out_keys[m-1], out_rows[m-1]); the pair is taken as two values,
 *              its row is never dereferenced.
 * The table is right iff result[0] == 0 and result[1] == m - 1 (m == 0: both words 0): strictly ascending genuine entries
 * are m distinct rows none of which comes after the last one, and exactly m rows do not come after the last one.
 * is_signed: the order of dbhip_topk_i32.  One read of the column.  DBHIP_EINVAL: result NULL, n >= 2^32, keys NULL with
 * n > 0, an output column NULL with m > 0.                                                                            */
int dbhip_check_topk_u32(const uint32_t *keys, size_t n, const uint32_t *out_keys, const uint32_t *out_rows, size_t k,
                         int largest, int is_signed, uint64_t *result /* 2 words, device */, dbhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBHIP_TOPK_H */
