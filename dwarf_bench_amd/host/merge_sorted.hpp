/* merge_sorted.hpp — the stable merge of two sorted (key, value) columns, and the union, intersection and difference
 * of two strictly ascending row-id lists: one merge-path kernel family (merge_path.hpp, merge_sorted.cpp).  Plain C,
 * exported by libdbench.so; the contract is that of include/dbhip.h and select_rows.hpp (error codes DBHIP_E*): device
 * pointers, a caller-owned 256-byte aligned workspace whose first word is the status word (cleared by a launch in
 * front of the first kernel; no kernel here raises it: the preconditions are not checked on the device), asynchronous
 * on `stream`, nothing allocates, frees, synchronises or reads back, capturable into a hipGraph, and repeated calls on a
 * workspace that held anything give identical outputs.
 *
 * Sizes.  ca = min(*a_count, a_capacity), a device uint64 read ON THE DEVICE (a_count == NULL: ca = a_capacity); the
 *   same for B.  Grids are sized from the capacities: the out_count of one call (of select_rows.hpp too) can be the
 *   count of the next inside one captured graph.  a_capacity + b_capacity < 2^32.
 * Merge.  a_keys[0 .. ca) and b_keys[0 .. cb) are ascending: as uint32, or as int32 with DBENCH_MERGE_SIGNED.
 *   out_keys[i] is the i-th element of the stable merge: by key, among equal keys every A element before every B
 *   element, inside a source in input order — the stable argsort of cat(a[:ca], b[:cb]) applied to it.
 *   *out_count = ca + cb is always written; out_keys and out_vals have room for a_capacity + b_capacity entries,
 *   entries from *out_count on are not touched.
 *   Values.  out_vals == NULL: keys only (a_vals, b_vals and DBENCH_MERGE_ROW_IDS must be absent).
 *   DBENCH_MERGE_ROW_IDS: a_vals and b_vals must be NULL; out_vals is r for A's row r and a_capacity + r for B's row
 *   r (the host value: the ids index the two capacity-sized buffers laid end to end).  Otherwise a_vals and b_vals
 *   (each required if its capacity is not 0) are carried with their keys.
 * Set operations.  a[0 .. ca) and b[0 .. cb) are STRICTLY ascending uint32 lists (what dbench_select_range_u32 over
 *   all rows returns).  out[0 .. *out_count) = the ascending union (DBENCH_SETOP_UNION), intersection
 *   (DBENCH_SETOP_INTERSECT) or A minus B (DBENCH_SETOP_DIFFERENCE); *out_count is always written; out has room for
 *   a_capacity + b_capacity, min(a_capacity, b_capacity) and a_capacity entries respectively, entries from *out_count
 *   on are not touched.  out == NULL: the count alone.
 * Preconditions are not checked on the device.  On inputs that are not sorted (not strictly ascending) the values
 *   written are unspecified; nothing outside the buffers is read or written, *out_count is within the bounds above,
 *   and the call ends.
 * Columns: any 4-byte alignment; counts: 8-byte aligned.
 * DBHIP_EINVAL (before any HIP call): an unknown flag bit or op, a capacity (or their sum) of 2^32 or more, a NULL
 *   column with capacity > 0 (out_keys with a_capacity + b_capacity > 0), out_count NULL, a count pointer whose column
 *   is NULL, the value-column rules above, a misaligned pointer, an output (out_count included) overlapping an input
 *   or another output.  DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (argument errors come first).  The
 *   device is looked for after both.
 *
 * Workspace of dbench_merge_workspace_bytes(a_capacity, b_capacity) — one query serves both entry points —
 * with t = (a_capacity + b_capacity) / DBENCH_MERGE_TILE_ROWS rounded up, and W(x) = 4 x rounded up to 256:
 *   [0, 256)                            header, word 0 = status
 *   [256, 256 + W(t + 1))               t + 1 x uint32 partition points: the A elements in front of diagonal i * T
 *   [.., + W(t))                        t x uint32 kept elements per tile          (set operations)
 *   [.., + W(t))                        t x uint32 first output position per tile  (set operations)
 * 256 + W(t + 1) + 2 W(t) bytes: a multiple of 256, monotone in both capacities, at most 1024 + 3 (a_capacity +
 * b_capacity) / 512 + 12 <= 4096 + (a_capacity + b_capacity) / 4, and 0 when the sum reaches 2^32 (no such call).
 *
 * Launches behind the header's clear, all dependent, no workgroup waits for another.  Merge: partition (one thread per
 * tile boundary: the diagonal search in global memory; *out_count), merge (one workgroup per tile: both runs into LDS,
 * a diagonal search and a serial merge per thread, keys and source indices back through LDS, coalesced stores; values
 * are gathered by source index).  Set operation: partition, count (the tile body with a keep flag per merged element),
 * scan (one workgroup: counts -> positions, *out_count), write (the tile body again, compacted through LDS); the
 * count-only call stops after the scan.
 */
#ifndef DBENCH_MERGE_SORTED_HPP
#define DBENCH_MERGE_SORTED_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_MERGE_TILE_ROWS 2048 /* merged positions per workgroup */
#define DBENCH_MERGE_SIGNED 1       /* keys compare as int32 */
#define DBENCH_MERGE_ROW_IDS 2      /* out_vals = position in the concatenation instead of carried values */
#define DBENCH_SETOP_UNION 0
#define DBENCH_SETOP_INTERSECT 1
#define DBENCH_SETOP_DIFFERENCE 2   /* A minus B */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_merge_workspace_bytes(size_t a_capacity, size_t b_capacity);
int dbench_merge_u32(const uint32_t *a_keys, const uint32_t *a_vals, const uint64_t *a_count, size_t a_capacity,
                     const uint32_t *b_keys, const uint32_t *b_vals, const uint64_t *b_count, size_t b_capacity,
                     int flags, uint32_t *out_keys, uint32_t *out_vals, uint64_t *out_count, void *workspace,
                     size_t workspace_bytes, void *stream);
int dbench_setop_u32(int op, const uint32_t *a, const uint64_t *a_count, size_t a_capacity, const uint32_t *b,
                     const uint64_t *b_count, size_t b_capacity, uint32_t *out, uint64_t *out_count, void *workspace,
                     size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
