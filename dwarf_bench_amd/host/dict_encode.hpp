/* dict_encode.hpp — dictionary encoding: what lifts the single-key operators to several key columns.  build collects the
 * distinct values of a 32-bit column, orders them and keeps a table value -> rank in the workspace; encode replaces each
 * row of a column by the rank of its value (its CODE), or by DBENCH_DICT_MISS; combine folds the codes of two columns
 * into the code of the column pair in lexicographic order.  Codes are dense and order-preserving: they can be the key of
 * every single-key operator of this library, the dense group-by included, and dbench_take_u32 with DBENCH_TAKE_OUTER
 * decodes them through out_keys (DBENCH_DICT_MISS is its "no row" id).  Plain C, exported by libdbench.so; the contract
 * is that of include/dbhip.h as take_rows.hpp restates it (error codes DBHIP_E*, status bits DBHIP_DEV_*): device
 * pointers, a caller-owned 256-byte aligned workspace whose first word is the status word (cleared by a launch in front
 * of the first kernel that can raise it), asynchronous on `stream`, nothing allocates, frees, synchronises or reads back,
 * capturable into a hipGraph, and repeated calls on a workspace that held anything give identical outputs.
 *
 * Length.  m = min(*count, n); count is a device uint64 read ON THE DEVICE (NULL: m = n) and may hold any 64-bit value.
 *   Grids are sized from n.  n < 2^32.
 * build.  Let d be the number of distinct values among col[0 .. m).  capacity in [1, 2^31).
 *   d <= capacity: out_keys[0 .. d) holds them in ascending order, as uint32, or as int32 with DBENCH_DICT_SIGNED;
 *     *out_count = d; the workspace holds the dictionary, every value mapped to its index in out_keys.  out_keys[d ..
 *     capacity) is unspecified (this implementation leaves it alone: the sort and its padding live in the workspace).
 *   d > capacity: DBHIP_DEV_TABLE_FULL is raised, *out_count = 0, out_keys is not written, and until the next build every
 *     encode through this workspace answers DBENCH_DICT_MISS for every row.  Nothing outside the outputs and the
 *     workspace is written, and every probe loop is bounded.
 *   All 2^32 values are legal keys, 0 and 0xFFFFFFFF included: a slot's CODE word says whether it is used
 *   (dict_layout.hpp).  A DBHIP_DEV_RANK_ORDER raised by the inner sort is carried into this workspace's status word.
 * encode.  For i < m: out_codes[i] = the index of col[i] in the dictionary's out_keys, or DBENCH_DICT_MISS if the value
 *   is absent.  Entries [m, n) are not touched.  out_misses (optional, device uint64) = the number of misses among the m
 *   rows, always written in full.  encode only READS the workspace: any number of encodes may follow one build,
 *   concurrently on several streams; a miss is a result, not an error, and encode never raises a status bit.  A
 *   workspace that no build has filled (or whose header does not describe a table inside workspace_bytes) answers
 *   DBENCH_DICT_MISS for every row; nothing outside the workspace's bytes is read.
 * combine.  out[i] = outer[i] * *inner_card + inner[i] for i < m, or DBENCH_DICT_MISS if either input is: the code of
 *   the pair (outer, inner) among inner_card * outer_card pairs in lexicographic order.  The cardinalities are device
 *   uint64 (the out_count of two builds), so build -> encode -> combine is one captured sequence.  If *outer_card *
 *   *inner_card > 0xFFFFFFFF the composite could collide with DBENCH_DICT_MISS or wrap: DBHIP_DEV_KEY_RANGE is raised and
 *   every out[i], i < m, is DBENCH_DICT_MISS.  out may be outer itself (the same pointer).  The workspace is 256 bytes of
 *   its own, the status word alone; it is NOT the dictionary's.
 * Columns, codes and outputs: any 4-byte alignment; count, out_count, out_misses and the cardinalities: 8-byte aligned.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits, a capacity of 0 or of 2^31 or more, n of 2^32 or more, a NULL
 *   column with n > 0, a NULL output (out_misses aside; out_codes and out only with n > 0), NULL cardinalities, a
 *   misaligned pointer, an output overlapping an input or another output (combine's out == outer aside).
 *   DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (argument errors come first); encode asks for the bytes of
 *   capacity 1 and trusts no more of the header than fits the bytes it is given.  The device is looked for after both.
 *
 * Workspace of dbench_dict_workspace_bytes(capacity), with S = dict_slots(capacity) of dict_layout.hpp (the smallest
 * power of two >= 2 * capacity) and each region rounded up to 256:
 *   [0, 256)  header, word 0 = status; 8 S bytes of slots (key, code); 4 capacity bytes where the distinct keys are
 *   sorted; 4 capacity bytes, the sort's other column; dbhip_radix_sort_workspace_bytes(capacity, 8) bytes, the sort's.
 * A multiple of 256, monotone in capacity, and 0 for capacity 0 and capacity >= 2^31 (no such call).
 *
 * Hash: dict_hash of dict_layout.hpp (Murmur3's 32-bit finaliser), home slot = hash & (S - 1), linear probing.
 *
 * Launches of build, no workgroup waits for another: (1) clear the header, the table and pad the key region with the
 * order's maximum; (2) insert: the slot is read before any compare-and-swap, and a workgroup keeps the keys it has
 * inserted in a small LDS filter, so a repeated key costs one LDS read; (3) compact the used slots into the key region;
 * (4) dbhip_radix_sort_u32 / _i32 over the capacity entries; (5) look each sorted key up, store its rank in its slot and
 * the key in out_keys, write *out_count and the status.  With capacity = n the sort runs over n entries whatever d is: a
 * caller who knows a bound on d passes it.
 * encode is one launch (two with out_misses: the word is cleared first).  A table of at most DBENCH_DICT_LDS_SLOTS slots
 * is copied into LDS by every workgroup once, then rows stream through 16-byte loads, four per lane; a larger table is
 * probed in global memory, a lane's four first probes issued before the first use.
 */
#ifndef DBENCH_DICT_ENCODE_HPP
#define DBENCH_DICT_ENCODE_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_DICT_SIGNED 1 /* build: order the keys as int32 */
#define DBENCH_DICT_MISS 0xFFFFFFFFu /* the code of a value the dictionary does not hold; dbench_take_u32's "no row" id */
/* the largest table the encode kernel copies into LDS: 8192 slots x 8 bytes = 64 KiB of a compute unit's 160 KiB, so two
 * workgroups of 1024 threads are resident and the compute unit runs its full 32 waves; capacities up to 4096 */
#define DBENCH_DICT_LDS_SLOTS 8192

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_dict_workspace_bytes(size_t capacity);
int dbench_dict_build_u32(const uint32_t *col, size_t n, const uint64_t *count, size_t capacity, int flags,
                          uint32_t *out_keys, uint64_t *out_count, void *workspace, size_t workspace_bytes, void *stream);
int dbench_dict_encode_u32(const uint32_t *col, size_t n, const uint64_t *count, uint32_t *out_codes, uint64_t *out_misses,
                           const void *workspace, size_t workspace_bytes, void *stream);
int dbench_dict_combine_u32(const uint32_t *outer, const uint32_t *inner, size_t n, const uint64_t *count,
                            const uint64_t *outer_card, const uint64_t *inner_card, uint32_t *out, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
