/* bloom_filter.hpp — a Bloom filter over 32-bit keys: build it from a column (all rows, or the rows of a row-id list) and
 * probe a column against it into the row-id lists of select_rows.hpp, so that a join sees only the probe rows that can
 * have a partner.  Plain C, exported by libdbench.so; the contract is that of select_rows.hpp (error codes DBHIP_E*, status
 * bits DBHIP_DEV_* of include/dbhip.h): device pointers, a caller-owned 256-byte aligned workspace whose first word is the
 * status word (cleared by a launch of its own in front of the first kernel that can raise it), asynchronous on `stream`,
 * nothing allocates, frees, synchronises or reads back, capturable into a hipGraph, and repeated calls on a workspace that
 * held anything give identical outputs.
 *
 * Format.  A filter is (filter, n_words, seed): n_words little-endian uint64 words at an 8-byte aligned address,
 *   1 <= n_words < 2^32 (any value, no power of two needed), seed a host uint32.  A key k (any 32-bit pattern, no value is
 *   special) owns ONE word and up to four bits in it (bloom_layout.hpp holds this text for host and device):
 *     h    = fmix32(k ^ seed)
 *     word = (uint64(h) * n_words) >> 32
 *     g    = fmix32(h ^ 0x9E3779B9)
 *     mask = OR over j = 0..3 of (1ull << ((g >> (6 * j)) & 63))          positions may coincide
 *   insert: filter[word] |= mask.  test: (filter[word] & mask) == mask.  OR is commutative and idempotent: the filter is a
 *   function of the key SET, the same in any arrival order, with any duplicates and under any contention.
 *   dbench_bloom_words(n_keys, bits_per_key) = max(1, ceil(n_keys * bits_per_key / 64)); 0 for bits_per_key outside 1 .. 64
 *   or a result of 2^32 or more.
 * build.  Keys.  rows == NULL: col[0 .. m), m = min(*count, n_col) (capacity is not looked at beyond its range check).
 *   Otherwise col[rows[i]] for i < m, m = min(*count, capacity).  count is a device uint64 read ON THE DEVICE (NULL: n_col,
 *   or capacity) and may hold any 64-bit value; grids are sized from n_col or capacity, so the out_count of a select can be
 *   the count of a build inside one captured graph.  The list may be unsorted and may repeat rows.  A row id >= n_col
 *   inserts nothing and raises DBHIP_DEV_KEY_RANGE; nothing outside col[0 .. n_col) is read, whatever the list holds.
 *   Without DBENCH_BLOOM_ACCUMULATE all n_words words are zeroed by a launch in front; with it the keys are added to what
 *   the filter holds.  Exactly the n_words words are written and nothing else.
 * probe.  The semantics of dbench_select_range_u32 with the predicate "the filter may hold col[r]" (no false negatives);
 *   with DBENCH_BLOOM_NEGATE, "it certainly does not".  Candidates: in_rows == NULL: rows 0 .. n_col-1 in that order;
 *   otherwise in_rows[0 .. m), m = min(*in_count, in_capacity), in list order, each occurrence a candidate of its own.
 *   Row ids >= n_col are never kept, not even under negate, and raise DBHIP_DEV_KEY_RANGE.  out_rows[0 .. *out_count) = the
 *   kept row ids in candidate order (stable); *out_count is always written; out_rows has room for `candidates` entries
 *   (n_col, or in_capacity), entries from *out_count on are not touched; out_rows == NULL: the count alone.
 * col, rows, in_rows, out_rows: any 4-byte alignment; filter, count, in_count, out_count: 8-byte aligned.  n_col, capacity,
 *   in_capacity < 2^32.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits (build takes DBENCH_BLOOM_ACCUMULATE only, probe
 *   DBENCH_BLOOM_NEGATE only), n_words == 0 or >= 2^32, a size of 2^32 or more, a NULL filter, a NULL column with rows to
 *   read, out_count NULL, in_count without in_rows, a misaligned pointer, the filter overlapping col, the list or the count
 *   (build), out_rows overlapping the filter, col or in_rows (probe).  DBHIP_EWORKSPACE: a NULL, short or misaligned
 *   workspace (argument errors come first).  The device is looked for after both.
 *
 * Workspace.  dbench_bloom_workspace_bytes(candidates) == dbench_select_workspace_bytes(candidates), with its layout
 *   (select_rows.hpp), 0 from 2^32 on: a SelectRows plan's workspace serves a probe as it stands.  build uses the header
 *   alone: the 256 bytes of candidates = 0 serve it at any size.
 *
 * Launches behind the clears; no workgroup waits for another, no CAS loop, no atomic that returns a value.
 *   build  one launch.  A lane takes four consecutive keys per step with one aligned 16-byte load (ragged ends word by
 *          word), reads each key's filter word with a plain load and issues one 64-bit atomic OR only where a bit of the
 *          mask is missing: a stale read costs a redundant atomic, never a wrong filter.
 *   probe  three launches as in select_rows.cpp: mark (a wave per segment of 4096 candidates: the keys, then one 8-byte
 *          gather per key, test -> ballots -> masks and the segment's count), scan (one workgroup), write (select's own
 *          kernel, select_write.hpp).
 */
#ifndef DBENCH_BLOOM_FILTER_HPP
#define DBENCH_BLOOM_FILTER_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_BLOOM_ACCUMULATE 1 /* build: add the keys to what the filter holds instead of clearing it first */
#define DBENCH_BLOOM_NEGATE 2     /* probe: keep the rows the filter certainly does not hold (DBENCH_SELECT_NEGATE) */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_bloom_words(size_t n_keys, unsigned bits_per_key);
size_t dbench_bloom_workspace_bytes(size_t candidates);
int dbench_bloom_build_u32(const uint32_t *col, size_t n_col, const uint32_t *rows, const uint64_t *count, size_t capacity,
                           uint32_t seed, int flags, uint64_t *filter, size_t n_words, void *workspace,
                           size_t workspace_bytes, void *stream);
int dbench_bloom_probe_u32(const uint64_t *filter, size_t n_words, uint32_t seed, const uint32_t *col, size_t n_col,
                           const uint32_t *in_rows, const uint64_t *in_count, size_t in_capacity, int flags,
                           uint32_t *out_rows, uint64_t *out_count, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
