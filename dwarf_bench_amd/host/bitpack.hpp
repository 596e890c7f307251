/* bitpack.hpp — bit-packed columns: fixed-width bit-packing over a frame of reference.  pack writes a 32-bit column in
 * `width` bits per row, unpack reads it back, densely or through a row-id list (take), and select_range filters the packed
 * form into the row-id lists of select_rows.hpp without materialising the decoded column.  Plain C, exported by
 * libdbench.so; the contract is that of include/dbhip.h as take_rows.hpp restates it (error codes DBHIP_E*, status bits
 * DBHIP_DEV_*): device pointers, a caller-owned 256-byte aligned workspace whose first word is the status word (cleared by
 * a launch in front of the first kernel that can raise it), asynchronous on `stream`, nothing allocates, frees,
 * synchronises or reads back, capturable into a hipGraph, and repeated calls on a workspace that held anything give
 * identical outputs.
 *
 * Format.  A packed column is (packed, n_rows, width, base): width a host value in 1 .. 32, base a host uint32.  Row i
 *   holds the code c_i = (v_i - base) mod 2^32, which must be < 2^width, in bits [i * width, i * width + width) of a
 *   little-endian bit stream over uint32 words: its first word is (i * width) >> 5, its first bit (i * width) & 31, least
 *   significant bit first; a code may straddle two words.  The column occupies dbench_bitpack_words(n_rows, width) words:
 *   ceil(n_rows * width / 32) rounded up to a multiple of 4 words (16 bytes), and every bit from n_rows * width up to
 *   that length is zero, so two packings of the same rows are byte-identical.  `packed` is 16-byte aligned.  32 rows are
 *   exactly `width` words, 128 rows `width` 16-byte chunks.  The decoded value is (base + c_i) mod 2^32: a signed column
 *   needs nothing special, base is the bit pattern of its minimum.  n_rows < 2^32.
 * Length.  m = min(*count, capacity); count is a device uint64 read ON THE DEVICE (NULL: m = capacity) and may hold any
 *   64-bit value.  Grids are sized from capacity: the out_count of dbench_select_range_u32, dbench_setop_u32 or
 *   dbench_bitpack_select_range_u32 can be the count of these calls inside one captured graph.  capacity < 2^32.
 * pack.  Writes exactly the dbench_bitpack_words(m, width) words of the packed form of col[0 .. m); words beyond that
 *   are not touched.  A row whose code does not fit stores its low `width` bits and raises DBHIP_DEV_KEY_RANGE in the
 *   status word; at any width below 32 that is what the DBENCH_DICT_MISS code of dict_encode.hpp does.  col: any 4-byte
 *   alignment.  Every output word is written by exactly one lane with a 16-byte vector store, no atomics; a wave owns
 *   whole groups of 32 rows, and the group that holds row m zero-fills its tail.
 * unpack.  rows == NULL: out[i] = decode(i) for every row i < n_rows (count must then be NULL, capacity is ignored).
 *   Otherwise take through a row-id list as dbench_take_u32 does it: for i < m, out[i] = decode(rows[i]) if rows[i] <
 *   n_rows; otherwise out[i] = fill and DBHIP_DEV_KEY_RANGE is raised — except that with DBENCH_BITPACK_OUTER the id
 *   0xFFFFFFFF ("no row") is filled without raising.  Entries [m, capacity) are not touched.  The list may be unsorted
 *   and may repeat rows.  Nothing outside the packed column's words is ever read, whatever the list holds; with n_rows ==
 *   0 every entry is filled.  rows and out: any 4-byte alignment.
 * select_range.  The semantics of dbench_select_range_u32 on the decoded column.  Candidates: in_rows == NULL: rows
 *   0 .. n_rows-1 in that order; otherwise in_rows[0 .. m), m = min(*in_count, in_capacity), in list order, each
 *   occurrence of a row a candidate of its own.  Candidate r is kept iff r < n_rows and (lo <= decode(r) && decode(r) <=
 *   hi) XOR DBENCH_BITPACK_NEGATE; unsigned comparison, or as int32 with DBENCH_BITPACK_SIGNED.  lo and hi are in the
 *   value domain (base + code); lo > hi is the empty interval.  Row ids >= n_rows are never kept and raise
 *   DBHIP_DEV_KEY_RANGE.  out_rows[0 .. *out_count) = the kept row ids in candidate order (stable); *out_count is always
 *   written; out_rows has room for `candidates` entries (n_rows, or in_capacity), entries from *out_count on are not
 *   touched; out_rows == NULL: the count alone.  in_rows, out_rows: any 4-byte alignment.
 * count, in_count, out_count: 8-byte aligned.
 * DBHIP_EINVAL (before any HIP call): a width outside 1 .. 32, unknown flag bits (pack takes none, unpack
 *   DBENCH_BITPACK_OUTER, select_range DBENCH_BITPACK_SIGNED and DBENCH_BITPACK_NEGATE), a size of 2^32 or more, a NULL
 *   column or output with something to read or write, out_count NULL, count without rows, a misaligned pointer (`packed`
 *   off a 16-byte boundary included), an output overlapping an input.  DBHIP_EWORKSPACE: a NULL, short or misaligned
 *   workspace (argument errors come first).  The device is looked for after both.
 *
 * Workspace of dbench_bitpack_workspace_bytes(capacity) — one query serves all three calls; capacity = the candidates of
 * select_range (n_rows, or in_capacity) — with S = capacity / DBENCH_BITPACK_SEGMENT_ROWS rounded up, A = 4 S rounded up
 * to 256:
 *   [0, 256)                       header, word 0 = status
 *   [256, 256 + A)                 S x uint32 matches per segment
 *   [256 + A, 256 + 2 A)           S x uint32 first output position per segment
 *   [256 + 2 A, 256 + 2 A + 512 S) S x 64 x uint64 match masks: bit l of word j of a segment is its candidate 64 j + l
 * A multiple of 256, monotone in capacity, at most 1536 + capacity / 7, and 0 for capacity >= 2^32 (no such call).
 * pack and unpack use the header alone: the 256 bytes of capacity 0 serve them at any size.
 *
 * Launches behind the header's clear; no workgroup waits for another.  A wave reads the packed words of its rows once,
 * with aligned 16-byte loads, into LDS, and every lane then extracts row 64 j + l of the segment in step j: the loads
 * coalesce whatever the width, and the 64 ballots of a segment are its match mask in row order.
 *   pack          one launch, a wave per tile of DBENCH_BITPACK_TILE_ROWS rows.
 *   unpack        one launch, a wave per segment.
 *   select_range  three launches as in select_rows.cpp: mark (a wave per segment: predicate -> ballots -> masks and the
 *                 segment's count), scan (one workgroup: counts -> positions, *out_count), write (segments with matches
 *                 only: masks -> ranks -> row ids; the packed column is not read again).
 */
#ifndef DBENCH_BITPACK_HPP
#define DBENCH_BITPACK_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_BITPACK_SEGMENT_ROWS 4096 /* one wave's rows in unpack and select_range */
#define DBENCH_BITPACK_TILE_ROWS 2048    /* one wave's rows in pack: 64 groups of 32 */
#define DBENCH_BITPACK_SIGNED 1          /* select_range: compare as int32 instead of uint32 */
#define DBENCH_BITPACK_NEGATE 2          /* select_range: keep the rows OUTSIDE [lo, hi] */
#define DBENCH_BITPACK_OUTER 4           /* unpack: row id 0xFFFFFFFF is "no row", not an error */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_bitpack_words(size_t n_rows, unsigned width);
size_t dbench_bitpack_workspace_bytes(size_t capacity);
int dbench_bitpack_pack_u32(const uint32_t *col, size_t capacity, const uint64_t *count, unsigned width, uint32_t base,
                            uint32_t *out_packed, void *workspace, size_t workspace_bytes, void *stream);
int dbench_bitpack_unpack_u32(const uint32_t *packed, size_t n_rows, unsigned width, uint32_t base, const uint32_t *rows,
                              const uint64_t *count, size_t capacity, int flags, uint32_t fill, uint32_t *out,
                              void *workspace, size_t workspace_bytes, void *stream);
int dbench_bitpack_select_range_u32(const uint32_t *packed, size_t n_rows, unsigned width, uint32_t base,
                                    const uint32_t *in_rows, const uint64_t *in_count, size_t in_capacity, uint32_t lo,
                                    uint32_t hi, int flags, uint32_t *out_rows, uint64_t *out_count, void *workspace,
                                    size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
