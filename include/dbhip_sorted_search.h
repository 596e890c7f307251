/* dbhip_sorted_search.h — vectorised lower and upper bound in a sorted 32-bit column on gfx950 (thrust's lower_bound /
 * upper_bound, searchsorted on both sides): for every probe row the position and the length of the interval [lo, hi] in the
 * column, and its device-side validator.  Behind the stable argsort of dbhip.h and in front of dbhip_join_pairs_u32 this is
 * the range join
 *   SELECT b.row, p.row FROM b JOIN p ON b.key BETWEEN p.lo AND p.hi
 * and, with lo == NULL, the ASOF join.  A fifth header next to dbhip.h (whose error codes, status bits and dbhip_stream_t it
 * uses); the contract of dbhip.h holds throughout: plain C ABI, device pointers, caller-owned workspace with a 256-byte header
 * whose first word is the status word, nothing allocates, frees, synchronises or reads back, every call can be captured into
 * a graph, dependent launches only, no workgroup waits for another, every loop bounded by the sizes.  No reference
 * counterpart.
 *
 * sorted[0..m) is ascending, duplicates allowed, compared as unsigned, or as int32 when keys_signed is set.  L(x) = the number
 * of entries < x, U(x) = the number of entries <= x.  For probe row i
 *   pos[i] = lo ? L(lo[i]) : 0
 *   end    = U(hi ? hi[i] : lo[i])
 *   cnt[i] = end > pos[i] ? end - pos[i] : 0
 * hi == NULL means hi = lo (the equality join); lo == NULL means minus infinity (cnt = U(hi), pos + cnt - 1 the ASOF row).
 * On a miss pos is still the insertion point.  The answer is unique.  (sorted, pos, cnt) with the id buffer of the argsort
 * feed dbhip_join_pairs_u32 as they are.
 *
 * THE INDEX.  dbhip_sorted_index_build_u32 writes a FENCE LADDER of fan-out 64 over the column into the workspace: level 0 is
 * the column, m_0 = m; level l+1 has m_{l+1} = ceil(m_l / 64) entries, F_{l+1}[j] = F_l[min(64 j + 63, m_l - 1)], the maximum
 * of block j.  The ladder stops at the first level T with m_T <= top, top = top_entries, 0 = the default
 * DBHIP_SORTED_SEARCH_TOP = 16384 (64 KiB, what a workgroup of the search keeps in LDS); the powers of two from 64 to 16384
 * are allowed.  With the default T = 0 up to 16384 entries, 1 up to 2^20, 2 up to 2^26, 3 up to 2^31.  At most T small
 * dependent launches behind the one that writes the header; level 1 reads one word per 256 bytes of the column.  The
 * header records m, top and the signedness: the search reads them from there.
 * Workspace: the 256-byte header | level 1 | ... | level T, every level at a 256-byte offset.
 *   dbhip_sorted_index_workspace_bytes(m, top_entries) <= 1536 + m / 15 for every allowed top (default: a multiple of 256,
 *   256 for m <= 16384); 0 for m > 2^31 or a top that is not allowed.
 * DBHIP_EINVAL, before any HIP call and in this order: m > 2^31; a top_entries that is not allowed; sorted NULL with m > 0.
 * Then DBHIP_EWORKSPACE: a NULL, short or misaligned workspace.  sorted needs only its natural alignment.  m == 0 is fine
 * (the header alone).  The status word is cleared.
 *
 * THE SEARCH.  dbhip_sorted_search_u32, DBHIP_EINVAL before any HIP call and in this order: m > 2^31 or n >= 2^32 (so that
 * pos + cnt fits and the columns feed dbhip_join_pairs_u32); lo and hi both NULL; out_pos and out_cnt both NULL; hi given
 * with out_cnt NULL; sorted NULL with m > 0 and n > 0; lo, hi, out_pos or out_cnt that is not NULL and not 16-byte aligned.
 * Then DBHIP_EWORKSPACE: a NULL or misaligned workspace, or one shorter than the smallest index of m entries
 * (dbhip_sorted_index_workspace_bytes(m, 0)).  n == 0: DBHIP_OK, nothing is launched.  m == 0: pos = cnt = 0 in every row.
 * Either output column may be NULL: it is then not written.  Every column that is passed has n entries; nothing else is
 * written.  Repeated calls on one workspace give identical outputs.
 * The host cannot see what the workspace holds, so a workspace that was not built for this m is refused ON THE DEVICE: the
 * search finds another m, a top that is not allowed or an index longer than workspace_bytes in the header, writes pos = cnt =
 * 0 in every row, reads nothing else of the workspace, and raises DBHIP_DEV_KEY_RANGE in the status word — the one write
 * of the search to the workspace.  No content of sorted, lo or hi raises anything: on an index that belongs to the call the
 * status word stays as the build cleared it.
 * A `sorted` that is not sorted (or that changed after the build): the answer is unspecified, but the call reads nothing
 * outside sorted[0..m) and the workspace and still writes pos <= m and pos + cnt <= m — every step down the ladder is
 * clamped to its level — so dbhip_join_pairs_u32 cannot raise DBHIP_DEV_KEY_RANGE on it.
 *
 * How: persistent workgroups, two per compute unit.  Each stages level T into LDS once; every lane takes four consecutive
 * probe rows (16-byte loads and stores; the ragged tail row by row) and finds their bounds in LDS by binary search.  The way
 * down through levels T-1 .. 0 is wave-cooperative: for each of the wave's rows in turn the wave loads the row's 64-entry
 * block with one coalesced 256-byte load from a wave-uniform base, a ballot of entry < lo (entry <= hi) and its population
 * count give the row's offset in the block, which goes back to the owning lane.  One load instruction per row, bound and
 * level, one for both bounds when they fall into the same block; lanes behind a level's end neither load nor vote. */
#ifndef DBHIP_SORTED_SEARCH_H
#define DBHIP_SORTED_SEARCH_H

#include "dbhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DBHIP_SORTED_SEARCH_FANOUT 64 /* entries under one fence: the wave width */
#define DBHIP_SORTED_SEARCH_TOP 16384 /* default and largest number of entries of the top level */

size_t dbhip_sorted_index_workspace_bytes(size_t m, uint32_t top_entries);
int dbhip_sorted_index_build_u32(const uint32_t *sorted, size_t m, int keys_signed, uint32_t top_entries, void *workspace,
                                 size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_sorted_search_u32(const uint32_t *sorted, size_t m, const uint32_t *lo, const uint32_t *hi, size_t n,
                            uint32_t *out_pos, uint32_t *out_cnt, const void *workspace /* built above */,
                            size_t workspace_bytes, dbhip_stream_t stream);

/* Validator of (pos, cnt) against the column and the probe values, exact, by an algorithm that never searches: it checks the
 * local conditions that pin the answer on a sorted column.  With s = sorted, hi' = hi ? hi[i] : lo[i], e = pos[i] + cnt[i]
 * (64-bit), comparisons as unsigned, or as int32 when keys_signed is set:
 *   pos   pos <= m; with lo == NULL pos == 0; otherwise (pos == 0 || s[pos-1] < lo) && (pos == m || s[pos] >= lo)
 *   cnt   e <= m; if the interval is empty (lo given and hi' < lo) cnt == 0; otherwise
 *         (e == 0 || s[e-1] <= hi') && (e == m || s[e] > hi')
 * It reads only s[pos-1], s[pos], s[e-1] and s[e], each after a range check in 64-bit arithmetic, whatever the columns hold.
 * A NULL pos column stands for pos = 0 in every row and is not judged (lo == NULL with out_pos == NULL); a NULL cnt column is
 * not judged.  The four result words are set by the call:
 *   result[0]  the number of (row, column) pairs that violate their rule
 *   result[1]  the lowest violating row, or ~0 when there is none
 *   result[2]  the 64-bit sum of cnt (0 without a cnt column): the number of pairs of the join
 *   result[3]  0
 * Whether the column is sorted is dbhip_check_sorted_u32's to say.  DBHIP_EINVAL, in this order: result NULL or not 8-byte
 * aligned; m > 2^31 or n >= 2^32; lo and hi both NULL; pos and cnt both NULL; hi given with cnt NULL; pos NULL with lo given
 * and cnt given (e needs pos); sorted NULL with m > 0 and n > 0.  The columns need only their natural alignment.
 * DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (dbhip_check_sorted_search_workspace_bytes(n): a bare 256-byte
 * header, whose status word the call clears; 0 for n >= 2^32).                                                          */
size_t dbhip_check_sorted_search_workspace_bytes(size_t n);
int dbhip_check_sorted_search_u32(const uint32_t *sorted, size_t m, int keys_signed, const uint32_t *lo, const uint32_t *hi,
                                  size_t n, const uint32_t *pos, const uint32_t *cnt, uint64_t *result /* 4 words, device */,
                                  void *workspace, size_t workspace_bytes, dbhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBHIP_SORTED_SEARCH_H */
