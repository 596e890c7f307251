/* hll_sketch.hpp — a HyperLogLog sketch over the rows of 1 .. 4 32-bit columns: approximate COUNT(DISTINCT) in one pass and
 * 2^p bytes, mergeable by element-wise max.  Build it from columns (all rows, or the rows of a row-id list), merge two
 * sketches, estimate on the host from the 256-byte histogram.  Plain C, exported by libdbench.so; the contract is that of
 * bloom_filter.hpp (error codes DBHIP_E*, status bits DBHIP_DEV_* of include/dbhip.h): device pointers, a caller-owned
 * 256-byte aligned workspace whose first word is the status word (cleared by a launch of its own in front of the first
 * kernel that can raise it), asynchronous on `stream`, nothing allocates, frees, synchronises or reads back, capturable into
 * a hipGraph, and repeated calls on a workspace that held anything give identical outputs.
 *
 * Format.  A sketch is (registers, p, seed): p in 4 .. 14, m = 2^p, q = 64 - p; registers is m bytes at a 4-byte aligned
 *   address, every byte in 0 .. q+1; seed a host uint32.  A row's key is the tuple of its values in n_cols = 1 .. 4 32-bit
 *   columns c_0 .. c_{k-1}; any bit pattern is allowed, no value is special (hll_layout.hpp holds this text for host and
 *   device):
 *     h = fmix32(c_0 ^ seed)            g = fmix32(c_0 ^ seed ^ 0x9E3779B9)
 *     for j = 1 .. k-1:  h = fmix32(h ^ c_j)    g = fmix32(g ^ c_j)
 *     x    = uint64(h) << 32 | g
 *     idx  = x >> (64 - p)
 *     w    = x << p                     (64-bit shift)
 *     rank = w ? clz64(w) + 1 : q + 1   (1 .. q+1)
 *   insert: registers[idx] = max(registers[idx], rank).  Max is commutative and idempotent: the registers are a function of
 *   the SET of key tuples, the same in any arrival order, with any duplicates and under any schedule.
 *   Beside the registers every build and merge writes hist: uint32 hist[64] at an 8-byte aligned address, hist[v] = the
 *   number of registers equal to v for v <= q+1, zero above.
 * estimate.  dbench_hll_estimate(hist, p) is a host function of the histogram alone and makes no HIP call: Ertl's improved
 *   raw estimator in double,
 *     z = m tau(1 - hist[q+1]/m);  for k = q down to 1: z = (z + hist[k]) / 2;  z += m sigma(hist[0]/m);
 *     E = m^2 / (2 ln 2 z)
 *   exactly 0.0 for an empty sketch, +infinity where every register is saturated, -1.0 when p is out of range, a count
 *   sits above q+1 or the counts do not sum to m.  The standard error is 1.04 / sqrt(m).
 * build.  cols[0 .. n_cols) are the columns, each of n_col rows.  Candidates.  rows == NULL: rows 0 .. min(*count, n_col)
 *   (capacity is not looked at beyond its range check).  Otherwise rows[i] for i < min(*count, capacity).  count is a device
 *   uint64 read ON THE DEVICE (NULL: all) and may hold any 64-bit value; grids are sized from n_col or capacity, so the
 *   out_count of a select can be the count of a build inside one captured graph.  The list may be unsorted and may repeat
 *   rows.  A row id >= n_col inserts nothing and raises DBHIP_DEV_KEY_RANGE; nothing outside a column's [0, n_col) is read,
 *   whatever the list holds.  Without DBENCH_HLL_ACCUMULATE the result is the sketch of the candidates alone; with it the
 *   max with what `registers` holds, where a stored byte above q+1 counts as q+1 and raises DBHIP_DEV_KEY_RANGE.  Exactly the
 *   m register bytes and the 64 histogram words are written outside the workspace.
 * merge.  dst becomes max(dst, src) byte for byte, with the same clamp and status rule for both; hist the histogram of the
 *   result.  src == dst is allowed (it recounts the histogram); any other overlap of the two is refused.
 * Columns, rows: any 4-byte alignment, each column at its own; registers: 4-byte aligned; hist, count: 8-byte aligned.
 *   n_col, capacity < 2^32.
 * DBHIP_EINVAL (before any HIP call): unknown flag bits, p outside 4 .. 14, n_cols outside 1 .. 4, a size of 2^32 or more,
 *   NULL registers, hist or cols, a NULL column with rows to read, a misaligned pointer, registers or hist overlapping a
 *   column, the list, the count or each other; merge: NULL dst, src or hist, a misaligned pointer, hist overlapping dst or
 *   src, dst and src overlapping without being equal.  DBHIP_EWORKSPACE: a NULL, short or misaligned workspace (argument
 *   errors come first).  The device is looked for after both.
 *
 * Workspace.  dbench_hll_workspace_bytes(p) = 0 for p outside 4 .. 14, otherwise the 256-byte header, 64 partial histograms
 *   of 256 bytes, and DBENCH_HLL_MAX_GRID partial sketches of m bytes: one per workgroup of the largest grid the build
 *   launches.  merge uses the header and the partial histograms alone: the workspace of any p serves it.
 *
 * Launches behind the clear of the header; no workgroup waits for another, no grid barrier, no CAS loop, no atomic that
 *   returns a value.
 *   build   a persistent grid of up to DBENCH_HLL_MAX_GRID workgroups walks segments of 4096 candidates.  A workgroup keeps
 *           the m registers in LDS as one 32-bit word each (64 KiB at p = 14: two workgroups to a CU), reads the word with a
 *           plain LDS load and issues the no-return LDS max only where the rank is larger, and stores its registers as bytes
 *           into its own slot of the workspace.
 *   reduce  one workgroup per 256 registers: the max over the slots of the workgroups that were launched (under accumulate
 *           also with the old bytes), the bytes, and a partial histogram counted in LDS.  merge is this kernel with src as
 *           its one slot.
 *   hist    one wave adds the partial histograms: one plain store per word.
 */
#ifndef DBENCH_HLL_SKETCH_HPP
#define DBENCH_HLL_SKETCH_HPP

#include <stddef.h>
#include <stdint.h>

#define DBENCH_HLL_ACCUMULATE 1 /* build: max with what `registers` holds instead of the candidates' sketch alone */
#define DBENCH_HLL_MAX_GRID 512 /* the most workgroups, and so partial sketches, of a build */

#ifdef __cplusplus
extern "C" {
#endif

size_t dbench_hll_workspace_bytes(unsigned p);
int dbench_hll_build_u32(const uint32_t *const *cols, int n_cols, size_t n_col, const uint32_t *rows, const uint64_t *count,
                         size_t capacity, uint32_t seed, int flags, unsigned p, uint8_t *registers, uint32_t *hist,
                         void *workspace, size_t workspace_bytes, void *stream);
int dbench_hll_merge(uint8_t *dst_registers, const uint8_t *src_registers, unsigned p, uint32_t *hist, void *workspace,
                     size_t workspace_bytes, void *stream);
double dbench_hll_estimate(const uint32_t *hist, unsigned p);

#ifdef __cplusplus
}
#endif
#endif
