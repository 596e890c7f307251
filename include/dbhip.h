/*
 * dbhip.h — C ABI of libdbhip.so, the MI355X (gfx950 / CDNA4) backend for dwarf_bench's
 * data-parallel dwarf kernels.
 *
 * This is the drop-in seam behind the reference's Dwarf::run() hook (common/dwarf.hpp:15-16):
 * every `...Hip` dwarf (dwarf_bench_amd/host/) and every test / bench driver calls exactly these
 * entry points.  Plain pointers and sizes only: all data pointers are DEVICE pointers (hipMalloc'd
 * or any allocator handing out device memory, e.g. torch), `stream` is a hipStream_t passed as
 * void*, and every call is asynchronous on that stream.  Nothing here allocates, frees or
 * synchronises: scratch memory is caller-provided through the `*_workspace_bytes` queries, so a
 * call sequence can be captured into a hipGraph.  (One exception, named as such below:
 * dbhip_radix_sort_prepare, an optional calibration call that is never needed inside a capture.)
 *
 * Return value: 0 on success, a negative DBHIP_E* code for argument errors detected on the host,
 * or a positive hipError_t if a launch failed.  Device-side failures (an out-of-range group key,
 * a full hash table) are reported through the status word that
 * lives at the start of the workspace: read it back with dbhip_workspace_status() after the
 * stream has been synchronised.
 *
 * Reference interfaces replaced (file:line in kurapov-peter/dwarf_bench):
 *   dbhip_copy_if_lt_i32      scan/scan.cl:3-42 (kernel simple_two_pass_scan), scan/scan.cpp:107-128,
 *                             common/dpcpp/dpl_wrapper/dpl_wrapper.hpp:27-33 (copy_if) <- scan/dplscan.cpp:43
 *   dbhip_radix_sort_*        dpl_wrapper.hpp:35-39 (sort) <- sort/radix.cpp:34
 *   dbhip_groupby_sum_u32     groupby/groupby.cpp:58-93 (hash_build + hash_build_check),
 *                             common/dpcpp/hashtable.hpp:136-153, groupby/groupby_local.cpp:58-112
 *   dbhip_join_*              common/dpcpp/omnisci_hashtable.hpp:58-261 <- join/join_omnisci.cpp:74-88
 *   dbhip_ujoin_*             join/join.cpp:60-104, common/dpcpp/hashtable.hpp:5-93,
 *                             common/dpcpp/hashfunctions.hpp:64-137 (MurmurHash3_x86_32)
 *   dbhip_groupby_partial/merge_u32  groupby/groupby_local.cpp:52-112 (the two timed phases of GroupByLocal)
 *   dbhip_groupby_hash_u32    groupby/groupby.cpp:58-93 (GroupBy's open-addressing table keyed by the group key)
 *   dbhip_bitmask_table_*     common/dpcpp/hashtable.hpp:5-93 (SimpleNonOwningHashTable) <- hash/hash_build.cpp:8-98,
 *                             join/join.cpp:30-38, tests/hash_table_tests.cpp
 *   dbhip_cuckoo_table_*      common/dpcpp/cuckoo_hashtable.hpp (CuckooHashtable) <- hash/cuckoo_hash_build.cpp:8-120,
 *                             tests/cuckoo_hashtable_tests.cpp
 *   dbhip_slab_table_*        common/dpcpp/slab_hash.hpp (SlabHashTable) <- hash/slab_hash_build.cpp:8-112,
 *                             probe/slab_probe.cpp, join/slab_join.cpp:10-144, tests/slab_tests.cpp
 *   dbhip_reduce_sum_i32      reduce/reduce.cpp:27-88
 *   dbhip_nested_join_u32     join/nested_join.cpp:52-66
 *   dbhip_radix_sort_pairs_*  no reference counterpart (the reference sorts keys only, dpl_wrapper.hpp:35-39)
 *   dbhip_pjoin_*             no reference counterpart (multi-GPU radix-partitioned join)
 *   dbhip_join_pairs_u32      no reference counterpart (the reference stops at HashTable::lookup's {pointer, size} record,
 *                             common/dpcpp/omnisci_hashtable.hpp:12-17)
 *   dbhip_gen_*               common/common.hpp:31-40, common/common.cpp:7-20 (data generators)
 *   dbhip_exclusive_scan_u32  scan/scan.cl:44-66, tests/scan_tests.cpp:14-21, dpl_wrapper.hpp:18-25 (exclusive_scan)
 *   dbhip_check_*             the dwarfs' own result checks (scan/scan.cpp:157-164, sort/radix.cpp:46-52,
 *                             groupby/groupby.cpp:95-103, join/join_omnisci.cpp:31-45, join/join.cpp:133-137)
 */
#ifndef DBHIP_H
#define DBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBHIP_VERSION 1

/* host-side argument errors (negative); positive values are hipError_t */
#define DBHIP_OK 0
#define DBHIP_EINVAL (-1)     /* null pointer / bad size / bad parameter */
#define DBHIP_EWORKSPACE (-2) /* workspace too small or misaligned (needs 256-byte alignment) */
#define DBHIP_ENODEVICE (-3)  /* no HIP device / not a gfx950-class device */

/* device-side status word values (dbhip_workspace_status) */
#define DBHIP_DEV_OK 0u
#define DBHIP_DEV_SPIN_TIMEOUT 1u  /* dbhip_copy_if_lt_dense_i32 and the single-launch path of dbhip_exclusive_scan_u32:
                                      a chunk waited 2 s for its predecessors (never seen); the output is then wrong;
                                      the slab table: an insert reached a loop bound (a workspace that was not reset) */
#define DBHIP_DEV_KEY_RANGE 2u     /* group key >= groups_count, or the 0xFFFFFFFF sentinel as a join build key;
                                      dbhip_join_pairs_u32: a probe row whose id range leaves the id buffer */
#define DBHIP_DEV_TABLE_FULL 4u    /* open-addressing table wrapped without finding a slot: the bitmask-claimed table (a
                                      table that really is full: the reference spins forever there) and the small-input
                                      unique-key table; the cuckoo table: an insert's eviction chain reached max_iter
                                      exchanges and the pair it carried was dropped (a normal result: rebuild with other
                                      seeds); the slab table: its overflow pool ran out and the row was not
                                      stored.  NOT the LDS-partitioned joins (dbhip_join_build* / _radix_* /
                                      dbhip_ujoin_* from 2^16 rows): a partition with more distinct keys than its 3072-slot
                                      LDS sub-table holds is built in a spill table of its own, any keys join (the one
                                      exception: a one-to-many build of exactly 2^31 rows has no spare bit to mark such a
                                      sub-table and still raises this).  dbhip_join_pairs_u32: more pairs than the
                                      caller's capacity (a normal result: *out_pairs holds the total) */
#define DBHIP_DEV_RANK_ORDER 8u    /* radix sort: a tile re-ordered by the pass's digit was not sorted by its lower digits —
                                      the ranking was not stable (or an earlier pass was damaged); the output is wrong */

typedef void *dbhip_stream_t; /* hipStream_t */

/* ---- library / device ------------------------------------------------------------------- */
int dbhip_version(void);
/* Fills name (<=len bytes), compute units and wavefront size of HIP device `device`. */
int dbhip_device_info(int device, char *name, size_t len, int *compute_units, int *wave_size);
/* Asynchronously copies the status word of a workspace to *host_status (pinned or pageable),
 * then synchronises `stream`.  Convenience for hosts that have no other D2H path. */
int dbhip_workspace_status(const void *workspace, uint32_t *host_status, dbhip_stream_t stream);

/* ---- deterministic synthetic data (counter-based; oracle/dbo.c dbo_gen_uniform_u32 / dbo_gen_unique_sorted_u32 are the CPU twins) ---------
 * element i of the logical column = lo + mix64(seed, first_index + i) % (hi - lo + 1)            */
int dbhip_gen_uniform_u32(uint32_t *out, size_t n, uint64_t seed, uint64_t first_index,
                          uint32_t lo, uint32_t hi, dbhip_stream_t stream);
/* the same column read at given positions: out[i] = lo + mix64(seed, indices[i]) % (hi - lo + 1) (a key column
 * regenerated in the order of a list of row ids: the partitioned join's checks) */
int dbhip_gen_uniform_at_u32(uint32_t *out, const uint32_t *indices, size_t n, uint64_t seed, uint32_t lo, uint32_t hi,
                             dbhip_stream_t stream);
/* unique ascending keys in [0, 10*N): element i = 10*(first_index+i) + mix64(seed, first_index+i) % 10
 * (same shape as helpers::make_unique_random, common/common.cpp:7-20) */
int dbhip_gen_unique_sorted_u32(uint32_t *out, size_t n, uint64_t seed, uint64_t first_index,
                                dbhip_stream_t stream);

/* ---- dwarf 1: scan / stream compaction --------------------------------------------------------
 * out[0..*out_size) = [x in src : x < filter_value] in source order (stable), *out_size = count.
 * src is read ONCE: a chunked kernel stages each chunk's matches in the workspace (which therefore holds n
 * elements) and a second small kernel moves them to their final offsets; no workgroup waits on another.  `out` needs room for n elements in the worst case.
 * out_size is a DEVICE pointer to one uint64.                                                    */
size_t dbhip_copy_if_lt_i32_workspace_bytes(size_t n);
int dbhip_copy_if_lt_i32(const int32_t *src, size_t n, int32_t filter_value, int32_t *out,
                         uint64_t *out_size, void *workspace, size_t workspace_bytes,
                         dbhip_stream_t stream);

/* The same compaction for DENSE predicates (more than about a tenth of the rows match): one launch, every match
 * written once at its final position (HBM bytes 4n + 4*out_size instead of 4n + 12*out_size).  A workgroup keeps
 * three quarters of its 128 KiB chunk in registers while it waits for the number of matches in front of the chunk
 * and reads the remaining quarter a second time (on-die) during that wait.  Chunks are taken by ticket, so every
 * wait is on a workgroup that is already running; waits are bounded (DBHIP_DEV_SPIN_TIMEOUT).
 * Same arguments, results and workspace size as dbhip_copy_if_lt_i32; slower than it for sparse predicates.        */
int dbhip_copy_if_lt_dense_i32(const int32_t *src, size_t n, int32_t filter_value, int32_t *out,
                               uint64_t *out_size, void *workspace, size_t workspace_bytes,
                               dbhip_stream_t stream);

/* ---- dwarf 2: LSD radix sort ---------------------------------------------------------------
 * Ascending sort of n 32-bit keys.  keys is sorted IN PLACE; tmp is an n-element ping-pong buffer.
 * radix_bits in {4, 8}: digit width of every pass (4 = the configuration named in BASELINE.json,
 * 8 = the tuned variant).  Passes whose digit is constant over the whole input are skipped.
 * keys and tmp must be 16-byte aligned (DBHIP_EINVAL otherwise).                                   */
size_t dbhip_radix_sort_workspace_bytes(size_t n, int radix_bits);
int dbhip_radix_sort_u32(uint32_t *keys, uint32_t *tmp, size_t n, int radix_bits, void *workspace,
                         size_t workspace_bytes, dbhip_stream_t stream);
/* signed order (the reference sorts `int`, sort/radix.cpp:8-12) */
int dbhip_radix_sort_i32(int32_t *keys, int32_t *tmp, size_t n, int radix_bits, void *workspace,
                         size_t workspace_bytes, dbhip_stream_t stream);
/* How the scatter ranks keys on the current device: 1 = one returning LDS atomic per key, 0 = wave ballots, -1 = no
 * device.  The atomic ranking is stable only if same-address lanes of one ds_add_rtn are served in lane order; gfx950
 * does that, the ISA manual does not promise it.  It is therefore (a) the default on gfx950 only, (b) watched by every
 * tile of every sort through the invariant it exists for: inside each run of 64 keys (a wave's row) of a tile re-ordered
 * by the pass's digit, every key is compared with its left neighbour under the mask of the digits sorted so far
 * (DBHIP_DEV_RANK_ORDER in the status word if a pair is out of order: about 2 % of the sort's time).  The pairs that
 * straddle two rows (one in 64) or two tiles are NOT compared: a tripwire for an unstable rank or a damaged earlier
 * pass, not a proof of sortedness.  And (c) pinned by dbhip_radix_sort_prepare.  The
 * same ranking is used inside and outside graph captures.  DBHIP_RS_RANK=ballot|atomic overrides.                 */
int dbhip_radix_sort_rank_mode(void);
/* OPTIONAL calibration, the one call of this library that allocates (a scratch word) and SYNCHRONISES `stream`: runs
 * a device-side self-test of the property above on every CU (~50 us) and pins the ranking of the current device to
 * what it saw (atomics where no lane ever disagreed with the ballots' prediction, ballots otherwise).  Returns the
 * resulting rank mode (1 / 0), DBHIP_EINVAL while `stream` is being captured, or an error code.  The sort entry
 * points never call it and never synchronise.                                                                    */
int dbhip_radix_sort_prepare(dbhip_stream_t stream);

/* ---- dwarf 2, key-value sort and argsort (no reference counterpart: the reference sorts keys only) ----------
 * Ascending STABLE sort of n (key, value) pairs, both columns in place: keys ends up ascending (_u32 as unsigned, _i32 as
 * signed: the sign bit is flipped on the fly as in dbhip_radix_sort_i32, keys unchanged), vals[i] is the value that
 * travelled with keys[i], equal keys keep their input order.  The result is therefore unique:
 * vals_out == vals_in[argsort_stable(keys_in)].  vals is 32 bits of anything, no value is special.  tmp_keys and tmp_vals
 * are n-element ping-pong buffers.
 *   vals_are_row_ids != 0  the argsort: vals is treated as holding 0..n-1 on entry and is NEVER READ (the first executed
 *                          pass makes the ids from the row position: 4n bytes of reads saved); on return vals is the
 *                          stable sort permutation.  Also when no pass executes (all keys equal, n == 1, every digit
 *                          constant): vals = 0..n-1, keys unchanged.
 * radix_bits in {4, 8}; n < 2^32 (the keys-only bound: row ids then fit 32 bits); all four buffers 16-byte aligned.
 * DBHIP_EINVAL: a NULL buffer with n > 0, other radix_bits, n >= 2^32, a misaligned buffer; DBHIP_EWORKSPACE: a short or
 * misaligned workspace — all before any HIP call.  n == 0 is DBHIP_OK (a workspace that was passed gets a clean status
 * word).  Never allocates, never synchronises, can be captured; ranks as dbhip_radix_sort_rank_mode() says, and every
 * tile runs the order check of the keys-only sort (DBHIP_DEV_RANK_ORDER); skipped passes are decided on the device.
 * The workspace is the keys-only layout (the kernels that fill it never see the values): the query returns
 * dbhip_radix_sort_workspace_bytes(n, radix_bits).                                                               */
size_t dbhip_radix_sort_pairs_workspace_bytes(size_t n, int radix_bits);
int dbhip_radix_sort_pairs_u32(uint32_t *keys, uint32_t *vals, uint32_t *tmp_keys, uint32_t *tmp_vals, size_t n,
                               int radix_bits, int vals_are_row_ids, void *workspace, size_t workspace_bytes,
                               dbhip_stream_t stream);
int dbhip_radix_sort_pairs_i32(int32_t *keys, uint32_t *vals, int32_t *tmp_keys, uint32_t *tmp_vals, size_t n,
                               int radix_bits, int vals_are_row_ids, void *workspace, size_t workspace_bytes,
                               dbhip_stream_t stream);

/* ---- dwarf 3: group-by hash aggregate, SUM ------------------------------------------------------
 * out[g] = sum of vals[i] over rows with keys[i] == g (uint32 wrap-around), g in [0, groups).
 * Keys must be < groups (the reference's dense output[key] contract, groupby/groupby.cpp:88-91);
 * a larger key sets DBHIP_DEV_KEY_RANGE and is ignored.  keys and vals must be 16-byte aligned
 * (DBHIP_EINVAL otherwise); the scan, reduce and exclusive-scan entry points take any 4-byte aligned column. */
size_t dbhip_groupby_sum_u32_workspace_bytes(size_t n, uint32_t groups);
int dbhip_groupby_sum_u32(const uint32_t *keys, const uint32_t *vals, size_t n, uint32_t groups,
                          uint32_t *out, void *workspace, size_t workspace_bytes,
                          dbhip_stream_t stream);

/* The two phases on their own (GroupByLocal reports group_by_time and reduction_time separately,
 * groupby/groupby_local.cpp:115-119): partial = private per-workgroup LDS tables written to the workspace,
 * merge = their sum into out[].  max_private_tables caps the number of private tables per key range
 * (the reference's `executors`); 0 = one per compute unit.  Same workspace size as the fused call.      */
int dbhip_groupby_partial_u32(const uint32_t *keys, const uint32_t *vals, size_t n, uint32_t groups,
                              uint32_t max_private_tables, void *workspace, size_t workspace_bytes,
                              dbhip_stream_t stream);
int dbhip_groupby_merge_u32(uint32_t groups, uint32_t max_private_tables, uint32_t *out, const void *workspace,
                            dbhip_stream_t stream);

/* ---- dwarf 3b: group-by on arbitrary 32-bit keys, SUM and COUNT (hash aggregation) -------------------------------
 * One output row per distinct key k of keys[0..n): out_keys[i] = k, out_sums[i] = the sum of its vals (uint32
 * wrap-around), out_counts[i] = its number of rows; *out_groups (a DEVICE uint64, like copy_if's out_size) = the number of
 * rows written.  The order of the rows is unspecified.  out_counts may be NULL: no counting.  Every key value is a key,
 * 0xFFFFFFFF included (the tables' empty marker: those rows are summed on the side, never lost, never flagged).
 * max_groups is the caller's bound on the number of distinct keys and the capacity of the three output arrays; 0 = n.
 * More distinct keys than max_groups: DBHIP_DEV_TABLE_FULL in the workspace status word, nothing written past max_groups
 * entries, *out_groups = max_groups; every probe loop is bounded (no fault, no hang).  keys and vals must be 16-byte aligned
 * (DBHIP_EINVAL otherwise); n <= 2^31; NULL pointers (out_counts aside) and n > 2^31 are DBHIP_EINVAL, a small workspace
 * DBHIP_EWORKSPACE, all before any HIP call.  n = 0 gives *out_groups = 0.  Never synchronises, never allocates; repeated
 * calls on one workspace give the same multiset of rows whatever the workspace held before.
 * The path is chosen on the host from max_groups alone (min(max_groups, n) distinct keys at most):
 *   <= 4096: private LDS tables per workgroup, one global insert per (workgroup, group) at the end;
 *   more:    the radix join's hash partitioning of the (key, val) pairs, then one workgroup per ~2048-row partition
 *            aggregates it in LDS and writes its groups out (hot keys: the partition is sliced over many workgroups).
 * So a caller who knows the number of keys is small should pass it: max_groups = n is always correct, and slower.
 * Workspace: a global table of 2 * min(max_groups, n) slots (at least 64) of key | sum | count, 24 bytes per group of the
 * bound, and for the partitioned path 16 bytes per row of pair buffers plus the partition offsets (~1 MiB): at most
 * 65 bytes per row plus 2 MiB.  DBHIP_GBH_PATH=lds|part|global pins a path (read once; global = every row into the table in HBM).   */
size_t dbhip_groupby_hash_workspace_bytes(size_t n, uint32_t max_groups);
int dbhip_groupby_hash_u32(const uint32_t *keys, const uint32_t *vals, size_t n, uint32_t max_groups, uint32_t *out_keys,
                           uint32_t *out_sums, uint32_t *out_counts, uint64_t *out_groups, void *workspace,
                           size_t workspace_bytes, dbhip_stream_t stream);

/* ---- dwarf 4a: one-to-many hash join (JoinOmnisci semantics) -----------------------------------
 * Build: hash table over the DISTINCT build keys, per-key match count, exclusive scan -> position,
 * ids[pos .. pos+count) = build row indices carrying that key (order inside a key's range is not
 * defined, as in the reference).  Probe: per probe row i, out_count[i] = number of build rows with
 * the same key and out_pos[i] = offset of their ids (0/0 on a miss).
 * 0xFFFFFFFF is the empty-slot sentinel and must not occur as a key
 * (join/join_omnisci.cpp:52): a build row carrying it sets DBHIP_DEV_KEY_RANGE and is dropped, a probe row
 * carrying it gets 0/0.  The table lives in the workspace between build and probe; the
 * probe takes n_build again because the table geometry is a pure function of it.
 * A key may repeat any number of times: the rows of a hot key are shared by all workgroups (from 2^18 build rows
 * on; a build in which every other row carries one key takes 1.3-1.6 x the time of uniform keys).  ANY keys join,
 * as with the reference's table (common/dpcpp/omnisci_hashtable.hpp:80-108, ht_size = 2 * distinct keys,
 * join/join_omnisci.cpp:69-70): keys that crowd one partition of the internal radix partitioning beyond its LDS
 * sub-table (constructed against the hash: hashed keys never do) are joined through a spill table — slowly,
 * correctly.  The workspace is 46 bytes per build row (12 table + 16 partition scratch + 18 spill pool).       */
size_t dbhip_join_workspace_bytes(size_t n_build);
int dbhip_join_build_u32(const uint32_t *build_keys, size_t n_build, uint32_t *ids, void *workspace,
                         size_t workspace_bytes, dbhip_stream_t stream);
/* same build over (key, row id) pairs: ids[] receives build_row_ids[] values instead of 0..n-1
 * (the partitioned multi-GPU join builds on received pairs carrying GLOBAL row ids) */
int dbhip_join_build_pairs_u32(const uint32_t *build_keys, const uint32_t *build_row_ids, size_t n_build,
                               uint32_t *ids, void *workspace, size_t workspace_bytes,
                               dbhip_stream_t stream);
int dbhip_join_probe_u32(const uint32_t *probe_keys, size_t n_probe, const void *workspace,
                         size_t n_build, uint32_t *out_pos, uint32_t *out_count,
                         dbhip_stream_t stream);

/* ---- dwarf 4a, radix join: the same one-to-many join for callers that do not need the results in probe-row order
 * (the multi-GPU join, whose results stay sharded anyway).  Both sides are partitioned with the BUILD side's geometry
 * (a pure function of n_build), then ONE launch builds every partition's sub-table in LDS and probes it with the
 * probe rows of the same partition while it is still there: no table in HBM, no random access leaves a CU.
 * Outputs: ids[] grouped by key as above; out_probe_row_ids / out_pos / out_count hold, in the probe side's PARTITION
 * order, each probe row's id (probe_row_ids[i], or i when probe_row_ids is NULL), the offset of its ids and their
 * number.  The three steps are separate entry points so that a host can overlap them with other work (the build
 * side's partition call opens a join: it clears the status word and must come first); dbhip_join_radix_u32 runs all
 * three.  The match may be repeated on one partitioned pair: every match gives the same answers (the order of ids
 * inside one key's range aside).  n_probe is at most 2^32 - 2048 (the fused kernel's 32-bit probe-row indices step
 * 2048 rows at a time); larger sizes are DBHIP_EINVAL in the partition and match calls.  Same contract as above (the
 * sentinel key is flagged; any other keys join).                                                                   */
size_t dbhip_join_radix_workspace_bytes(size_t n_build, size_t n_probe);
int dbhip_join_radix_partition_u32(int probe_side, const uint32_t *keys, const uint32_t *row_ids, size_t n,
                                   size_t n_build, size_t n_probe, void *workspace, size_t workspace_bytes,
                                   dbhip_stream_t stream);
int dbhip_join_radix_match_u32(size_t n_build, size_t n_probe, uint32_t *ids, uint32_t *out_probe_row_ids,
                               uint32_t *out_pos, uint32_t *out_count, void *workspace, size_t workspace_bytes,
                               dbhip_stream_t stream);
int dbhip_join_radix_u32(const uint32_t *build_keys, const uint32_t *build_row_ids, size_t n_build,
                         const uint32_t *probe_keys, const uint32_t *probe_row_ids, size_t n_probe, uint32_t *ids,
                         uint32_t *out_probe_row_ids, uint32_t *out_pos, uint32_t *out_count, void *workspace,
                         size_t workspace_bytes, dbhip_stream_t stream);

/* The reference's answer record (JoinOneToMany<global_ptr<size_t>>, common/dpcpp/omnisci_hashtable.hpp:12-17: pointer
 * into the id buffer + number of ids) for callers that want that shape instead of two 32-bit columns:
 * answers[i] = {ids + out_pos[i], out_count[i]} (a miss: {ids, 0}).  16 bytes per probe row.          */
typedef struct dbhip_join_one_to_many {
  const uint32_t *vals;
  size_t size;
} dbhip_join_one_to_many;
int dbhip_join_answers_u32(const uint32_t *ids, const uint32_t *out_pos, const uint32_t *out_count, size_t n_probe,
                           dbhip_join_one_to_many *answers, dbhip_stream_t stream);

/* ---- dwarf 4a, the join result as rows (no reference counterpart: OmniSci::HashTable::lookup stops at the per-row
 * {pointer, size} record) ----------------------------------------------------------------------------------------------
 * Turns the answer of either one-to-many join into the table of matching (build row, probe row) pairs.  Input: (ids, pos,
 * cnt) of dbhip_join_probe_u32 (probe-row order, probe_row_ids = NULL: probe row i has id i) or (ids, out_probe_row_ids,
 * out_pos, out_count) of dbhip_join_radix_match_u32.  With rid(i) = probe_row_ids ? probe_row_ids[i] : i, e[i] = cnt[i]
 * (inner) or max(cnt[i], 1) (left_outer != 0) and off the 64-BIT exclusive prefix sum of e: for k < cnt[i], pair number
 * off[i] + k is (ids[pos[i] + k], rid(i)); a probe row with cnt[i] == 0 yields in left-outer mode the one pair
 * (0xFFFFFFFF, rid(i)).  The pairs are thus grouped by probe row in input order and follow the id buffer inside a row:
 * given (ids, pos, cnt) the output is unique.  *out_pairs (a DEVICE uint64, like copy_if's out_size) = the sum of e, always
 * the full total, which may exceed 2^32.
 *   capacity   entries of out_build_rows and of out_probe_rows.  Only pairs numbered below it are written; a total above
 *              it sets DBHIP_DEV_TABLE_FULL in the workspace status word, and *out_pairs still holds the total, so a caller
 *              can allocate and call again.  The count-only call, capacity == 0 with both output pointers NULL, computes
 *              *out_pairs alone and never raises DBHIP_DEV_TABLE_FULL.
 *   a row with pos[i] + cnt[i] > n_build (not an answer of this library) counts as cnt[i] = 0 and sets
 *              DBHIP_DEV_KEY_RANGE: nothing outside ids[0..n_build) is read whatever the input holds.
 * Any 4-byte aligned columns, inputs and outputs (16-byte stores are used when both output columns sit at the same distance
 * from a 16-byte boundary).  n_probe < 2^32, n_build <= 2^31, as in the joins.  n_probe == 0: *out_pairs = 0 (when given)
 * and a clean status word (when a workspace is given).  DBHIP_EINVAL: sizes out of range, a NULL output with capacity > 0,
 * and with n_probe > 0 a NULL ids (n_build > 0), pos, cnt, out_pairs or workspace; DBHIP_EWORKSPACE: a short or misaligned
 * workspace; all before any HIP call.  Never allocates, never synchronises, no workgroup waits on another (four dependent
 * launches: chunk sums, their scan, the row offsets, the expansion), can be captured into a graph, and gives the same
 * answers whatever the workspace held before.  The expansion is partitioned by output: a fixed grid takes equal chunks of
 * 2048 items, an item being a probe row or a pair, so neither a row with millions of matches nor millions of rows with no
 * match make one workgroup's share longer than another's.
 * Workspace: 256-byte header (status word, total, pairs written) | 4096 chunk sums | off[n_probe], 8 bytes per probe row;
 * the query returns 0 for n_probe >= 2^32.                                                                           */
size_t dbhip_join_pairs_workspace_bytes(size_t n_probe);
int dbhip_join_pairs_u32(const uint32_t *ids, size_t n_build, const uint32_t *probe_row_ids, const uint32_t *pos,
                         const uint32_t *cnt, size_t n_probe, int left_outer, uint64_t capacity,
                         uint32_t *out_build_rows, uint32_t *out_probe_rows, uint64_t *out_pairs, void *workspace,
                         size_t workspace_bytes, dbhip_stream_t stream);

/* ---- dwarf 4b: unique-key join carrying payloads (Join semantics, join/join.cpp:60-104) ---------
 * Build keys are unique.  For probe row i: on a hit out_key[i] = key, out_build_val[i] = payload of
 * the build row, out_probe_val[i] = probe payload; on a miss all three are left at 0xFFFFFFFF
 * (the caller's sentinel fill, join/join.cpp:41-43 — this call writes the sentinel itself).       */
size_t dbhip_ujoin_workspace_bytes(size_t n_build);
int dbhip_ujoin_build_u32(const uint32_t *build_keys, const uint32_t *build_vals, size_t n_build,
                          void *workspace, size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_ujoin_probe_u32(const uint32_t *probe_keys, const uint32_t *probe_vals, size_t n_probe,
                          const void *workspace, size_t n_build, uint32_t *out_key,
                          uint32_t *out_build_val, uint32_t *out_probe_val, dbhip_stream_t stream);

/* ---- bitmask-claimed table: HIP counterpart of SimpleNonOwningHashTable (common/dpcpp/hashtable.hpp:5-93),
 * the table of the reference's Join / HashBuild dwarfs: slots claimed by fetch_or on an occupancy bitmask
 * + ctz over occupied runs; duplicate keys take separate slots.  hash_kind 0 = key % table_size
 * (StaticSimpleHasher / SimpleHasher), 1 = MurmurHash3_x86_32(key, seed) % table_size
 * (hashfunctions.hpp:64-137).  serial != 0 inserts with ONE work-item in input order (reproduces the slot
 * layouts the reference's hash_table_tests expect).  Workspace: header | keys[size] | vals[size] | bitmask. */
size_t dbhip_bitmask_table_workspace_bytes(size_t table_size);
int dbhip_bitmask_table_reset(void *workspace, size_t workspace_bytes, size_t table_size, dbhip_stream_t stream);
int dbhip_bitmask_table_insert_u32(const uint32_t *keys, const uint32_t *vals, size_t n, void *workspace,
                                   size_t workspace_bytes, size_t table_size, int hash_kind, uint32_t seed,
                                   int serial, dbhip_stream_t stream);
int dbhip_bitmask_table_lookup_u32(const uint32_t *keys, size_t n, const void *workspace, size_t table_size,
                                   int hash_kind, uint32_t seed, uint32_t *out_vals, uint32_t *out_found,
                                   dbhip_stream_t stream);

/* ---- cuckoo table: HIP counterpart of CuckooHashtable (common/dpcpp/cuckoo_hashtable.hpp), the table of the
 * reference's CuckooHashBuild dwarf.  Two positions per key, h1(k) and h2(k): hash_kind 0 = (k % size + seed) % size
 * (StaticSimpleHasher / StaticSimpleHasherWithOffset, hashfunctions.hpp:33-41), 1 = MurmurHash3_x86_32(k, seed) % size
 * (hashfunctions.hpp:64-130), 2 = (mix64(seed, k) >> 32) % size (the generators' splitmix64); seed1 makes h1, seed2
 * makes h2.  Kind 1 is the reference's pair, but two Murmur3 seeds are related by an XOR: for every key there is a key
 * whose two positions are the same two slots swapped, and from about 2^22 keys a build fails for any seeds (DESIGN.md
 * §4).  Kind 2 is the pair for large builds.  Workspace: header | slots[table_size] of 8 bytes,
 * key in the low word and value in the high word, empty = key 0xFFFFFFFF / value 0; table_size <= 2^32 - 1.
 *   reset   clears the status word and empties every slot.
 *   insert  lock-free: each row carries its (key, value) pair through a chain of 64-bit atomic exchanges, from h1(key)
 *           on, each evicted pair moving to its other position (cuckoo_hashtable.hpp:43-63); the chain ends at an empty
 *           slot or after max_iter exchanges (0 = the reference's min(n, 100000); at most 2^20), where the pair carried
 *           last is DROPPED, as in the reference, and DBHIP_DEV_TABLE_FULL is ORed into the status word.  Key
 *           0xFFFFFFFF is not stored (DBHIP_DEV_KEY_RANGE).  out_inserted (nullable) gets 1 / 0 per row.  The status
 *           word accumulates until the next reset.  serial != 0 inserts with ONE work-item in input order (reproduces
 *           the slot layouts and per-insert results of the reference's cuckoo_hashtable_tests).
 *           Rebuilding with other seeds after a failure is the caller's job (hash/cuckoo_hash_build.cpp:43-92).
 *   lookup  after an insert call has finished (a pair that is being moved sits in no slot): h1(k), then h2(k) only if
 *           the h1 slot holds another key; out_vals[i] = the value or 0, out_found[i] = 1 / 0.  The h1 slot wins when
 *           both hold k (duplicate keys; at(), :29-37).
 *   export  out_keys[i] / out_vals[i] = the pair in slot i (the slot layout, for tests and callers).           */
size_t dbhip_cuckoo_table_workspace_bytes(size_t table_size);
int dbhip_cuckoo_table_reset(void *workspace, size_t workspace_bytes, size_t table_size, dbhip_stream_t stream);
int dbhip_cuckoo_table_insert_u32(const uint32_t *keys, const uint32_t *vals, size_t n, void *workspace,
                                  size_t workspace_bytes, size_t table_size, int hash_kind, uint32_t seed1,
                                  uint32_t seed2, uint32_t max_iter, int serial, uint32_t *out_inserted /* nullable */,
                                  dbhip_stream_t stream);
int dbhip_cuckoo_table_lookup_u32(const uint32_t *keys, size_t n, const void *workspace, size_t table_size,
                                  int hash_kind, uint32_t seed1, uint32_t seed2, uint32_t *out_vals,
                                  uint32_t *out_found, dbhip_stream_t stream);
int dbhip_cuckoo_table_export_u32(const void *workspace, size_t table_size, uint32_t *out_keys,
                                  uint32_t *out_vals, dbhip_stream_t stream);

/* ---- slab table: HIP counterpart of SlabHashTable (common/dpcpp/slab_hash.hpp), the table of the reference's
 * SlabHashBuild, SlabProbe and SlabJoin dwarfs.  A multimap: bucket = ((A*k + B) % P) % buckets, computed exactly as
 * DefaultHasher<A, B, P> does in 64 bits (:60-64; A, B <= 2^32 - 1, 1 <= P <= 2^32 - 1); each bucket heads a chain of
 * slabs of 32 (key, value) slots (SLAB_SIZE, :20-22), node b being bucket b's root slab and nodes
 * [buckets, buckets + pool_nodes) the overflow pool (the reference's heap, :84-99, with its end checked); buckets >= 1,
 * buckets + pool_nodes <= 2^32 - 1.  Workspace: header (status word, pool cursor) | vals[nodes][32] | keys[nodes][32] |
 * 8-byte link words[nodes]; empty = key 0xFFFFFFFF, value 0.
 *   reset   clears the status word and the pool cursor, empties every slab and unlinks every node.
 *   insert  lock-free (the reference appends slabs under a spin lock, :209-222): each row goes into the first empty slot
 *           of the first slab of its chain that has one (:224-262), a duplicate key into a slot of its own; a full
 *           chain gets a pool node linked at its end with one CAS.  Pool exhausted: the row is NOT stored and
 *           DBHIP_DEV_TABLE_FULL is ORed into the status word (the reference writes past its heap, :92-97).  Key
 *           0xFFFFFFFF is not stored (DBHIP_DEV_KEY_RANGE).  Every loop is bounded (a chain walk by buckets + pool_nodes
 *           steps, a slab by 32 CASes); DBHIP_DEV_SPIN_TIMEOUT: a bound was reached or a link pointed outside the
 *           table (a workspace that was not reset), the row is not stored.  out_inserted (nullable) gets 1 / 0 per row.
 *           serial != 0 inserts with ONE group in input order: the slot, slab and chain layout of a sequential run of
 *           the reference's algorithm.  A concurrent insert may leave one pool node unlinked per row group (a group
 *           that loses the race to link a node keeps it for its next append; pool_used counts it), at most
 *           DBHIP_SLAB_INSERT_GROUPS in all.
 *   lookup  after an insert call has finished: out_vals[i] = the value of the first slot, in chain and slot order,
 *           that holds keys[i] (find(), :177-196, :264-294), or 0; out_found[i] = 1 / 0.
 *   join_probe  SlabJoin's probe (join/slab_join.cpp:88-111) in dbhip_ujoin_probe_u32's convention: for probe row i
 *           out_key[i] = the key, out_build_val[i] = lookup's value, out_probe_val[i] = probe_vals[i] on a hit, and all
 *           three 0xFFFFFFFF on a miss (the reference marks a miss with key 0 and loses a real key 0, :127).
 *   export  out_keys / out_vals[node * 32 + slot], out_next[node] (0xFFFFFFFF: none), *out_pool_used = pool nodes
 *           taken (at most pool_nodes): the layout, for tests and callers.                                          */
#define DBHIP_SLAB_INSERT_GROUPS 16384 /* most row groups of one concurrent insert call: it leaves at most this many
                                         pool nodes unlinked, so a pool of (overflow slabs needed) + this never runs out */
size_t dbhip_slab_table_workspace_bytes(size_t buckets, size_t pool_nodes);
int dbhip_slab_table_reset(void *workspace, size_t workspace_bytes, size_t buckets, size_t pool_nodes,
                           dbhip_stream_t stream);
int dbhip_slab_table_insert_u32(const uint32_t *keys, const uint32_t *vals, size_t n, void *workspace,
                                size_t workspace_bytes, size_t buckets, size_t pool_nodes, uint64_t hash_a,
                                uint64_t hash_b, uint64_t hash_p, int serial, uint32_t *out_inserted /* nullable */,
                                dbhip_stream_t stream);
int dbhip_slab_table_lookup_u32(const uint32_t *keys, size_t n, const void *workspace, size_t buckets,
                                size_t pool_nodes, uint64_t hash_a, uint64_t hash_b, uint64_t hash_p,
                                uint32_t *out_vals, uint32_t *out_found, dbhip_stream_t stream);
int dbhip_slab_table_join_probe_u32(const uint32_t *probe_keys, const uint32_t *probe_vals, size_t n,
                                    const void *workspace, size_t buckets, size_t pool_nodes, uint64_t hash_a,
                                    uint64_t hash_b, uint64_t hash_p, uint32_t *out_key, uint32_t *out_build_val,
                                    uint32_t *out_probe_val, dbhip_stream_t stream);
int dbhip_slab_table_export_u32(const void *workspace, size_t buckets, size_t pool_nodes, uint32_t *out_keys,
                                uint32_t *out_vals, uint32_t *out_next, uint32_t *out_pool_used,
                                dbhip_stream_t stream);

/* ---- multi-GPU radix-partitioned join: device pieces (no reference counterpart) ---------
 * Partition a local column shard into `parts` (1..1024) destination buckets by a mixed hash of
 * the key (independent of the hash the local join partitions by): out_keys / out_row_ids are bucket-major (bucket d occupies
 * [sum(out_counts[0..d)), +out_counts[d])), out_row_ids[i] = first_row_id + local index of the key
 * (global row ids must fit 32 bits), out_counts is a DEVICE array of `parts` uint64.  The exchange
 * between GPUs is the host's job (RCCL all-to-all); the local join on the received pairs is
 * dbhip_join_build_u32 / dbhip_join_probe_u32, and dbhip_gather_u32 (out[i] = table[idx[i]]) turns
 * its build-row indices into global row ids.                                                      */
size_t dbhip_pjoin_partition_workspace_bytes(size_t n, uint32_t parts);
int dbhip_pjoin_partition_u32(const uint32_t *keys, size_t n, uint64_t first_row_id, uint32_t parts,
                              uint32_t *out_keys, uint32_t *out_row_ids, uint64_t *out_counts,
                              void *workspace, size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_gather_u32(const uint32_t *table, const uint32_t *idx, size_t n, uint32_t *out,
                     dbhip_stream_t stream);
/* validator of the exchange's routing: result[0] (DEVICE uint64) = number of keys that dbhip_pjoin_partition_u32
 * would NOT put into bucket `rank` of `parts` (0 on a rank that received only its own keys)            */
int dbhip_check_pjoin_route_u32(const uint32_t *keys, size_t n, uint32_t parts, uint32_t rank, uint64_t *result,
                                dbhip_stream_t stream);

/* ---- the two small dwarfs that complete the taxonomy ---------------------------
 * dbhip_reduce_sum_i32: *out = sum of src[0..n) with int32 wrap-around (reduce/reduce.cpp:27-88, the
 *   oneAPI plus<> reduction into an int; the reference's oracle is std::accumulate(..., 0), :10-22).
 * dbhip_nested_join_u32: the dense n_a x n_b cell matrix of join/nested_join.cpp:52-66, row-major
 *   over (a row, b row): a matching cell holds (key, a_val, b_val), every other cell holds the
 *   reference's "empty" markers (key 0, values 0xFFFFFFFF, nested_join.cpp:30-32).  The kernel writes
 *   all cells, so the three outputs need no initialisation.  n_a <= 1,048,560.                       */
int dbhip_reduce_sum_i32(const int32_t *src, size_t n, int32_t *out, dbhip_stream_t stream);
int dbhip_nested_join_u32(const uint32_t *a_keys, const uint32_t *a_vals, const uint32_t *b_keys,
                          const uint32_t *b_vals, size_t n_a, size_t n_b, uint32_t *out_key,
                          uint32_t *out_val1, uint32_t *out_val2, dbhip_stream_t stream);

/* ---- exclusive prefix sum -------------------------------------------------------
 * dst[0] = init, dst[i] = init + src[0] + ... + src[i-1], uint32 wrap-around: the semantics of the reference's
 * prefix_sum_scalar / prefix_local_test (tests/scan_tests.cpp:14-21, :46-51, scan/scan.cl:44-66) and of
 * oneDPL exclusive_scan behind DPLWrapper::exclusive_scan (common/dpcpp/dpl_wrapper/dpl_wrapper.hpp:18-25,
 * used by common/dpcpp/omnisci_hashtable.hpp:252-254).  dst may alias src.
 * 16-byte aligned src and dst: ONE launch, every element read once and written once (128 KiB chunks kept in registers
 * across a ticketed chunk-to-chunk hand-off; bounded wait: DBHIP_DEV_SPIN_TIMEOUT); other alignments: three launches. */
size_t dbhip_exclusive_scan_u32_workspace_bytes(size_t n);
int dbhip_exclusive_scan_u32(const uint32_t *src, size_t n, uint32_t init, uint32_t *dst, void *workspace,
                             size_t workspace_bytes, dbhip_stream_t stream);

/* ---- device-side validators: Result::valid of the `...Hip` dwarfs above the host-check size -------------
 * Each is an algorithm independent of the kernel it checks; `result` is a DEVICE array of uint64 words,
 * zeroed by the call.  Reference checks replaced: scan/scan.cpp:157-164 (out == std::copy_if),
 * sort/radix.cpp:46-52 (== std::sort), groupby/groupby.cpp:95-103 (== expected_GroupBy),
 * join/join_omnisci.cpp:31-45 (are_equal: size per probe row + membership of every id),
 * join/join.cpp:133-137 (== seq_join).
 *   fingerprint_lt_i32  result[0] = order-sensitive fingerprint of the subsequence x < filter_value,
 *                       result[1] = its length.  copy_if is right iff the pair computed over src equals the
 *                       pair computed over out[0..out_size) (every element of out passes the same filter).
 *   sorted_u32          result[0] = number of i with key[i] > key[i+1] (signed_order != 0: as int32),
 *                       result[1], result[2] = commutative multiset fingerprint (compare with the input's).
 *   weighted_sum_u32    result[0], result[1] = sum vals[i] * w(keys[i]) mod 2^32 for two weight functions with odd
 *                       weights; keys == NULL means keys[i] = i (the dense group-by output).  Compared between a group-by
 *                       output and its rows: a right output always agrees, an error confined to one group never does
 *                       (an odd weight is a bijection mod 2^32), and an error spread over several groups is caught unless
 *                       both weighted differences vanish.  A value d moved from one group to another shows as
 *                       d * (w(g1) - w(g2)) with an even second factor: d = 2^31 is never seen, and a random multiple d of
 *                       2^t goes unseen in 0.8 % (t = 24), 12.5 % (t = 28), 50 % (t = 30) of moves among 1000 groups; a
 *                       random d (t = 0) in none of 200 000 ("What the device-side validators cannot see").
 *   permutation_u32     result[0] = number of entries >= n or seen before (0 iff ids is a permutation of 0..n-1).
 *   join_u32            sorted_build_keys = the build column sorted ascending.  result[0] = number of probe rows
 *                       whose count differs from the key's multiplicity in the build column, whose id range
 *                       leaves the id buffer, or whose first / last / one id at mix64(7, row) % count does not carry the
 *                       key (n_probe < 2^32, so the count fills the LOW 32 bits); in the HIGH 32 bits, mod 2^32, the
 *                       number of j < n_build - 1 where ids[j] and ids[j+1] carry different keys (an id that names no row
 *                       differs from all) less the number of j where sorted_build_keys[j] != [j+1].  The halves cannot
 *                       cancel: result[0] == 0 only if no row is bad, whatever ids holds.  The three ids alone leave 36 %
 *                       of the probed id positions of the benchmark's join unread; with ids a permutation of the build
 *                       rows (permutation_u32 on ids, which JoinOmnisciHip and JoinPairsHip run beside this check; ProbeHip
 *                       and the partitioned join do not) the high half is 0 iff every key is one run of ids, which makes
 *                       every id of every probed range right.  It means nothing after a build that dropped rows
 *                       (0xFFFFFFFF build keys, DBHIP_DEV_KEY_RANGE).  out_pos of a row without a match is not looked at.
 *                       n_probe == 0: nothing is launched, both words are 0 whatever n_build is.
 *                       result[1] = sum of all counts.  build_keys != NULL: ids are build row indices and the key
 *                       of id is build_keys[id]; build_keys == NULL: ids are global row ids of a generated column
 *                       and the key of id is gen_lo + mix64(gen_seed, id) % (gen_hi - gen_lo + 1).
 *   ujoin_u32           build keys unique and sorted ascending (what dbhip_gen_unique_sorted_u32 produces):
 *                       result[0] = probe rows whose (key, build payload, probe payload) triple or sentinels are
 *                       wrong, result[1] = number of hits.
 *   gen_uniform_u32     result[0] = number of i with values[i] != lo + mix64(seed, index_i) % (hi - lo + 1),
 *                       index_i = indices ? indices[i] : first_index + i.
 *   distinct_u32        result[0] = number of i with s[i] >= s[i+1] over a sorted copy s of keys (dbhip_radix_sort_u32 in
 *                       the workspace): 0 iff the keys are distinct.  A group-by output (dbhip_groupby_hash_u32) is taken
 *                       as right when its keys are distinct, weighted_sum over (out_keys, out_sums) equals weighted_sum
 *                       over (keys, vals), the same holds for (out_keys, out_counts) against a column of ones, and the
 *                       counts sum to n: every right output passes, and a wrong one passes only through the gap of
 *                       weighted_sum_u32 named above.
 *   sorted_pairs_u32    (n < 2^32) result[0] = number of i < n-1 with (keys_out[i], ids_out[i]) >= (keys_out[i+1],
 *                       ids_out[i+1]), compared lexicographically, keys as int32 when signed_order != 0; result[1] =
 *                       number of i with ids_out[i] >= n or keys_in[ids_out[i]] != keys_out[i].  Both zero iff ids_out is
 *                       the stable sort permutation of keys_in and keys_out the sorted column: strictly increasing
 *                       pairs are n distinct pairs, and as every id names a row that carries the key beside it, equal
 *                       ids would make equal pairs — so the ids are n distinct values below n, a permutation; keys_out
 *                       is keys_in under it, ascending, and ties stand in row order.
 *   join_pairs_u32      the pair table of dbhip_join_pairs_u32 against the answer it was made from.  result[0] = number of
 *                       bad pairs among out_*[0..n_pairs): a row id out of range, build_keys[b] != probe_keys[p], or
 *                       b == 0xFFFFFFFF when left_outer is 0 (a sentinel on a row that has matches shows in the
 *                       fingerprints); result[1] = the number of pairs expected; result[2] = fingerprint of the pairs
 *                       given, result[3] = fingerprint expected: order-independent 64-bit sums of a mix of (b, p), the
 *                       expected one from a one-thread-per-probe-row walk over (pos, cnt, ids): another algorithm than
 *                       the expansion, slow, a checker only.  Valid iff result[0] == 0 && result[1] == n_pairs &&
 *                       result[2] == result[3].  Row ids are taken as ROW INDICES into the key columns given, which is
 *                       what both joins produce when no row_ids column is passed to them.                       */
size_t dbhip_check_fingerprint_workspace_bytes(size_t n);
int dbhip_check_fingerprint_lt_i32(const int32_t *src, size_t n, int32_t filter_value, uint64_t *result,
                                   void *workspace, size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_check_sorted_u32(const uint32_t *keys, size_t n, int signed_order, uint64_t *result,
                           dbhip_stream_t stream);
int dbhip_check_weighted_sum_u32(const uint32_t *keys, const uint32_t *vals, size_t n, uint64_t *result,
                                 dbhip_stream_t stream);
size_t dbhip_check_permutation_workspace_bytes(size_t n);
int dbhip_check_permutation_u32(const uint32_t *ids, size_t n, uint64_t *result, void *workspace,
                                size_t workspace_bytes, dbhip_stream_t stream);
int dbhip_check_join_u32(const uint32_t *sorted_build_keys, size_t n_build, const uint32_t *probe_keys,
                         size_t n_probe, const uint32_t *out_pos, const uint32_t *out_count, const uint32_t *ids,
                         const uint32_t *build_keys, uint64_t gen_seed, uint32_t gen_lo, uint32_t gen_hi,
                         uint64_t *result, dbhip_stream_t stream);
int dbhip_check_ujoin_u32(const uint32_t *sorted_build_keys, const uint32_t *build_vals, size_t n_build,
                          const uint32_t *probe_keys, const uint32_t *probe_vals, size_t n_probe,
                          const uint32_t *out_key, const uint32_t *out_build_val, const uint32_t *out_probe_val,
                          uint64_t *result, dbhip_stream_t stream);
size_t dbhip_check_distinct_workspace_bytes(size_t n);
int dbhip_check_distinct_u32(const uint32_t *keys, size_t n, uint64_t *result, void *workspace, size_t workspace_bytes,
                             dbhip_stream_t stream);
int dbhip_check_sorted_pairs_u32(const uint32_t *keys_in, const uint32_t *keys_out, const uint32_t *ids_out, size_t n,
                                 int signed_order, uint64_t *result, dbhip_stream_t stream);
int dbhip_check_join_pairs_u32(const uint32_t *build_keys, size_t n_build, const uint32_t *probe_keys, size_t n_probe,
                               const uint32_t *ids, const uint32_t *probe_row_ids, const uint32_t *pos, const uint32_t *cnt,
                               int left_outer, const uint32_t *out_build_rows, const uint32_t *out_probe_rows,
                               uint64_t n_pairs, uint64_t *result /* 4 device words */, dbhip_stream_t stream);
int dbhip_check_gen_uniform_u32(const uint32_t *values, const uint32_t *indices, size_t n, uint64_t seed,
                                uint64_t first_index, uint32_t lo, uint32_t hi, uint64_t *result,
                                dbhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBHIP_H */
