"""development aid: `python tools/ab.py <dwarf> [log2 size]` — HIP-event timings of one dwarf through the C ABI, one
line per run, for A/B comparisons of library builds (DBHIP_LIB=<path to a libdbhip_*.so built by tools/build_variant.sh>
selects the build; the line starts with its tag).  Every mode also checks its result against torch, so a faster
variant that computes something else shows up as WRONG.  This is how the per-kernel figures in DESIGN.md were taken;
the contract numbers come from bench.py.

  scan            two-launch vs dense copy_if at 2^28 rows over a selectivity sweep (median of 9)
  sort [lg]       2^lg-key sort, 8- and 4-bit digits (drop-max-mean of 9, refresh copy subtracted); default lg 24
  sort-pairs [lg] key-value sort and argsort (dbhip_radix_sort_pairs_*), 8- and 4-bit digits, at 2^20 / 2^24 / 2^26 rows (or
                  2^lg alone), full-range keys and keys in [1, 10000]; beside them, in the same run, the keys-only sort and
                  torch.sort(stable=True) (which returns 8-byte indices) (median of 9, refresh copy subtracted); every
                  column of every mode checked against torch's stable sort
  topk [lg]       ORDER BY key LIMIT k at 2^lg rows (default 24): ops.topk (sorted), the argsort route (clone + radix_argsort_ +
                  slice; the copy belongs to it, the argsort destroys its input) and torch.topk on the same int32 column, in
                  one process, alternating, REPS (default 5) repetitions of a median of 5 each; k = 1, 64, 1024, 2^16, 2^20, n/2;
                  uniform full-range keys, keys in [1, 10000], all keys equal, sorted ascending (TOPK_INPUTS=uniform: that one alone); prints every repetition, and
                  per row the range of each leg; ops.topk's answer checked by dbhip_check_topk_u32 and against the argsort
  launch-topk [lg] five sorted top-k calls at k = 1024 and five at k = 2^20 on 2^lg uniform rows (default 24), nothing else
                  (`rocprofv3 --kernel-trace --stats`)
  groupby-sorted [lg] dbhip_reduce_by_key_u32 at 2^lg rows (default 24).  Part 1, sorted input (R = 1, 64, 2^16, 2^20, n runs, and half the
                  rows in one run with the rest distinct): ReduceByKey.launch with all five aggregates against
                  torch.unique_consecutive(return_inverse, return_counts) + scatter_add_ on int64 + scatter_reduce_ amin / amax, in
                  one process, alternating, REPS (default 5) repetitions of a median of 5; beside it the time of (12n + 24R)
                  bytes at 8 TB/s.  Part 2, the same keys shuffled: copy + pairs sort + reduce (ops.groupby_sorted's launches)
                  against GroupByHash.launch (wrapping SUM and COUNT, unordered) and torch.unique(return_inverse,
                  return_counts) + the same scatters.  Every answer checked by dbhip_check_reduce_by_key_u32
  launch-groupby-sorted [lg] five reduce calls each on sorted keys with 64, 2^20 and n runs at 2^lg rows, nothing else
                  (`rocprofv3 --kernel-trace --stats`)
  window [lg]     dbhip_scan_by_key_u32 at 2^lg rows (default 24).  Part 1, grouped input (the shapes of groupby-sorted):
                  ScanByKey.launch with all five columns against the torch composition of the same columns (cumsum for the run
                  numbers and the sums, cummax for the row numbers, cummin / cummax over the composite int64 words
                  ((R-1-run) << 32 | x) and (run << 32 | x) for the extremes), in one process, alternating, REPS (default 5)
                  repetitions of a median of 5; beside it the time of 16n + 24n bytes at 8 TB/s.  Part 2, the same keys
                  shuffled: copy + argsort + gather + scan (ops.window_sorted's launches).  Every answer checked by
                  dbhip_check_scan_by_key_u32 and, in part 1, against the torch columns
  launch-window [lg] five scan-by-key calls on every grouped shape at 2^lg rows, nothing else (`rocprofv3 --kernel-trace`)
  join-pairs [lg] the join's pair table (dbhip_join_pairs_u32: scan + expansion, one call, capacity given) on the radix join's
                  answer at 2^20 / 2^24 / 2^26 rows a side (or 2^lg alone) with keys in [1, n], and on 2^13 x 2^13 rows of one
                  key (2^26 pairs); beside it the count-only call and, in the same process on the same (ids, pos, cnt), the
                  torch composition repeat_interleave + cumsum + gather (median of 9); both columns of both legs compared
                  with each other and the pair table checked by dbhip_check_join_pairs_u32
  sorted-search [lg] dbhip_sorted_search_u32 of 2^lg probe rows (default 24) in sorted columns of 2^14, 2^20, 2^24 and 2^26 entries
                  (SS_M=<lg m>: that one alone), uniform and with 2^13 distinct values; probe values uniform, the same sorted, all
                  one value; hi == lo and a band of about 16 matches per row; SortedSearch.search against
                  torch.searchsorted(side="left") on lo, side="right") on hi and the subtraction, in one process, alternating,
                  REPS (default 5) repetitions of a median of 5; beside it the index build, the ladder's levels, the gather model
                  (rows x block loads that leave the CU / 53 G/s) and whether this code's slowest repetition beat torch's fastest
                  (the floor); every answer checked by dbhip_check_sorted_search_u32 and against torch.  lg 10: the
                  single-launch cost against a large column
  range-join [lg] the band join at 2^lg rows a side (default 24), keys in [1, n], hi = lo + 2: copy + argsort + index + search +
                  pairs (ops.range_join's launches, capacity given) against torch.sort(stable) + two searchsorted + join-pairs'
                  torch expansion, same protocol; both pair columns compared with torch's
  selection [lg]  the selection vectors (ops.SelectRows: dbench_select_range_u32 of host/select_rows.hpp) against torch on the same
                  int32 columns, same protocol and floor as sorted-search.  Dense: 2^22, 2^24, 2^26 rows (or 2^lg alone) of uniform
                  values at selectivities 0, 0.01, 1, 10, 50, 100 % against torch.nonzero((x >= lo) & (x <= hi)), beside the
                  time of 4n + n/4 + 4m bytes at 8 TB/s; lists of 2^20 and 2^24 rows out of 2^26, sorted and shuffled, against
                  rows[(col[rows] >= lo) & (col[rows] <= hi)]; the three-predicate chain at 2^26 rows against the torch
                  conjunction; the semi join 2^24 x 2^24 against torch.isin + nonzero.  Both legs run until the row ids and
                  their number are usable on the host; every result compared with torch's (SEL_PARTS picks parts)
  merge [lg]      the merge-path entry points of host/merge_sorted.hpp (ops.MergeSorted, ops.RowSets, select + select + union),
                  same protocol and floor as sorted-search (one process, profiler off, legs alternating, REPS (default 5)
                  repetitions of a median of 5, this code's slowest repetition against the comparison's fastest).  Merge with
                  row ids at 2^22, 2^24, 2^26 output rows (or 2^lg alone): na = nb uniform, all keys equal, A below B, nb = 2^10
                  against a large A; the comparison is this library's RadixSortPairs argsort of the preloaded concatenation (the
                  restoring copy runs in front of the timed span); beside it the keys-only and carried-value merges and the
                  time of their bytes at 8 TB/s.  Set operations on two random strictly ascending lists of 2^20, 2^24, 2^26
                  rows each against torch.unique(torch.cat), a[torch.isin(a, b, assume_unique=True)] and its negation, both legs
                  run until the rows and their number are usable on the host.  select + select + union at 2^26 rows against
                  torch.nonzero(ka | kb) at shares (1 %, 1 %) and (50 %, 50 %).  Every result compared with the comparison
                  leg's (MERGE_PARTS=merge,sets,any picks parts)
  take [lg]       late materialisation through a row-id list (ops.TakeRows, ops.AggregateRows: host/take_rows.hpp) out of a
                  2^26-row column (or 2^lg), same protocol and floor as sorted-search.  Lists: ascending as a selection leaves them
                  at 1, 10, 50 and 100 % kept, random subsets of 2^20 and 2^24 rows ascending and shuffled, and a permutation of
                  all rows.  take of 1, 2 and 4 columns against torch.index_select per column; the aggregate against
                  index_select + sum (int64), min, max, and against this library's own take followed by the same reductions;
                  the aggregate over all rows against the torch reductions; select -> refine -> aggregate against the boolean
                  mask form.  The aggregate legs end with the four numbers on the host, the take legs with the columns on the
                  device.  Beside each row the gather rate (entries x columns / s, the chip's random-gather rate is 53-57 G/s)
                  and the time of 4m + 4km bytes plus the gathered 128-byte lines at 8 TB/s.  Every result compared with
                  torch's (TAKE_PARTS=take,aggregate,dense,chain picks parts)
  dict [lg]       dictionary encoding (ops.Dictionary, ops.groupby_columns: host/dict_encode.hpp) at 2^20, 2^24 and 2^26 rows (or
                  2^lg alone), same protocol and floor as sorted-search, over columns of 1, 64, 4096 (the encode kernel's LDS body),
                  2^20 and all-distinct values (its global body) spread over the 32 bits.  factorize (build + encode, the
                  capacity the number of distinct values) against torch.unique(sorted=True, return_inverse=True), and beside it
                  the same with capacity = n, whose build sorts n padded entries whatever the column holds; encode alone against
                  torch.searchsorted on the sorted uniques, with the time of its 8n bytes at 8 TB/s; GROUP BY two columns SUM,
                  COUNT (ops.groupby_columns, up to 2^DICT_GROUPBY_LG rows, default 24) against torch.unique(dim=0,
                  return_inverse=True) + scatter_add.  Every result compared with torch's (DICT_PARTS=factorize,encode,groupby
                  and DICT_CARDS=1,64,4096,1048576,0 pick parts and cardinalities; 0 = all distinct)
  launch-join-pairs [lg]  five expansions at 2^lg rows a side (default 24) and five of the one-key shape, nothing else
                  (`rocprofv3 --kernel-trace --stats`)
  launch-sort-pairs [lg]  five 8-bit argsorts of 2^lg full-range keys (default 24) and nothing else (`rocprofv3 --kernel-trace`)
  sort-only       three 2^24 sorts and nothing else (counter collection; SORT_BITS=4|8, SORT_SHAPE=<index into sort-shapes' list>)
  groupby         2^26 rows at 2^16 / 2^15 / 2^10 / 64 groups (drop-max-mean of 9)
  groupby-shapes  more than 32768 groups over row counts, group counts and value ranges (median of 5): run it with
                  DBHIP_GB_PACKED=0 beside the default to see what the kernel's choice between its two large-table modes
                  buys and that it costs nothing where the packed table would be slow
  groupby-hash    dbhip_groupby_hash_u32 at 2^24 and 2^26 rows: 1 .. 2^20 and all-distinct sparse keys, half the rows on one
                  key, and groupby_sum's BASELINE input (2^16 dense groups), beside groupby_sum on the dense draw and the torch
                  composition unique(return_inverse, return_counts) + scatter_add (median of 7 / 7 / 3)
  groupby-skew    2^26 rows whose keys crowd into one or a few groups, at 64 .. 2^16 groups (median of 5)
  sort-shapes [lg] 2^lg keys of eight distributions (few distinct values, sorted, reversed, skewed ...; median of 5)
  join [lg]       build / probe / radix join of 2^lg x 2^lg (drop-max-mean of 7); default lg 26
  radix [lg]      the radix join alone at 2^lg x 2^lg (default 30: the P = 1 point of the partitioned join)
  radix-sizes     the radix join at 1, 1.25, 1.5, 1.75 x 2^25 .. 2^29 rows (geometry steps)
  join-skew [lg]  the same over key shapes (hot keys, strided keys, sorted, few distinct keys; median of 3)
  size-sweep      every dwarf at sizes next to and between powers of two, 2^13 .. 2^26 (geometry cliffs)
  partition       rank-level partition (dbhip_pjoin_partition_u32) of 2^27 rows into P buckets
  reduce          2^28-row reduce (median of 15; DBHIP_RED_WGS)
  cuckoo [lg]     cuckoo table (hash_kind 2) at 2^lg unique keys in 4 * 2^lg slots (default lg 24): reset, insert, lookups of present
                  and of absent keys (median of 9), each checked against torch
  slab [lg]       slab table at 2^lg rows (default lg 24), the dwarfs' n / 20 buckets and n / 20 + 16384 pool nodes: reset, insert of unique keys,
                  of SlabHashBuild's keys in [1, 10000] and of 2^(lg-8) rows of one key, lookups of present and absent keys
                  (median of 9), each with the tail hint on and off (DBHIP_SLAB_HINT) and the first CAS at the lowest or at a
                  spread empty slot (DBHIP_SLAB_SPREAD 0 / default / 1); every build checked
  xscan [lg]      exclusive scan of 2^lg uint32, aligned (one launch) and offset by one element (three launches)
  graph [lg]      direct launches vs hipGraph replay of sort and join at 2^14..2^20 rows, or 2^lg alone (host wall clock)
  bitpack [lg]    bit-packed columns (ops.BitPack, ops.unpack, ops.SelectRows on a PackedColumn: host/bitpack.hpp) at 2^lg rows
                  (default 26; one process per size: 20, 24, 26), same protocol as sorted-search (legs alternating, REPS
                  repetitions of a median of 5, HIP events, every leg's result checked), widths 4, 8, 12, 16, 24, 32
                  (BITPACK_WIDTHS).  select: the dense range filter on the packed codes against dbench_select_range_u32 on the
                  decoded 32-bit column at 0 / 1 / 50 / 100 % kept, with the share of n width / 8 + n / 4 + 4 m bytes at
                  8 TB/s; the floor (this code's slowest repetition against the plain select's fastest) applies at widths up
                  to 16, wider ones are reported.  Report only: pack and the dense unpack against their bytes and against
                  torch.clone of the 32-bit column; unpack through lists of 1 % and 50 % of the rows, ascending and shuffled,
                  against dbench_take_u32 on the decoded column.  BITPACK_PARTS=select,pack,unpack,take picks parts
  bloom [lg]      Bloom filter (ops.BloomFilter, SelectRows.launch_in, ops.semi_join with bloom_bits: host/bloom_filter.hpp), same
                  protocol as bitpack (legs alternating, REPS repetitions of a median of 5, HIP events, every leg's result
                  checked); report only, nothing is gated.  BLOOM_PARTS=build,probe,semi picks parts.
                  build: 2^24 rows (BLOOM_BUILD_LG), distinct keys and keys in [1, 10000] at 16 bits per key, the distinct keys
                  also into filters of 2^10, 2^16, 2^20 and 2^26 words; each against the same build without test-before-set
                  (bloom_filter.cpp compiled with -DDBENCH_BLOOM_ALWAYS_SET into _lib/ab/, built on first use).
                  probe: 2^lg rows (default 26) at 0 / 1 / 50 / 100 % of rows holding a key of the filter, filters of those
                  four sizes, against select_range on the same column (the stream the mark kernel shares) and
                  HashJoin.probe of the same rows (the gather it stands in front of).
                  semi: ops.semi_join with and without bloom_bits=16, build sides of 2^16, 2^20, 2^24 distinct keys, a probe
                  side of 2^lg, 0 / 1 / 10 / 50 / 100 % of probe rows with a partner
  hll             HyperLogLog (ops.HyperLogLog: host/hll_sketch.hpp), same protocol as bloom (legs alternating, REPS repetitions of a
                  median of 5, HIP events, registers and histogram checked against the second build); report only, nothing
                  is gated.  2^20, 2^24 and 2^26 rows (HLL_LGS) at p = 12 and 14 (HLL_PS); all rows distinct, keys in
                  [1, 10000], one hot key (99 % of the rows), sorted keys, two columns, and lists of 1 % and 50 % of the rows
                  (HLL_SHAPES).  Legs: the sketch, the same build without test-before-set (hll_sketch.cpp compiled with
                  -DDBENCH_HLL_ALWAYS_MAX into _lib/ab/, built on first use), the dictionary build behind ops.factorize
                  (its cardinality; capacity = the true count), torch.unique(col).numel(), and select_range on the same
                  column as the stream yardstick.  The floor, HELD or MISSED: the sketch's slowest repetition against the
                  faster exact route's fastest.  The estimate's relative error is printed for every shape
  quantile        exact order statistics (ops.Quantiles: host/quantile_select.hpp), same protocol as hll (legs alternating, REPS
                  repetitions of a median of 5, HIP events, every leg's values checked against the select's).  2^20, 2^24 and
                  2^26 rows (QUANTILE_LGS); uniform full-range keys, keys in [1, 10000], all keys equal, sorted keys, and
                  lists of 1 % and 50 % of the rows of the uniform column (QUANTILE_SHAPES); one rank (the median) and nine
                  (the deciles), int32 order.  Legs: the select, the routes the library had before it — copy +
                  RadixSort + index, torch.kthvalue per rank, and for one rank TopK(k = r + 1, sorted=False) with the max of
                  its keys — behind TakeRows where there is a list, and for one rank the same rank sixteen times (the
                  sixteen-slot kernel with one live slot).  The floor, HELD or MISSED: the select's slowest repetition
                  against the fastest other route's fastest
  launch-join [lg] / launch-sort [lg] / launch-all
                  a few untimed calls and nothing else: the program to put behind `rocprofv3 --kernel-trace --stats` or
                  `--pmc` (tools/pmc_kernel_counters.sh); tools/prof_show.py prints the tables
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dwarf_bench_amd import ops  # noqa: E402

TAG = os.environ.get("DBHIP_LIB", "default").split("libdbhip_")[-1]


def times(fn, k, warm=2):
    """device time of k calls, us each (events on torch's current stream = the launch stream), sorted"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return sorted(out)


def dropmax(ts):
    return sum(ts[:-1]) / (len(ts) - 1)


def median(ts):
    return ts[len(ts) // 2]


def u64(t):
    return t.to(torch.int64) & 0xFFFFFFFF


def bits32(t):
    """int64 values in [0, 2^32) as the int32 tensor holding the same bits (how the C ABI takes uint32 keys)"""
    return ((t + 2**31) % 2**32 - 2**31).to(torch.int32)


def scan(_):
    n = 1 << 28
    src = ops.gen_uniform_u32(n, 42, 1, 10000)
    plan = ops.CopyIfLt(n)
    for filt in (5, 101, 251, 501, 751, 1001, 1501, 2001, 2501, 5001, 7501, 10001):
        t0 = median(times(lambda: plan.launch(src, filt, dense=False), 9))
        m = plan.result().numel()
        t1 = median(times(lambda: plan.launch(src, filt, dense=True), 9))
        m1 = plan.result().numel()
        byts = 4 * n + 4 * m
        print(f"{TAG:16s} s={m / n:6.4f}: two-launch {t0:7.1f} us ({byts / t0 / 8e6 * 100:4.1f} %)   dense {t1:7.1f} us "
              f"({byts / t1 / 8e6 * 100:4.1f} %)  {'same count' if m == m1 == int((src < filt).sum()) else 'COUNT DIFFERS'}", flush=True)


def sort(lg):
    n = 1 << (lg or 24)
    keys0 = ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    keys = keys0.clone()
    ref = torch.sort(u64(keys0)).values
    res = []
    for bits in (8, 4):
        plan = ops.RadixSort(n, bits)

        def run():
            keys.copy_(keys0)
            plan.launch(keys)

        t = dropmax(times(run, 9)) - dropmax(times(lambda: keys.copy_(keys0), 9))
        run()
        ok = bool(torch.equal(u64(keys), ref)) and ops.workspace_status(plan.ws) == 0
        res.append(f"{bits}-bit {t:7.1f} us {'ok' if ok else 'WRONG'}")
    print(f"{TAG:24s} 2^{lg or 24}: " + "   ".join(res), flush=True)


def sort_pairs(lg):
    for n in ([1 << lg] if lg else [1 << 20, 1 << 24, 1 << 26]):
        for lo, hi, name in ((0, 2**32 - 1, "full-range"), (1, 10000, "[1,10000]")):
            keys0 = ops.gen_uniform_u32(n, 42, lo, hi)
            vals0 = ops.gen_uniform_u32(n, 43, 0, 2**32 - 1)
            keys, vals = keys0.clone(), vals0.clone()
            ref = torch.sort(u64(keys0), stable=True)
            copy_k = median(times(lambda: keys.copy_(keys0), 9))
            copy_kv = median(times(lambda: (keys.copy_(keys0), vals.copy_(vals0)), 9))
            t_torch = median(times(lambda: torch.sort(u64(keys0), stable=True), 5))
            res = []
            for bits in (8, 4):
                plan, ko = ops.RadixSortPairs(n, bits), ops.RadixSort(n, bits)

                def pairs():
                    keys.copy_(keys0)
                    vals.copy_(vals0)
                    plan.launch(keys, vals)

                def argsort():
                    keys.copy_(keys0)
                    plan.launch(keys)

                def keys_only():
                    keys.copy_(keys0)
                    ko.launch(keys)

                t_p = median(times(pairs, 9)) - copy_kv
                pairs()
                ok_p = torch.equal(u64(keys), ref.values) and torch.equal(vals, vals0[ref.indices]) and ops.workspace_status(plan.ws) == 0
                t_a = median(times(argsort, 9)) - copy_k
                argsort()
                ok_a = (torch.equal(u64(keys), ref.values) and torch.equal(u64(plan.perm[:n]), ref.indices) and ops.workspace_status(plan.ws) == 0
                        and ops.check_sorted_pairs(keys0, keys, plan.perm[:n]) == (0, 0))
                t_k = median(times(keys_only, 9)) - copy_k
                keys_only()
                ok_k = torch.equal(u64(keys), ref.values) and ops.workspace_status(ko.ws) == 0
                res.append(f"{bits}-bit pairs {t_p:8.1f} us {'ok' if ok_p else 'WRONG'}  argsort {t_a:8.1f} us {'ok' if ok_a else 'WRONG'}  "
                           f"keys-only {t_k:8.1f} us {'ok' if ok_k else 'WRONG'}  (pairs / keys-only {t_p / t_k:4.2f}, argsort / keys-only {t_a / t_k:4.2f})")
            for r in res:
                print(f"{TAG:12s} n={n:9d} {name:10s} {r}   torch.sort(stable) {t_torch:8.1f} us", flush=True)
            del keys0, vals0, keys, vals, ref


def _topk_columns(n):
    yield "uniform", ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    yield "[1,10000]", ops.gen_uniform_u32(n, 42, 1, 10000)
    yield "all equal", torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    yield "ascending", torch.sort(ops.gen_uniform_u32(n, 42, 0, 2**31 - 1)).values


def topk(lg):
    n = 1 << (lg or 24)
    reps = int(os.environ.get("REPS", "5"))
    only = os.environ.get("TOPK_INPUTS")  # e.g. "uniform": that column alone
    for name, keys in _topk_columns(n):
        if only and name not in only.split(","):
            continue
        srt = ops.RadixSortPairs(n, 8)
        scratch = torch.empty_like(keys)
        for k in (1, 64, 1024, 1 << 16, 1 << 20, n // 2):
            plan = ops.TopK(n, k)

            def select():
                plan.launch(keys, signed=True)

            def argsort():
                scratch.copy_(keys)
                srt.launch(scratch, None, signed=True)  # the answer: scratch[:k], srt.perm[:k]

            def vendor():
                torch.topk(keys, k, largest=False, sorted=True)

            legs = {"topk": [], "argsort": [], "torch.topk": []}
            for _ in range(reps):  # alternating
                legs["topk"].append(median(times(select, 5)))
                legs["argsort"].append(median(times(argsort, 5)))
                legs["torch.topk"].append(median(times(vendor, 5)))
            select()
            argsort()
            got_keys, got_rows = plan.result()
            ok = (ops.check_topk(keys, got_keys, got_rows, signed=True) == (0, k - 1) and torch.equal(got_rows, srt.perm[:k])
                  and torch.equal(got_keys, scratch[:k]) and ops.workspace_status(srt.ws) == 0)
            cols = "  ".join(f"{leg} {min(ts):8.1f} .. {max(ts):8.1f} us" for leg, ts in legs.items())
            verdict = "select wins beyond both ranges" if max(legs["topk"]) < min(legs["argsort"]) else "SELECT DOES NOT WIN"
            print(f"{TAG:10s} n=2^{lg or 24} {name:10s} k={k:9d}  {cols}  {'ok' if ok else 'WRONG'}  {verdict}   "
                  + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)
        del keys, srt, scratch


def launch_topk(lg):
    n = 1 << (lg or 24)
    keys = ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    for k in (1024, 1 << 20):
        plan = ops.TopK(n, k)
        for _ in range(5):
            plan.launch(keys, signed=True)
        plan.result()
    print("ok")


def _sorted_key_shapes(n):
    """(name, sorted keys, R)"""
    rows = torch.arange(n, dtype=torch.int64, device="cuda")
    for r in (1, 64, 1 << 16, 1 << 20, n):
        if r <= n:
            yield f"R={r}", (rows * r // n).to(torch.int32), r
    half = torch.where(rows < n // 2, torch.zeros_like(rows), rows - n // 2 + 1).to(torch.int32)
    yield "half+distinct", half, n - n // 2 + 1


def _torch_aggregates(inverse, groups, vals64, vals):
    sums = torch.zeros(groups, dtype=torch.int64, device="cuda").scatter_add_(0, inverse, vals64)
    mins = torch.full((groups,), 2**31 - 1, dtype=torch.int32, device="cuda").scatter_reduce_(0, inverse, vals, "amin")
    maxs = torch.full((groups,), -2**31, dtype=torch.int32, device="cuda").scatter_reduce_(0, inverse, vals, "amax")
    return sums, mins, maxs


def groupby_sorted(lg):
    n = 1 << (lg or 24)
    reps = int(os.environ.get("REPS", "5"))
    vals = ops.gen_uniform_u32(n, 43, 1, 10000)
    vals64 = vals.to(torch.int64)

    def report(part, name, R, legs, ok, model=None):
        cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
        extra = f"  model {model:7.1f} us" if model else ""
        print(f"{TAG:10s} {part} n=2^{lg or 24} {name:14s} runs={R:9d}  {cols}{extra}  {'ok' if ok else 'WRONG'}   "
              + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)

    for name, keys, R in _sorted_key_shapes(n):
        plan = ops.ReduceByKey(n, R)

        def reduce():
            plan.launch(keys, vals)

        def vendor():
            u, inv, cnt = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
            return (u, cnt) + _torch_aggregates(inv, u.numel(), vals64, vals)

        legs = {"reduce_by_key": [], "torch": []}
        for _ in range(reps):  # alternating
            legs["reduce_by_key"].append(median(times(reduce, 5)))
            legs["torch"].append(median(times(vendor, 5)))
        reduce()
        got = plan.result()
        words = ops.check_reduce_by_key(keys, vals, *got)
        u, cnt, sums, mins, maxs = vendor()
        ok = (words[0] == 0 and words[1] == 0 and words[2] == words[3] and got[0].numel() == R and torch.equal(got[0], u)
              and torch.equal(got[1].to(torch.int64), cnt) and torch.equal(got[2], sums) and torch.equal(got[3], mins)
              and torch.equal(got[4], maxs))
        report("sorted  ", name, R, legs, ok, model=(12 * n + 24 * R) / 8e12 * 1e6)
        del plan, got, u, cnt, sums, mins, maxs

        # part 2: the same groups in no order
        shuffled = keys[torch.randperm(n, device="cuda")]
        srt = ops.RadixSortPairs(n, 8)
        plan = ops.ReduceByKey(n, R)
        hashed = ops.GroupByHash(n, R)
        k2, v2 = torch.empty_like(shuffled), torch.empty_like(vals)

        def sort_route():
            k2.copy_(shuffled)
            v2.copy_(vals)
            srt.launch(k2, v2)
            plan.launch(k2, v2)

        def hash_route():
            hashed.launch(shuffled, vals)

        def vendor2():
            u, inv, cnt = torch.unique(shuffled, return_inverse=True, return_counts=True)
            return (u, cnt) + _torch_aggregates(inv, u.numel(), vals64, vals)

        legs = {"groupby_sorted": [], "groupby_hash": [], "torch": []}
        for _ in range(reps):
            legs["groupby_sorted"].append(median(times(sort_route, 5)))
            legs["groupby_hash"].append(median(times(hash_route, 5)))
            legs["torch"].append(median(times(vendor2, 5)))
        sort_route()
        got = plan.result()
        words = ops.check_reduce_by_key(k2, v2, *got)
        ok = (words[0] == 0 and words[1] == 0 and words[2] == words[3] and got[0].numel() == R
              and ops.workspace_status(srt.ws) == 0 and ops.check_sorted(k2)[0] == 0)
        report("unsorted", name, R, legs, ok)
        del plan, srt, hashed, shuffled, k2, v2, got


def launch_groupby_sorted(lg):
    n = 1 << (lg or 24)
    vals = ops.gen_uniform_u32(n, 43, 1, 10000)
    for name, keys, R in _sorted_key_shapes(n):
        if R not in (64, 1 << 20, n):
            continue
        plan = ops.ReduceByKey(n, R)
        for _ in range(5):
            plan.launch(keys, vals)
        plan.result()
    print("ok")


def _torch_window(keys, vals64):
    """the five columns of dbhip_scan_by_key_u32 (unsigned values below 2^31) from torch's scans"""
    n = keys.numel()
    rows = torch.arange(n, dtype=torch.int64, device="cuda")
    head = torch.ones(n, dtype=torch.bool, device="cuda")
    head[1:] = keys[1:] != keys[:-1]
    run = torch.cumsum(head, 0) - 1
    head_row = torch.cummax(torch.where(head, rows, torch.zeros_like(rows)), 0).values
    total = torch.cumsum(vals64, 0)
    sums = total - (total - vals64)[head_row]
    mins = torch.cummin(((run[-1] - run) << 32) | vals64, 0).values & 0xFFFFFFFF
    maxs = torch.cummax((run << 32) | vals64, 0).values & 0xFFFFFFFF
    return run, rows - head_row + 1, sums, mins, maxs


def window(lg):
    n = 1 << (lg or 24)
    reps = int(os.environ.get("REPS", "5"))
    vals = ops.gen_uniform_u32(n, 43, 1, 10000)
    vals64 = vals.to(torch.int64)

    def report(part, name, R, legs, ok, model=None):
        cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
        extra = f"  model {model:7.1f} us" if model else ""
        print(f"{TAG:10s} {part} n=2^{lg or 24} {name:14s} runs={R:9d}  {cols}{extra}  {'ok' if ok else 'WRONG'}   "
              + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)

    for name, keys, R in _sorted_key_shapes(n):
        plan = ops.ScanByKey(n)

        def scan_call():
            plan.launch(keys, vals)

        def vendor():
            return _torch_window(keys, vals64)

        legs = {"scan_by_key": [], "torch": []}
        for _ in range(reps):  # alternating
            legs["scan_by_key"].append(median(times(scan_call, 5)))
            legs["torch"].append(median(times(vendor, 5)))
        scan_call()
        got = plan.result()
        words = ops.check_scan_by_key(keys, vals, *got)
        want = vendor()
        ok = words[0] == 0 and words[2] == R and all(torch.equal(g.to(torch.int64), w) for g, w in zip(got, want))
        report("grouped ", name, R, legs, ok, model=40 * n / 8e12 * 1e6)
        del plan, got, want

        # part 2: the same groups in no order
        shuffled = keys[torch.randperm(n, device="cuda")]
        srt = ops.RadixSortPairs(n, 8)
        plan = ops.ScanByKey(n)
        k2 = torch.empty_like(shuffled)
        kept = {}

        def sort_route():
            k2.copy_(shuffled)
            kept["v"] = ops.gather_u32(vals, srt.launch(k2, None))
            plan.launch(k2, kept["v"])

        legs = {"window_sorted": []}
        for _ in range(reps):
            legs["window_sorted"].append(median(times(sort_route, 5)))
        sort_route()
        got = plan.result()
        words = ops.check_scan_by_key(k2, kept["v"], *got)
        ok = words[0] == 0 and words[2] == R and ops.workspace_status(srt.ws) == 0 and ops.check_sorted(k2)[0] == 0
        report("unsorted", name, R, legs, ok)
        del plan, srt, shuffled, k2, got, kept


def launch_window(lg):
    n = 1 << (lg or 24)
    vals = ops.gen_uniform_u32(n, 43, 1, 10000)
    for name, keys, R in _sorted_key_shapes(n):
        plan = ops.ScanByKey(n)
        for _ in range(5):
            plan.launch(keys, vals)
        plan.result()
        print(name, R, flush=True)
    print("ok")


def _join_pairs_shapes(lg):
    """(name, build keys, probe keys)"""
    for n in ([1 << lg] if lg else [1 << 20, 1 << 24, 1 << 26]):
        yield f"2^{n.bit_length() - 1} keys [1,n]", ops.gen_uniform_u32(n, 42, 1, n), ops.gen_uniform_u32(n, 43, 1, n)
    hot = torch.full((1 << 13,), 12345, dtype=torch.int32, device="cuda")
    yield "2^13 x 2^13 one key", hot, hot.clone()


def _torch_pairs(ids, pos, cnt, rid):
    """the same pairs from the same answer with torch ops: what a caller of ops.radix_join had to write before"""
    c = u64(cnt)
    rows = torch.repeat_interleave(torch.arange(c.numel(), device=c.device), c)
    first = torch.cumsum(c, 0) - c
    k = torch.arange(rows.numel(), device=c.device) - first[rows]
    return ids[u64(pos)[rows] + k], rid[rows]


def join_pairs(lg):
    for name, bk, pk in _join_pairs_shapes(lg):
        n = pk.numel()
        rid, pos, cnt, ids = ops.radix_join(bk, pk)
        counter = ops.JoinPairs(n, 0)
        counter.launch(ids, pos, cnt, rid)
        total = counter.count()
        plan = ops.JoinPairs(n, total)
        t_count = median(times(lambda: counter.launch(ids, pos, cnt, rid), 9))
        t_mine = median(times(lambda: plan.launch(ids, pos, cnt, rid), 9))
        b, p = plan.result()
        t_torch = median(times(lambda: _torch_pairs(ids, pos, cnt, rid), 9))
        tb, tp = _torch_pairs(ids, pos, cnt, rid)
        words = ops.check_join_pairs(bk, pk, ids, pos, cnt, b, p, rid)
        ok = (b.numel() == total and torch.equal(b, tb) and torch.equal(p, tp) and words[0] == 0 and words[1] == total
              and words[2] == words[3])
        gbytes = (12 * total + 44 * n) / 1e9  # 8 P written + 4 P ids + 44 n_probe of per-row columns and offsets
        print(f"{TAG:12s} {name:22s} pairs={total:9d}  join_pairs {t_mine:8.1f} us ({t_mine * 1e3 / max(total, 1):6.3f} ns/pair, "
              f"{gbytes / (t_mine * 1e-6) / 1e3:5.2f} TB/s = {gbytes / (t_mine * 1e-6) / 8e3:4.2f} of 8 TB/s)  count-only {t_count:7.1f} us  "
              f"torch {t_torch:9.1f} us  (torch / join_pairs {t_torch / t_mine:5.2f})  {'ok' if ok else 'WRONG'}", flush=True)
        del rid, pos, cnt, ids, b, p, tb, tp, plan, counter


def launch_join_pairs(lg):
    for name, bk, pk in _join_pairs_shapes(lg or 24):
        n = pk.numel()
        rid, pos, cnt, ids = ops.radix_join(bk, pk)
        counter = ops.JoinPairs(n, 0)
        counter.launch(ids, pos, cnt, rid)
        plan = ops.JoinPairs(n, counter.count())
        for _i in range(5):
            plan.launch(ids, pos, cnt, rid)
        b, p = plan.result()
        words = ops.check_join_pairs(bk, pk, ids, pos, cnt, b, p, rid)
        print(name, "ok" if words[0] == 0 and words[1] == b.numel() and words[2] == words[3] else "WRONG")


def _search_columns(m):
    """(name, ascending int32 column of m entries in [0, 2^31): torch's signed order is the unsigned one)"""
    yield "uniform", torch.sort(ops.gen_uniform_u32(m, 42, 0, 2**31 - 1)).values
    yield "2^13 distinct", torch.sort(ops.gen_uniform_u32(m, 42, 0, 8191) * (1 << 18)).values


def _search_levels(m, top=16384):
    levels = 0
    while m > top:
        m, levels = (m + 63) // 64, levels + 1
    return levels


def sorted_search(lg):
    """SS_M=<lg m> takes one column size instead of 2^14, 2^20, 2^24, 2^26"""
    n = 1 << (lg or 24)
    reps = int(os.environ.get("REPS", "5"))
    sizes = [int(os.environ["SS_M"])] if os.environ.get("SS_M") else [14, 20, 24, 26]
    draw = ops.gen_uniform_u32(n, 43, 0, 2**31 - 1)
    for lgm in sizes:
        m = 1 << lgm
        levels = _search_levels(m)
        for col_name, col in _search_columns(m):
            plan = ops.SortedSearch(m, n)
            t_index = median(times(lambda: plan.index(col), 9))
            width = max((16 << 31) // m, 1)
            for probe_name, lo in (("uniform", draw), ("sorted", torch.sort(draw).values),
                                   ("one value", torch.full_like(draw, 1 << 30))):
                for band_name, hi in (("hi == lo", None), ("band ~16", torch.clamp(lo.to(torch.int64) + width, max=2**31 - 1)
                                                           .to(torch.int32))):
                    top_hi = hi if hi is not None else lo

                    def mine():
                        plan.search(lo, hi)

                    def vendor():
                        pos = torch.searchsorted(col, lo, side="left")
                        return pos, torch.searchsorted(col, top_hi, side="right") - pos

                    legs = {"sorted_search": [], "torch": []}
                    for _ in range(reps):  # alternating
                        legs["sorted_search"].append(median(times(mine, 5)))
                        legs["torch"].append(median(times(vendor, 5)))
                    mine()
                    pos, cnt = plan.result()
                    words = ops.check_sorted_search(col, lo, hi, pos, cnt)
                    want = vendor()
                    ok = (words[0] == 0 and words[2] == int(want[1].sum()) and torch.equal(u64(pos), want[0])
                          and torch.equal(u64(cnt), want[1]))
                    floor = max(legs["sorted_search"]) <= min(legs["torch"])
                    model = n * levels * (1 if hi is None else 2) / 53e9 * 1e6  # block loads that leave the CU, at most
                    cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
                    print(f"{TAG:10s} n=2^{lg or 24} m=2^{lgm} {col_name:13s} probe {probe_name:9s} {band_name:8s} pairs={words[2]:11d}  "
                          f"{cols}  index {t_index:6.1f} us  levels {levels}  model {model:8.1f} us  floor {'holds' if floor else 'MISSED'}  "
                          f"{'ok' if ok else 'WRONG'}   "
                          + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)
                    del pos, cnt, want
            del plan, col


def range_join(lg):
    """the whole band join at 2^lg rows a side, keys in [1, n], hi = lo + 2: copy + argsort + index + search + pairs against
    torch.sort(stable) + two searchsorted + the expansion of join-pairs"""
    n = 1 << (lg or 24)
    reps = int(os.environ.get("REPS", "5"))
    build = ops.gen_uniform_u32(n, 42, 1, n)
    lo = ops.gen_uniform_u32(n, 43, 1, n)
    hi = lo + 2
    rid = torch.arange(n, dtype=torch.int32, device="cuda")
    keys = torch.empty_like(build)
    srt, search = ops.RadixSortPairs(n, 8), ops.SortedSearch(n, n)
    counter = ops.JoinPairs(n, 0)
    kept = {}

    def front():
        keys.copy_(build)
        kept["ids"] = srt.launch(keys, None)
        search.index(keys)
        search.search(lo, hi)

    front()
    counter.launch(kept["ids"], search.pos, search.cnt)
    total = counter.count()
    plan = ops.JoinPairs(n, total)

    def mine():
        front()
        plan.launch(kept["ids"], search.pos, search.cnt)

    def vendor():
        s, ids = torch.sort(build, stable=True)
        pos = torch.searchsorted(s, lo, side="left")
        cnt = torch.searchsorted(s, hi, side="right") - pos
        return _torch_pairs(ids, pos, cnt, rid)

    legs = {"range_join": [], "torch": []}
    for _ in range(reps):  # alternating
        legs["range_join"].append(median(times(mine, 5)))
        legs["torch"].append(median(times(vendor, 5)))
    mine()
    b, p = plan.result()
    words = ops.check_sorted_search(keys, lo, hi, search.pos, search.cnt)
    tb, tp = vendor()
    ok = (words[0] == 0 and words[2] == total == b.numel() and ops.check_sorted(keys)[0] == 0
          and torch.equal(u64(b), tb) and torch.equal(p, tp) and ops.workspace_status(search.ws) == 0)
    floor = max(legs["range_join"]) <= min(legs["torch"])
    cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
    print(f"{TAG:10s} range-join n=2^{lg or 24} pairs={total:11d}  {cols}  floor {'holds' if floor else 'MISSED'}  "
          f"{'ok' if ok else 'WRONG'}   " + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()),
          flush=True)


def _selection_row(name, mine, vendor, result, reps, floor_applies=True, model_us=None):
    """one shape of `selection`: alternating legs, the floor, and this code's row ids against torch's"""
    legs = {"select": [], "torch": []}
    for _ in range(reps):  # alternating
        legs["select"].append(median(times(mine, 5)))
        legs["torch"].append(median(times(vendor, 5)))
    mine()
    got, want = result(), vendor()
    ok = got.numel() == want.numel() and torch.equal(u64(got), want.to(torch.int64))
    floor = max(legs["select"]) <= min(legs["torch"])
    cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
    model = "" if model_us is None else f"  bytes at 8 TB/s {model_us:7.1f} us = {100 * model_us / median(sorted(legs['select'])):3.0f} %"
    verdict = ("floor " + ("holds" if floor else "MISSED")) if floor_applies else "no floor (below 2^20)"
    print(f"{TAG:10s} {name:58s} rows={got.numel():10d}  {cols}{model}  {verdict}  {'ok' if ok else 'WRONG'}   "
          + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)


def selection(lg):
    """dense sizes 2^22, 2^24, 2^26 (or 2^lg alone; below 20 no floor applies), then lists, the chain and the semi join
    (SEL_PARTS=dense,list,chain,semi picks parts).  Both legs run through the point where the row ids and their number are
    usable on the host: this code reads its device count, torch's nonzero synchronises by itself."""
    reps = int(os.environ.get("REPS", "5"))
    parts = os.environ.get("SEL_PARTS", "dense,list,chain,semi").split(",")
    shares = (0.0, 0.0001, 0.01, 0.1, 0.5, 1.0)

    def hi_of(share):  # lo = 1 so that share 0 is the empty interval [1, 0]; values below 2^31: torch compares int32
        return min(int(share * 2**31), 2**31 - 1)

    if "dense" in parts:
        for lgn in ([lg] if lg else [22, 24, 26]):
            n = 1 << lgn
            col = ops.gen_uniform_u32(n, 42, 0, 2**31 - 1)
            plan = ops.SelectRows(n)
            for share in shares:
                hi = hi_of(share)

                def mine():
                    plan.launch(col, 1, hi)
                    return plan.count()

                def vendor():
                    return torch.nonzero((col >= 1) & (col <= hi)).flatten()

                m = mine()
                _selection_row(f"dense n=2^{lgn} share {100 * share:7.2f} %", mine, vendor, plan.result, reps,
                               floor_applies=lgn >= 20, model_us=(4 * n + n / 4 + 4 * m) / 8e12 * 1e6)
            del col, plan
    n = 1 << 26
    if "list" in parts:
        col = ops.gen_uniform_u32(n, 42, 0, 2**31 - 1)
        for lgm in (20, 24):
            m = 1 << lgm
            shuffled = torch.randperm(n, device="cuda")[:m].to(torch.int32)
            plan = ops.SelectRows(m)
            for order, rows in (("sorted", torch.sort(shuffled).values), ("shuffled", shuffled)):
                rows64 = rows.to(torch.int64)
                for share in (0.01, 0.5):
                    hi = hi_of(share)

                    def mine():
                        plan.launch(col, 1, hi, rows=rows)
                        return plan.count()

                    def vendor():
                        v = col[rows64]
                        return rows[(v >= 1) & (v <= hi)]

                    _selection_row(f"list m=2^{lgm} of 2^26 {order:8s} share {100 * share:6.2f} %", mine, vendor, plan.result,
                                   reps)
            del plan
        del col
    if "chain" in parts:
        cols = [ops.gen_uniform_u32(n, 50 + i, 0, 2**31 - 1) for i in range(3)]
        his = [hi_of(0.5), hi_of(0.1), hi_of(0.5)]
        plan = ops.SelectRows(n)

        def mine():
            plan.launch(cols[0], 1, his[0])
            plan.refine(cols[1], 1, his[1])
            plan.refine(cols[2], 1, his[2])
            return plan.count()

        def vendor():
            keep = None
            for c, hi in zip(cols, his):
                k = (c >= 1) & (c <= hi)
                keep = k if keep is None else keep & k
            return torch.nonzero(keep).flatten()

        _selection_row("chain n=2^26 three predicates (50 %, 10 %, 50 %)", mine, vendor, plan.result, reps)
        del cols, plan
    if "semi" in parts:
        m = 1 << 24
        build, probe = ops.gen_uniform_u32(m, 42, 1, m), ops.gen_uniform_u32(m, 43, 1, m)
        join, plan = ops.HashJoin(m, m), ops.SelectRows(m)

        def mine():
            join.build(build)
            join.probe(probe)
            plan.launch(join.cnt, 1, 0xFFFFFFFF)
            return plan.count()

        def vendor():
            return torch.nonzero(torch.isin(probe, build)).flatten()

        _selection_row("semi join 2^24 x 2^24, keys in [1, 2^24]", mine, vendor, plan.result, reps)


def _times_after(prep, fn, k, warm=2):
    """times(), with prep() run in front of every timed span and outside it"""
    for _ in range(warm):
        prep()
        fn()
    out = []
    for _ in range(k):
        prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return sorted(out)


def _merge_row(name, legs, ok, floor_of=None, model_us=None, extra=""):
    """one shape of `merge`: the legs' ranges over the repetitions, the floor of floor_of = (mine, comparison)"""
    cols = "  ".join(f"{leg} {min(ts):9.1f} .. {max(ts):9.1f} us" for leg, ts in legs.items())
    verdict = ""
    if floor_of:
        mine, other = (legs[x] for x in floor_of)
        verdict = f"  floor {'holds' if max(mine) <= min(other) else 'MISSED'}  x{median(sorted(other)) / median(sorted(mine)):5.2f}"
        if model_us is not None:
            verdict += f"  bytes at 8 TB/s {model_us:7.1f} us = {100 * model_us / median(sorted(mine)):3.0f} %"
    if callable(extra):
        extra = extra(legs)
    print(f"{TAG:10s} {name:52s} {cols}{verdict}  {'ok' if ok else 'WRONG'}{extra}   "
          + " ".join(f"{leg}:" + "/".join(f"{t:.1f}" for t in ts) for leg, ts in legs.items()), flush=True)


def merge(lg):
    """MERGE_PARTS=merge,sets,any picks parts; sizes below 2^20 are not measured"""
    reps = int(os.environ.get("REPS", "5"))
    parts = os.environ.get("MERGE_PARTS", "merge,sets,any").split(",")

    def ascending(n, seed, step=3):
        """a strictly ascending int32 list of n rows: random gaps of 1 .. step"""
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.cumsum(torch.randint(1, step + 1, (n,), device="cuda", generator=g, dtype=torch.int32), 0, dtype=torch.int32)

    if "merge" in parts:
        for lgn in ([lg] if lg else [22, 24, 26]):
            n = 1 << lgn
            half = n // 2
            shapes = [("na = nb uniform", lambda: (ops.gen_uniform_u32(half, 42, 0, 2**31 - 1), ops.gen_uniform_u32(half, 43, 0, 2**31 - 1))),
                      ("all keys equal", lambda: (torch.full((half,), 7, dtype=torch.int32, device="cuda"),) * 2),
                      ("A below B", lambda: (torch.arange(half, dtype=torch.int32, device="cuda"),
                                             torch.arange(half, n, dtype=torch.int32, device="cuda"))),
                      ("nb = 2^10", lambda: (ops.gen_uniform_u32(n - 1024, 42, 0, 2**31 - 1), ops.gen_uniform_u32(1024, 43, 0, 2**31 - 1)))]
            for shape, build in shapes:
                a, b = (torch.sort(x).values.contiguous() for x in build())
                cat = torch.cat([a, b])
                va, vb = ops.gen_uniform_u32(a.numel(), 44, 0, 2**31 - 1), ops.gen_uniform_u32(b.numel(), 45, 0, 2**31 - 1)
                work = cat.clone()
                plan, sort = ops.MergeSorted(a.numel(), b.numel()), ops.RadixSortPairs(n, 8)
                legs = {"merge ids": [], "argsort": [], "merge keys": [], "merge pairs": []}
                for _ in range(reps):  # alternating
                    legs["merge ids"].append(median(times(lambda: plan.launch(a, b, row_ids=True), 5)))
                    legs["argsort"].append(median(_times_after(lambda: work.copy_(cat), lambda: sort.launch(work), 5)))
                    legs["merge keys"].append(median(times(lambda: plan.launch(a, b), 5)))
                    legs["merge pairs"].append(median(times(lambda: plan.launch(a, b, va, vb), 5)))
                work.copy_(cat)
                perm = sort.launch(work)
                plan.launch(a, b, row_ids=True)
                keys, ids = plan.result()
                ok = torch.equal(keys, work) and torch.equal(ids, perm[:n]) and ops.workspace_status(sort.ws) == 0
                plan.launch(a, b, va, vb)
                keys, vals = plan.result()
                ok = ok and torch.equal(keys, work) and torch.equal(vals, torch.cat([va, vb])[u64(perm[:n])])
                _merge_row(f"merge out=2^{lgn} {shape}", legs, ok, ("merge ids", "argsort"), 12 * n / 8e12 * 1e6,
                           f"  keys 8n {8 * n / 8e12 * 1e6:.1f} us pairs 16n {16 * n / 8e12 * 1e6:.1f} us")
                del a, b, cat, va, vb, work, plan, sort, perm, keys, ids, vals
    if "sets" in parts:
        for lgn in ([lg] if lg else [20, 24, 26]):
            n = 1 << lgn
            a, b = ascending(n, 1), ascending(n, 2)
            plan = ops.RowSets(n, n)
            vendors = {"union": lambda: torch.unique(torch.cat((a, b))),
                       "intersect": lambda: a[torch.isin(a, b, assume_unique=True)],
                       "difference": lambda: a[~torch.isin(a, b, assume_unique=True)]}
            for op, vendor in vendors.items():
                def mine():
                    plan.launch(op, a, b)
                    return plan.count()

                legs = {op: [], "torch": []}
                for _ in range(reps):
                    legs[op].append(median(times(mine, 5)))
                    legs["torch"].append(median(times(vendor, 5)))
                mine()
                got, want = plan.result(), vendor()
                ok = got.numel() == want.numel() and torch.equal(got, want)
                reads = 2 * 8 * n  # count, then the merge again where a tile keeps something
                _merge_row(f"{op} 2^{lgn} + 2^{lgn} rows -> {got.numel()}", legs, ok, (op, "torch"),
                           (reads + 4 * got.numel()) / 8e12 * 1e6)
            del a, b, plan
    if "any" in parts:
        n = 1 << 26
        cols = [ops.gen_uniform_u32(n, 50 + i, 0, 2**31 - 1) for i in range(2)]
        first, second, sets = ops.SelectRows(n), ops.SelectRows(n), ops.RowSets(n, n)
        for share in (0.01, 0.5):
            hi = min(int(share * 2**31), 2**31 - 1)

            def mine():
                first.launch(cols[0], 1, hi)
                second.launch(cols[1], 1, hi)
                (ra, ca), (rb, cb) = first.output(), second.output()
                sets.launch("union", ra, rb, ca, cb)
                return sets.count()

            def vendor():
                return torch.nonzero(((cols[0] >= 1) & (cols[0] <= hi)) | ((cols[1] >= 1) & (cols[1] <= hi))).flatten()

            legs = {"select_any": [], "torch": []}
            for _ in range(reps):
                legs["select_any"].append(median(times(mine, 5)))
                legs["torch"].append(median(times(vendor, 5)))
            mine()
            got, want = sets.result(), vendor()
            ok = got.numel() == want.numel() and torch.equal(u64(got), want.to(torch.int64))
            _merge_row(f"select_any n=2^26 shares ({100 * share:.0f} %, {100 * share:.0f} %) -> {got.numel()}", legs, ok,
                       ("select_any", "torch"))


def take(lg):
    """TAKE_PARTS=take,aggregate,dense,chain picks parts; lists below 2^19 entries are not measured"""
    reps = int(os.environ.get("REPS", "5"))
    parts = os.environ.get("TAKE_PARTS", "take,aggregate,dense,chain").split(",")
    n = 1 << (lg or 26)
    cols = [ops.gen_uniform_u32(n, 60 + i, 0, 2**31 - 1) for i in range(4)]

    def lists():
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        for share in (0.01, 0.1, 0.5):
            keep = torch.rand(n, device="cuda", generator=g) < share
            yield f"ascending {100 * share:3.0f} % kept", torch.nonzero(keep).flatten().to(torch.int32)
        yield "ascending 100 % kept", torch.arange(n, dtype=torch.int32, device="cuda")
        perm = torch.randperm(n, device="cuda", generator=g).to(torch.int32)
        for lgm in (20, 24):
            if (1 << lgm) < n:
                yield f"ascending 2^{lgm} random", torch.sort(perm[: 1 << lgm]).values.contiguous()
                yield f"shuffled  2^{lgm} random", perm[: 1 << lgm].contiguous()
        yield "shuffled  all rows", perm

    def reduced(v):  # the four numbers on the host after one transfer
        return [v.numel()] + torch.stack([v.sum(dtype=torch.int64), v.min().to(torch.int64), v.max().to(torch.int64)]).tolist()

    def run(name, legs_fn, ok_fn, floor_of, model_us, extra):
        legs = {leg: [] for leg in legs_fn}
        for _ in range(reps):  # alternating
            for leg, fn in legs_fn.items():
                legs[leg].append(median(times(fn, 5)))
        _merge_row(name, legs, ok_fn(), floor_of, model_us, extra)

    if "take" in parts or "aggregate" in parts:
        for name, rows in lists():
            m = rows.numel()
            lines = torch.unique(rows >> 5).numel()  # 128-byte lines of a column the list touches
            if "take" in parts:
                for k in (1, 2, 4):
                    plan = ops.TakeRows(m, k)
                    mine = lambda: plan.launch(cols[:k], rows)  # noqa: E731
                    vendor = lambda: [torch.index_select(c, 0, rows) for c in cols[:k]]  # noqa: E731

                    def ok():
                        mine()
                        return all(torch.equal(g, w) for g, w in zip(plan.result(), vendor()))

                    model = (4 * m + 4 * k * m + 128 * k * lines) / 8e12 * 1e6
                    run(f"take k={k} m={m} {name}", {"take": mine, "torch": vendor}, ok, ("take", "torch"), model,
                        lambda legs: f"  {k * m / median(sorted(legs['take'])) / 1e3:6.1f} G gathers/s")
                    del plan
            if "aggregate" in parts:
                agg, plan = ops.AggregateRows(m), ops.TakeRows(m, 1)

                def mine():
                    agg.launch(cols[0], rows)
                    return agg.result()

                def vendor():
                    return reduced(torch.index_select(cols[0], 0, rows))

                def own_take():
                    plan.launch(cols[0], rows)
                    return reduced(plan.outs[0][:m])

                model = (4 * m + 128 * lines) / 8e12 * 1e6
                run(f"aggregate m={m} {name}", {"aggregate": mine, "torch": vendor, "take+torch": own_take},
                    lambda: list(mine()) == vendor() == own_take(), ("aggregate", "torch"), model,
                    lambda legs: f"  {m / median(sorted(legs['aggregate'])) / 1e3:6.1f} G gathers/s  against take+torch "
                                 f"{'holds' if max(legs['aggregate']) <= min(legs['take+torch']) else 'MISSED'}")
                del agg, plan
            del rows
    if "dense" in parts:
        for lgn in sorted({20, 24, 26, lg or 26}):
            if (1 << lgn) > n:
                continue
            col = cols[0][: 1 << lgn]
            agg = ops.AggregateRows(col.numel())

            def mine():
                agg.launch(col)
                return agg.result()

            run(f"aggregate over all rows n=2^{lgn}", {"aggregate": mine, "torch": lambda: reduced(col)},
                lambda: list(mine()) == reduced(col), ("aggregate", "torch"), 4 * col.numel() / 8e12 * 1e6, lambda legs: "")
            del agg
    if "chain" in parts:
        sel, agg = ops.SelectRows(n), ops.AggregateRows(n)
        for share in (0.01, 0.5):
            hi = min(int(share ** 0.5 * 2**31), 2**31 - 1)  # two predicates of sqrt(share) each

            def mine():
                sel.launch(cols[0], 1, hi)
                sel.refine(cols[1], 1, hi)
                agg.launch(cols[2], *sel.output())
                return agg.result()

            def vendor():
                keep = (cols[0] >= 1) & (cols[0] <= hi) & (cols[1] >= 1) & (cols[1] <= hi)
                return reduced(cols[2][keep])

            run(f"select -> refine -> aggregate n={n} share {100 * share:.0f} %", {"chain": mine, "torch": vendor},
                lambda: list(mine()) == vendor(), ("chain", "torch"), None, lambda legs: f"  rows {mine()[0]}")


def dict_encoding(lg):
    """DICT_PARTS=factorize,encode,groupby picks parts; DICT_CARDS=64,4096,... picks cardinalities (0: all rows distinct,
    1: the one-key column)"""
    reps = int(os.environ.get("REPS", "5"))
    parts = os.environ.get("DICT_PARTS", "factorize,encode,groupby").split(",")
    cards = [int(c) for c in os.environ.get("DICT_CARDS", "1,64,4096,1048576,0").split(",")]
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def spread(t):  # distinct int64 values -> distinct 32-bit patterns all over the range (an odd multiplier is a bijection)
        return bits32((t * 2654435761) % 2**32)

    def column(n, card):
        if card == 0:
            return spread(torch.randperm(n, device="cuda", generator=g))
        values = spread(torch.randperm(max(card, 2) * 4, device="cuda", generator=g)[:card])
        return values[torch.randint(0, card, (n,), device="cuda", generator=g)].contiguous()

    def run(name, legs_fn, ok_fn, floor_of, model_us=None, extra=""):
        legs = {leg: [] for leg in legs_fn}
        for _ in range(reps):  # alternating
            for leg, fn in legs_fn.items():
                legs[leg].append(median(times(fn, 5)))
        _merge_row(name, legs, ok_fn(), floor_of, model_us, extra)

    for lgn in ([lg] if lg else [20, 24, 26]):
        n = 1 << lgn
        for card in cards:
            if card > n:
                continue
            d = card or n
            label = f"n=2^{lgn} d={'n' if card == 0 else card}"
            col = column(n, card)
            if "factorize" in parts or "encode" in parts:
                # the order is int32's on both sides: what torch.unique gives for an int32 column
                bound, whole = ops.Dictionary(n, d), (ops.Dictionary(n) if d < n else None)
                codes = torch.empty(n, dtype=torch.int32, device="cuda")

                def mine(plan=bound):
                    plan.build(col, signed=True)
                    plan.encode(col, out=codes)

                vendor = lambda: torch.unique(col, sorted=True, return_inverse=True)  # noqa: E731

                def ok(plan=bound):
                    mine(plan)
                    uniques, inverse = vendor()
                    return torch.equal(plan.result(), uniques) and torch.equal(codes.to(torch.int64), inverse)

                if "factorize" in parts:
                    legs = {"factorize": mine, "torch": vendor}
                    if whole is not None:  # capacity = n: the build sorts n padded entries whatever d is
                        legs["capacity=n"] = lambda: mine(whole)
                    run(f"factorize {label}", legs, lambda: ok() and (whole is None or ok(whole)), ("factorize", "torch"), None,
                        lambda legs: f"  capacity=n costs x{median(sorted(legs['capacity=n'])) / median(sorted(legs['factorize'])):.2f}"
                        if "capacity=n" in legs else "")
                if "encode" in parts:
                    mine()
                    uniques = bound.result().clone()
                    enc = lambda: bound.encode(col, out=codes)  # noqa: E731
                    search = lambda: torch.searchsorted(uniques, col)  # noqa: E731
                    body = "LDS" if 2 * d <= ops.DICT_LDS_SLOTS else "global"
                    run(f"encode ({body} body) {label}", {"encode": enc, "torch": search},
                        lambda: (enc(), torch.equal(codes.to(torch.int64), search()))[1], ("encode", "torch"), 8 * n / 8e12 * 1e6)
                del bound, whole, codes
            if "groupby" in parts and card != 0 and lgn <= int(os.environ.get("DICT_GROUPBY_LG", "24")):
                # two key columns of about sqrt(d) values each: about d groups
                side = max(int(round(d ** 0.5)), 1)
                a, b = column(n, side), column(n, side)
                vals = ops.gen_uniform_u32(n, 9, 0, 2**31 - 1)
                vals64 = vals.to(torch.int64)

                def mine_groups():
                    return ops.groupby_columns([a, b], vals, signed=True)

                def vendor_groups():
                    rows, inverse = torch.unique(torch.stack([a, b], dim=1), dim=0, return_inverse=True)
                    return rows, torch.zeros(rows.shape[0], dtype=torch.int64, device="cuda").scatter_add_(0, inverse.flatten(), vals64)

                def ok_groups():
                    (ka, kb), sums, _ = mine_groups()
                    rows, want = vendor_groups()
                    return torch.equal(ka, rows[:, 0]) and torch.equal(kb, rows[:, 1]) and torch.equal(u64(sums), want % 2**32)

                run(f"group by two columns n=2^{lgn} {side} x {side}", {"groupby_columns": mine_groups, "torch": vendor_groups},
                    ok_groups, ("groupby_columns", "torch"))
                del a, b, vals, vals64
            del col


def bitpack(lg):
    """BITPACK_PARTS=select,pack,unpack,take picks parts; BITPACK_WIDTHS=4,8,... picks widths"""
    reps = int(os.environ.get("REPS", "5"))
    parts = os.environ.get("BITPACK_PARTS", "select,pack,unpack,take").split(",")
    widths = [int(w) for w in os.environ.get("BITPACK_WIDTHS", "4,8,12,16,24,32").split(",")]
    n = 1 << (lg or 26)
    us = lambda nbytes: nbytes / 8e12 * 1e6  # noqa: E731

    def run(name, legs_fn, ok, floor_of, model_us, report=None):
        legs = {leg: [] for leg in legs_fn}
        for _ in range(reps):  # alternating
            for leg, fn in legs_fn.items():
                legs[leg].append(median(times(fn, 5)))
        extra = ""
        if report:  # no floor: the ratio and the bytes all the same
            mine, other = (median(sorted(legs[x])) for x in report)
            extra = f"  (no floor) x{other / mine:5.2f}  bytes at 8 TB/s {model_us:7.1f} us = {100 * model_us / mine:3.0f} %"
        _merge_row(name, legs, ok, floor_of, model_us, extra)

    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    perm = torch.randperm(n, device="cuda", generator=g).to(torch.int32)
    for width in widths:
        codes = ops.gen_uniform_u32(n, 70 + width, 0, 2**width - 1)  # the decoded column; base 0
        packer = ops.BitPack(n, width)
        packer.launch(codes)
        pc = packer.result()
        if "select" in parts:
            packed_plan, plain_plan = ops.SelectRows(n), ops.SelectRows(n)
            for share in (0, 0.01, 0.5, 1.0):
                lo, hi = (1, 0) if share == 0 else (0, 2**32 - 1) if share == 1.0 else (0, max(int(share * 2**width) - 1, 0))
                mine = lambda: packed_plan.launch(pc, lo, hi)  # noqa: E731
                plain = lambda: plain_plan.launch(codes, lo, hi)  # noqa: E731
                mine(), plain()
                ok = torch.equal(packed_plan.result(), plain_plan.result())
                m = packed_plan.count()
                floor = width <= 16
                run(f"select n=2^{lg or 26} width {width:2d} kept {100 * m / n:5.1f} %", {"packed": mine, "plain": plain}, ok,
                    ("packed", "plain") if floor else None, us(n * width / 8 + n / 4 + 4 * m), None if floor else ("packed", "plain"))
            del packed_plan, plain_plan
        if "pack" in parts:
            ok = torch.equal(ops.unpack(pc), codes)
            run(f"pack n=2^{lg or 26} width {width:2d}", {"pack": lambda: packer.launch(codes), "clone": lambda: torch.clone(codes)},
                ok, None, us(4 * n + n * width / 8), ("pack", "clone"))
        if "unpack" in parts:
            out, ws = torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(256, dtype=torch.uint8, device="cuda")
            ops.unpack(pc, out=out, ws=ws)
            ok = torch.equal(out, codes) and ops.workspace_status(ws) == 0
            run(f"unpack n=2^{lg or 26} width {width:2d}", {"unpack": lambda: ops.unpack(pc, out=out, ws=ws), "clone": lambda: torch.clone(codes)},
                ok, None, us(4 * n + n * width / 8), ("unpack", "clone"))
            del out
        if "take" in parts:
            for share in (0.01, 0.5):
                m = int(share * n)
                for order, rows in (("ascending", torch.sort(perm[:m]).values.contiguous()), ("shuffled", perm[:m].contiguous())):
                    out, ws = torch.empty(m, dtype=torch.int32, device="cuda"), torch.zeros(256, dtype=torch.uint8, device="cuda")
                    taker = ops.TakeRows(m, 1)
                    mine = lambda: ops.unpack(pc, rows, out=out, ws=ws)  # noqa: E731
                    plain = lambda: taker.launch(codes, rows)  # noqa: E731
                    mine(), plain()
                    ok = torch.equal(out, taker.result()[0]) and ops.workspace_status(ws) == 0
                    lines = torch.unique(rows >> 5).numel()  # 128-byte lines of the 32-bit column the list touches
                    run(f"take n=2^{lg or 26} width {width:2d} m={m} {order}", {"unpack": mine, "take": plain}, ok, None,
                        us(8 * m + 128 * lines * width / 32), ("unpack", "take"))
                    del out, taker, rows
        del codes, packer, pc


def _bloom_always_set_lib():
    """bloom_filter.cpp built without test-before-set (measurement only) -> its ctypes handle"""
    import ctypes
    import subprocess
    from dwarf_bench_amd import bloom_native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host, lib = os.path.join(root, "dwarf_bench_amd", "host"), os.path.join(root, "dwarf_bench_amd", "_lib")
    so = os.path.join(lib, "ab", "libbloom_always_set.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(os.path.join(host, "bloom_filter.cpp")):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC", "-shared", "-DHIP_ENABLED",
                        "-DDBENCH_BLOOM_ALWAYS_SET", "-I", host, "-I", os.path.join(root, "include"), "-I",
                        os.path.join(root, "dwarf_bench_amd", "csrc"), "-x", "hip", "--offload-arch=gfx950",
                        os.path.join(host, "bloom_filter.cpp"), "-o", so, "-L", lib, "-ldbench", "-ldbhip",
                        "-Wl,-rpath,$ORIGIN/.."], check=True)
    bloom_native.lib()  # libdbhip.so and libdbench.so first
    h = ctypes.CDLL(so)
    res, args = bloom_native.ENTRY_POINTS["dbench_bloom_build_u32"]
    h.dbench_bloom_build_u32.restype, h.dbench_bloom_build_u32.argtypes = res, args
    return h


def bloom(lg):
    """BLOOM_PARTS=build,probe,semi picks parts; BLOOM_BUILD_LG the build's rows"""
    reps = int(os.environ.get("REPS", "3"))
    parts = os.environ.get("BLOOM_PARTS", "build,probe,semi").split(",")
    n = 1 << (lg or 26)
    nb = 1 << int(os.environ.get("BLOOM_BUILD_LG", "24"))
    sizes = [1 << 10, 1 << 16, 1 << 20, 1 << 26]

    def run(name, legs_fn, ok, report, extra=""):
        legs = {leg: [] for leg in legs_fn}
        for _ in range(reps):  # alternating
            for leg, fn in legs_fn.items():
                legs[leg].append(median(times(fn, 5)))
        mine = median(sorted(legs[report[0]]))
        ratios = "  ".join(f"{other} / {report[0]} x{median(sorted(legs[other])) / mine:5.2f}" for other in report[1:])
        _merge_row(name, legs, ok, None, None, f"  (no floor) {ratios}{extra}")

    def distinct(count, salt):  # distinct 32-bit keys: an odd multiple of a permutation; salt moves the set
        g = torch.Generator(device="cuda")
        g.manual_seed(salt)
        return bits32((torch.randperm(count, device="cuda", generator=g) * 2654435761 + salt * 2**27) % 2**32)

    keys = distinct(nb, 1)
    if "build" in parts:
        always = _bloom_always_set_lib()
        few = ops.gen_uniform_u32(nb, 5, 1, 10000)
        for name, col, words in [("distinct 16 b/key", keys, ops.bloom_words(nb, 16)), ("[1, 10000] 16 b/key", few, ops.bloom_words(nb, 16))] + \
                [(f"distinct {w} words", keys, w) for w in sizes]:
            tested, plain = ops.BloomFilter(words), ops.BloomFilter(words)
            unconditional = lambda: always.dbench_bloom_build_u32(  # noqa: E731
                col.data_ptr(), nb, None, None, 0, 0, 0, plain.filter.data_ptr(), words, plain.ws.data_ptr(), 256,
                torch.cuda.current_stream().cuda_stream)
            tested.build(col)
            assert unconditional() == 0
            ok = torch.equal(tested.filter, plain.filter) and tested.status() == 0
            fill = float((tested.filter.view(torch.uint8).to(torch.int32).unsqueeze(1) >> torch.arange(8, device="cuda") & 1).float().mean()) if words <= 1 << 22 else float("nan")
            run(f"build n=2^{nb.bit_length() - 1} {name} ({8 * words >> 10} KiB)", {"test-before-set": lambda: tested.build(col), "always-set": unconditional,
                "clone": lambda: torch.clone(col)}, ok, ("test-before-set", "always-set", "clone"),
                f"  {nb / median(times(lambda: tested.build(col), 5)) / 1e3:6.2f} G keys/s  fill {fill:.3f}")
            del tested, plain
    if "probe" in parts:
        strangers = distinct(n, 2)  # salt 2: disjoint from `keys` with overwhelming share; the check below is exact anyway
        for words in sizes:
            held = keys[: min(4 * words, nb)].contiguous()
            bl = ops.BloomFilter(words)
            bl.build(held)
            join = ops.HashJoin(held.numel(), n)
            join.build(held)
            for share in (0.0, 0.01, 0.5, 1.0):
                g = torch.Generator(device="cuda")
                g.manual_seed(int(share * 100) + 7)
                pick = torch.rand(n, device="cuda", generator=g) < share
                col = torch.where(pick, held[torch.randint(0, held.numel(), (n,), device="cuda", generator=g)], strangers)
                del pick
                mine_plan, range_plan = ops.SelectRows(n), ops.SelectRows(n)
                hi = 0 if share == 0 else min(int(share * 2**32), 2**32 - 1)
                lo = 1 if share == 0 else 0  # lo > hi: nothing kept
                mine = lambda: mine_plan.launch_in(bl, col)  # noqa: E731
                stream = lambda: range_plan.launch(col, lo, hi)  # noqa: E731
                gather = lambda: join.probe(col)  # noqa: E731
                mine(), gather()
                kept = mine_plan.count()
                _, cnt, _ = join.result()
                partners = int((cnt != 0).sum())
                ok = kept >= partners and mine_plan.status() == 0 and bool((cnt[mine_plan.result().long()] != 0).sum() == partners)
                run(f"probe n=2^{lg or 26} filter {8 * words >> 10} KiB partners {100 * partners / n:5.1f} % kept {100 * kept / n:5.1f} %",
                    {"bloom": mine, "select_range": stream, "join probe": gather}, ok, ("bloom", "select_range", "join probe"),
                    f"  {n / median(times(mine, 5)) / 1e3:6.2f} G rows/s")
                del col, mine_plan, range_plan
            del bl, join, held
        del strangers
    if "semi" in parts:
        strangers = distinct(n, 2)
        for lb in (16, 20, 24):
            build = distinct(1 << lb, 1)
            for share in (0.0, 0.01, 0.1, 0.5, 1.0):
                g = torch.Generator(device="cuda")
                g.manual_seed(int(share * 100) + 11)
                pick = torch.rand(n, device="cuda", generator=g) < share
                probe = torch.where(pick, build[torch.randint(0, build.numel(), (n,), device="cuda", generator=g)], strangers)
                del pick
                plain = lambda: ops.semi_join(build, probe)  # noqa: E731
                pre = lambda: ops.semi_join(build, probe, bloom_bits=16)  # noqa: E731
                a, b = plain(), pre()
                ok = torch.equal(a, b)
                m = a.numel()
                del a, b
                legs = {"prefiltered": [], "plain": []}
                for _ in range(reps):
                    legs["prefiltered"].append(median(times(pre, 5)))
                    legs["plain"].append(median(times(plain, 5)))
                verdict = "wins" if max(legs["prefiltered"]) <= min(legs["plain"]) else "MISSED"
                _merge_row(f"semi_join build 2^{lb} probe 2^{lg or 26} partners {100 * m / n:5.1f} %", legs, ok, None, None,
                           f"  prefilter {verdict}  x{median(sorted(legs['plain'])) / median(sorted(legs['prefiltered'])):5.2f}")
                del probe
            del build


def _hll_always_max_lib():
    """hll_sketch.cpp built without test-before-set (measurement only) -> its ctypes handle"""
    import ctypes
    import subprocess
    from dwarf_bench_amd import hll_native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host, lib = os.path.join(root, "dwarf_bench_amd", "host"), os.path.join(root, "dwarf_bench_amd", "_lib")
    so = os.path.join(lib, "ab", "libhll_always_max.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(os.path.join(host, "hll_sketch.cpp")):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC", "-shared", "-DHIP_ENABLED",
                        "-DDBENCH_HLL_ALWAYS_MAX", "-I", host, "-I", os.path.join(root, "include"), "-I",
                        os.path.join(root, "dwarf_bench_amd", "csrc"), "-x", "hip", "--offload-arch=gfx950",
                        os.path.join(host, "hll_sketch.cpp"), "-o", so, "-L", lib, "-ldbench", "-ldbhip",
                        "-Wl,-rpath,$ORIGIN/.."], check=True)
    hll_native.lib()  # libdbhip.so and libdbench.so first
    h = ctypes.CDLL(so)
    res, args = hll_native.ENTRY_POINTS["dbench_hll_build_u32"]
    h.dbench_hll_build_u32.restype, h.dbench_hll_build_u32.argtypes = res, args
    return h


def hll(_):
    """HLL_LGS=20,24,26 picks the sizes, HLL_PS=12,14 the precisions, HLL_SHAPES a subset of the shape names, separated by ;"""
    import ctypes
    reps = int(os.environ.get("REPS", "3"))
    lgs = [int(x) for x in os.environ.get("HLL_LGS", "20,24,26").split(",")]
    ps = [int(x) for x in os.environ.get("HLL_PS", "12,14").split(",")]
    names = ("distinct", "[1, 10000]", "one hot key", "sorted", "two columns", "list 1 %", "list 50 %")
    shapes = [s for s in os.environ.get("HLL_SHAPES", ";".join(names)).split(";") if s in names]  # (a name holds a comma)
    always = _hll_always_max_lib()
    stream_ptr = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    for lg in lgs:
        n = 1 << lg
        g = torch.Generator(device="cuda")
        g.manual_seed(lg)
        for shape in shapes:
            second = rows = None
            if shape in ("distinct", "list 1 %", "list 50 %"):  # an odd multiple of a permutation
                col = bits32((torch.randperm(n, device="cuda", generator=g) * 2654435761) % 2**32)
            elif shape == "[1, 10000]":
                col = ops.gen_uniform_u32(n, 5, 1, 10000)
            elif shape == "one hot key":  # 99 % of the rows hold one key
                col = bits32(torch.randint(0, 2**32, (n,), device="cuda", generator=g))
                col[torch.rand(n, device="cuda", generator=g) < 0.99] = 12345
            elif shape == "sorted":
                col = bits32(torch.sort(torch.randint(0, n // 4, (n,), device="cuda", generator=g))[0])
            else:  # 2^16 x up to 2^10 tuples
                col = ops.gen_uniform_u32(n, 6, 0, (1 << 16) - 1)
                second = ops.gen_uniform_u32(n, 7, 0, (1 << 10) - 1)
            if shape.startswith("list"):
                m = n // 100 if shape == "list 1 %" else n // 2
                rows = torch.randint(0, n, (m,), device="cuda", generator=g).to(torch.int32)  # unsorted, rows repeat
            cols = [col] if second is None else [col, second]
            # the exact routes: the dictionary build's cardinality and torch.unique, through the list where there is one
            if second is not None:
                exact_in = None
                truth = int(torch.unique((u64(col) << 32) | u64(second)).numel())
            else:
                exact_in = (lambda: col) if rows is None else (lambda: ops.take(col, rows))
                truth = int(torch.unique(exact_in()).numel())
            legs_exact = {}
            if exact_in is not None:
                d = ops.Dictionary(rows.numel() if rows is not None else n, max(truth, 1))
                legs_exact["factorize"] = lambda: d.build(exact_in())
                legs_exact["torch.unique"] = (lambda: torch.unique(col).numel()) if rows is None else (lambda: torch.unique(col[rows.long()]).numel())
                legs_exact["factorize"]()
                assert d.count() == truth
            else:  # two columns: encode_columns' composite codes, and torch.unique over the 64-bit pairs
                legs_exact["torch.unique"] = lambda: torch.unique((u64(col) << 32) | u64(second)).numel()
            sel = ops.SelectRows(n)
            for p in ps:
                mine, plain = ops.HyperLogLog(p, 0), ops.HyperLogLog(p, 0)
                ptrs = (ctypes.c_void_p * 4)(*[c.data_ptr() for c in cols])
                unconditional = lambda: always.dbench_hll_build_u32(  # noqa: E731
                    ptrs, len(cols), n, rows.data_ptr() if rows is not None else None, None, rows.numel() if rows is not None else 0,
                    0, 0, p, plain.registers.data_ptr(), plain.hist.data_ptr(), plain.ws.data_ptr(), plain.ws_bytes, stream_ptr())
                sketch = lambda: mine.build(cols, rows=rows)  # noqa: E731
                sketch()
                assert unconditional() == 0
                estimate = mine.estimate()
                ok = torch.equal(mine.registers, plain.registers) and torch.equal(mine.hist, plain.hist) and plain.status() == 0
                err = (estimate - truth) / truth
                legs_fn = {"sketch": sketch, "always-max": unconditional, **legs_exact, "select_range": lambda: sel.launch(col, 0, 0)}
                legs = {leg: [] for leg in legs_fn}
                for _ in range(reps):  # alternating
                    for leg, fn in legs_fn.items():
                        legs[leg].append(median(times(fn, 5)))
                best = min(min(legs[x]) for x in legs_exact)
                verdict = "HELD" if max(legs["sketch"]) <= best else "MISSED"
                s = median(sorted(legs["sketch"]))
                _merge_row(f"hll n=2^{lg} p={p} {shape}", legs, ok, None, None,
                           f"  floor {verdict} x{best / s:7.2f}  always-max / sketch x{median(sorted(legs['always-max'])) / s:5.2f}"
                           f"  sketch / select_range x{s / median(sorted(legs['select_range'])):5.2f}"
                           f"  distinct {truth} estimate {estimate:.0f} error {100 * err:+.2f} % = {err / ops.hll_relative_error(p):+.2f} se")
                del mine, plain
            del col, second, rows, cols, sel, legs_exact


def quantile(_):
    """QUANTILE_LGS=20,24,26 picks the sizes, QUANTILE_SHAPES a subset of the shape names, separated by ;"""
    reps = int(os.environ.get("REPS", "3"))
    lgs = [int(x) for x in os.environ.get("QUANTILE_LGS", "20,24,26").split(",")]
    names = ("uniform", "[1, 10000]", "all equal", "sorted", "list 1 %", "list 50 %")
    shapes = [s for s in os.environ.get("QUANTILE_SHAPES", ";".join(names)).split(";") if s in names]
    rank_sets = {"median": [(1, 2)], "deciles": [(i, 10) for i in range(1, 10)]}

    for lg in lgs:
        n = 1 << lg
        g = torch.Generator(device="cuda")
        g.manual_seed(lg)
        for shape in shapes:
            rows = None
            if shape in ("uniform", "list 1 %", "list 50 %"):
                col = ops.gen_uniform_u32(n, 5, 0, 2**32 - 1)
            elif shape == "[1, 10000]":
                col = ops.gen_uniform_u32(n, 5, 1, 10000)
            elif shape == "all equal":
                col = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
            else:
                col = torch.sort(ops.gen_uniform_u32(n, 5, 0, 2**32 - 1))[0]
            if shape.startswith("list"):
                m = n // 100 if shape == "list 1 %" else n // 2
                rows = torch.randint(0, n, (m,), device="cuda", generator=g).to(torch.int32)  # unsorted, rows repeat
            m = n if rows is None else rows.numel()
            taker = ops.TakeRows(m) if rows is not None else None
            candidates = (lambda: col) if rows is None else (lambda: taker.launch([col], rows) or taker.output()[0][0][:m])
            tmp = torch.empty(m, dtype=torch.int32, device="cuda")
            sorter = ops.RadixSort(m)
            for set_name, qs in rank_sets.items():
                ranks = [-(-num * m // den) - 1 for num, den in qs]  # ceil(num m / den) - 1
                at = torch.tensor(ranks, dtype=torch.int64, device="cuda")
                plan, wide = ops.Quantiles(len(qs)), ops.Quantiles(16)
                answers = {}

                def mine():
                    plan.launch(col, qs, rows=rows, signed=True)

                def sixteen():  # one rank sixteen times: the sixteen-slot kernel with one live slot
                    wide.launch(col, qs * 16, rows=rows, signed=True)

                def by_sort():
                    tmp.copy_(candidates())
                    sorter.launch(tmp, True)
                    answers["sort"] = tmp[at]

                def by_kthvalue():
                    c = candidates()
                    answers["kthvalue"] = torch.stack([torch.kthvalue(c, r + 1)[0] for r in ranks])

                legs_fn = {"quantile": mine, "sort": by_sort, "kthvalue": by_kthvalue}
                if len(qs) == 1:
                    legs_fn["sixteen-slot"] = sixteen
                    top = ops.TopK(m, ranks[0] + 1)

                    def by_topk():  # unsorted: the k-th key is the largest of the k it returns
                        answers["topk"] = top.launch(candidates(), signed=True, sorted=False)[0].max().reshape(1)

                    legs_fn["topk"] = by_topk
                mine()
                for leg in [x for x in legs_fn if x != "quantile"]:
                    try:
                        legs_fn[leg]()
                    except RuntimeError as e:  # a route this build of torch does not offer for the shape
                        print(f"{TAG:10s} quantile n=2^{lg} {shape} {set_name}: leg {leg} left out: {str(e).splitlines()[0]}", flush=True)
                        del legs_fn[leg]
                        answers.pop(leg, None)
                got = plan.result()[0].cuda()
                ok = all(torch.equal(got, a.to(torch.int64)) for a in answers.values())
                if len(qs) == 1:
                    ok = ok and torch.equal(wide.result()[0].cuda(), got.repeat(16))
                legs = {leg: [] for leg in legs_fn}
                slow = {leg for leg, fn in legs_fn.items() if times(fn, 1, warm=0)[0] > 20000.0}  # (torch.kthvalue on 2^24 rows up)
                for _ in range(reps):  # alternating; a leg of more than 20 ms a call is timed once per repetition
                    for leg, fn in legs_fn.items():
                        legs[leg].append(times(fn, 1, warm=0)[0] if leg in slow else median(times(fn, 5)))
                others =[x for x in legs if x not in ("quantile", "sixteen-slot")]
                best = min(others, key=lambda x: min(legs[x]))
                verdict = "HELD" if max(legs["quantile"]) <= min(legs[best]) else "MISSED"
                s = median(sorted(legs["quantile"]))
                extra = f"  floor {verdict} against {best} x{min(legs[best]) / s:7.2f}  three reads at 8 TB/s {3 * 4 * m / 8e6:7.1f} us"
                if "sixteen-slot" in legs:
                    extra += f"  sixteen-slot / quantile x{median(sorted(legs['sixteen-slot'])) / s:5.2f}"
                _merge_row(f"quantile n=2^{lg} {shape} {set_name}", legs, ok, None, None, extra)
                del plan, wide
            del col, rows, tmp, sorter, taker


def launch_sort_pairs(lg):
    n = 1 << (lg or 24)
    keys0 = ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    plan = ops.RadixSortPairs(n, 8)
    for _i in range(5):
        k = keys0.clone()
        plan.launch(k)
    torch.cuda.synchronize()
    print("ok" if ops.workspace_status(plan.ws) == 0 and ops.check_sorted_pairs(keys0, k, plan.perm[:n]) == (0, 0) else "WRONG")


def sort_only(_):
    n = 1 << 24
    keys0 = _shape_keys(n, SHAPES[int(os.environ.get("SORT_SHAPE", "0"))])
    keys = keys0.clone()
    plan = ops.RadixSort(n, int(os.environ.get("SORT_BITS", "8")))
    for _i in range(3):
        keys.copy_(keys0)
        plan.launch(keys)
    torch.cuda.synchronize()
    print("ok")


def groupby(_):
    n = 1 << 26
    res = []
    for groups in (1 << 16, 1 << 15, 1 << 10, 64):
        keys = ops.gen_uniform_u32(n, 42, 0, groups - 1)
        vals = ops.gen_uniform_u32(n, 43, 1, 10000)
        plan = ops.GroupBySum(n, groups)
        t = dropmax(times(lambda: plan.launch(keys, vals), 9))
        ref = torch.zeros(groups, dtype=torch.int64, device="cuda").index_add_(0, keys.to(torch.int64), vals.to(torch.int64))
        ok = bool(torch.equal(u64(plan.result()), ref & 0xFFFFFFFF))
        res.append(f"G={groups}: {t:6.1f} us {'ok' if ok else 'WRONG'}")
    print(f"{TAG:16s} " + "  ".join(res), flush=True)


def groupby_hash(_):
    """dbhip_groupby_hash_u32 (max_groups = the number of distinct keys) against groupby_sum on the dense draw the keys
    come from and against torch.unique(return_inverse, return_counts) + scatter_add (median of 7 / 7 / 3)"""
    def mixed(u):  # a bijective spread of [0, d) over the uint32 range: sparse keys
        return bits32((u.to(torch.int64) * 2654435761 + 12345) % 2**32)

    def composed(keys, vals):
        u, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
        return u, torch.zeros(len(u), dtype=torch.int64, device="cuda").scatter_add_(0, inv, u64(vals)), cnt

    for lg in (24, 26):
        n = 1 << lg
        vals = ops.gen_uniform_u32(n, 43, 1, 10000)
        cases = [(f"d={d}", d) for d in (1, 64, 4096, 1 << 16, 1 << 20) if d <= n] + [("all-distinct", n), ("hot-half", n)]
        if lg == 26:
            cases.append(("dense 2^16 (BASELINE)", 1 << 16))
        for name, d in cases:
            u = torch.arange(n, dtype=torch.int32, device="cuda") if d == n else ops.gen_uniform_u32(n, 42, 0, d - 1)
            keys = u if name.startswith("dense") else mixed(u)
            if name == "hot-half":
                keys = keys.clone()
                keys[ops.gen_uniform_u32(n, 7, 0, 1) == 0] = 777
            plan = ops.GroupByHash(n, d)
            t = median(times(lambda: plan.launch(keys, vals), 7))
            k, sm, c = plan.result()
            ru, rs, rc = composed(keys, vals)
            o, r = torch.argsort(u64(k)), torch.argsort(u64(ru))  # (torch.unique orders the int32 bits as signed)
            ok = (torch.equal(u64(k)[o], u64(ru)[r]) and torch.equal(u64(sm)[o], rs[r] & 0xFFFFFFFF)
                  and torch.equal(c[o].to(torch.int64), rc[r]))
            tt = median(times(lambda: composed(keys, vals), 3, warm=1))
            dense = ""
            if name != "hot-half" and d <= 1 << 20:  # (above, groupby_sum reads every row once per 32768 groups)
                gplan = ops.GroupBySum(n, d)
                td = median(times(lambda: gplan.launch(u, vals), 7))
                dense = f"  groupby_sum(dense draw) {td:8.1f} us"
            print(f"{TAG:10s} 2^{lg} {name:22s} groupby_hash {t:8.1f} us {'ok' if ok else 'WRONG'}  torch {tt:9.1f} us{dense}",
                  flush=True)
            del plan


def groupby_shapes(_):
    tag = "packed=" + os.environ.get("DBHIP_GB_PACKED", "auto")
    for lg, groups, hi in ((26, 65536, 10000), (27, 65536, 10000), (28, 65536, 10000), (26, 65536, 60000),
                           (26, 65536, 2**32 - 1), (26, 1 << 18, 10000), (27, 1 << 17, 10000), (24, 65536, 10000)):
        n = 1 << lg
        keys = ops.gen_uniform_u32(n, 42, 0, groups - 1)
        vals = ops.gen_uniform_u32(n, 43, 1, hi)
        plan = ops.GroupBySum(n, groups)
        t = median(times(lambda: plan.launch(keys, vals), 5))
        ref = torch.zeros(groups, dtype=torch.int64, device="cuda").index_add_(0, keys.to(torch.int64), vals.to(torch.int64))
        ok = bool(torch.equal(u64(plan.result()), ref & 0xFFFFFFFF))
        mode = int(plan.ws[4:8].view(torch.int32).item())
        print(f"{tag:12s} n=2^{lg} G={groups} vals<={hi}: {t:8.1f} us  mode {('-', 'packed', 'wide')[mode]}  {'ok' if ok else 'WRONG'}", flush=True)
        del keys, vals, plan


def _shape_keys(n, kind):
    g = torch.Generator(device="cuda").manual_seed(7)
    if kind == "uniform 32-bit":
        return ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    if kind == "[1, 10000]":
        return ops.gen_uniform_u32(n, 42, 1, 10000)
    if kind == "two values":
        return bits32(torch.randint(0, 2, (n,), device="cuda", generator=g, dtype=torch.int64) * 0xFFFFFFFF)
    if kind == "16 values":
        return bits32(torch.randint(0, 16, (n,), device="cuda", generator=g, dtype=torch.int64) * 0x11111111)
    if kind == "90 % one value":
        k = torch.randint(0, 2**32, (n,), device="cuda", generator=g, dtype=torch.int64)
        hot = torch.rand(n, device="cuda", generator=g) < 0.9
        return bits32(torch.where(hot, torch.full_like(k, 0x9E3779B9), k))
    if kind == "sorted":
        return bits32(torch.sort(u64(ops.gen_uniform_u32(n, 42, 0, 2**32 - 1))).values)
    if kind == "reversed":
        return bits32(torch.sort(u64(ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)), descending=True).values)
    if kind == "geometric":  # key = 2^32 * u^8: most keys small, every byte still varies
        u = torch.rand(n, device="cuda", generator=g, dtype=torch.float64)
        return bits32((u ** 8 * 4294967295.0).to(torch.int64))
    raise ValueError(kind)


SHAPES = ("uniform 32-bit", "[1, 10000]", "two values", "16 values", "90 % one value", "sorted", "reversed", "geometric")


def sort_shapes(lg):
    n = 1 << (lg or 24)
    for kind in SHAPES:
        keys0 = _shape_keys(n, kind)
        keys = keys0.clone()
        ref = torch.sort(u64(keys0)).values
        res = []
        for bits in (8, 4):
            plan = ops.RadixSort(n, bits)

            def run():
                keys.copy_(keys0)
                plan.launch(keys)

            t = median(times(run, 5)) - median(times(lambda: keys.copy_(keys0), 5))
            run()
            ok = bool(torch.equal(u64(keys), ref)) and ops.workspace_status(plan.ws) == 0
            res.append(f"{bits}-bit {t:8.1f} us {'ok' if ok else 'WRONG'}")
        print(f"{TAG:16s} 2^{lg or 24} {kind:16s}: " + "   ".join(res), flush=True)


def groupby_skew(_):
    n = 1 << 26
    for groups in (64, 1 << 10, 1 << 12, 1 << 14, 1 << 15, 1 << 16):
        for kind in ("uniform", "one group", "90 % one group", "16 groups", "sorted keys"):
            g = torch.Generator(device="cuda").manual_seed(7)
            keys = ops.gen_uniform_u32(n, 42, 0, groups - 1)
            if kind == "one group":
                keys = torch.full_like(keys, groups // 3)
            elif kind == "90 % one group":
                hot = torch.rand(n, device="cuda", generator=g) < 0.9
                keys = torch.where(hot, torch.full_like(keys, groups // 3), keys)
            elif kind == "16 groups":
                keys = bits32(u64(keys) % 16 * (groups // 16))
            elif kind == "sorted keys":
                keys = bits32(torch.sort(u64(keys)).values)
            vals = ops.gen_uniform_u32(n, 43, 1, 10000)
            plan = ops.GroupBySum(n, groups)
            t = median(times(lambda: plan.launch(keys, vals), 5))
            ref = torch.zeros(groups, dtype=torch.int64, device="cuda").index_add_(0, u64(keys), u64(vals))
            ok = bool(torch.equal(u64(plan.result()), ref & 0xFFFFFFFF))
            print(f"{TAG:16s} G={groups:6d} {kind:16s}: {t:9.1f} us {'ok' if ok else 'WRONG'}", flush=True)
            del keys, vals, plan


def join(lg):
    lg = lg or 26
    n = 1 << lg
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(n, 43, 0, n - 1)
    plan = ops.HashJoin(n, n)
    plan.build(build)
    plan.probe(probe)
    b = dropmax(times(lambda: plan.build(build), 7, warm=0))
    p = dropmax(times(lambda: plan.probe(probe), 7, warm=0))
    plan.result()
    total = int(plan.cnt.to(torch.int64).sum())
    del plan
    rj = ops.RadixJoin(n, n)

    def radix():
        rj.partition_build(build)
        rj.partition_probe(probe)
        rj.match()

    r = dropmax(times(radix, 7, warm=1))
    pb = dropmax(times(lambda: rj.partition_build(build), 7, warm=0))
    m = dropmax(times(rj.match, 7, warm=0))
    rj.result()
    ok = int(rj.cnt.to(torch.int64).sum()) == total
    print(f"{TAG:20s} 2^{lg}: build {b:8.1f} probe {p:8.1f} total {b + p:8.1f} us | radix join {r:8.1f} us "
          f"(partition one side {pb:7.1f}, match {m:7.1f}) matches {'equal' if ok else 'DIFFER'}", flush=True)


def radix(lg):
    """the radix join alone (no table in HBM): sizes up to 2^30 x 2^30 fit; the match count is printed so that variants
    can be compared with each other (at 2^26 it is checked against torch by `join`)"""
    lg = lg or 30
    n = 1 << lg
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(n, 43, 0, n - 1)
    rj = ops.RadixJoin(n, n)

    def run():
        rj.partition_build(build)
        rj.partition_probe(probe)
        rj.match()

    k = 5 if lg >= 29 else 7
    r = dropmax(times(run, k, warm=1))
    pb = dropmax(times(lambda: rj.partition_build(build), k, warm=0))
    m = dropmax(times(rj.match, k, warm=0))
    rj.result()
    total = int(rj.cnt.to(torch.int64).sum())
    ids_ok = int(rj.ids.to(torch.int64).sum()) == n * (n - 1) // 2  # the id buffer is a permutation of the build rows
    print(f"{TAG:20s} 2^{lg}: radix join {r:9.1f} us (partition one side {pb:8.1f}, match {m:8.1f}) matches {total} "
          f"ids {'a permutation sum' if ids_ok else 'WRONG'}", flush=True)


def radix_offsets(lg):
    """does the partition's time depend on WHERE its buffers lie?  One side of the radix join partitioned with the key
    column and the workspace at different byte offsets inside two larger allocations (the same kernels, the same data)"""
    lg = lg or 30
    n = 1 << lg
    rj = ops.RadixJoin(n, n)
    slack = 1 << 27
    big_ws = torch.empty(rj.ws_bytes + slack, dtype=torch.uint8, device="cuda")
    big_in = torch.empty(n + slack // 4, dtype=torch.int32, device="cuda")
    src = ops.gen_uniform_u32(n, 42, 0, n - 1)
    print(f"{TAG:12s} 2^{lg}: workspace {rj.ws_bytes / 2**30:.1f} GiB at {big_ws.data_ptr():#x}, keys at {big_in.data_ptr():#x}", flush=True)
    for in_off in (0, 4096, 1 << 20, (1 << 21) + (1 << 16), (1 << 26) + (1 << 13)):
        keys = big_in[in_off // 4: in_off // 4 + n]
        keys.copy_(src)
        row = []
        for ws_off in (0, 256, 4096, 1 << 16, 1 << 20, 1 << 21, (1 << 21) + 4096, 3 << 21, (1 << 25) + (1 << 12), (1 << 26) + (1 << 18)):
            rj.ws = big_ws[ws_off: ws_off + rj.ws_bytes]
            t = dropmax(times(lambda: rj.partition_build(keys), 4, warm=1))
            row.append(f"{t:8.1f}")
        print(f"{TAG:12s} keys +{in_off:9d} B | workspace +0, +256, +4K, +64K, +1M, +2M, +2M4K, +6M, +32M4K, +64M256K: {' '.join(row)}", flush=True)


def radix_alloc(lg):
    """the same radix join on buffers from torch's allocator and on buffers from plain hipMalloc calls in two orders (the
    C++ engine allocates that way): does the allocation decide the partition's time?"""
    import ctypes as C
    from dwarf_bench_amd import _capi
    lg = lg or 30
    n = 1 << lg
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    L = _capi.lib()
    ws_bytes = L.dbhip_join_radix_workspace_bytes(n, n)

    def raw(size):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), size) == 0
        return p.value

    def run(label, build, probe, ws, ids, rid, pos, cnt):
        st = ops._stream()
        assert L.dbhip_gen_uniform_u32(build, n, 42, 0, 0, n - 1, st) == 0
        assert L.dbhip_gen_uniform_u32(probe, n, 43, 0, 0, n - 1, st) == 0
        pb = lambda: _capi.check(L.dbhip_join_radix_partition_u32(0, build, None, n, n, n, ws, ws_bytes, st), "p")
        pp = lambda: _capi.check(L.dbhip_join_radix_partition_u32(1, probe, None, n, n, n, ws, ws_bytes, st), "p")
        mm = lambda: _capi.check(L.dbhip_join_radix_match_u32(n, n, ids, rid, pos, cnt, ws, ws_bytes, st), "m")

        def whole():
            pb(); pp(); mm()

        r = dropmax(times(whole, 4, warm=1))
        a = dropmax(times(pb, 4, warm=0))
        b = dropmax(times(pp, 4, warm=0))
        m = dropmax(times(mm, 4, warm=0))
        print(f"{TAG:12s} 2^{lg} {label:44s}: radix join {r:9.1f} us (build side {a:8.1f}, probe side {b:8.1f}, match {m:8.1f}) "
              f"ws at {ws:#x} keys at {build:#x} / {probe:#x}", flush=True)

    t = [ops.gen_uniform_u32(n, 42, 0, n - 1), ops.gen_uniform_u32(n, 43, 0, n - 1), torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")]
    t += [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4)]
    run("torch tensors", *[x.data_ptr() for x in t])
    del t
    torch.cuda.empty_cache()
    for label, order in (("hipMalloc: keys, keys, 512 B, workspace, out", "bpcwo"), ("hipMalloc: workspace first", "wbpco"),
                         ("hipMalloc: keys, keys, workspace, out (no small)", "bpwo")):
        got, ptrs = {}, []
        for ch in order:
            if ch == "o":
                for k in ("ids", "rid", "pos", "cnt"):
                    got[k] = raw(n * 4)
            else:
                got[ch] = raw({"b": n * 4, "p": n * 4, "c": 512, "w": ws_bytes}[ch])
        run(label, got["b"], got["p"], got["w"], got["ids"], got["rid"], got["pos"], got["cnt"])
        torch.cuda.synchronize()
        for v in got.values():
            hip.hipFree(v)


def radix_stream(lg):
    """the radix join on the null stream and on a created (non-blocking) stream, the kind the C++ engine launches on"""
    lg = lg or 30
    n = 1 << lg
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(n, 43, 0, n - 1)
    rj = ops.RadixJoin(n, n)

    def run():
        rj.partition_build(build)
        rj.partition_probe(probe)
        rj.match()

    torch.cuda.synchronize()
    for label, stream in (("null stream", None), ("created stream", torch.cuda.Stream()), ("null stream again", None),
                          ("created stream again", torch.cuda.Stream())):
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream())
        with ctx:
            r = dropmax(times(run, 5, warm=1))
            pb = dropmax(times(lambda: rj.partition_build(build), 5, warm=0))
            pp = dropmax(times(lambda: rj.partition_probe(probe), 5, warm=0))
            m = dropmax(times(rj.match, 5, warm=0))
        torch.cuda.synchronize()
        print(f"{TAG:12s} 2^{lg} {label:22s}: radix join {r:9.1f} us (build side {pb:8.1f}, probe side {pp:8.1f}, match {m:8.1f})", flush=True)


def radix_idle(lg):
    """what an idle GPU costs the next join: the radix join timed after the device sat idle for a given time (events
    around each phase of ONE join; 4 joins per gap, the mean)"""
    import time
    lg = lg or 30
    n = 1 << lg
    build = ops.gen_uniform_u32(n, 42, 0, n - 1)
    probe = ops.gen_uniform_u32(n, 43, 0, n - 1)
    rj = ops.RadixJoin(n, n)
    rj.partition_build(build); rj.partition_probe(probe); rj.match()
    torch.cuda.synchronize()
    for gap in (0.0, 0.0005, 0.002, 0.01, 0.05, 0.25, 1.0, 0.0):
        acc = [0.0, 0.0, 0.0]
        for _ in range(4):
            torch.cuda.synchronize()
            time.sleep(gap)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(); rj.partition_build(build); ev[1].record(); rj.partition_probe(probe); ev[2].record(); rj.match(); ev[3].record()
            torch.cuda.synchronize()
            for i in range(3):
                acc[i] += ev[i].elapsed_time(ev[i + 1]) * 1e3 / 4
        print(f"{TAG:12s} 2^{lg} idle {gap * 1e3:7.1f} ms before: radix join {sum(acc):9.1f} us (build side {acc[0]:8.1f}, probe side {acc[1]:8.1f}, match {acc[2]:8.1f})", flush=True)


def ramp(_):
    """how long after an idle period do the dwarfs run slower?  Each dwarf: 100 ms idle, then back-to-back steps with an
    event between every two; the mean step time over windows of the sequence"""
    import time
    n = 1 << 28
    src = ops.gen_uniform_u32(n, 42, 1, 10000)
    scan_plan = ops.CopyIfLt(n)
    gk = ops.gen_uniform_u32(1 << 26, 42, 0, 65535)
    gv = ops.gen_uniform_u32(1 << 26, 43, 1, 10000)
    gb = ops.GroupBySum(1 << 26, 1 << 16)
    k0 = ops.gen_uniform_u32(1 << 24, 42, 0, 2**32 - 1)
    keys = k0.clone()
    sp = ops.RadixSort(1 << 24, 8)

    def sort_step():
        keys.copy_(k0)
        sp.launch(keys)

    for name, fn, steps in (("scan 2^28", lambda: scan_plan.launch(src, 5), 600), ("group-by 2^26", lambda: gb.launch(gk, gv), 600),
                            ("sort 2^24 (+ copy)", sort_step, 400)):
        fn()
        for idle in (0.1, 0.0):
            torch.cuda.synchronize()
            time.sleep(idle)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ev[0].record()
            for i in range(steps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            t = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(steps)]
            cum = [ev[0].elapsed_time(ev[i + 1]) for i in range(steps)]
            wins = [(0, 5), (5, 25), (25, 50), (50, 100), (100, 200), (200, 400), (400, steps)]
            row = "  ".join(f"[{a}:{b}) {sum(t[a:b]) / (b - a):6.1f}" for a, b in wins if b <= steps and a < b)
            print(f"{TAG:12s} {name:20s} after {idle * 1e3:5.0f} ms idle, us per step: {row}   (step 25 ends at {cum[24]:.1f} ms, step 100 at {cum[99]:.1f} ms)", flush=True)


def radix_sizes(_):
    """the radix join at sizes between the powers of two (2^25 .. 2^30): ns per row should move smoothly — a row that
    costs much more than its neighbours is a geometry step (level fan-outs and tile shapes follow the partition count)"""
    for lg in (25, 26, 27, 28, 29):
        for num in (4, 5, 6, 7):
            n = (num << lg) // 4
            build = ops.gen_uniform_u32(n, 42, 0, n - 1)
            probe = ops.gen_uniform_u32(n, 43, 0, n - 1)
            rj = ops.RadixJoin(n, n)

            def run():
                rj.partition_build(build)
                rj.partition_probe(probe)
                rj.match()

            r = dropmax(times(run, 5, warm=1))
            pb = dropmax(times(lambda: rj.partition_build(build), 5, warm=0))
            rj.result()
            ok = int(rj.ids.to(torch.int64).sum()) == n * (n - 1) // 2
            print(f"{TAG:12s} n = {num}/4 * 2^{lg} = {n:11d}: radix join {r:9.1f} us  {r * 1e3 / n:6.3f} ns/row  (partition one side "
                  f"{pb:8.1f} us) {'ok' if ok else 'WRONG'}", flush=True)
            del build, probe, rj
            torch.cuda.empty_cache()


def _matches(build, probe):
    """number of (build row, probe row) pairs with equal keys, by torch"""
    bk, bc = torch.unique(u64(build), return_counts=True)
    pk, pc = torch.unique(u64(probe), return_counts=True)
    at = torch.searchsorted(bk, pk).clamp(max=bk.numel() - 1)
    hit = bk[at] == pk
    return int((bc[at][hit] * pc[hit]).sum())


def join_skew(lg):
    lg = lg or 26
    n = 1 << lg
    g = torch.Generator(device="cuda").manual_seed(7)
    uni_b, uni_p = ops.gen_uniform_u32(n, 42, 0, n - 1), ops.gen_uniform_u32(n, 43, 0, n - 1)
    hot = torch.rand(n, device="cuda", generator=g) < 0.5

    def shapes():
        yield "uniform", uni_b, uni_p
        yield "half the build rows one key", torch.where(hot, torch.full_like(uni_b, 12345), uni_b), uni_p
        yield "half the probe rows one key", uni_b, torch.where(hot, torch.full_like(uni_p, 12345), uni_p)
        yield "keys are multiples of 65536", bits32(u64(uni_b) % 1024 * 65536), bits32(u64(uni_p) % 2048 * 65536)
        yield "keys are multiples of 1024", bits32(u64(uni_b) % 65536 * 1024), bits32(u64(uni_p) % 65536 * 1024)
        yield "sorted", bits32(torch.sort(u64(uni_b)).values), bits32(torch.sort(u64(uni_p)).values)
        yield "1024 distinct keys on the build side", bits32(u64(uni_b) % 1024), uni_p
        yield "both sides in [1, 10000] (reference)", ops.gen_uniform_u32(n, 42, 1, 10000), ops.gen_uniform_u32(n, 43, 1, 10000)
        yield "both sides in [0, 2^15)", bits32(u64(uni_b) % 32768), bits32(u64(uni_p) % 32768)

    for kind, build, probe in shapes():
        plan = ops.HashJoin(n, n)
        plan.build(build)
        plan.probe(probe)
        b = median(times(lambda: plan.build(build), 3, warm=0))
        p = median(times(lambda: plan.probe(probe), 3, warm=0))
        plan.result()
        total = int(plan.cnt.to(torch.int64).sum())
        del plan
        rj = ops.RadixJoin(n, n)

        def radix():
            rj.partition_build(build)
            rj.partition_probe(probe)
            rj.match()

        r = median(times(radix, 3, warm=1))
        rj.result()
        ok = int(rj.cnt.to(torch.int64).sum()) == total == _matches(build, probe)
        del rj
        print(f"{TAG:16s} 2^{lg} {kind:38s}: build {b:9.1f} probe {p:9.1f} | radix join {r:9.1f} us  matches {'equal' if ok else 'DIFFER'}", flush=True)


def size_sweep(_):
    """every dwarf over sizes next to and between powers of two (median of 5): a row that costs much more per element
    than its neighbours is a geometry cliff"""
    def line(name, n, us):
        print(f"{TAG:12s} {name:28s} n={n:10d}: {us:9.1f} us  {us * 1e3 / max(n, 1):8.3f} ns/row", flush=True)

    for lg in (13, 14, 16, 18, 20, 22, 24, 26):
        for n in ((1 << lg) - 1, 1 << lg, (1 << lg) + 1, 3 << (lg - 1)):
            src = ops.gen_uniform_u32(n, 42, 1, 10000)
            plan = ops.CopyIfLt(n)
            line("scan x<5", n, median(times(lambda: plan.launch(src, 5), 5)))
            line("scan x<5001 dense", n, median(times(lambda: plan.launch(src, 5001, dense=True), 5)))
            keys0 = ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
            keys = keys0.clone()
            cp = median(times(lambda: keys.copy_(keys0), 5))
            for bits in (8, 4):
                sp = ops.RadixSort(n, bits)

                def run():
                    keys.copy_(keys0)
                    sp.launch(keys)

                line(f"sort {bits}-bit", n, median(times(run, 5)) - cp)
            for groups in (1000, 32768, 32769, 65536, 65537):
                gk = ops.gen_uniform_u32(n, 42, 0, groups - 1)
                gp = ops.GroupBySum(n, groups)
                line(f"groupby G={groups}", n, median(times(lambda: gp.launch(gk, src), 5)))
                del gk, gp
            b = ops.gen_uniform_u32(n, 42, 0, n - 1)
            jp = ops.HashJoin(n, n)
            line("join build", n, median(times(lambda: jp.build(b), 3)))
            line("join probe", n, median(times(lambda: jp.probe(keys0), 3)))
            del jp, b, src, plan, keys0, keys
            torch.cuda.empty_cache()


def partition(_):
    n = 1 << 27
    keys = ops.gen_uniform_u32(n, 42, 0, (1 << 30) - 1)
    for parts in (2, 4, 8, 16, 64, 256):
        t = median(times(lambda: ops.partition_by_hash(keys, 0, parts), 5, warm=1))
        print(f"{TAG:12s} 2^27 rows -> {parts:4d} buckets: {t:8.1f} us (incl. output allocation)", flush=True)


def reduce(_):
    n = 1 << 28
    src = ops.gen_uniform_u32(n, 42, 1, 10000)
    want = int(src.sum(dtype=torch.int64)) & 0xFFFFFFFF
    t = median(times(lambda: ops.reduce_sum(src), 15, warm=3))
    got = int(ops.reduce_sum(src)) & 0xFFFFFFFF
    print(f"{TAG:12s} wgs={os.environ.get('DBHIP_RED_WGS', '-')}: {t:7.1f} us ({4 * n / t / 8e6 * 100:4.1f} %) "
          f"{'ok' if got == want else 'WRONG'}", flush=True)


def cuckoo(lg):
    lg = lg or 24
    n = 1 << lg
    keys = ops.gen_unique_sorted_u32(n, 11)
    absent = bits32(u64(keys) - u64(keys) % 10 + (u64(keys) % 10 + 1) % 10)  # same decade, another digit: never generated
    t = ops.CuckooTable(4 * n, 2, ops.cuckoo_seed_pair(0, 0))  # the dwarf's hasher pair
    t.insert(keys, keys)
    if t.failed():
        raise SystemExit(f"{TAG}: the first seed pair failed at 2^{lg}")
    r = median(times(t.reset, 9))

    def build():
        t.reset()
        t.insert(keys, keys)

    b = median(times(build, 9))
    if t.failed():
        raise SystemExit(f"{TAG}: a timed build failed at 2^{lg}")
    vals, found = t.lookup(keys)
    ok = bool((found == 1).all()) and torch.equal(vals, keys)
    lp = median(times(lambda: t.lookup(keys), 9))
    vals, found = t.lookup(absent)
    ok = ok and not bool(found.any()) and not bool(vals.any())
    la = median(times(lambda: t.lookup(absent), 9))
    print(f"{TAG:20s} 2^{lg} keys, {4 * n} slots: reset {r:8.1f} us, reset + insert {b:8.1f} us (insert {b - r:8.1f} us, "
          f"{n / (b - r) / 1e3:6.2f} G keys/s) | lookup present {lp:8.1f} us ({n / lp / 1e3:6.2f} G/s), absent {la:8.1f} us "
          f"({n / la / 1e3:6.2f} G/s) | {'ok' if ok else 'WRONG'}", flush=True)


def slab(lg):
    lg = lg or 24
    n = 1 << lg
    uniq = ops.gen_unique_sorted_u32(n, 11)
    absent = bits32(u64(uniq) - u64(uniq) % 10 + (u64(uniq) % 10 + 1) % 10)  # same decade, another digit: never generated
    ref = ops.gen_uniform_u32(n, 21, 1, 10000)
    one = torch.full((n >> 8,), 77, dtype=torch.int32, device="cuda")
    cases = [("unique", uniq, None), ("keys 1..10000", ref, None), ("one key", one, (n >> 8) // 32 + ops.SLAB_MAX_GROUPS)]
    for hint, spread in (("1", ""), ("0", ""), ("1", "0"), ("1", "1")):
        os.environ["DBHIP_SLAB_HINT"], os.environ["DBHIP_SLAB_SPREAD"] = hint, spread
        for name, keys, pool in cases:
            m = keys.numel()
            b = ops.slab_buckets(m)
            t = ops.SlabTable(b, pool if pool is not None else b + ops.SLAB_MAX_GROUPS)
            r = median(times(t.reset, 9))

            def build():
                t.reset()
                t.insert(keys, keys)

            bt = median(times(build, 9))
            vals, found = t.lookup(keys)
            ok = t.status() == ops.DEV_OK and bool((found == 1).all()) and torch.equal(vals, keys)
            line = (f"{TAG:12s} hint={hint} spread={spread} {name:14s} {m:9d} rows: reset {r:8.1f} us, insert {bt - r:9.1f} us "
                    f"({m / max(bt - r, 1e-3) / 1e3:6.2f} G rows/s)")
            if keys is uniq:
                lp = median(times(lambda: t.lookup(uniq), 9))
                av, af = t.lookup(absent)
                ok = ok and not bool(af.any()) and not bool(av.any())
                la = median(times(lambda: t.lookup(absent), 9))
                line += f" | lookup present {lp:8.1f} us ({m / lp / 1e3:6.2f} G/s), absent {la:8.1f} us ({m / la / 1e3:6.2f} G/s)"
            elif keys is ref:
                lr = median(times(lambda: t.lookup(ref), 9))
                line += f" | lookup {lr:8.1f} us"
            print(line + f" | {'ok' if ok else 'WRONG'}", flush=True)
    os.environ.pop("DBHIP_SLAB_HINT")
    os.environ.pop("DBHIP_SLAB_SPREAD")


def xscan(lg):
    lg = lg or 28
    n = 1 << lg
    base = ops.gen_uniform_u32(n + 4, 42, 0, 1000)
    outb = torch.empty(n + 4, dtype=torch.int32, device="cuda")
    for off in (0, 1):
        src, out = base[off: off + n], outb[off: off + n]
        plan = ops.ExclusiveScan(n)
        t = median(times(lambda: plan.launch(src, out=out), 9))
        plan.result()
        m = min(n - 1, 1 << 20)
        ref = torch.cumsum(src[:m].to(torch.int64), 0)
        ok = bool(torch.equal(u64(out[1:m + 1]), ref & 0xFFFFFFFF)) and int(out[0]) == 0
        print(f"{TAG:12s} 2^{lg} offset {off}: {t:8.1f} us  ({8 * n / t / 8e6 * 100:4.1f} % of 8 TB/s on 8n bytes)  "
              f"{'ok' if ok else 'WRONG'}", flush=True)


def graph(only):
    import time

    def wall(fn, iters=200):
        for _i in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _i in range(iters):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    def captured(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    for lg in ([only] if only else (14, 16, 18, 20)):
        n = 1 << lg
        keys = ops.gen_uniform_u32(n, 1, 0, 2**32 - 1)
        plan = ops.RadixSort(n, 8)
        direct = wall(lambda: plan.launch(keys))
        replay = wall(captured(lambda: plan.launch(keys)).replay)
        b, p = ops.gen_uniform_u32(n, 2, 0, n - 1), ops.gen_uniform_u32(n, 3, 0, n - 1)
        j = ops.HashJoin(n, n)

        def both():
            j.build(b)
            j.probe(p)

        jd = wall(both)
        jg = wall(captured(both).replay)
        print(f"n=2^{lg}: sort direct {direct:.1f} us  graph {replay:.1f} us | join direct {jd:.1f} us  graph {jg:.1f} us", flush=True)


def launch_join(lg):
    n = 1 << (lg or 26)
    build, probe = ops.gen_uniform_u32(n, 42, 0, n - 1), ops.gen_uniform_u32(n, 43, 0, n - 1)
    hot = os.environ.get("JOIN_HOT", "")  # build | probe: every other row of that side carries one key; few: 1024 distinct build keys
    if hot == "build":
        build[::2] = 12345
    if hot == "probe":
        probe[::2] = 12345
    if hot == "few":  # 1024 distinct build keys
        build = bits32(u64(build) % 1024)
    plan = ops.HashJoin(n, n)
    for _i in range(5):
        plan.build(build)
        plan.probe(probe)
    torch.cuda.synchronize()
    plan.result()
    if os.environ.get("JOIN_RADIX"):
        rj = ops.RadixJoin(n, n)
        for _i in range(3):
            rj.partition_build(build)
            rj.partition_probe(probe)
            rj.match()
        rj.result()
    print("ok")


def launch_sort(lg):
    n = 1 << (lg or 24)
    keys0 = ops.gen_uniform_u32(n, 42, 0, 2**32 - 1)
    for bits in (8, 4):
        plan = ops.RadixSort(n, bits)
        for _i in range(5):
            k = keys0.clone()
            plan.launch(k)
    torch.cuda.synchronize()
    print("ok")


def launch_all(_):
    """a few calls of every BASELINE configuration (SQ counters per kernel)"""
    n = 1 << 28
    src = ops.gen_uniform_u32(n, 42, 1, 10000)
    sc = ops.CopyIfLt(n)
    for filt in (5, 5, 5001, 5001):
        sc.launch(src, filt, dense=filt > 1000)
    del src, sc
    launch_sort(24)
    n = 1 << 26
    keys, vals = ops.gen_uniform_u32(n, 42, 0, 65535), ops.gen_uniform_u32(n, 43, 1, 10000)
    gb = ops.GroupBySum(n, 1 << 16)
    for _i in range(3):
        gb.launch(keys, vals)
    torch.cuda.synchronize()
    print("ok")


MODES = {"radix": radix, "ramp": ramp, "radix-idle": radix_idle, "radix-stream": radix_stream, "radix-alloc": radix_alloc, "radix-offsets": radix_offsets, "radix-sizes": radix_sizes, "graph": graph, "launch-join": launch_join, "launch-sort": launch_sort, "launch-all": launch_all, "scan": scan, "sort": sort, "sort-only": sort_only, "groupby": groupby, "groupby-shapes": groupby_shapes, "groupby-skew": groupby_skew, "sort-shapes": sort_shapes, "join": join, "join-skew": join_skew, "size-sweep": size_sweep, "partition": partition,
         "reduce": reduce, "xscan": xscan, "cuckoo": cuckoo, "slab": slab,
         "groupby-hash": groupby_hash, "sort-pairs": sort_pairs, "launch-sort-pairs": launch_sort_pairs,
         "join-pairs": join_pairs, "launch-join-pairs": launch_join_pairs, "topk": topk, "launch-topk": launch_topk,
         "groupby-sorted": groupby_sorted, "launch-groupby-sorted": launch_groupby_sorted,
         "window": window, "launch-window": launch_window, "sorted-search": sorted_search, "range-join": range_join,
         "selection": selection, "merge": merge, "take": take, "dict": dict_encoding, "bitpack": bitpack, "bloom": bloom, "hll": hll,
         "quantile": quantile}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in MODES:
        raise SystemExit(__doc__)
    MODES[sys.argv[1]](int(sys.argv[2]) if len(sys.argv) > 2 else None)
