// register_dwarfs.cpp — populate_registry() (reference: register_dwarfs.cpp:20-56).  The reference
// registers its dwarfs under EXPERIMENTAL / DPCPP_ENABLED / CUDA_ENABLED guards; this build has one
// guard, HIP_ENABLED, and registers the hand-written gfx950 dwarfs — plus, unguarded, the two HOST dwarfs of the hot
// path under the reference's own names (cpu_dwarfs.cpp: TwoPassScan for --device=cpu, TBBSort).
// populate_experimental_registry() is the reference's `#ifdef EXPERIMENTAL` block (:41-47): only the
// dwarf_bench_experimental CLI (main.cpp built with -DEXPERIMENTAL) calls it.
#include "cpu_dwarfs.hpp"
#include "dwarf_api.hpp"
#include "hip_dwarfs.hpp"

void populate_registry() {
  Registry *registry = Registry::instance();
  registry->registerd(new TwoPassScan());  // scan/scan.cpp:22-195 (register_dwarfs.cpp:24 in the reference)
  registry->registerd(new TBBSort());      // sort/tbbsort.cpp:15-48
#ifdef HIP_ENABLED
  registry->registerd(new TwoPassScanHip());
  registry->registerd(new DPLScanHip());
  registry->registerd(new RadixHip());
  registry->registerd(new GroupByHip());
  registry->registerd(new JoinOmnisciHip());
  registry->registerd(new JoinHip());
  registry->registerd(new PartitionedJoinHip());
  registry->registerd(new GroupByLocalHip());
  registry->registerd(new HashBuildHip());
  registry->registerd(new HashBuildNonBitmaskHip());
  registry->registerd(new ProbeHip());
  registry->registerd(new ReduceHip());
  registry->registerd(new NestedLoopJoinHip());
#endif
}

void populate_experimental_registry() {
#ifdef HIP_ENABLED
  Registry *registry = Registry::instance();
  registry->registerd(new CuckooHashBuildHip());  // hash/cuckoo_hash_build.cpp (register_dwarfs.cpp:44 in the reference)
#endif
}

// the reference's SlabHashBuild, SlabJoin and SlabProbe (register_dwarfs.cpp:44-46): only the dwarf_bench_slab CLI (main.cpp
// built with -DEXPERIMENTAL_SLAB) calls this, so the lists of dwarf_bench and dwarf_bench_experimental stay as they are
void populate_slab_registry() {
#ifdef HIP_ENABLED
  Registry *registry = Registry::instance();
  registry->registerd(new SlabHashBuildHip());  // hash/slab_hash_build.cpp
  registry->registerd(new SlabJoinHip());       // join/slab_join.cpp
  registry->registerd(new SlabProbeHip());      // probe/slab_probe.cpp
#endif
}

// the general group-by (dbhip_groupby_hash_u32): only the dwarf_bench_groupby_hash CLI (main.cpp built with
// -DEXPERIMENTAL_GROUPBY_HASH) calls this, so the lists of the other three CLIs stay as they are
void populate_groupby_hash_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new GroupByHashHip());
#endif
}

// the key-value sort's argsort (dbhip_radix_sort_pairs_i32): only the dwarf_bench_sort_pairs CLI (main.cpp built with
// -DEXPERIMENTAL_SORT_PAIRS) calls this, so the lists of the other four CLIs stay as they are
void populate_sort_pairs_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new RadixPairsHip());
#endif
}

// the join's pair table (dbhip_join_pairs_u32): only the dwarf_bench_join_pairs CLI (main.cpp built with
// -DEXPERIMENTAL_JOIN_PAIRS) calls this, so the lists of the other five CLIs stay as they are
void populate_join_pairs_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new JoinPairsHip());
#endif
}

// the top-k (dbhip_topk_i32): only the dwarf_bench_topk CLI (main.cpp built with -DEXPERIMENTAL_TOPK) calls this, so the
// lists of the other six CLIs stay as they are
void populate_topk_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new TopKHip());
#endif
}

// the sort-based group-by (dbhip_radix_sort_pairs_u32 + dbhip_reduce_by_key_u32): only the dwarf_bench_groupby_sorted CLI
// (main.cpp built with -DEXPERIMENTAL_GROUPBY_SORTED) calls this, so the lists of the other seven CLIs stay as they are
void populate_groupby_sorted_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new GroupBySortedHip());
#endif
}

// the window functions (dbhip_radix_sort_pairs_u32 + dbhip_scan_by_key_u32): only the dwarf_bench_window CLI (main.cpp built
// with -DEXPERIMENTAL_WINDOW) calls this, so the lists of the other eight CLIs stay as they are
void populate_window_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new WindowSortedHip());
#endif
}

// the range join (dbhip_radix_sort_pairs_u32 + the sorted search + dbhip_join_pairs_u32): only the dwarf_bench_range_join CLI
// (main.cpp built with -DEXPERIMENTAL_RANGE_JOIN) calls this, so the lists of the other nine CLIs stay as they are
void populate_range_join_registry() {
#ifdef HIP_ENABLED
  Registry::instance()->registerd(new RangeJoinHip());
#endif
}
