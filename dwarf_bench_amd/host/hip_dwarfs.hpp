// hip_dwarfs.hpp — the `...Hip` Dwarf subclasses: C++ host code behind the reference's Dwarf::run() hook
// (common/dwarf.hpp:15-16) that drives the hand-written gfx950 kernels through the C ABI of
// include/dbhip.h.  One class per reference dwarf on the hot path:
//   TwoPassScanHip / DPLScanHip   scan/scan.cpp:22-195, scan/dplscan.cpp:22-92
//   RadixHip                      sort/radix.cpp:17-80
//   GroupByHip                    groupby/groupby.cpp:24-122
//   JoinOmnisciHip                join/join_omnisci.cpp:49-118
//   JoinHip                       join/join.cpp:8-154
//   GroupByLocalHip, HashBuildHip, HashBuildNonBitmaskHip, ProbeHip: the "next" rows of SURVEY 8(f)
#pragma once
#include "dwarf_api.hpp"

// The frame of every `...Hip` dwarf: run() prints the device banner and calls _run once per input size, init() hands
// the options to the meter and records the device type.  A dwarf supplies its name and _run.
class HipDwarf : public Dwarf {
 public:
  explicit HipDwarf(const std::string &name) : Dwarf(name) {}
  void run(const RunOptions &opts) override;
  void init(const RunOptions &opts) override;

 private:
  virtual void _run(size_t buf_size, Meter &meter) = 0;
};

struct TwoPassScanHip : HipDwarf {
  TwoPassScanHip() : HipDwarf("TwoPassScanHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct DPLScanHip : HipDwarf {
  DPLScanHip() : HipDwarf("DPLScanHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct RadixHip : HipDwarf {
  explicit RadixHip(const std::string &name = "RadixHip") : HipDwarf(name) {}
  void init(const RunOptions &opts) override;  // HipDwarf::init, then dbhip_radix_sort_prepare
  void _run(size_t buf_size, Meter &meter) override;
  static int digit_bits();  // DWARF_BENCH_RADIX_BITS: 4, anything else the tuned 8
};
struct GroupByHip : HipDwarf {
  GroupByHip() : HipDwarf("GroupByHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct JoinOmnisciHip : HipDwarf {
  JoinOmnisciHip() : HipDwarf("JoinOmnisciHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct JoinHip : HipDwarf {
  JoinHip() : HipDwarf("JoinHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct PartitionedJoinHip : HipDwarf {  // radix-partitioned join over --gpus ranks, RCCL exchange
  PartitionedJoinHip() : HipDwarf("PartitionedJoinHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// SURVEY 8(f) "next" rows
struct GroupByLocalHip : HipDwarf {  // groupby/groupby_local.cpp:24-142 (two-phase timings, --executors)
  GroupByLocalHip();
  void _run(size_t buf_size, Meter &meter) override;
};
struct HashBuildHip : HipDwarf {  // hash/hash_build.cpp:8-98 (bitmask-claimed table, build only)
  HashBuildHip() : HipDwarf("HashBuildHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct HashBuildNonBitmaskHip : HipDwarf {  // hash/hash_build_non_bitmask.cpp:7-91 (CAS table, build only)
  HashBuildNonBitmaskHip() : HipDwarf("HashBuildNonBitmaskHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct ProbeHip : HipDwarf {  // probe/slab_probe.cpp:9-107 (table built untimed, lookups timed)
  ProbeHip() : HipDwarf("ProbeHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct ReduceHip : HipDwarf {  // reduce/reduce.cpp:27-98 (int sum)
  ReduceHip() : HipDwarf("ReduceHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct NestedLoopJoinHip : HipDwarf {  // join/nested_join.cpp:10-110 (dense cell matrix, small n)
  NestedLoopJoinHip() : HipDwarf("NestedLoopJoinHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// the reference's EXPERIMENTAL block: registered by the set "experimental" only (register_dwarfs.cpp kDwarfSets)
struct CuckooHashBuildHip : HipDwarf {  // hash/cuckoo_hash_build.cpp:8-134 (lock-free cuckoo table, rebuild on failure)
  CuckooHashBuildHip() : HipDwarf("CuckooHashBuildHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// the reference's EXPERIMENTAL slab dwarfs: registered by the set "slab" only
struct SlabHashBuildHip : HipDwarf {  // hash/slab_hash_build.cpp:9-108 (lock-free slab table, insert timed)
  SlabHashBuildHip() : HipDwarf("SlabHashBuildHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct SlabProbeHip : HipDwarf {  // probe/slab_probe.cpp:9-107 (slab table built untimed, lookups timed)
  SlabProbeHip() : HipDwarf("SlabProbeHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
struct SlabJoinHip : HipDwarf {  // join/slab_join.cpp:10-144 (build and probe timed separately)
  SlabJoinHip() : HipDwarf("SlabJoinHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// group-by on arbitrary 32-bit keys (SUM and COUNT): registered by the set "groupby_hash" only
struct GroupByHashHip : HipDwarf {  // groupby/groupby.cpp:58-93 (the hash table keyed by the group key)
  GroupByHashHip() : HipDwarf("GroupByHashHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// the argsort (key-value radix sort with row ids as values): registered by the set "sort_pairs" only; no
// reference counterpart, the reference sorts keys only
struct RadixPairsHip : RadixHip {  // RadixHip's init and digit width
  RadixPairsHip() : RadixHip("RadixPairsHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// the join result as a table of (build row, probe row) pairs (radix join + dbhip_join_pairs_u32): registered by
// the set "join_pairs" only; no reference counterpart, JoinOmnisci stops at the per-row {pointer, size} record
struct JoinPairsHip : HipDwarf {
  JoinPairsHip() : HipDwarf("JoinPairsHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// ORDER BY key LIMIT k (dbhip_topk_i32, include/dbhip_topk.h): registered by the set "topk" only; no
// reference counterpart.  k: DWARF_BENCH_TOPK_K (default 1024, clipped to the row count),
// DWARF_BENCH_TOPK_LARGEST=1: the largest keys
struct TopKHip : HipDwarf {
  TopKHip() : HipDwarf("TopKHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// GROUP BY key ORDER BY key with COUNT, 64-bit SUM, MIN, MAX: the stable pairs sort and dbhip_reduce_by_key_u32
// (include/dbhip_reduce_by_key.h); registered by the set "groupby_sorted" only; no reference counterpart.
// --groups_count as GroupByHashHip
struct GroupBySortedHip : HipDwarf {
  GroupBySortedHip() : HipDwarf("GroupBySortedHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// ROW_NUMBER, running 64-bit SUM, MIN, MAX and the run number per row over PARTITION BY key ORDER BY row: the stable pairs
// sort and dbhip_scan_by_key_u32 (include/dbhip_scan_by_key.h); registered by the set "window" only; no reference
// counterpart.  --groups_count as GroupByHashHip
struct WindowSortedHip : HipDwarf {
  WindowSortedHip() : HipDwarf("WindowSortedHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
// The band join b.key BETWEEN p.lo AND p.hi as (build row, probe row) pairs: the stable pairs sort, the sorted search of
// include/dbhip_sorted_search.h and dbhip_join_pairs_u32; registered by the set "range_join" only; no reference
// counterpart.  DWARF_BENCH_RANGE_WIDTH: hi - lo (default 2)
struct RangeJoinHip : HipDwarf {
  RangeJoinHip() : HipDwarf("RangeJoinHip") {}
  void _run(size_t buf_size, Meter &meter) override;
};
