// register_dwarfs.cpp — populate_registry() (reference: register_dwarfs.cpp:20-56).  The reference
// registers its dwarfs under EXPERIMENTAL / DPCPP_ENABLED / CUDA_ENABLED guards; this build has one
// guard, HIP_ENABLED, and registers the hand-written gfx950 dwarfs — plus, unguarded, the two HOST dwarfs of the hot
// path under the reference's own names (cpu_dwarfs.cpp: TwoPassScan for --device=cpu, TBBSort).
// The dwarfs beyond that list come in named sets, kDwarfSets below: the dwarf_bench_<set> CLI is main.cpp built with
// -DDWARF_BENCH_SET="<set>" and registers the default list plus the rows of its set, so `dwarf_bench list` and
// DwarfBench::makeMeasurements stay what they are in the reference.
#include "cpu_dwarfs.hpp"
#include "dwarf_api.hpp"
#include "hip_dwarfs.hpp"

#include <vector>

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

namespace {
template <class T>
Dwarf *make() {
  return new T();
}
struct SetRow {
  const char *set;
  Dwarf *(*make)();
};
// set name (the CLI's suffix, a word of SETS in the Makefile) -> a dwarf it registers; one set per dwarf
const std::vector<SetRow> kDwarfSets = {
#ifdef HIP_ENABLED
    {"experimental", make<CuckooHashBuildHip>},  // hash/cuckoo_hash_build.cpp, the reference's EXPERIMENTAL block (:41-47)
    {"slab", make<SlabHashBuildHip>},            // hash/slab_hash_build.cpp (:44-46 in the reference, with the next two)
    {"slab", make<SlabJoinHip>},                 // join/slab_join.cpp
    {"slab", make<SlabProbeHip>},                // probe/slab_probe.cpp
    {"groupby_hash", make<GroupByHashHip>},      // group-by on arbitrary 32-bit keys (dbhip_groupby_hash_u32)
    {"sort_pairs", make<RadixPairsHip>},         // the key-value sort's argsort (dbhip_radix_sort_pairs_i32)
    {"join_pairs", make<JoinPairsHip>},          // the join's pair table (dbhip_join_pairs_u32)
    {"topk", make<TopKHip>},                     // ORDER BY key LIMIT k (dbhip_topk_i32)
    {"groupby_sorted", make<GroupBySortedHip>},  // pairs sort + dbhip_reduce_by_key_u32
    {"window", make<WindowSortedHip>},           // pairs sort + dbhip_scan_by_key_u32
    {"range_join", make<RangeJoinHip>},          // pairs sort + the sorted search + dbhip_join_pairs_u32
#endif
};
}  // namespace

bool populate_dwarf_set(const std::string &set) {
  bool known = false;
  for (const SetRow &row : kDwarfSets) {
    if (set != row.set) continue;
    Registry::instance()->registerd(row.make());
    known = true;
  }
  return known;
}
