// main.cpp — the `dwarf_bench` CLI (reference: main.cpp:13-101) with the same positional argument and
// flags, parsed by hand (Boost.program_options is not available here):
//   dwarf_bench <Dwarf|list> [--input_size N [N ...]] [--iterations K] [--device cpu|gpu|igpu|hip]
//               [--report_path FILE] [--groups_count G] [--executors E] [--gpus P] [--help]
// Exit codes as in the reference: 1 for an unknown dwarf, 0 otherwise — also after a caught exception.
// Built twice: `dwarf_bench`, and with -DEXPERIMENTAL `dwarf_bench_experimental`, which also registers the reference's
// EXPERIMENTAL dwarfs that have a HIP counterpart (populate_experimental_registry), and with -DEXPERIMENTAL_SLAB
// `dwarf_bench_slab`, the default set plus the slab dwarfs (populate_slab_registry), and with -DEXPERIMENTAL_GROUPBY_HASH
// `dwarf_bench_groupby_hash`, the default set plus GroupByHashHip (populate_groupby_hash_registry), and with
// -DEXPERIMENTAL_SORT_PAIRS `dwarf_bench_sort_pairs`, the default set plus RadixPairsHip (populate_sort_pairs_registry),
// and with -DEXPERIMENTAL_JOIN_PAIRS `dwarf_bench_join_pairs`, the default set plus JoinPairsHip
// (populate_join_pairs_registry), and with -DEXPERIMENTAL_TOPK `dwarf_bench_topk`, the default set plus TopKHip
// (populate_topk_registry), and with -DEXPERIMENTAL_GROUPBY_SORTED `dwarf_bench_groupby_sorted`, the default set plus
// GroupBySortedHip (populate_groupby_sorted_registry), and with -DEXPERIMENTAL_WINDOW `dwarf_bench_window`, the default
// set plus WindowSortedHip (populate_window_registry), and with -DEXPERIMENTAL_RANGE_JOIN `dwarf_bench_range_join`, the
// default set plus RangeJoinHip (populate_range_join_registry).
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "bench.hpp"
#include "dwarf_api.hpp"

namespace {
// the dwarfs that read --groups_count (WindowSortedHip partitions by the keys GroupBySortedHip groups by)
bool isGroupBy(const std::string &dwarfName) {
  return dwarfName.find("GroupBy") != std::string::npos || dwarfName.find("WindowSorted") != std::string::npos;
}

const char *kHelp =
    "Dwarf bench:\n"
    "  --help                 Show help message\n"
    "  --dwarf arg            Dwarf to run. List all with 'list' option.\n"
    "  --input_size arg       Data array size, ususally a column size in elements\n"
    "  --iterations arg       Number of iterations to run a bmark.\n"
    "  --device arg           Device to run on.\n"
    "  --report_path arg      Full/Relative path to a report file.\n"
    "  --groups_count arg     Number of unique keys for dwarfs with keys (groupby, hash build etc.).\n"
    "  --executors arg        Number of executors for GroupByLocal.\n"
    "  --gpus arg             Number of GPUs (ranks) for PartitionedJoinHip (default 1).\n";

bool is_flag(const std::string &s) { return s.rfind("--", 0) == 0; }
}  // namespace

int main(int argc, char *argv[]) {
  populate_registry();
#ifdef EXPERIMENTAL
  populate_experimental_registry();  // dwarf_bench_experimental
#endif
#ifdef EXPERIMENTAL_SLAB
  populate_slab_registry();  // dwarf_bench_slab
#endif
#ifdef EXPERIMENTAL_GROUPBY_HASH
  populate_groupby_hash_registry();  // dwarf_bench_groupby_hash
#endif
#ifdef EXPERIMENTAL_SORT_PAIRS
  populate_sort_pairs_registry();  // dwarf_bench_sort_pairs
#endif
#ifdef EXPERIMENTAL_JOIN_PAIRS
  populate_join_pairs_registry();  // dwarf_bench_join_pairs
#endif
#ifdef EXPERIMENTAL_TOPK
  populate_topk_registry();  // dwarf_bench_topk
#endif
#ifdef EXPERIMENTAL_GROUPBY_SORTED
  populate_groupby_sorted_registry();  // dwarf_bench_groupby_sorted
#endif
#ifdef EXPERIMENTAL_WINDOW
  populate_window_registry();  // dwarf_bench_window
#endif
#ifdef EXPERIMENTAL_RANGE_JOIN
  populate_range_join_registry();  // dwarf_bench_range_join
#endif
  Registry *registry = Registry::instance();

  auto opts = std::make_unique<RunOptions>();
  size_t groups_count = 1, executors = 1;
  opts->root_path = helpers::get_kernels_root_env(argv[0]);
  std::cout << "DWARF_BENCH_ROOT is set to " << opts->root_path << std::endl
            << "You can change that with 'export DWARF_BENCH_ROOT=/your/path'\n";

  std::string dwarf_name;
  bool want_help = false;
  try {
    for (int i = 1; i < argc; ++i) {
      std::string arg = argv[i], value;
      const size_t eq = arg.find('=');
      const bool has_inline = is_flag(arg) && eq != std::string::npos;
      if (has_inline) {
        value = arg.substr(eq + 1);
        arg = arg.substr(0, eq);
      }
      auto next_value = [&]() -> std::string {
        if (has_inline) return value;
        if (i + 1 >= argc) throw std::invalid_argument("the required argument for option '" + arg + "' is missing");
        return argv[++i];
      };
      if (arg == "--help") {
        want_help = true;
      } else if (arg == "--dwarf") {
        dwarf_name = next_value();
      } else if (arg == "--input_size") {  // multitoken: every following non-flag token is a size
        opts->input_size.push_back(std::stoull(next_value()));
        while (i + 1 < argc && !is_flag(argv[i + 1])) opts->input_size.push_back(std::stoull(argv[++i]));
      } else if (arg == "--iterations") {
        opts->iterations = std::stoull(next_value());
      } else if (arg == "--device") {
        std::istringstream in(next_value());
        in >> opts->device_ty;
      } else if (arg == "--report_path") {
        opts->report_path = next_value();
      } else if (arg == "--groups_count") {
        groups_count = std::stoull(next_value());
      } else if (arg == "--executors") {
        executors = std::stoull(next_value());
      } else if (arg == "--gpus") {
        opts->devices = std::stoull(next_value());
      } else if (!is_flag(arg) && dwarf_name.empty()) {
        dwarf_name = arg;  // positional: the dwarf
      } else {
        throw std::invalid_argument("unrecognised option '" + arg + "'");
      }
    }

    if (dwarf_name == "list") {
      std::cout << "Supported dwarfs:\n";
      for (const auto &dw : *registry) std::cout << "\t" << dw.first << std::endl;
      return 0;
    }
    Dwarf *dwarf = registry->find(dwarf_name);
    if (want_help) {
      std::cout << kHelp;
      return 0;
    } else if (!dwarf) {
      std::cerr << "List supported dwarfs to run with '" << argv[0] << " list'" << std::endl;
      return 1;
    }
    if (opts->input_size.empty()) opts->input_size.push_back(1);

    if (isGroupBy(dwarf_name)) opts = std::make_unique<GroupByRunOptions>(*opts, groups_count, executors);

    dwarf->init(*opts);
    dwarf->run(*opts);
    dwarf->report(*opts);
  } catch (std::exception &e) {
    std::cerr << "Caught exception: " << e.what() << std::endl;
  }
  return 0;
}
