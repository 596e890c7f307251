// A client of the public library API written the way the reference's usage example (example/bench_usage/main.cpp)
// calls it: <bench.hpp> on the include path, RunConfig filled by designated initialisers in the reference's member
// order with the added members left at their defaults, the unscoped enums streamed as integers, and the fields of
// every Measurement read.  Compiled with -fsyntax-only by tests/test_host_layer.py; it never runs.
#include <bench.hpp>

#include <iostream>
#include <type_traits>
#include <vector>

static_assert(std::is_same<decltype(DwarfBench::Measurement{}.dataSize), size_t>::value, "Measurement::dataSize");
static_assert(std::is_same<decltype(DwarfBench::Measurement{}.microseconds), size_t>::value, "Measurement::microseconds");

int main() {
  const std::vector<DwarfBench::Dwarf> dwarfs = {DwarfBench::Dwarf::Scan, DwarfBench::Dwarf::Join,
                                                 DwarfBench::Dwarf::GroupBy, DwarfBench::Dwarf::Sort};
  const std::vector<DwarfBench::DeviceType> devices = {DwarfBench::DeviceType::CPU, DwarfBench::DeviceType::GPU};
  DwarfBench::DwarfBench bench;
  for (DwarfBench::DeviceType device : devices) {
    for (DwarfBench::Dwarf dwarf : dwarfs) {
      DwarfBench::RunConfig config = {
          .device = device,
          .inputSize = 4096,
          .iterations = 3,
          .dwarf = dwarf,
      };
      const auto measurements = bench.makeMeasurements(config);
      for (const auto &m : measurements) {
        std::cout << device << ' ' << dwarf << ": " << m.dataSize << " elements in " << m.microseconds << " us\n";
      }
    }
  }
  // the positional aggregate form of the same four members
  DwarfBench::RunConfig positional{DwarfBench::DeviceType::CPU, 1024, 10, DwarfBench::Dwarf::Sort};
  return bench.makeMeasurements(positional).empty() ? 1 : 0;
}
