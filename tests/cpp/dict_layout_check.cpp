// dict_layout_check.cpp — dwarf_bench_amd/host/dict_layout.hpp on the host, the text the kernels of dict_encode.cpp run:
// the hash against Murmur3's finaliser written out again, the slot count and the workspace regions for every capacity
// the file named on the command line lists (capacity, the inner sort's workspace bytes, the exported query's answer:
// tests/test_dict_layout_cpp.py writes it from the two libraries), and the insert and find loops on a host copy of the
// table: an array that aborts on an index outside it, a claim that is a plain store.  Chains that wrap past the table's
// end, a table filled to the last slot, keys 0 and 0xFFFFFFFF.  No GPU, no HIP: plain C++.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "dict_layout.hpp"

namespace {

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

long g_reads = 0;

// a table that sees every index used on it; the storage is exactly `slots` entries, so an index that slipped past the
// check would also be a heap overflow for a sanitizer to see
struct Checked {
  std::vector<DictSlot> *data;
  DictSlot operator[](uint32_t s) const {
    REQUIRE(s < data->size());
    ++g_reads;
    return (*data)[s];
  }
};

std::vector<DictSlot> empty_table(uint64_t slots) {
  DictSlot e;
  e.key = 0;
  e.code = DBENCH_DICT_EMPTY;
  return std::vector<DictSlot>(slots, e);
}

int insert(std::vector<DictSlot> &t, uint32_t key) {
  const uint32_t mask = static_cast<uint32_t>(t.size() - 1);
  return dict_insert(Checked{&t}, mask, key, [&](uint32_t s, uint32_t k) {
    REQUIRE(s < t.size());
    const DictSlot before = t[s];
    REQUIRE(before.code == DBENCH_DICT_EMPTY);  // the loop claims only a slot it has read as empty
    t[s].key = k;
    t[s].code = DBENCH_DICT_PENDING;
    return before;
  });
}

uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

void check_hash_and_slots() {
  REQUIRE(dict_hash(0) == 0 && dict_hash(1) == 0x514E28B7u && dict_hash(0xFFFFFFFFu) == 0x81F16F39u);
  std::mt19937 rng(7);
  for (int i = 0; i < 100000; ++i) {
    const uint32_t k = rng();
    REQUIRE(dict_hash(k) == fmix32(k));
  }
  uint64_t last = 0;
  for (uint64_t c = 1; c <= 4096; ++c) {
    const uint64_t s = dict_slots(c);
    REQUIRE((s & (s - 1)) == 0 && s >= 2 * c && (s == 2 || s / 2 < 2 * c) && s >= last);
    last = s;
  }
  REQUIRE(dict_slots(1) == 2 && dict_slots(2) == 4 && dict_slots(3) == 8 && dict_slots(4096) == DBENCH_DICT_LDS_SLOTS);
  REQUIRE(dict_slots(4097) == 2 * DBENCH_DICT_LDS_SLOTS && dict_slots((1ull << 31) - 1) == (1ull << 32));
  REQUIRE(dict_slots(1ull << 30) == (1ull << 31) && dict_slots((1ull << 30) + 1) == (1ull << 32));
}

// the regions in order, each aligned, none overlapping the next, the last ending at the exported total
long check_layouts(const char *path) {
  std::FILE *f = std::fopen(path, "r");
  REQUIRE(f != nullptr);
  uint64_t capacity, sort_bytes, total, last_total = 0, last_capacity = 0;
  long rows = 0;
  while (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &capacity, &sort_bytes, &total) == 3) {
    const DictLayout l = dict_layout(capacity, sort_bytes);
    REQUIRE(l.slots == dict_slots(capacity));
    REQUIRE(l.table == 256 && l.table % 256 == 0 && l.keys % 256 == 0 && l.tmp % 256 == 0 && l.sort % 256 == 0 && l.total % 256 == 0);
    REQUIRE(l.table + 8 * l.slots <= l.keys);    // header | table
    REQUIRE(l.keys + 4 * capacity <= l.tmp);     // table | keys
    REQUIRE(l.tmp + 4 * capacity <= l.sort);     // keys | tmp
    REQUIRE(l.sort + sort_bytes <= l.total);     // tmp | sort
    REQUIRE(l.keys - l.table < 8 * l.slots + 256 && l.tmp - l.keys < 4 * capacity + 256 && l.total - l.sort < sort_bytes + 256);
    REQUIRE(l.total == total);                   // what dbench_dict_workspace_bytes answers
    REQUIRE(capacity > last_capacity && total >= last_total);
    last_capacity = capacity;
    last_total = total;
    ++rows;
  }
  std::fclose(f);
  return rows;
}

void check_find(const std::vector<DictSlot> &t, const std::set<uint32_t> &held, const std::vector<uint32_t> &absent) {
  const uint32_t mask = static_cast<uint32_t>(t.size() - 1);
  for (uint32_t k : held) {
    REQUIRE(dict_find(Checked{const_cast<std::vector<DictSlot> *>(&t)}, mask, k) == DBENCH_DICT_PENDING);
    const int64_t s = dict_find_slot(Checked{const_cast<std::vector<DictSlot> *>(&t)}, mask, k);
    REQUIRE(s >= 0 && static_cast<uint64_t>(s) < t.size() && t[s].key == k && t[s].code != DBENCH_DICT_EMPTY);
  }
  for (uint32_t k : absent) {
    if (held.count(k)) continue;
    REQUIRE(dict_find(Checked{const_cast<std::vector<DictSlot> *>(&t)}, mask, k) == DBENCH_DICT_EMPTY);
    REQUIRE(dict_find_slot(Checked{const_cast<std::vector<DictSlot> *>(&t)}, mask, k) == -1);
  }
}

// keys that share the home slot `home` of a table of `slots`
std::vector<uint32_t> colliding(uint64_t slots, uint32_t home, size_t how_many) {
  std::vector<uint32_t> out;
  for (uint32_t k = 0; out.size() < how_many; ++k) {
    if ((dict_hash(k) & (slots - 1)) == home) out.push_back(k);
  }
  return out;
}

void check_tables() {
  // a chain that wraps: capacity 8, 16 slots, every key at home in slot 13 -> slots 13, 14, 15, 0, 1, ...
  for (uint64_t capacity : {1ull, 2ull, 8ull, 100ull}) {
    const uint64_t slots = dict_slots(capacity);
    const uint32_t home = static_cast<uint32_t>(slots >= 4 ? slots - 3 : slots - 1);
    const std::vector<uint32_t> keys = colliding(slots, home, slots + 1);
    std::vector<DictSlot> t = empty_table(slots);
    std::set<uint32_t> held;
    for (size_t i = 0; i < slots; ++i) {  // up to the last slot: the chain goes round the end and fills the table
      REQUIRE(insert(t, keys[i]) == 1);
      held.insert(keys[i]);
      REQUIRE(insert(t, keys[i]) == 0 && insert(t, keys[0]) == 0);  // there already: nothing claimed
      REQUIRE(t[(home + i) & (slots - 1)].key == keys[i]);           // the chain's i-th slot, modulo the table
      check_find(t, held, keys);
    }
    REQUIRE(insert(t, keys[slots]) == -1);  // one key more than slots: a whole round, then full
    REQUIRE(dict_find(Checked{&t}, static_cast<uint32_t>(slots - 1), keys[slots]) == DBENCH_DICT_EMPTY);
    for (const DictSlot &e : t) REQUIRE(e.code == DBENCH_DICT_PENDING);
  }
  // the key values at the ends of both number lines are keys like any other: 0 is not "empty", 0xFFFFFFFF is not
  {
    std::vector<DictSlot> t = empty_table(dict_slots(4));
    const std::vector<uint32_t> edges = {0u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    check_find(t, {}, edges);  // an empty table holds none of them, key 0 included
    std::set<uint32_t> held;
    for (uint32_t k : edges) {
      REQUIRE(insert(t, k) == 1 && insert(t, k) == 0);
      held.insert(k);
      check_find(t, held, edges);
    }
  }
  // random keys with repeats at load 1/2 against std::set, ranks stored as the finalize kernel stores them
  std::mt19937 rng(11);
  for (uint64_t capacity : {3ull, 64ull, 1000ull, 4096ull, 4097ull}) {
    std::vector<DictSlot> t = empty_table(dict_slots(capacity));
    const uint32_t mask = static_cast<uint32_t>(t.size() - 1);
    std::set<uint32_t> held;
    std::vector<uint32_t> absent;
    while (held.size() < capacity) {
      const uint32_t k = rng() % (4 * capacity);
      REQUIRE(insert(t, k) == (held.insert(k).second ? 1 : 0));
    }
    for (int i = 0; i < 1000; ++i) absent.push_back(rng());
    check_find(t, held, absent);
    uint32_t rank = 0;
    for (uint32_t k : held) t[dict_find_slot(Checked{&t}, mask, k)].code = rank++;  // std::set iterates in order
    rank = 0;
    for (uint32_t k : held) {
      const DictSlot home = Checked{&t}[dict_hash(k) & mask];
      REQUIRE(dict_find_after(Checked{&t}, mask, k, home) == rank && dict_find(Checked{&t}, mask, k) == rank);
      ++rank;
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  REQUIRE(argc == 2);
  check_hash_and_slots();
  const long layouts = check_layouts(argv[1]);
  REQUIRE(layouts >= 4096);
  check_tables();
  std::printf("dict layout ok: %ld layouts, %ld table reads\n", layouts, g_reads);
  return 0;
}
