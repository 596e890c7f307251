// hip_dwarfs.cpp — host side of the `...Hip` dwarfs (see hip_dwarfs.hpp).
//
// Every _run follows the reference's shape: generate the inputs once per size, then per iteration time the device
// work between steady_clock stamps (host_time: launch + sync, the reference's figure) and between hipEvents
// (kernel_time; time_launch, time_build_probe), validate, record() -> meter.add_result({{"buf_size", n}}, result).
// Differences, all deliberate:
//   * inputs are generated ON the device by the counter-based generators of libdbhip (deterministic
//     seeds instead of std::random_device, common/common.hpp:34-35) and stay resident: host_time does
//     not contain the reference's H2D/D2H of whole columns (scan/scan.cpp:108-120);
//   * validation is ALWAYS on and covers every size (the reference validates every iteration at every size,
//     scan/scan.cpp:157-164, but DPLScan/Radix/GroupBy/JoinOmnisci only in Debug builds): up to
//     DWARF_BENCH_VALIDATE_MAX elements (default 2^24) with the same host algorithms the reference dwarfs use
//     (std::copy_if, std::sort, the expected_GroupBy loop, per-key match counts); above it, where a host check
//     would dominate the run or not fit, with the device-side validators of libdbhip (dbhip_check_*: ordered
//     fingerprint of the compaction, sortedness + multiset fingerprint, weighted group sums, per-row match
//     counts against the sorted build column + id permutation).  DWARF_BENCH_INJECT_FAULT=1 corrupts one word
//     of every result before it is checked: every Result must then come out valid = false (tests use it to
//     show that the checks can fail);
//   * DWARF_BENCH_TIME_TRANSFERS=1 (scan dwarfs): host_time then contains the blocking H2D of src and the D2H
//     of all n output ints, exactly the reference's timed region (scan/scan.cpp:107-128), so the figure is
//     comparable with existing dwarf_bench CSVs;
//   * HIP failures throw DwarfBenchException (setup errors are exceptions in the reference too).
#include "hip_dwarfs.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <unordered_map>

#include "../../include/dbhip.h"
#include "../../include/dbhip_reduce_by_key.h"
#include "../../include/dbhip_scan_by_key.h"
#include "../../include/dbhip_sorted_search.h"
#include "../../include/dbhip_topk.h"
#include "errors.hpp"

using namespace dbench_errors;

namespace {

using clk = std::chrono::steady_clock;

// device buffer with the 256-byte alignment the C ABI asks for (hipMalloc gives more)
template <class T>
class DevBuf {
 public:
  explicit DevBuf(size_t n) : n_(n) { hip_ok(hipMalloc(&p_, std::max<size_t>(n, 1) * sizeof(T)), "hipMalloc"); }
  ~DevBuf() { (void)hipFree(p_); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  T *get() const { return static_cast<T *>(p_); }
  size_t size() const { return n_; }
  // Validation copies go through one pinned staging buffer: a hipMemcpy into pageable memory pins and
  // lazily unpins the destination, and that unpin lands inside the NEXT iteration's timed launch
  // (measured: 40 us -> 7-13 ms of host_time after a 64 MiB pageable D2H).
  std::vector<T> to_host(size_t count) const {
    std::vector<T> h(count);
    const size_t bytes = count * sizeof(T);
    if (bytes == 0) return h;
    if (bytes < (static_cast<size_t>(1) << 20)) {
      hip_ok(hipMemcpy(h.data(), p_, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
      return h;
    }
    struct Pinned {  // lives until the process ends: freeing it from a static destructor would call into a HIP runtime
      void *p = nullptr;  // that may already be shutting down
      size_t cap = 0;
    };
    static Pinned stage;
    constexpr size_t kChunk = static_cast<size_t>(64) << 20;
    if (!stage.p) {
      hip_ok(hipHostMalloc(&stage.p, kChunk, hipHostMallocDefault), "hipHostMalloc");
      stage.cap = kChunk;
    }
    for (size_t off = 0; off < bytes; off += stage.cap) {
      const size_t len = std::min(stage.cap, bytes - off);
      hip_ok(hipMemcpy(stage.p, static_cast<const char *>(p_) + off, len, hipMemcpyDeviceToHost), "hipMemcpy D2H");
      std::memcpy(reinterpret_cast<char *>(h.data()) + off, stage.p, len);
    }
    return h;
  }

 private:
  void *p_ = nullptr;
  size_t n_;
};

struct Events {
  hipEvent_t a, b;
  Events() {
    hip_ok(hipEventCreate(&a), "hipEventCreate");
    hip_ok(hipEventCreate(&b), "hipEventCreate");
  }
  ~Events() {
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
  Duration elapsed() const {
    float ms = 0;
    hip_ok(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
    return Duration(ms * 1000.0);
  }
};

size_t validate_limit() {
  static const size_t v = [] {
    const char *e = std::getenv("DWARF_BENCH_VALIDATE_MAX");
    return e ? static_cast<size_t>(std::strtoull(e, nullptr, 10)) : (static_cast<size_t>(1) << 24);
  }();
  return v;
}

bool env_flag(const char *name) {
  const char *e = std::getenv(name);
  return e && std::atoi(e) != 0;
}
bool inject_fault() {
  static const bool v = env_flag("DWARF_BENCH_INJECT_FAULT");
  return v;
}
bool time_transfers() {
  static const bool v = env_flag("DWARF_BENCH_TIME_TRANSFERS");
  return v;
}
// fault injection: flip bits of one device word (after the timed region, before the check)
void poke_xor(void *dev_word, uint32_t mask) {
  uint32_t h = 0;
  hip_ok(hipMemcpy(&h, dev_word, sizeof(h), hipMemcpyDeviceToHost), "poke D2H");
  h ^= mask;
  hip_ok(hipMemcpy(dev_word, &h, sizeof(h), hipMemcpyHostToDevice), "poke H2D");
}

// result words of a dbhip_check_* call
class CheckWords {
 public:
  CheckWords() : dev_(4) {}
  uint64_t *dev() const { return dev_.get(); }
  std::array<uint64_t, 4> get() const {
    std::array<uint64_t, 4> h{};
    hip_ok(hipMemcpy(h.data(), dev_.get(), sizeof(h), hipMemcpyDeviceToHost), "check D2H");  // syncs the null stream
    return h;
  }

 private:
  DevBuf<uint64_t> dev_;
};

void check_status(const void *ws, const char *what) {
  uint32_t st = 0xFFFFFFFFu;
  db_ok(dbhip_workspace_status(ws, &st, nullptr), "dbhip_workspace_status");
  if (st != DBHIP_DEV_OK) fail(std::string(what) + ": device status " + std::to_string(st));
}

void banner(const std::string &dwarf) {
  char name[64] = {0};
  int cus = 0, wave = 0;
  int dev = 0;
  hip_ok(hipGetDevice(&dev), "hipGetDevice");
  db_ok(dbhip_device_info(dev, name, sizeof(name), &cus, &wave), "dbhip_device_info");
  std::cout << "Selected device: " << name << " (" << cus << " CUs, wave" << wave << ") for " << dwarf << "\n";
}

DwarfParams size_param(size_t n) { return DwarfParams{{"buf_size", std::to_string(n)}}; }

// the end of every iteration: a failed check prints `message` (if any) on stderr and makes the Result invalid
void record(Meter &meter, size_t n, std::unique_ptr<Result> result, bool ok, const char *message) {
  if (!ok) {
    if (message) std::cerr << message << std::endl;
    result->valid = false;
  }
  meter.add_result(size_param(n), std::move(result));
}

// the timed region of one launch: host_time = launch + sync between steady_clock stamps, kernel_time = the event pair
template <class Launch>
void time_launch(Result &result, const Events &ev, Launch &&launch) {
  const auto host_start = clk::now();
  hip_ok(hipEventRecord(ev.a, nullptr), "event");
  launch();
  hip_ok(hipEventRecord(ev.b, nullptr), "event");
  hip_ok(hipStreamSynchronize(nullptr), "sync");
  const auto host_end = clk::now();
  result.host_time = host_end - host_start;
  result.kernel_time = ev.elapsed();
}

// the timed region of a join: build, sync, probe, sync, each launch between its own event pair; build_time ends at the
// build's sync, probe_time is the rest
template <class Build, class Probe>
void time_build_probe(HashJoinResult &result, const Events &build_ev, const Events &probe_ev, Build &&build,
                      Probe &&probe) {
  const auto host_start = clk::now();
  hip_ok(hipEventRecord(build_ev.a, nullptr), "event");
  build();
  hip_ok(hipEventRecord(build_ev.b, nullptr), "event");
  hip_ok(hipStreamSynchronize(nullptr), "sync");
  const auto build_end = clk::now();
  hip_ok(hipEventRecord(probe_ev.a, nullptr), "event");
  probe();
  hip_ok(hipEventRecord(probe_ev.b, nullptr), "event");
  hip_ok(hipStreamSynchronize(nullptr), "sync");
  const auto host_end = clk::now();
  result.host_time = host_end - host_start;
  result.build_time = build_end - host_start;
  result.probe_time = host_end - build_end;
  result.kernel_time = build_ev.elapsed() + probe_ev.elapsed();
}

// dbhip_gen_unique_sorted_u32 draws n unique keys from [0, 10n)
void require_unique_keys_fit(size_t n, const std::string &who) {
  if (10ull * n > 0xFFFFFFFFull) fail(who + ": keys are drawn from [0, 10*n) and must fit 32 bits");
}

constexpr uint64_t kSlabUniformSeed = 21;  // SlabHashBuildHip's keys: uniform in [1, 10000] from this seed

// every key found (found = n ones) with value == key: vals against the generator itself (uniform keys) or against the
// sorted keys' fingerprint (unique sorted keys); host comparison up to DWARF_BENCH_VALIDATE_MAX
bool found_own_keys(const DevBuf<uint32_t> &keys, const DevBuf<uint32_t> &vals, const DevBuf<uint32_t> &found, size_t n,
                    bool uniform_keys, const std::array<uint64_t, 4> &key_fp, CheckWords &chk) {
  if (n <= validate_limit()) {
    const auto hf = found.to_host(n);
    return std::all_of(hf.begin(), hf.end(), [](uint32_t f) { return f == 1u; }) && vals.to_host(n) == keys.to_host(n);
  }
  db_ok(dbhip_check_sorted_u32(found.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
  const auto g = chk.get();
  bool ok = g[0] == 0 && g[2] == n;  // non-decreasing 0/1 entries summing to n: all ones
  if (uniform_keys) {
    db_ok(dbhip_check_gen_uniform_u32(vals.get(), nullptr, n, kSlabUniformSeed, 0, 1, 10000, chk.dev(), nullptr),
          "dbhip_check_gen_uniform_u32");
    return ok && chk.get()[0] == 0;
  }
  db_ok(dbhip_check_sorted_u32(vals.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
  const auto v = chk.get();
  return ok && v[0] == 0 && v[1] == key_fp[1] && v[2] == key_fp[2];
}

// ---- scan: shared by TwoPassScanHip and DPLScanHip -------------------------------------------------
void run_scan(const char *who, size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  // scan/scan.cpp:73, scan/dplscan.cpp:43 hard-code 5 (selectivity 4e-4 on keys 1..10000); DWARF_BENCH_SCAN_FILTER
  // overrides it for the selectivity sweep of SURVEY 8(d)
  const char *filter_env = std::getenv("DWARF_BENCH_SCAN_FILTER");
  const int filter_value = filter_env ? std::atoi(filter_env) : 5;
  DevBuf<int32_t> src(n), out(n);
  DevBuf<uint64_t> out_size(1);
  const size_t ws_bytes = dbhip_copy_if_lt_i32_workspace_bytes(n);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(reinterpret_cast<uint32_t *>(src.get()), n, 42, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");

  std::vector<int32_t> expected;
  const bool host_check = n <= validate_limit();
  CheckWords want, got;
  const size_t fp_bytes = dbhip_check_fingerprint_workspace_bytes(n);
  DevBuf<unsigned char> fp_ws(fp_bytes);
  std::array<uint64_t, 4> want_fp{};
  if (host_check) {  // scan/scan.cpp:12-17 expected_out_lt
    const std::vector<int32_t> host = src.to_host(n);
    std::copy_if(host.begin(), host.end(), std::back_inserter(expected),
                 [filter_value](int v) { return v < filter_value; });
  } else {  // order-sensitive fingerprint + length of the matching subsequence, straight from src
    db_ok(dbhip_check_fingerprint_lt_i32(src.get(), n, filter_value, want.dev(), fp_ws.get(), fp_bytes, nullptr),
          "dbhip_check_fingerprint_lt_i32");
    want_fp = want.get();
  }
  // DWARF_BENCH_TIME_TRANSFERS=1: the reference's timed region (scan/scan.cpp:107-128) — blocking write of src,
  // kernel, blocking read of all n output ints and of out_size — from/to pageable host vectors like the reference's
  std::vector<int32_t> host_src, host_out;
  if (time_transfers()) {
    host_src = src.to_host(n);
    host_out.resize(n);
  }
  Events ev;
  bool dense = false;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    const auto host_start = clk::now();
    if (time_transfers() && n)
      hip_ok(hipMemcpy(src.get(), host_src.data(), n * sizeof(int32_t), hipMemcpyHostToDevice), "src H2D");
    hip_ok(hipEventRecord(ev.a, nullptr), "event");
    // dense predicates (more than 7.5 % of the rows matched in the previous iteration: the two variants cross between
    // 5 % and 10 % at 2^28 rows, tools/ab.py scan) take the single-launch variant
    if (dense)
      db_ok(dbhip_copy_if_lt_dense_i32(src.get(), n, filter_value, out.get(), out_size.get(), ws.get(), ws_bytes,
                                       nullptr), "dbhip_copy_if_lt_dense_i32");
    else
      db_ok(dbhip_copy_if_lt_i32(src.get(), n, filter_value, out.get(), out_size.get(), ws.get(), ws_bytes, nullptr),
            "dbhip_copy_if_lt_i32");
    hip_ok(hipEventRecord(ev.b, nullptr), "event");
    if (time_transfers() && n)
      hip_ok(hipMemcpy(host_out.data(), out.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost), "out D2H");
    uint64_t count = 0;
    hip_ok(hipMemcpy(&count, out_size.get(), sizeof(count), hipMemcpyDeviceToHost), "out_size D2H");  // syncs
    const auto host_end = clk::now();
    result->host_time = host_end - host_start;
    result->kernel_time = ev.elapsed();
    result->bytes = n * sizeof(int32_t) + count * sizeof(int32_t);
    check_status(ws.get(), who);
    dense = n && count > n / 40 * 3;
    if (inject_fault() && count) poke_xor(out.get() + count / 2, 1u);
    bool ok;
    if (host_check) {
      ok = count == expected.size() && out.to_host(count) == expected;
    } else {  // every element of out passes the filter iff the lengths agree; order and values: the fingerprint
      db_ok(dbhip_check_fingerprint_lt_i32(out.get(), count <= n ? count : n, filter_value, got.dev(), fp_ws.get(),
                                           fp_bytes, nullptr),
            "dbhip_check_fingerprint_lt_i32");
      const auto g = got.get();
      ok = count == want_fp[1] && g[1] == want_fp[1] && g[0] == want_fp[0];
    }
    record(meter, n, std::move(result), ok, "incorrect results");  // scan/scan.cpp:162
  }
}

}  // namespace

void HipDwarf::run(const RunOptions &opts) {
  for (auto size : opts.input_size) {
    banner(name());
    _run(size, meter());
  }
}
void HipDwarf::init(const RunOptions &opts) {
  meter().set_opts(opts);
  meter().set_params({{"device_type", to_string(opts.device_ty)}});
}

// =====================================================================================================
void TwoPassScanHip::_run(const size_t n, Meter &meter) { run_scan("TwoPassScanHip", n, meter); }
void DPLScanHip::_run(const size_t n, Meter &meter) { run_scan("DPLScanHip", n, meter); }

// =====================================================================================================
void RadixHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  const int bits = digit_bits();
  DevBuf<int32_t> src(n), keys(n), tmp(n);
  const size_t ws_bytes = dbhip_radix_sort_workspace_bytes(n, bits);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(reinterpret_cast<uint32_t *>(src.get()), n, 42, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool host_check = n <= validate_limit();
  std::vector<int32_t> expected;
  CheckWords chk;
  std::array<uint64_t, 4> want{};
  if (host_check) {  // sort/radix.cpp:8-12
    expected = src.to_host(n);
    std::sort(expected.begin(), expected.end());
  } else {  // multiset fingerprint of the unsorted column
    db_ok(dbhip_check_sorted_u32(reinterpret_cast<uint32_t *>(src.get()), n, 1, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    want = chk.get();
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    // every iteration sorts the unsorted column again (the reference re-wraps the const host vector,
    // sort/radix.cpp:31); the refresh copy is not timed
    hip_ok(hipMemcpy(keys.get(), src.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice), "refresh");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_radix_sort_i32(keys.get(), tmp.get(), n, bits, ws.get(), ws_bytes, nullptr), "dbhip_radix_sort_i32");
    });
    if (n) check_status(ws.get(), "RadixHip");
    if (inject_fault() && n) poke_xor(keys.get() + n / 2, 0x100u);
    bool ok;
    if (host_check) {
      ok = keys.to_host(n) == expected;
    } else {  // ascending as int32 and the same multiset as the input
      db_ok(dbhip_check_sorted_u32(reinterpret_cast<uint32_t *>(keys.get()), n, 1, chk.dev(), nullptr), "dbhip_check_sorted_u32");
      const auto g = chk.get();
      ok = g[0] == 0 && g[1] == want[1] && g[2] == want[2];
    }
    record(meter, n, std::move(result), ok, "incorrect results");  // sort/radix.cpp:61
  }
}
int RadixHip::digit_bits() {
  const char *e = std::getenv("DWARF_BENCH_RADIX_BITS");
  return (e && std::atoi(e) == 4) ? 4 : 8;
}
void RadixHip::init(const RunOptions &opts) {
  HipDwarf::init(opts);
  // optional calibration, outside every timed region: pins the sort's ranking to what the device-side self-test of
  // the lane order saw (the sorts themselves never synchronise; every tile checks the order invariant regardless)
  (void)dbhip_radix_sort_prepare(nullptr);
}

// =====================================================================================================
// RadixPairsHip — the argsort (dbhip_radix_sort_pairs_i32 with vals_are_row_ids): RadixHip's column, the timed region
// is one call that sorts the keys and returns the stable sort permutation.  No reference counterpart.
void RadixPairsHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  if (n >= (static_cast<size_t>(1) << 32)) fail("RadixPairsHip: fewer than 2^32 rows");
  const int bits = digit_bits();
  DevBuf<int32_t> src(n), keys(n), tmp(n);
  DevBuf<uint32_t> perm(n), tmp_perm(n);
  const size_t ws_bytes = dbhip_radix_sort_pairs_workspace_bytes(n, bits);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(reinterpret_cast<uint32_t *>(src.get()), n, 42, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool host_check = n <= validate_limit();
  std::vector<int32_t> expected_keys;
  std::vector<uint32_t> expected_perm;
  CheckWords chk;
  if (host_check) {  // the stable sort of (key, row) pairs
    const std::vector<int32_t> h = src.to_host(n);
    expected_perm.resize(n);
    for (size_t i = 0; i < n; ++i) expected_perm[i] = static_cast<uint32_t>(i);
    std::stable_sort(expected_perm.begin(), expected_perm.end(), [&](uint32_t a, uint32_t b) { return h[a] < h[b]; });
    expected_keys.resize(n);
    for (size_t i = 0; i < n; ++i) expected_keys[i] = h[expected_perm[i]];
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    hip_ok(hipMemcpy(keys.get(), src.get(), n * sizeof(int32_t), hipMemcpyDeviceToDevice), "refresh");  // not timed
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_radix_sort_pairs_i32(keys.get(), perm.get(), tmp.get(), tmp_perm.get(), n, bits, 1, ws.get(), ws_bytes,
                                       nullptr),
            "dbhip_radix_sort_pairs_i32");
    });
    if (n) check_status(ws.get(), "RadixPairsHip");
    if (inject_fault() && n) poke_xor(perm.get() + n / 2, 1u);  // one id
    bool ok;
    if (host_check) {
      ok = keys.to_host(n) == expected_keys && perm.to_host(n) == expected_perm;
    } else {  // strictly increasing (key, id) pairs, every id naming a row with that key (include/dbhip.h)
      db_ok(dbhip_check_sorted_pairs_u32(reinterpret_cast<uint32_t *>(src.get()), reinterpret_cast<uint32_t *>(keys.get()),
                                         perm.get(), n, 1, chk.dev(), nullptr),
            "dbhip_check_sorted_pairs_u32");
      const auto g = chk.get();
      ok = g[0] == 0 && g[1] == 0;
    }
    record(meter, n, std::move(result), ok, "incorrect results");
  }
}

// =====================================================================================================
// TopKHip — ORDER BY key LIMIT k (dbhip_topk_i32, sorted output): a uniform full-range column, the timed region is one
// call that returns keys and row ids of the first k rows.  No reference counterpart.
void TopKHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  if (n >= (static_cast<size_t>(1) << 32)) fail("TopKHip: fewer than 2^32 rows");
  const char *ek = std::getenv("DWARF_BENCH_TOPK_K");
  const size_t k = std::min<size_t>(ek ? static_cast<size_t>(std::strtoull(ek, nullptr, 10)) : 1024, n);
  const int largest = env_flag("DWARF_BENCH_TOPK_LARGEST") ? 1 : 0;
  DevBuf<int32_t> src(n), out_keys(k);
  DevBuf<uint32_t> out_rows(k);
  const size_t ws_bytes = dbhip_topk_workspace_bytes(n, k);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(reinterpret_cast<uint32_t *>(src.get()), n, 42, 0, 0, 0xFFFFFFFFu, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool host_check = n <= validate_limit();
  std::vector<int32_t> expected_keys;
  std::vector<uint32_t> expected_rows;
  CheckWords chk;
  if (host_check) {  // the first k of the (key, row) pairs, as one number each: better key first, equal keys by row
    const std::vector<int32_t> h = src.to_host(n);
    const uint32_t mask = largest ? 0x7FFFFFFFu : 0x80000000u;  // signed order as unsigned order of key ^ mask
    std::vector<uint64_t> pairs(n);
    for (size_t i = 0; i < n; ++i) pairs[i] = (static_cast<uint64_t>(static_cast<uint32_t>(h[i]) ^ mask) << 32) | i;
    if (k < n) std::nth_element(pairs.begin(), pairs.begin() + k, pairs.end());
    std::sort(pairs.begin(), pairs.begin() + k);
    expected_keys.resize(k);
    expected_rows.resize(k);
    for (size_t i = 0; i < k; ++i) {
      expected_rows[i] = static_cast<uint32_t>(pairs[i]);
      expected_keys[i] = h[expected_rows[i]];
    }
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_topk_i32(src.get(), n, k, largest, 1, out_keys.get(), out_rows.get(), ws.get(), ws_bytes, nullptr),
            "dbhip_topk_i32");
    });
    check_status(ws.get(), "TopKHip");
    if (inject_fault() && k) poke_xor(out_rows.get() + k / 2, 1u);  // one row id
    bool ok;
    if (host_check) {
      ok = out_keys.to_host(k) == expected_keys && out_rows.to_host(k) == expected_rows;
    } else {  // include/dbhip_topk.h: no wrong entry, and exactly k - 1 rows in front of the last one
      db_ok(dbhip_check_topk_u32(reinterpret_cast<uint32_t *>(src.get()), n, reinterpret_cast<uint32_t *>(out_keys.get()),
                                 out_rows.get(), k, largest, 1, chk.dev(), nullptr),
            "dbhip_check_topk_u32");
      const auto g = chk.get();
      ok = g[0] == 0 && g[1] == (k ? k - 1 : 0);
    }
    record(meter, n, std::move(result), ok, "incorrect results");
  }
}

// =====================================================================================================
// ---- group-by: the buffers and the check shared by GroupByHip and GroupByLocalHip ----------------
namespace {
class GroupByBuffers {
 public:
  GroupByBuffers(size_t n, uint32_t groups)
      : keys(n), vals(n), out(groups), ws_bytes(dbhip_groupby_sum_u32_workspace_bytes(n, groups)), ws(ws_bytes),
        host_check_(n <= validate_limit()), expected_(groups, 0) {
    db_ok(dbhip_gen_uniform_u32(vals.get(), n, 43, 0, 1, 10000, nullptr), "gen vals");        // groupby.cpp:29-30
    db_ok(dbhip_gen_uniform_u32(keys.get(), n, 42, 0, 0, groups - 1, nullptr), "gen keys");  // groupby.cpp:31-32
    hip_ok(hipDeviceSynchronize(), "sync");
    if (host_check_) {  // groupby/groupby.cpp:8-19 expected_GroupBy with f = +
      const auto hk = keys.to_host(n);
      const auto hv = vals.to_host(n);
      for (size_t i = 0; i < n; ++i) expected_[hk[i]] = expected_[hk[i]] + hv[i];
    } else {  // sum of val * w(key) mod 2^32 for two weight functions, over the rows
      db_ok(dbhip_check_weighted_sum_u32(keys.get(), vals.get(), n, chk_.dev(), nullptr), "dbhip_check_weighted_sum_u32");
      want_ = chk_.get();
    }
  }
  // the sums in `out` after a run
  bool check() {
    if (host_check_) return out.to_host(out.size()) == expected_;
    // ... and over (g, out[g]): equal iff every row's value reached its own group (mod 2^32, as the sums)
    db_ok(dbhip_check_weighted_sum_u32(nullptr, out.get(), out.size(), chk_.dev(), nullptr), "dbhip_check_weighted_sum_u32");
    const auto g = chk_.get();
    return g[0] == want_[0] && g[1] == want_[1];
  }

  DevBuf<uint32_t> keys, vals, out;
  const size_t ws_bytes;
  DevBuf<unsigned char> ws;

 private:
  const bool host_check_;
  std::vector<uint32_t> expected_;
  CheckWords chk_;
  std::array<uint64_t, 4> want_{};
};
}  // namespace

void GroupByHip::_run(const size_t n, Meter &meter) {
  // callers hand a GroupByRunOptions to GroupBy-family dwarfs (main.cpp:87-92, bench.cpp:80)
  const auto &opts = static_cast<const GroupByRunOptions &>(meter.opts());
  const uint32_t groups = static_cast<uint32_t>(opts.groups_count ? opts.groups_count : 1);
  GroupByBuffers buf(n, groups);
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_groupby_sum_u32(buf.keys.get(), buf.vals.get(), n, groups, buf.out.get(), buf.ws.get(), buf.ws_bytes,
                                  nullptr),
            "dbhip_groupby_sum_u32");
    });
    check_status(buf.ws.get(), "GroupByHip");
    if (inject_fault()) poke_xor(buf.out.get() + groups / 2, 1u);
    record(meter, n, std::move(result), buf.check(), "Incorrect results");
  }
}

// =====================================================================================================
void JoinOmnisciHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  DevBuf<uint32_t> a(n), b(n), ids(n), pos(n), cnt(n);
  const size_t ws_bytes = dbhip_join_workspace_bytes(n);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(a.get(), n, 42, 0, 1, 10000, nullptr), "gen a");  // join_omnisci.cpp:53-58
  db_ok(dbhip_gen_uniform_u32(b.get(), n, 43, 0, 1, 10000, nullptr), "gen b");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool host_check = n <= validate_limit();
  std::vector<uint32_t> ha, hb;
  std::unordered_map<uint32_t, uint32_t> key_count;
  // device-side check above the host limit: the build column sorted (an algorithm that shares nothing with the
  // hash join) gives every probe key's exact multiplicity by binary search
  DevBuf<uint32_t> sorted_a(host_check ? 0 : n), sort_tmp(host_check ? 0 : n);
  const size_t perm_bytes = dbhip_check_permutation_workspace_bytes(n);
  DevBuf<unsigned char> perm_ws(host_check ? 0 : perm_bytes);
  CheckWords chk;
  if (host_check) {
    ha = a.to_host(n);
    hb = b.to_host(n);
    for (uint32_t k : ha) ++key_count[k];
  } else {
    const size_t sort_bytes = dbhip_radix_sort_workspace_bytes(n, 8);
    DevBuf<unsigned char> sort_ws(sort_bytes);
    hip_ok(hipMemcpy(sorted_a.get(), a.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "copy");
    db_ok(dbhip_radix_sort_u32(sorted_a.get(), sort_tmp.get(), n, 8, sort_ws.get(), sort_bytes, nullptr), "sort build keys");
    hip_ok(hipDeviceSynchronize(), "sync");
  }
  Events build_ev, probe_ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<HashJoinResult>();
    time_build_probe(
        *result, build_ev, probe_ev,
        [&] { db_ok(dbhip_join_build_u32(a.get(), n, ids.get(), ws.get(), ws_bytes, nullptr), "dbhip_join_build_u32"); },
        [&] { db_ok(dbhip_join_probe_u32(b.get(), n, ws.get(), n, pos.get(), cnt.get(), nullptr), "dbhip_join_probe_u32"); });
    check_status(ws.get(), "JoinOmnisciHip");
    if (inject_fault() && n) poke_xor(cnt.get() + n / 2, 1u);
    bool ok = true;
    if (host_check) {
      // join/join_omnisci.cpp:31-45 are_equal: size per probe row + every returned id really matches; on top of
      // it the id buffer must be a permutation of the build rows (a key's ids are then distinct rows)
      const auto hpos = pos.to_host(n), hcnt = cnt.to_host(n), hids = ids.to_host(n);
      std::vector<char> seen(n, 0);
      for (size_t j = 0; j < n && ok; ++j) {
        ok = hids[j] < n && !seen[hids[j]];
        if (ok) seen[hids[j]] = 1;
      }
      for (size_t i = 0; i < n && ok; ++i) {
        const auto f = key_count.find(hb[i]);
        const uint32_t want = f == key_count.end() ? 0u : f->second;
        ok = hcnt[i] == want && static_cast<size_t>(hpos[i]) + hcnt[i] <= n;
        // every id of a short list, a spread of 64 (always with both ends) of a long one
        const uint32_t step = hcnt[i] > 64 ? hcnt[i] / 64 : 1;
        for (uint32_t j = 0; ok && j < hcnt[i]; j += step) ok = ha[hids[hpos[i] + j]] == hb[i];
        if (ok && hcnt[i]) ok = ha[hids[hpos[i] + hcnt[i] - 1]] == hb[i];
      }
    } else {
      db_ok(dbhip_check_join_u32(sorted_a.get(), n, b.get(), n, pos.get(), cnt.get(), ids.get(), a.get(), 0, 0, 0,
                                 chk.dev(), nullptr),
            "dbhip_check_join_u32");
      const auto g = chk.get();
      db_ok(dbhip_check_permutation_u32(ids.get(), n, chk.dev(), perm_ws.get(), perm_bytes, nullptr),
            "dbhip_check_permutation_u32");
      ok = g[0] == 0 && chk.get()[0] == 0;
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// JoinPairsHip — the one-to-many join as a table of (build row, probe row) pairs: dbhip_join_radix_u32, then
// dbhip_join_pairs_u32 on its answer.  No reference counterpart (JoinOmnisci stops at the per-row {pointer, size} record).
// n rows a side, keys uniform in [1, max(10000, n)] from JoinOmnisciHip's seeds: the reference's distribution up to 10000
// rows and about n pairs above (n^2 / 10000 would be 2.8e10 pairs at 2^24 rows).  Timed: the join (build_time) and the
// expansion (probe_time) with the capacity an untimed count-only call returned.
void JoinPairsHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  if (n == 0 || n > (static_cast<size_t>(1) << 31)) fail("JoinPairsHip: between 1 and 2^31 rows a side");
  DevBuf<uint32_t> a(n), b(n), ids(n), rid(n), pos(n), cnt(n);
  const size_t join_bytes = dbhip_join_radix_workspace_bytes(n, n), pairs_bytes = dbhip_join_pairs_workspace_bytes(n);
  DevBuf<unsigned char> join_ws(join_bytes), pairs_ws(pairs_bytes);
  DevBuf<uint64_t> total(1);
  const uint32_t key_hi = static_cast<uint32_t>(std::max<size_t>(10000, n));
  db_ok(dbhip_gen_uniform_u32(a.get(), n, 42, 0, 1, key_hi, nullptr), "gen a");
  db_ok(dbhip_gen_uniform_u32(b.get(), n, 43, 0, 1, key_hi, nullptr), "gen b");
  const auto join = [&] {
    db_ok(dbhip_join_radix_u32(a.get(), nullptr, n, b.get(), nullptr, n, ids.get(), rid.get(), pos.get(), cnt.get(),
                               join_ws.get(), join_bytes, nullptr),
          "dbhip_join_radix_u32");
  };
  const auto pairs = [&](uint64_t capacity, uint32_t *out_b, uint32_t *out_p) {
    db_ok(dbhip_join_pairs_u32(ids.get(), n, rid.get(), pos.get(), cnt.get(), n, 0, capacity, out_b, out_p, total.get(),
                               pairs_ws.get(), pairs_bytes, nullptr),
          "dbhip_join_pairs_u32");
  };
  join();  // not timed: the count-only call that sizes the output
  pairs(0, nullptr, nullptr);
  check_status(join_ws.get(), "JoinPairsHip");
  check_status(pairs_ws.get(), "JoinPairsHip");
  const uint64_t capacity = total.to_host(1)[0];
  DevBuf<uint32_t> out_b(capacity), out_p(capacity);

  const bool host_check = n <= validate_limit();
  std::vector<uint64_t> expected;  // probe row << 32 | build row, ascending
  DevBuf<uint32_t> sorted_a(host_check ? 0 : n), sort_tmp(host_check ? 0 : n), b_part(host_check ? 0 : n);
  const size_t perm_bytes = dbhip_check_permutation_workspace_bytes(n);
  DevBuf<unsigned char> perm_ws(host_check ? 0 : perm_bytes);
  CheckWords chk;
  if (host_check) {  // sort-merge join of the two key columns on the host
    const auto ha = a.to_host(n), hb = b.to_host(n);
    std::vector<uint32_t> ia(n), ib(n);
    for (size_t i = 0; i < n; ++i) ia[i] = ib[i] = static_cast<uint32_t>(i);
    std::sort(ia.begin(), ia.end(), [&](uint32_t x, uint32_t y) { return ha[x] < ha[y]; });
    std::sort(ib.begin(), ib.end(), [&](uint32_t x, uint32_t y) { return hb[x] < hb[y]; });
    for (size_t i = 0, j = 0; i < n && j < n;) {
      if (ha[ia[i]] < hb[ib[j]]) {
        ++i;
      } else if (ha[ia[i]] > hb[ib[j]]) {
        ++j;
      } else {
        size_t i1 = i, j1 = j;
        while (i1 < n && ha[ia[i1]] == ha[ia[i]]) ++i1;
        while (j1 < n && hb[ib[j1]] == hb[ib[j]]) ++j1;
        for (size_t y = j; y < j1; ++y)
          for (size_t x = i; x < i1; ++x) expected.push_back(static_cast<uint64_t>(ib[y]) << 32 | ia[x]);
        i = i1;
        j = j1;
      }
    }
    std::sort(expected.begin(), expected.end());
  } else {
    const size_t sort_bytes = dbhip_radix_sort_workspace_bytes(n, 8);
    DevBuf<unsigned char> sort_ws(sort_bytes);
    hip_ok(hipMemcpy(sorted_a.get(), a.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "copy");
    db_ok(dbhip_radix_sort_u32(sorted_a.get(), sort_tmp.get(), n, 8, sort_ws.get(), sort_bytes, nullptr), "sort build keys");
    hip_ok(hipDeviceSynchronize(), "sync");
  }
  Events join_ev, pairs_ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<HashJoinResult>();
    time_build_probe(*result, join_ev, pairs_ev, join, [&] { pairs(capacity, out_b.get(), out_p.get()); });
    check_status(join_ws.get(), "JoinPairsHip");
    check_status(pairs_ws.get(), "JoinPairsHip");
    if (inject_fault() && capacity) poke_xor(out_b.get() + capacity / 2, 1u);  // one build-row id
    bool ok = total.to_host(1)[0] == capacity;
    if (host_check) {
      const auto hb_rows = out_b.to_host(capacity), hp_rows = out_p.to_host(capacity);
      std::vector<uint64_t> got(capacity);
      for (size_t k = 0; k < capacity; ++k) got[k] = static_cast<uint64_t>(hp_rows[k]) << 32 | hb_rows[k];
      std::sort(got.begin(), got.end());
      ok = ok && got == expected;
    } else {
      // the pair table against the answer it was made from, and the answer itself as JoinOmnisciHip checks it (the
      // probe keys brought into the radix join's partition order first)
      db_ok(dbhip_check_join_pairs_u32(a.get(), n, b.get(), n, ids.get(), rid.get(), pos.get(), cnt.get(), 0, out_b.get(),
                                       out_p.get(), capacity, chk.dev(), nullptr),
            "dbhip_check_join_pairs_u32");
      const auto g = chk.get();
      db_ok(dbhip_gather_u32(b.get(), rid.get(), n, b_part.get(), nullptr), "dbhip_gather_u32");
      db_ok(dbhip_check_join_u32(sorted_a.get(), n, b_part.get(), n, pos.get(), cnt.get(), ids.get(), a.get(), 0, 0, 0,
                                 chk.dev(), nullptr),
            "dbhip_check_join_u32");
      const auto j = chk.get();
      db_ok(dbhip_check_permutation_u32(ids.get(), n, chk.dev(), perm_ws.get(), perm_bytes, nullptr),
            "dbhip_check_permutation_u32");
      const auto pi = chk.get();
      db_ok(dbhip_check_permutation_u32(rid.get(), n, chk.dev(), perm_ws.get(), perm_bytes, nullptr),
            "dbhip_check_permutation_u32");
      ok = ok && g[0] == 0 && g[1] == capacity && g[2] == g[3] && j[0] == 0 && j[1] == capacity && pi[0] == 0 &&
           chk.get()[0] == 0;
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// ---- unique-key join: the buffers and the check shared by JoinHip and SlabJoinHip -----------------
namespace {
class UniqueJoinBuffers {
 public:
  UniqueJoinBuffers(size_t n, size_t ws_bytes)
      : ak(n), av(n), bk(n), bv(n), ok_(n), o1(n), o2(n), ws_bytes(ws_bytes), ws(ws_bytes), n_(n),
        host_check_(n <= validate_limit()) {
    // unique, ascending keys in [0, 10n) like helpers::make_unique_random (common/common.cpp:7-20)
    db_ok(dbhip_gen_unique_sorted_u32(ak.get(), n, 11, 0, nullptr), "gen");
    db_ok(dbhip_gen_unique_sorted_u32(av.get(), n, 12, 0, nullptr), "gen");
    db_ok(dbhip_gen_unique_sorted_u32(bk.get(), n, 13, 0, nullptr), "gen");
    db_ok(dbhip_gen_unique_sorted_u32(bv.get(), n, 14, 0, nullptr), "gen");
    hip_ok(hipDeviceSynchronize(), "sync");
    if (host_check_) {
      const auto hak = ak.to_host(n), hav = av.to_host(n);
      hbk_ = bk.to_host(n);
      hbv_ = bv.to_host(n);
      for (size_t i = 0; i < n; ++i) a_payload_.emplace(hak[i], hav[i]);
    }
  }
  // the probe's (ok_, o1, o2) after a run: per probe row (key, build value, probe value), all 0xFFFFFFFF on a miss
  bool check() {
    bool ok = true;
    if (host_check_) {
      // same table as seq_join would produce (join.cpp:27-28, :133): unique keys -> per probe row
      const auto hk = ok_.to_host(n_), h1 = o1.to_host(n_), h2 = o2.to_host(n_);
      for (size_t i = 0; i < n_ && ok; ++i) {
        const auto f = a_payload_.find(hbk_[i]);
        if (f == a_payload_.end())
          ok = hk[i] == 0xFFFFFFFFu && h1[i] == 0xFFFFFFFFu && h2[i] == 0xFFFFFFFFu;
        else
          ok = hk[i] == hbk_[i] && h1[i] == f->second && h2[i] == hbv_[i];
      }
    } else {  // the build keys are generated ascending and unique: binary search finds every probe row's partner
      db_ok(dbhip_check_ujoin_u32(ak.get(), av.get(), n_, bk.get(), bv.get(), n_, ok_.get(), o1.get(), o2.get(), chk_.dev(),
                                  nullptr),
            "dbhip_check_ujoin_u32");
      ok = chk_.get()[0] == 0;
    }
    return ok;
  }

  DevBuf<uint32_t> ak, av, bk, bv, ok_, o1, o2;
  const size_t ws_bytes;  // the join's table
  DevBuf<unsigned char> ws;

 private:
  const size_t n_;
  const bool host_check_;
  std::unordered_map<uint32_t, uint32_t> a_payload_;
  std::vector<uint32_t> hbk_, hbv_;
  CheckWords chk_;
};
}  // namespace

void JoinHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  require_unique_keys_fit(n, name());
  UniqueJoinBuffers buf(n, dbhip_ujoin_workspace_bytes(n));
  Events build_ev, probe_ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<HashJoinResult>();
    time_build_probe(
        *result, build_ev, probe_ev,
        [&] {
          db_ok(dbhip_ujoin_build_u32(buf.ak.get(), buf.av.get(), n, buf.ws.get(), buf.ws_bytes, nullptr),
                "dbhip_ujoin_build_u32");
        },
        [&] {
          db_ok(dbhip_ujoin_probe_u32(buf.bk.get(), buf.bv.get(), n, buf.ws.get(), n, buf.ok_.get(), buf.o1.get(),
                                      buf.o2.get(), nullptr),
                "dbhip_ujoin_probe_u32");
        });
    check_status(buf.ws.get(), "JoinHip");
    if (inject_fault() && n) poke_xor(buf.o1.get() + n / 2, 1u);
    record(meter, n, std::move(result), buf.check(), "Incorrect results");
  }
}

// =====================================================================================================
// GroupByLocalHip — the reference's privatised group-by as its own dwarf (groupby/groupby_local.cpp:24-142):
// GroupByAggResult with the two phases timed separately and the CSV header
// "total_time,group_by_time,reduction_time"; --executors caps the number of private tables.
GroupByLocalHip::GroupByLocalHip() : HipDwarf("GroupByLocalHip") {
  reporting_header_ = "total_time,group_by_time,reduction_time";  // groupby_local.cpp:138
}
void GroupByLocalHip::_run(const size_t n, Meter &meter) {
  const auto &opts = static_cast<const GroupByRunOptions &>(meter.opts());
  const uint32_t groups = static_cast<uint32_t>(opts.groups_count ? opts.groups_count : 1);
  const uint32_t executors = static_cast<uint32_t>(opts.executors);
  GroupByBuffers buf(n, groups);
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<GroupByAggResult>();
    const auto host_start = clk::now();
    hip_ok(hipEventRecord(ev.a, nullptr), "event");
    db_ok(dbhip_groupby_partial_u32(buf.keys.get(), buf.vals.get(), n, groups, executors, buf.ws.get(), buf.ws_bytes,
                                    nullptr),
          "dbhip_groupby_partial_u32");
    hip_ok(hipStreamSynchronize(nullptr), "sync");  // the reference waits between the two kernels (:83, :112)
    const auto group_by_end = clk::now();
    db_ok(dbhip_groupby_merge_u32(groups, executors, buf.out.get(), buf.ws.get(), nullptr), "dbhip_groupby_merge_u32");
    hip_ok(hipEventRecord(ev.b, nullptr), "event");
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    const auto host_end = clk::now();
    result->host_time = host_end - host_start;
    result->group_by_time = group_by_end - host_start;
    result->reduction_time = host_end - group_by_end;
    result->kernel_time = ev.elapsed();
    check_status(buf.ws.get(), "GroupByLocalHip");
    if (inject_fault()) poke_xor(buf.out.get() + groups / 2, 1u);
    record(meter, n, std::move(result), buf.check(), "Incorrect results");
  }
}

// =====================================================================================================
// HashBuildHip — build-only timing of the bitmask-claimed table (hash/hash_build.cpp:8-98): every row
// inserts (key, key) into a table of 2n slots, Murmur3 hash; afterwards every key must be found.
void HashBuildHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  const size_t ht_size = n ? n * 2 : 1;  // hash_build.cpp:19
  const uint32_t seed = 421;             // the reference draws it at random (helpers::make_random)
  DevBuf<uint32_t> src(n), found(n);
  const size_t ws_bytes = dbhip_bitmask_table_workspace_bytes(ht_size);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(src.get(), n, 42, 0, 1, 10000, nullptr), "gen");
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    db_ok(dbhip_bitmask_table_reset(ws.get(), ws_bytes, ht_size, nullptr), "reset");  // fresh table, untimed (:23-26)
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_bitmask_table_insert_u32(src.get(), src.get(), n, ws.get(), ws_bytes, ht_size, 1, seed, 0, nullptr),
            "dbhip_bitmask_table_insert_u32");
    });
    check_status(ws.get(), "HashBuildHip");
    // hash_build.cpp:60-83: has(key) must be 1 for every inserted key
    db_ok(dbhip_bitmask_table_lookup_u32(src.get(), n, ws.get(), ht_size, 1, seed, nullptr, found.get(), nullptr),
          "dbhip_bitmask_table_lookup_u32");
    const auto h = found.to_host(n);
    record(meter, n, std::move(result), std::all_of(h.begin(), h.end(), [](uint32_t f) { return f == 1u; }),
           "Incorrect results");
  }
}

// =====================================================================================================
// HashBuildNonBitmaskHip — build-only timing of the CAS-claimed table (hash/hash_build_non_bitmask.cpp:7-91):
// distinct keys claim slots with atomicCAS, duplicates land on the same slot; every key must be found.
void HashBuildNonBitmaskHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  DevBuf<uint32_t> src(n), ok_(n), o1(n), o2(n);
  const size_t ws_bytes = dbhip_ujoin_workspace_bytes(n);
  DevBuf<unsigned char> ws(ws_bytes);
  db_ok(dbhip_gen_uniform_u32(src.get(), n, 42, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_ujoin_build_u32(src.get(), src.get(), n, ws.get(), ws_bytes, nullptr), "dbhip_ujoin_build_u32");
    });
    check_status(ws.get(), "HashBuildNonBitmaskHip");
    db_ok(dbhip_ujoin_probe_u32(src.get(), src.get(), n, ws.get(), n, ok_.get(), o1.get(), o2.get(), nullptr), "probe");
    const auto hk = ok_.to_host(n), hs = src.to_host(n);
    // every key found (a miss would leave the 0xFFFFFFFF sentinel)
    record(meter, n, std::move(result), hk == hs, "Incorrect results");
  }
}

// =====================================================================================================
// ProbeHip — probe-only timing (probe/slab_probe.cpp:9-107: the table is built untimed, :38-62, the timed region is the
// lookup kernel alone, :64-95, over the SAME unique keys that were inserted, so every lookup must hit, :100-103).
// Table = the LDS-partitioned one-to-many table of dwarf 4a (DWARF_BENCH_PROBE_TABLE=bitmask: the bitmask-claimed
// SimpleNonOwningHashTable instead); keys from the make_unique_random twin.  Isolates the probe's share of the join:
// algorithmic bytes 4n (keys) + 8n (position, count).
void ProbeHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  require_unique_keys_fit(n, name());
  const char *table_env = std::getenv("DWARF_BENCH_PROBE_TABLE");
  const bool bitmask = table_env && std::string(table_env) == "bitmask";
  DevBuf<uint32_t> keys(n), ids(n), pos(n), cnt(n);
  db_ok(dbhip_gen_unique_sorted_u32(keys.get(), n, 11, 0, nullptr), "gen");  // slab_probe.cpp:17
  const size_t ht_size = n ? 2 * n : 1;
  const uint32_t seed = 421;
  const size_t ws_bytes = bitmask ? dbhip_bitmask_table_workspace_bytes(ht_size) : dbhip_join_workspace_bytes(n);
  DevBuf<unsigned char> ws(ws_bytes);
  CheckWords chk;
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    // build: untimed, a fresh table every iteration like the reference's AllocAdapter (:26-33)
    if (bitmask) {
      db_ok(dbhip_bitmask_table_reset(ws.get(), ws_bytes, ht_size, nullptr), "reset");
      db_ok(dbhip_bitmask_table_insert_u32(keys.get(), keys.get(), n, ws.get(), ws_bytes, ht_size, 1, seed, 0, nullptr),
            "dbhip_bitmask_table_insert_u32");
    } else {
      db_ok(dbhip_join_build_u32(keys.get(), n, ids.get(), ws.get(), ws_bytes, nullptr), "dbhip_join_build_u32");
    }
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      if (bitmask)
        db_ok(dbhip_bitmask_table_lookup_u32(keys.get(), n, ws.get(), ht_size, 1, seed, pos.get(), cnt.get(), nullptr),
              "dbhip_bitmask_table_lookup_u32");
      else
        db_ok(dbhip_join_probe_u32(keys.get(), n, ws.get(), n, pos.get(), cnt.get(), nullptr), "dbhip_join_probe_u32");
    });
    result->bytes = 12 * n;
    if (n) check_status(ws.get(), "ProbeHip");
    if (inject_fault() && n) poke_xor(cnt.get() + n / 2, 1u);
    // slab_probe.cpp:36-37, :100-103: output == vector(n, 1) — every key found (once); the payload / the id the
    // probe leads to must be the key's own
    bool ok = true;
    if (n <= validate_limit()) {
      const auto hc = cnt.to_host(n), hp = pos.to_host(n);
      ok = std::all_of(hc.begin(), hc.end(), [](uint32_t c) { return c == 1u; });
      if (ok && bitmask) {
        ok = hp == keys.to_host(n);  // payload = key
      } else if (ok) {
        const auto hi = ids.to_host(n);
        for (size_t i = 0; i < n && ok; ++i) ok = hp[i] < n && hi[hp[i]] == i;
      }
    } else {  // sum of the counts == n with every count <= 1 is "all ones"; the join check covers both on the device
      if (bitmask) {
        db_ok(dbhip_check_sorted_u32(cnt.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
        const auto g = chk.get();
        ok = g[0] == 0 && g[2] == n;  // non-decreasing and summing to n over n entries that are 0 or 1
      } else {
        db_ok(dbhip_check_join_u32(keys.get(), n, keys.get(), n, pos.get(), cnt.get(), ids.get(), keys.get(), 0, 0, 0,
                                   chk.dev(), nullptr),
              "dbhip_check_join_u32");
        const auto g = chk.get();
        ok = g[0] == 0 && g[1] == n;
      }
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// ReduceHip — int sum of a column (reduce/reduce.cpp:27-98); expected = std::accumulate(..., 0) (:21).
void ReduceHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  DevBuf<int32_t> src(n), out(1);
  db_ok(dbhip_gen_uniform_u32(reinterpret_cast<uint32_t *>(src.get()), n, 42, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool host_check = n <= validate_limit();
  int32_t expected = 0;
  if (host_check) {
    const auto h = src.to_host(n);
    uint32_t acc = 0;  // accumulate with defined wrap-around; equals the int sum wherever that is defined
    for (int32_t v : h) acc += static_cast<uint32_t>(v);
    expected = static_cast<int32_t>(acc);
  } else {  // the 64-bit key sum of the sortedness check's kernel, truncated: another code path over the same column
    CheckWords chk;
    db_ok(dbhip_check_sorted_u32(reinterpret_cast<uint32_t *>(src.get()), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    expected = static_cast<int32_t>(static_cast<uint32_t>(chk.get()[2]));
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    const auto host_start = clk::now();
    hip_ok(hipEventRecord(ev.a, nullptr), "event");
    db_ok(dbhip_reduce_sum_i32(src.get(), n, out.get(), nullptr), "dbhip_reduce_sum_i32");
    hip_ok(hipEventRecord(ev.b, nullptr), "event");
    int32_t host_out = 0;
    hip_ok(hipMemcpy(&host_out, out.get(), sizeof(host_out), hipMemcpyDeviceToHost), "D2H");  // syncs
    const auto host_end = clk::now();
    result->host_time = host_end - host_start;
    result->kernel_time = ev.elapsed();
    result->bytes = n * sizeof(int32_t);
    if (inject_fault()) host_out ^= 1;
    record(meter, n, std::move(result), host_out == expected, "Incorrect results");
  }
}

// =====================================================================================================
// NestedLoopJoinHip — join/nested_join.cpp:10-110: n x n cell matrix on the device, compacted on the host in
// cell order (:81-90), compared with the a-major/b-minor nested loop of join_helpers::seq_join.
void NestedLoopJoinHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  if (n > (static_cast<size_t>(1) << 15)) fail("NestedLoopJoinHip: the n x n cell matrix is limited to n <= 32768");
  const size_t cells = n * n;
  DevBuf<uint32_t> ak(n), av(n), bk(n), bv(n), ok_(cells), o1(cells), o2(cells);
  db_ok(dbhip_gen_uniform_u32(ak.get(), n, 42, 0, 1, 10000, nullptr), "gen");
  db_ok(dbhip_gen_uniform_u32(av.get(), n, 43, 0, 1, 10000, nullptr), "gen");
  db_ok(dbhip_gen_uniform_u32(bk.get(), n, 44, 0, 1, 10000, nullptr), "gen");
  db_ok(dbhip_gen_uniform_u32(bv.get(), n, 45, 0, 1, 10000, nullptr), "gen");
  hip_ok(hipDeviceSynchronize(), "sync");
  const bool validate = cells <= validate_limit();
  using Row = std::array<uint32_t, 3>;
  std::vector<Row> expected;
  if (validate) {  // join_helpers.hpp:86-104
    const auto hak = ak.to_host(n), hav = av.to_host(n), hbk = bk.to_host(n), hbv = bv.to_host(n);
    for (size_t i = 0; i < n; ++i)
      for (size_t j = 0; j < n; ++j)
        if (hak[i] == hbk[j]) expected.push_back({hak[i], hav[i], hbv[j]});
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_nested_join_u32(ak.get(), av.get(), bk.get(), bv.get(), n, n, ok_.get(), o1.get(), o2.get(), nullptr),
            "dbhip_nested_join_u32");
    });
    result->bytes = 12 * cells;
    bool ok = true;
    if (validate) {
      const auto hk = ok_.to_host(cells), h1 = o1.to_host(cells), h2 = o2.to_host(cells);
      std::vector<Row> got;
      for (size_t c = 0; c < cells; ++c)
        if (hk[c] != 0u) got.push_back({hk[c], h1[c], h2[c]});
      ok = got == expected;
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// CuckooHashBuildHip — build timing of the cuckoo table (hash/cuckoo_hash_build.cpp:8-134): unique keys from the
// make_unique_random twin, vals = keys, ht_size = 4n (:14).  Hasher pair: hash_kind 2 (splitmix64), not the reference's
// two Murmur3 seeds, whose positions come in swapped pairs and cannot hold 2^24 keys for any seeds (include/dbhip.h,
// DESIGN.md §4.6).  The timed region is the reference's rebuild loop (:43-92):
// reset, insert, read the status word, and again with the next seed pair while a row reports a dropped pair, at most
// kCuckooMaxAttempts times (the reference retries without bound).  Seeds: the deterministic sequence of
// ops.cuckoo_seed_pair (the reference draws them at random), one sequence per iteration.  kernel_time = the sum of
// the attempts' reset + insert.  Afterwards every key must be found with its own value (:104-119); a build that failed
// every attempt is "Incorrect results".
namespace {
constexpr int kCuckooMaxAttempts = 16;
constexpr int kCuckooHashKind = 2;
uint64_t splitmix64(uint64_t seed, uint64_t i) {  // dbhip mix64 (csrc/dbhip_common.hpp)
  uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1B54A32D192ED03ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
void cuckoo_seed_pair(uint64_t seed, uint64_t attempt, uint32_t *s1, uint32_t *s2) {  // = ops.cuckoo_seed_pair
  *s1 = static_cast<uint32_t>(splitmix64(seed, 2 * attempt));
  *s2 = static_cast<uint32_t>(splitmix64(seed, 2 * attempt + 1));
  if (*s2 == *s1) *s2 ^= 1u;
}
}  // namespace

void CuckooHashBuildHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  require_unique_keys_fit(n, name());
  const size_t ht_size = n ? 4 * n : 1;  // cuckoo_hash_build.cpp:14
  DevBuf<uint32_t> keys(n), vals(n), found(n);
  db_ok(dbhip_gen_unique_sorted_u32(keys.get(), n, 11, 0, nullptr), "gen");  // make_unique_random (:12)
  const size_t ws_bytes = dbhip_cuckoo_table_workspace_bytes(ht_size);
  DevBuf<unsigned char> ws(ws_bytes);
  CheckWords chk;
  std::array<uint64_t, 4> key_fp{};
  if (n > validate_limit()) {  // sortedness + multiset fingerprint of the keys: what the looked-up values must reproduce
    db_ok(dbhip_check_sorted_u32(keys.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    key_fp = chk.get();
  }
  hip_ok(hipDeviceSynchronize(), "sync");
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    uint32_t s1 = 0, s2 = 0;
    int attempts = 0;
    bool built = false;
    Duration kernel{0};
    const auto host_start = clk::now();
    while (!built && attempts < kCuckooMaxAttempts) {
      cuckoo_seed_pair(it, attempts, &s1, &s2);
      ++attempts;
      hip_ok(hipEventRecord(ev.a, nullptr), "event");
      db_ok(dbhip_cuckoo_table_reset(ws.get(), ws_bytes, ht_size, nullptr), "dbhip_cuckoo_table_reset");
      db_ok(dbhip_cuckoo_table_insert_u32(keys.get(), keys.get(), n, ws.get(), ws_bytes, ht_size, kCuckooHashKind, s1, s2, 0, 0,
                                          nullptr, nullptr),
            "dbhip_cuckoo_table_insert_u32");
      hip_ok(hipEventRecord(ev.b, nullptr), "event");
      uint32_t st = 0xFFFFFFFFu;
      db_ok(dbhip_workspace_status(ws.get(), &st, nullptr), "dbhip_workspace_status");  // synchronises
      kernel += ev.elapsed();
      if (st != DBHIP_DEV_OK && st != DBHIP_DEV_TABLE_FULL)
        fail("CuckooHashBuildHip: device status " + std::to_string(st));
      built = st == DBHIP_DEV_OK;
    }
    const auto host_end = clk::now();
    result->host_time = host_end - host_start;
    result->kernel_time = kernel;
    std::cout << "CuckooHashBuildHip: " << n << " keys, " << ht_size << " slots: " << attempts
              << (attempts == 1 ? " attempt" : " attempts") << (built ? "" : ", every one failed") << "\n";
    bool ok = built;
    if (ok && n) {  // cuckoo_hash_build.cpp:104-119: every key is found, here also with its own value
      db_ok(dbhip_cuckoo_table_lookup_u32(keys.get(), n, ws.get(), ht_size, kCuckooHashKind, s1, s2, vals.get(), found.get(), nullptr),
            "dbhip_cuckoo_table_lookup_u32");
      hip_ok(hipStreamSynchronize(nullptr), "sync");
      if (inject_fault()) poke_xor(vals.get() + n / 2, 1u);
      ok = found_own_keys(keys, vals, found, n, false, key_fp, chk);
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// The slab dwarfs (hash/slab_hash_build.cpp, probe/slab_probe.cpp, join/slab_join.cpp) over the lock-free slab table
// of csrc/slab.hip.  Sizing: calculate_buckets_count(n, 60) = n / 20 buckets (at least 1: the reference takes % 0
// below 20 rows) and a pool of as many nodes, the reference's 2 * buckets heap with the roots preallocated, plus
// DBHIP_SLAB_INSERT_GROUPS nodes: the reference appends under a lock and wastes no node, while a lock-free append can
// leave one unlinked node per row group, and on SlabHashBuild's hot chains below about 2^22 rows those spares alone
// would exhaust a pool of `buckets` nodes (measured at 2^16 rows).  Hasher:
// DefaultHasher<242792921, 653019598, 2147483647>.  The table is reset (the reference builds its AllocAdapter) before
// host_start, untimed.  A build that reports DBHIP_DEV_TABLE_FULL is "Incorrect results".
namespace {
constexpr uint64_t kSlabA = 242792921, kSlabB = 653019598, kSlabP = 2147483647;
size_t slab_buckets(size_t n) { return std::max<size_t>(1, n / 20); }
size_t slab_pool(size_t n) { return slab_buckets(n) + DBHIP_SLAB_INSERT_GROUPS; }

// the status word of a finished build: true = every row stored; throws on anything but TABLE_FULL
bool slab_built(const void *ws, const char *who) {
  uint32_t st = 0xFFFFFFFFu;
  db_ok(dbhip_workspace_status(ws, &st, nullptr), "dbhip_workspace_status");
  if (st != DBHIP_DEV_OK && st != DBHIP_DEV_TABLE_FULL) fail(std::string(who) + ": device status " + std::to_string(st));
  if (st == DBHIP_DEV_TABLE_FULL) std::cerr << who << ": the slab pool ran out, rows were not stored\n";
  return st == DBHIP_DEV_OK;
}
}  // namespace

// SlabHashBuildHip — hash/slab_hash_build.cpp:9-108: keys = make_random (uniform in [1, 10000], the
// dbhip_gen_uniform_u32 twin), vals = keys, so every key repeats about n / 10000 times and about 10,000 chains grow
// n / 320000 slabs long.  Timed: the insert alone (:41-64).  Then every key must be found (:66-99), here also with its
// own value.
void SlabHashBuildHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  const size_t buckets = slab_buckets(n), pool = slab_pool(n);
  if (buckets + pool > 0xFFFFFFFFull) fail("SlabHashBuildHip: too many rows for 32-bit node ids");
  DevBuf<uint32_t> keys(n), vals(n), found(n);
  db_ok(dbhip_gen_uniform_u32(keys.get(), n, kSlabUniformSeed, 0, 1, 10000, nullptr), "gen");
  const size_t ws_bytes = dbhip_slab_table_workspace_bytes(buckets, pool);
  DevBuf<unsigned char> ws(ws_bytes);
  CheckWords chk;
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    db_ok(dbhip_slab_table_reset(ws.get(), ws_bytes, buckets, pool, nullptr), "dbhip_slab_table_reset");
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_slab_table_insert_u32(keys.get(), keys.get(), n, ws.get(), ws_bytes, buckets, pool, kSlabA, kSlabB,
                                        kSlabP, 0, nullptr, nullptr),
            "dbhip_slab_table_insert_u32");
    });
    bool ok = slab_built(ws.get(), "SlabHashBuildHip");
    if (ok && n) {
      db_ok(dbhip_slab_table_lookup_u32(keys.get(), n, ws.get(), buckets, pool, kSlabA, kSlabB, kSlabP, vals.get(),
                                        found.get(), nullptr),
            "dbhip_slab_table_lookup_u32");
      hip_ok(hipStreamSynchronize(nullptr), "sync");
      if (inject_fault()) poke_xor(vals.get() + n / 2, 1u);
      ok = found_own_keys(keys, vals, found, n, true, {}, chk);
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// SlabProbeHip — probe/slab_probe.cpp:9-107: unique keys (make_unique_random twin), vals = keys, built untimed; timed:
// the lookups of the same keys, every one of which must be found (:100-103), here also with its own value.
void SlabProbeHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  require_unique_keys_fit(n, name());
  const size_t buckets = slab_buckets(n), pool = slab_pool(n);
  DevBuf<uint32_t> keys(n), vals(n), found(n);
  db_ok(dbhip_gen_unique_sorted_u32(keys.get(), n, 11, 0, nullptr), "gen");  // slab_probe.cpp:17
  const size_t ws_bytes = dbhip_slab_table_workspace_bytes(buckets, pool);
  DevBuf<unsigned char> ws(ws_bytes);
  CheckWords chk;
  std::array<uint64_t, 4> key_fp{};
  if (n > validate_limit()) {
    db_ok(dbhip_check_sorted_u32(keys.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    key_fp = chk.get();
  }
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    // build: untimed, a fresh table every iteration like the reference's AllocAdapter (:26-62)
    db_ok(dbhip_slab_table_reset(ws.get(), ws_bytes, buckets, pool, nullptr), "dbhip_slab_table_reset");
    db_ok(dbhip_slab_table_insert_u32(keys.get(), keys.get(), n, ws.get(), ws_bytes, buckets, pool, kSlabA, kSlabB,
                                      kSlabP, 0, nullptr, nullptr),
          "dbhip_slab_table_insert_u32");
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_slab_table_lookup_u32(keys.get(), n, ws.get(), buckets, pool, kSlabA, kSlabB, kSlabP, vals.get(),
                                        found.get(), nullptr),
            "dbhip_slab_table_lookup_u32");
    });
    bool ok = slab_built(ws.get(), "SlabProbeHip");
    if (ok && n) {
      if (inject_fault()) poke_xor(vals.get() + n / 2, 1u);
      ok = found_own_keys(keys, vals, found, n, false, key_fp, chk);
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// SlabJoinHip — join/slab_join.cpp:10-144: unique sorted keys and unique sorted values on both sides (the
// make_unique_random twin, the seeds of JoinHip), build and probe timed separately (HashJoinResult).  The reference
// fixes 1024 buckets, a 20000-node heap and the hasher <32, 48, 1031> (:37-39, :72, :100): its heap holds 640,000
// pairs and it writes past it beyond that, and at 2^24 rows its chains would be about 512 slabs long.  Here the table
// is sized like SlabHashBuild's (n / 20 buckets, a pool of as many nodes + DBHIP_SLAB_INSERT_GROUPS) with its hasher.  The probe writes per probe row
// (key, build value, probe value), all 0xFFFFFFFF on a miss (dbhip_ujoin_probe_u32's convention): the reference
// compacts by key != 0 (:127) and drops a real key 0.  Checked like JoinHip, against seq_join's table.
void SlabJoinHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  require_unique_keys_fit(n, name());
  const size_t buckets = slab_buckets(n), pool = slab_pool(n);
  UniqueJoinBuffers buf(n, dbhip_slab_table_workspace_bytes(buckets, pool));
  Events build_ev, probe_ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    db_ok(dbhip_slab_table_reset(buf.ws.get(), buf.ws_bytes, buckets, pool, nullptr), "dbhip_slab_table_reset");
    hip_ok(hipStreamSynchronize(nullptr), "sync");
    auto result = std::make_unique<HashJoinResult>();
    time_build_probe(
        *result, build_ev, probe_ev,
        [&] {
          db_ok(dbhip_slab_table_insert_u32(buf.ak.get(), buf.av.get(), n, buf.ws.get(), buf.ws_bytes, buckets, pool,
                                            kSlabA, kSlabB, kSlabP, 0, nullptr, nullptr),
                "dbhip_slab_table_insert_u32");
        },
        [&] {
          db_ok(dbhip_slab_table_join_probe_u32(buf.bk.get(), buf.bv.get(), n, buf.ws.get(), buckets, pool, kSlabA,
                                                kSlabB, kSlabP, buf.ok_.get(), buf.o1.get(), buf.o2.get(), nullptr),
                "dbhip_slab_table_join_probe_u32");
        });
    bool ok = slab_built(buf.ws.get(), "SlabJoinHip");
    if (inject_fault() && n) poke_xor(buf.o1.get() + n / 2, 1u);
    record(meter, n, std::move(result), ok && buf.check(), "Incorrect results");
  }
}

// =====================================================================================================
// PartitionedJoinHip — the radix-partitioned hash join of SURVEY 8(e) behind the Dwarf hook: one process driving
// `--gpus P` ranks through pjoin::Engine (pjoin_engine.hpp: per-rank compute and exchange streams, counts by
// ncclAllGather, exchange of R overlapping partition S, exchange of S overlapping build R).  No reference
// counterpart; JoinOmnisci semantics (join/join_omnisci.cpp:49-118).  `buf_size` rows per relation IN TOTAL; rank r
// owns the contiguous shard [r*n/P, (r+1)*n/P) of both key columns, generated in place on its GPU.
// Ranks on distinct GPUs exchange through ONE RCCL group of ncclSend/ncclRecv per relation; more ranks than GPUs
// (rehearsal on one GPU; DWARF_BENCH_PJOIN_EXCHANGE=copy forces it) share devices and push with hipMemcpyPeerAsync.
// DWARF_BENCH_PJOIN_DIRECT=1 with --gpus 1: the plain local join (the P = 1 point of a scaling curve).
// The local join of every rank is the radix join (dbhip_join_radix_*: received pairs partitioned once more, fused LDS
// build + probe, no table in HBM).
// HashJoinResult: build_time = start -> every rank's build done, probe_time = the rest; the phase lines printed per
// iteration are device-event spans (max over ranks) and overlap by design.
// Checks, every iteration and at every size, on the device: the exchange conserves the four columns (wrap-around
// sums sent == received), every received pair is what the generator produced for its row id, every received key
// hashes to the receiving rank, every probe row's count equals the key's multiplicity among the rank's build keys
// and its ids carry the key.  Up to DWARF_BENCH_VALIDATE_MAX rows additionally on the host against per-key counts
// of the whole build column (all rows of a key must have met on ONE rank).
#include "pjoin_engine.hpp"

void PartitionedJoinHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  pjoin::Options po;
  po.world = static_cast<unsigned>(opts.devices ? opts.devices : 1);
  const char *force = std::getenv("DWARF_BENCH_PJOIN_EXCHANGE");
  po.force_copy = force && std::string(force) == "copy";
  po.direct_single = env_flag("DWARF_BENCH_PJOIN_DIRECT");
  int ndev = 0;
  hip_ok(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
  pjoin::Engine engine(n, po);
  const unsigned P = engine.world();
  std::cout << "PartitionedJoinHip: " << P << " rank(s) on " << std::min<int>(P, ndev) << " GPU(s), exchange by "
            << (engine.uses_rccl() ? "RCCL send/recv group"
                                   : (po.direct_single && P == 1 ? "nothing (direct local join)" : "hipMemcpyPeerAsync"))
            << (engine.sub_joins() > 1 ? ", " + std::to_string(engine.sub_joins()) + " pipelined sub-joins" : std::string()) << "\n";
  engine.plan();

  // host copy of the global columns for the host-side check
  const bool host_check = n <= validate_limit();
  std::vector<uint32_t> build_all, probe_all;
  std::unordered_map<uint32_t, uint32_t> key_count;
  if (host_check) {
    for (unsigned r = 0; r < engine.local_ranks(); ++r) {
      const auto b = engine.download_column(r, true), p = engine.download_column(r, false);
      build_all.insert(build_all.end(), b.begin(), b.end());
      probe_all.insert(probe_all.end(), p.begin(), p.end());
    }
    for (uint32_t k : build_all) ++key_count[k];
  }

  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<HashJoinResult>();
    const pjoin::StepTimes t = engine.step();
    result->host_time = Duration(t.total);
    result->build_time = Duration(t.until_build_done);
    result->probe_time = Duration(t.total - t.until_build_done);
    result->kernel_time = Duration(t.total);  // no single device timeline spans the ranks
    std::cout << "Partition time: " << t.partition << " us\nExchange time: " << t.exchange << " us\nLocal build time: "
              << t.build << " us\nLocal probe time: " << t.probe << " us\n";
    if (inject_fault() && n) engine.corrupt_one_count();
    const pjoin::CheckReport rep = engine.check();
    bool ok = true;
    if (!engine.conserved(rep)) {
      std::cerr << "Incorrect results (the exchange did not conserve its columns)" << std::endl;
      ok = false;
    }
    if (rep.bad_pairs || rep.bad_route || rep.bad_rows || rep.recv_build != n || rep.recv_probe != n) {
      std::cerr << "Incorrect results (device checks: " << rep.bad_pairs << " damaged pairs, " << rep.bad_route
                << " misrouted keys, " << rep.bad_rows << " wrong probe rows, " << rep.recv_build << " + " << rep.recv_probe
                << " rows delivered)" << std::endl;
      ok = false;
    }
    if (host_check && ok) {
      std::vector<char> seen(n, 0);
      size_t delivered = 0;
      uint64_t matches = 0;
      for (unsigned r = 0; r < engine.local_ranks() && ok; ++r) {
        const pjoin::Engine::HostShard h = engine.download(r);
        for (size_t i = 0; i < h.probe_keys.size() && ok; ++i) {
          const uint32_t rid = h.probe_row_ids[i], key = h.probe_keys[i];
          ok = rid < n && !seen[rid] && probe_all[rid] == key;  // every probe row arrives once, intact
          if (!ok) break;
          seen[rid] = 1;
          ++delivered;
          const auto f = key_count.find(key);
          const uint32_t want = f == key_count.end() ? 0u : f->second;
          ok = h.cnt[i] == want && static_cast<size_t>(h.pos[i]) + h.cnt[i] <= h.ids.size();  // all rows of the key met here
          matches += h.cnt[i];
          const uint32_t stepj = h.cnt[i] > 64 ? h.cnt[i] / 64 : 1;
          for (uint32_t j = 0; ok && j < h.cnt[i]; j += stepj) {
            const uint32_t id = h.ids[h.pos[i] + j];
            ok = id < n && build_all[id] == key;
          }
        }
      }
      if (!ok || delivered != n || matches != rep.matches) {
        std::cerr << "Incorrect results" << std::endl;
        ok = false;
      }
    }
    record(meter, n, std::move(result), ok, nullptr);  // the lines above said what failed
  }
}

// =====================================================================================================
// GroupByHashHip — GROUP BY key SUM(val), COUNT(*) over sparse keys (dbhip_groupby_hash_u32): vals uniform in [1, 10000]
// as GroupByHip's, keys = the low 32 bits of mix64 of a uniform draw from [0, groups_count) — groups_count values (a few
// fewer where two draws mix to one word) spread over the whole uint32 range.  max_groups = groups_count.  Result::valid
// from the device validators: distinct output keys, the weighted sums of (out_keys, out_sums) and of (out_keys,
// out_counts) equal those of (keys, vals) and of (keys, ones), and the counts sum to n.
void GroupByHashHip::_run(const size_t n, Meter &meter) {
  const auto &opts = static_cast<const GroupByRunOptions &>(meter.opts());
  if (n > (static_cast<size_t>(1) << 31)) fail("GroupByHashHip: at most 2^31 rows");
  const uint32_t groups = static_cast<uint32_t>(opts.groups_count ? opts.groups_count : 1);
  const size_t cap = std::max<size_t>(std::min<size_t>(groups, n), 1);
  DevBuf<uint32_t> keys(n), vals(n), ones(n), draw(n), out_keys(cap), out_sums(cap), out_counts(cap);
  DevBuf<uint64_t> out_groups(1);
  const size_t ws_bytes = dbhip_groupby_hash_workspace_bytes(n, groups);
  DevBuf<unsigned char> ws(ws_bytes);
  const size_t dws_bytes = dbhip_check_distinct_workspace_bytes(cap);
  DevBuf<unsigned char> dws(dws_bytes);
  db_ok(dbhip_gen_uniform_u32(vals.get(), n, 43, 0, 1, 10000, nullptr), "gen vals");
  db_ok(dbhip_gen_uniform_u32(draw.get(), n, 42, 0, 0, groups - 1, nullptr), "gen draw");
  db_ok(dbhip_gen_uniform_at_u32(keys.get(), draw.get(), n, 44, 0, 0xFFFFFFFFu, nullptr), "gen keys");
  db_ok(dbhip_gen_uniform_u32(ones.get(), n, 0, 0, 1, 1, nullptr), "gen ones");
  CheckWords chk;
  db_ok(dbhip_check_weighted_sum_u32(keys.get(), vals.get(), n, chk.dev(), nullptr), "dbhip_check_weighted_sum_u32");
  const auto want_sums = chk.get();
  db_ok(dbhip_check_weighted_sum_u32(keys.get(), ones.get(), n, chk.dev(), nullptr), "dbhip_check_weighted_sum_u32");
  const auto want_counts = chk.get();
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_groupby_hash_u32(keys.get(), vals.get(), n, groups, out_keys.get(), out_sums.get(), out_counts.get(),
                                   out_groups.get(), ws.get(), ws_bytes, nullptr),
            "dbhip_groupby_hash_u32");
    });
    check_status(ws.get(), "GroupByHashHip");
    const size_t g = static_cast<size_t>(out_groups.to_host(1)[0]);
    if (inject_fault() && g) poke_xor(out_sums.get() + g / 2, 1u);
    bool ok = g <= cap;
    if (ok) {
      db_ok(dbhip_check_weighted_sum_u32(out_keys.get(), out_sums.get(), g, chk.dev(), nullptr), "dbhip_check_weighted_sum_u32");
      const auto s = chk.get();
      db_ok(dbhip_check_weighted_sum_u32(out_keys.get(), out_counts.get(), g, chk.dev(), nullptr), "dbhip_check_weighted_sum_u32");
      const auto c = chk.get();
      db_ok(dbhip_check_distinct_u32(out_keys.get(), g, chk.dev(), dws.get(), dws_bytes, nullptr), "dbhip_check_distinct_u32");
      const auto d = chk.get();
      uint64_t total = 0;  // the counts sum to n: summed on the host (g words, at most groups_count)
      for (uint32_t x : out_counts.to_host(g)) total += x;
      ok = s[0] == want_sums[0] && s[1] == want_sums[1] && c[0] == want_counts[0] && c[1] == want_counts[1] && d[0] == 0 &&
           total == n;
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// GroupBySortedHip — GROUP BY key ORDER BY key with COUNT, 64-bit SUM, MIN, MAX: the stable pairs sort
// (dbhip_radix_sort_pairs_u32, the values travel with the keys) and dbhip_reduce_by_key_u32 behind it
// (include/dbhip_reduce_by_key.h).  Keys and values as GroupByHashHip's; the timed region is the sort plus the reduce, the
// columns are copied afresh outside it (the sort works in place).  Result::valid from dbhip_check_reduce_by_key_u32 on the
// sorted columns, the sort's own check on the keys, and the number of runs against the bound.  No reference counterpart.
void GroupBySortedHip::_run(const size_t n, Meter &meter) {
  const auto &opts = static_cast<const GroupByRunOptions &>(meter.opts());
  if (n >= (static_cast<size_t>(1) << 32)) fail("GroupBySortedHip: fewer than 2^32 rows");
  const uint32_t groups = static_cast<uint32_t>(opts.groups_count ? opts.groups_count : 1);
  const size_t cap = std::max<size_t>(std::min<size_t>(groups, n), 1);
  DevBuf<uint32_t> src_keys(n), src_vals(n), draw(n), keys(n), vals(n), tmp_keys(n), tmp_vals(n);
  DevBuf<uint32_t> out_keys(cap), out_counts(cap), out_mins(cap), out_maxs(cap);
  DevBuf<uint64_t> out_sums(cap), out_runs(1);
  const size_t sort_bytes = dbhip_radix_sort_pairs_workspace_bytes(n, 8);
  const size_t ws_bytes = dbhip_reduce_by_key_workspace_bytes(n);
  const size_t cws_bytes = dbhip_check_reduce_by_key_workspace_bytes(n, cap);
  DevBuf<unsigned char> sort_ws(sort_bytes), ws(ws_bytes), cws(cws_bytes);
  db_ok(dbhip_gen_uniform_u32(src_vals.get(), n, 43, 0, 1, 10000, nullptr), "gen vals");
  db_ok(dbhip_gen_uniform_u32(draw.get(), n, 42, 0, 0, groups - 1, nullptr), "gen draw");
  db_ok(dbhip_gen_uniform_at_u32(src_keys.get(), draw.get(), n, 44, 0, 0xFFFFFFFFu, nullptr), "gen keys");
  hip_ok(hipDeviceSynchronize(), "sync");
  CheckWords chk;
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    hip_ok(hipMemcpy(keys.get(), src_keys.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "refresh");  // not timed
    hip_ok(hipMemcpy(vals.get(), src_vals.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "refresh");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_radix_sort_pairs_u32(keys.get(), vals.get(), tmp_keys.get(), tmp_vals.get(), n, 8, 0, sort_ws.get(),
                                       sort_bytes, nullptr),
            "dbhip_radix_sort_pairs_u32");
      db_ok(dbhip_reduce_by_key_u32(keys.get(), vals.get(), n, 0, out_keys.get(), out_counts.get(), out_sums.get(),
                                    out_mins.get(), out_maxs.get(), cap, out_runs.get(), ws.get(), ws_bytes, nullptr),
            "dbhip_reduce_by_key_u32");
    });
    if (n) check_status(sort_ws.get(), "GroupBySortedHip");
    if (n) check_status(ws.get(), "GroupBySortedHip");
    const size_t runs = n ? static_cast<size_t>(out_runs.to_host(1)[0]) : 0;
    if (inject_fault() && runs) poke_xor(out_sums.get() + runs / 2, 1u);  // the low word of one sum
    bool ok = runs <= cap;
    if (ok) {  // sorted keys (so equal keys are one run), and the table is the reduce of the sorted columns
      db_ok(dbhip_check_sorted_u32(keys.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
      const auto srt = chk.get();
      db_ok(dbhip_check_reduce_by_key_u32(keys.get(), vals.get(), n, 0, out_keys.get(), out_counts.get(), out_sums.get(),
                                          out_mins.get(), out_maxs.get(), runs, chk.dev(), cws.get(), cws_bytes, nullptr),
            "dbhip_check_reduce_by_key_u32");
      const auto g = chk.get();
      ok = srt[0] == 0 && g[0] == 0 && g[1] == 0 && g[2] == g[3];
    }
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// WindowSortedHip — ROW_NUMBER, running 64-bit SUM, MIN, MAX and the run number over PARTITION BY key ORDER BY row: the
// stable pairs sort (dbhip_radix_sort_pairs_u32, the values travel with the keys) and dbhip_scan_by_key_u32 behind it
// (include/dbhip_scan_by_key.h).  Keys and values as GroupBySortedHip's; the timed region is the sort plus the scan, the
// columns are copied afresh outside it (the sort works in place).  Result::valid from the sort's own check on the keys and
// dbhip_check_scan_by_key_u32 on the sorted columns.  No reference counterpart.
void WindowSortedHip::_run(const size_t n, Meter &meter) {
  const auto &opts = static_cast<const GroupByRunOptions &>(meter.opts());
  if (n >= (static_cast<size_t>(1) << 32)) fail("WindowSortedHip: fewer than 2^32 rows");
  const uint32_t groups = static_cast<uint32_t>(opts.groups_count ? opts.groups_count : 1);
  DevBuf<uint32_t> src_keys(n), src_vals(n), draw(n), keys(n), vals(n), tmp_keys(n), tmp_vals(n);
  DevBuf<uint32_t> run_ids(n), row_numbers(n), mins(n), maxs(n);
  DevBuf<uint64_t> sums(n);
  const size_t sort_bytes = dbhip_radix_sort_pairs_workspace_bytes(n, 8);
  const size_t ws_bytes = dbhip_scan_by_key_workspace_bytes(n);
  const size_t cws_bytes = dbhip_check_scan_by_key_workspace_bytes(n);
  DevBuf<unsigned char> sort_ws(sort_bytes), ws(ws_bytes), cws(cws_bytes);
  db_ok(dbhip_gen_uniform_u32(src_vals.get(), n, 43, 0, 1, 10000, nullptr), "gen vals");
  db_ok(dbhip_gen_uniform_u32(draw.get(), n, 42, 0, 0, groups - 1, nullptr), "gen draw");
  db_ok(dbhip_gen_uniform_at_u32(src_keys.get(), draw.get(), n, 44, 0, 0xFFFFFFFFu, nullptr), "gen keys");
  hip_ok(hipDeviceSynchronize(), "sync");
  CheckWords chk;
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    hip_ok(hipMemcpy(keys.get(), src_keys.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "refresh");  // not timed
    hip_ok(hipMemcpy(vals.get(), src_vals.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "refresh");
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] {
      db_ok(dbhip_radix_sort_pairs_u32(keys.get(), vals.get(), tmp_keys.get(), tmp_vals.get(), n, 8, 0, sort_ws.get(),
                                       sort_bytes, nullptr),
            "dbhip_radix_sort_pairs_u32");
      db_ok(dbhip_scan_by_key_u32(keys.get(), vals.get(), n, 0, run_ids.get(), row_numbers.get(), sums.get(), mins.get(),
                                  maxs.get(), ws.get(), ws_bytes, nullptr),
            "dbhip_scan_by_key_u32");
    });
    if (n) check_status(sort_ws.get(), "WindowSortedHip");
    if (n) check_status(ws.get(), "WindowSortedHip");
    if (inject_fault() && n) poke_xor(sums.get() + n / 2, 1u);  // the low word of one sum
    // sorted keys (so equal keys are one run), and every row continues the row above it
    db_ok(dbhip_check_sorted_u32(keys.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    const auto srt = chk.get();
    db_ok(dbhip_check_scan_by_key_u32(keys.get(), vals.get(), n, 0, run_ids.get(), row_numbers.get(), sums.get(), mins.get(),
                                      maxs.get(), chk.dev(), cws.get(), cws_bytes, nullptr),
          "dbhip_check_scan_by_key_u32");
    const auto w = chk.get();
    const bool ok = srt[0] == 0 && w[0] == 0 && w[1] == ~0ull && w[3] == 0;
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}

// =====================================================================================================
// RangeJoinHip — the band join b.key BETWEEN p.lo AND p.hi as a table of (build row, probe row) pairs: the stable pairs sort
// of the build keys on row ids, the fence ladder over the sorted keys and the search of include/dbhip_sorted_search.h, then
// dbhip_join_pairs_u32 in probe-row order.  n rows a side; build keys and probe lo uniform in [1, max(10000, n)] from
// JoinPairsHip's seeds, hi = lo + W saturating, W from DWARF_BENCH_RANGE_WIDTH (default 2).  The timed region is the sort,
// the index build, the search and the expansion, with the capacity an untimed count-only pass returned; the keys are copied
// afresh outside it (the sort works in place).  Result::valid from dbhip_check_sorted_u32 on the sorted keys,
// dbhip_check_sorted_search_u32 on (pos, cnt) and *out_pairs == its pair total.  No reference counterpart.
void RangeJoinHip::_run(const size_t n, Meter &meter) {
  const RunOptions &opts = meter.opts();
  if (n == 0 || n > (static_cast<size_t>(1) << 31)) fail("RangeJoinHip: between 1 and 2^31 rows a side");
  uint32_t width = 2;
  if (const char *w = std::getenv("DWARF_BENCH_RANGE_WIDTH")) width = static_cast<uint32_t>(std::strtoul(w, nullptr, 10));
  DevBuf<uint32_t> src(n), keys(n), ids(n), tmp_keys(n), tmp_ids(n), lo(n), hi(n), pos(n), cnt(n);
  const size_t sort_bytes = dbhip_radix_sort_pairs_workspace_bytes(n, 8);
  const size_t index_bytes = dbhip_sorted_index_workspace_bytes(n, 0);
  const size_t pairs_bytes = dbhip_join_pairs_workspace_bytes(n);
  const size_t check_bytes = dbhip_check_sorted_search_workspace_bytes(n);
  DevBuf<unsigned char> sort_ws(sort_bytes), index_ws(index_bytes), pairs_ws(pairs_bytes), check_ws(check_bytes);
  DevBuf<uint64_t> total(1);
  const uint32_t key_hi = static_cast<uint32_t>(std::max<size_t>(10000, n));
  db_ok(dbhip_gen_uniform_u32(src.get(), n, 42, 0, 1, key_hi, nullptr), "gen build keys");
  db_ok(dbhip_gen_uniform_u32(lo.get(), n, 43, 0, 1, key_hi, nullptr), "gen probe lo");
  {
    auto h = lo.to_host(n);
    for (auto &v : h) v = v > 0xFFFFFFFFu - width ? 0xFFFFFFFFu : v + width;  // saturating
    hip_ok(hipMemcpy(hi.get(), h.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice), "probe hi");
  }
  const auto refresh = [&] {
    hip_ok(hipMemcpy(keys.get(), src.get(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "refresh");
  };
  const auto join = [&](uint64_t capacity, uint32_t *out_b, uint32_t *out_p) {
    db_ok(dbhip_radix_sort_pairs_u32(keys.get(), ids.get(), tmp_keys.get(), tmp_ids.get(), n, 8, 1, sort_ws.get(), sort_bytes,
                                     nullptr),
          "dbhip_radix_sort_pairs_u32");
    db_ok(dbhip_sorted_index_build_u32(keys.get(), n, 0, 0, index_ws.get(), index_bytes, nullptr),
          "dbhip_sorted_index_build_u32");
    db_ok(dbhip_sorted_search_u32(keys.get(), n, lo.get(), hi.get(), n, pos.get(), cnt.get(), index_ws.get(), index_bytes,
                                  nullptr),
          "dbhip_sorted_search_u32");
    db_ok(dbhip_join_pairs_u32(ids.get(), n, nullptr, pos.get(), cnt.get(), n, 0, capacity, out_b, out_p, total.get(),
                               pairs_ws.get(), pairs_bytes, nullptr),
          "dbhip_join_pairs_u32");
  };
  const auto statuses = [&] {
    check_status(sort_ws.get(), "RangeJoinHip");
    check_status(index_ws.get(), "RangeJoinHip");
    check_status(pairs_ws.get(), "RangeJoinHip");
  };
  refresh();
  join(0, nullptr, nullptr);  // not timed: the count-only pass that sizes the output
  statuses();
  const uint64_t capacity = total.to_host(1)[0];
  DevBuf<uint32_t> out_b(capacity), out_p(capacity);
  CheckWords chk;
  Events ev;
  for (size_t it = 0; it < opts.iterations; ++it) {
    refresh();  // not timed
    auto result = std::make_unique<Result>();
    time_launch(*result, ev, [&] { join(capacity, out_b.get(), out_p.get()); });
    statuses();
    if (inject_fault()) poke_xor(cnt.get() + n / 2, 1u);  // one row's interval length
    db_ok(dbhip_check_sorted_u32(keys.get(), n, 0, chk.dev(), nullptr), "dbhip_check_sorted_u32");
    const auto srt = chk.get();
    db_ok(dbhip_check_sorted_search_u32(keys.get(), n, 0, lo.get(), hi.get(), n, pos.get(), cnt.get(), chk.dev(),
                                        check_ws.get(), check_bytes, nullptr),
          "dbhip_check_sorted_search_u32");
    const auto w = chk.get();
    const bool ok = srt[0] == 0 && w[0] == 0 && w[1] == ~0ull && w[3] == 0 && total.to_host(1)[0] == w[2] && w[2] == capacity;
    record(meter, n, std::move(result), ok, "Incorrect results");
  }
}
