// errors.hpp — internal to the host layer (hip_dwarfs.cpp, pjoin_engine.cpp): a failed HIP or libdbhip call becomes a
// DwarfBenchException that names the call.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "bench.hpp"

namespace dbench_errors {

[[noreturn]] inline void fail(const std::string &what) { throw DwarfBench::DwarfBenchException(what); }
inline void hip_ok(hipError_t e, const char *what) {
  if (e != hipSuccess) fail(std::string(what) + ": " + hipGetErrorString(e));
}
inline void db_ok(int rc, const char *what) {
  if (rc != 0) fail(std::string(what) + " failed with status " + std::to_string(rc));
}

}  // namespace dbench_errors
