// rowlist.cpp — the one scan of the row-id operators (rowlist.hpp): the selection vectors and the packed filter scan
// their segments' match counts with it, the set operations their tiles' kept counts.
#include "rowlist.hpp"

namespace dbhip {
namespace {

constexpr int kScanThreads = 256;  // four counts each: 1024 segments or tiles a round

// one workgroup: cnt[i] -> pos[i] = the counts in front of i; *out_count = all of them, at most `bound`.
// Every caller pads both arrays to 256 bytes in its workspace layout (sel_layout, mp_layout, bitpack_layout): the
// 16-byte accesses below rely on it, a thread's four entries are always inside the arrays.
__global__ __launch_bounds__(kScanThreads) void rowlist_scan_kernel(const unsigned *__restrict__ cnt,
                                                                    unsigned *__restrict__ pos, size_t n,
                                                                    unsigned long long bound, unsigned long long *out_count) {
  __shared__ unsigned s_wsum[kScanThreads / kWave];
  // total of the rounds so far (the same in every thread).  The counts of a call add up to its candidates or merged
  // elements, fewer than 2^32, so no sum here leaves 32 bits, whatever the inputs hold
  unsigned run = 0;
  for (size_t base = 0; base < n; base += 4 * kScanThreads) {
    const size_t i = base + 4 * threadIdx.x;
    u32x4 c = {0u, 0u, 0u, 0u};
    if (i < n) {
      c = *reinterpret_cast<const u32x4 *>(cnt + i);
      if (i + 1 >= n) c.y = 0u;
      if (i + 2 >= n) c.z = 0u;
      if (i + 3 >= n) c.w = 0u;
    }
    unsigned round_total;
    const unsigned first = run + block_exclusive_scan<kScanThreads>(c.x + c.y + c.z + c.w, s_wsum, round_total);
    if (i < n) *reinterpret_cast<u32x4 *>(pos + i) = u32x4{first, first + c.x, first + c.x + c.y, first + c.x + c.y + c.z};
    run += round_total;
  }
  // of unsorted inputs the set operations can count an element in two tiles: the count stays within the output's room
  if (threadIdx.x == 0) *out_count = run < bound ? run : bound;
}

}  // namespace

void launch_rowlist_scan(const unsigned *cnt, unsigned *pos, size_t n, u64 bound, u64 *out_count, hipStream_t s) {
  hipLaunchKernelGGL(rowlist_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, cnt, pos, n, bound, out_count);
}

}  // namespace dbhip
