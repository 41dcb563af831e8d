// What the scan layer (scan_*.h) and the merge layer (merge_rows.h,
// sort_rows.h, unify_strings.h, partition_rows.h, encode_table.h,
// render_points.h) share, and nothing else: the hash
// finisher, the relaxed atomics of the claim-and-publish tables, and the
// segment search.  The first part is plain C++17 under a host compiler
// (scan_text.h includes it); the second is device only.
#pragma once
#include "common.h"

namespace dn {

constexpr uint64_t FNV_OFFSET = 0xCBF29CE484222325ull;

DN_HD_INLINE uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33; return x;
}

#if defined(__HIPCC__)

#define DEV __device__ __forceinline__

template <typename T>
DEV T atomic_load_relaxed(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
DEV void atomic_store_relaxed(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV void drain_stores() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Ordinal of the segment (index file, sending rank) that row r belongs
// to: the last f with seg_start[f] <= r.  Empty segments repeat a value
// and are never chosen (their successor starts at the same row).
// seg_start is a few KB at most, shared by every row: it stays in L2.
DEV uint32_t file_ordinal(const uint32_t* seg_start, uint32_t nfiles,
                          uint32_t r) {
  uint32_t lo = 0, hi = nfiles;  // seg_start[lo] <= r < seg_start[hi]
  while (hi - lo > 1) {
    uint32_t mid = lo + ((hi - lo) >> 1);
    if (seg_start[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

#endif  // __HIPCC__

}  // namespace dn
