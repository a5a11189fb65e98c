// The searches in non-decreasing int64 arrays that the samplers and the graph ops share: which
// row owns slot p of a scanned count (wave_search by a whole wave, last_le by one lane) and
// where a sorted row stores a column (first_equal).  The one-lane forms are plain C++, so a
// `_host` export runs the very text the kernels run, and halve at most 64 times: no loop here
// depends on its input being sorted to terminate.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rng.h"

namespace psa {

// Largest r in [lo, hi) with ptr[r] <= p, given ptr[lo] <= p; called by a whole wave (64
// probes per step: 4 dependent loads for 2^24 rows).
__device__ __forceinline__ int64_t wave_search(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t p) {
  const int lane = threadIdx.x & 63;
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t x = lo + lane * step;
    const bool ok = x < hi && ptr[x] <= p;
    const int cnt = __popcll(__ballot(ok));  // lanes [0, cnt) hold: ptr is non-decreasing
    const int64_t nhi = lo + cnt * step;
    lo += (cnt - 1) * step;
    hi = nhi < hi ? nhi : hi;
  }
  return lo;
}

// Largest r in [lo, hi) with ptr[r] <= p, given ptr[lo] <= p; one lane.
PSA_HD int64_t last_le(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t p) {
  for (int i = 0; i < 64 && hi - lo > 1; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Position of the first entry of a[lo .. hi) equal to x, or -1: a lower bound, so of a
// duplicated entry it is the FIRST.
PSA_HD int64_t first_equal(const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
  const int64_t end = hi;
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && a[lo] == x ? lo : -1;
}

}  // namespace psa
