// The edge-weighted pick shared by random_walk and sample_adj (weighted.hip), in plain C++
// so that the host export psa_weighted_pick_host runs the very text the kernels run.
//
// cum[0 .. deg) is one row of psa_row_cdf: the inclusive left-to-right float64 prefix sum
// of the row's weights, non-decreasing, with cum[e] == cum[e-1] exactly where w[e] == 0.
// The random word r is the word rand_draw (rng.h) turns into an index; here it becomes
// u = (r >> 11) * 2^-53 in [0, 1) and target = u * total (ONE rounded multiply), and the
// pick is the smallest e with cum[e] > target: cum[pick-1] <= target < cum[pick], hence
// w[pick] > 0.  target < total whenever total is a normal number; for a subnormal total
// the product can round up to total, and the pick is then the smallest e with
// cum[e] == total (the last entry of positive weight).  Both searches halve [lo, hi) at
// most 64 times by construction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSA_PICK_FN __host__ __device__ inline
#else
#define PSA_PICK_FN inline
#endif

namespace psa {

// Index in [0, deg) of the pick (deg > 0), or -1 when the row's total is not positive.
PSA_PICK_FN int64_t weighted_pick(const double* cum, int64_t deg, uint64_t r) {
#if defined(__clang__)
#pragma clang fp contract(off)  // target is a product rounded once, never part of an fma
#endif
  const double total = cum[deg - 1];
  if (!(total > 0.0)) return -1;
  const double u = static_cast<double>(r >> 11) * 0x1p-53;
  const double target = u * total;
  int64_t lo = 0, hi = deg;  // smallest e with cum[e] > target, deg for none
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  if (lo < deg) return lo;
  lo = 0, hi = deg;  // target rounded up to total: smallest e with cum[e] == total
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] >= total) hi = mid;
    else lo = mid + 1;
  }
  return lo < deg ? lo : deg - 1;  // never past the row, whatever cum holds
}

}  // namespace psa
