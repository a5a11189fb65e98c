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

// ---- successive weighted picks WITHOUT replacement, on the row CDF alone ----
//
// The n positions taken so far, ascending, cut the row into n + 1 gaps; the mass of a gap is
// the difference of the cum entries at its two ends (0.0 below the row's first entry), so it
// is exactly 0 when the gap holds no entry of positive weight and positive otherwise.  A
// draw first chooses a gap in proportion to the masses (stage 1: word words.gap(t), none at
// draw 0, where there is one gap), then an entry inside it as weighted_pick does (stage 2:
// word words.entry(t)).  Draw 0 is weighted_pick(cum, deg, words.entry(0)) bit for bit.  The
// draws end when no mass is left: a row yields min(k, entries of positive weight) picks, all
// distinct, none of weight zero.  Every loop is bounded by k, by k + 1 gaps or by 64 halvings.
// Row totals so large that the sum of the gap masses overflows are not supported.

namespace psa {

// Words given explicitly (the host export).
struct PickWordArrays {
  const uint64_t* entry_words;
  const uint64_t* gap_words;
  PSA_PICK_FN uint64_t entry(int64_t t) const { return entry_words[t]; }
  PSA_PICK_FN uint64_t gap(int64_t t) const { return gap_words[t]; }
};

// Stage 2: the pick among positions [lo, hi) of the row, base = cum[lo - 1] (0.0 for lo == 0),
// top = cum[hi - 1], mass = top - base > 0.
PSA_PICK_FN int64_t weighted_pick_gap(const double* cum, int64_t lo0, int64_t hi0, double base, double top,
                                      double mass, uint64_t r) {
#if defined(__clang__)
#pragma clang fp contract(off)  // one rounded multiply, then one rounded add
#endif
  const double u = static_cast<double>(r >> 11) * 0x1p-53;
  const double part = u * mass;
  const double target = base + part;
  int64_t lo = lo0, hi = hi0;  // smallest e with cum[e] > target, hi0 for none
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  if (lo < hi0) return lo;
  lo = lo0, hi = hi0;  // target rounded up to top: smallest e with cum[e] == top
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] >= top) hi = mid;
    else lo = mid + 1;
  }
  return lo < hi0 ? lo : hi0 - 1;
}

// The stage-1 target of draw t: u1 * total, one rounded multiply.
PSA_PICK_FN double weighted_gap_target(double total, uint64_t r1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double u1 = static_cast<double>(r1 >> 11) * 0x1p-53;
  return u1 * total;
}

// k <= KMAX picks of a row of deg <= INT32_MAX entries into out[0 .. count), in draw order,
// as indices in [0, deg); returns count.  The taken positions and the gap masses live in
// arrays whose every index is static once the inner loops are unrolled (registers on the
// device); inserting a pick splits one mass in two, which gives the bits a fresh difference
// of the gap's ends would give.
template <int KMAX, class Words>
PSA_PICK_FN int64_t weighted_pick_without_small(const double* cum, int64_t deg, int64_t k, const Words& words,
                                                int64_t* out) {
  int32_t taken[KMAX];     // ascending, [0, n)
  double mass[KMAX + 1];   // of gap g = (taken[g-1], taken[g]), [0, n]
#pragma unroll
  for (int j = 0; j < KMAX; ++j) taken[j] = 0;
#pragma unroll
  for (int j = 0; j <= KMAX; ++j) mass[j] = 0.0;
  mass[0] = cum[deg - 1] - 0.0;
  const int32_t d = static_cast<int32_t>(deg);
  int64_t n = 0;
#pragma unroll 1
  for (; n < k; ++n) {
    double total = 0.0;
#pragma unroll
    for (int j = 0; j <= KMAX; ++j)
      if (j <= n) total = total + mass[j];
    if (!(total > 0.0)) break;
    // stage 1: the smallest g with S_g > target, else the largest g of positive mass
    const double target = n > 0 ? weighted_gap_target(total, words.gap(n)) : 0.0;
    int g = -1, last = 0;
    int32_t lo0 = 0, hi0 = d, last_lo = 0, last_hi = d;
    double m = 0.0, last_m = 0.0, run = 0.0;
#pragma unroll
    for (int j = 0; j <= KMAX; ++j) {
      if (j <= n) {
        run = run + mass[j];
        const int32_t lo_j = j > 0 ? taken[j > 0 ? j - 1 : 0] + 1 : 0;
        const int32_t hi_j = j < n ? taken[j < KMAX ? j : KMAX - 1] : d;
        if (mass[j] > 0.0) last = j, last_m = mass[j], last_lo = lo_j, last_hi = hi_j;
        if (g < 0 && (n == 0 || run > target)) g = j, m = mass[j], lo0 = lo_j, hi0 = hi_j;
      }
    }
    if (g < 0) g = last, m = last_m, lo0 = last_lo, hi0 = last_hi;
    if (!(m > 0.0)) break;  // never with a row CDF; whatever cum holds, a chosen gap is not empty
    // stage 2
    const double base = lo0 > 0 ? cum[lo0 - 1] : 0.0;
    const double top = cum[hi0 - 1];
    const int32_t e = static_cast<int32_t>(weighted_pick_gap(cum, lo0, hi0, base, top, m, words.entry(n)));
    out[n] = e;
    const double left = e > lo0 ? cum[e - 1] - base : 0.0;
    const double right = e + 1 < hi0 ? top - cum[e] : 0.0;
    // insert e at index g: gap g becomes (left, right)
#pragma unroll
    for (int j = KMAX; j >= 1; --j) {
      if (j > g + 1) mass[j] = mass[j - 1];
      else if (j == g + 1) mass[j] = right;
    }
#pragma unroll
    for (int j = KMAX - 1; j >= 1; --j)
      if (j > g) taken[j] = taken[j - 1];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      if (j == g) taken[j] = e;
    }
#pragma unroll
    for (int j = 0; j <= KMAX; ++j)
      if (j == g) mass[j] = left;
  }
  return n;
}

// Any k >= 1 and any deg: the ascending view of the taken positions lives in sorted[0 .. k)
// (memory of the caller), the masses are differences read afresh at every draw.
template <class Words>
PSA_PICK_FN int64_t weighted_pick_without_large(const double* cum, int64_t deg, int64_t k, const Words& words,
                                                int64_t* sorted, int64_t* out) {
  int64_t n = 0;
  for (; n < k; ++n) {
    double total = 0.0;
    for (int64_t j = 0; j <= n; ++j) {
      const int64_t lo_j = j > 0 ? sorted[j - 1] + 1 : 0, hi_j = j < n ? sorted[j] : deg;
      const double m_j = hi_j > lo_j ? cum[hi_j - 1] - (lo_j > 0 ? cum[lo_j - 1] : 0.0) : 0.0;
      total = total + m_j;
    }
    if (!(total > 0.0)) break;
    const double target = n > 0 ? weighted_gap_target(total, words.gap(n)) : 0.0;
    int64_t g = -1, lo0 = 0, hi0 = deg, last = 0, last_lo = 0, last_hi = deg;
    double run = 0.0;
    for (int64_t j = 0; j <= n && g < 0; ++j) {
      const int64_t lo_j = j > 0 ? sorted[j - 1] + 1 : 0, hi_j = j < n ? sorted[j] : deg;
      const double m_j = hi_j > lo_j ? cum[hi_j - 1] - (lo_j > 0 ? cum[lo_j - 1] : 0.0) : 0.0;
      run = run + m_j;
      if (m_j > 0.0) last = j, last_lo = lo_j, last_hi = hi_j;
      if (n == 0 || run > target) g = j, lo0 = lo_j, hi0 = hi_j;
    }
    if (g < 0) g = last, lo0 = last_lo, hi0 = last_hi;  // the loop ran over every gap
    if (hi0 <= lo0) break;  // never with a row CDF; whatever cum holds, a chosen gap is not empty
    const double base = lo0 > 0 ? cum[lo0 - 1] : 0.0;
    const double top = cum[hi0 - 1];
    const int64_t e = weighted_pick_gap(cum, lo0, hi0, base, top, top - base, words.entry(n));
    out[n] = e;
    for (int64_t j = n; j > g; --j) sorted[j] = sorted[j - 1];
    sorted[g] = e;
  }
  return n;
}

}  // namespace psa
