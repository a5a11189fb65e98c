// The two steps of negative.hip, in plain C++ so that the host exports psa_edge_lookup_host and
// psa_negative_sample_host run the very text the kernels run.
//
// edge_find looks a column up in one sorted row: a lower bound, so the position it returns is
// the FIRST of a duplicated entry.  negative_try_loop is rejection sampling against that
// lookup: sample i proposes pairs from its counter-based stream (rng.h) and takes the first
// one the matrix does not store.  Try j (0-based) of sample i reads
//   c = rand_stream(seed, i) + j,   column word mix64(c),   row word mix64(c + 2^63)
// and turns a word into an index as the walks do: the high half of word * size.  Every loop
// here has its bound before it starts: max_tries tries, and at most 64 halvings in a search.
#pragma once

#include <stdint.h>

#include "rng.h"
#include "weighted_pick.h"

namespace psa {

constexpr int kNegativeMaxTries = 32768;
constexpr int64_t kLookupRange = 1;     // flag bit 0: a query or a given row outside the matrix
constexpr int64_t kNegativeFailed = 2;  // flag bit 1: a sample whose tries were all refused

// high half of a 64 x 64 product: the index in [0, n) for the word r
PSA_PICK_FN uint64_t edge_mulhi(uint64_t r, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, n);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(r) * n) >> 64);
#endif
}

// Position of the first entry of col[lo .. hi) (non-decreasing) equal to x, or -1.  Lower
// bound, at most 64 halvings.
PSA_PICK_FN int64_t edge_find(const int64_t* col, int64_t lo, int64_t hi, int64_t x) {
  const int64_t end = hi;
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && col[lo] == x ? lo : -1;
}

// One query of psa_edge_lookup: the position of the first entry (r, c), -1 when it is not
// stored, -1 with *flag |= kLookupRange when (r, c) lies outside M x N (nothing is read then).
PSA_PICK_FN int64_t edge_lookup_one(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, int64_t r,
                                    int64_t c, int64_t* flag) {
  if (r < 0 || r >= M || c < 0 || c >= N) {
    *flag |= kLookupRange;
    return -1;
  }
  return edge_find(col, rowptr[r], rowptr[r + 1], c);
}

// Sample i: the first of max_tries proposals (r, cc) that is not stored (and, no_self_loops,
// not on the diagonal).  GIVEN_ROWS: r = given (the caller's src[i / k]) at every try; else r
// is drawn.  Returns the column and the row in *row_out, or -1 for both with *flag |=
// kNegativeFailed when every try was refused, or M or N is zero (nothing is read then); with
// GIVEN_ROWS and given outside [0, M), -1 with *flag |= kLookupRange and nothing read.
template <bool GIVEN_ROWS>
PSA_PICK_FN int64_t negative_try_loop(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, int64_t given,
                                      int64_t i, bool no_self_loops, int max_tries, uint64_t seed, int64_t* row_out,
                                      int64_t* flag) {
  *row_out = -1;
  if (GIVEN_ROWS && (given < 0 || given >= M)) {
    *flag |= kLookupRange;
    return -1;
  }
  if (M > 0 && N > 0) {
    const uint64_t stream = rand_stream(seed, i);
    int64_t lo = 0, hi = 0;
    if (GIVEN_ROWS) lo = rowptr[given], hi = rowptr[given + 1];
    for (int j = 0; j < max_tries; ++j) {
      const uint64_t c = stream + static_cast<uint64_t>(j);
      const int64_t cc = static_cast<int64_t>(edge_mulhi(mix64(c), static_cast<uint64_t>(N)));
      int64_t r = given;
      if (!GIVEN_ROWS) {
        r = static_cast<int64_t>(edge_mulhi(mix64(c + (1ull << 63)), static_cast<uint64_t>(M)));
        lo = rowptr[r], hi = rowptr[r + 1];
      }
      if (no_self_loops && r == cc) continue;
      if (edge_find(col, lo, hi, cc) < 0) {
        *row_out = r;
        return cc;
      }
    }
  }
  *flag |= kNegativeFailed;
  return -1;
}

}  // namespace psa
