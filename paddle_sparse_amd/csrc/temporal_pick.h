// The time-bounded pick of temporal_neighbor_sample (temporal.hip), in plain C++
// so that the host export psa_temporal_pick_host runs the very text the kernels run.
//
// sorted_time[start .. start + deg) is one row of an EdgeTimeOrder: the times of the row's
// entries, ascending.  The eligible set of a bound T is the prefix of the entries with
// time <= T; c = temporal_count(...) is its length (an upper-bound search, at most 64
// halvings).  A pick is a RANK in [0, c); the caller turns it into a storage position
// through order[start + rank].
//
// Rules (k >= 0; k < 0 takes ranks 0 .. c-1 and needs no rule):
//   last                      ranks c-1, c-2, ..., c-min(k, c)
//   uniform, replace          randint(stream, t, c) for t < k, none when c == 0
//   uniform, no replace, c<=k ranks 0 .. c-1
//   uniform, no replace, c>k  the EXACT Floyd walk: j = c - k + t, r = randint(stream, t, j + 1)
//                             in [0, j], pick = r was picked before ? j : r
// The walk is uniform_pick.h's floyd_walk with kDrawClosed and base 0 (it stores ranks), which
// also says why sample_adj's draw in [0, j) will not do here.  The draws are rng.h's.
#pragma once

#include <stdint.h>

#include "uniform_pick.h"

namespace psa {

constexpr int kTemporalUniform = 0, kTemporalLast = 1;

// Entries of sorted_time[start, start + deg) that are <= bound.
PSA_HD int64_t temporal_count(const int64_t* sorted_time, int64_t start, int64_t deg, int64_t bound) {
  int64_t lo = 0, hi = deg;  // smallest index with time > bound, deg for none
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted_time[start + mid] > bound) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Picks of a parent with c eligible entries (k >= 0).
PSA_HD int64_t temporal_picks_of(int64_t c, int64_t k, int replace, int strategy) {
  return picks_of(c, k, strategy == kTemporalUniform && replace);
}

// True for the parents whose picks are a Floyd walk; every other pick is a function of its slot alone.
PSA_HD bool temporal_is_floyd(int64_t c, int64_t k, int replace, int strategy) {
  return strategy == kTemporalUniform && !replace && c > k;
}

// Rank of pick t < temporal_picks_of(...) of a parent that is not a Floyd parent.
PSA_HD int64_t temporal_slot_rank(int64_t c, int replace, int strategy, uint64_t stream, int64_t t) {
  if (strategy == kTemporalLast) return c - 1 - t;
  if (replace) return rand_draw(stream, t, c);
  return t;
}

}  // namespace psa
