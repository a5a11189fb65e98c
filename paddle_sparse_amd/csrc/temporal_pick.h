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
// The draw in [0, j] is what makes every k-subset equally likely; the walk of sample_adj
// draws in [0, j) (upstream's rule) and under-samples the last k ranks, which here are the
// most recent entries.
//
// The random word is rng.h's: mix64(stream + t), turned into an index by the high half of a
// 64 x 64 product.  The device takes it from __umul64hi, the host from a 128-bit product: the
// same integer.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSA_TPICK_FN __host__ __device__ inline
#else
#define PSA_TPICK_FN inline
#endif

namespace psa {

constexpr int kTemporalUniform = 0, kTemporalLast = 1;

PSA_TPICK_FN uint64_t temporal_mix64(uint64_t z) {  // rng.h's mix64
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

PSA_TPICK_FN uint64_t temporal_stream(uint64_t seed, int64_t i) {  // rng.h's rand_stream
  return temporal_mix64(seed ^ temporal_mix64(static_cast<uint64_t>(i)));
}

PSA_TPICK_FN uint64_t temporal_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * static_cast<unsigned __int128>(b)) >> 64);
#endif
}

// rng.h's rand_draw: uniform integer in [0, n) of draw t of a stream (n > 0)
PSA_TPICK_FN int64_t temporal_draw(uint64_t stream, int64_t t, int64_t n) {
  return static_cast<int64_t>(temporal_mulhi(temporal_mix64(stream + static_cast<uint64_t>(t)), static_cast<uint64_t>(n)));
}

// Entries of sorted_time[start, start + deg) that are <= bound.
PSA_TPICK_FN int64_t temporal_count(const int64_t* sorted_time, int64_t start, int64_t deg, int64_t bound) {
  int64_t lo = 0, hi = deg;  // smallest index with time > bound, deg for none
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted_time[start + mid] > bound) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Picks of a parent with c eligible entries (k >= 0).
PSA_TPICK_FN int64_t temporal_picks_of(int64_t c, int64_t k, int replace, int strategy) {
  if (strategy == kTemporalUniform && replace) return c > 0 ? k : 0;
  return c < k ? c : k;
}

// True for the parents whose picks are a Floyd walk; every other pick is a function of its slot alone.
PSA_TPICK_FN bool temporal_is_floyd(int64_t c, int64_t k, int replace, int strategy) {
  return strategy == kTemporalUniform && !replace && c > k;
}

// Rank of pick t < temporal_picks_of(...) of a parent that is not a Floyd parent.
PSA_TPICK_FN int64_t temporal_slot_rank(int64_t c, int replace, int strategy, uint64_t stream, int64_t t) {
  if (strategy == kTemporalLast) return c - 1 - t;
  if (replace) return temporal_draw(stream, t, c);
  return t;
}

// The exact Floyd walk for k <= KMAX < c: out[0 .. k) in draw order.  Every index is static
// once the loops are unrolled, so the picks stay in registers on the device.
template <int KMAX>
PSA_TPICK_FN void temporal_floyd_small(int64_t c, int64_t k, uint64_t stream, int64_t* out) {
#pragma unroll
  for (int t = 0; t < KMAX; ++t) {
    if (t < k) {
      const int64_t j = c - k + t;  // >= 1
      const int64_t r = temporal_draw(stream, t, j + 1);
      bool taken = false;
#pragma unroll
      for (int u = 0; u < t; ++u) taken |= out[u] == r;
      out[t] = taken ? j : r;
    }
  }
}

// The same for any k < c, the picks in memory of the caller (out[0 .. k)).
PSA_TPICK_FN void temporal_floyd_large(int64_t c, int64_t k, uint64_t stream, int64_t* out) {
  for (int64_t t = 0; t < k; ++t) {
    const int64_t j = c - k + t;
    const int64_t r = temporal_draw(stream, t, j + 1);
    bool taken = false;
    for (int64_t u = 0; u < t && !taken; ++u) taken = out[u] == r;
    out[t] = taken ? j : r;
  }
}

}  // namespace psa
