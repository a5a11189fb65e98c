// The uniform pick that sample_adj (sample.hip), neighbor_sample (neighbor.hip),
// ego_k_hop_sample (ego.hip) and temporal_neighbor_sample (temporal_pick.h, temporal.hip)
// share, in plain C++ so that a `_host` export runs the very text the kernels run: how many
// picks a row makes, where a row lies, and Floyd's walk without replacement on the draws of
// rng.h.  The kernels around it differ per op (what a pick claims or emits) and stay apart.
#pragma once

#include <stdint.h>

#include "rng.h"

namespace psa {

constexpr int kFloydRegs = 32;             // largest fan-out whose Floyd picks stay in registers
constexpr int64_t kMaxSlots = 0x7ffffff0;  // slots of one hop: -2 - p must stay above INT32_MIN

// Picks of a row of deg entries for a fan-out of k (k < 0: every entry).
PSA_HD int64_t picks_of(int64_t deg, int64_t k, int replace) {
  if (k < 0) return deg;                       // sample_cpu.cpp:45-63
  if (replace) return deg > 0 ? k : 0;         // :66-88
  return deg < k ? deg : k;                    // :90-121
}

// start and degree of the row of node v; a node outside the matrix (a bad seed, whose flag is
// up, or the -1 of an empty walk entry) has no entries.
PSA_HD void row_of(const int64_t* __restrict__ rowptr, int64_t N, int64_t v, int64_t* start, int64_t* deg) {
  if (static_cast<uint64_t>(v) >= static_cast<uint64_t>(N)) {
    *start = 0;
    *deg = 0;
    return;
  }
  *start = rowptr[v];
  *deg = rowptr[v + 1] - *start;
}

// Floyd's walk: k distinct ranks of a row of n > k entries, out[t] = base + rank in draw
// order.  For j = n - k + t (>= 1) draw r, take r unless it was taken before, then take j
// (sample_cpu.cpp:100-106).  The two draw rules:
//   kDrawHalfOpen  r in [0, j), upstream's rule, kept by sample_adj, neighbor_sample and
//                  ego_k_hop_sample so that their picks stay upstream's for a given stream
//   kDrawClosed    r in [0, j], the EXACT walk of temporal_neighbor_sample
// The draw in [0, j] is what makes every k-subset equally likely; the half-open walk
// under-samples the last k ranks, which in a row ordered by time are the most recent entries.
constexpr bool kDrawHalfOpen = false, kDrawClosed = true;

// k <= KMAX, the picks in an array of the caller's: every index is static once the loops are
// unrolled, so on the device the picks stay in registers and a step does not wait for the
// previous step's store to come back from memory.
template <int KMAX, bool CLOSED>
PSA_HD void floyd_walk_regs(int64_t n, int64_t k, uint64_t stream, int64_t base, int64_t* out) {
#pragma unroll
  for (int t = 0; t < KMAX; ++t) {
    if (t < k) {
      const int64_t j = n - k + t;
      const int64_t pick = base + rand_draw(stream, t, CLOSED ? j + 1 : j);
      bool taken = false;
#pragma unroll
      for (int u = 0; u < t; ++u) taken |= out[u] == pick;
      out[t] = taken ? base + j : pick;
    }
  }
}

// Any k < n, the picks in memory of the caller, which doubles as the "already taken" set (k
// is small: the scan is k^2 / 2 compares).
template <bool CLOSED>
PSA_HD void floyd_walk(int64_t n, int64_t k, uint64_t stream, int64_t base, int64_t* out) {
  for (int64_t t = 0; t < k; ++t) {
    const int64_t j = n - k + t;
    const int64_t pick = base + rand_draw(stream, t, CLOSED ? j + 1 : j);
    bool taken = false;
    for (int64_t u = 0; u < t && !taken; ++u) taken = out[u] == pick;
    out[t] = taken ? base + j : pick;
  }
}

}  // namespace psa
