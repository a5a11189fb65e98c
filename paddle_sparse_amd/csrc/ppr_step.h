// The steps of the forward push of ppr.hip, in plain C++ so that the host export psa_ppr_host
// runs the very text the kernel runs.
//
// Personalised PageRank of one source by the Andersen-Chung-Lang push, in fixed point: a unit
// of mass is kPprOne = 2^48, alpha is alpha_q / 2^32 and eps is eps_q / 2^48.  Every quantity is
// an unsigned integer and every update is an integer add, so the state after a round does not
// depend on the order in which lanes ran.
//
// A ROUND.  Node u with residual x and deg(u) stored columns is ACTIVE iff
//   x >= eps_q * max(deg(u), 1)                                   (ppr_active)
// judged on the state at the start of the round.  Every active node is split (ppr_split):
//   deg == 0:  p += x, r = 0                 (the limit of a self loop; mass stays conserved)
//   deg >= 1:  keep  = (x * alpha_q) >> 32   (an 81-bit product)
//              share = (x - keep) / deg      (floored)
//              p += keep,  r = x - keep - share * deg
// and after ALL splits of the round every stored column v of u receives r[v] += share(u).
//
// WHAT BOUNDS THE WORK.  With k0 = (alpha_q * eps_q) >> 32 (>= 1 because alpha_q >= 2^16 and
// eps_q >= 2^16) an active node of degree d >= 1 has x >= d * eps_q, hence
//   keep = floor(x * alpha_q / 2^32) >= floor(d * eps_q * alpha_q / 2^32) >= d * k0,
// and the keeps of a run add up to at most kPprOne.  So
//   sum of deg(u) over all pushes  <=  kPprOne / k0   (integer division)   =: bound
// (ppr_work_bound), a node is first touched by one of those entries, so at most 1 + bound
// nodes ever hold mass, and every round with an active node moves at least k0 into p, so a run
// has at most bound + 1 rounds.  share >= 1 for every active node with entries (x - keep >=
// x * 2^-16 >= deg because alpha_q <= 2^32 - 2^16), which is what lets a slot's `s` word say
// "a push is pending" by being non-zero.
//
// THE TABLE.  State lives in an open-addressing table of cap slots (a power of two): key
// (the node, kPprEmpty when free), r, p and s, the share that a split leaves for the entry
// phase of the same round.  A node's home slot is ppr_hash; a probe goes on to the next slot
// (linear, wrapping) at most cap times (ppr_add).  The memory policy M says how a word is
// read, written, compared-and-swapped and added to: plain accesses on the host, atomics on
// the device.
#pragma once

#include <stdint.h>

#include "rng.h"

namespace psa {

constexpr uint64_t kPprOne = 1ull << 48;
constexpr int64_t kPprEmpty = -1;
constexpr int64_t kPprTableFull = 1;  // == PSA_PPR_TABLE_FULL
constexpr int64_t kPprBadIndex = 2;   // == PSA_PPR_BAD_INDEX
constexpr int64_t kPprInLds = 4;      // == PSA_PPR_IN_LDS

// kPprOne / ((alpha_q * eps_q) >> 32): see the header comment.  alpha_q < 2^32, eps_q <= 2^48.
PSA_HD uint64_t ppr_work_bound(uint64_t alpha_q, uint64_t eps_q) {
  const uint64_t k0 = (mulhi64(alpha_q, eps_q) << 32) | ((alpha_q * eps_q) >> 32);
  return k0 ? kPprOne / k0 : kPprOne;
}

// x >= eps_q * max(deg, 1), without overflow for any deg
PSA_HD bool ppr_active(uint64_t x, int64_t deg, uint64_t eps_q) {
  const uint64_t d = deg > 0 ? static_cast<uint64_t>(deg) : 1;
  return mulhi64(eps_q, d) == 0 && x >= eps_q * d;
}

// The split of an active node: what goes to p, what every stored column gets, what stays.
struct PprSplit {
  uint64_t keep, share, rem;
};

PSA_HD PprSplit ppr_split(uint64_t x, int64_t deg, uint64_t alpha_q) {
  if (deg <= 0) return {x, 0, 0};
  const uint64_t keep = (mulhi64(x, alpha_q) << 32) | ((x * alpha_q) >> 32);
  const uint64_t y = x - keep, d = static_cast<uint64_t>(deg);
  const uint64_t share = y / d;
  return {keep, share, y - share * d};
}

// deg(u) from rowptr, 0 and *flags |= kPprBadIndex when the row's bounds are not inside [0, nnz]
PSA_HD int64_t ppr_row(const int64_t* rowptr, int64_t nnz, int64_t u, int64_t* begin, int64_t* flags) {
  const int64_t b = rowptr[u], e = rowptr[u + 1];
  *begin = b;
  if (0 <= b && b <= e && e <= nnz) return e - b;
  *flags |= kPprBadIndex;
  return 0;
}

PSA_HD int64_t ppr_hash(int64_t v, int64_t cap) {
  uint64_t h = static_cast<uint64_t>(v) * 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  return static_cast<int64_t>(h & static_cast<uint64_t>(cap - 1));
}

// The largest i in [0, n) with scan[i] <= e, scan non-decreasing with scan[0] = 0 <= e < scan[n]:
// the node of a chunk that owns entry number e.  At most 64 halvings.
template <typename Scan>
PSA_HD int ppr_owner(const Scan* scan, int n, int64_t e) {
  int lo = 0, hi = n;  // the answer is in [lo, hi)
  for (int i = 0; i < 64 && hi - lo > 1; ++i) {
    const int mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(scan[mid]) <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Plain accesses: the host's memory policy.
struct PprHostMem {
  static inline int64_t load(const int64_t* p) { return *p; }
  static inline void store(uint64_t* p, uint64_t v) { *p = v; }
  static inline int64_t cas(int64_t* p, int64_t expect, int64_t v) {
    const int64_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static inline void add(uint64_t* p, uint64_t v) { *p += v; }
};

// r[v] += share in the table of cap slots: finds v's slot or claims a free one (whose p the
// claimer zeroes; r and s of a free slot are zero already).  Returns 0, kPprBadIndex when v is no
// node (nothing is touched) or kPprTableFull when cap probes found neither v nor a free slot
// (the add is dropped).  No slot outside [0, cap) is ever addressed.
template <typename M>
PSA_HD int64_t ppr_add(int64_t* key, uint64_t* r, uint64_t* p, uint64_t* s, int64_t cap, int64_t N, int64_t v,
                           uint64_t share) {
  if (v < 0 || v >= N) return kPprBadIndex;
  int64_t slot = ppr_hash(v, cap);
  for (int64_t probe = 0; probe < cap; ++probe) {
    int64_t k = M::load(key + slot);
    if (k == kPprEmpty) {
      k = M::cas(key + slot, kPprEmpty, v);
      if (k == kPprEmpty) {
        M::store(p + slot, 0);
        k = v;
      }
    }
    if (k == v) {
      M::add(r + slot, share);
      return 0;
    }
    slot = (slot + 1) & (cap - 1);
  }
  return kPprTableFull;
}

}  // namespace psa
