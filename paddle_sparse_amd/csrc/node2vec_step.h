// One step of the node2vec (p, q) walk (node2vec.hip), in plain C++ so that the host export
// psa_node2vec_walk_host runs the very text the kernel runs.
//
// A walk at node v (row [s, s + deg)) that arrived from t (row [ts, te)) proposes an entry of
// v's row exactly as the plain walks do (rand_draw's index, or weighted_pick in the row's
// cum) and accepts it with a chance that depends on the proposal's class: 0 = it leads back
// to t, 1 = row t stores its column (distance 1 from t, in the direction t -> x of the
// node2vec paper), 2 = neither.  The chances are thr[class] / 2^53, integers made by the
// caller from 1/p, 1, 1/q divided by the largest of them; the test is a 53-bit integer
// compare, so a restatement in any language gives the same bits.
//
// Try j of step l of a walk reads two words of the walk's counter-based stream:
//   c = stream + l + (j << 32),  proposal word mix64(c),  acceptance word mix64(c + 2^63)
// so try 0's proposal is the plain walk's draw of step l.  Every loop here has its bound
// before it starts: max_tries tries (the LAST proposal is taken when none was accepted),
// and at most 64 halvings in each search.
#pragma once

#include <stdint.h>

#include "rng.h"
#include "weighted_pick.h"

namespace psa {

constexpr uint64_t kNode2vecOne = 1ull << 53;  // the threshold of "always accept"
constexpr int kNode2vecMaxTries = 32768;

// high half of a 64 x 64 product: rand_draw's index for the word r among n entries
PSA_PICK_FN uint64_t node2vec_mulhi(uint64_t r, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, n);
#else
  return static_cast<uint64_t>((static_cast<unsigned __int128>(r) * n) >> 64);
#endif
}

// Does col[lo .. hi) (non-decreasing) hold x?  Lower bound, at most 64 halvings.
PSA_PICK_FN bool node2vec_row_has(const int64_t* col, int64_t lo, int64_t hi, int64_t x) {
  const int64_t end = hi;
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && col[lo] == x;
}

// Step l (0-based) of a walk of `stream` at a node whose row is [s, s + deg), having arrived
// from node t whose row is [ts, te) (at l == 0 nothing is read of them).  thr0, thr1, thr2
// (each <= 2^53) are the acceptance thresholds of the classes, max_tries >= 1.  Returns the
// storage position of the entry taken and its column in *x, or -1 (and *x untouched) when the
// row is empty or, WEIGHTED, its total is not positive.
template <bool WEIGHTED>
PSA_PICK_FN int64_t node2vec_step(const int64_t* col, const double* cum, int64_t s, int64_t deg, int64_t t,
                                  int64_t ts, int64_t te, uint64_t stream, int64_t l, uint64_t thr0, uint64_t thr1,
                                  uint64_t thr2, int max_tries, int64_t* x) {
  if (deg <= 0) return -1;
  const bool search = thr1 != thr2;  // equal chances: no need to tell class 1 from 2
  const uint64_t base = stream + static_cast<uint64_t>(l);
  int64_t e = -1, xe = 0;
  for (int j = 0; j < max_tries; ++j) {
    const uint64_t c = base + (static_cast<uint64_t>(j) << 32);
    const uint64_t r = mix64(c);
    if (WEIGHTED) {
      const int64_t pick = weighted_pick(cum + s, deg, r);
      if (pick < 0) return -1;  // the row's total: the same answer at every try
      e = s + pick;
    } else {
      e = s + static_cast<int64_t>(node2vec_mulhi(r, static_cast<uint64_t>(deg)));
    }
    xe = col[e];
    if (l == 0) break;  // no previous node: the plain walk's step
    uint64_t thr = thr0;
    if (xe != t) thr = !search || node2vec_row_has(col, ts, te, xe) ? thr1 : thr2;
    if (thr == kNode2vecOne) break;  // every 53-bit word is below it
    if ((mix64(c + (1ull << 63)) >> 11) < thr) break;
  }
  *x = xe;
  return e;
}

}  // namespace psa
