// The steps of components.hip, in plain C++ so that the host export psa_components_host runs
// the very text the kernels run: a lock-free union-find over parent[0 .. N) in the style of
// ECL-CC (Jaiganesh and Burtscher, HPDC 2018).
//
// What holds at every moment, under any interleaving of the lanes of a launch:
//   (a) parent[x] <= x, and parent[x] == x exactly when x is a root;
//   (b) parent[x] is x or a proper ancestor of x in the forest, so its component is x's.
// A location changes in two ways only.  The CAS of uf_link turns a root hi into a child of a
// smaller node lo; it succeeds only while hi still is a root, so no tree is ever cut.  The
// halving store of uf_find replaces the parent of a non-root by its grandparent as read a
// moment earlier.  A lane that read either of them late still holds an ancestor, and parents
// of non-roots are strictly smaller than the node, so a stale or overwritten value costs steps,
// never the answer: correctness rests on (a) and (b), not on how fresh a read is, and no fence
// is needed.  Without a racing halving store the value at a location only decreases; such a
// store may put back an older (larger) ancestor, which (a) and (b) allow.
//
// uf_find ends because every step moves to a strictly smaller node: at most x steps.
// uf_link ends because each retry strictly lowers the sum of the two roots it holds: a failed
// CAS on parent[hi] returns a value below hi, the chase from it ends at or below it, and lo is
// kept; the sum is at most u + v at the start and never below 0, so u + v retries bound it.
// Nothing here waits on another lane or workgroup and nothing spins on a flag.
//
// Device build: loads and stores of parent are relaxed agent-scope atomics, which the L2
// serves past the per-CU L1 (a plain load could sit on a stale L1 line for the whole launch),
// and the CAS is 64-bit at agent scope.  Host build: plain loads and stores, one caller.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSA_UF_FN __host__ __device__ inline
#else
#define PSA_UF_FN inline
#endif

namespace psa {

constexpr int64_t kComponentsRange = 1;  // flag bit 0: an entry whose row or column lies outside [0, N)

PSA_UF_FN int64_t uf_load(const int64_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

PSA_UF_FN void uf_store(int64_t* p, int64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = x;
#endif
}

// *p = desired if *p == expected; returns what *p held before
PSA_UF_FN int64_t uf_cas(int64_t* p, int64_t expected, int64_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return expected;
#else
  const int64_t old = *p;
  if (old == expected) *p = desired;
  return old;
#endif
}

// The root of x, with path halving: every node passed is re-pointed at its grandparent.
PSA_UF_FN int64_t uf_find(int64_t* parent, int64_t x) {
  int64_t p = uf_load(parent + x);
  while (p != x) {
    const int64_t g = uf_load(parent + p);
    if (g == p) return p;
    uf_store(parent + x, g);
    x = g;
    p = uf_load(parent + x);
  }
  return x;
}

// Joins the trees of u and v: the larger root becomes a child of the smaller.
PSA_UF_FN void uf_link(int64_t* parent, int64_t u, int64_t v) {
  int64_t a = uf_find(parent, u), b = uf_find(parent, v);
  while (a != b) {
    const int64_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int64_t seen = uf_cas(parent + hi, hi, lo);
    if (seen == hi) return;
    a = uf_find(parent, seen);  // hi was no root any more: go on from its parent
    b = lo;
  }
}

// init, node v: the first stored column of row v when it is a smaller node, else v itself.
// Most entries of a graph numbered with any locality then find their ends joined already.
// rowptr values outside [0, nnz) read nothing.
PSA_UF_FN int64_t uf_first_parent(const int64_t* rowptr, const int64_t* col, int64_t nnz, int64_t v) {
  const int64_t p = rowptr[v];
  if (p < 0 || p >= nnz || p >= rowptr[v + 1]) return v;
  const int64_t c = col[p];
  return c >= 0 && c < v ? c : v;
}

// hook, entry (u, v): returns kComponentsRange and joins nothing when either end lies outside
// [0, N), 0 otherwise.
PSA_UF_FN int64_t uf_hook(int64_t* parent, int64_t N, int64_t u, int64_t v) {
  if (u < 0 || u >= N || v < 0 || v >= N) return kComponentsRange;
  if (u != v) uf_link(parent, u, v);
  return 0;
}

}  // namespace psa
