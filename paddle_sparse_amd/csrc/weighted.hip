// Edge-weighted sampling on a sorted CSR matrix for gfx950: the row CDF, the weighted
// random walk (with edge ids) and the weighted count / select steps of sample_adj.
//
// row CDF: cum[e] = inclusive prefix sum of the row's float64 weights, STRICTLY left to
// right (cum[s] = w[s], cum[e] = fl(cum[e-1] + w[e])), so cum is np.cumsum of the row bit
// for bit, non-decreasing, and flat exactly across zero weights (a tree scan guarantees
// neither under rounding).  A wave first takes 64 consecutive rows: a row of up to kLaneMax
// entries is summed by its own lane (the 64 rows of a wave are one contiguous stretch of
// w, so its lines are shared among the lanes).  Then it takes the longer ones among rows
// g, g + P, g + 2 P, ... (an odd stride, so that neighbouring hubs fall to different
// waves), each by the whole wave: 64 entries per coalesced load, the next 64 already in
// flight, and the 64 dependent adds by one lane that reads the entries from LDS and leaves
// the sums there, 16 bytes at a time.  The longest row's chain is the critical path of the
// launch (DESIGN.md §3.17 states its cost).  No workspace, no float atomics, no waiting on
// another workgroup.
//
// The pick is weighted_pick.h: the random word of rng.h's draw (stream, t) looked up in
// the row's cum by binary search: log2(deg) dependent 8-byte loads after the total.
//
// weighted walk: psa_random_walk's launch shape (one lane per walk, the node in a register,
// bursts of stores), each step's entry chosen by the pick; also the uniform walk when cum
// is NULL, which is what gives psa_random_walk's bits together with the edge ids.
#include "common.h"
#include "rng.h"
#include "weighted_pick.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kLaneMax = 16;  // longest row summed by one lane, its entries held in registers
constexpr int kBuf = 16;      // steps per burst of stores, as walk.hip
constexpr int kBufEdges = 8;  // with edge ids two rows are buffered: half the steps each

constexpr unsigned kNegative = 1, kNonFinite = 2, kOverflow = 4;

// ---- row CDF ----------------------------------------------------------------------

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= DBL_MAX; }

__device__ __forceinline__ unsigned weight_bits(double x) {
  return (x < 0.0 ? kNegative : 0u) | (finite(x) ? 0u : kNonFinite);  // -0.0 < 0.0 is false
}

// LDS written by some lanes of a wave is read by others of the same wave after this: the wave's LDS
// operations complete in order, and the fence keeps the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lane k's x in every lane (k is wave-uniform: two v_readlane).
__device__ __forceinline__ double lane_read(double x, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k),
                          __builtin_amdgcn_readlane(__double2loint(x), k));
}

__global__ void __launch_bounds__(kThreads)
row_cdf_kernel(const int64_t* __restrict__ rowptr, const double* __restrict__ w, int64_t N, int64_t P,
               double* __restrict__ cum, unsigned long long* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  int64_t s = 0, deg = 0;
  if (r < N) {
    s = rowptr[r];
    deg = rowptr[r + 1] - s;
  }
  unsigned bits = 0;
  if (deg > 0 && deg <= kLaneMax) {
    // every load first, then the chain, then every store: a store between two loads would put its
    // completion on the next load's wait (vmcnt counts both)
    double x[kLaneMax];
#pragma unroll
    for (int k = 0; k < kLaneMax; ++k) x[k] = k < deg ? w[s + k] : 0.0;
    double c = -0.0;  // -0.0 + x == x for every x, -0.0 included: cum[s] = w[s]
    unsigned row_bits = 0;
#pragma unroll
    for (int k = 0; k < kLaneMax; ++k) {
      row_bits |= weight_bits(x[k]);
      c = c + x[k];  // past the row's end: + 0.0 after its last entry
      x[k] = c;
    }
#pragma unroll
    for (int k = 0; k < kLaneMax; ++k)
      if (k < deg) cum[s + k] = x[k];
    if (!(row_bits & kNonFinite) && c == INFINITY) row_bits |= kOverflow;
    bits = row_bits;
  }
  // The long rows, dealt out afresh: wave g looks at rows g, g + P, g + 2 P, ... (P odd, 64 P >= N),
  // so that neighbouring hub rows, and the hub ids of an R-MAT graph, which differ in single bits, are
  // chained by different waves instead of one after the other by the wave that owns their 64 rows.
  const int64_t g = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  const int64_t r2 = g + lane * P;
  s = 0, deg = 0;
  if (g < P && r2 < N) {
    s = rowptr[r2];
    deg = rowptr[r2 + 1] - s;
  }
  __shared__ double s_chain[kThreads / 64][2][64];
  double* s_in = s_chain[threadIdx.x >> 6][0];
  double* s_out = s_chain[threadIdx.x >> 6][1];
  uint64_t longs = __ballot(deg > kLaneMax);
  while (longs) {  // wave-uniform
    const int j = __ffsll(static_cast<unsigned long long>(longs)) - 1;
    longs &= longs - 1;
    const int64_t rs = __shfl(s, j), end = rs + __shfl(deg, j);
    double carry = -0.0;
    double x = rs + lane < end ? w[rs + lane] : 0.0;
    unsigned row_bits = weight_bits(x);  // x has arrived before the loop starts (see the end of the loop)
    double pending = 0.0;     // the previous 64 sums, stored one round late: issued BEFORE the next load, they
    int64_t pending_at = -1;  // have the whole chain to complete and the wait for that load does not wait for them
    for (int64_t base = rs; base < end; base += 64) {
      if (pending_at >= 0) cum[pending_at] = pending;
      const int64_t nb = base + 64 + lane;
      const double nx = nb < end ? w[nb] : 0.0;  // the next 64 entries, in flight during the chain
      s_in[lane] = x;
      wave_sync();
      if (lane == 0) {  // the chain itself: 64 dependent adds in one lane, fed and drained through LDS
#pragma unroll
        for (int k = 0; k < 64; ++k) {
          carry = carry + s_in[k];  // lanes past the row's end hold +0.0, added after its last entry
          s_out[k] = carry;
        }
      }
      wave_sync();
      pending = s_out[lane];
      pending_at = base + lane < end ? base + lane : -1;
      // the first use of nx, and so the wait for it, stands after the chain: were x still in flight at
      // the top of the loop, the compiler's wait for it there would wait for the load just issued as well
      row_bits |= weight_bits(nx);
      x = nx;
    }
    if (pending_at >= 0) cum[pending_at] = pending;
    if (lane_read(carry, 0) == INFINITY && !__any(row_bits & kNonFinite)) row_bits |= kOverflow;
    bits |= row_bits;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off);
  if (lane == 0 && bits) atomicOr(flags, static_cast<unsigned long long>(bits));
}

// ---- random walk --------------------------------------------------------------------

// One lane per walk; BUF steps per burst of stores.  WEIGHTED: cum chooses the entry;
// otherwise rand_draw does, as random_walk_kernel (walk.hip).  EDGES: edge_out too.
template <bool WEIGHTED, bool EDGES, int BUF>
__global__ void __launch_bounds__(kThreads)
weighted_walk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                     const double* __restrict__ cum, const int64_t* __restrict__ start, int64_t S, int64_t L,
                     int64_t N, uint64_t seed, int64_t* __restrict__ out, int64_t* __restrict__ edge_out,
                     unsigned long long* __restrict__ flags) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  bool live = n < S;
  int64_t cur = live ? start[n] : 0;
  if (live && (cur < 0 || cur >= N)) {
    atomicOr(flags, 1ull);
    live = false;
  }
  const int64_t row = n * (L + 1), erow = n * L;
  const uint64_t stream = psa::rand_stream(seed, n);
  if (live) out[row] = cur;
  for (int64_t l0 = 0; l0 < L; l0 += BUF) {
    int64_t buf[BUF], ebuf[EDGES ? BUF : 1];
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      const int64_t l = l0 + j;
      if (l < L) {  // uniform across the grid
        const int64_t s = live ? rowptr[cur] : 0;
        const int64_t deg = live ? rowptr[cur + 1] - s : 0;
        int64_t e = -1;
        if (deg > 0) {
          if (WEIGHTED) {
            const int64_t pick = psa::weighted_pick(cum + s, deg, psa::mix64(stream + static_cast<uint64_t>(l)));
            if (pick >= 0) e = s + pick;
          } else {
            e = s + psa::rand_draw(stream, l, deg);
          }
        }
        if (e >= 0) cur = col[e];
        buf[j] = cur;
        if (EDGES) ebuf[j] = e;
      }
    }
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      if (l0 + j < L && live) {
        out[row + l0 + j + 1] = buf[j];
        if (EDGES) edge_out[erow + l0 + j] = ebuf[j];
      }
    }
  }
}

// ---- sample_adj: count and select -----------------------------------------------------

__global__ void __launch_bounds__(kThreads)
sample_count_weighted_kernel(const int64_t* __restrict__ rowptr, const double* __restrict__ cum,
                             const int64_t* __restrict__ idx, int64_t S, int64_t k,
                             int64_t* __restrict__ counts) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t n = idx[i];
  const int64_t s = rowptr[n], deg = rowptr[n + 1] - s;
  if (k < 0) counts[i] = deg;
  else counts[i] = deg > 0 && cum[s + deg - 1] > 0.0 ? k : 0;
}

__global__ void __launch_bounds__(kThreads)
sample_select_weighted_kernel(const int64_t* __restrict__ rowptr, const double* __restrict__ cum,
                              const int64_t* __restrict__ idx, const int64_t* __restrict__ out_rowptr,
                              const int64_t* __restrict__ owner, int64_t E, int64_t k, uint64_t seed,
                              int64_t* __restrict__ e_raw) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= E) return;
  const int64_t i = owner[p];
  const int64_t t = p - out_rowptr[i];
  const int64_t n = idx[i];
  const int64_t s = rowptr[n], deg = rowptr[n + 1] - s;
  if (k < 0) {
    e_raw[p] = s + t;
  } else {  // the count made slots only for rows with a positive total
    const int64_t pick = psa::weighted_pick(cum + s, deg, psa::mix64(psa::rand_stream(seed, i) + static_cast<uint64_t>(t)));
    e_raw[p] = s + (pick > 0 ? pick : 0);
  }
}

int grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = psa::ceil_div(n > 0 ? n : 1, kThreads);
  if (b > 0x7fffffff) return 0;
  *blocks = static_cast<unsigned>(b);
  return 1;
}

}  // namespace

extern "C" {

int psa_row_cdf(const int64_t* rowptr, const double* w, int64_t N, double* cum, int64_t* flags,
                psa_stream_t stream) {
  PSA_REQUIRE(N >= 0, "negative size");
  if (N == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && flags, "NULL pointer");  // w and cum may be NULL when the matrix has no entries
  const int64_t P = psa::ceil_div(N, 64) | 1;  // waves that take long rows: odd, and 64 P >= N
  unsigned blocks;
  PSA_REQUIRE(grid_for(P * 64, &blocks), "N too large for one launch");
  hipLaunchKernelGGL(row_cdf_kernel, dim3(blocks), dim3(kThreads), 0, psa::as_stream(stream), rowptr, w, N, P, cum,
                     reinterpret_cast<unsigned long long*>(flags));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int64_t psa_weighted_pick_host(const double* cum, int64_t deg, uint64_t r) {
  if (cum == nullptr || deg <= 0) return -1;
  return psa::weighted_pick(cum, deg, r);
}

int psa_random_walk_weighted(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                             const int64_t* start, int64_t S, int64_t walk_length, uint64_t seed, int64_t* out,
                             int64_t* edge_out, int64_t* flags, psa_stream_t stream) {
  PSA_REQUIRE(N >= 0 && S >= 0 && walk_length >= 0, "negative size");
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && start && out && flags, "NULL pointer");
  PSA_REQUIRE(walk_length < INT64_MAX / S - 1, "output too large");
  hipStream_t s = psa::as_stream(stream);
  unsigned blocks;
  PSA_REQUIRE(grid_for(S, &blocks), "too many walks for one launch");
  auto* f = reinterpret_cast<unsigned long long*>(flags);
#define PSA_WALK(W, E, B)                                                                                     \
  hipLaunchKernelGGL((weighted_walk_kernel<W, E, B>), dim3(blocks), dim3(kThreads), 0, s, rowptr, col, cum, \
                     start, S, walk_length, N, seed, out, edge_out, f)
  if (cum && edge_out) PSA_WALK(true, true, kBufEdges);
  else if (cum) PSA_WALK(true, false, kBuf);
  else if (edge_out) PSA_WALK(false, true, kBufEdges);
  else PSA_WALK(false, false, kBuf);
#undef PSA_WALK
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_sample_count_weighted(const int64_t* rowptr, const double* cum, const int64_t* idx, int64_t S,
                              int64_t num_neighbors, int replace, int64_t* counts, psa_stream_t stream) {
  PSA_REQUIRE(S >= 0, "negative size");
  PSA_REQUIRE(num_neighbors < 0 || replace, "weighted picks without replacement are not supported");
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && idx && counts && (cum || num_neighbors < 0), "NULL pointer");
  unsigned blocks;
  PSA_REQUIRE(grid_for(S, &blocks), "subset too large for one launch");
  hipLaunchKernelGGL(sample_count_weighted_kernel, dim3(blocks), dim3(kThreads), 0, psa::as_stream(stream), rowptr,
                     cum, idx, S, num_neighbors, counts);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_sample_select_weighted(const int64_t* rowptr, const double* cum, const int64_t* idx, int64_t S,
                               const int64_t* out_rowptr, const int64_t* owner, int64_t E, int64_t num_neighbors,
                               int replace, uint64_t seed, int64_t* e_raw, psa_stream_t stream) {
  PSA_REQUIRE(S >= 0 && E >= 0, "negative size");
  PSA_REQUIRE(num_neighbors < 0 || replace, "weighted picks without replacement are not supported");
  if (S == 0 || E == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && idx && out_rowptr && owner && e_raw && (cum || num_neighbors < 0), "NULL pointer");
  unsigned blocks;
  PSA_REQUIRE(grid_for(E, &blocks), "too many picks for one launch");
  hipLaunchKernelGGL(sample_select_weighted_kernel, dim3(blocks), dim3(kThreads), 0, psa::as_stream(stream), rowptr,
                     cum, idx, out_rowptr, owner, E, num_neighbors, seed, e_raw);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"
