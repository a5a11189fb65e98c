// Pair intersection: out[p] = sum over k in X[pair_x[p]] n Y[pair_y[p]] of x_val * y_val * weight[k], for two
// families of ascending, duplicate-free lists in CSR form.  The sampled sparse x sparse product
// C = (A @ diag(w) @ B) at the entries of a mask is this with X = the rows of A, Y = the columns of B and the pairs
// = the mask's entries; both of its value gradients and common_neighbors are the same call over other views.
//
// The shorter list of a pair is the PROBE list (tie: X), every probe element is binary-searched in the other one.
//   short mode  probe length <= kLongFrom: the pair is run by a group of kGroup = 8 lanes, a wave holds 8 pairs.
//               Lane l of the group takes probe elements l, l + 8, ... in order.
//   long mode   probe length  > kLongFrom: the group sits the short pass out; afterwards the wave takes its
//               deferred pairs one at a time (a ballot over the groups) with all 64 lanes, lane l taking probe
//               elements l, l + 64, ...  A hub n hub pair of a power-law graph is spread over a wave that way
//               without a list of long pairs, so the op needs no scratch and no second launch.
// Sum order (what tests/intersect_ref.py restates): a lane starts from 0 and adds its matches' terms in probe
// order, term = (x_val * y_val) * weight[k], every multiply and add rounded on its own (contraction is off for
// this file: an FMA would round once where numpy rounds twice); a lane without a match keeps its 0.  The W lane
// partials (W = 8 or 64) are folded by the xor butterfly 1, 2, 4, ...: every lane adds its partner's partial, so
// all lanes hold the same bits and lane 0 writes.  The order is a function of the two lengths alone.  A NULL
// value array or weight multiplies by one, which is exact, so the absent factors are simply not multiplied.
//
// A pair index outside [0, lists) reads nothing and writes 0: the pair list is the one operand whose contents
// this kernel does not take on trust.  Index values are compared as int64 and every address is 64-bit; the
// grid is capped and the waves stride over the tiles of 8 pairs, so P has no 32-bit bound.  No atomics, no
// host read: bitwise reproducible and capturable.
#include <type_traits>

#include "common.h"
#include "lane_fold.h"

#pragma clang fp contract(off)

#ifndef PSA_INTERSECT_T
#define PSA_INTERSECT_T 32
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / psa::kWave;
constexpr int kGroup = 8;                          // lanes of a pair in short mode
constexpr int kPairsPerWave = psa::kWave / kGroup;
constexpr int kLongFrom = PSA_INTERSECT_T;         // probe lists LONGER than this take the whole wave
constexpr int64_t kMaxBlocks = 65536;              // 2 M pairs per sweep of the grid

// x + x(lane ^ OFF): the DPP and permute forms of lane_fold.h for fp32, ds_bpermute for the 8-byte types
template <int OFF, typename T>
__device__ __forceinline__ T add_partner(T x) {
  if constexpr (std::is_same<T, float>::value) {
    if constexpr (OFF == 1 || OFF == 2) return x + psa::lane_xor<OFF>(x);
    else return psa::add_xor<OFF>(x);
  } else {
    return x + __shfl_xor(x, OFF);
  }
}

template <int W, typename T>
__device__ __forceinline__ T fold(T x) {
  x = add_partner<1>(x);
  x = add_partner<2>(x);
  x = add_partner<4>(x);
  if constexpr (W == 64) {
    x = add_partner<8>(x);
    x = add_partner<16>(x);
    x = add_partner<32>(x);
  }
  return x;
}

// This lane's partial: probe elements l, l + W, ... of pidx[0, np), each looked up in sidx[0, ns).  The
// probe elements of a lane ascend, so each search starts where the last one ended.
template <int W, typename T>
__device__ __forceinline__ T lane_partial(const int64_t* __restrict__ pidx, const T* __restrict__ pval, int64_t np,
                                          const int64_t* __restrict__ sidx, const T* __restrict__ sval, int64_t ns,
                                          const T* __restrict__ weight, int l) {
  T acc = T(0);
  int64_t lo = 0;
  for (int64_t i = l; i < np; i += W) {
    const int64_t k = pidx[i];
    int64_t hi = ns;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (sidx[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    if (lo < ns && sidx[lo] == k) {
      if constexpr (std::is_same<T, int64_t>::value) {
        acc += 1;
      } else {
        T term = T(1);
        if (pval && sval) term = pval[i] * sval[lo];
        else if (pval) term = pval[i];
        else if (sval) term = sval[lo];
        if (weight) term = term * weight[k];
        acc = acc + term;
      }
    }
  }
  return acc;
}

template <typename P>
__device__ __forceinline__ P* broadcast_ptr(P* p, int src) {
  return reinterpret_cast<P*>(__shfl(static_cast<long long>(reinterpret_cast<uintptr_t>(p)), src));
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
pair_intersect_kernel(const int64_t* __restrict__ x_ptr, const int64_t* __restrict__ x_idx, const T* __restrict__ x_val,
                      int64_t x_lists, const int64_t* __restrict__ y_ptr, const int64_t* __restrict__ y_idx,
                      const T* __restrict__ y_val, int64_t y_lists, const T* __restrict__ weight,
                      const int64_t* __restrict__ pair_x, const int64_t* __restrict__ pair_y, int64_t P,
                      T* __restrict__ out) {
  const int lane = threadIdx.x & (psa::kWave - 1);
  const int l = lane & (kGroup - 1);
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t tiles = (P + kPairsPerWave - 1) / kPairsPerWave;
  for (int64_t tile = wave; tile < tiles; tile += waves) {  // wave-uniform: every lane reaches every fold
    const int64_t p = tile * kPairsPerWave + (lane >> 3);
    const int64_t* pidx = nullptr;
    const int64_t* sidx = nullptr;
    const T* pval = nullptr;
    const T* sval = nullptr;
    int64_t np = 0, ns = 0;
    if (p < P) {
      const int64_t px = pair_x[p], py = pair_y[p];
      if (px >= 0 && px < x_lists && py >= 0 && py < y_lists) {
        const int64_t xs = x_ptr[px], nx = x_ptr[px + 1] - xs;
        const int64_t ys = y_ptr[py], ny = y_ptr[py + 1] - ys;
        const bool probe_x = nx <= ny;
        pidx = probe_x ? x_idx + xs : y_idx + ys;
        sidx = probe_x ? y_idx + ys : x_idx + xs;
        np = probe_x ? nx : ny;
        ns = probe_x ? ny : nx;
        const T* xv = x_val ? x_val + xs : nullptr;
        const T* yv = y_val ? y_val + ys : nullptr;
        pval = probe_x ? xv : yv;
        sval = probe_x ? yv : xv;
      }
    }
    const bool deferred = np > kLongFrom;
    T acc = lane_partial<kGroup>(pidx, pval, deferred ? int64_t(0) : np, sidx, sval, ns, weight, l);
    acc = fold<kGroup>(acc);
    if (l == 0 && p < P && !deferred) out[p] = acc;

    unsigned long long todo = __ballot(deferred);
    while (todo) {  // the wave's long pairs, one at a time, in group order
      const int src = __ffsll(todo) - 1;  // first lane of the group
      todo &= ~(0xffull << src);
      T a = lane_partial<psa::kWave>(broadcast_ptr(pidx, src), broadcast_ptr(pval, src),
                                     static_cast<int64_t>(__shfl(static_cast<long long>(np), src)),
                                     broadcast_ptr(sidx, src), broadcast_ptr(sval, src),
                                     static_cast<int64_t>(__shfl(static_cast<long long>(ns), src)), weight, lane);
      a = fold<psa::kWave>(a);
      if (lane == 0) out[tile * kPairsPerWave + (src >> 3)] = a;
    }
  }
}

template <typename T>
int launch(const int64_t* x_ptr, const int64_t* x_idx, const void* x_val, int64_t x_lists, const int64_t* y_ptr,
           const int64_t* y_idx, const void* y_val, int64_t y_lists, const void* weight, const int64_t* pair_x,
           const int64_t* pair_y, int64_t P, void* out, hipStream_t s) {
  const int64_t tiles = psa::ceil_div(P, kPairsPerWave);
  int64_t blocks = psa::ceil_div(tiles, kWavesPerBlock);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(pair_intersect_kernel<T>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, x_ptr, x_idx,
                     static_cast<const T*>(x_val), x_lists, y_ptr, y_idx, static_cast<const T*>(y_val), y_lists,
                     static_cast<const T*>(weight), pair_x, pair_y, P, static_cast<T*>(out));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

int psa_pair_intersect(int dtype, const int64_t* x_ptr, const int64_t* x_idx, const void* x_val, int64_t x_lists,
                       const int64_t* y_ptr, const int64_t* y_idx, const void* y_val, int64_t y_lists,
                       const void* weight, const int64_t* pair_x, const int64_t* pair_y, int64_t P, void* out,
                       psa_stream_t stream) {
  PSA_REQUIRE(P >= 0 && x_lists >= 0 && y_lists >= 0, "negative size");
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_F64 || dtype == PSA_I64, "dtype must be f32, f64 or i64");
  PSA_REQUIRE(dtype != PSA_I64 || (!x_val && !y_val && !weight),
              "the counting form (i64) takes no values and no weight");
  if (P == 0) return PSA_OK;
  PSA_REQUIRE(x_ptr && x_idx && y_ptr && y_idx && pair_x && pair_y && out, "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  switch (dtype) {
    case PSA_F32:
      return launch<float>(x_ptr, x_idx, x_val, x_lists, y_ptr, y_idx, y_val, y_lists, weight, pair_x, pair_y, P,
                           out, s);
    case PSA_F64:
      return launch<double>(x_ptr, x_idx, x_val, x_lists, y_ptr, y_idx, y_val, y_lists, weight, pair_x, pair_y, P,
                            out, s);
    default:
      return launch<int64_t>(x_ptr, x_idx, x_val, x_lists, y_ptr, y_idx, y_val, y_lists, weight, pair_x, pair_y, P,
                             out, s);
  }
}

}  // extern "C"
