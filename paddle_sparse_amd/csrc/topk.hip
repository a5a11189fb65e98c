// Segmented top-k selection for gfx950: keep[j] = 1 for the k entries of every segment with the
// greatest keys, 0 for the others (topk_select.h states the key, the rule and the steps, and
// the host export below runs the same text).  A selection, not a sort: nothing is reordered and
// nothing is written but one byte per entry.
//
// Two launches, no workspace, no host read, no atomics on global memory:
//
//   topk_short_kernel  a group of W lanes (W = 8 .. 64, chosen on the host from the mean segment
//                      length) per segment of up to kTopkShort entries.  The keys sit in
//                      registers (64 / W per lane); every lane counts the rank of its entries
//                      against all entries of the segment through cross-lane reads inside its
//                      group.  No threshold, no LDS.  The grid covers the segments, it is not
//                      capped.  Longer segments are skipped here.
//   topk_long_kernel   at most kTopkGrid workgroups of 256 lanes stride over the segments,
//                      kTopkChunk per workgroup and trip, dealt out by a bijection that scatters
//                      the ids (scatter_slot): every lane looks at one segment's bounds, the longer
//                      ones are listed in LDS, and the workgroup takes the listed segments one
//                      after another.  Up to kTopkLds entries the keys are read once into LDS;
//                      above, every pass reads the segment again from global memory (the caches),
//                      so that a hub row needs no scratch.  The threshold comes from the radix
//                      select of topk_select.h: per pass a 256-counter LDS histogram (integer LDS
//                      atomics, one add per wave and digit through wave_match), walked from the
//                      top by the first wave.  The write keeps key > T and the first q entries
//                      equal to T in position order: an in-order scan over 256-entry chunks
//                      (ballots, the waves' totals through LDS) with a running carry.
//                      Launched only when n > kTopkShort.
//
// k_s >= len keeps all and k_s <= 0 keeps none without a select.  Every address is formed in
// 64-bit arithmetic, every loop is bounded by the segment length, the digit count or the
// segment count, and no lane waits on a lane of another workgroup.  A segment whose bounds do
// not satisfy 0 <= begin <= end <= n is not touched.  The result is a pure function of the
// input: the order in which a workgroup takes its listed segments is the one thing that
// varies, and no segment reads what another wrote.
#include <vector>

#include "common.h"
#include "radix_util.h"
#include "topk_select.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;  // 256-entry steps of a long segment whose loads are issued together

template <typename K>
__device__ __forceinline__ K shfl_key(K v, int src, int width) {
  if constexpr (sizeof(K) == 8) return static_cast<K>(__shfl(static_cast<unsigned long long>(v), src, width));
  else return static_cast<K>(__shfl(static_cast<unsigned>(v), src, width));
}

// One group of W lanes per segment of 1 .. kTopkShort entries.
template <int DT, int W>
__global__ void __launch_bounds__(kThreads)
topk_short_kernel(const void* __restrict__ value, const int64_t* __restrict__ perm,
                  const int64_t* __restrict__ indptr, int64_t nseg, int64_t n, int64_t k,
                  const int64_t* __restrict__ k_seg, int smallest, uint8_t* __restrict__ keep) {
  using K = typename psa::TopkKey<DT>::type;
  constexpr int R = psa::kTopkShort / W;  // entries per lane
  const int64_t seg = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / W;
  if (seg >= nseg) return;  // group-uniform, as every branch around a cross-lane read below
  const int lig = threadIdx.x & (W - 1);
  const int64_t b = indptr[seg], e = indptr[seg + 1];
  if (!psa::topk_valid_segment(b, e, n)) return;
  const int64_t len64 = e - b;
  if (len64 == 0 || len64 > psa::kTopkShort) return;
  const int len = static_cast<int>(len64);
  const int64_t ks = k_seg ? k_seg[seg] : k;
  K key[R];
  int64_t at[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int p = i * W + lig;
    key[i] = 0;
    at[i] = 0;
    if (p < len) {
      at[i] = perm ? perm[b + p] : b + p;
      key[i] = psa::topk_key<DT>(value, at[i], smallest != 0);
    }
  }
  if (ks <= 0 || ks >= len) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (i * W + lig < len) keep[at[i]] = ks > 0 ? 1 : 0;
    return;
  }
  int rank[R];
#pragma unroll
  for (int i = 0; i < R; ++i) rank[i] = 0;
#pragma unroll
  for (int i2 = 0; i2 < R; ++i2) {
    const int lim = len - i2 * W < W ? len - i2 * W : W;  // entries of step i2: <= 0 when there are none
    for (int l2 = 0; l2 < lim; ++l2) {
      const K other = shfl_key(key[i2], l2, W);
      const int p2 = i2 * W + l2;
#pragma unroll
      for (int i = 0; i < R; ++i) rank[i] += psa::topk_beats(other, p2, key[i], i * W + lig) ? 1 : 0;
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
    if (i * W + lig < len) keep[at[i]] = rank[i] < ks ? 1 : 0;
}

// The keys of a segment as the select reads them: staged in LDS, or formed again from global memory.
template <typename K>
struct LdsKeys {
  const K* keys;
  __device__ __forceinline__ K operator()(int64_t i) const { return keys[i]; }
};

template <int DT>
struct StreamKeys {
  const void* value;
  const int64_t* perm;
  int64_t b;
  bool smallest;
  __device__ __forceinline__ typename psa::TopkKey<DT>::type operator()(int64_t i) const {
    const int64_t j = b + i;
    return psa::topk_key<DT>(value, perm ? perm[j] : j, smallest);
  }
};

// topk_pick_digit on the 64 lanes of one wave: lane l owns the digits 255 - 4l .. 252 - 4l, an
// inclusive prefix sum over the lanes finds the lane whose digits hold the k-th greatest entry,
// and that lane walks its four counters.  Every lane of the wave calls it.
__device__ __forceinline__ void pick_digit_wave(const unsigned long long* hist, int64_t k, long long* pick,
                                                int lane) {
  unsigned long long c[4], sum = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    c[t] = hist[255 - 4 * lane - t];
    sum += c[t];
  }
  unsigned long long incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const unsigned long long want = static_cast<unsigned long long>(k);
  unsigned long long above = incl - sum;
  if (above < want && want <= incl) {
    int t = 0;  // the first of the four digits that reaches k
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      if (t == u && above + c[u] < want) {
        above += c[u];
        ++t;
      }
    }
    pick[0] = 255 - 4 * lane - t;
    pick[1] = static_cast<long long>(above);
  }
}

struct LongShared {
  unsigned long long hist[psa::kRadix];
  long long pick[2];
  int wave_total[kWaves];
};

// (T, q) of one segment with 0 < ks < len, then the ordered write.  Every lane of the workgroup calls it.
template <typename K, typename Keys>
__device__ __forceinline__ void select_and_write(const Keys keys, int64_t len, int64_t ks,
                                                 const int64_t* __restrict__ perm, int64_t b,
                                                 uint8_t* __restrict__ keep, LongShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kPasses = static_cast<int>(sizeof(K));
  K prefix = 0;
  int64_t krem = ks;
  for (int pass = 0; pass < kPasses; ++pass) {
    const int shift = (kPasses - 1 - pass) * 8;
    sh.hist[tid] = 0;
    __syncthreads();
    for (int64_t base = 0; base < len; base += kThreads * kUnroll) {
      K key[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {  // the loads first: kUnroll of them in flight per lane
        const int64_t i = base + u * kThreads + tid;
        key[u] = i < len ? keys(i) : K(0);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (base + u * kThreads < len) {  // workgroup-uniform: wave_match sees full waves
          const bool valid = base + u * kThreads + tid < len && psa::topk_matches(key[u], prefix, shift);
          const unsigned d = psa::topk_digit(key[u], shift);
          const uint32_t m = psa::wave_match(d, valid);
          if (valid && (m & 0xffu) == 0u) atomicAdd(&sh.hist[d], static_cast<unsigned long long>(m >> 8));
        }
      }
    }
    __syncthreads();
    if (wave == 0) pick_digit_wave(sh.hist, krem, sh.pick, lane);
    __syncthreads();
    psa::topk_narrow(&prefix, &krem, static_cast<unsigned>(sh.pick[0]) & 255u, sh.pick[1], shift);
  }
  const K T = prefix;
  const int64_t q = krem;
  int64_t carry = 0;  // entries equal to T before this chunk
  for (int64_t base0 = 0; base0 < len; base0 += kThreads * kUnroll) {
    K keyu[kUnroll];
    int64_t at[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base0 + u * kThreads + tid;
      keyu[u] = K(0);
      at[u] = 0;
      if (i < len) {
        keyu[u] = keys(i);
        at[u] = perm ? perm[b + i] : b + i;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t base = base0 + u * kThreads;
      if (base >= len) break;  // workgroup-uniform
      const bool valid = base + tid < len;
      const K key = keyu[u];
      int64_t before = q;  // once the quota is used up no equal entry is kept
      if (carry < q) {     // workgroup-uniform
        const unsigned long long eq = __ballot(valid && key == T);
        const int in_wave = __popcll(eq & ((1ull << lane) - 1ull));
        if (lane == 0) sh.wave_total[wave] = __popcll(eq);
        __syncthreads();
        int pre = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          const int c = sh.wave_total[w];
          pre += w < wave ? c : 0;
          total += c;
        }
        before = carry + pre + in_wave;
        carry += total;
        __syncthreads();
      }
      if (valid) keep[at[u]] = psa::topk_keep(key, T, before, q);
    }
  }
}

// A bijection of [0, 2^bits) that scatters every bit pattern: which workgroup takes a segment must not follow
// the bits of its id, or the hub rows of a power-law graph (the ids with many zero bits, R-MAT) meet in one
// workgroup.  Right xor-shifts and odd multipliers modulo 2^bits are each invertible.
__device__ __forceinline__ int64_t scatter_slot(uint64_t x, int bits) {
  const uint64_t mask = (1ull << bits) - 1ull;
  const int half = (bits + 1) >> 1;
  x ^= x >> half;
  x = (x * 0x9E3779B97F4A7C15ull) & mask;
  x ^= x >> half;
  x = (x * 0xD6E8FEB86659FD93ull) & mask;
  x ^= x >> half;
  return static_cast<int64_t>(x);
}

template <int DT>
__global__ void __launch_bounds__(kThreads)
topk_long_kernel(const void* __restrict__ value, const int64_t* __restrict__ perm,
                 const int64_t* __restrict__ indptr, int64_t nseg, int64_t n, int64_t k,
                 const int64_t* __restrict__ k_seg, int smallest, int bits, uint8_t* __restrict__ keep) {
  using K = typename psa::TopkKey<DT>::type;
  __shared__ K skeys[psa::kTopkLds];
  __shared__ LongShared sh;
  __shared__ int64_t list[psa::kTopkChunk];
  __shared__ int nlist;
  static_assert(psa::kTopkChunk == kThreads, "one lane per segment of a chunk");
  const int tid = threadIdx.x;
  // Trip r covers the slots [r * span, (r + 1) * span) of [0, 2^bits), span = kTopkChunk * gridDim.x; lane t
  // of workgroup w has slot r * span + t * gridDim.x + w and looks at the segment scatter_slot(slot).
  const int64_t stride = gridDim.x, span = stride * psa::kTopkChunk, slots = int64_t{1} << bits;
  for (int64_t first = blockIdx.x; first < slots; first += span) {
    __syncthreads();  // the list of the trip before is used up
    if (tid == 0) nlist = 0;
    __syncthreads();
    const int64_t slot = first + tid * stride;
    const int64_t mine = slot < slots ? scatter_slot(static_cast<uint64_t>(slot), bits) : nseg;
    if (mine < nseg) {
      const int64_t b = indptr[mine], e = indptr[mine + 1];
      if (psa::topk_valid_segment(b, e, n) && e - b > psa::kTopkShort) list[atomicAdd(&nlist, 1)] = mine;
    }
    __syncthreads();
    const int count = nlist;
    for (int t = 0; t < count; ++t) {
      __syncthreads();  // the segment before is written: its keys in LDS may go
      const int64_t seg = list[t];
      const int64_t b = indptr[seg], len = indptr[seg + 1] - b;
      const int64_t ks = k_seg ? k_seg[seg] : k;
      if (ks <= 0 || ks >= len) {
        const uint8_t v = ks > 0 ? 1 : 0;
        for (int64_t i = tid; i < len; i += kThreads) {
          const int64_t j = b + i;
          keep[perm ? perm[j] : j] = v;
        }
      } else if (len <= psa::kTopkLds) {
        for (int64_t i = tid; i < len; i += kThreads) {
          const int64_t j = b + i;
          skeys[i] = psa::topk_key<DT>(value, perm ? perm[j] : j, smallest != 0);
        }
        __syncthreads();
        select_and_write<K>(LdsKeys<K>{skeys}, len, ks, perm, b, keep, sh);
      } else {
        select_and_write<K>(StreamKeys<DT>{value, perm, b, smallest != 0}, len, ks, perm, b, keep, sh);
      }
    }
  }
}

template <int DT>
void host_run(const void* value, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t n, int64_t k,
              const int64_t* k_seg, bool smallest, uint8_t* keep) {
  using K = typename psa::TopkKey<DT>::type;
  constexpr int kPasses = static_cast<int>(sizeof(K));
  std::vector<K> keys;
  for (int64_t seg = 0; seg < nseg; ++seg) {
    const int64_t b = indptr[seg], e = indptr[seg + 1];
    if (!psa::topk_valid_segment(b, e, n)) continue;
    const int64_t len = e - b, ks = k_seg ? k_seg[seg] : k;
    auto at = [&](int64_t i) { return perm ? perm[b + i] : b + i; };
    if (ks <= 0 || ks >= len) {
      for (int64_t i = 0; i < len; ++i) keep[at(i)] = ks > 0 ? 1 : 0;
      continue;
    }
    keys.resize(static_cast<size_t>(len));
    for (int64_t i = 0; i < len; ++i) keys[i] = psa::topk_key<DT>(value, at(i), smallest);
    if (len <= psa::kTopkShort) {
      for (int i = 0; i < len; ++i) {
        int rank = 0;
        for (int i2 = 0; i2 < len; ++i2) rank += psa::topk_beats(keys[i2], i2, keys[i], i) ? 1 : 0;
        keep[at(i)] = rank < ks ? 1 : 0;
      }
      continue;
    }
    K prefix = 0;
    int64_t krem = ks;
    for (int pass = 0; pass < kPasses; ++pass) {
      const int shift = (kPasses - 1 - pass) * 8;
      unsigned long long hist[psa::kRadix] = {};
      for (int64_t i = 0; i < len; ++i)
        if (psa::topk_matches(keys[i], prefix, shift)) ++hist[psa::topk_digit(keys[i], shift)];
      int64_t above = 0;
      const unsigned d = psa::topk_pick_digit(hist, krem, &above);
      psa::topk_narrow(&prefix, &krem, d, above, shift);
    }
    int64_t before = 0;
    for (int64_t i = 0; i < len; ++i) {
      keep[at(i)] = psa::topk_keep(keys[i], prefix, before, krem);
      before += keys[i] == prefix ? 1 : 0;
    }
  }
}

// The argument checks both entry points share: 1 = run, 0 = nothing to do, < 0 = refused.
int check_args(const char* fn, const void* value, int dtype, const void* indptr, int64_t nseg, int64_t n,
               const void* keep) {
  const char* msg = nullptr;
  if (nseg < 0 || n < 0) msg = "negative size";
  else if (dtype < PSA_F32 || dtype > PSA_BF16) msg = "unknown dtype";
  else if (nseg == 0 || n == 0) return 0;
  else if (!value || !indptr || !keep) msg = "NULL pointer";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

template <int DT, int W>
void launch_short(const void* value, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t n, int64_t k,
                  const int64_t* k_seg, int smallest, uint8_t* keep, hipStream_t s) {
  const int64_t blocks = psa::ceil_div(nseg, kThreads / W);
  hipLaunchKernelGGL((topk_short_kernel<DT, W>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, value,
                     perm, indptr, nseg, n, k, k_seg, smallest, keep);
}

template <int DT>
int run(const void* value, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t n, int64_t k,
        const int64_t* k_seg, int smallest, uint8_t* keep, hipStream_t s) {
  // lanes per short segment: enough for the mean segment in one step, at least 8, at most the wave
  const int64_t mean_len = psa::ceil_div(n, nseg);
  int W = 8;
  while (W < 64 && W < mean_len) W <<= 1;
  PSA_REQUIRE(psa::ceil_div(nseg, kThreads / W) <= 0x7fffffff, "too many segments for one launch");
  switch (W) {
    case 8: launch_short<DT, 8>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s); break;
    case 16: launch_short<DT, 16>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s); break;
    case 32: launch_short<DT, 32>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s); break;
    default: launch_short<DT, 64>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s); break;
  }
  if (n > psa::kTopkShort) {  // else no segment can be long
    int bits = 1;  // the segments are dealt out of [0, 2^bits), the power of two that holds them
    while (bits < 62 && (int64_t{1} << bits) < nseg) ++bits;
    int64_t blocks = psa::ceil_div(int64_t{1} << bits, psa::kTopkChunk);
    blocks = blocks > psa::kTopkGrid ? psa::kTopkGrid : blocks;
    hipLaunchKernelGGL((topk_long_kernel<DT>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, value, perm,
                       indptr, nseg, n, k, k_seg, smallest, bits, keep);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

int psa_segment_topk(const void* value, int dtype, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t n,
                     int64_t k, const int64_t* k_seg, int largest, uint8_t* keep, psa_stream_t stream) {
  const int go = check_args(__func__, value, dtype, indptr, nseg, n, keep);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  hipStream_t s = psa::as_stream(stream);
  const int smallest = largest ? 0 : 1;
  switch (dtype) {
    case PSA_F32: return run<PSA_F32>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
    case PSA_F64: return run<PSA_F64>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
    case PSA_I32: return run<PSA_I32>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
    case PSA_I64: return run<PSA_I64>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
    case PSA_F16: return run<PSA_F16>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
    default: return run<PSA_BF16>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep, s);
  }
}

int psa_segment_topk_host(const void* value, int dtype, const int64_t* perm, const int64_t* indptr, int64_t nseg,
                          int64_t n, int64_t k, const int64_t* k_seg, int largest, uint8_t* keep) {
  const int go = check_args(__func__, value, dtype, indptr, nseg, n, keep);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const bool smallest = largest == 0;
  switch (dtype) {
    case PSA_F32: host_run<PSA_F32>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
    case PSA_F64: host_run<PSA_F64>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
    case PSA_I32: host_run<PSA_I32>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
    case PSA_I64: host_run<PSA_I64>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
    case PSA_F16: host_run<PSA_F16>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
    default: host_run<PSA_BF16>(value, perm, indptr, nseg, n, k, k_seg, smallest, keep); break;
  }
  return PSA_OK;
}

}  // extern "C"
