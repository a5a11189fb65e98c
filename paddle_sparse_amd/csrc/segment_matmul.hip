// segment_matmul: out[r] = x_row(r) @ weight[t] for the rows r of segment t, and its weight gradient, on MFMA.
//
// Both kernels run the same inner product: a 64 x 64 tile of D = A * B owned by one workgroup of four waves in a
// 2 x 2 grid, each wave a 32 x 32 sub-tile in 16 accumulator registers per lane, the reduction dimension in steps of
// BK = 32.  The two operand tiles go global -> registers -> LDS, double buffered: the loads of step s + 1 are issued
// before the MFMAs of step s and stored to the other buffer after them, one barrier per step.
//
// LDS layout, both operands, both dtypes: tile[row][BK + PAD] with the REDUCTION index contiguous, row = the m index of
// A or the n index of B, PAD = 16 bytes.  A lane then reads its operand values as ONE 16-byte word: lane l takes
// tile[l % 32][g * 2 * VPL + VPL * (l / 32) ..] with VPL = 4 floats or 8 bf16.  For bf16 that word is the operand of
// one v_mfma_f32_32x32x16_bf16 as it stands.  For fp32 its four floats feed four v_mfma_f32_32x32x2_f32; the
// instruction takes k0 from lanes 0..31 and k0 + 1 from lanes 32..63, here these are k and k + 4 of the group: a
// permutation of the reduction index that A and B share, so the products pair up as they must.  The row stride
// BK + PAD is 144 bytes (fp32) or 80 bytes (bf16): 16-byte aligned, and 36 or 20 banks, so the eight rows that one
// pass of a 16-byte read covers start at banks 0, 4, .. 28 (or 0, 20, 8, 28, 16, 4, 24, 12) and cover all 32 once.
//
// An operand whose rows run along the reduction index in memory (x in the forward, weight with trans_w) is copied
// as 16-byte words.  An operand that is contiguous along m or n (weight [K, F], and both operands of the weight
// gradient, whose reduction runs over rows) is transposed on the way in: one 16-byte global load, VPL narrow LDS
// stores.  Eight lanes with consecutive reduction indices share a word column, which keeps those stores to a two-way
// conflict.  VEC = false takes the same route with element loads (any K, F and element alignment).
//
// No split over K, no atomics: every output element has one writer and one summation order.
#include "common.h"

namespace {

constexpr int BM = 64;    // rows of a tile (forward: rows of one segment; weight gradient: k)
constexpr int BN = 64;    // output columns of a tile
constexpr int BK = 32;    // reduction step
constexpr int CH = 1024;  // rows of a chunk of the weight gradient
constexpr int THREADS = 256;

typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

template <typename T>
struct Geo {
  static constexpr int VPL = 16 / static_cast<int>(sizeof(T));  // elements of a 16-byte word
  static constexpr int LD = BK + VPL;                           // row stride of an LDS tile, in elements
  static constexpr int KV = BK / VPL;                           // words of a row of a directly copied tile
  static constexpr int ROWS = THREADS / KV;                     // rows one pass of the workgroup copies
  static constexpr int MQ = 64 / VPL;                           // words along m / n of a transposed tile
  static constexpr int TROWS = THREADS / MQ;                    // reduction rows one transposing pass takes
  static constexpr int NV = BM * KV / THREADS;                  // words per thread and operand: 2 (fp32), 1 (bf16)
  static_assert(NV * TROWS == BK && BM == BN && NV * ROWS == BM, "tile geometry");
};

template <typename T>
union Word {
  uint4 q;
  T e[16 / sizeof(T)];
};

// VPL elements from p, of which the first `valid` exist (<= 0: none; p is not read then).  VEC: K or F is a
// multiple of VPL, so a word is whole or absent.
template <typename T, bool VEC>
__device__ __forceinline__ uint4 load_word(const T* p, int64_t valid) {
  constexpr int VPL = Geo<T>::VPL;
  if constexpr (VEC) {
    return valid > 0 ? *reinterpret_cast<const uint4*>(p) : make_uint4(0, 0, 0, 0);
  } else {
    Word<T> w;
#pragma unroll
    for (int i = 0; i < VPL; ++i) w.e[i] = i < valid ? p[i] : T(0);
    return w.q;
  }
}

// rows of the tile are rows of memory: word (row, kq) of pass `it`
template <typename T>
__device__ __forceinline__ void store_direct(T* tile, int it, uint4 q) {
  const int kq = threadIdx.x % Geo<T>::KV, m = threadIdx.x / Geo<T>::KV + it * Geo<T>::ROWS;
  *reinterpret_cast<uint4*>(tile + m * Geo<T>::LD + kq * Geo<T>::VPL) = q;
}

// position of this thread's word in a transposing pass: j = reduction row, mq = word along m / n
template <typename T>
__device__ __forceinline__ void trans_pos(int it, int& j, int& mq) {
  const int t = threadIdx.x;
  mq = (t / 8) % Geo<T>::MQ;
  j = it * Geo<T>::TROWS + (t / (8 * Geo<T>::MQ)) * 8 + t % 8;
}

template <typename T>
__device__ __forceinline__ void store_trans(T* tile, int it, uint4 q) {
  int j, mq;
  trans_pos<T>(it, j, mq);
  Word<T> w;
  w.q = q;
#pragma unroll
  for (int i = 0; i < Geo<T>::VPL; ++i) tile[(mq * Geo<T>::VPL + i) * Geo<T>::LD + j] = w.e[i];
}

// one BK step of the wave's 32 x 32 sub-tile: sa / sb are the LDS tiles, wm / wn the wave's place in the 2 x 2 grid
template <typename T>
__device__ __forceinline__ void mma_step(const T* sa, const T* sb, int wm, int wn, v16f& acc) {
  constexpr int VPL = Geo<T>::VPL, LD = Geo<T>::LD;
  const int lane = threadIdx.x % 64, r = lane % 32, h = lane / 32;
#pragma unroll
  for (int g = 0; g < BK / (2 * VPL); ++g) {
    const int k = g * 2 * VPL + h * VPL;
    const uint4 a = *reinterpret_cast<const uint4*>(sa + (wm * 32 + r) * LD + k);
    const uint4 b = *reinterpret_cast<const uint4*>(sb + (wn * 32 + r) * LD + k);
    if constexpr (sizeof(T) == 4) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc, 0, 0,
                                                    0);
    }
  }
}

// row of the sub-tile that accumulator v of this lane holds (its column is lane % 32)
__device__ __forceinline__ int acc_row(int v) { return 8 * (v / 4) + 4 * ((threadIdx.x % 64) / 32) + v % 4; }

// fp32 -> the output type, one round to nearest even for bf16 (a NaN stays a quiet NaN)
template <typename T>
__device__ __forceinline__ T narrow(float f) {
  if constexpr (sizeof(T) == 4) {
    return f;
  } else {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
  }
}

// largest t in [0, T) with table[t] <= w, for table[0] = 0 <= w < table[T]: the owner of work item w.  An owner has
// table[t] < table[t + 1], so a segment without work is never returned.
__device__ __forceinline__ int64_t owner_of(const int64_t* table, int64_t T, int64_t w) {
  int64_t lo = 0, hi = T;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (table[mid] <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- the maps from work items to segments, one workgroup looping over T ----------------------------------------
// BW = false: first[t] = sum over t' < t of ceil(len / BM), the row tiles of the forward.
// BW = true:  first[t] = sum of the work items of the weight gradient, 1 for a segment of at most CH rows (an empty
//             one included: it writes zeros) and ceil(len / CH) for a longer one; second[t] = sum of the partial
//             slots, ceil(len / CH) for the longer ones only.
template <bool BW>
__global__ __launch_bounds__(THREADS) void seg_map_kernel(const int64_t* __restrict__ ptr, int64_t T,
                                                          int64_t* __restrict__ first, int64_t* __restrict__ second) {
  __shared__ int64_t sa[THREADS], sb[THREADS];
  const int tid = threadIdx.x;
  int64_t carry_a = 0, carry_b = 0;
  for (int64_t base = 0; base < T; base += THREADS) {
    const int64_t t = base + tid;
    int64_t a = 0, b = 0;
    if (t < T) {
      int64_t len = ptr[t + 1] - ptr[t];
      if (len < 0) len = 0;
      if constexpr (BW) {
        b = len > CH ? (len + CH - 1) / CH : 0;
        a = len > CH ? b : 1;
      } else {
        a = (len + BM - 1) / BM;
      }
    }
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
      const int64_t xa = tid >= off ? sa[tid - off] : 0, xb = tid >= off ? sb[tid - off] : 0;
      __syncthreads();
      sa[tid] += xa;
      sb[tid] += xb;
      __syncthreads();
    }
    if (t < T) {
      first[t] = carry_a + sa[tid] - a;
      if constexpr (BW) second[t] = carry_b + sb[tid] - b;
    }
    carry_a += sa[THREADS - 1];
    carry_b += sb[THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) {
    first[T] = carry_a;
    if constexpr (BW) second[T] = carry_b;
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, bool VEC, bool TRANS>
__global__ __launch_bounds__(THREADS) void seg_mm_kernel(const T* __restrict__ x, const int64_t* __restrict__ index,
                                                         const int64_t* __restrict__ ptr, const T* __restrict__ weight,
                                                         const int64_t* __restrict__ out_index,
                                                         const int64_t* __restrict__ tile_ptr, int64_t nseg, int64_t K,
                                                         int64_t F, int64_t col_tiles, T* __restrict__ out) {
  using G = Geo<T>;
  __shared__ __attribute__((aligned(16))) T sA[2][BM * G::LD];
  __shared__ __attribute__((aligned(16))) T sB[2][BN * G::LD];
  const int64_t rt = blockIdx.x / col_tiles, n0 = (blockIdx.x % col_tiles) * BN;
  if (rt >= tile_ptr[nseg]) return;  // the grid is the bound ceil(R / BM) + T
  const int64_t t = owner_of(tile_ptr, nseg, rt);
  const int64_t row0 = ptr[t] + (rt - tile_ptr[t]) * BM, rend = ptr[t + 1];
  const T* __restrict__ w = weight + t * K * F;
  const int tid = threadIdx.x;

  // the rows this thread copies do not change over the K loop
  const T* arow[G::NV];
  const T* brow[G::NV];  // TRANS only: row n of weight[t] [F, K]
  const int kq = tid % G::KV;
#pragma unroll
  for (int it = 0; it < G::NV; ++it) {
    const int m = tid / G::KV + it * G::ROWS;
    const int64_t r = row0 + m;
    arow[it] = r < rend ? x + (index ? index[r] : r) * K : nullptr;
    brow[it] = n0 + m < F ? w + (n0 + m) * K : nullptr;
  }

  uint4 ra[G::NV], rb[G::NV];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      const int64_t k = k0 + kq * G::VPL;
      ra[it] = load_word<T, VEC>(arow[it] + k, arow[it] ? K - k : 0);
      if constexpr (TRANS) {
        rb[it] = load_word<T, VEC>(brow[it] + k, brow[it] ? K - k : 0);
      } else {
        int j, mq;
        trans_pos<T>(it, j, mq);
        const int64_t kk = k0 + j, n = n0 + mq * G::VPL;
        rb[it] = load_word<T, VEC>(w + kk * F + n, kk < K ? F - n : 0);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      store_direct<T>(sA[buf], it, ra[it]);
      if constexpr (TRANS) store_direct<T>(sB[buf], it, rb[it]);
      else store_trans<T>(sB[buf], it, rb[it]);
    }
  };

  const int wave = tid / 64, wm = wave / 2, wn = wave % 2;
  v16f acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  const int64_t steps = (K + BK - 1) / BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int64_t s = 0; s < steps; ++s) {
    const int buf = static_cast<int>(s & 1);
    if (s + 1 < steps) fetch((s + 1) * BK);
    mma_step<T>(sA[buf], sB[buf], wm, wn, acc);
    if (s + 1 < steps) stash(buf ^ 1);
    __syncthreads();
  }

  const int64_t n = n0 + wn * 32 + tid % 32;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t r = row0 + wm * 32 + acc_row(v);
    if (r < rend && n < F) out[(out_index ? out_index[r] : r) * F + n] = narrow<T>(acc[v]);
  }
}

// ---- weight gradient: D[k][f] = sum over the rows r of a chunk of x_row(r)[k] * g_row(r)[f] ------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void seg_mm_bw_kernel(const T* __restrict__ x, const int64_t* __restrict__ index,
                                                            const T* __restrict__ g,
                                                            const int64_t* __restrict__ out_index,
                                                            const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ work_ptr,
                                                            const int64_t* __restrict__ part_ptr, int64_t nseg,
                                                            int64_t K, int64_t F, int64_t k_tiles, int64_t f_tiles,
                                                            float* __restrict__ partial, T* __restrict__ grad_weight) {
  using G = Geo<T>;
  __shared__ __attribute__((aligned(16))) T sA[2][BM * G::LD];
  __shared__ __attribute__((aligned(16))) T sB[2][BN * G::LD];
  const int64_t per = k_tiles * f_tiles, item = blockIdx.x / per, rem = blockIdx.x % per;
  if (item >= work_ptr[nseg]) return;  // the grid is the bound T + 2 * ceil(R / CH)
  const int64_t t = owner_of(work_ptr, nseg, item), c = item - work_ptr[t];
  const int64_t seg0 = ptr[t], seg1 = ptr[t + 1];
  const bool direct = seg1 - seg0 <= CH;
  const int64_t slot = part_ptr[t] + c;  // below psa_segment_matmul_bw_chunks(R), which the entry demands of partial
  const int64_t r0 = seg0 + c * CH, r1 = seg1 < r0 + CH ? seg1 : r0 + CH;
  const int64_t k0 = (rem / f_tiles) * BM, f0 = (rem % f_tiles) * BN;
  const int tid = threadIdx.x;

  uint4 ra[G::NV], rb[G::NV];
  auto fetch = [&](int64_t row) {
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      int j, mq;
      trans_pos<T>(it, j, mq);
      const int64_t r = row + j, k = k0 + mq * G::VPL, f = f0 + mq * G::VPL;
      const bool live = r < r1;
      const int64_t xr = live ? (index ? index[r] : r) : 0, gr = live ? (out_index ? out_index[r] : r) : 0;
      ra[it] = load_word<T, VEC>(x + xr * K + k, live ? K - k : 0);
      rb[it] = load_word<T, VEC>(g + gr * F + f, live ? F - f : 0);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int it = 0; it < G::NV; ++it) {
      store_trans<T>(sA[buf], it, ra[it]);
      store_trans<T>(sB[buf], it, rb[it]);
    }
  };

  const int wave = tid / 64, wm = wave / 2, wn = wave % 2;
  v16f acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  const int64_t steps = r1 > r0 ? (r1 - r0 + BK - 1) / BK : 0;
  if (steps > 0) {
    fetch(r0);
    stash(0);
    __syncthreads();
  }
  for (int64_t s = 0; s < steps; ++s) {
    const int buf = static_cast<int>(s & 1);
    if (s + 1 < steps) fetch(r0 + (s + 1) * BK);
    mma_step<T>(sA[buf], sB[buf], wm, wn, acc);
    if (s + 1 < steps) stash(buf ^ 1);
    __syncthreads();
  }

  const int64_t f = f0 + wn * 32 + tid % 32;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t k = k0 + wm * 32 + acc_row(v);
    if (k < K && f < F) {
      if (direct) grad_weight[(t * K + k) * F + f] = narrow<T>(acc[v]);
      else partial[(slot * K + k) * F + f] = acc[v];
    }
  }
}

// folds the fp32 partials of every segment above CH rows in chunk order; one thread per element of grad_weight[t]
template <typename T>
__global__ __launch_bounds__(THREADS) void seg_mm_fold_kernel(const int64_t* __restrict__ ptr,
                                                              const int64_t* __restrict__ part_ptr, int64_t KF,
                                                              int64_t blocks_per, const float* __restrict__ partial,
                                                              T* __restrict__ grad_weight) {
  const int64_t t = blockIdx.x / blocks_per, e = (blockIdx.x % blocks_per) * THREADS + threadIdx.x;
  const int64_t len = ptr[t + 1] - ptr[t];
  if (len <= CH || e >= KF) return;
  const int64_t first = part_ptr[t], chunks = (len + CH - 1) / CH;
  float sum = 0.0f;
  for (int64_t c = 0; c < chunks; ++c) sum += partial[(first + c) * KF + e];
  grad_weight[t * KF + e] = narrow<T>(sum);
}

template <typename T>
bool vec_ok(const void* a, const void* b, int64_t K, int64_t F) {
  constexpr int VPL = Geo<T>::VPL;
  return K % VPL == 0 && F % VPL == 0 && psa::aligned(a, 16) && psa::aligned(b, 16);
}

template <typename T>
int launch_fw(const void* x, const int64_t* index, const int64_t* ptr, const void* weight, const int64_t* out_index,
              const int64_t* tile_ptr, int64_t T_, int64_t K, int64_t F, int trans_w, int64_t blocks, int64_t col_tiles,
              void* out, hipStream_t s) {
  const bool vec = vec_ok<T>(x, weight, K, F);
  const T* xx = static_cast<const T*>(x);
  const T* ww = static_cast<const T*>(weight);
  T* oo = static_cast<T*>(out);
  const dim3 grid(static_cast<unsigned>(blocks)), block(THREADS);
#define PSA_SEG_FW(V, TR) \
  hipLaunchKernelGGL((seg_mm_kernel<T, V, TR>), grid, block, 0, s, xx, index, ptr, ww, out_index, tile_ptr, T_, K, F, \
                     col_tiles, oo)
  if (vec && trans_w) PSA_SEG_FW(true, true);
  else if (vec) PSA_SEG_FW(true, false);
  else if (trans_w) PSA_SEG_FW(false, true);
  else PSA_SEG_FW(false, false);
#undef PSA_SEG_FW
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

template <typename T>
int launch_bw(const void* x, const int64_t* index, const void* grad, const int64_t* out_index, const int64_t* ptr,
              const int64_t* work_ptr, const int64_t* part_ptr, int64_t T_, int64_t K, int64_t F, int64_t blocks,
              int64_t k_tiles, int64_t f_tiles, float* partial, int64_t partial_chunks, void* grad_weight,
              int64_t fold_blocks, int64_t fold_per, hipStream_t s) {
  const T* xx = static_cast<const T*>(x);
  const T* gg = static_cast<const T*>(grad);
  T* ww = static_cast<T*>(grad_weight);
  const dim3 grid(static_cast<unsigned>(blocks)), block(THREADS);
  if (vec_ok<T>(x, grad, K, F))
    hipLaunchKernelGGL((seg_mm_bw_kernel<T, true>), grid, block, 0, s, xx, index, gg, out_index, ptr, work_ptr,
                       part_ptr, T_, K, F, k_tiles, f_tiles, partial, ww);
  else
    hipLaunchKernelGGL((seg_mm_bw_kernel<T, false>), grid, block, 0, s, xx, index, gg, out_index, ptr, work_ptr,
                       part_ptr, T_, K, F, k_tiles, f_tiles, partial, ww);
  PSA_LAUNCH_CHECK();
  if (partial_chunks > 0) {
    hipLaunchKernelGGL((seg_mm_fold_kernel<T>), dim3(static_cast<unsigned>(fold_blocks)), block, 0, s, ptr, part_ptr,
                       K * F, fold_per, partial, ww);
    PSA_LAUNCH_CHECK();
  }
  return PSA_OK;
}

constexpr int64_t kMaxGrid = 0xffffffffLL / THREADS;  // a launch holds fewer than 2^32 threads

}  // namespace

extern "C" {

int psa_segment_matmul_tile(int* bm, int* bn, int* bk, int* ch) {
  PSA_REQUIRE(bm && bn && bk && ch, "NULL pointer");
  *bm = BM;
  *bn = BN;
  *bk = BK;
  *ch = CH;
  return PSA_OK;
}

int64_t psa_segment_matmul_bw_chunks(int64_t R) { return R > 0 ? 2 * psa::ceil_div(R, CH) : 0; }

int psa_segment_matmul(int dtype, const void* x, const int64_t* index, const int64_t* ptr, const void* weight,
                       const int64_t* out_index, int64_t Nx, int64_t R, int64_t T, int64_t K, int64_t F, int trans_w,
                       int64_t* tile_ptr, void* out, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(Nx >= 0 && R >= 0 && T >= 0 && K >= 1 && F >= 1, "negative size, or K or F below 1");
  PSA_REQUIRE(index || Nx == R, "without index, x has one row per output row (Nx == R)");
  if (R == 0 || T == 0) return PSA_OK;
  PSA_REQUIRE(x && ptr && weight && tile_ptr && out, "NULL required pointer");
  PSA_REQUIRE(Nx > 0, "rows are asked of an x without rows");
  const int64_t col_tiles = psa::ceil_div(F, BN), row_tiles = psa::ceil_div(R, BM) + T;
  PSA_REQUIRE(row_tiles <= kMaxGrid / col_tiles, "the tile grid does not fit one launch");
  hipStream_t s = psa::as_stream(stream);
  hipLaunchKernelGGL((seg_map_kernel<false>), dim3(1), dim3(THREADS), 0, s, ptr, T, tile_ptr,
                     static_cast<int64_t*>(nullptr));
  PSA_LAUNCH_CHECK();
  if (dtype == PSA_F32)
    return launch_fw<float>(x, index, ptr, weight, out_index, tile_ptr, T, K, F, trans_w, row_tiles * col_tiles,
                            col_tiles, out, s);
  return launch_fw<uint16_t>(x, index, ptr, weight, out_index, tile_ptr, T, K, F, trans_w, row_tiles * col_tiles,
                             col_tiles, out, s);
}

int psa_segment_matmul_bw_weight(int dtype, const void* x, const int64_t* index, const void* grad,
                                 const int64_t* out_index, const int64_t* ptr, int64_t Nx, int64_t R, int64_t T,
                                 int64_t K, int64_t F, int64_t* chunk_ptr, float* partial, int64_t partial_chunks,
                                 void* grad_weight, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(Nx >= 0 && R >= 0 && T >= 0 && K >= 1 && F >= 1 && partial_chunks >= 0,
              "negative size, or K or F below 1");
  PSA_REQUIRE(index || Nx == R, "without index, x has one row per output row (Nx == R)");
  if (T == 0) return PSA_OK;
  PSA_REQUIRE(ptr && chunk_ptr && grad_weight, "NULL required pointer");
  PSA_REQUIRE(R == 0 || (x && grad && Nx > 0), "NULL required pointer");
  PSA_REQUIRE(partial_chunks >= psa_segment_matmul_bw_chunks(R) && (partial || partial_chunks == 0),
              "partial must hold psa_segment_matmul_bw_chunks(R) chunks of K * F floats");
  const int64_t k_tiles = psa::ceil_div(K, BM), f_tiles = psa::ceil_div(F, BN);
  const int64_t items = T + psa_segment_matmul_bw_chunks(R), fold_per = psa::ceil_div(K * F, THREADS);
  PSA_REQUIRE(k_tiles <= kMaxGrid / f_tiles && items <= kMaxGrid / (k_tiles * f_tiles) && T <= kMaxGrid / fold_per,
              "the tile grid does not fit one launch");
  hipStream_t s = psa::as_stream(stream);
  int64_t* work_ptr = chunk_ptr;
  int64_t* part_ptr = chunk_ptr + T + 1;
  hipLaunchKernelGGL((seg_map_kernel<true>), dim3(1), dim3(THREADS), 0, s, ptr, T, work_ptr, part_ptr);
  PSA_LAUNCH_CHECK();
  if (dtype == PSA_F32)
    return launch_bw<float>(x, index, grad, out_index, ptr, work_ptr, part_ptr, T, K, F, items * k_tiles * f_tiles,
                            k_tiles, f_tiles, partial, partial_chunks, grad_weight, T * fold_per, fold_per, s);
  return launch_bw<uint16_t>(x, index, grad, out_index, ptr, work_ptr, part_ptr, T, K, F, items * k_tiles * f_tiles,
                             k_tiles, f_tiles, partial, partial_chunks, grad_weight, T * fold_per, fold_per, s);
}

}  // extern "C"
