// typed_spmm: out[i] = sum over the stored entries e = (i, j) of type t of v_e * x[j] @ weight[t], and its weight
// gradient, aggregate first and transform second, on MFMA.  No message [nnz, F] is ever formed.
//
// The entries come in the order of a RelationalPlan (typed_spmm.py): by (tile of BM = 64 rows, type, row).  A
// SEGMENT is the run of one (tile, type); the identity is out[tile rows] = sum over the tile's segments of
// H_t @ weight[t] with H_t = (A_t x)[tile rows].
//
// Forward: one workgroup of four waves owns one row tile and keeps its 64 x BN fp32 result in MFMA accumulators from
// start to finish, BN = 64 (F <= 64: waves 2 x 2, 16 accumulators per lane) or 128 (waves 2 x 2, two 32 x 32 sub-tiles
// side by side per wave, 32 accumulators), so the gather runs once per tile up to F = 128.  Per segment and per slab of
// KS = 128 columns of x:
//   1. aggregate(): H[64][KS] in LDS.  Each wave owns 16 of the tile's rows and finds its sub-range of the segment
//      (sorted by row): a segment of at most PASS = 64 entries is read whole, one entry per lane, and two ballots on
//      the tile-local rows give the range; a longer one takes two searches and passes of 64.  Lanes span K, two
//      columns per lane.  The column ids, rows and scales that the lanes hold go round by readlane; the wave
//      keeps FLY = 8 row gathers in flight, sums a run of one row in registers (fp32) and stores the finished row
//      once, rounded to the operand type; rows without entries are stored as zeros on the way.  Every row of H has one
//      writer and is written exactly once: no zero pass, no LDS atomics.
//   2. acc += H @ weight[t][slab, BN columns], weight staged global -> registers -> LDS in BK = 32 steps, double
//      buffered, the first tile of a slab travelling while stage 1 gathers.
// LDS layout: every operand tile is tile[m or n][reduction index contiguous + 16 bytes of pad], as in
// segment_matmul.hip: a lane reads ONE 16-byte word per operand and step group; the row strides (H: 528 / 272 bytes,
// weight: 144 / 80 bytes) are 16-byte aligned and 4 or 20 banks mod 32, so the eight rows of one pass of a 16-byte
// read cover the 32 banks once.
//
// Weight gradient: grad_weight[t] = sum over the tiles of H_t^T @ G[tile rows].  A work item is a chunk of at most
// CS = 128 consecutive segments of one type (the plan's by-type order) times one 64 x 64 tile of [K, F]; per
// segment it runs aggregate() with a transposed store (H^T[k][m], the tile's rows m are the reduction index), loads
// the tile's 64 rows of grad_out transposed, and runs 64 reduction steps on MFMA.  A type with one chunk writes
// grad_weight[t], a type with more writes fp32 partials that a fold kernel sums in chunk order.
//
// No atomics, no split of a sum over workgroups other than the chunks, whose order the plan fixes.
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int CS = 128;   // segments in a chunk of the weight gradient
constexpr int PASS = 64;  // entries whose ids one wave reads at once
constexpr int FLY = 8;    // row gathers a wave keeps in flight
constexpr int THREADS = 256;

// first entry e in [lo, hi) with lrow[e] >= r (hi if none); the same in every lane
__device__ __forceinline__ int64_t first_at_or_above(const uint8_t* __restrict__ lrow, int64_t lo, int64_t hi, int r) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (lrow[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// largest t in [0, T) with table[t] <= w, for table[0] = 0 <= w < table[T]
__device__ __forceinline__ int64_t owner_of(const int64_t* table, int64_t T, int64_t w) {
  int64_t lo = 0, hi = T;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (table[mid] <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- stage 1 --------------------------------------------------------------------------------------------------
// H[r][c] = sum over the entries e in [e0, e1) with lrow[e] = r of scale[e] * x[col[e]][k0 + c], for the 16 rows r of
// this wave and the 64 * CPL columns c of the slab, stored at H[r * SR + c * SC] (SR = row stride and SC = 1 in the
// forward; SR = 1 and SC = row stride for the transposed tile of the weight gradient).  Columns at or past K hold
// zeros.  PAIR (CPL = 2): the lane owns columns 2 * lane and 2 * lane + 1 and moves them as one word (K even, x
// aligned); otherwise it owns lane and lane + 64 and moves elements.
template <typename T, int CPL, bool PAIR, int SR, int SC>
__device__ __forceinline__ void aggregate(const T* __restrict__ x, const float* __restrict__ scale,
                                          const int32_t* __restrict__ col, const uint8_t* __restrict__ lrow,
                                          int64_t e0, int64_t e1, int64_t K, int64_t k0, T* __restrict__ H) {
  static_assert(!PAIR || CPL == 2, "a pair is two columns");
  const int lane = threadIdx.x % 64;
  const int r0 = __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * (BM / 4);

  int c[CPL];
  bool live[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    c[j] = PAIR ? 2 * lane + j : lane + 64 * j;
    live[j] = k0 + c[j] < K;
  }
  auto put = [&](int r, const float* s) {
    if constexpr (PAIR && SC == 1) {
      T pair[2] = {narrow<T>(s[0]), narrow<T>(s[1])};
      if constexpr (sizeof(T) == 4) *reinterpret_cast<uint2*>(H + r * SR + c[0]) = *reinterpret_cast<uint2*>(pair);
      else *reinterpret_cast<uint32_t*>(H + r * SR + c[0]) = *reinterpret_cast<uint32_t*>(pair);
    } else {
#pragma unroll
      for (int j = 0; j < CPL; ++j) H[r * SR + c[j] * SC] = narrow<T>(s[j]);
    }
  };
  float sum[CPL], zero[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) sum[j] = zero[j] = 0.0f;
  int next = r0;  // the first row of this wave that is not stored yet
  int cur = -1;   // the row whose run is being summed
  auto finish = [&](int upto) {  // stores the open run, and zeros for the rows below `upto` that have no entries
    if (cur >= 0) {
      for (; next < cur; ++next) put(next, zero);
      put(cur, sum);
      next = cur + 1;
    }
    for (; next < upto; ++next) put(next, zero);
  };

  // the entries that lanes a .. a + n - 1 hold, FLY row gathers in flight
  auto pass = [&](int my_col, int my_row, float my_scale, int a, int n) {
    for (int u = 0; u < n; u += FLY) {
      T v[FLY][CPL];
      int row[FLY];
      float s[FLY];
#pragma unroll
      for (int i = 0; i < FLY; ++i) {
        const int src = a + (u + i < n ? u + i : n - 1);  // past the end: the last entry again, not added below
        const T* __restrict__ p = x + static_cast<int64_t>(__builtin_amdgcn_readlane(my_col, src)) * K + k0;
        row[i] = __builtin_amdgcn_readlane(my_row, src);
        s[i] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_scale), src));
        if constexpr (PAIR) {
          T pair[2] = {T(0), T(0)};
          if (live[0]) {
            if constexpr (sizeof(T) == 4) *reinterpret_cast<uint2*>(pair) = *reinterpret_cast<const uint2*>(p + c[0]);
            else *reinterpret_cast<uint32_t*>(pair) = *reinterpret_cast<const uint32_t*>(p + c[0]);
          }
          v[i][0] = pair[0];
          v[i][1] = pair[1];
        } else {
#pragma unroll
          for (int j = 0; j < CPL; ++j) v[i][j] = live[j] ? p[c[j]] : T(0);
        }
      }
#pragma unroll
      for (int i = 0; i < FLY; ++i) {
        if (row[i] != cur) {
          finish(row[i]);
          cur = row[i];
#pragma unroll
          for (int j = 0; j < CPL; ++j) sum[j] = 0.0f;
        }
        if (u + i < n) {
#pragma unroll
          for (int j = 0; j < CPL; ++j) sum[j] += s[i] * widen<T>(v[i][j]);
        }
      }
    }
  };

  if (e1 - e0 <= PASS) {
    // the whole segment in one load per lane: the wave's rows are the lanes between two counts, no search
    const int64_t e = e0 + lane;
    const bool in = e < e1;
    const int my_row = in ? lrow[e] : 255, my_col = in ? col[e] : 0;
    const float my_scale = in && scale ? scale[e] : 1.0f;
    const int a = __popcll(__ballot(my_row < r0)), z = __popcll(__ballot(my_row < r0 + BM / 4));
    if (z > a) pass(my_col, my_row, my_scale, a, z - a);
  } else {
    const int64_t lo = first_at_or_above(lrow, e0, e1, r0), hi = first_at_or_above(lrow, lo, e1, r0 + BM / 4);
    for (int64_t b = lo; b < hi; b += PASS) {
      const int n = hi - b < PASS ? static_cast<int>(hi - b) : PASS;
      const int64_t e = b + (lane < n ? lane : n - 1);
      pass(col[e], lrow[e], scale ? scale[e] : 1.0f, 0, n);
    }
  }
  finish(r0 + BM / 4);
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, int NT, bool VEC, bool TRANS>
__global__ __launch_bounds__(THREADS) void typed_spmm_kernel(
    const T* __restrict__ x, const T* __restrict__ weight, const float* __restrict__ scale,
    const int32_t* __restrict__ col, const uint8_t* __restrict__ lrow, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ seg_type, const int64_t* __restrict__ tile_seg_ptr, int64_t M, int64_t K, int64_t F,
    int64_t col_tiles, T* __restrict__ out) {
  using G = Geo<T>;
  constexpr int VPL = G::VPL, LD = G::LD, LDH = G::LDH;
  constexpr int BN = 64 * NT;                    // columns of the workgroup's tile
  constexpr int NW = BN * BK / VPL / THREADS;    // 16-byte words of a weight tile per thread
  constexpr int KV = BK / VPL;                   // words of a row of a directly copied tile
  constexpr int NQ = BN / VPL;                   // words along n of a transposed tile
  __shared__ __attribute__((aligned(16))) T sH[BM * LDH];
  __shared__ __attribute__((aligned(16))) T sB[2][BN * LD];
  const int64_t tile = blockIdx.x / col_tiles, n0 = (blockIdx.x % col_tiles) * BN;
  const int64_t s0 = tile_seg_ptr[tile], s1 = tile_seg_ptr[tile + 1];
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, wm = wave / 2, wn = wave % 2;

  v16f acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[j][v] = 0.0f;

  int64_t e_next = s0 < s1 ? seg_ptr[s0] : 0, e_after = s0 < s1 ? seg_ptr[s0 + 1] : 0;
  int t_next = s0 < s1 ? seg_type[s0] : 0;
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t e0 = e_next, e1 = e_after;
    const T* __restrict__ w = weight + static_cast<int64_t>(t_next) * K * F;
    if (s + 1 < s1) {  // the next segment's bounds and type travel one segment ahead
      e_next = e1;
      e_after = seg_ptr[s + 2];
      t_next = seg_type[s + 1];
    }
    uint4 rb[NW];
    // weight[t][k .. k + BK][n0 .. n0 + BN] -> registers; TRANS: weight[t] is [F, K], rows of the tile are rows of memory
    auto fetch = [&](int64_t k) {
#pragma unroll
      for (int it = 0; it < NW; ++it) {
        const int word = tid + it * THREADS;
        if constexpr (TRANS) {
          const int64_t n = n0 + word / KV, kk = k + (word % KV) * VPL;
          rb[it] = load_word<T, VEC>(w + n * K + kk, n < F ? K - kk : 0);
        } else {
          // eight lanes with consecutive reduction indices share a word column: two-way conflicts on the stores
          const int64_t kk = k + (word / (8 * NQ)) * 8 + word % 8, n = n0 + ((word / 8) % NQ) * VPL;
          rb[it] = load_word<T, VEC>(w + kk * F + n, kk < K ? F - n : 0);
        }
      }
    };
    auto stash = [&](int buf) {
#pragma unroll
      for (int it = 0; it < NW; ++it) {
        const int word = tid + it * THREADS;
        if constexpr (TRANS) {
          *reinterpret_cast<uint4*>(sB[buf] + (word / KV) * LD + (word % KV) * VPL) = rb[it];
        } else {
          const int j = (word / (8 * NQ)) * 8 + word % 8, nq = (word / 8) % NQ;
          Word<T> q;
          q.q = rb[it];
#pragma unroll
          for (int i = 0; i < VPL; ++i) sB[buf][(nq * VPL + i) * LD + j] = q.e[i];
        }
      }
    };

    for (int64_t k0 = 0; k0 < K; k0 += KS) {
      const int width = K - k0 < KS ? static_cast<int>(K - k0) : KS;
      const int steps = (width + BK - 1) / BK;
      fetch(k0);  // travels while the rows are gathered
      aggregate<T, 2, VEC, LDH, 1>(x, scale, col, lrow, e0, e1, K, k0, sH);
      stash(0);
      __syncthreads();
      for (int st = 0; st < steps; ++st) {
        const int buf = st & 1;
        if (st + 1 < steps) fetch(k0 + (st + 1) * BK);
#pragma unroll
        for (int g = 0; g < BK / (2 * VPL); ++g) {
          const int k = g * 2 * VPL + (lane / 32) * VPL;
          const uint4 a = *reinterpret_cast<const uint4*>(sH + (wm * 32 + lane % 32) * LDH + st * BK + k);
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const uint4 b = *reinterpret_cast<const uint4*>(sB[buf] + ((wn * NT + j) * 32 + lane % 32) * LD + k);
            acc[j] = mfma(a, b, acc[j], T());
          }
        }
        if (st + 1 < steps) stash(buf ^ 1);
        __syncthreads();  // the last one also frees H and both weight buffers for the next slab or segment
      }
    }
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t n = n0 + (wn * NT + j) * 32 + lane % 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t r = tile * BM + wm * 32 + acc_row(v);
      if (r < M && n < F) out[r * F + n] = narrow<T>(acc[j][v]);
    }
  }
}

// ---- weight gradient --------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void typed_spmm_bw_kernel(
    const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ scale, const int32_t* __restrict__ col,
    const uint8_t* __restrict__ lrow, const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ seg_tile,
    const int64_t* __restrict__ type_seg_ptr, const int64_t* __restrict__ by_type, const int64_t* __restrict__ work_ptr,
    const int64_t* __restrict__ part_ptr, int64_t T_, int64_t M, int64_t K, int64_t F, int64_t k_tiles, int64_t f_tiles,
    float* __restrict__ partial, T* __restrict__ grad_weight) {
  using G = Geo<T>;
  constexpr int VPL = G::VPL, LDW = G::LDW;
  constexpr int FQ = 64 / VPL;                 // words of a row of the grad_out tile
  constexpr int NW = BM * FQ / THREADS;        // words per thread
  __shared__ __attribute__((aligned(16))) T sA[64 * LDW];  // H^T[k][m]
  __shared__ __attribute__((aligned(16))) T sB[64 * LDW];  // G^T[f][m]
  const int64_t per = k_tiles * f_tiles, item = blockIdx.x / per, rem = blockIdx.x % per;
  const int64_t t = owner_of(work_ptr, T_, item), c = item - work_ptr[t];
  const bool direct = work_ptr[t + 1] - work_ptr[t] == 1;
  const int64_t b0 = type_seg_ptr[t] + c * CS, bend = type_seg_ptr[t + 1], b1 = bend < b0 + CS ? bend : b0 + CS;
  const int64_t k0 = (rem / f_tiles) * 64, f0 = (rem % f_tiles) * 64;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, wm = wave / 2, wn = wave % 2;

  v16f acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t s = by_type[b], row0 = static_cast<int64_t>(seg_tile[s]) * BM;
    uint4 rg[NW];
#pragma unroll
    for (int it = 0; it < NW; ++it) {  // travels while the rows are gathered
      const int word = tid + it * THREADS;
      const int64_t m = row0 + (word / (8 * FQ)) * 8 + word % 8, f = f0 + ((word / 8) % FQ) * VPL;
      rg[it] = load_word<T, VEC>(g + m * F + f, m < M ? F - f : 0);
    }
    aggregate<T, 1, false, 1, LDW>(x, scale, col, lrow, seg_ptr[s], seg_ptr[s + 1], K, k0, sA);
#pragma unroll
    for (int it = 0; it < NW; ++it) {
      const int word = tid + it * THREADS;
      const int m = (word / (8 * FQ)) * 8 + word % 8, fq = (word / 8) % FQ;
      Word<T> q;
      q.q = rg[it];
#pragma unroll
      for (int i = 0; i < VPL; ++i) sB[(fq * VPL + i) * LDW + m] = q.e[i];
    }
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < BM / (2 * VPL); ++grp) {
      const int m = grp * 2 * VPL + (lane / 32) * VPL;
      const uint4 a = *reinterpret_cast<const uint4*>(sA + (wm * 32 + lane % 32) * LDW + m);
      const uint4 bb = *reinterpret_cast<const uint4*>(sB + (wn * 32 + lane % 32) * LDW + m);
      acc = mfma(a, bb, acc, T());
    }
    __syncthreads();
  }

  const int64_t f = f0 + wn * 32 + lane % 32;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t k = k0 + wm * 32 + acc_row(v);
    if (k < K && f < F) {
      if (direct) grad_weight[(t * K + k) * F + f] = narrow<T>(acc[v]);
      else partial[((part_ptr[t] + c) * K + k) * F + f] = acc[v];
    }
  }
}

// folds the fp32 partials of every type with more than one chunk in chunk order; one thread per element
template <typename T>
__global__ __launch_bounds__(THREADS) void typed_spmm_fold_kernel(const int64_t* __restrict__ work_ptr,
                                                                  const int64_t* __restrict__ part_ptr, int64_t KF,
                                                                  int64_t blocks_per, const float* __restrict__ partial,
                                                                  T* __restrict__ grad_weight) {
  const int64_t t = blockIdx.x / blocks_per, e = (blockIdx.x % blocks_per) * THREADS + threadIdx.x;
  const int64_t chunks = work_ptr[t + 1] - work_ptr[t];
  if (chunks <= 1 || e >= KF) return;
  const int64_t first = part_ptr[t];
  float sum = 0.0f;
  for (int64_t c = 0; c < chunks; ++c) sum += partial[(first + c) * KF + e];
  grad_weight[t * KF + e] = narrow<T>(sum);
}

template <typename T>
bool vec_ok(const void* a, const void* b, int64_t K, int64_t F) {
  constexpr int VPL = Geo<T>::VPL;
  return K % VPL == 0 && F % VPL == 0 && psa::aligned(a, 16) && psa::aligned(b, 16);
}

template <typename T, int NT>
void launch_fw_nt(bool vec, int trans_w, dim3 grid, hipStream_t s, const T* x, const T* w, const float* scale,
                  const int32_t* col, const uint8_t* lrow, const int64_t* seg_ptr, const int32_t* seg_type,
                  const int64_t* tile_seg_ptr, int64_t M, int64_t K, int64_t F, int64_t col_tiles, T* out) {
  const dim3 block(THREADS);
#define PSA_TYPED_FW(V, TR)                                                                                       \
  hipLaunchKernelGGL((typed_spmm_kernel<T, NT, V, TR>), grid, block, 0, s, x, w, scale, col, lrow, seg_ptr, seg_type, \
                     tile_seg_ptr, M, K, F, col_tiles, out)
  if (vec && trans_w) PSA_TYPED_FW(true, true);
  else if (vec) PSA_TYPED_FW(true, false);
  else if (trans_w) PSA_TYPED_FW(false, true);
  else PSA_TYPED_FW(false, false);
#undef PSA_TYPED_FW
}

constexpr int64_t kMaxGrid = 0xffffffffLL / THREADS;  // a launch holds fewer than 2^32 threads

template <typename T>
int launch_fw(const void* x, const void* weight, const float* scale, const int32_t* col, const uint8_t* lrow,
              const int64_t* seg_ptr, const int32_t* seg_type, const int64_t* tile_seg_ptr, int64_t M, int64_t K,
              int64_t F, int trans_w, void* out, hipStream_t s) {
  const bool vec = vec_ok<T>(x, weight, K, F), wide = F > 64;
  const int64_t col_tiles = psa::ceil_div(F, wide ? 128 : 64), tiles = psa::ceil_div(M, BM);
  PSA_REQUIRE(tiles <= kMaxGrid / col_tiles, "the tile grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(tiles * col_tiles));
  if (wide)
    launch_fw_nt<T, 2>(vec, trans_w, grid, s, static_cast<const T*>(x), static_cast<const T*>(weight), scale, col,
                       lrow, seg_ptr, seg_type, tile_seg_ptr, M, K, F, col_tiles, static_cast<T*>(out));
  else
    launch_fw_nt<T, 1>(vec, trans_w, grid, s, static_cast<const T*>(x), static_cast<const T*>(weight), scale, col,
                       lrow, seg_ptr, seg_type, tile_seg_ptr, M, K, F, col_tiles, static_cast<T*>(out));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

template <typename T>
int launch_bw(const void* x, const void* grad, const float* scale, const int32_t* col, const uint8_t* lrow,
              const int64_t* seg_ptr, const int32_t* seg_tile, const int64_t* type_seg_ptr, const int64_t* by_type,
              const int64_t* work_ptr, const int64_t* part_ptr, int64_t items, int64_t T_, int64_t M, int64_t K,
              int64_t F, float* partial, void* grad_weight, hipStream_t s) {
  const int64_t k_tiles = psa::ceil_div(K, 64), f_tiles = psa::ceil_div(F, 64);
  PSA_REQUIRE(k_tiles <= kMaxGrid / f_tiles && items <= kMaxGrid / (k_tiles * f_tiles),
              "the tile grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(items * k_tiles * f_tiles)), block(THREADS);
  const T* xx = static_cast<const T*>(x);
  const T* gg = static_cast<const T*>(grad);
  T* ww = static_cast<T*>(grad_weight);
  if (F % Geo<T>::VPL == 0 && psa::aligned(grad, 16))
    hipLaunchKernelGGL((typed_spmm_bw_kernel<T, true>), grid, block, 0, s, xx, gg, scale, col, lrow, seg_ptr, seg_tile,
                       type_seg_ptr, by_type, work_ptr, part_ptr, T_, M, K, F, k_tiles, f_tiles, partial, ww);
  else
    hipLaunchKernelGGL((typed_spmm_bw_kernel<T, false>), grid, block, 0, s, xx, gg, scale, col, lrow, seg_ptr, seg_tile,
                       type_seg_ptr, by_type, work_ptr, part_ptr, T_, M, K, F, k_tiles, f_tiles, partial, ww);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

int psa_typed_spmm_tile(int* bm, int* bk, int* ks, int* cs, int* pass) {
  PSA_REQUIRE(bm && bk && ks && cs && pass, "NULL pointer");
  *bm = BM;
  *bk = BK;
  *ks = KS;
  *cs = CS;
  *pass = PASS;
  return PSA_OK;
}

int psa_typed_spmm(int dtype, const void* x, const void* weight, const float* scale, const int32_t* col,
                   const uint8_t* lrow, const int64_t* seg_ptr, const int32_t* seg_type, const int64_t* tile_seg_ptr,
                   int64_t M, int64_t N, int64_t nnz, int64_t T, int64_t K, int64_t F, int trans_w, void* out,
                   psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && T >= 0 && K >= 1 && F >= 1, "negative size, or K or F below 1");
  if (M == 0) return PSA_OK;
  PSA_REQUIRE(seg_ptr && tile_seg_ptr && out, "NULL required pointer");
  PSA_REQUIRE(nnz == 0 || (x && weight && col && lrow && seg_type && N > 0 && T > 0), "entries without their operands");
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32)
    return launch_fw<float>(x, weight, scale, col, lrow, seg_ptr, seg_type, tile_seg_ptr, M, K, F, trans_w, out, s);
  return launch_fw<uint16_t>(x, weight, scale, col, lrow, seg_ptr, seg_type, tile_seg_ptr, M, K, F, trans_w, out, s);
}

int psa_typed_spmm_bw_weight(int dtype, const void* x, const void* grad, const float* scale, const int32_t* col,
                             const uint8_t* lrow, const int64_t* seg_ptr, const int32_t* seg_tile,
                             const int64_t* type_seg_ptr, const int64_t* by_type, const int64_t* work_ptr,
                             const int64_t* part_ptr, int64_t items, int64_t partial_chunks, int64_t M, int64_t N,
                             int64_t nnz, int64_t T, int64_t K, int64_t F, float* partial, void* grad_weight,
                             psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && T >= 0 && K >= 1 && F >= 1 && partial_chunks >= 0,
              "negative size, or K or F below 1");
  if (T == 0) return PSA_OK;
  PSA_REQUIRE(items >= T && items <= T + partial_chunks, "every type has a work item, and every further one a partial");
  PSA_REQUIRE(seg_ptr && type_seg_ptr && work_ptr && part_ptr && grad_weight && (partial || partial_chunks == 0),
              "NULL required pointer");
  PSA_REQUIRE(nnz == 0 || (x && grad && col && lrow && seg_tile && by_type && N > 0 && M > 0),
              "entries without their operands");
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32)
    return launch_bw<float>(x, grad, scale, col, lrow, seg_ptr, seg_tile, type_seg_ptr, by_type, work_ptr, part_ptr,
                            items, T, M, K, F, partial, grad_weight, s);
  return launch_bw<uint16_t>(x, grad, scale, col, lrow, seg_ptr, seg_tile, type_seg_ptr, by_type, work_ptr, part_ptr,
                             items, T, M, K, F, partial, grad_weight, s);
}

int psa_typed_spmm_bw_fold(int dtype, const int64_t* work_ptr, const int64_t* part_ptr, int64_t T, int64_t K,
                           int64_t F, const float* partial, void* grad_weight, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(T >= 0 && K >= 1 && F >= 1, "negative size, or K or F below 1");
  if (T == 0) return PSA_OK;
  PSA_REQUIRE(work_ptr && part_ptr && partial && grad_weight, "NULL required pointer");
  const int64_t per = psa::ceil_div(K * F, THREADS);
  PSA_REQUIRE(T <= kMaxGrid / per, "the grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(T * per)), block(THREADS);
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32)
    hipLaunchKernelGGL((typed_spmm_fold_kernel<float>), grid, block, 0, s, work_ptr, part_ptr, K * F, per, partial,
                       static_cast<float*>(grad_weight));
  else
    hipLaunchKernelGGL((typed_spmm_fold_kernel<uint16_t>), grid, block, 0, s, work_ptr, part_ptr, K * F, per, partial,
                       static_cast<uint16_t*>(grad_weight));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"
