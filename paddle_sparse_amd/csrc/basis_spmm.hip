// basis_spmm: the RGCN basis decomposition W_t = sum over b of comp[t][b] * V_b, fused with the aggregation:
//   out[i] = sum over the stored entries e = (i, j) of type t of v_e * x[j] @ W_t = sum over b of Z_b[i] @ V_b,
//   Z_b[i] = sum over the entries e of row i of v_e * comp[t_e][b] * x[col_e].
// The entries stay in CSR order; the type is a scalar per entry that picks a row of the small comp table, so the work
// is 2 nnz K B VALU flops plus 2 M B K F MFMA flops whatever the number of types.  No [T, K, F] weight, no message
// [nnz, F], no type sort, no atomics.
//
// Forward (and with `trans` the gradient wrt x on the CSC view): one workgroup of four waves owns a tile of BM = 64 rows
// and keeps its 64 x BN fp32 result (BN = 64 or 128, as in typed_spmm.hip) in MFMA accumulators from the first basis to
// the last.  Per group of G = 4 bases and per slab of KB = 64 columns of x:
//   1. aggregate(): Z[G][64][KB] in LDS.  A wave owns 16 rows, whose entries are ONE contiguous range of the CSR arrays:
//      lanes 0 .. 16 hold the 17 row offsets, the wave reads PASS = 64 (col, type, scale) triples at a time, one per lane,
//      hands them round by readlane and keeps FLY = 8 row gathers in flight.  Lanes span the slab, one column per lane:
//      a row of x is gathered ONCE and multiplied into G sums with scale * comp[type][b0 + g], a wave-uniform scalar that
//      comes by a scalar load from a table of T * B floats.  A row's sums are stored once when its range ends, rounded to
//      the operand type; rows without entries store zeros on the way: one writer per row, no zero pass, no LDS atomics.
//   2. acc += Z_g @ V_(b0 + g)[slab, BN columns] for the group's bases: one reduction of up to G * KB, the weight tiles
//      staged global -> registers -> LDS in BK = 32 steps, double buffered, the first one travelling while stage 1 gathers.
// Why G = 4 and KB = 64: Z costs G * 64 * (KB + pad) elements of LDS.  fp32: 4 * 64 * 68 * 4 = 69632 bytes plus
// 18432 / 36864 bytes of weight buffers = 88064 / 106496 of 163840: one workgroup per CU; G = 8 would not fit with
// KB = 64, and KB = 32 would leave half of the lanes of a gather idle.  bf16: 36864 + 10240 / 20480 = 47104 / 57344
// bytes, three / two workgroups per CU.  The gather of x, the col / type / scale reads and the row bookkeeping are shared
// by four bases; the G sums cost four registers.
// LDS layout: every operand tile is tile[m or n][reduction index contiguous + 16 bytes of pad].  Row strides: Z and its
// transposed forms 272 bytes (fp32) / 144 bytes (bf16), weight tiles 144 / 80 bytes: 16-byte aligned and 4 or 20 banks
// mod 32, so the eight rows of one pass of a 16-byte read cover the 32 banks once.
//
// Basis gradient: grad_basis[b] = sum over the tiles of Z_b^T @ G[tile rows].  A work item is a chunk of TC = 64
// consecutive row tiles times one 64 x 64 tile of [K, F] times one group of G bases; per tile it runs aggregate() with a
// transposed store (Z^T[g][k][m]), loads the tile's rows of grad_out transposed and runs 64 reduction steps per basis on
// MFMA (G accumulator tiles).  Tiles without entries are skipped.  One chunk writes grad_basis, more write fp32
// partials that a fold kernel sums in chunk order.
//
// Coefficient gradient: s[e][b] = v_e * <x[col_e], P_b[row_e]> with P_b = G[tile rows] @ V_b^T, [64, KB] per basis, by
// MFMA into LDS (rounded once to the operand type), then the same walk over the entries: a gathered row of x is dotted
// with G rows of P, the FLY * G = 32 partial dots of a batch are folded across the lanes by one transposing fold
// (lane_fold.h) and lane i * G + g writes s[e_i][b0 + g].  With K above KB the same lane adds the later slabs to what
// it wrote.  The reduction over the types is the caller's (a gather through the by-type order and segment_csr).
#include "common.h"
#include "lane_fold.h"
#include "mfma_tile.h"

namespace {

constexpr int G = 4;      // bases that share one gather of x
constexpr int KB = 64;    // columns of x in one slab of Z: one per lane
constexpr int TC = 64;    // row tiles in a chunk of the basis gradient
constexpr int PASS = 64;  // entries whose ids one wave reads at once
constexpr int FLY = 8;    // row gathers a wave keeps in flight
constexpr int THREADS = 256;
constexpr int ROWS = BM / 4;  // rows of a wave
static_assert(KB == BM && KB % BK == 0 && FLY * G <= 64, "Z and Z^T share one stride; a batch folds in one wave");

__device__ __forceinline__ int64_t readlane64(int64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v)), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint64_t>(v) >> 32), src);
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// the 17 offsets of this wave's 16 rows, one per lane 0 .. 16; rows at or past M are empty
__device__ __forceinline__ int64_t wave_offsets(const int64_t* __restrict__ rowptr, int64_t M, int64_t row0) {
  const int lane = threadIdx.x % 64;
  const int r0 = __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * ROWS;
  const int64_t r = row0 + r0 + (lane <= ROWS ? lane : 0);
  return rowptr[r < M ? r : M];
}

__device__ __forceinline__ bool tile_is_empty(const int64_t* __restrict__ rowptr, int64_t M, int64_t row0) {
  return rowptr[row0 < M ? row0 : M] == rowptr[row0 + BM < M ? row0 + BM : M];
}

// ---- stage 1 --------------------------------------------------------------------------------------------------
// Z[g][r][c] = sum over the entries e of row row0 + r of scale[e] * comp[etype[e]][b0 + g] * x[col[e]][k0 + c] for the 16
// rows r of this wave, g < G and the KB columns c of the slab, stored at Z[g * BM * LDW + r * SR + c * SC] (SR = LDW and
// SC = 1 in the forward; SR = 1 and SC = LDW for the transposed tile of the basis gradient).  Columns at or past K and
// bases at or past B hold zeros.
template <typename T, int SR, int SC>
__device__ __forceinline__ void aggregate(const T* __restrict__ x, const float* __restrict__ comp,
                                          const float* __restrict__ scale, const int64_t* __restrict__ rowptr,
                                          const int32_t* __restrict__ col, const int32_t* __restrict__ etype, int64_t M,
                                          int64_t row0, int64_t K, int64_t k0, int64_t B, int64_t b0,
                                          T* __restrict__ Z) {
  constexpr int GZ = BM * Geo<T>::LDW;
  const int lane = threadIdx.x % 64;
  const int r0 = __builtin_amdgcn_readfirstlane(threadIdx.x / 64) * ROWS;
  const int64_t my_ptr = wave_offsets(rowptr, M, row0);
  const int64_t begin = readlane64(my_ptr, 0), end = readlane64(my_ptr, ROWS);
  const bool live = k0 + lane < K;

  float sum[G];
#pragma unroll
  for (int g = 0; g < G; ++g) sum[g] = 0.0f;
  int cur = 0;  // the row whose range is being summed
  int64_t end_cur = readlane64(my_ptr, 1);
  auto put = [&]() {  // stores the sums of row cur and clears them
#pragma unroll
    for (int g = 0; g < G; ++g) {
      Z[g * GZ + (r0 + cur) * SR + lane * SC] = narrow<T>(sum[g]);
      sum[g] = 0.0f;
    }
  };

  for (int64_t b = begin; b < end; b += PASS) {
    const int n = end - b < PASS ? static_cast<int>(end - b) : PASS;
    const int64_t e = b + (lane < n ? lane : n - 1);
    const int my_col = col[e], my_type = etype[e];
    const float my_scale = scale ? scale[e] : 1.0f;
    for (int u = 0; u < n; u += FLY) {
      T v[FLY];
      float w[FLY][G];
#pragma unroll
      for (int i = 0; i < FLY; ++i) {
        const int src = u + i < n ? u + i : n - 1;  // past the end: the last entry again, not added below
        const T* __restrict__ p = x + static_cast<int64_t>(__builtin_amdgcn_readlane(my_col, src)) * K + k0;
        const float* __restrict__ c = comp + static_cast<int64_t>(__builtin_amdgcn_readlane(my_type, src)) * B + b0;
        const float s = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_scale), src));
        v[i] = live ? p[lane] : T(0);
#pragma unroll
        for (int g = 0; g < G; ++g) w[i][g] = b0 + g < B ? s * c[g] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < FLY; ++i) {
        if (u + i < n) {
          while (b + u + i >= end_cur) {  // ends below `end`, so cur stays below ROWS
            put();
            ++cur;
            end_cur = readlane64(my_ptr, cur + 1);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) sum[g] += w[i][g] * widen<T>(v[i]);
        }
      }
    }
  }
  for (;;) {
    put();
    if (++cur == ROWS) break;
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------
template <typename T, int NT, bool VEC, bool TRANS>
__global__ __launch_bounds__(THREADS) void basis_spmm_kernel(
    const T* __restrict__ x, const T* __restrict__ basis, const float* __restrict__ comp,
    const float* __restrict__ scale, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ etype, int64_t M, int64_t K, int64_t F, int64_t B, int64_t col_tiles,
    T* __restrict__ out) {
  using Ge = Geo<T>;
  constexpr int VPL = Ge::VPL, LD = Ge::LD, LDZ = Ge::LDW;
  constexpr int BN = 64 * NT;                    // columns of the workgroup's tile
  constexpr int NW = BN * BK / VPL / THREADS;    // 16-byte words of a weight tile per thread
  constexpr int KV = BK / VPL;                   // words of a row of a directly copied tile
  constexpr int NQ = BN / VPL;                   // words along n of a transposed tile
  __shared__ __attribute__((aligned(16))) T sZ[G * BM * LDZ];
  __shared__ __attribute__((aligned(16))) T sB[2][BN * LD];
  const int64_t tile = blockIdx.x / col_tiles, n0 = (blockIdx.x % col_tiles) * BN, row0 = tile * BM;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, wm = wave / 2, wn = wave % 2;

  v16f acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[j][v] = 0.0f;

  uint4 rb[NW];
  // basis[b][k .. k + BK][n0 .. n0 + BN] -> registers; TRANS: basis[b] is [F, K], rows of the tile are rows of memory
  auto fetch = [&](int64_t b, int64_t k) {
    const T* __restrict__ w = basis + b * K * F;
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

  if (!tile_is_empty(rowptr, M, row0)) {
    for (int64_t b0 = 0; b0 < B; b0 += G) {
      const int gc = B - b0 < G ? static_cast<int>(B - b0) : G;
      for (int64_t k0 = 0; k0 < K; k0 += KB) {
        const int width = K - k0 < KB ? static_cast<int>(K - k0) : KB;
        const int steps = (width + BK - 1) / BK, Q = gc * steps;
        fetch(b0, k0);  // travels while the rows are gathered
        aggregate<T, LDZ, 1>(x, comp, scale, rowptr, col, etype, M, row0, K, k0, B, b0, sZ);
        stash(0);
        __syncthreads();
        for (int q = 0; q < Q; ++q) {
          const int buf = q & 1, g = q / steps, st = q % steps;
          if (q + 1 < Q) fetch(b0 + (q + 1) / steps, k0 + ((q + 1) % steps) * BK);
#pragma unroll
          for (int grp = 0; grp < BK / (2 * VPL); ++grp) {
            const int k = grp * 2 * VPL + (lane / 32) * VPL;
            const uint4 a =
                *reinterpret_cast<const uint4*>(sZ + g * BM * LDZ + (wm * 32 + lane % 32) * LDZ + st * BK + k);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              const uint4 b = *reinterpret_cast<const uint4*>(sB[buf] + ((wn * NT + j) * 32 + lane % 32) * LD + k);
              acc[j] = mfma(a, b, acc[j], T());
            }
          }
          if (q + 1 < Q) stash(buf ^ 1);
          __syncthreads();  // the last one also frees Z and both weight buffers for the next slab or group
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t n = n0 + (wn * NT + j) * 32 + lane % 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int64_t r = row0 + wm * 32 + acc_row(v);
      if (r < M && n < F) out[r * F + n] = narrow<T>(acc[j][v]);
    }
  }
}

// ---- basis gradient ---------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void basis_spmm_bw_basis_kernel(
    const T* __restrict__ x, const T* __restrict__ gr, const float* __restrict__ comp, const float* __restrict__ scale,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ etype, int64_t M,
    int64_t K, int64_t F, int64_t B, int64_t tiles, int64_t chunks, int64_t groups, int64_t k_tiles, int64_t f_tiles,
    float* __restrict__ partial, T* __restrict__ grad_basis) {
  using Ge = Geo<T>;
  constexpr int VPL = Ge::VPL, LDW = Ge::LDW;
  constexpr int FQ = 64 / VPL;                 // words of a row of the grad_out tile
  constexpr int NW = BM * FQ / THREADS;        // words per thread
  __shared__ __attribute__((aligned(16))) T sA[G * BM * LDW];  // Z^T[g][k][m]
  __shared__ __attribute__((aligned(16))) T sB[64 * LDW];      // G^T[f][m]
  const int64_t per = k_tiles * f_tiles, item = blockIdx.x / per, rem = blockIdx.x % per;
  const int64_t chunk = item / groups, b0 = (item % groups) * G;
  const int64_t k0 = (rem / f_tiles) * 64, f0 = (rem % f_tiles) * 64;
  const int64_t t0 = chunk * TC, t1 = t0 + TC < tiles ? t0 + TC : tiles;
  const int gc = B - b0 < G ? static_cast<int>(B - b0) : G;
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, wm = wave / 2, wn = wave % 2;

  v16f acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[g][v] = 0.0f;

  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t row0 = tile * BM;
    if (tile_is_empty(rowptr, M, row0)) continue;  // the same in every thread
    uint4 rg[NW];
#pragma unroll
    for (int it = 0; it < NW; ++it) {  // travels while the rows are gathered
      const int word = tid + it * THREADS;
      const int64_t m = row0 + (word / (8 * FQ)) * 8 + word % 8, f = f0 + ((word / 8) % FQ) * VPL;
      rg[it] = load_word<T, VEC>(gr + m * F + f, m < M ? F - f : 0);
    }
    aggregate<T, 1, LDW>(x, comp, scale, rowptr, col, etype, M, row0, K, k0, B, b0, sA);
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
      const uint4 bb = *reinterpret_cast<const uint4*>(sB + (wn * 32 + lane % 32) * LDW + m);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g < gc) {
          const uint4 a = *reinterpret_cast<const uint4*>(sA + g * BM * LDW + (wm * 32 + lane % 32) * LDW + m);
          acc[g] = mfma(a, bb, acc[g], T());
        }
      }
    }
    __syncthreads();
  }

  const int64_t f = f0 + wn * 32 + lane % 32;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g < gc) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t k = k0 + wm * 32 + acc_row(v);
        if (k < K && f < F) {
          if (chunks == 1) grad_basis[((b0 + g) * K + k) * F + f] = narrow<T>(acc[g][v]);
          else partial[(((chunk * B) + b0 + g) * K + k) * F + f] = acc[g][v];
        }
      }
    }
  }
}

// sums the fp32 partials [chunks][n] in chunk order; one thread per element of grad_basis
template <typename T>
__global__ __launch_bounds__(THREADS) void basis_spmm_fold_kernel(const float* __restrict__ partial, int64_t chunks,
                                                                  int64_t n, T* __restrict__ grad_basis) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
  if (e >= n) return;
  float sum = 0.0f;
  for (int64_t c = 0; c < chunks; ++c) sum += partial[c * n + e];
  grad_basis[e] = narrow<T>(sum);
}

// ---- coefficient gradient ---------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(THREADS) void basis_spmm_bw_comp_kernel(
    const T* __restrict__ x, const T* __restrict__ gr, const T* __restrict__ basis, const float* __restrict__ scale,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t M, int64_t K, int64_t F, int64_t B,
    float* s_out) {
  using Ge = Geo<T>;
  constexpr int VPL = Ge::VPL, LD = Ge::LD, LDZ = Ge::LDW;
  constexpr int KV = BK / VPL;                  // words of a row of a tile
  constexpr int NW = 64 * KV / THREADS;         // words of a tile per thread
  __shared__ __attribute__((aligned(16))) T sP[G * BM * LDZ];  // P[g][m][k]
  __shared__ __attribute__((aligned(16))) T sA[2][64 * LD];    // grad_out[m][f step]
  __shared__ __attribute__((aligned(16))) T sV[2][64 * LD];    // V_b[k][f step]
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * BM;
  if (tile_is_empty(rowptr, M, row0)) return;  // the same in every thread
  const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, wm = wave / 2, wn = wave % 2;
  const int r0 = __builtin_amdgcn_readfirstlane(wave) * ROWS;
  const int64_t my_ptr = wave_offsets(rowptr, M, row0);
  const int64_t begin = readlane64(my_ptr, 0), end = readlane64(my_ptr, ROWS);
  const int FS = static_cast<int>((F + BK - 1) / BK);

  for (int64_t b0 = 0; b0 < B; b0 += G) {
    const int gc = B - b0 < G ? static_cast<int>(B - b0) : G;
    for (int64_t k0 = 0; k0 < K; k0 += KB) {
      // P[g] = grad_out[tile rows] @ V_(b0 + g)[k0 .. k0 + KB]^T, both operands copied as they lie in memory
      uint4 ra[NW], rv[NW];
      auto fetch = [&](int g, int64_t f) {
#pragma unroll
        for (int it = 0; it < NW; ++it) {
          const int word = tid + it * THREADS;
          const int64_t r = word / KV, ff = f + (word % KV) * VPL;
          ra[it] = load_word<T, VEC>(gr + (row0 + r) * F + ff, row0 + r < M ? F - ff : 0);
          rv[it] = load_word<T, VEC>(basis + ((b0 + g) * K + k0 + r) * F + ff, k0 + r < K ? F - ff : 0);
        }
      };
      auto stash = [&](int buf) {
#pragma unroll
        for (int it = 0; it < NW; ++it) {
          const int word = tid + it * THREADS;
          *reinterpret_cast<uint4*>(sA[buf] + (word / KV) * LD + (word % KV) * VPL) = ra[it];
          *reinterpret_cast<uint4*>(sV[buf] + (word / KV) * LD + (word % KV) * VPL) = rv[it];
        }
      };
      const int Q = gc * FS;
      fetch(0, 0);
      stash(0);
      __syncthreads();
      v16f acc;
      for (int q = 0; q < Q; ++q) {
        const int buf = q & 1, g = q / FS, st = q % FS;
        if (st == 0) {
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
        }
        if (q + 1 < Q) fetch((q + 1) / FS, static_cast<int64_t>((q + 1) % FS) * BK);
#pragma unroll
        for (int grp = 0; grp < BK / (2 * VPL); ++grp) {
          const int k = grp * 2 * VPL + (lane / 32) * VPL;
          const uint4 a = *reinterpret_cast<const uint4*>(sA[buf] + (wm * 32 + lane % 32) * LD + k);
          const uint4 b = *reinterpret_cast<const uint4*>(sV[buf] + (wn * 32 + lane % 32) * LD + k);
          acc = mfma(a, b, acc, T());
        }
        if (st == FS - 1) {
#pragma unroll
          for (int v = 0; v < 16; ++v)
            sP[g * BM * LDZ + (wm * 32 + acc_row(v)) * LDZ + wn * 32 + lane % 32] = narrow<T>(acc[v]);
        }
        if (q + 1 < Q) stash(buf ^ 1);
        __syncthreads();  // the last one publishes P
      }

      // the entries of this wave's rows: s[e][b0 + g] (+)= scale[e] * <x[col[e]][slab], P[g][row of e]>
      const bool live = k0 + lane < K;
      int cur = 0;
      int64_t end_cur = readlane64(my_ptr, 1);
      for (int64_t b = begin; b < end; b += PASS) {
        const int n = end - b < PASS ? static_cast<int>(end - b) : PASS;
        const int64_t e = b + (lane < n ? lane : n - 1);
        const int my_col = col[e];
        const float my_scale = scale ? scale[e] : 1.0f;
        for (int u = 0; u < n; u += FLY) {
          T v[FLY];
          float s[FLY];
#pragma unroll
          for (int i = 0; i < FLY; ++i) {
            const int src = u + i < n ? u + i : n - 1;  // past the end: the last entry again, not written below
            const T* __restrict__ p = x + static_cast<int64_t>(__builtin_amdgcn_readlane(my_col, src)) * K + k0;
            s[i] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_scale), src));
            v[i] = live ? p[lane] : T(0);
          }
          float dot[FLY * G];
#pragma unroll
          for (int i = 0; i < FLY; ++i) {
            if (u + i < n) {
              while (b + u + i >= end_cur) {  // ends below `end`, so cur stays below ROWS
                ++cur;
                end_cur = readlane64(my_ptr, cur + 1);
              }
            }
            const float xs = s[i] * widen<T>(v[i]);
#pragma unroll
            for (int g = 0; g < G; ++g) dot[i * G + g] = xs * widen<T>(sP[g * BM * LDZ + (r0 + cur) * LDZ + lane]);
          }
          psa::fold_group_dots<64, FLY * G>(dot, lane);  // lane i * G + g ends with the dot of entry i and basis g
          const int i = lane / G, g = lane % G;
          if (lane < FLY * G && u + i < n && b0 + g < B) {
            const int64_t at = (b + u + i) * B + b0 + g;
            s_out[at] = k0 > 0 ? s_out[at] + dot[0] : dot[0];  // this lane wrote the earlier slabs
          }
        }
      }
      __syncthreads();  // P is rewritten by the next slab or group
    }
  }
}

template <typename T>
bool vec_ok(const void* a, const void* b, int64_t K, int64_t F) {
  constexpr int VPL = Geo<T>::VPL;
  return K % VPL == 0 && F % VPL == 0 && psa::aligned(a, 16) && psa::aligned(b, 16);
}

constexpr int64_t kMaxGrid = 0xffffffffLL / THREADS;  // a launch holds fewer than 2^32 threads

template <typename T, int NT>
void launch_fw_nt(bool vec, int trans, dim3 grid, hipStream_t s, const T* x, const T* basis, const float* comp,
                  const float* scale, const int64_t* rowptr, const int32_t* col, const int32_t* etype, int64_t M,
                  int64_t K, int64_t F, int64_t B, int64_t col_tiles, T* out) {
  const dim3 block(THREADS);
#define PSA_BASIS_FW(V, TR)                                                                                          \
  hipLaunchKernelGGL((basis_spmm_kernel<T, NT, V, TR>), grid, block, 0, s, x, basis, comp, scale, rowptr, col, etype, \
                     M, K, F, B, col_tiles, out)
  if (vec && trans) PSA_BASIS_FW(true, true);
  else if (vec) PSA_BASIS_FW(true, false);
  else if (trans) PSA_BASIS_FW(false, true);
  else PSA_BASIS_FW(false, false);
#undef PSA_BASIS_FW
}

template <typename T>
int launch_fw(const void* x, const void* basis, const float* comp, const float* scale, const int64_t* rowptr,
              const int32_t* col, const int32_t* etype, int64_t M, int64_t K, int64_t F, int64_t B, int trans,
              void* out, hipStream_t s) {
  const bool vec = vec_ok<T>(basis, basis, K, F), wide = F > 64;
  const int64_t col_tiles = psa::ceil_div(F, wide ? 128 : 64), tiles = psa::ceil_div(M, BM);
  PSA_REQUIRE(tiles <= kMaxGrid / col_tiles, "the tile grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(tiles * col_tiles));
  if (wide)
    launch_fw_nt<T, 2>(vec, trans, grid, s, static_cast<const T*>(x), static_cast<const T*>(basis), comp, scale, rowptr,
                       col, etype, M, K, F, B, col_tiles, static_cast<T*>(out));
  else
    launch_fw_nt<T, 1>(vec, trans, grid, s, static_cast<const T*>(x), static_cast<const T*>(basis), comp, scale, rowptr,
                       col, etype, M, K, F, B, col_tiles, static_cast<T*>(out));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

template <typename T>
int launch_bw_basis(const void* x, const void* grad, const float* comp, const float* scale, const int64_t* rowptr,
                    const int32_t* col, const int32_t* etype, int64_t M, int64_t K, int64_t F, int64_t B,
                    int64_t chunks, float* partial, void* grad_basis, hipStream_t s) {
  const int64_t k_tiles = psa::ceil_div(K, 64), f_tiles = psa::ceil_div(F, 64), groups = psa::ceil_div(B, G);
  PSA_REQUIRE(k_tiles <= kMaxGrid / f_tiles && groups <= kMaxGrid / (k_tiles * f_tiles) &&
                  chunks <= kMaxGrid / (groups * k_tiles * f_tiles),
              "the tile grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(chunks * groups * k_tiles * f_tiles)), block(THREADS);
  const T* xx = static_cast<const T*>(x);
  const T* gg = static_cast<const T*>(grad);
  T* out = static_cast<T*>(grad_basis);
  const int64_t tiles = psa::ceil_div(M, BM);
  if (F % Geo<T>::VPL == 0 && psa::aligned(grad, 16))
    hipLaunchKernelGGL((basis_spmm_bw_basis_kernel<T, true>), grid, block, 0, s, xx, gg, comp, scale, rowptr, col, etype,
                       M, K, F, B, tiles, chunks, groups, k_tiles, f_tiles, partial, out);
  else
    hipLaunchKernelGGL((basis_spmm_bw_basis_kernel<T, false>), grid, block, 0, s, xx, gg, comp, scale, rowptr, col,
                       etype, M, K, F, B, tiles, chunks, groups, k_tiles, f_tiles, partial, out);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

template <typename T>
int launch_bw_comp(const void* x, const void* grad, const void* basis, const float* scale, const int64_t* rowptr,
                   const int32_t* col, int64_t M, int64_t K, int64_t F, int64_t B, float* s_out, hipStream_t s) {
  const int64_t tiles = psa::ceil_div(M, BM);
  PSA_REQUIRE(tiles <= kMaxGrid, "the tile grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(tiles)), block(THREADS);
  const T* xx = static_cast<const T*>(x);
  const T* gg = static_cast<const T*>(grad);
  const T* vv = static_cast<const T*>(basis);
  if (vec_ok<T>(grad, basis, F, F))
    hipLaunchKernelGGL((basis_spmm_bw_comp_kernel<T, true>), grid, block, 0, s, xx, gg, vv, scale, rowptr, col, M, K, F,
                       B, s_out);
  else
    hipLaunchKernelGGL((basis_spmm_bw_comp_kernel<T, false>), grid, block, 0, s, xx, gg, vv, scale, rowptr, col, M, K, F,
                       B, s_out);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

int psa_basis_spmm_tile(int* bm, int* g, int* kb, int* pass, int* tc) {
  PSA_REQUIRE(bm && g && kb && pass && tc, "NULL pointer");
  *bm = BM;
  *g = G;
  *kb = KB;
  *pass = PASS;
  *tc = TC;
  return PSA_OK;
}

int64_t psa_basis_spmm_bw_chunks(int64_t M) { return M <= 0 ? 1 : psa::ceil_div(psa::ceil_div(M, BM), TC); }

int psa_basis_spmm(int dtype, const void* x, const void* basis, const float* comp, const float* scale,
                   const int64_t* rowptr, const int32_t* col, const int32_t* etype, int64_t M, int64_t N, int64_t nnz,
                   int64_t T, int64_t B, int64_t K, int64_t F, int trans, void* out, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && T >= 0 && B >= 1 && K >= 1 && F >= 1,
              "negative size, or B, K or F below 1");
  if (M == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && out, "NULL required pointer");
  PSA_REQUIRE(nnz == 0 || (x && basis && comp && col && etype && N > 0 && T > 0), "entries without their operands");
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32) return launch_fw<float>(x, basis, comp, scale, rowptr, col, etype, M, K, F, B, trans, out, s);
  return launch_fw<uint16_t>(x, basis, comp, scale, rowptr, col, etype, M, K, F, B, trans, out, s);
}

int psa_basis_spmm_bw_basis(int dtype, const void* x, const void* grad, const float* comp, const float* scale,
                            const int64_t* rowptr, const int32_t* col, const int32_t* etype, int64_t M, int64_t N,
                            int64_t nnz, int64_t T, int64_t B, int64_t K, int64_t F, float* partial,
                            int64_t partial_chunks, void* grad_basis, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && T >= 0 && B >= 1 && K >= 1 && F >= 1,
              "negative size, or B, K or F below 1");
  const int64_t chunks = psa_basis_spmm_bw_chunks(M);
  PSA_REQUIRE(rowptr && grad_basis, "NULL required pointer");
  PSA_REQUIRE(chunks == 1 || (partial && partial_chunks >= chunks), "the partial buffer holds too few chunks");
  PSA_REQUIRE(nnz == 0 || (x && grad && comp && col && etype && N > 0 && T > 0 && M > 0),
              "entries without their operands");
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32)
    return launch_bw_basis<float>(x, grad, comp, scale, rowptr, col, etype, M, K, F, B, chunks, partial, grad_basis, s);
  return launch_bw_basis<uint16_t>(x, grad, comp, scale, rowptr, col, etype, M, K, F, B, chunks, partial, grad_basis, s);
}

int psa_basis_spmm_bw_fold(int dtype, const float* partial, int64_t chunks, int64_t B, int64_t K, int64_t F,
                           void* grad_basis, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(chunks >= 1 && B >= 1 && K >= 1 && F >= 1, "chunks, B, K or F below 1");
  PSA_REQUIRE(partial && grad_basis, "NULL required pointer");
  const int64_t n = B * K * F, blocks = psa::ceil_div(n, THREADS);
  PSA_REQUIRE(blocks <= kMaxGrid, "the grid does not fit one launch");
  const dim3 grid(static_cast<unsigned>(blocks)), block(THREADS);
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32)
    hipLaunchKernelGGL((basis_spmm_fold_kernel<float>), grid, block, 0, s, partial, chunks, n,
                       static_cast<float*>(grad_basis));
  else
    hipLaunchKernelGGL((basis_spmm_fold_kernel<uint16_t>), grid, block, 0, s, partial, chunks, n,
                       static_cast<uint16_t*>(grad_basis));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_basis_spmm_bw_comp(int dtype, const void* x, const void* grad, const void* basis, const float* scale,
                           const int64_t* rowptr, const int32_t* col, int64_t M, int64_t N, int64_t nnz, int64_t B,
                           int64_t K, int64_t F, float* s_out, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && B >= 1 && K >= 1 && F >= 1, "negative size, or B, K or F below 1");
  if (M == 0 || nnz == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && x && grad && basis && col && s_out && N > 0, "NULL required pointer");
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32) return launch_bw_comp<float>(x, grad, basis, scale, rowptr, col, M, K, F, B, s_out, s);
  return launch_bw_comp<uint16_t>(x, grad, basis, scale, rowptr, col, M, K, F, B, s_out, s);
}

}  // extern "C"
