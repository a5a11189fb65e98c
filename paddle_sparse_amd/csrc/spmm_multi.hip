// Multi-aggregation SpMM forward, fp32, gfx950: several statistics of the SAME neighbourhood
// from ONE gather of the dense operand (PNA's aggregator block, PyG's MultiAggregation).
//
//   m_e = value[e] * mat[col[e], :]   (value NULL: mat[col[e], :]),  n = entries of row r
//   sum = S m   mean = sum / n   min / max as psa_spmm   var = max(S m^2 / n - mean^2, 0)
//   std = sqrt(var + eps)             out[r, a, :] = statistic order[a] of row r
//
// The op is the forward's pure gather (spmm.hip) with more than one accumulator per gathered
// float: the gathered row is in registers when the first statistic is taken, the others cost
// VALU work and A - 1 more output tiles, no second gather.
//   * one wave owns one CSR row and is the only writer of its A * K outputs;
//   * col / value are read once per 64 entries, coalesced, one per lane, and handed to the
//     gather loop by cross-lane moves;
//   * LPR lanes x VEC floats cover a K tile (LPR = the power of two >= K / VEC, 4 <= LPR <= 64,
//     chosen on the host; VEC = 4: 16-byte gathers, K % 4 == 0 and 16-byte aligned operands;
//     VEC = 1 otherwise), G = 64 / LPR entries share a wave instruction and kU = 4 such steps
//     are issued before the first is consumed (4 G gathers in flight per wave); K above one tile
//     of LPR * VEC floats (256 / 64) loops over tiles inside the wave;
//   * WHAT IS KEPT PER LANE IS A COMPILE-TIME SET (ST): S m, S m^2, min, max and the two
//     winners.  sum / mean / var / std share S m and S m^2 and are finished in the epilogue, so
//     ("mean", "std") is one pass and ("mean", "max") carries neither S m^2 nor a min;
//   * lane group g takes entries g, g + G, ... in that order; the groups are folded with xor
//     shuffles over the lane bits above LPR, lowest bit first: a fixed order.  Winners are
//     32-bit offsets local to the range, ties go to the smaller offset, and they are widened
//     to the int64 entry id where they are stored;
//   * rows above psa::kLongRow entries go to the long_rows.h list: one wave per 128-entry
//     chunk leaves {S m, S m^2, min, max} partials and chunk-local winners, one wave per listed
//     row folds them IN CHUNK ORDER (strict comparisons: the first chunk keeps a tie).
// min / max follow psa_spmm: accumulators start at -/+FLT_MAX and only a strictly
// better product replaces them, so a NaN never wins, neither does -inf under max / +inf under
// min, and a row none of whose products wins keeps -/+FLT_MAX with arg = nnz; a row without
// entries is 0 in every statistic.  The bits are psa_spmm's with the exception psa_spmm has itself:
// +0 and -0 compare equal, so where both tie for the extreme the zero that is stored depends on
// how the entries fall on the lane groups and on whether winners are tracked (the fold then takes
// the value of the smaller offset, without winners a group keeps its own).  Telling them apart would
// need the offsets in every instantiation, which is what the sets without winners exist to save.  No float atomics, no host read: the bits repeat from run to
// run and the call can be captured.  Every address is formed in 64-bit arithmetic; a row that
// stays on one wave (no workspace given) must have fewer than 2^31 entries.
#include "common.h"
#include "long_rows.h"
#include "vec_io.h"

namespace {

using psa::load_vec;
using psa::shfl_i64;
using psa::store_vec_nt;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kU = 4;                  // steps of G entries in flight
constexpr int kMinLanes = 4;           // LPR >= 4: G * kU <= 64, an entry batch divides the wave
constexpr int kChunkBlocks = 2048;     // capped grid of the chunk / combine launches: 8192 waves
constexpr int kNumStats = 6;

// accumulator set (template parameter ST)
enum { A_SUM = 1, A_SQ = 2, A_MIN = 4, A_MAX = 8, A_ARG = 16 };

template <int VEC>
struct Acc {  // members outside the set ST are never touched and cost nothing
  float sm[VEC], sq[VEC], mn[VEC], mx[VEC];
  int32_t amn[VEC], amx[VEC];
};

constexpr int num_float_parts(int st) {
  return ((st & A_SUM) ? 1 : 0) + ((st & A_SQ) ? 1 : 0) + ((st & A_MIN) ? 1 : 0) + ((st & A_MAX) ? 1 : 0);
}
constexpr int num_arg_parts(int st) {
  return (st & A_ARG) ? ((st & A_MIN) ? 1 : 0) + ((st & A_MAX) ? 1 : 0) : 0;
}

struct Geo {
  int64_t K;
  int64_t ntiles;  // tiles of (1 << shift) * VEC floats over K
  int shift;       // log2(LPR)
};

// where statistic `code` goes in a row of out (-1: not wanted), and what the epilogue needs
struct Slots {
  int at[kNumStats];
  int A;
  float eps;
};

template <int VEC, int ST>
__device__ __forceinline__ void acc_init(Acc<VEC>& a) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if constexpr (ST & A_SUM) a.sm[i] = 0.f;
    if constexpr (ST & A_SQ) a.sq[i] = 0.f;
    if constexpr (ST & A_MIN) a.mn[i] = __FLT_MAX__;
    if constexpr (ST & A_MAX) a.mx[i] = -__FLT_MAX__;
    if constexpr ((ST & A_ARG) && (ST & A_MIN)) a.amn[i] = INT32_MAX;
    if constexpr ((ST & A_ARG) && (ST & A_MAX)) a.amx[i] = INT32_MAX;
  }
}

// `o` (with winners oa) joins `a`: a strictly better value, or an equal one from an earlier entry
template <bool IS_MAX, bool ARG>
__device__ __forceinline__ void join_extreme(float& v, int32_t& la, float o, int32_t oa) {
  const bool better = IS_MAX ? (o > v) : (o < v);
  if constexpr (ARG) {
    if (better || (o == v && oa < la)) {
      v = o;
      la = oa;
    }
  } else {
    if (better) v = o;
  }
}

// The statistics kept in ST over the entries [s, e) of one row, for the K tile whose floats of
// this lane start at matk[c * K]; winners are offsets from s (INT32_MAX: none).  Every lane ends
// with the folded result of the floats it owns.
template <int VEC, int ST>
__device__ __forceinline__ void multi_range(const int64_t* __restrict__ col, const float* __restrict__ val,
                                            const float* __restrict__ matk, int64_t K, bool kact, int64_t s,
                                            int64_t e, int lane, int shift, Acc<VEC>& a) {
  constexpr bool ARG = (ST & A_ARG) != 0;
  const int G = 64 >> shift;
  const int grp = lane >> shift;
  acc_init<VEC, ST>(a);
  for (int64_t base = s; base < e; base += 64) {
    const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
    int64_t c_l = 0;
    float v_l = 0.f;
    if (lane < n) {
      c_l = col[base + lane];
      v_l = val ? val[base + lane] : 1.f;
    }
    for (int j = 0; j < n; j += G * kU) {  // G * kU divides 64: idx below stays under 64
      float b[kU][VEC];
      float w[kU];
      bool ok[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int idx = j + u * G + grp;
        const int64_t c = shfl_i64(c_l, idx);
        w[u] = __shfl(v_l, idx);
        ok[u] = (idx < n) && kact;
#pragma unroll
        for (int i = 0; i < VEC; ++i) b[u][i] = 0.f;
        if (ok[u]) load_vec<VEC>(matk + c * K, b[u]);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (ok[u]) {
          const int32_t eid = static_cast<int32_t>(base - s) + j + u * G + grp;
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float x = w[u] * b[u][i];
            if constexpr (ST & A_SUM) a.sm[i] += x;
            if constexpr (ST & A_SQ) a.sq[i] = fmaf(x, x, a.sq[i]);
            if constexpr (ST & A_MIN) {
              if (x < a.mn[i]) {
                a.mn[i] = x;
                if constexpr (ARG) a.amn[i] = eid;
              }
            }
            if constexpr (ST & A_MAX) {
              if (x > a.mx[i]) {
                a.mx[i] = x;
                if constexpr (ARG) a.amx[i] = eid;
              }
            }
          }
        }
      }
    }
  }
  // fold the G lane groups, lowest lane bit above LPR first
  for (int off = 1 << shift; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if constexpr (ST & A_SUM) a.sm[i] += __shfl_xor(a.sm[i], off);
      if constexpr (ST & A_SQ) a.sq[i] += __shfl_xor(a.sq[i], off);
      if constexpr (ST & A_MIN) {
        const float o = __shfl_xor(a.mn[i], off);
        int32_t oa = 0;
        if constexpr (ARG) oa = __shfl_xor(a.amn[i], off);
        join_extreme<false, ARG>(a.mn[i], a.amn[i], o, oa);
      }
      if constexpr (ST & A_MAX) {
        const float o = __shfl_xor(a.mx[i], off);
        int32_t oa = 0;
        if constexpr (ARG) oa = __shfl_xor(a.amx[i], off);
        join_extreme<true, ARG>(a.mx[i], a.amx[i], o, oa);
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_ids_nt(int64_t* p, const int64_t (&src)[VEC]) {
  if constexpr (VEC == 4) {  // two 16-byte stores: the rows of an int64 [M, K] array are 16-byte aligned only
    const int64_t lo[2] = {src[0], src[1]}, hi[2] = {src[2], src[3]};
    psa::store_arg_nt<2>(p, lo);
    psa::store_arg_nt<2>(p + 2, hi);
  } else {
    psa::store_arg_nt<VEC>(p, src);
  }
}

// Epilogue: the wanted statistics of VEC columns from their finished accumulators.  orow = the
// row's first output tile at this lane's column (out + r * A * K + k0); first = global id of the
// entry the winners count from; arg_min / arg_max / mean_out at (r, k0) or NULL.
template <int VEC, int ST>
__device__ __forceinline__ void emit(const Acc<VEC>& a, int64_t deg, int64_t first, int64_t nnz, const Slots& sl,
                                     int64_t K, float* __restrict__ orow, int64_t* __restrict__ arg_min,
                                     int64_t* __restrict__ arg_max, float* __restrict__ mean_out) {
  const float d = static_cast<float>(deg);
  float r[VEC];
  if constexpr (ST & A_SUM) {
    float mean[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) mean[i] = deg > 0 ? a.sm[i] / d : 0.f;
    if (sl.at[0] >= 0) store_vec_nt<VEC>(orow + sl.at[0] * K, a.sm);
    if (sl.at[1] >= 0) store_vec_nt<VEC>(orow + sl.at[1] * K, mean);
    if (mean_out) store_vec_nt<VEC>(mean_out, mean);  // the backward's copy of a mean that is no statistic of the call
    if constexpr (ST & A_SQ) {
      float var[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float v = deg > 0 ? a.sq[i] / d - mean[i] * mean[i] : 0.f;
        var[i] = v < 0.f ? 0.f : v;  // a NaN stays
      }
      if (sl.at[4] >= 0) store_vec_nt<VEC>(orow + sl.at[4] * K, var);
      if (sl.at[5] >= 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) r[i] = deg > 0 ? sqrtf(var[i] + sl.eps) : 0.f;
        store_vec_nt<VEC>(orow + sl.at[5] * K, r);
      }
    }
  }
  if constexpr (ST & A_MIN) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[i] = deg > 0 ? a.mn[i] : 0.f;
    store_vec_nt<VEC>(orow + sl.at[2] * K, r);
    if constexpr (ST & A_ARG) {
      if (arg_min) {
        int64_t id[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) id[i] = a.amn[i] == INT32_MAX ? nnz : first + a.amn[i];
        store_ids_nt<VEC>(arg_min, id);
      }
    }
  }
  if constexpr (ST & A_MAX) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) r[i] = deg > 0 ? a.mx[i] : 0.f;
    store_vec_nt<VEC>(orow + sl.at[3] * K, r);
    if constexpr (ST & A_ARG) {
      if (arg_max) {
        int64_t id[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) id[i] = a.amx[i] == INT32_MAX ? nnz : first + a.amx[i];
        store_ids_nt<VEC>(arg_max, id);
      }
    }
  }
}

// VEC elements of one partial row; returns the place of the next statistic's row
template <int VEC, typename T>
__device__ __forceinline__ T* put_part(T* p, const T (&src)[VEC], int64_t K) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) p[i] = src[i];
  return p + K;
}

__device__ __forceinline__ void clamp_range(int64_t& s, int64_t& e, int64_t nnz) {
  s = s < 0 ? 0 : (s > nnz ? nnz : s);
  e = e < s ? s : (e > nnz ? nnz : e);
}

// One wave per CSR row, every K tile of it.
template <int VEC, int ST>
__global__ void __launch_bounds__(kThreads)
spmm_multi_row_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                      const float* __restrict__ val, const float* __restrict__ mat, const Geo g, const Slots sl,
                      int64_t M, int64_t nnz, float* __restrict__ out, int64_t* __restrict__ arg_min,
                      int64_t* __restrict__ arg_max, float* __restrict__ mean_out,
                      unsigned long long* __restrict__ long_ctr,
                      psa::LongEntry* __restrict__ long_list) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (row >= M) return;
  int64_t s = rowptr[row], e = rowptr[row + 1];
  clamp_range(s, e, nnz);
  if (long_list && e - s > psa::kLongRow) {  // wave-uniform: hand the row to chunk waves
    if (lane == 0) psa::push_long_row(long_ctr, long_list, row, e - s);
    return;
  }
  const int l = lane & ((1 << g.shift) - 1);
  for (int64_t t = 0; t < g.ntiles; ++t) {
    const int64_t k0 = ((t << g.shift) + l) * VEC;
    const bool kact = k0 < g.K;
    Acc<VEC> a;
    multi_range<VEC, ST>(col, val, mat + k0, g.K, kact, s, e, lane, g.shift, a);
    if ((lane >> g.shift) == 0 && kact)
      emit<VEC, ST>(a, e - s, s, nnz, sl, g.K, out + row * sl.A * g.K + k0, arg_min ? arg_min + row * g.K + k0 : nullptr,
                    arg_max ? arg_max + row * g.K + k0 : nullptr, mean_out ? mean_out + row * g.K + k0 : nullptr);
  }
}

// One wave per 128-entry chunk of a listed row: part_f[c, f, :] for the float statistics of ST in
// the order {S m, S m^2, min, max}, part_a[c, q, :] for the chunk-local winners {min, max}.
template <int VEC, int ST>
__global__ void __launch_bounds__(kThreads)
spmm_multi_chunk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                        const float* __restrict__ val, const float* __restrict__ mat, const Geo g, int64_t nnz,
                        const unsigned long long* __restrict__ long_ctr,
                        const psa::LongEntry* __restrict__ long_list, float* __restrict__ part_f,
                        int32_t* __restrict__ part_a) {
  constexpr int NF = num_float_parts(ST), NA = num_arg_parts(ST);
  const int lane = threadIdx.x & 63;
  const unsigned long long ctr = *long_ctr;
  const uint32_t total = static_cast<uint32_t>(ctr & 0xffffffffull);
  const int nrows = static_cast<int>(ctr >> 32);
  const uint32_t num_waves = gridDim.x * kWaves;
  const int l = lane & ((1 << g.shift) - 1);
  for (uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6); c < total; c += num_waves) {
    const psa::LongEntry ent = psa::find_long_entry(long_list, nrows, c);
    int64_t rs = rowptr[ent.row], re = rowptr[ent.row + 1];
    clamp_range(rs, re, nnz);
    const int64_t s = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
    const int64_t e = s + psa::kLongChunk < re ? s + psa::kLongChunk : re;
    for (int64_t t = 0; t < g.ntiles; ++t) {
      const int64_t k0 = ((t << g.shift) + l) * VEC;
      const bool kact = k0 < g.K;
      Acc<VEC> a;
      multi_range<VEC, ST>(col, val, mat + k0, g.K, kact, s, e, lane, g.shift, a);
      if ((lane >> g.shift) == 0 && kact) {
        float* pf = part_f + static_cast<int64_t>(c) * NF * g.K + k0;
        if constexpr (ST & A_SUM) pf = put_part<VEC>(pf, a.sm, g.K);
        if constexpr (ST & A_SQ) pf = put_part<VEC>(pf, a.sq, g.K);
        if constexpr (ST & A_MIN) pf = put_part<VEC>(pf, a.mn, g.K);
        if constexpr (ST & A_MAX) pf = put_part<VEC>(pf, a.mx, g.K);
        if constexpr (NA > 0) {
          int32_t* pa = part_a + static_cast<int64_t>(c) * NA * g.K + k0;
          if constexpr (ST & A_MIN) pa = put_part<VEC>(pa, a.amn, g.K);
          if constexpr (ST & A_MAX) pa = put_part<VEC>(pa, a.amx, g.K);
        }
      }
    }
  }
}

// One wave per listed row, a lane per column: the chunks' partials folded in chunk order (sums
// added, extremes replaced by a strictly better chunk only, so the first chunk keeps a tie and
// its winner), then the same epilogue as a short row.
template <int ST>
__global__ void __launch_bounds__(kThreads)
spmm_multi_combine_kernel(const int64_t* __restrict__ rowptr, int64_t K, int64_t nnz, const Slots sl,
                          const unsigned long long* __restrict__ long_ctr,
                          const psa::LongEntry* __restrict__ long_list, const float* __restrict__ part_f,
                          const int32_t* __restrict__ part_a, float* __restrict__ out,
                          int64_t* __restrict__ arg_min, int64_t* __restrict__ arg_max,
                          float* __restrict__ mean_out) {
  constexpr int NF = num_float_parts(ST), NA = num_arg_parts(ST);
  constexpr bool ARG = (ST & A_ARG) != 0;
  const int lane = threadIdx.x & 63;
  const int nrows = static_cast<int>(*long_ctr >> 32);
  const int num_waves = static_cast<int>(gridDim.x) * kWaves;
  for (int slot = blockIdx.x * kWaves + (threadIdx.x >> 6); slot < nrows; slot += num_waves) {
    const psa::LongEntry ent = long_list[slot];
    int64_t rs = rowptr[ent.row], re = rowptr[ent.row + 1];
    clamp_range(rs, re, nnz);
    for (int64_t k = lane; k < K; k += 64) {
      Acc<1> a;
      acc_init<1, ST>(a);
      for (uint32_t ch = 0; ch < ent.num_chunks; ++ch) {
        const int64_t c = static_cast<int64_t>(ent.first_chunk) + ch;
        const float* pf = part_f + c * NF * K + k;
        [[maybe_unused]] const int32_t* pa = part_a + c * NA * K + k;
        [[maybe_unused]] const int32_t lift = static_cast<int32_t>(ch) * psa::kLongChunk;  // chunk-local -> row-local
        if constexpr (ST & A_SUM) {
          a.sm[0] += *pf;
          pf += K;
        }
        if constexpr (ST & A_SQ) {
          a.sq[0] += *pf;
          pf += K;
        }
        if constexpr (ST & A_MIN) {
          if (*pf < a.mn[0]) {  // a strictly better chunk has a winner
            a.mn[0] = *pf;
            if constexpr (ARG) a.amn[0] = *pa + lift;
          }
          pf += K;
          if constexpr (ARG) pa += K;
        }
        if constexpr (ST & A_MAX) {
          if (*pf > a.mx[0]) {
            a.mx[0] = *pf;
            if constexpr (ARG) a.amx[0] = *pa + lift;
          }
        }
      }
      emit<1, ST>(a, re - rs, rs, nnz, sl, K, out + ent.row * sl.A * K + k, arg_min ? arg_min + ent.row * K + k : nullptr,
                  arg_max ? arg_max + ent.row * K + k : nullptr, mean_out ? mean_out + ent.row * K + k : nullptr);
    }
  }
}

// The workspace is long_rows.h's {list, 4-byte partials [chunks, D]} with D = (NF + NA) * K: the float partials
// [chunks, NF, K] in front, the int32 winners [chunks, NA, K] behind them.  Its size is therefore
// psa_spmm_heads_workspace_bytes(nnz, NF + NA, K); no size function of its own.
struct MultiScratch : psa::LongList {
  float* part_f = nullptr;
  int32_t* part_a = nullptr;
  size_t bytes = 0;
};

MultiScratch multi_layout(void* workspace, int st, int64_t K, int64_t nnz) {
  const psa::LongSums sums = psa::long_sums_layout(workspace, nnz, (num_float_parts(st) + num_arg_parts(st)) * K);
  MultiScratch w;
  w.ctr = sums.ctr;
  w.list = sums.list;
  w.part_f = sums.part;
  w.part_a = reinterpret_cast<int32_t*>(sums.part + psa::max_long_chunks(nnz) * num_float_parts(st) * K);
  w.bytes = sums.bytes;
  return w;
}

struct Call {
  const int64_t* rowptr;
  const int64_t* col;
  const float* value;
  const float* mat;
  Geo g;
  Slots sl;
  int64_t M, nnz;
  float* out;
  int64_t* arg_min;
  int64_t* arg_max;
  float* mean_out;
  MultiScratch w;
  hipStream_t s;
};

template <int VEC, int ST>
int launch_multi(const Call& a) {
  const int64_t gx = psa::ceil_div(a.M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((spmm_multi_row_kernel<VEC, ST>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, a.s, a.rowptr,
                     a.col, a.value, a.mat, a.g, a.sl, a.M, a.nnz, a.out, a.arg_min, a.arg_max, a.mean_out, a.w.ctr, a.w.list);
  if (a.w.list) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(a.nnz), kWaves);
    cb = cb > kChunkBlocks ? kChunkBlocks : cb;
    int64_t rb = psa::ceil_div(psa::max_long_rows(a.nnz), kWaves);
    rb = rb > kChunkBlocks ? kChunkBlocks : rb;
    hipLaunchKernelGGL((spmm_multi_chunk_kernel<VEC, ST>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, a.s,
                       a.rowptr, a.col, a.value, a.mat, a.g, a.nnz, a.w.ctr, a.w.list, a.w.part_f, a.w.part_a);
    hipLaunchKernelGGL((spmm_multi_combine_kernel<ST>), dim3(static_cast<unsigned>(rb)), dim3(kThreads), 0, a.s, a.rowptr,
                       a.g.K, a.nnz, a.sl, a.w.ctr, a.w.list, a.w.part_f, a.w.part_a, a.out, a.arg_min, a.arg_max,
                       a.mean_out);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

// The 20 accumulator sets: {-, S m, S m + S m^2} x {-, min, max, min + max}, the empty one
// left out, and every set with an extreme once more with its winners.
template <int VEC>
int launch_set(int st, const Call& a) {
  switch (st) {
#define PSA_MULTI_SET(ST) \
  case ST:                \
    return launch_multi<VEC, ST>(a)
    PSA_MULTI_SET(1);
    PSA_MULTI_SET(3);
    PSA_MULTI_SET(4);
    PSA_MULTI_SET(5);
    PSA_MULTI_SET(7);
    PSA_MULTI_SET(8);
    PSA_MULTI_SET(9);
    PSA_MULTI_SET(11);
    PSA_MULTI_SET(12);
    PSA_MULTI_SET(13);
    PSA_MULTI_SET(15);
    PSA_MULTI_SET(16 + 4);
    PSA_MULTI_SET(16 + 5);
    PSA_MULTI_SET(16 + 7);
    PSA_MULTI_SET(16 + 8);
    PSA_MULTI_SET(16 + 9);
    PSA_MULTI_SET(16 + 11);
    PSA_MULTI_SET(16 + 12);
    PSA_MULTI_SET(16 + 13);
    PSA_MULTI_SET(16 + 15);
#undef PSA_MULTI_SET
  }
  psa::set_error("psa_spmm_multi: no kernel for this set of statistics");
  return PSA_ERR_INVALID_ARG;
}

constexpr int kAllStats = (1 << kNumStats) - 1;

// bit set of statistic codes (+ winners wanted) -> accumulator set
int accumulator_set(int stats, bool want_arg) {
  int st = 0;
  if (stats & ((1 << PSA_SUM) | (1 << PSA_MEAN) | (1 << PSA_VAR) | (1 << PSA_STD))) st |= A_SUM;
  if (stats & ((1 << PSA_VAR) | (1 << PSA_STD))) st |= A_SUM | A_SQ;
  if (stats & (1 << PSA_MIN)) st |= A_MIN;
  if (stats & (1 << PSA_MAX)) st |= A_MAX;
  if (want_arg && (st & (A_MIN | A_MAX))) st |= A_ARG;
  return st;
}

}  // namespace

extern "C" {

int psa_spmm_multi(const int64_t* rowptr, const int64_t* col, const float* value, const float* mat, int64_t M,
                   int64_t N, int64_t K, int64_t nnz, int stats, float eps, const int* order, int64_t A, float* out,
                   int64_t* arg_min, int64_t* arg_max, float* mean_out, void* workspace, size_t workspace_bytes,
                   psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && N >= 0 && K >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(K < (int64_t{1} << 24), "K too large");
  PSA_REQUIRE(A >= 1 && A <= kNumStats && order != nullptr, "order must name 1 to 6 statistics");
  PSA_REQUIRE(stats > 0 && stats <= kAllStats, "bad statistics bit set");
  PSA_REQUIRE(eps >= 0.f, "eps must be >= 0");  // refuses a NaN too
  Slots sl;
  for (int c = 0; c < kNumStats; ++c) sl.at[c] = -1;
  int seen = 0;
  for (int64_t a = 0; a < A; ++a) {
    const int c = order[a];
    PSA_REQUIRE(c >= 0 && c < kNumStats, "unknown statistic code");
    PSA_REQUIRE(!(seen & (1 << c)), "a statistic is named twice");
    seen |= 1 << c;
    sl.at[c] = static_cast<int>(a);
  }
  PSA_REQUIRE(seen == stats, "order and the statistics bit set disagree");
  PSA_REQUIRE(arg_min == nullptr || (stats & (1 << PSA_MIN)), "arg_min without min");
  PSA_REQUIRE(arg_max == nullptr || (stats & (1 << PSA_MAX)), "arg_max without max");
  PSA_REQUIRE(mean_out == nullptr || (stats & ~((1 << PSA_MIN) | (1 << PSA_MAX))), "mean_out without sum, mean, var or std");
  sl.A = static_cast<int>(A);
  sl.eps = eps;
  if (M == 0 || K == 0) return PSA_OK;
  PSA_REQUIRE(rowptr != nullptr, "rowptr is NULL");
  PSA_REQUIRE(out != nullptr, "out is NULL");
  hipStream_t s = psa::as_stream(stream);
  if (nnz == 0) {  // every row is empty: 0 in every statistic, "no winner" = nnz = 0
    const size_t mk = static_cast<size_t>(M) * static_cast<size_t>(K);
    PSA_ZERO(out, sizeof(float) * mk * static_cast<size_t>(A), s);
    if (arg_min) PSA_ZERO(arg_min, sizeof(int64_t) * mk, s);
    if (arg_max) PSA_ZERO(arg_max, sizeof(int64_t) * mk, s);
    if (mean_out) PSA_ZERO(mean_out, sizeof(float) * mk, s);
    return PSA_OK;
  }
  PSA_REQUIRE(col != nullptr && mat != nullptr, "col/mat is NULL");
  const int st = accumulator_set(stats, arg_min != nullptr || arg_max != nullptr);
  Call a{rowptr, col, value, mat, Geo{}, sl, M, nnz, out, arg_min, arg_max, mean_out, MultiScratch{}, s};
  // Long-row path: on when the caller brings a workspace (NULL keeps every row on its own wave:
  // same semantics, slow on power-law graphs; a caller that knows its longest row skips it).
  if (workspace != nullptr && nnz > psa::kLongRow) {
    a.w = multi_layout(workspace, st, K, nnz);
    const int rc = psa::begin_long_rows(__func__, workspace, workspace_bytes, a.w.bytes, a.w.ctr, s);
    if (rc != PSA_OK) return rc;
    PSA_REQUIRE(psa::max_long_chunks(nnz) < (1ll << 32), "too many chunks");
  }
  const bool v4 = (K % 4 == 0) && psa::aligned(mat, 16) && psa::aligned(out, 16) &&
                  (arg_min == nullptr || psa::aligned(arg_min, 16)) && (arg_max == nullptr || psa::aligned(arg_max, 16)) &&
                  (mean_out == nullptr || psa::aligned(mean_out, 16));
  const int vec = v4 ? 4 : 1;
  const int64_t q = psa::ceil_div(K, vec);
  int shift = 2;  // kMinLanes
  while ((1 << shift) < 64 && (int64_t{1} << shift) < q) ++shift;
  static_assert((1 << 2) == kMinLanes, "shift starts at log2(kMinLanes)");
  a.g.K = K;
  a.g.shift = shift;
  a.g.ntiles = psa::ceil_div(q, int64_t{1} << shift);
  return v4 ? launch_set<4>(st, a) : launch_set<1>(st, a);
}

}  // extern "C"
