// Multi-head SpMM over fp32 per-head edge values with a two-byte dense operand (bf16), gfx950:
//
//   psa_spmm_heads_half   out[r, h, f] = round(alpha * sum_{e in row r} value[e, h] * mat[col[e], h, f])
//
// value is fp32 [nnz, H], mat and out are bf16 [N, H, F] / [M, H, F], every product and sum is fp32 and the
// result is rounded once (nearest even), after alpha.  It serves the backward of the bf16 fused attention
// (attention_half.hip): grad_q = (dS, k) * scale over the CSR view, grad_k = (dS, q) * scale and
// grad_v = (p, grad_out) over the CSC view, without an fp32 copy of k, q or grad_out.
//
// spmm_heads.hip's plan with half-width gathers: one wave per CSR row, a lane owns VEC consecutive elements
// of the H * F of a row of mat (VEC = 8: one 16-byte gather, when F % 8 == 0 and mat / out start on 16
// bytes; VEC = 1: 2-byte loads otherwise, any 2-byte alignment) and reads value[e, head of those elements];
// P lanes serve an entry, lane group g adds entries g, g + G, ... in that order, the groups fold with xor
// shuffles; up to four tiles of fp32 accumulators.  Rows above psa::kLongRow entries go through the
// long_rows.h list: a chunk wave leaves its fp32 partial row in the workspace and one wave per listed row adds
// the partials in chunk order, applies alpha and rounds.  No float atomics, no host read; no zero skipping.
// Every address is formed in 64-bit arithmetic.
#include "common.h"
#include "half_rows.h"
#include "long_rows.h"

namespace {

using psa_half::BF16;
using psa_half::clamp_range;
using psa_half::elem_t;
using psa_half::load_f32;
using psa_half::load_vec;
using psa_half::pow2_at_least;
using psa_half::store_f32;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChunkBlocks = 4096;
constexpr int kMaxTiles = 4;  // tiles of accumulators kept in registers

// round(alpha * src): the one rounding of a result
template <typename T, int VEC>
__device__ __forceinline__ void store_scaled(elem_t* p, float alpha, float (&src)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) src[i] = __fmul_rn(alpha, src[i]);
  if constexpr (VEC == 8) {
    *reinterpret_cast<uint4*>(p) = psa_half::narrow8<T>(src);
  } else {
    *p = psa_half::narrow1<T>(src[0]);
  }
}

struct SpmmGeo {
  int64_t H, F, D;  // D = H * F
  int P;            // lanes per entry
  int shift;        // log2(P)
};

// The NT tiles from tile0 on of sum_{e in [s, e)} value[e, head] * mat[col[e], :], folded over the
// lane groups: every lane ends with the fp32 sum of the elements it owns.
template <typename T, int VEC, int NT>
__device__ __forceinline__ void spmm_heads_range(const int64_t* __restrict__ col, const float* __restrict__ value,
                                                 const elem_t* __restrict__ mat, const SpmmGeo g, int64_t tile0,
                                                 int64_t s, int64_t e, int lane, float (&acc)[NT][VEC]) {
  constexpr int U = kMaxTiles / NT;  // entries in flight per lane: U * NT gathers
  const int grp = lane >> g.shift;
  const int p = lane & (g.P - 1);
  const int G = 64 >> g.shift;
  int64_t d[NT], hd[NT];
  bool act[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    d[t] = ((tile0 + t) * g.P + p) * VEC;
    act[t] = d[t] < g.D;
    hd[t] = act[t] ? d[t] / g.F : 0;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[t][i] = 0.f;
  }
  for (int64_t base = s; base < e; base += 64) {
    const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
    int64_t c_l = 0;
    if (lane < n) c_l = col[base + lane];
    for (int j = 0; j < n; j += G * U) {
      float b[U][NT][VEC], v[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = j + u * G + grp;
        const bool ok = idx < n;
        const int64_t c = __shfl(static_cast<long long>(c_l), idx & 63);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          v[u][t] = 0.f;
#pragma unroll
          for (int i = 0; i < VEC; ++i) b[u][t][i] = 0.f;
          if (ok && act[t]) {
            v[u][t] = value[(base + idx) * g.H + hd[t]];
            load_vec<T, VEC>(mat + c * g.D + d[t], b[u][t]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[t][i] += v[u][t] * b[u][t][i];
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    if (off >= g.P) {  // wave-uniform
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[t][i] += __shfl_xor(acc[t][i], off);
      }
    }
  }
}

// All tiles of the range [s, e) into dst[0 .. D): the row itself (FINAL: dst is elements, round(alpha * sum))
// or a chunk's partial (dst is floats, the sum as it is).
template <typename T, int VEC, int NT, bool FINAL>
__device__ __forceinline__ void spmm_heads_row(const int64_t* __restrict__ col, const float* __restrict__ value,
                                               const elem_t* __restrict__ mat, const SpmmGeo g, int64_t ntiles,
                                               float alpha, int64_t s, int64_t e, int lane, void* __restrict__ dst) {
  const int grp = lane >> g.shift;
  const int p = lane & (g.P - 1);
  for (int64_t tile0 = 0; tile0 < ntiles; tile0 += NT) {
    float acc[NT][VEC];
    spmm_heads_range<T, VEC, NT>(col, value, mat, g, tile0, s, e, lane, acc);
    if (grp == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int64_t d = ((tile0 + t) * g.P + p) * VEC;
        if (d < g.D) {
          if constexpr (FINAL) store_scaled<T, VEC>(static_cast<elem_t*>(dst) + d, alpha, acc[t]);
          else store_f32<VEC>(static_cast<float*>(dst) + d, acc[t]);
        }
      }
    }
  }
}

template <typename T, int VEC, int NT>
__global__ void __launch_bounds__(kThreads)
spmm_heads_half_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                       const float* __restrict__ value, const elem_t* __restrict__ mat, const SpmmGeo g,
                       int64_t ntiles, float alpha, int64_t M, int64_t nnz, elem_t* __restrict__ out,
                       unsigned long long* __restrict__ long_ctr, psa::LongEntry* __restrict__ long_list) {
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
  spmm_heads_row<T, VEC, NT, true>(col, value, mat, g, ntiles, alpha, s, e, lane, out + row * g.D);
}

// One wave per 128-entry chunk of a listed row: part[c, 0 .. D), fp32.
template <typename T, int VEC, int NT>
__global__ void __launch_bounds__(kThreads)
spmm_heads_half_chunk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                             const float* __restrict__ value, const elem_t* __restrict__ mat, const SpmmGeo g,
                             int64_t ntiles, int64_t nnz, const unsigned long long* __restrict__ long_ctr,
                             const psa::LongEntry* __restrict__ long_list, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ctr = *long_ctr;
  const uint32_t total = static_cast<uint32_t>(ctr & 0xffffffffull);
  const int nrows = static_cast<int>(ctr >> 32);
  const uint32_t num_waves = gridDim.x * kWaves;
  for (uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6); c < total; c += num_waves) {
    const psa::LongEntry ent = psa::find_long_entry(long_list, nrows, c);
    int64_t rs = rowptr[ent.row], re = rowptr[ent.row + 1];
    clamp_range(rs, re, nnz);
    const int64_t s = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
    const int64_t e = s + psa::kLongChunk < re ? s + psa::kLongChunk : re;
    spmm_heads_row<T, VEC, NT, false>(col, value, mat, g, ntiles, 1.f, s, e, lane,
                                      part + static_cast<int64_t>(c) * g.D);
  }
}

// One wave per listed row: its chunks' fp32 partial rows, added in chunk order, then alpha and the rounding.
template <typename T, int VEC>
__global__ void __launch_bounds__(kThreads)
spmm_heads_half_combine_kernel(int64_t D, float alpha, const unsigned long long* __restrict__ long_ctr,
                               const psa::LongEntry* __restrict__ long_list, const float* __restrict__ part,
                               elem_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int nrows = static_cast<int>(*long_ctr >> 32);
  const int num_waves = static_cast<int>(gridDim.x) * kWaves;
  for (int slot = blockIdx.x * kWaves + (threadIdx.x >> 6); slot < nrows; slot += num_waves) {
    const psa::LongEntry ent = long_list[slot];
    for (int64_t d = static_cast<int64_t>(lane) * VEC; d < D; d += 64 * VEC) {
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (uint32_t k = 0; k < ent.num_chunks; ++k) {
        float b[VEC];
        load_f32<VEC>(part + static_cast<int64_t>(ent.first_chunk + k) * D + d, b);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += b[i];
      }
      store_scaled<T, VEC>(out + ent.row * D + d, alpha, acc);
    }
  }
}

// out of a pattern without entries: n zeros (a two-byte buffer need not be 4-byte aligned or sized)
__global__ void __launch_bounds__(kThreads) zero_elems_kernel(elem_t* __restrict__ out, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) out[i] = 0;
}

template <typename T, int VEC, int NT>
int launch_spmm_heads(const int64_t* rowptr, const int64_t* col, const float* value, const elem_t* mat,
                      const SpmmGeo g, int64_t ntiles, float alpha, int64_t M, int64_t nnz, elem_t* out,
                      unsigned long long* ctr, psa::LongEntry* list, float* part, hipStream_t s) {
  const int64_t gx = psa::ceil_div(M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((spmm_heads_half_kernel<T, VEC, NT>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s,
                     rowptr, col, value, mat, g, ntiles, alpha, M, nnz, out, ctr, list);
  if (list) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(nnz), kWaves);
    cb = cb > kMaxChunkBlocks ? kMaxChunkBlocks : cb;
    int64_t rb = psa::ceil_div(psa::max_long_rows(nnz), kWaves);
    rb = rb > kMaxChunkBlocks ? kMaxChunkBlocks : rb;
    hipLaunchKernelGGL((spmm_heads_half_chunk_kernel<T, VEC, NT>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0,
                       s, rowptr, col, value, mat, g, ntiles, nnz, ctr, list, part);
    hipLaunchKernelGGL((spmm_heads_half_combine_kernel<T, VEC>), dim3(static_cast<unsigned>(rb)), dim3(kThreads), 0, s,
                       g.D, alpha, ctr, list, part, out);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" int psa_spmm_heads_half(int dtype, const int64_t* rowptr, const int64_t* col, const float* value,
                                   const void* mat, float alpha, int64_t M, int64_t N, int64_t H, int64_t F,
                                   int64_t nnz, void* out, void* workspace, size_t workspace_bytes,
                                   psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_BF16, "dtype must be PSA_BF16");
  PSA_REQUIRE(M >= 0 && N >= 0 && H >= 0 && F >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(H < (int64_t{1} << 24) && F < (int64_t{1} << 24), "H or F too large");
  const int64_t D = H * F;
  if (M == 0 || D == 0) return PSA_OK;
  PSA_REQUIRE(out != nullptr, "out is NULL");
  PSA_REQUIRE(psa::aligned(mat, 2) && psa::aligned(out, 2), "mat and out must be 2-byte aligned");
  hipStream_t s = psa::as_stream(stream);
  elem_t* o = static_cast<elem_t*>(out);
  if (nnz == 0) {
    const int64_t n = M * D;
    int64_t zb = psa::ceil_div(n, kThreads);
    zb = zb > kMaxChunkBlocks ? kMaxChunkBlocks : zb;
    hipLaunchKernelGGL(zero_elems_kernel, dim3(static_cast<unsigned>(zb)), dim3(kThreads), 0, s, o, n);
    PSA_LAUNCH_CHECK();
    return PSA_OK;
  }
  PSA_REQUIRE(rowptr && col && value && mat, "NULL pointer");
  psa::LongSums w;
  if (nnz > psa::kLongRow) {  // fp32 partials: the workspace of psa_spmm_heads
    w = psa::long_sums_layout(workspace, nnz, D);
    const int rc = psa::begin_long_rows(__func__, workspace, workspace_bytes, w.bytes, w.ctr, s);
    if (rc != PSA_OK) return rc;
  }
  const bool v8 = (F % 8 == 0) && psa::aligned(mat, 16) && psa::aligned(out, 16);
  const int vec = v8 ? 8 : 1;
  SpmmGeo g;
  g.H = H;
  g.F = F;
  g.D = D;
  g.P = pow2_at_least(psa::ceil_div(D, vec), 64, &g.shift);
  const int64_t ntiles = psa::ceil_div(D, static_cast<int64_t>(g.P) * vec);
#define PSA_SPMM_HEADS(VEC, NT)                                                                                     \
  return launch_spmm_heads<BF16, VEC, NT>(rowptr, col, value, static_cast<const elem_t*>(mat), g, ntiles, alpha, M, \
                                          nnz, o, w.ctr, w.list, w.part, s)
  if (v8) {
    if (ntiles == 1) PSA_SPMM_HEADS(8, 1);
    if (ntiles == 2) PSA_SPMM_HEADS(8, 2);
    PSA_SPMM_HEADS(8, 4);
  }
  if (ntiles == 1) PSA_SPMM_HEADS(1, 1);
  if (ntiles == 2) PSA_SPMM_HEADS(1, 2);
  PSA_SPMM_HEADS(1, 4);
#undef PSA_SPMM_HEADS
}
