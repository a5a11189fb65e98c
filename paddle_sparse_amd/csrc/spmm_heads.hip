// Multi-head SpMM over per-head edge values and multi-head sddmm, fp32, gfx950: the two
// ends of a multi-head attention step (softmax.hip is its middle).
//
//   psa_spmm_heads    out[r, h, f] = sum_{e in row r} value[e, h] * mat[col[e], h, f]
//   psa_sddmm_heads   out[e, h]    = <x[row(e), h, :], y[col[e], h, :]>
//
// Both are gather kernels with one wave per CSR row; rows above psa::kLongRow entries are
// handed to chunk waves through the long_rows.h list (one wave per 128-entry chunk).
//
// psa_spmm_heads.  The H * F floats of a row of mat are contiguous, so a lane owns VEC
// consecutive floats of them (VEC = 4: one 16-byte gather, when F % 4 == 0 and mat / out are
// 16-byte aligned, so that the four floats share a head; VEC = 1 otherwise) and reads
// value[e, head of those floats].  P = the power of two >= min(H * F / VEC, 64) lanes serve
// one entry and the wave takes G = 64 / P entries per step (P is chosen on the host); a row
// wider than one tile of 64 * VEC floats keeps up to four tiles of accumulators and loops
// over the rest.  Lane group g adds entries g, g + G, ... of its range in that order, then
// the groups fold with xor shuffles over the lane bits above P: a fixed order.  A chunk wave
// leaves its partial row in the workspace and one wave per listed row adds the partials in
// chunk order, whatever order the list was built in.  No float atomics, no host read: the
// bits repeat from run to run and the call can be captured.  No zero skipping: a stored 0
// against an inf is NaN.
//
// psa_sddmm_heads.  psa_spmm_value_bw's plan with the dot segmented per head: PK = the
// power of two >= min(K / VEC, 64) lanes share a head (K wider than PK * VEC loops), PH
// heads sit side by side in the wave (H above PH loops) and G = 64 / (PH * PK) entries are
// taken per step.  The slices of the row of x that a lane meets stay in registers (up to
// four of them; wider rows re-read x through the caches).  Per head every lane adds its k
// steps in order, then the PK lanes fold with xor shuffles: a fixed order.  Chunk waves write
// disjoint entries, so long rows need no combine.
//
// Every address is formed in 64-bit arithmetic: no bound on N * H * F * 4.
#include "common.h"
#include "half_rows.h"
#include "long_rows.h"

namespace {

using psa_half::clamp_range;
using psa_half::pow2_at_least;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChunkBlocks = 4096;
constexpr int kMaxTiles = 4;  // tiles of accumulators (spmm) / slices of x (sddmm) kept in registers

template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, float (&dst)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
    dst[3] = v.w;
  } else {
    dst[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* p, const float (&src)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(src[0], src[1], src[2], src[3]);
  } else {
    *p = src[0];
  }
}

// ---- SpMM over per-head values ------------------------------------------------------------------

struct SpmmGeo {
  int64_t H, F, D;  // D = H * F
  int P;            // lanes per entry
  int shift;        // log2(P)
};

// The NT tiles from tile0 on of sum_{e in [s, e)} value[e, head] * mat[col[e], :], folded over the
// lane groups: every lane ends with the sum of the floats it owns.
template <int VEC, int NT>
__device__ __forceinline__ void spmm_heads_range(const int64_t* __restrict__ col, const float* __restrict__ value,
                                                 const float* __restrict__ mat, const SpmmGeo g, int64_t tile0,
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
            load_vec<VEC>(mat + c * g.D + d[t], b[u][t]);
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

// All tiles of the range [s, e) into dst[0 .. D).
template <int VEC, int NT>
__device__ __forceinline__ void spmm_heads_row(const int64_t* __restrict__ col, const float* __restrict__ value,
                                               const float* __restrict__ mat, const SpmmGeo g, int64_t ntiles,
                                               int64_t s, int64_t e, int lane, float* __restrict__ dst) {
  const int grp = lane >> g.shift;
  const int p = lane & (g.P - 1);
  for (int64_t tile0 = 0; tile0 < ntiles; tile0 += NT) {
    float acc[NT][VEC];
    spmm_heads_range<VEC, NT>(col, value, mat, g, tile0, s, e, lane, acc);
    if (grp == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int64_t d = ((tile0 + t) * g.P + p) * VEC;
        if (d < g.D) store_vec<VEC>(dst + d, acc[t]);
      }
    }
  }
}

template <int VEC, int NT>
__global__ void __launch_bounds__(kThreads)
spmm_heads_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                  const float* __restrict__ value, const float* __restrict__ mat, const SpmmGeo g, int64_t ntiles,
                  int64_t M, int64_t nnz, float* __restrict__ out, unsigned long long* __restrict__ long_ctr,
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
  spmm_heads_row<VEC, NT>(col, value, mat, g, ntiles, s, e, lane, out + row * g.D);
}

// One wave per 128-entry chunk of a listed row: part[c, 0 .. D).
template <int VEC, int NT>
__global__ void __launch_bounds__(kThreads)
spmm_heads_chunk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                        const float* __restrict__ value, const float* __restrict__ mat, const SpmmGeo g,
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
    spmm_heads_row<VEC, NT>(col, value, mat, g, ntiles, s, e, lane, part + static_cast<int64_t>(c) * g.D);
  }
}

// One wave per listed row: its chunks' partial rows, added in chunk order.
template <int VEC>
__global__ void __launch_bounds__(kThreads)
spmm_heads_combine_kernel(int64_t D, const unsigned long long* __restrict__ long_ctr,
                          const psa::LongEntry* __restrict__ long_list, const float* __restrict__ part,
                          float* __restrict__ out) {
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
        load_vec<VEC>(part + static_cast<int64_t>(ent.first_chunk + k) * D + d, b);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += b[i];
      }
      store_vec<VEC>(out + ent.row * D + d, acc);
    }
  }
}

template <int VEC, int NT>
int launch_spmm_heads(const int64_t* rowptr, const int64_t* col, const float* value, const float* mat,
                      const SpmmGeo g, int64_t ntiles, int64_t M, int64_t nnz, float* out, unsigned long long* ctr,
                      psa::LongEntry* list, float* part, hipStream_t s) {
  const int64_t gx = psa::ceil_div(M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((spmm_heads_kernel<VEC, NT>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s, rowptr,
                     col, value, mat, g, ntiles, M, nnz, out, ctr, list);
  if (list) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(nnz), kWaves);
    cb = cb > kMaxChunkBlocks ? kMaxChunkBlocks : cb;
    int64_t rb = psa::ceil_div(psa::max_long_rows(nnz), kWaves);
    rb = rb > kMaxChunkBlocks ? kMaxChunkBlocks : rb;
    hipLaunchKernelGGL((spmm_heads_chunk_kernel<VEC, NT>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, s,
                       rowptr, col, value, mat, g, ntiles, nnz, ctr, list, part);
    hipLaunchKernelGGL((spmm_heads_combine_kernel<VEC>), dim3(static_cast<unsigned>(rb)), dim3(kThreads), 0, s, g.D,
                       ctr, list, part, out);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

// ---- sddmm per head -----------------------------------------------------------------------------

struct SddmmGeo {
  int64_t H, K, D;  // D = H * K
  int PK, kshift;   // lanes per head
  int PH, hshift;   // heads side by side
  int kiters;       // steps of PK * VEC floats over K
  int nit;          // head passes * kiters: slices of the row of x that a lane meets
};

struct Slice {
  int64_t h;    // head of the slice
  int64_t off;  // h * K + k: first float of it in a row
  bool act;     // the lane has floats in it
  bool last;    // the head's dot is complete after it
};

template <int VEC>
__device__ __forceinline__ Slice slice_of(const SddmmGeo g, int it, int hs, int jl) {
  const int hp = it / g.kiters;
  const int ki = it - hp * g.kiters;
  const int64_t k = (static_cast<int64_t>(ki) * g.PK + jl) * VEC;
  Slice sl;
  sl.h = static_cast<int64_t>(hp) * g.PH + hs;
  sl.act = sl.h < g.H && k < g.K;
  sl.off = sl.h * g.K + k;
  sl.last = ki == g.kiters - 1;
  return sl;
}

__device__ __forceinline__ float fold_head(float dot, int PK) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    if (off < PK) dot += __shfl_xor(dot, off);  // wave-uniform
  }
  return dot;
}

// out[e, :] for the entries [s, e) of ONE row (xrow = that row of x).  NR > 0: the row's nit <= NR
// slices stay in registers; NR == 0: any nit, x re-read through the caches.
template <int VEC, int NR>
__device__ __forceinline__ void sddmm_heads_range(const int64_t* __restrict__ col, const float* __restrict__ y,
                                                  const float* __restrict__ xrow, const SddmmGeo g, int64_t s,
                                                  int64_t e, int lane, float* __restrict__ out) {
  const int jl = lane & (g.PK - 1);
  const int hs = (lane >> g.kshift) & (g.PH - 1);
  const int grp = lane >> (g.kshift + g.hshift);
  const int G = 64 >> (g.kshift + g.hshift);
  constexpr int NX = NR > 0 ? NR : 1;
  float xr[NX][VEC];
  if constexpr (NR > 0) {
#pragma unroll
    for (int it = 0; it < NR; ++it) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) xr[it][i] = 0.f;
      if (it < g.nit) {
        const Slice sl = slice_of<VEC>(g, it, hs, jl);
        if (sl.act) load_vec<VEC>(xrow + sl.off, xr[it]);
      }
    }
  }
  for (int64_t base = s; base < e; base += 64) {
    const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
    int64_t c_l = 0;
    if (lane < n) c_l = col[base + lane];
    for (int j = 0; j < n; j += G) {
      const int idx = j + grp;
      const bool ok = idx < n;
      const int64_t c = __shfl(static_cast<long long>(c_l), idx & 63);
      const float* __restrict__ yrow = y + c * g.D;
      float* __restrict__ orow = out + (base + idx) * g.H;
      float dot = 0.f;
      if constexpr (NR > 0) {
#pragma unroll
        for (int it = 0; it < NR; ++it) {
          if (it < g.nit) {  // wave-uniform
            const Slice sl = slice_of<VEC>(g, it, hs, jl);
            if (ok && sl.act) {
              float b[VEC];
              load_vec<VEC>(yrow + sl.off, b);
#pragma unroll
              for (int i = 0; i < VEC; ++i) dot += b[i] * xr[it][i];
            }
            if (sl.last) {
              dot = fold_head(dot, g.PK);
              if (ok && jl == 0 && sl.h < g.H) orow[sl.h] = dot;
              dot = 0.f;
            }
          }
        }
      } else {
        for (int it = 0; it < g.nit; ++it) {
          const Slice sl = slice_of<VEC>(g, it, hs, jl);
          if (ok && sl.act) {
            float b[VEC], xv[VEC];
            load_vec<VEC>(yrow + sl.off, b);
            load_vec<VEC>(xrow + sl.off, xv);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dot += b[i] * xv[i];
          }
          if (sl.last) {
            dot = fold_head(dot, g.PK);
            if (ok && jl == 0 && sl.h < g.H) orow[sl.h] = dot;
            dot = 0.f;
          }
        }
      }
    }
  }
}

template <int VEC, int NR>
__global__ void __launch_bounds__(kThreads)
sddmm_heads_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, const float* __restrict__ x,
                   const float* __restrict__ y, const SddmmGeo g, int64_t M, int64_t nnz, float* __restrict__ out,
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
  sddmm_heads_range<VEC, NR>(col, y, x + row * g.D, g, s, e, lane, out);
}

// One wave per 128-entry chunk of a listed row; chunks write disjoint entries.
template <int VEC, int NR>
__global__ void __launch_bounds__(kThreads)
sddmm_heads_chunk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                         const float* __restrict__ x, const float* __restrict__ y, const SddmmGeo g, int64_t nnz,
                         float* __restrict__ out, const unsigned long long* __restrict__ long_ctr,
                         const psa::LongEntry* __restrict__ long_list) {
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
    sddmm_heads_range<VEC, NR>(col, y, x + ent.row * g.D, g, s, e, lane, out);
  }
}

template <int VEC, int NR>
int launch_sddmm_heads(const int64_t* rowptr, const int64_t* col, const float* x, const float* y, const SddmmGeo g,
                       int64_t M, int64_t nnz, float* out, unsigned long long* ctr, psa::LongEntry* list,
                       hipStream_t s) {
  const int64_t gx = psa::ceil_div(M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((sddmm_heads_kernel<VEC, NR>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s, rowptr,
                     col, x, y, g, M, nnz, out, ctr, list);
  if (list) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(nnz), kWaves);
    cb = cb > kMaxChunkBlocks ? kMaxChunkBlocks : cb;
    hipLaunchKernelGGL((sddmm_heads_chunk_kernel<VEC, NR>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, s,
                       rowptr, col, x, y, g, nnz, out, ctr, list);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

size_t psa_spmm_heads_workspace_bytes(int64_t nnz, int64_t H, int64_t F) {
  if (H <= 0 || F <= 0 || nnz <= psa::kLongRow) return 0;  // no row can be long
  return psa::long_sums_layout(nullptr, nnz, H * F).bytes;
}

int psa_spmm_heads(const int64_t* rowptr, const int64_t* col, const float* value, const float* mat, int64_t M,
                   int64_t N, int64_t H, int64_t F, int64_t nnz, float* out, void* workspace,
                   size_t workspace_bytes, psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && N >= 0 && H >= 0 && F >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(H < (int64_t{1} << 24) && F < (int64_t{1} << 24), "H or F too large");
  const int64_t D = H * F;
  if (M == 0 || D == 0) return PSA_OK;
  PSA_REQUIRE(out != nullptr, "out is NULL");
  hipStream_t s = psa::as_stream(stream);
  if (nnz == 0) {
    PSA_ZERO(out, sizeof(float) * static_cast<size_t>(M) * static_cast<size_t>(D), s);
    return PSA_OK;
  }
  PSA_REQUIRE(rowptr && col && value && mat, "NULL pointer");
  psa::LongSums w;
  if (nnz > psa::kLongRow) {
    w = psa::long_sums_layout(workspace, nnz, D);
    const int rc = psa::begin_long_rows(__func__, workspace, workspace_bytes, w.bytes, w.ctr, s);
    if (rc != PSA_OK) return rc;
  }
  const bool v4 = (F % 4 == 0) && psa::aligned(mat, 16) && psa::aligned(out, 16);
  const int vec = v4 ? 4 : 1;
  SpmmGeo g;
  g.H = H;
  g.F = F;
  g.D = D;
  g.P = pow2_at_least(psa::ceil_div(D, vec), 64, &g.shift);
  const int64_t ntiles = psa::ceil_div(D, static_cast<int64_t>(g.P) * vec);
#define PSA_SPMM_HEADS(VEC, NT) \
  return launch_spmm_heads<VEC, NT>(rowptr, col, value, mat, g, ntiles, M, nnz, out, w.ctr, w.list, w.part, s)
  if (v4) {
    if (ntiles == 1) PSA_SPMM_HEADS(4, 1);
    if (ntiles == 2) PSA_SPMM_HEADS(4, 2);
    PSA_SPMM_HEADS(4, 4);
  }
  if (ntiles == 1) PSA_SPMM_HEADS(1, 1);
  if (ntiles == 2) PSA_SPMM_HEADS(1, 2);
  PSA_SPMM_HEADS(1, 4);
#undef PSA_SPMM_HEADS
}

size_t psa_sddmm_heads_workspace_bytes(int64_t nnz) {
  return nnz > psa::kLongRow ? psa::long_list_bytes(nnz) : 0;
}

int psa_sddmm_heads(const int64_t* rowptr, const int64_t* col, const float* x, const float* y, int64_t M, int64_t H,
                    int64_t K, int64_t nnz, float* out, void* workspace, size_t workspace_bytes,
                    psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && H >= 0 && K >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(H < (int64_t{1} << 24) && K < (int64_t{1} << 24), "H or K too large");
  if (nnz == 0 || H == 0) return PSA_OK;
  PSA_REQUIRE(out != nullptr, "out is NULL");
  hipStream_t s = psa::as_stream(stream);
  if (M == 0 || K == 0) {
    PSA_ZERO(out, sizeof(float) * static_cast<size_t>(nnz) * static_cast<size_t>(H), s);
    return PSA_OK;
  }
  PSA_REQUIRE(rowptr && col && x && y, "NULL pointer");
  psa::LongList w;
  if (nnz > psa::kLongRow) {
    psa::Carver c(workspace);
    psa::take_long_list(c, nnz, &w);
    const int rc = psa::begin_long_rows(__func__, workspace, workspace_bytes, c.off, w.ctr, s);
    if (rc != PSA_OK) return rc;
  }
  const bool v4 = (K % 4 == 0) && psa::aligned(x, 16) && psa::aligned(y, 16);
  const int vec = v4 ? 4 : 1;
  SddmmGeo g;
  g.H = H;
  g.K = K;
  g.D = H * K;
  const int64_t q = psa::ceil_div(K, vec);
  g.PK = pow2_at_least(q, 64, &g.kshift);
  g.PH = pow2_at_least(H, 64 / g.PK, &g.hshift);
  g.kiters = static_cast<int>(psa::ceil_div(q, g.PK));
  const int64_t nit = psa::ceil_div(H, g.PH) * g.kiters;
  PSA_REQUIRE(nit <= 0x7fffffff, "H * K too large");
  g.nit = static_cast<int>(nit);
#define PSA_SDDMM_HEADS(VEC, NR) \
  return launch_sddmm_heads<VEC, NR>(rowptr, col, x, y, g, M, nnz, out, w.ctr, w.list, s)
  if (v4) {
    if (nit == 1) PSA_SDDMM_HEADS(4, 1);
    if (nit == 2) PSA_SDDMM_HEADS(4, 2);
    if (nit <= kMaxTiles) PSA_SDDMM_HEADS(4, 4);
    PSA_SDDMM_HEADS(4, 0);
  }
  if (nit == 1) PSA_SDDMM_HEADS(1, 1);
  if (nit == 2) PSA_SDDMM_HEADS(1, 2);
  if (nit <= kMaxTiles) PSA_SDDMM_HEADS(1, 4);
  PSA_SDDMM_HEADS(1, 0);
#undef PSA_SDDMM_HEADS
}

}  // extern "C"
