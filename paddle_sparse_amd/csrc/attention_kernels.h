// Fused sparse attention, gfx950: sddmm + row softmax + SpMM in one pass per row.  The kernels and their host
// dispatch, written once over the element format of the dense operands (Fp32, Bf16 below) and instantiated by
// attention.hip (fp32) and attention_half.hip (bf16), which hold the extern "C" entry points.
//
//   s[e, h]      = scale * <q[row(e), h, :], k[col[e], h, :]> (+ bias[e, h] or bias[e])
//   p[e, h]      = softmax of s[., h] over the entries of row(e)
//   out[r, h, :] = sum_{e in row r} p[e, h] * v[col[e], h, :]
//
//   attention_fw  out [M, H, F] and stat [M, H, 2] = {m, l}: the row maximum and sum of exp(s - m)
//   attention_bw  p [nnz, H] and dS = p * (dP - delta) [nnz, H] from q, k, v, grad_out, out, stat
//                 both with dropout of the weights after the softmax where A::kDrop (attention_dropout.h):
//                 out = inv_keep * sum keep * p * v; the kernels are templates over their argument struct and
//                 the mask's statements sit under if constexpr
//   gat_fw / gat_bw  the additive scores of a GAT layer through the same kernels (A::kGat):
//                 s = LeakyReLU(a_row[row(e), h] + a_col[col[e], h] (+ bias)); only stage (a) below differs
//                 (gat_tile: no dot), stage (b), the long-row plan and the mask are shared; the backward writes
//                 dZ = dS * (z > 0 ? 1 : negative_slope) where dS was
//
// Nothing per entry is written by the forward: the backward recomputes s with the same code and forms
// p = exp(s - m) / l from the saved pair.
//
// Plan.  One wave per CSR row; rows above psa::kLongRow entries go through the long_rows.h list: one wave
// per 128-entry chunk leaves {m, l, unnormalised partial row} in the workspace and one wave per listed row
// merges the chunks in chunk order.  A wave walks its entries in tiles of 64.  Per tile
//   (a) the scores of the tile are computed in the psa_sddmm_heads layout (PK lanes share a head and fold
//       with xor shuffles, PH heads side by side, 64 / (PH * PK) entries per step) and written, scaled and
//       biased, to a per-wave LDS tile of 64 x Hb floats;
//   (b) the tile is consumed in the psa_spmm_heads layout: a lane owns VEC elements of the Hb * F elements of
//       a row of v, P lanes serve an entry, lane group g takes entries g, g + G, ... and keeps a running
//       {m, l, acc} for the head of its elements (online softmax: a new maximum rescales l and acc by
//       exp(m_old - m_new)).
// At the end of the range the lane groups merge with xor shuffles; the merge is written without
// contraction, so both partners of a step hold the same bits.  VEC is the format's 16-byte form when the
// widths divide by it and the dense operands start on 16 bytes, else 1 (element loads at any element
// alignment; there is no 8-byte middle form).  Heads are taken in blocks of Hb <= 16 with Hb * F elements
// within the tiles of accumulators a lane keeps (a single head wider than that repeats the pass per group of
// tiles), so any H, K, F >= 1 is served; H <= 16 with H * F <= 1024 is one pass in either format.
//
// fp32.  VEC = 4 or 1, four tiles of accumulators in both forms.  Every value is fp32 from load to store.
//
// bf16.  q, k, v, out and grad_out (GAT: a_row, a_col, v, out, grad_out) are two-byte; every product, the scores,
// the online softmax, {m, l}, the accumulators and the long-row partials are fp32, and a result is rounded once
// (nearest even) where it is written: inv_keep is applied in fp32 before that rounding, and the backward's
// delta = <grad_out, out> is taken from the saved, rounded out.  The bias, stat, p and dS stay fp32.  VEC = 8
// (half_util.h: widen8 / narrow8) or 1 (widen1 / narrow1).  The 16-byte form keeps two tiles of accumulators,
// not four: a tile is 8 fp32 accumulators per lane there, and four of them beside the four slices of q took
// the chunk kernel to 256 VGPRs and into AGPR copies.  The partials are written as floats (two 16-byte stores
// per lane for VEC = 8).
//
// Non-finite values by plain IEEE arithmetic, as softmax.hip: fmaxf drops a NaN but exp(NaN - m) poisons
// l; +inf gives inf - inf; a row of nothing but -inf ends with {-inf, 0} and 0 / 0; -inf among finite
// scores has weight exp(-inf) = 0 exactly, and 0 * inf in v is NaN (no zero skipping).  exp is expf.
// No float atomics, no host read: the bits repeat from run to run and the calls can be captured.
// Every address is formed in 64-bit arithmetic.
#pragma once

#include <cmath>

#include "common.h"
#include "attention_dropout.h"
#include "half_rows.h"
#include "long_rows.h"

namespace {

using psa_half::clamp_range;
using psa_half::load_f32;
using psa_half::pow2_at_least;
using psa_half::store_f32;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxChunkBlocks = 4096;
constexpr int kMaxTiles = 4;  // tiles of accumulators / slices of the row of q kept in registers
constexpr int kHeadBlock = 16;  // heads per pass: the LDS tile is 64 entries x kHeadBlock floats per wave

// ---- the element formats of the dense operands ------------------------------------------------------

// load<VEC> gives a lane's VEC elements as fp32, store<VEC> writes VEC fp32 results; VEC is kVec16 (one 16-byte
// access, p 16-byte aligned) or 1.
struct Fp32 {
  typedef float elem_t;
  static constexpr int kVec16 = 4;          // elements of the 16-byte form
  static constexpr int kTiles16 = 4;        // tiles of accumulators of the forward's 16-byte form
  static constexpr bool kTwoByte = false;
  static constexpr elem_t kZero = 0.f;      // an empty row
  template <int VEC>
  static __device__ __forceinline__ void load(const float* p, float (&dst)[VEC]) { load_f32<VEC>(p, dst); }
  template <int VEC>
  static __device__ __forceinline__ void store(float* p, const float (&src)[VEC]) { store_f32<VEC>(p, src); }
  static __device__ __forceinline__ float load1(const float* p, int64_t i) { return p[i]; }
};

// Widened exactly on load; store is the one rounding of a result (nearest even).
struct Bf16 {
  typedef psa_half::elem_t elem_t;
  static constexpr int kVec16 = 8;
  static constexpr int kTiles16 = 2;        // four tiles of eight accumulators took the chunk kernel to 256 VGPRs
  static constexpr bool kTwoByte = true;    // the entry points take a dtype and check the element alignment
  static constexpr elem_t kZero = 0;        // +0 has the same bits in both formats
  template <int VEC>
  static __device__ __forceinline__ void load(const elem_t* p, float (&dst)[VEC]) {
    psa_half::load_vec<psa_half::BF16, VEC>(p, dst);
  }
  template <int VEC>
  static __device__ __forceinline__ void store(elem_t* p, const float (&src)[VEC]) {
    psa_half::store_vec<psa_half::BF16, VEC>(p, src);
  }
  static __device__ __forceinline__ float load1(const elem_t* p, int64_t i) {
    return psa_half::widen1<psa_half::BF16>(p, i);
  }
};

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

// The lanes of a wave hand data to each other through their LDS tile: LDS operations of one wave
// complete in order, the fences keep the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- per-head dots of one row against gathered rows (the psa_sddmm_heads layout) ------------------

struct DotGeo {
  int64_t K;       // elements per head
  int64_t stride;  // elements per row of the dense operands (H * K)
  int PK, kshift;  // lanes per head
  int PH, hshift;  // heads side by side
  int kiters;      // steps of PK * VEC elements over K
  int nit;         // head passes * kiters for a full head block
};

struct Slice {
  int h;        // head of the slice inside the head block
  int64_t off;  // h * K + k: first element of it from the block's first head
  bool act;     // the lane has elements in it
  bool last;    // the head's dot is complete after it
};

template <int VEC>
__device__ __forceinline__ Slice slice_of(const DotGeo g, int Hs, int it, int hs, int jl) {
  const int hp = it / g.kiters;
  const int ki = it - hp * g.kiters;
  const int64_t k = (static_cast<int64_t>(ki) * g.PK + jl) * VEC;
  Slice sl;
  sl.h = hp * g.PH + hs;
  sl.act = sl.h < Hs && k < g.K;
  sl.off = static_cast<int64_t>(sl.h) * g.K + k;
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

// The slices of xrow that the lane meets, as fp32 in registers (NR > 0 and nit <= NR).
template <class Fmt, int VEC, int NR>
__device__ __forceinline__ void load_slices(const typename Fmt::elem_t* __restrict__ xrow, const DotGeo g, int Hs,
                                            int lane, float (&xr)[NR > 0 ? NR : 1][VEC]) {
  if constexpr (NR > 0) {
    const int jl = lane & (g.PK - 1);
    const int hs = (lane >> g.kshift) & (g.PH - 1);
#pragma unroll
    for (int it = 0; it < NR; ++it) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) xr[it][i] = 0.f;
      if (it < g.nit) {
        const Slice sl = slice_of<VEC>(g, Hs, it, hs, jl);
        if (sl.act) Fmt::template load<VEC>(xrow + sl.off, xr[it]);
      }
    }
  }
}

// tile[idx * ldt + h] = scale * <xrow[h, :], y[c(idx), h, :]> (+ bias[idx * bstride + h * bhstep]) for the
// n <= 64 entries whose gathered rows lane idx names in c_l and the Hs heads of the block.  xrow, y and
// bias point at the block's first head (bias also at the tile's first entry).
template <class Fmt, int VEC, int NR>
__device__ __forceinline__ void dots_tile(const typename Fmt::elem_t* __restrict__ y,
                                          const typename Fmt::elem_t* __restrict__ xrow,
                                          const float (&xr)[NR > 0 ? NR : 1][VEC], const DotGeo g, int Hs,
                                          int64_t c_l, int n, int lane, float scale, const float* __restrict__ bias,
                                          int64_t bstride, int bhstep, float* __restrict__ tile, int ldt) {
  const int jl = lane & (g.PK - 1);
  const int hs = (lane >> g.kshift) & (g.PH - 1);
  const int grp = lane >> (g.kshift + g.hshift);
  const int G = 64 >> (g.kshift + g.hshift);
  for (int j = 0; j < n; j += G) {
    const int idx = j + grp;
    const bool ok = idx < n;
    const int64_t c = __shfl(static_cast<long long>(c_l), idx & 63);
    const typename Fmt::elem_t* __restrict__ yrow = y + c * g.stride;
    float dot = 0.f;
    auto finish = [&](const Slice sl) {
      dot = fold_head(dot, g.PK);
      if (ok && jl == 0 && sl.h < Hs) {
        float sc = __fmul_rn(scale, dot);
        if (bias) sc = __fadd_rn(sc, bias[static_cast<int64_t>(idx) * bstride + static_cast<int64_t>(sl.h) * bhstep]);
        tile[idx * ldt + sl.h] = sc;
      }
      dot = 0.f;
    };
    if constexpr (NR > 0) {
#pragma unroll
      for (int it = 0; it < NR; ++it) {
        if (it < g.nit) {  // wave-uniform
          const Slice sl = slice_of<VEC>(g, Hs, it, hs, jl);
          if (ok && sl.act) {
            float b[VEC];
            Fmt::template load<VEC>(yrow + sl.off, b);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dot += b[i] * xr[it][i];
          }
          if (sl.last) finish(sl);
        }
      }
    } else {
      for (int it = 0; it < g.nit; ++it) {
        const Slice sl = slice_of<VEC>(g, Hs, it, hs, jl);
        if (ok && sl.act) {
          float b[VEC], xv[VEC];
          Fmt::template load<VEC>(yrow + sl.off, b);
          Fmt::template load<VEC>(xrow + sl.off, xv);
#pragma unroll
          for (int i = 0; i < VEC; ++i) dot += b[i] * xv[i];
        }
        if (sl.last) finish(sl);
      }
    }
  }
}

// ---- additive scores of a GAT layer: stage (a) without a dot ---------------------------------------

// s of z: z itself where z > 0, the rounded product otherwise (z == 0 and a NaN take the slope branch).
__device__ __forceinline__ float gat_act(float z, float slope) { return z > 0.f ? z : __fmul_rn(slope, z); }

// tile[idx * Hb + h] = s (ACT) or z, with z = (a_row[row, h] + a_col[c(idx), h]) (+ bias), for the n <= 64
// entries from base on and the Hs heads from hb on, in fp32; no contraction, so forward and backward agree bit for bit.
// Lane t takes (idx, h) = (t / Hs, t % Hs) for t = lane, lane + 64, ...: the mapping of attn_bw_range's
// consumer loop.  Element loads at any element alignment.
template <class A, bool ACT>
__device__ __forceinline__ void gat_tile(const A& a, int64_t row, int64_t hb, int Hs, int64_t c_l, int n,
                                         int64_t base, int lane, float* __restrict__ tile) {
  const int total = n * Hs;
  for (int t0 = 0; t0 < total; t0 += 64) {  // wave-uniform trips: the shuffle reads every lane's c_l
    const int t = t0 + lane;
    const bool ok = t < total;
    const int idx = ok ? t / Hs : 0;
    const int h = t - idx * Hs;
    const int64_t c = __shfl(static_cast<long long>(c_l), idx);
    if (ok) {
      const int64_t hh = hb + h;
      float z = __fadd_rn(A::Fmt::load1(a.a_row, row * a.H + hh), A::Fmt::load1(a.a_col, c * a.H + hh));
      if (a.bias) z = __fadd_rn(z, a.bias[(base + idx) * a.bias_heads + (a.bias_heads == 1 ? 0 : hh)]);
      tile[idx * a.Hb + h] = ACT ? gat_act(z, a.slope) : z;
    }
  }
}

// ---- forward --------------------------------------------------------------------------------------

template <class Format>
struct FwArgs {
  using Fmt = Format;
  const int64_t* rowptr;
  const int64_t* col;
  const typename Format::elem_t* q;
  const typename Format::elem_t* k;
  const typename Format::elem_t* v;
  const float* bias;  // NULL: no bias
  int64_t bias_heads;  // 1 or H
  float scale;
  int64_t M, H, K, F, nnz;
  int Hb;       // heads per block
  DotGeo dot;   // scores
  int P, shift;  // lanes per entry in the aggregation
  int ntiles;   // tiles of P * VEC elements over Hb * F
  static constexpr bool kDrop = false;
  static constexpr bool kGat = false;
};

// The dropout forms of the kernels take their arguments with the mask's parameters behind them; the plain
// forms never see them (every use sits under if constexpr (A::kDrop)).
template <class Format>
struct FwDropArgs : FwArgs<Format> {
  static constexpr bool kDrop = true;
  psa::Drop drop;
};

// The GAT forms: q, k, scale, K and dot are not used (every use sits under if constexpr (!A::kGat)).
template <class Format, bool DROP>
struct GatFwArgs : FwArgs<Format> {
  static constexpr bool kDrop = DROP;
  static constexpr bool kGat = true;
  const typename Format::elem_t* a_row;  // [M, H]
  const typename Format::elem_t* a_col;  // [N, H]
  float slope;
  psa::Drop drop;
};

// {m, l} of two disjoint sets of entries and the factors that bring their sums to the common maximum.
// Commutative bit for bit (no contraction), so that both partners of an xor step agree.
__device__ __forceinline__ void merge_factors(float am, float bm, float& m, float& fa, float& fb) {
  m = fmaxf(am, bm);
  fa = am == m ? 1.f : expf(am - m);
  fb = bm == m ? 1.f : expf(bm - m);
}

__device__ __forceinline__ float merge_sum(float a, float fa, float b, float fb) {
  return __fadd_rn(__fmul_rn(a, fa), __fmul_rn(b, fb));
}

// {m, l, acc} of the entries [s, e) of one row for the NT tiles from tile0 on of head block hb, merged over
// the lane groups: every lane ends with the fp32 state of the elements it owns.
// Dropout: keeps[h] holds the keep bits of the tile's 64 entries for head h of the block; a dropped entry
// counts in l and adds an exact 0 * v to acc.
template <class A, int VEC, int NR, int NT>
__device__ __forceinline__ void attn_range(const A& a, int64_t row, int hb, int Hs, int tile0, int64_t s,
                                           int64_t e, int lane, float* __restrict__ tile,
                                           unsigned long long* __restrict__ keeps, float (&m)[NT],
                                           float (&l)[NT], float (&acc)[NT][VEC]) {
  using Fmt = typename A::Fmt;
  using E = typename Fmt::elem_t;
  constexpr int U = kMaxTiles / NT;  // entries in flight per lane
  const int grp = lane >> a.shift;
  const int p = lane & (a.P - 1);
  const int G = 64 >> a.shift;
  const int64_t Ds = static_cast<int64_t>(Hs) * a.F;
  const int64_t vstride = a.H * a.F;
  const E* __restrict__ qrow = nullptr;
  const E* __restrict__ kb = nullptr;
  if constexpr (!A::kGat) {
    qrow = a.q + row * a.dot.stride + static_cast<int64_t>(hb) * a.K;
    kb = a.k + static_cast<int64_t>(hb) * a.K;
  }
  const E* __restrict__ vb = a.v + static_cast<int64_t>(hb) * a.F;
  const int bhstep = a.bias_heads == 1 ? 0 : 1;
  const float* __restrict__ biasb = a.bias ? a.bias + (bhstep ? hb : 0) : nullptr;
  int64_t d[NT];
  int hd[NT];
  bool act[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    d[t] = (static_cast<int64_t>(tile0 + t) * a.P + p) * VEC;
    act[t] = d[t] < Ds;
    hd[t] = act[t] ? static_cast<int>(d[t] / a.F) : 0;
    m[t] = neg_inf();
    l[t] = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[t][i] = 0.f;
  }
  float xr[NR > 0 ? NR : 1][VEC];
  if constexpr (!A::kGat) load_slices<Fmt, VEC, NR>(qrow, a.dot, Hs, lane, xr);
  for (int64_t base = s; base < e; base += 64) {
    const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
    int64_t c_l = 0;
    if (lane < n) c_l = a.col[base + lane];
    wave_sync();  // the previous tile has been consumed
    if constexpr (A::kGat) {
      gat_tile<A, true>(a, row, hb, Hs, c_l, n, base, lane, tile);
    } else {
      dots_tile<Fmt, VEC, NR>(kb, qrow, xr, a.dot, Hs, c_l, n, lane, a.scale,
                         biasb ? biasb + base * a.bias_heads : nullptr, a.bias_heads, bhstep, tile, a.Hb);
    }
    if constexpr (A::kDrop) {  // one draw per (entry, head): lane i draws for entry base + i, a ballot per head
      const uint64_t stream = psa::rand_stream(a.drop.seed, base + lane);
      for (int h = 0; h < Hs; ++h) {
        const unsigned long long bits = __ballot(psa::keep_of(stream, static_cast<int64_t>(hb) + h, a.drop.T));
        if (lane == 0) keeps[h] = bits;
      }
    }
    wave_sync();
    for (int j = 0; j < n; j += G * U) {
      float b[U][NT][VEC], sc[U][NT];
      bool ok[U], kept[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = j + u * G + grp;
        ok[u] = idx < n;
        const int64_t c = __shfl(static_cast<long long>(c_l), idx & 63);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          sc[u][t] = 0.f;
          kept[u][t] = true;
#pragma unroll
          for (int i = 0; i < VEC; ++i) b[u][t][i] = 0.f;
          if (ok[u] && act[t]) {
            sc[u][t] = tile[idx * a.Hb + hd[t]];
            if constexpr (A::kDrop) kept[u][t] = (keeps[hd[t]] >> idx) & 1ull;
            Fmt::template load<VEC>(vb + c * vstride + d[t], b[u][t]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (ok[u] && act[t]) {
            const float mn = fmaxf(m[t], sc[u][t]);
            if (mn != m[t]) {  // a new maximum: bring l and acc to it (exp(-inf) = 0 for the first entry)
              const float f = expf(m[t] - mn);
              l[t] *= f;
#pragma unroll
              for (int i = 0; i < VEC; ++i) acc[t][i] *= f;
              m[t] = mn;
            }
            // nothing but -inf so far: against 0, so that -inf adds an exact 0 and a NaN stays a NaN
            const float w = expf(sc[u][t] - (mn == neg_inf() ? 0.f : mn));
            l[t] += w;
            const float wk = kept[u][t] ? w : 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[t][i] += wk * b[u][t][i];
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    if (off >= a.P) {  // wave-uniform
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float om = __shfl_xor(m[t], off), ol = __shfl_xor(l[t], off);
        float mn, fa, fb;
        merge_factors(m[t], om, mn, fa, fb);
        l[t] = merge_sum(l[t], fa, ol, fb);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[t][i] = merge_sum(acc[t][i], fa, __shfl_xor(acc[t][i], off), fb);
        m[t] = mn;
      }
    }
  }
}

// All head blocks and tiles of the range [s, e) of one row into dst[0 .. H * F) and sdst[0 .. 2 * H):
// the row itself (NORMALISE: dst is elements, acc / l stored once) or a chunk's partial (dst is floats, acc as it is).
template <class A, int VEC, int NR, int NT, bool NORMALISE>
__device__ __forceinline__ void attn_row(const A& a, int64_t row, int64_t s, int64_t e, int lane,
                                         float* __restrict__ tile, unsigned long long* __restrict__ keeps,
                                         void* __restrict__ dst, float* __restrict__ sdst) {
  using Fmt = typename A::Fmt;
  const int grp = lane >> a.shift;
  const int p = lane & (a.P - 1);
  for (int64_t hb = 0; hb < a.H; hb += a.Hb) {
    const int Hs = a.H - hb < a.Hb ? static_cast<int>(a.H - hb) : a.Hb;
    const int64_t Ds = static_cast<int64_t>(Hs) * a.F;
    for (int tile0 = 0; tile0 < a.ntiles; tile0 += NT) {
      float m[NT], l[NT], acc[NT][VEC];
      attn_range<A, VEC, NR, NT>(a, row, static_cast<int>(hb), Hs, tile0, s, e, lane, tile, keeps, m, l, acc);
      if (grp == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int64_t d = (static_cast<int64_t>(tile0 + t) * a.P + p) * VEC;
          if (d < Ds) {
            if constexpr (NORMALISE) {
#pragma unroll
              for (int i = 0; i < VEC; ++i) acc[t][i] = acc[t][i] / l[t];
              if constexpr (A::kDrop) {  // once per output element, after the division
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[t][i] = __fmul_rn(acc[t][i], a.drop.inv_keep);
              }
              Fmt::template store<VEC>(static_cast<typename Fmt::elem_t*>(dst) + hb * a.F + d, acc[t]);
            } else {
              store_f32<VEC>(static_cast<float*>(dst) + hb * a.F + d, acc[t]);
            }
            if (d % a.F == 0) {  // the first element of a head
              const int64_t h = hb + d / a.F;
              sdst[2 * h] = m[t];
              sdst[2 * h + 1] = l[t];
            }
          }
        }
      }
    }
  }
}

// The dropout forms keep their keep bits (kHeadBlock x 64 bits per wave) behind the wave's tile.
template <class A>
constexpr int tile_floats() { return 64 * kHeadBlock + (A::kDrop ? 2 * kHeadBlock : 0); }

template <class A>
__device__ __forceinline__ unsigned long long* keeps_of(float* tile) {
  return reinterpret_cast<unsigned long long*>(tile + 64 * kHeadBlock);  // 4096 bytes in: 8-byte aligned
}

template <class A, int VEC, int NR, int NT>
__global__ void __launch_bounds__(kThreads)
attn_fw_kernel(const A a, typename A::Fmt::elem_t* __restrict__ out, float* __restrict__ stat,
               unsigned long long* __restrict__ long_ctr, psa::LongEntry* __restrict__ long_list) {
  __shared__ float tiles[kWaves][tile_floats<A>()];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (row >= a.M) return;
  int64_t s = a.rowptr[row], e = a.rowptr[row + 1];
  clamp_range(s, e, a.nnz);
  if (long_list && e - s > psa::kLongRow) {  // wave-uniform: hand the row to chunk waves
    if (lane == 0) psa::push_long_row(long_ctr, long_list, row, e - s);
    return;
  }
  const int64_t D = a.H * a.F;
  typename A::Fmt::elem_t* __restrict__ orow = out + row * D;
  float* __restrict__ srow = stat + row * a.H * 2;
  if (e <= s) {  // a row without entries: zeros and {-inf, 0}
    for (int64_t dd = lane; dd < D; dd += 64) orow[dd] = A::Fmt::kZero;
    for (int64_t h = lane; h < a.H; h += 64) {
      srow[2 * h] = neg_inf();
      srow[2 * h + 1] = 0.f;
    }
    return;
  }
  attn_row<A, VEC, NR, NT, true>(a, row, s, e, lane, tiles[wave], keeps_of<A>(tiles[wave]), orow, srow);
}

// One wave per 128-entry chunk of a listed row: part[c, 0 .. D) unnormalised and pstat[c, h] = {m, l}, fp32.
template <class A, int VEC, int NR, int NT>
__global__ void __launch_bounds__(kThreads)
attn_fw_chunk_kernel(const A a, const unsigned long long* __restrict__ long_ctr,
                     const psa::LongEntry* __restrict__ long_list, float* __restrict__ part,
                     float* __restrict__ pstat) {
  __shared__ float tiles[kWaves][tile_floats<A>()];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long ctr = *long_ctr;
  const uint32_t total = static_cast<uint32_t>(ctr & 0xffffffffull);
  const int nrows = static_cast<int>(ctr >> 32);
  const uint32_t num_waves = gridDim.x * kWaves;
  const int64_t D = a.H * a.F;
  for (uint32_t c = blockIdx.x * kWaves + wave; c < total; c += num_waves) {
    const psa::LongEntry ent = psa::find_long_entry(long_list, nrows, c);
    int64_t rs = a.rowptr[ent.row], re = a.rowptr[ent.row + 1];
    clamp_range(rs, re, a.nnz);
    const int64_t s = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
    const int64_t e = s + psa::kLongChunk < re ? s + psa::kLongChunk : re;
    attn_row<A, VEC, NR, NT, false>(a, ent.row, s, e, lane, tiles[wave], keeps_of<A>(tiles[wave]),
                                    part + static_cast<int64_t>(c) * D, pstat + static_cast<int64_t>(c) * a.H * 2);
  }
}

// One wave per listed row: its chunks' fp32 partials merged in chunk order, whatever order the list was built
// in, then stored once.  An all -inf chunk carries {-inf, 0} and merges as nothing.
// DROP: inv_keep is applied here, once per output element and before the store, not by the chunks.
template <class Fmt, int VEC, bool DROP>
__global__ void __launch_bounds__(kThreads)
attn_fw_combine_kernel(int64_t H, int64_t F, const unsigned long long* __restrict__ long_ctr,
                       const psa::LongEntry* __restrict__ long_list, const float* __restrict__ part,
                       const float* __restrict__ pstat, typename Fmt::elem_t* __restrict__ out,
                       float* __restrict__ stat, float inv_keep) {
  const int lane = threadIdx.x & 63;
  const int nrows = static_cast<int>(*long_ctr >> 32);
  const int num_waves = static_cast<int>(gridDim.x) * kWaves;
  const int64_t D = H * F;
  for (int slot = blockIdx.x * kWaves + (threadIdx.x >> 6); slot < nrows; slot += num_waves) {
    const psa::LongEntry ent = long_list[slot];
    for (int64_t d = static_cast<int64_t>(lane) * VEC; d < D; d += 64 * VEC) {
      const int64_t h = d / F;
      float m = neg_inf(), l = 0.f, acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
      for (uint32_t k = 0; k < ent.num_chunks; ++k) {
        const int64_t c = static_cast<int64_t>(ent.first_chunk + k);
        const float cm = pstat[(c * H + h) * 2], cl = pstat[(c * H + h) * 2 + 1];
        float b[VEC];
        load_f32<VEC>(part + c * D + d, b);
        float mn, fa, fb;
        merge_factors(m, cm, mn, fa, fb);
        l = merge_sum(l, fa, cl, fb);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = merge_sum(acc[i], fa, b[i], fb);
        m = mn;
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = acc[i] / l;
      if constexpr (DROP) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = __fmul_rn(acc[i], inv_keep);
      }
      Fmt::template store<VEC>(out + ent.row * D + d, acc);
      if (d % F == 0) {
        stat[(ent.row * H + h) * 2] = m;
        stat[(ent.row * H + h) * 2 + 1] = l;
      }
    }
  }
}

// ---- backward, the per-entry half -----------------------------------------------------------------

template <class Format>
struct BwArgs {
  using Fmt = Format;
  const int64_t* rowptr;
  const int64_t* col;
  const typename Format::elem_t* q;
  const typename Format::elem_t* k;
  const typename Format::elem_t* v;
  const float* bias;
  int64_t bias_heads;
  float scale;
  const typename Format::elem_t* grad_out;
  const typename Format::elem_t* out;  // as the forward stored it
  const float* stat;
  int64_t M, H, K, F, nnz;
  int Hb;
  DotGeo dot;   // scores: over K
  DotGeo dotf;  // dP and delta: over F
  float* p;
  float* ds;
  static constexpr bool kDrop = false;
  static constexpr bool kGat = false;
};

template <class Format>
struct BwDropArgs : BwArgs<Format> {
  static constexpr bool kDrop = true;
  psa::Drop drop;
};

// The GAT forms: ds receives dZ; q, k, scale, K and dot are not used.
template <class Format, bool DROP>
struct GatBwArgs : BwArgs<Format> {
  static constexpr bool kDrop = DROP;
  static constexpr bool kGat = true;
  const typename Format::elem_t* a_row;
  const typename Format::elem_t* a_col;
  float slope;
  psa::Drop drop;
};

// p and dS of the entries [s, e) of one row.  Dropout, with D = keep * inv_keep recomputed per (entry, head)
// by the lane that writes it: p * D where p is written, and dS = p * (D * dP - delta).
// GAT: tile_s receives z (gat_tile, NRK = 0); the consumer applies the activation, so that it has the sign of z
// for dZ = dS * (z > 0 ? 1 : slope), rounded once more.
template <class A, int VEC, int NRK, int NRF>
__device__ __forceinline__ void attn_bw_range(const A& a, int64_t row, int64_t s, int64_t e, int lane,
                                              float* __restrict__ tile_s, float* __restrict__ tile_p,
                                              float* __restrict__ delta) {
  using Fmt = typename A::Fmt;
  using E = typename Fmt::elem_t;
  const int bhstep = a.bias_heads == 1 ? 0 : 1;
  for (int64_t hb = 0; hb < a.H; hb += a.Hb) {
    const int Hs = a.H - hb < a.Hb ? static_cast<int>(a.H - hb) : a.Hb;
    const E* __restrict__ qrow = nullptr;
    if constexpr (!A::kGat) qrow = a.q + row * a.dot.stride + hb * a.K;
    const E* __restrict__ grow = a.grad_out + row * a.dotf.stride + hb * a.F;
    const float* __restrict__ biasb = a.bias ? a.bias + (bhstep ? hb : 0) : nullptr;
    float xq[NRK > 0 ? NRK : 1][VEC], xg[NRF > 0 ? NRF : 1][VEC];
    if constexpr (!A::kGat) load_slices<Fmt, VEC, NRK>(qrow, a.dot, Hs, lane, xq);
    load_slices<Fmt, VEC, NRF>(grow, a.dotf, Hs, lane, xg);
    wave_sync();  // the previous head block has been consumed
    // delta[h] = <grad_out[row, h, :], out[row, h, :]>: the row of the saved out as the one gathered row
    dots_tile<Fmt, VEC, NRF>(a.out + hb * a.F, grow, xg, a.dotf, Hs, row, 1, lane, 1.f, nullptr, 0, 0, delta, 0);
    for (int64_t base = s; base < e; base += 64) {
      const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
      int64_t c_l = 0;
      if (lane < n) c_l = a.col[base + lane];
      if constexpr (A::kGat) {
        gat_tile<A, false>(a, row, hb, Hs, c_l, n, base, lane, tile_s);
      } else {
        dots_tile<Fmt, VEC, NRK>(a.k + hb * a.K, qrow, xq, a.dot, Hs, c_l, n, lane, a.scale,
                            biasb ? biasb + base * a.bias_heads : nullptr, a.bias_heads, bhstep, tile_s, a.Hb);
      }
      dots_tile<Fmt, VEC, NRF>(a.v + hb * a.F, grow, xg, a.dotf, Hs, c_l, n, lane, 1.f, nullptr, 0, 0, tile_p, a.Hb);
      wave_sync();
      for (int t = lane; t < n * Hs; t += 64) {
        const int idx = t / Hs;
        const int h = t - idx * Hs;
        const float m = a.stat[(row * a.H + hb + h) * 2], l = a.stat[(row * a.H + hb + h) * 2 + 1];
        float sc = tile_s[idx * a.Hb + h], fac = 1.f;
        if constexpr (A::kGat) {
          fac = sc > 0.f ? 1.f : a.slope;
          sc = gat_act(sc, a.slope);
        }
        const float pe = expf(sc - m) / l;
        const int64_t at = (base + idx) * a.H + hb + h;
        float dse;
        if constexpr (A::kDrop) {
          const bool kept = psa::keep_of(psa::rand_stream(a.drop.seed, base + idx), hb + h, a.drop.T);
          const float dk = kept ? a.drop.inv_keep : 0.f;
          a.p[at] = __fmul_rn(pe, dk);
          dse = pe * (__fmul_rn(dk, tile_p[idx * a.Hb + h]) - delta[h]);
        } else {
          a.p[at] = pe;
          dse = pe * (tile_p[idx * a.Hb + h] - delta[h]);
        }
        a.ds[at] = A::kGat ? __fmul_rn(dse, fac) : dse;
      }
      wave_sync();  // before the next tile overwrites
    }
  }
}

template <class A, int VEC, int NRK, int NRF>
__global__ void __launch_bounds__(kThreads)
attn_bw_kernel(const A a, unsigned long long* __restrict__ long_ctr, psa::LongEntry* __restrict__ long_list) {
  __shared__ float tiles[kWaves][2][64 * kHeadBlock];
  __shared__ float deltas[kWaves][kHeadBlock];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (row >= a.M) return;
  int64_t s = a.rowptr[row], e = a.rowptr[row + 1];
  clamp_range(s, e, a.nnz);
  if (e <= s) return;  // a row without entries writes nothing
  if (long_list && e - s > psa::kLongRow) {  // wave-uniform: hand the row to chunk waves
    if (lane == 0) psa::push_long_row(long_ctr, long_list, row, e - s);
    return;
  }
  attn_bw_range<A, VEC, NRK, NRF>(a, row, s, e, lane, tiles[wave][0], tiles[wave][1], deltas[wave]);
}

// One wave per 128-entry chunk of a listed row; chunks write disjoint entries.
template <class A, int VEC, int NRK, int NRF>
__global__ void __launch_bounds__(kThreads)
attn_bw_chunk_kernel(const A a, const unsigned long long* __restrict__ long_ctr,
                     const psa::LongEntry* __restrict__ long_list) {
  __shared__ float tiles[kWaves][2][64 * kHeadBlock];
  __shared__ float deltas[kWaves][kHeadBlock];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long ctr = *long_ctr;
  const uint32_t total = static_cast<uint32_t>(ctr & 0xffffffffull);
  const int nrows = static_cast<int>(ctr >> 32);
  const uint32_t num_waves = gridDim.x * kWaves;
  for (uint32_t c = blockIdx.x * kWaves + wave; c < total; c += num_waves) {
    const psa::LongEntry ent = psa::find_long_entry(long_list, nrows, c);
    int64_t rs = a.rowptr[ent.row], re = a.rowptr[ent.row + 1];
    clamp_range(rs, re, a.nnz);
    const int64_t s = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
    const int64_t e = s + psa::kLongChunk < re ? s + psa::kLongChunk : re;
    attn_bw_range<A, VEC, NRK, NRF>(a, ent.row, s, e, lane, tiles[wave][0], tiles[wave][1], deltas[wave]);
  }
}

// ---- host -----------------------------------------------------------------------------------------

// Tiles of accumulators of the forward: kMaxTiles in the element form, the format's budget in its 16-byte form.
template <class Fmt>
constexpr int fw_tiles(int vec) { return vec == 1 ? kMaxTiles : Fmt::kTiles16; }

// Heads per pass: at most kHeadBlock, and Hb * F elements within fw_tiles(vec) tiles of 64 * vec elements.
template <class Fmt>
int head_block(int64_t H, int64_t F, int vec) {
  int64_t hb = (static_cast<int64_t>(fw_tiles<Fmt>(vec)) * 64 * vec) / F;
  hb = hb < 1 ? 1 : hb;
  hb = hb > kHeadBlock ? kHeadBlock : hb;
  return static_cast<int>(hb > H ? H : hb);
}

DotGeo dot_geo(int64_t H, int Hb, int64_t K, int vec) {
  DotGeo g;
  g.K = K;
  g.stride = H * K;
  const int64_t q = psa::ceil_div(K, vec);
  g.PK = pow2_at_least(q, 64, &g.kshift);
  g.PH = pow2_at_least(Hb, 64 / g.PK, &g.hshift);
  g.kiters = static_cast<int>(psa::ceil_div(q, g.PK));
  g.nit = static_cast<int>(psa::ceil_div(Hb, g.PH)) * g.kiters;
  return g;
}

int chunk_blocks(int64_t n) {
  const int64_t b = psa::ceil_div(n, kWaves);
  return static_cast<int>(b > kMaxChunkBlocks ? kMaxChunkBlocks : b);
}

// The entry points share their bodies; errors carry the caller's name.
#define ATTN_REQUIRE(cond, msg)                          \
  do {                                                   \
    if (!(cond)) {                                       \
      psa::set_error(std::string(who) + ": " + (msg));   \
      return PSA_ERR_INVALID_ARG;                        \
    }                                                    \
  } while (0)

// What a call has of the workspace: all NULL when no row can be long.
struct LongRows : psa::LongList {
  float* part = nullptr;   // forward only: [chunks, H * F]
  float* pstat = nullptr;  // forward only: [chunks, H, 2]
  size_t bytes = 0;
};

// {list} and, for the forward (partials), the two arrays of the chunks behind it.  The partials are fp32 whatever
// the operands are: one layout, whose full form is psa_attention_workspace_bytes.
LongRows long_layout(void* workspace, int64_t nnz, int64_t H, int64_t F, bool partials) {
  psa::Carver c(workspace);
  LongRows lr;
  psa::take_long_list(c, nnz, &lr);
  if (partials) {
    lr.part = psa::take_long_chunks<float>(c, nnz, H * F);
    lr.pstat = psa::take_long_chunks<float>(c, nnz, H * 2);
  }
  lr.bytes = c.off;
  return lr;
}

// The layout over the caller's workspace, checked, its counter zeroed (0 rows listed so far).
int take_long_rows(const char* who, void* workspace, size_t have, int64_t nnz, int64_t H, int64_t F, bool partials,
                   hipStream_t s, LongRows* lr) {
  if (nnz <= psa::kLongRow) return PSA_OK;
  const LongRows w = long_layout(workspace, nnz, H, F, partials);
  const int rc = psa::begin_long_rows(who, workspace, have, w.bytes, w.ctr, s);
  if (rc == PSA_OK) *lr = w;
  return rc;
}

// The checks every entry point begins with; the GAT forms pass K = 1 and their messages do not name it.
template <class Fmt>
int check_sizes(const char* who, bool gat, int dtype, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F,
                int64_t nnz, const float* bias, int64_t bias_heads) {
  if constexpr (Fmt::kTwoByte) ATTN_REQUIRE(dtype == PSA_BF16, "dtype must be PSA_BF16");
  ATTN_REQUIRE(M >= 0 && N >= 0 && nnz >= 0, "negative size");
  ATTN_REQUIRE(H >= 1 && K >= 1 && F >= 1, gat ? "H and F must be at least 1" : "H, K and F must be at least 1");
  ATTN_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  ATTN_REQUIRE(H < (int64_t{1} << 24) && K < (int64_t{1} << 24) && F < (int64_t{1} << 24),
               gat ? "H or F too large" : "H, K or F too large");
  ATTN_REQUIRE(bias == nullptr || bias_heads == 1 || bias_heads == H, "bias_heads must be 1 or H");
  return PSA_OK;
}

inline bool all_aligned(std::initializer_list<const void*> ps, size_t a) {
  for (const void* p : ps) {
    if (!psa::aligned(p, a)) return false;
  }
  return true;
}

// The pointers of a forward; x, y are q, k or a_row, a_col.
template <class Fmt>
int check_fw_pointers(const char* who, const int64_t* rowptr, const int64_t* col, const void* x, const void* y,
                      const void* v, int64_t nnz, const void* out, const float* stat) {
  ATTN_REQUIRE(rowptr && out && stat, "NULL pointer");
  ATTN_REQUIRE(nnz == 0 || (col && x && y && v), "NULL pointer");
  if constexpr (Fmt::kTwoByte) ATTN_REQUIRE(all_aligned({x, y, v, out}, 2), "operands must be 2-byte aligned");
  return PSA_OK;
}

template <class Fmt>
int check_bw_pointers(const char* who, const int64_t* rowptr, const int64_t* col, const void* x, const void* y,
                      const void* v, const void* grad_out, const void* out, const float* stat, const float* p,
                      const float* ds) {
  ATTN_REQUIRE(rowptr && col && x && y && v && grad_out && out && stat && p && ds, "NULL pointer");
  if constexpr (Fmt::kTwoByte) {
    ATTN_REQUIRE(all_aligned({x, y, v, grad_out, out}, 2), "operands must be 2-byte aligned");
  }
  return PSA_OK;
}

// The 16-byte form when the widths divide by it (K = 0: no K) and the operands start on 16 bytes, else 1.
template <class Fmt>
int vec_of(int64_t K, int64_t F, std::initializer_list<const void*> ps) {
  return (K % Fmt::kVec16 == 0) && (F % Fmt::kVec16 == 0) && all_aligned(ps, 16) ? Fmt::kVec16 : 1;
}

// What the four bodies set alike.
template <class A>
void set_common(A* a, const int64_t* rowptr, const int64_t* col, const void* v, const float* bias, int64_t bias_heads,
                int64_t M, int64_t H, int64_t F, int64_t nnz) {
  a->rowptr = rowptr;
  a->col = col;
  a->v = static_cast<const typename A::Fmt::elem_t*>(v);
  a->bias = bias;
  a->bias_heads = bias ? bias_heads : 1;
  a->M = M;
  a->H = H;
  a->F = F;
  a->nnz = nnz;
}

// The forward's aggregation: heads per block, lanes per entry and tiles of P * vec elements over Hb * F.
template <class A>
void fw_geometry(A* a, int vec) {
  a->Hb = head_block<typename A::Fmt>(a->H, a->F, vec);
  const int64_t Db = static_cast<int64_t>(a->Hb) * a->F;
  a->P = pow2_at_least(psa::ceil_div(Db, vec), 64, &a->shift);
  a->ntiles = static_cast<int>(psa::ceil_div(Db, static_cast<int64_t>(a->P) * vec));
}

template <class A, int VEC, int NR, int NT>
int launch_fw(const A& a, typename A::Fmt::elem_t* out, float* stat, const LongRows& lr, hipStream_t s) {
  const int64_t gx = psa::ceil_div(a.M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((attn_fw_kernel<A, VEC, NR, NT>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s, a, out,
                     stat, lr.ctr, lr.list);
  if (lr.list) {
    hipLaunchKernelGGL((attn_fw_chunk_kernel<A, VEC, NR, NT>), dim3(chunk_blocks(psa::max_long_chunks(a.nnz))),
                       dim3(kThreads), 0, s, a, lr.ctr, lr.list, lr.part, lr.pstat);
    float inv_keep = 1.f;
    if constexpr (A::kDrop) inv_keep = a.drop.inv_keep;
    hipLaunchKernelGGL((attn_fw_combine_kernel<typename A::Fmt, VEC, A::kDrop>),
                       dim3(chunk_blocks(psa::max_long_rows(a.nnz))), dim3(kThreads), 0, s, a.H, a.F, lr.ctr, lr.list,
                       lr.part, lr.pstat, out, stat, inv_keep);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

template <class A, int VEC, int NRK, int NRF>
int launch_bw(const A& a, const LongRows& lr, hipStream_t s) {
  const int64_t gx = psa::ceil_div(a.M, kWaves);
  PSA_REQUIRE(gx <= 0x7fffffff, "M too large for one launch");
  hipLaunchKernelGGL((attn_bw_kernel<A, VEC, NRK, NRF>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s, a,
                     lr.ctr, lr.list);
  if (lr.list) {
    hipLaunchKernelGGL((attn_bw_chunk_kernel<A, VEC, NRK, NRF>), dim3(chunk_blocks(psa::max_long_chunks(a.nnz))),
                       dim3(kThreads), 0, s, a, lr.ctr, lr.list);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

// NT = 1, 2 or 4 tiles per pass, as far as the form's budget goes; more tiles repeat the pass per NT of them.
template <class A, int VEC, int NR>
int dispatch_fw_nt(const A& a, typename A::Fmt::elem_t* out, float* stat, const LongRows& lr, hipStream_t s) {
  if (a.ntiles == 1) return launch_fw<A, VEC, NR, 1>(a, out, stat, lr, s);
  if constexpr (fw_tiles<typename A::Fmt>(VEC) == 2) {
    return launch_fw<A, VEC, NR, 2>(a, out, stat, lr, s);
  } else {
    if (a.ntiles == 2) return launch_fw<A, VEC, NR, 2>(a, out, stat, lr, s);
    return launch_fw<A, VEC, NR, 4>(a, out, stat, lr, s);
  }
}

// regs: the slices of q fit the registers (never for GAT, which has no q).
template <class A>
int dispatch_fw(const A& a, int vec, bool regs, typename A::Fmt::elem_t* out, float* stat, const LongRows& lr,
                hipStream_t s) {
  constexpr int W = A::Fmt::kVec16;
  constexpr int NR = A::kGat ? 0 : kMaxTiles;
  if (vec == W) {
    return regs ? dispatch_fw_nt<A, W, NR>(a, out, stat, lr, s) : dispatch_fw_nt<A, W, 0>(a, out, stat, lr, s);
  }
  return regs ? dispatch_fw_nt<A, 1, NR>(a, out, stat, lr, s) : dispatch_fw_nt<A, 1, 0>(a, out, stat, lr, s);
}

// rk, rf: the slices of q (never for GAT) and of grad_out fit the registers.
template <class A, int VEC>
int dispatch_bw_nr(const A& a, bool rk, bool rf, const LongRows& lr, hipStream_t s) {
  constexpr int NRK = A::kGat ? 0 : kMaxTiles;
  if (rk && rf) return launch_bw<A, VEC, NRK, kMaxTiles>(a, lr, s);
  if (rk) return launch_bw<A, VEC, NRK, 0>(a, lr, s);
  if (rf) return launch_bw<A, VEC, 0, kMaxTiles>(a, lr, s);
  return launch_bw<A, VEC, 0, 0>(a, lr, s);
}

template <class A>
int dispatch_bw(const A& a, int vec, bool rk, bool rf, const LongRows& lr, hipStream_t s) {
  if (vec == A::Fmt::kVec16) return dispatch_bw_nr<A, A::Fmt::kVec16>(a, rk, rf, lr, s);
  return dispatch_bw_nr<A, 1>(a, rk, rf, lr, s);
}

// dtype is looked at by the two-byte format alone.
template <class A>
int attention_fw(const char* who, const psa::Drop& drop, int dtype, const int64_t* rowptr, const int64_t* col,
                 const void* q, const void* k, const void* v, const float* bias, int64_t bias_heads, float scale,
                 int64_t M, int64_t N, int64_t H, int64_t K, int64_t F, int64_t nnz, void* out, float* stat,
                 void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  using Fmt = typename A::Fmt;
  using E = typename Fmt::elem_t;
  int rc = check_sizes<Fmt>(who, false, dtype, M, N, H, K, F, nnz, bias, bias_heads);
  if (rc != PSA_OK || M == 0) return rc;
  rc = check_fw_pointers<Fmt>(who, rowptr, col, q, k, v, nnz, out, stat);
  if (rc != PSA_OK) return rc;
  hipStream_t s = psa::as_stream(stream);
  LongRows lr;
  rc = take_long_rows(who, workspace, workspace_bytes, nnz, H, F, true, s, &lr);
  if (rc != PSA_OK) return rc;
  const int vec = vec_of<Fmt>(K, F, {q, k, v, out});
  A a;
  if constexpr (A::kDrop) a.drop = drop;
  set_common(&a, rowptr, col, v, bias, bias_heads, M, H, F, nnz);
  a.q = static_cast<const E*>(q);
  a.k = static_cast<const E*>(k);
  a.scale = scale;
  a.K = K;
  fw_geometry(&a, vec);
  a.dot = dot_geo(H, a.Hb, K, vec);
  return dispatch_fw(a, vec, a.dot.nit <= kMaxTiles, static_cast<E*>(out), stat, lr, s);
}

template <class A>
int attention_bw(const char* who, const psa::Drop& drop, int dtype, const int64_t* rowptr, const int64_t* col,
                 const void* q, const void* k, const void* v, const float* bias, int64_t bias_heads, float scale,
                 const void* grad_out, const void* out, const float* stat, int64_t M, int64_t N, int64_t H,
                 int64_t K, int64_t F, int64_t nnz, float* p, float* ds, void* workspace, size_t workspace_bytes,
                 psa_stream_t stream) {
  using Fmt = typename A::Fmt;
  using E = typename Fmt::elem_t;
  int rc = check_sizes<Fmt>(who, false, dtype, M, N, H, K, F, nnz, bias, bias_heads);
  if (rc != PSA_OK || M == 0 || nnz == 0) return rc;
  rc = check_bw_pointers<Fmt>(who, rowptr, col, q, k, v, grad_out, out, stat, p, ds);
  if (rc != PSA_OK) return rc;
  hipStream_t s = psa::as_stream(stream);
  LongRows lr;
  rc = take_long_rows(who, workspace, workspace_bytes, nnz, H, F, false, s, &lr);
  if (rc != PSA_OK) return rc;
  const int vec = vec_of<Fmt>(K, F, {q, k, v, grad_out, out});
  A a;
  if constexpr (A::kDrop) a.drop = drop;
  set_common(&a, rowptr, col, v, bias, bias_heads, M, H, F, nnz);
  a.q = static_cast<const E*>(q);
  a.k = static_cast<const E*>(k);
  a.scale = scale;
  a.K = K;
  a.grad_out = static_cast<const E*>(grad_out);
  a.out = static_cast<const E*>(out);
  a.stat = stat;
  a.Hb = static_cast<int>(H < kHeadBlock ? H : kHeadBlock);
  a.dot = dot_geo(H, a.Hb, K, vec);
  a.dotf = dot_geo(H, a.Hb, F, vec);
  a.p = p;
  a.ds = ds;
  return dispatch_bw(a, vec, a.dot.nit <= kMaxTiles, a.dotf.nit <= kMaxTiles, lr, s);
}

// ---- GAT: the same launches without the slices of q (NR = NRK = 0) --------------------------------

// Everything of the argument struct that the dot-product scores alone use.
template <class A>
void gat_no_dot(A* a) {
  a->q = nullptr;
  a->k = nullptr;
  a->scale = 1.f;
  a->K = 1;
  a->dot = DotGeo{};
}

template <class Fmt, bool DROP>
int gat_fw(const char* who, const psa::Drop& drop, int dtype, const int64_t* rowptr, const int64_t* col,
           const void* a_row, const void* a_col, const void* v, const float* bias, int64_t bias_heads, float slope,
           int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, void* out, float* stat, void* workspace,
           size_t workspace_bytes, psa_stream_t stream) {
  using A = GatFwArgs<Fmt, DROP>;
  using E = typename Fmt::elem_t;
  int rc = check_sizes<Fmt>(who, true, dtype, M, N, H, 1, F, nnz, bias, bias_heads);
  if (rc != PSA_OK) return rc;
  ATTN_REQUIRE(std::isfinite(slope), "negative_slope must be finite");
  if (M == 0) return PSA_OK;
  rc = check_fw_pointers<Fmt>(who, rowptr, col, a_row, a_col, v, nnz, out, stat);
  if (rc != PSA_OK) return rc;
  hipStream_t s = psa::as_stream(stream);
  LongRows lr;
  rc = take_long_rows(who, workspace, workspace_bytes, nnz, H, F, true, s, &lr);
  if (rc != PSA_OK) return rc;
  const int vec = vec_of<Fmt>(0, F, {v, out});
  A a;
  gat_no_dot(&a);
  a.drop = drop;
  set_common(&a, rowptr, col, v, bias, bias_heads, M, H, F, nnz);
  a.a_row = static_cast<const E*>(a_row);
  a.a_col = static_cast<const E*>(a_col);
  a.slope = slope;
  fw_geometry(&a, vec);
  return dispatch_fw(a, vec, false, static_cast<E*>(out), stat, lr, s);
}

template <class Fmt, bool DROP>
int gat_bw(const char* who, const psa::Drop& drop, int dtype, const int64_t* rowptr, const int64_t* col,
           const void* a_row, const void* a_col, const void* v, const float* bias, int64_t bias_heads, float slope,
           const void* grad_out, const void* out, const float* stat, int64_t M, int64_t N, int64_t H, int64_t F,
           int64_t nnz, float* p, float* dz, void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  using A = GatBwArgs<Fmt, DROP>;
  using E = typename Fmt::elem_t;
  int rc = check_sizes<Fmt>(who, true, dtype, M, N, H, 1, F, nnz, bias, bias_heads);
  if (rc != PSA_OK) return rc;
  ATTN_REQUIRE(std::isfinite(slope), "negative_slope must be finite");
  if (M == 0 || nnz == 0) return PSA_OK;
  rc = check_bw_pointers<Fmt>(who, rowptr, col, a_row, a_col, v, grad_out, out, stat, p, dz);
  if (rc != PSA_OK) return rc;
  hipStream_t s = psa::as_stream(stream);
  LongRows lr;
  rc = take_long_rows(who, workspace, workspace_bytes, nnz, H, F, false, s, &lr);
  if (rc != PSA_OK) return rc;
  const int vec = vec_of<Fmt>(0, F, {v, grad_out, out});
  A a;
  gat_no_dot(&a);
  a.drop = drop;
  set_common(&a, rowptr, col, v, bias, bias_heads, M, H, F, nnz);
  a.a_row = static_cast<const E*>(a_row);
  a.a_col = static_cast<const E*>(a_col);
  a.slope = slope;
  a.grad_out = static_cast<const E*>(grad_out);
  a.out = static_cast<const E*>(out);
  a.stat = stat;
  a.Hb = static_cast<int>(H < kHeadBlock ? H : kHeadBlock);
  a.dotf = dot_geo(H, a.Hb, F, vec);
  a.p = p;
  a.ds = dz;
  return dispatch_bw(a, vec, false, a.dotf.nit <= kMaxTiles, lr, s);
}

#undef ATTN_REQUIRE

}  // namespace
