// Segmented softmax over stored values, forward and backward, fp32, gfx950.
//
//   forward   out[j,h] = exp(src[j,h] - m[s,h]) / sum_{j' in s} exp(src[j',h] - m[s,h])
//   backward  grad_src[j,h] = y[j,h] * (g[j,h] - sum_{j' in s} y[j',h] * g[j',h])
//
// for every segment s of indptr and every one of the D columns ("heads") of the
// [n, D] row-major value array; with perm, position j of the segment order is row
// perm[j] of the arrays (dim = 0 of a CSR matrix runs over colptr / csr2csc).
//
// Lane mapping.  P = the power of two >= min(D, 64).  A group of W lanes (W = 8 .. 64, a
// power of two >= P, chosen on the host from the mean segment length) owns one segment:
// lane l of the group sits on head l % P of entry l / P, E = W / P entries per step.
// For D | 64 that is the contiguous run of W floats of the segment per step; other D leave
// P - D lanes of every entry idle (D < 64) or walk the heads in tiles of 64 (D > 64).  Per
// head the group folds with xor shuffles over the lane bits above P, so every lane of
// the group ends with the same bits.  Loads and stores are 4 bytes per lane: no
// alignment beyond the element's is asked of any array.
//
// A segment of up to kCache steps (128 entries for D <= 8 at W = 64) is read once and
// kept in registers; longer ones are streamed again from the caches (max, sum, write).
//
// Segments above psa::kLongRow entries leave their group: the long_rows.h list names
// them, one wave per 128-entry chunk leaves a partial {max, sum} (backward: a partial
// dot) per head, one wave per listed segment folds the chunks' partials in chunk order
// (lane by lane, then the xor tree: a fixed order, whatever order the list was built
// in), and a last launch of chunk waves writes the entries.  No floating-point atomics
// and no host read anywhere: the bits repeat from run to run and the calls can be
// captured into a graph.
//
// Non-finite values follow torch.softmax on the dense row by plain IEEE arithmetic:
// fmaxf drops a NaN, but that entry's exp(NaN - m) poisons the sum; +inf gives inf - inf;
// a group of nothing but -inf has m = -inf and x - m = NaN; -inf among finite entries
// gives exp(-inf) = 0 exactly.  exp is expf (within 1 ulp), never the fast intrinsic.
#include "common.h"
#include "long_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCache = 16;          // steps of a segment kept in registers
constexpr int kChunkWaves = kThreads / 64;
constexpr int kMaxChunkBlocks = 4096;

struct Part {
  float m;  // forward: the maximum (NaN dropped); backward: unused
  float s;  // forward: sum of exp(x - m), m read as 0 when it is -inf; backward: the dot
};

struct Geo {
  int64_t D;
  int P;       // lanes per entry
  int shift;   // log2(P)
};

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

template <bool BW>
__device__ __forceinline__ Part identity() {
  Part p;
  p.m = BW ? 0.f : neg_inf();
  p.s = 0.f;
  return p;
}

// Commutative bit for bit (no contraction), so that both partners of an xor step agree.
template <bool BW>
__device__ __forceinline__ Part merge(const Part a, const Part b) {
  Part r;
  if constexpr (BW) {
    r.m = 0.f;
    r.s = __fadd_rn(a.s, b.s);
  } else {
    r.m = fmaxf(a.m, b.m);
    const float fa = a.m == r.m ? 1.f : expf(a.m - r.m);
    const float fb = b.m == r.m ? 1.f : expf(b.m - r.m);
    r.s = __fadd_rn(__fmul_rn(a.s, fa), __fmul_rn(b.s, fb));
  }
  return r;
}

template <int W, bool BW>
__device__ __forceinline__ Part group_fold(Part p, int P) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) {
    if (off >= P) {  // group-uniform
      Part o;
      o.m = __shfl_xor(p.m, off);
      o.s = __shfl_xor(p.s, off);
      p = merge<BW>(p, o);
    }
  }
  return p;
}

__device__ __forceinline__ float safe_max(float m) { return m == neg_inf() ? 0.f : m; }

// Partial of positions [cs, ce) for head h, streamed (the second forward pass hits the caches).
// Every lane of the group calls it; lanes without a head or an entry add nothing.
template <int W, bool BW>
__device__ __forceinline__ Part range_partial(const float* __restrict__ a, const float* __restrict__ b,
                                              const int64_t* __restrict__ perm, const Geo g, int64_t h, bool hact,
                                              int e0, int E, int64_t cs, int64_t ce) {
  Part p = identity<BW>();
  if constexpr (BW) {
    float d = 0.f;
    if (hact) {
      for (int64_t j = cs + e0; j < ce; j += E) {
        const int64_t r = perm ? perm[j] : j;
        d += a[r * g.D + h] * b[r * g.D + h];
      }
    }
    p.s = d;
  } else {
    float m = neg_inf();
    if (hact) {
      for (int64_t j = cs + e0; j < ce; j += E) {
        const int64_t r = perm ? perm[j] : j;
        m = fmaxf(m, a[r * g.D + h]);
      }
    }
    // the group's maximum first: every lane then sums against the same reference
    {
      Part t;
      t.m = m;
      t.s = 0.f;
#pragma unroll
      for (int off = W / 2; off >= 1; off >>= 1) {
        if (off >= g.P) t.m = fmaxf(t.m, __shfl_xor(t.m, off));
      }
      m = t.m;
    }
    const float ref = safe_max(m);
    float sum = 0.f;
    if (hact) {
      for (int64_t j = cs + e0; j < ce; j += E) {
        const int64_t r = perm ? perm[j] : j;
        sum += expf(a[r * g.D + h] - ref);
      }
    }
    p.m = m;
    p.s = sum;
  }
  return p;
}

// Plain sum of the lanes' parts for the forward (all share p.m already), merge for the backward.
template <int W, bool BW>
__device__ __forceinline__ Part finish_partial(Part p, int P) {
  if constexpr (BW) {
    return group_fold<W, true>(p, P);
  } else {
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
      if (off >= P) p.s = __fadd_rn(p.s, __shfl_xor(p.s, off));
    }
    return p;
  }
}

// Entries [cs, ce) of head h from the segment's folded {m, s}.
template <bool BW>
__device__ __forceinline__ void write_range(const float* __restrict__ a, const float* __restrict__ b,
                                            const int64_t* __restrict__ perm, const Geo g, int64_t h, int e0, int E,
                                            int64_t cs, int64_t ce, const Part tot, float* __restrict__ out) {
  for (int64_t j = cs + e0; j < ce; j += E) {
    const int64_t r = perm ? perm[j] : j;
    const int64_t at = r * g.D + h;
    if constexpr (BW) out[at] = a[at] * (b[at] - tot.s);
    else out[at] = expf(a[at] - tot.m) / tot.s;
  }
}

// One group of W lanes per segment; segments above kLongRow entries are skipped when the
// long-segment launches follow (skip_long).
template <int W, bool BW>
__global__ void __launch_bounds__(kThreads)
softmax_group_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ perm,
                     const int64_t* __restrict__ indptr, int64_t nseg, int64_t n, const Geo g, int skip_long,
                     float* __restrict__ out) {
  const int64_t seg = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) / W;
  if (seg >= nseg) return;  // group-uniform
  const int lig = threadIdx.x & (W - 1);
  const int e0 = lig >> g.shift;
  const int hl = lig & (g.P - 1);
  const int E = W >> g.shift;
  int64_t s = indptr[seg], e = indptr[seg + 1];
  s = s < 0 ? 0 : s;
  e = e > n ? n : e;  // never past the arrays, whatever indptr holds
  const int64_t len = e - s;
  if (len <= 0 || (skip_long && len > psa::kLongRow)) return;
  const int64_t steps = (len + E - 1) / E;
  for (int64_t h0 = 0; h0 < g.D; h0 += g.P) {
    const int64_t h = h0 + hl;
    const bool hact = h < g.D;
    if (steps <= kCache) {
      float va[kCache], vb[kCache];
      Part p = identity<BW>();
#pragma unroll
      for (int i = 0; i < kCache; ++i) {
        const int64_t j = s + e0 + static_cast<int64_t>(i) * E;
        va[i] = BW ? 0.f : neg_inf();
        vb[i] = 0.f;
        if (hact && j < e) {
          const int64_t r = perm ? perm[j] : j;
          va[i] = a[r * g.D + h];
          if constexpr (BW) vb[i] = b[r * g.D + h];
        }
        if constexpr (BW) p.s += va[i] * vb[i];
        else p.m = fmaxf(p.m, va[i]);
      }
      if constexpr (!BW) {
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) {
          if (off >= g.P) p.m = fmaxf(p.m, __shfl_xor(p.m, off));
        }
#pragma unroll
        for (int i = 0; i < kCache; ++i) {
          const int64_t j = s + e0 + static_cast<int64_t>(i) * E;
          if (hact && j < e) {
            // against the true maximum (the whole segment is here: no partial to merge later): a group of
            // nothing but -inf gets its NaN from -inf - -inf
            va[i] = expf(va[i] - p.m);
            p.s += va[i];
          }
        }
      }
      p = finish_partial<W, BW>(p, g.P);
#pragma unroll
      for (int i = 0; i < kCache; ++i) {
        const int64_t j = s + e0 + static_cast<int64_t>(i) * E;
        if (hact && j < e) {
          const int64_t r = perm ? perm[j] : j;
          out[r * g.D + h] = BW ? va[i] * (vb[i] - p.s) : va[i] / p.s;
        }
      }
    } else {
      Part p = range_partial<W, BW>(a, b, perm, g, h, hact, e0, E, s, e);
      p = finish_partial<W, BW>(p, g.P);
      if (hact) write_range<BW>(a, b, perm, g, h, e0, E, s, e, p, out);
    }
  }
}

// Slot of the list entry owning chunk c: the largest slot with first_chunk <= c.
__device__ __forceinline__ int find_slot(const psa::LongEntry* __restrict__ list, int nrows, uint32_t c) {
  int lo = 0, hi = nrows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (list[mid].first_chunk <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct ChunkRange {
  int slot;
  int64_t cs, ce;
};

__device__ __forceinline__ ChunkRange chunk_range(const int64_t* __restrict__ indptr, int64_t n,
                                                  const psa::LongEntry* __restrict__ list, int nrows, uint32_t c) {
  ChunkRange cr;
  cr.slot = find_slot(list, nrows, c);
  const psa::LongEntry ent = list[cr.slot];
  int64_t rs = indptr[ent.row], re = indptr[ent.row + 1];
  rs = rs < 0 ? 0 : rs;
  re = re > n ? n : re;
  cr.cs = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
  cr.ce = cr.cs + psa::kLongChunk < re ? cr.cs + psa::kLongChunk : re;
  return cr;
}

// One wave per 128-entry chunk of a listed segment: part[c, h].
template <bool BW>
__global__ void __launch_bounds__(kThreads)
softmax_chunk_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ perm,
                     const int64_t* __restrict__ indptr, int64_t n, const Geo g,
                     const unsigned long long* __restrict__ ctr, const psa::LongEntry* __restrict__ list,
                     Part* __restrict__ part) {
  const unsigned long long cv = *ctr;
  const uint32_t total = static_cast<uint32_t>(cv & 0xffffffffull);
  const int nrows = static_cast<int>(cv >> 32);
  const int lane = threadIdx.x & 63;
  const int e0 = lane >> g.shift, hl = lane & (g.P - 1), E = 64 >> g.shift;
  const uint32_t num_waves = gridDim.x * kChunkWaves;
  for (uint32_t c = blockIdx.x * kChunkWaves + (threadIdx.x >> 6); c < total; c += num_waves) {
    const ChunkRange cr = chunk_range(indptr, n, list, nrows, c);
    for (int64_t h0 = 0; h0 < g.D; h0 += g.P) {
      const int64_t h = h0 + hl;
      const bool hact = h < g.D;
      Part p = range_partial<64, BW>(a, b, perm, g, h, hact, e0, E, cr.cs, cr.ce);
      p = finish_partial<64, BW>(p, g.P);
      if (hact && e0 == 0) part[static_cast<int64_t>(c) * g.D + h] = p;
    }
  }
}

// One wave per listed segment: its chunks' partials in chunk order -> fin[slot, h].
template <bool BW>
__global__ void __launch_bounds__(kThreads)
softmax_combine_kernel(const Geo g, const unsigned long long* __restrict__ ctr,
                       const psa::LongEntry* __restrict__ list, const Part* __restrict__ part,
                       Part* __restrict__ fin) {
  const int nrows = static_cast<int>(*ctr >> 32);
  const int lane = threadIdx.x & 63;
  const int e0 = lane >> g.shift, hl = lane & (g.P - 1), E = 64 >> g.shift;
  const int num_waves = static_cast<int>(gridDim.x) * kChunkWaves;
  for (int slot = blockIdx.x * kChunkWaves + (threadIdx.x >> 6); slot < nrows; slot += num_waves) {
    const psa::LongEntry ent = list[slot];
    for (int64_t h0 = 0; h0 < g.D; h0 += g.P) {
      const int64_t h = h0 + hl;
      const bool hact = h < g.D;
      Part p = identity<BW>();
      if (hact) {
        for (uint32_t k = e0; k < ent.num_chunks; k += E)
          p = merge<BW>(p, part[static_cast<int64_t>(ent.first_chunk + k) * g.D + h]);
      }
      p = group_fold<64, BW>(p, g.P);
      if (hact && e0 == 0) fin[static_cast<int64_t>(slot) * g.D + h] = p;
    }
  }
}

// One wave per chunk again: the entries, from the segment's folded partial.
template <bool BW>
__global__ void __launch_bounds__(kThreads)
softmax_write_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ perm,
                     const int64_t* __restrict__ indptr, int64_t n, const Geo g,
                     const unsigned long long* __restrict__ ctr, const psa::LongEntry* __restrict__ list,
                     const Part* __restrict__ fin, float* __restrict__ out) {
  const unsigned long long cv = *ctr;
  const uint32_t total = static_cast<uint32_t>(cv & 0xffffffffull);
  const int nrows = static_cast<int>(cv >> 32);
  const int lane = threadIdx.x & 63;
  const int e0 = lane >> g.shift, hl = lane & (g.P - 1), E = 64 >> g.shift;
  const uint32_t num_waves = gridDim.x * kChunkWaves;
  for (uint32_t c = blockIdx.x * kChunkWaves + (threadIdx.x >> 6); c < total; c += num_waves) {
    const ChunkRange cr = chunk_range(indptr, n, list, nrows, c);
    for (int64_t h0 = 0; h0 < g.D; h0 += g.P) {
      const int64_t h = h0 + hl;
      if (h < g.D)
        write_range<BW>(a, b, perm, g, h, e0, E, cr.cs, cr.ce, fin[static_cast<int64_t>(cr.slot) * g.D + h], out);
    }
  }
}

// {list, the chunks' partials [chunks, D], the long segments' folded partials [long rows, D]}
struct LongScratch : psa::LongList {
  Part* part = nullptr;
  Part* fin = nullptr;
  size_t bytes = 0;
};

LongScratch long_layout(void* workspace, int64_t n, int64_t D) {
  psa::Carver c(workspace);
  LongScratch w;
  psa::take_long_list(c, n, &w);
  w.part = psa::take_long_chunks<Part>(c, n, D);
  w.fin = c.take<Part>(static_cast<size_t>(psa::max_long_rows(n)) * static_cast<size_t>(D), 256);
  w.bytes = c.off;
  return w;
}

template <int W, bool BW>
void launch_groups(const float* a, const float* b, const int64_t* perm, const int64_t* indptr, int64_t nseg,
                   int64_t n, const Geo g, int skip_long, float* out, int64_t blocks, hipStream_t s) {
  hipLaunchKernelGGL((softmax_group_kernel<W, BW>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, a, b,
                     perm, indptr, nseg, n, g, skip_long, out);
}

template <bool BW>
int run(const char* who, const float* a, const float* b, const int64_t* perm, const int64_t* indptr, int64_t nseg,
        int64_t D, int64_t n, float* out, void* workspace, size_t ws_bytes, hipStream_t s) {
  Geo g;
  g.D = D;
  g.P = 1;
  g.shift = 0;
  while (g.P < 64 && g.P < D) {
    g.P <<= 1;
    ++g.shift;
  }
  // lanes per segment: enough for the mean segment in one step, at least 8, at most the wave
  const int64_t mean_len = psa::ceil_div(n, nseg);
  int W = g.P < 8 ? 8 : g.P;
  while (W < 64 && W / g.P < mean_len) W <<= 1;
  const int64_t blocks = psa::ceil_div(nseg, kThreads / W);
  if (blocks > 0x7fffffff) {
    psa::set_error(std::string(who) + ": too many segments for one launch");
    return PSA_ERR_INVALID_ARG;
  }
  const bool longs = n > psa::kLongRow;
  LongScratch w;
  if (longs) {
    w = long_layout(workspace, n, D);
    const int rc = psa::begin_long_rows(who, workspace, ws_bytes, w.bytes, w.ctr, s);
    if (rc != PSA_OK) return rc;
    hipLaunchKernelGGL(psa::find_long_rows_kernel,
                       dim3(static_cast<unsigned>(psa::ceil_div(nseg, psa::kFindThreads * psa::kFindIters))),
                       dim3(psa::kFindThreads), 0, s, indptr, nseg, w.ctr, w.list);
  }
  const int skip = longs ? 1 : 0;
  switch (W) {
    case 8: launch_groups<8, BW>(a, b, perm, indptr, nseg, n, g, skip, out, blocks, s); break;
    case 16: launch_groups<16, BW>(a, b, perm, indptr, nseg, n, g, skip, out, blocks, s); break;
    case 32: launch_groups<32, BW>(a, b, perm, indptr, nseg, n, g, skip, out, blocks, s); break;
    default: launch_groups<64, BW>(a, b, perm, indptr, nseg, n, g, skip, out, blocks, s); break;
  }
  if (longs) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(n), kChunkWaves);
    cb = cb > kMaxChunkBlocks ? kMaxChunkBlocks : cb;
    int64_t rb = psa::ceil_div(psa::max_long_rows(n), kChunkWaves);
    rb = rb > kMaxChunkBlocks ? kMaxChunkBlocks : rb;
    hipLaunchKernelGGL((softmax_chunk_kernel<BW>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, s, a, b, perm,
                       indptr, n, g, w.ctr, w.list, w.part);
    hipLaunchKernelGGL((softmax_combine_kernel<BW>), dim3(static_cast<unsigned>(rb)), dim3(kThreads), 0, s, g, w.ctr,
                       w.list, w.part, w.fin);
    hipLaunchKernelGGL((softmax_write_kernel<BW>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, s, a, b, perm,
                       indptr, n, g, w.ctr, w.list, w.fin, out);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // namespace

extern "C" {

size_t psa_segment_softmax_workspace_bytes(int64_t n, int64_t D) {
  if (n <= psa::kLongRow || D <= 0) return 0;  // no segment can be long
  return long_layout(nullptr, n, D).bytes;
}

int psa_segment_softmax(const float* src, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t D,
                        int64_t n, float* out, void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  PSA_REQUIRE(nseg >= 0 && D >= 0 && n >= 0, "negative size");
  if (nseg == 0 || n == 0 || D == 0) return PSA_OK;
  PSA_REQUIRE(src != nullptr && indptr != nullptr && out != nullptr, "NULL pointer");
  PSA_REQUIRE(n < (int64_t{1} << 38), "n too large");
  return run<false>("psa_segment_softmax", src, nullptr, perm, indptr, nseg, D, n, out, workspace, workspace_bytes,
                    psa::as_stream(stream));
}

int psa_segment_softmax_bw(const float* y, const float* grad, const int64_t* perm, const int64_t* indptr,
                           int64_t nseg, int64_t D, int64_t n, float* grad_src, void* workspace,
                           size_t workspace_bytes, psa_stream_t stream) {
  PSA_REQUIRE(nseg >= 0 && D >= 0 && n >= 0, "negative size");
  if (nseg == 0 || n == 0 || D == 0) return PSA_OK;
  PSA_REQUIRE(y != nullptr && grad != nullptr && indptr != nullptr && grad_src != nullptr, "NULL pointer");
  PSA_REQUIRE(n < (int64_t{1} << 38), "n too large");
  return run<true>("psa_segment_softmax_bw", y, grad, perm, indptr, nseg, D, n, grad_src, workspace, workspace_bytes,
                   psa::as_stream(stream));
}

}  // extern "C"
