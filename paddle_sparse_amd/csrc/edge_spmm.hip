// SpMM over per-entry feature vectors, fp32 and bf16, gfx950: the aggregation of the message-passing
// layers that carry edge features (CFConv / MPNN / CGConv: x_j * e_ij, u_add_e_sum: x_j + e_ij, GINE:
// relu(x_j + e_ij)), forward and both gradients, without the [nnz, K] intermediates of the unfused route.
//
//   m[e, :]   = x[col[e], :] (*, +, relu of +) edge[e, :]        edge [nnz, K] in CSR order
//   out[r, :] = sum of m[e, :] over the entries of row r         (mean: that sum / float(n_r); no entries: 0)
//
// There is no contraction in this op (every output element meets every input element once), so it is a
// pure stream: the [nnz, K] edge operand is read exactly once and is the dominant traffic, x[col] is a
// gather that lives in the caches.  The plan is spmm_multi.hip's gather with a second operand beside it:
//   * one wave owns one CSR row and is the only writer of its K outputs;
//   * col is read once per 64 entries, one per lane, and handed to the loop by cross-lane moves;
//   * LPR lanes x VEC elements cover a K tile (LPR = the power of two >= K / VEC, 4 <= LPR <= 64; VEC = 4
//     fp32 / 8 bf16: 16-byte accesses, K % VEC == 0 and 16-byte aligned operands; VEC = 1 otherwise, any
//     K >= 1 and any element alignment), G = 64 / LPR entries share a wave instruction and kU = 4 such steps
//     are issued before the first is consumed: 4 gathers of x AND the 4 loads of the edge slab they meet
//     are in flight together.  The G groups of one step read G consecutive edge rows, so with K = LPR * VEC
//     a step's edge load is one contiguous run of G * K elements.  Loads stay in their raw width (a 16-byte
//     register quad) until they are consumed; bf16 is widened there, exactly;
//   * K above one tile (256 fp32 / 512 bf16 elements, 64 in the element form) loops over tiles in the wave;
//   * every message and every sum is fp32; lane group g takes entries g, g + G, ... in that order and the
//     groups are folded with xor shuffles over the lane bits above LPR, lowest bit first: a fixed order;
//   * rows above psa::kLongRow entries go to the long_rows.h list: one wave per 128-entry chunk leaves an
//     fp32 partial row, one wave per listed row adds them IN CHUNK ORDER, divides for mean and rounds.
// All loads and stores are the ordinary cached kind: nothing here was measured to gain from another.
//
// grad_x runs the same three kernels over the CSC view (BW = true): one wave per column j, the gathered
// row is grad_out[row(e)] (times 1 / n of that row for mean), the edge row is edge[csr2csc[e']] (each read
// once, but through a permutation), and add_relu recomputes its mask from x[j] + edge: the forward saves
// nothing of nnz rows.  op = add needs no edge operand at all there and is the package's A^T g.
// grad_edge has no reduction: lane groups walk a flat range of entries (the COO row of the storage names
// the row of grad_out), so a hub row needs no path of its own, and stores are contiguous.
// No zero skipping (0 * inf = NaN), relu(NaN) = NaN, no float atomics, no host read: the bits repeat
// from run to run and every call can be captured.  Every address is formed in 64-bit arithmetic.
#include <type_traits>

#include "common.h"
#include "half_util.h"
#include "long_rows.h"
#include "vec_io.h"

namespace {

using psa::shfl_i64;
using psa_half::BF16;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kU = 4;               // steps of G entries in flight
constexpr int kMinShift = 2;        // LPR >= 4: G * kU <= 64, an entry batch divides the wave
constexpr int kChunkBlocks = 2048;  // capped grid of the chunk / combine launches: 8192 waves
constexpr int kEntryBlocks = 2048;  // capped grid of grad_edge: 524 288 lanes, grid-stride over the entries
// (the caps and the tile widths reach Python, and the second-trip test, through psa_edge_spmm_tile below)

enum { OP_MUL = 0, OP_ADD = 1, OP_ADD_RELU = 2 };

// ---- VEC elements of T (float, or the tag BF16) as they travel: raw until they are consumed ----
template <typename T>
constexpr int kElemBytes = std::is_same<T, float>::value ? 4 : 2;

template <typename T, int VEC>
struct Raw;
template <>
struct Raw<float, 1> {
  using type = float;
};
template <>
struct Raw<float, 4> {
  using type = float4;
};
template <>
struct Raw<BF16, 1> {
  using type = uint16_t;
};
template <>
struct Raw<BF16, 8> {
  using type = uint4;
};
template <typename T, int VEC>
using raw_t = typename Raw<T, VEC>::type;

template <typename T, int VEC>
__device__ __forceinline__ raw_t<T, VEC> zero_raw() {
  if constexpr (VEC == 1) return raw_t<T, VEC>(0);
  else if constexpr (std::is_same<T, float>::value) return make_float4(0.f, 0.f, 0.f, 0.f);
  else return make_uint4(0u, 0u, 0u, 0u);
}

template <typename T, int VEC>
__device__ __forceinline__ raw_t<T, VEC> load_raw(const void* base, int64_t elem) {
  return *reinterpret_cast<const raw_t<T, VEC>*>(static_cast<const char*>(base) + elem * kElemBytes<T>);
}

template <typename T, int VEC>
__device__ __forceinline__ void widen(const raw_t<T, VEC>& r, float (&f)[VEC]) {
  if constexpr (std::is_same<T, float>::value) {
    if constexpr (VEC == 4) {
      f[0] = r.x;
      f[1] = r.y;
      f[2] = r.z;
      f[3] = r.w;
    } else {
      f[0] = r;
    }
  } else {
    if constexpr (VEC == 8) psa_half::widen8<BF16>(r, f);
    else f[0] = __uint_as_float(static_cast<uint32_t>(r) << 16);
  }
}

// the one rounding of bf16 is here
template <typename T, int VEC>
__device__ __forceinline__ void store_elems(void* base, int64_t elem, const float (&f)[VEC]) {
  char* p = static_cast<char*>(base) + elem * kElemBytes<T>;
  if constexpr (std::is_same<T, float>::value) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    else *reinterpret_cast<float*>(p) = f[0];
  } else {
    if constexpr (VEC == 8) *reinterpret_cast<uint4*>(p) = psa_half::narrow8<BF16>(f);
    else *reinterpret_cast<uint16_t*>(p) = psa_half::narrow1<BF16>(f[0]);
  }
}

template <int OP>
__device__ __forceinline__ float message(float a, float b) {
  if constexpr (OP == OP_MUL) {
    return a * b;
  } else {
    const float v = a + b;
    if constexpr (OP == OP_ADD) return v;
    else return v > 0.f ? v : (v != v ? v : 0.f);  // a NaN stays a NaN
  }
}

struct Geo {
  int64_t K;
  int64_t ntiles;  // tiles of (1 << shift) * VEC elements over K
  int shift;       // log2(LPR)
};

// One reduction pass: the forward over the CSR rows, or grad_x over the CSC columns.
struct Pass {
  const int64_t* ptr;   // rowptr | colptr
  const int64_t* idx;   // the gathered row of every entry: col | row in CSC order
  const int64_t* perm;  // the edge row of every entry: NULL (the entry itself) | csr2csc
  const void* gath;     // x | grad_out
  const void* edge;
  const void* self;     // grad_x of add_relu: x, whose row j meets every entry of column j
  const float* scale;   // grad_x of mean: 1 / n of every row of grad_out, or NULL
  int64_t R;            // rows of the pass: M | N
  int64_t nnz;
  int mean;             // forward: divide the sum by n
  void* out;
};

// The sum over the entries [s, e) of row `owner` of the pass, for the K tile whose elements of this lane
// start at k0.  Every lane ends with the folded result of the elements it owns.
template <typename T, int VEC, int OP, bool BW>
__device__ __forceinline__ void edge_range(const Pass& p, const Geo& g, int64_t k0, bool kact, int64_t owner, int64_t s,
                                           int64_t e, int lane, float (&acc)[VEC]) {
  const int G = 64 >> g.shift;
  const int grp = lane >> g.shift;
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
  [[maybe_unused]] float self[VEC];
  if constexpr (BW && OP == OP_ADD_RELU) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) self[i] = 0.f;
    if (kact) widen<T, VEC>(load_raw<T, VEC>(p.self, owner * g.K + k0), self);
  }
  for (int64_t base = s; base < e; base += 64) {
    const int n = (e - base) < 64 ? static_cast<int>(e - base) : 64;
    int64_t c_l = 0;
    [[maybe_unused]] int64_t q_l = 0;
    [[maybe_unused]] float w_l = 1.f;
    if (lane < n) {
      c_l = p.idx[base + lane];
      if constexpr (BW) {
        q_l = p.perm[base + lane];
        if (p.scale) w_l = p.scale[c_l];
      }
    }
    for (int j = 0; j < n; j += G * kU) {  // G * kU divides 64: idx below stays under 64
      raw_t<T, VEC> a[kU], b[kU];
      [[maybe_unused]] float w[kU];
      bool ok[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int idx = j + u * G + grp;
        const int64_t c = shfl_i64(c_l, idx);
        int64_t q = base + idx;
        if constexpr (BW) {
          q = shfl_i64(q_l, idx);
          w[u] = __shfl(w_l, idx);
        }
        ok[u] = (idx < n) && kact;
        a[u] = zero_raw<T, VEC>();
        b[u] = zero_raw<T, VEC>();
        if (ok[u]) {
          a[u] = load_raw<T, VEC>(p.gath, c * g.K + k0);  // the gather
          b[u] = load_raw<T, VEC>(p.edge, q * g.K + k0);  // the stream
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (ok[u]) {
          float fa[VEC], fb[VEC];
          widen<T, VEC>(a[u], fa);
          widen<T, VEC>(b[u], fb);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            if constexpr (!BW) {
              acc[i] += message<OP>(fa[i], fb[i]);
            } else {
              const float ga = w[u] * fa[i];
              if constexpr (OP == OP_MUL) acc[i] += ga * fb[i];
              else acc[i] += (self[i] + fb[i] > 0.f) ? ga : 0.f;
            }
          }
        }
      }
    }
  }
  // fold the G lane groups, lowest lane bit above LPR first
  for (int off = 1 << g.shift; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
}

__device__ __forceinline__ void clamp_range(int64_t& s, int64_t& e, int64_t nnz) {
  s = s < 0 ? 0 : (s > nnz ? nnz : s);
  e = e < s ? s : (e > nnz ? nnz : e);
}

// One wave per row of the pass, every K tile of it.
template <typename T, int VEC, int OP, bool BW>
__global__ void __launch_bounds__(kThreads)
edge_row_kernel(const Pass p, const Geo g, unsigned long long* __restrict__ long_ctr,
                psa::LongEntry* __restrict__ long_list) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (row >= p.R) return;
  int64_t s = p.ptr[row], e = p.ptr[row + 1];
  clamp_range(s, e, p.nnz);
  if (long_list && e - s > psa::kLongRow) {  // wave-uniform: hand the row to chunk waves
    if (lane == 0) psa::push_long_row(long_ctr, long_list, row, e - s);
    return;
  }
  const int l = lane & ((1 << g.shift) - 1);
  for (int64_t t = 0; t < g.ntiles; ++t) {
    const int64_t k0 = ((t << g.shift) + l) * VEC;
    const bool kact = k0 < g.K;
    float acc[VEC];
    edge_range<T, VEC, OP, BW>(p, g, k0, kact, row, s, e, lane, acc);
    if ((lane >> g.shift) == 0 && kact) {
      if (p.mean) {
        const float d = static_cast<float>(e - s);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = e > s ? acc[i] / d : 0.f;
      }
      store_elems<T, VEC>(p.out, row * g.K + k0, acc);
    }
  }
}

// One wave per 128-entry chunk of a listed row: part[c, :] = the fp32 sum over the chunk.
template <typename T, int VEC, int OP, bool BW>
__global__ void __launch_bounds__(kThreads)
edge_chunk_kernel(const Pass p, const Geo g, const unsigned long long* __restrict__ long_ctr,
                  const psa::LongEntry* __restrict__ long_list, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ctr = *long_ctr;
  const uint32_t total = static_cast<uint32_t>(ctr & 0xffffffffull);
  const int nrows = static_cast<int>(ctr >> 32);
  const uint32_t num_waves = gridDim.x * kWaves;
  const int l = lane & ((1 << g.shift) - 1);
  for (uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6); c < total; c += num_waves) {
    const psa::LongEntry ent = psa::find_long_entry(long_list, nrows, c);
    int64_t rs = p.ptr[ent.row], re = p.ptr[ent.row + 1];
    clamp_range(rs, re, p.nnz);
    const int64_t s = rs + static_cast<int64_t>(c - ent.first_chunk) * psa::kLongChunk;
    const int64_t e = s + psa::kLongChunk < re ? s + psa::kLongChunk : re;
    for (int64_t t = 0; t < g.ntiles; ++t) {
      const int64_t k0 = ((t << g.shift) + l) * VEC;
      const bool kact = k0 < g.K;
      float acc[VEC];
      edge_range<T, VEC, OP, BW>(p, g, k0, kact, ent.row, s, e, lane, acc);
      if ((lane >> g.shift) == 0 && kact) {
        float* pf = part + static_cast<int64_t>(c) * g.K + k0;
#pragma unroll
        for (int i = 0; i < VEC; ++i) pf[i] = acc[i];
      }
    }
  }
}

// One wave per listed row, a lane per column: the chunks' partial rows added in chunk order.
template <typename T>
__global__ void __launch_bounds__(kThreads)
edge_combine_kernel(const int64_t* __restrict__ ptr, int64_t K, int64_t nnz, int mean,
                    const unsigned long long* __restrict__ long_ctr, const psa::LongEntry* __restrict__ long_list,
                    const float* __restrict__ part, void* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int nrows = static_cast<int>(*long_ctr >> 32);
  const int num_waves = static_cast<int>(gridDim.x) * kWaves;
  for (int slot = blockIdx.x * kWaves + (threadIdx.x >> 6); slot < nrows; slot += num_waves) {
    const psa::LongEntry ent = long_list[slot];
    int64_t rs = ptr[ent.row], re = ptr[ent.row + 1];
    clamp_range(rs, re, nnz);
    for (int64_t k = lane; k < K; k += 64) {
      float acc[1] = {0.f};
      for (uint32_t ch = 0; ch < ent.num_chunks; ++ch) acc[0] += part[(static_cast<int64_t>(ent.first_chunk) + ch) * K + k];
      if (mean) acc[0] = acc[0] / static_cast<float>(re - rs);  // a listed row has entries
      store_elems<T, 1>(out, ent.row * K + k, acc);
    }
  }
}

// grad_edge[e, :] = g[row[e], :] * x[col[e], :] (mul), g[row[e], :] (add), g[row[e], :] where
// x[col[e], :] + edge[e, :] > 0 (add_relu); g = grad_out, times scale[row[e]] for mean.  Groups of
// 1 << shift lanes take entries from the flat range, a capped grid strides over it.
template <typename T, int VEC, int OP>
__global__ void __launch_bounds__(kThreads)
edge_grad_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col, const void* __restrict__ grad,
                 const void* __restrict__ x, const void* __restrict__ edge, const float* __restrict__ scale, const Geo g,
                 int64_t nnz, void* __restrict__ out) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int l = static_cast<int>(tid & ((1 << g.shift) - 1));
  const int64_t groups = (static_cast<int64_t>(gridDim.x) * kThreads) >> g.shift;
  for (int64_t e = tid >> g.shift; e < nnz; e += groups) {
    const int64_t r = row[e];
    [[maybe_unused]] int64_t c = 0;
    if constexpr (OP != OP_ADD) c = col[e];
    const float w = scale ? scale[r] : 1.f;
    for (int64_t t = 0; t < g.ntiles; ++t) {
      const int64_t k0 = ((t << g.shift) + l) * VEC;
      if (k0 >= g.K) continue;
      float fg[VEC];
      widen<T, VEC>(load_raw<T, VEC>(grad, r * g.K + k0), fg);
      if constexpr (OP != OP_ADD) {
        float fx[VEC];
        widen<T, VEC>(load_raw<T, VEC>(x, c * g.K + k0), fx);
        if constexpr (OP == OP_MUL) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) fg[i] = (w * fg[i]) * fx[i];
        } else {
          float fe[VEC];
          widen<T, VEC>(load_raw<T, VEC>(edge, e * g.K + k0), fe);
#pragma unroll
          for (int i = 0; i < VEC; ++i) fg[i] = (fx[i] + fe[i] > 0.f) ? w * fg[i] : 0.f;
        }
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) fg[i] = w * fg[i];
      }
      store_elems<T, VEC>(out, e * g.K + k0, fg);
    }
  }
}

// PSA_REQUIRE for the helpers, which carry the entry point's name
int refuse(const char* who, const char* msg) {
  psa::set_error(std::string(who) + ": " + msg);
  return PSA_ERR_INVALID_ARG;
}

Geo geometry(int64_t K, int vec, int min_shift) {
  const int64_t q = psa::ceil_div(K, vec);
  int shift = min_shift;
  while ((1 << shift) < 64 && (int64_t{1} << shift) < q) ++shift;
  return Geo{K, psa::ceil_div(q, int64_t{1} << shift), shift};
}

template <typename T, int VEC, int OP, bool BW>
int launch_pass(const char* who, const Pass& p, const Geo& g, const psa::LongSums& w, hipStream_t s) {
  const int64_t gx = psa::ceil_div(p.R, kWaves);
  if (gx > 0x7fffffff) return refuse(who, "too many rows for one launch");
  hipLaunchKernelGGL((edge_row_kernel<T, VEC, OP, BW>), dim3(static_cast<unsigned>(gx)), dim3(kThreads), 0, s, p, g, w.ctr,
                     w.list);
  if (w.list) {
    int64_t cb = psa::ceil_div(psa::max_long_chunks(p.nnz), kWaves);
    cb = cb > kChunkBlocks ? kChunkBlocks : cb;
    int64_t rb = psa::ceil_div(psa::max_long_rows(p.nnz), kWaves);
    rb = rb > kChunkBlocks ? kChunkBlocks : rb;
    hipLaunchKernelGGL((edge_chunk_kernel<T, VEC, OP, BW>), dim3(static_cast<unsigned>(cb)), dim3(kThreads), 0, s, p, g,
                       w.ctr, w.list, w.part);
    hipLaunchKernelGGL((edge_combine_kernel<T>), dim3(static_cast<unsigned>(rb)), dim3(kThreads), 0, s, p.ptr, g.K, p.nnz,
                       p.mean, w.ctr, w.list, w.part, p.out);
  }
  return PSA_OK;  // the entry point asks for the launch error, under its own name
}

template <typename T, int VEC, bool BW>
int launch_op(const char* who, int op, const Pass& p, const Geo& g, const psa::LongSums& w, hipStream_t s) {
  if (op == OP_MUL) return launch_pass<T, VEC, OP_MUL, BW>(who, p, g, w, s);
  if constexpr (!BW) {
    if (op == OP_ADD) return launch_pass<T, VEC, OP_ADD, BW>(who, p, g, w, s);
  }
  return launch_pass<T, VEC, OP_ADD_RELU, BW>(who, p, g, w, s);
}

// 16-byte accesses when the width and every operand allow them
int vector_width(int dtype, int64_t K, std::initializer_list<const void*> operands) {
  const int vec = dtype == PSA_F32 ? 4 : 8;
  if (K % vec != 0) return 1;
  for (const void* q : operands)
    if (q != nullptr && !psa::aligned(q, 16)) return 1;
  return vec;
}

// the shared tail of the two reduction entry points
template <bool BW>
int run_pass(const char* who, int dtype, int op, Pass p, int64_t K, void* workspace, size_t workspace_bytes,
             hipStream_t s) {
  psa::LongSums w;
  // Long-row path: on when the caller brings a workspace (NULL keeps every row on its own wave: same
  // semantics, slow on power-law graphs; a caller that knows its longest row skips it).
  if (workspace != nullptr && p.nnz > psa::kLongRow) {
    w = psa::long_sums_layout(workspace, p.nnz, K);
    const int rc = psa::begin_long_rows(who, workspace, workspace_bytes, w.bytes, w.ctr, s);
    if (rc != PSA_OK) return rc;
    if (psa::max_long_chunks(p.nnz) >= (1ll << 32)) return refuse(who, "too many chunks");
  }
  const int vec = vector_width(dtype, K, {p.gath, p.edge, p.self, p.out});
  const Geo g = geometry(K, vec, kMinShift);
  if (dtype == PSA_F32)
    return vec == 4 ? launch_op<float, 4, BW>(who, op, p, g, w, s) : launch_op<float, 1, BW>(who, op, p, g, w, s);
  return vec == 8 ? launch_op<BF16, 8, BW>(who, op, p, g, w, s) : launch_op<BF16, 1, BW>(who, op, p, g, w, s);
}

template <typename T, int VEC>
void launch_grad(int op, const int64_t* row, const int64_t* col, const void* grad, const void* x, const void* edge,
                const float* scale, const Geo& g, int64_t nnz, void* out, hipStream_t s) {
  int64_t blocks = psa::ceil_div(nnz << g.shift, kThreads);
  blocks = blocks > kEntryBlocks ? kEntryBlocks : blocks;
  const dim3 grid(static_cast<unsigned>(blocks)), block(kThreads);
  if (op == OP_MUL)
    hipLaunchKernelGGL((edge_grad_kernel<T, VEC, OP_MUL>), grid, block, 0, s, row, col, grad, x, edge, scale, g, nnz, out);
  else if (op == OP_ADD)
    hipLaunchKernelGGL((edge_grad_kernel<T, VEC, OP_ADD>), grid, block, 0, s, row, col, grad, x, edge, scale, g, nnz, out);
  else
    hipLaunchKernelGGL((edge_grad_kernel<T, VEC, OP_ADD_RELU>), grid, block, 0, s, row, col, grad, x, edge, scale, g, nnz,
                       out);
}

}  // namespace

extern "C" {

int psa_edge_spmm(int dtype, int op, int mean, const int64_t* rowptr, const int64_t* col, const void* x,
                  const void* edge, int64_t M, int64_t N, int64_t K, int64_t nnz, void* out, void* workspace,
                  size_t workspace_bytes, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(op == OP_MUL || op == OP_ADD || op == OP_ADD_RELU, "unknown op");
  PSA_REQUIRE(mean == 0 || mean == 1, "mean must be 0 or 1");
  PSA_REQUIRE(M >= 0 && N >= 0 && K >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(K < (int64_t{1} << 24), "K too large");
  if (M == 0 || K == 0) return PSA_OK;
  PSA_REQUIRE(rowptr != nullptr, "rowptr is NULL");
  PSA_REQUIRE(out != nullptr, "out is NULL");
  PSA_REQUIRE(nnz == 0 || (col != nullptr && x != nullptr && edge != nullptr), "col/x/edge is NULL");
  // nnz == 0: the row waves find empty ranges and write the zeros
  const Pass p{rowptr, col, nullptr, x, edge, nullptr, nullptr, M, nnz, mean, out};
  const int rc = run_pass<false>(__func__, dtype, op, p, K, workspace, workspace_bytes, psa::as_stream(stream));
  if (rc != PSA_OK) return rc;
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_edge_spmm_bw_x(int dtype, int op, const int64_t* colptr, const int64_t* row_csc, const int64_t* csr2csc,
                       const void* grad_out, const void* edge, const void* x, const float* row_scale, int64_t M,
                       int64_t N, int64_t K, int64_t nnz, void* grad_x, void* workspace, size_t workspace_bytes,
                       psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(op == OP_MUL || op == OP_ADD_RELU,
              op == OP_ADD ? "op add is A^T grad_out: psa_spmm over the CSC view" : "unknown op");
  PSA_REQUIRE(M >= 0 && N >= 0 && K >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(K < (int64_t{1} << 24), "K too large");
  if (N == 0 || K == 0) return PSA_OK;
  PSA_REQUIRE(colptr != nullptr, "colptr is NULL");
  PSA_REQUIRE(grad_x != nullptr, "grad_x is NULL");
  PSA_REQUIRE(op != OP_ADD_RELU || x != nullptr, "x is NULL");
  PSA_REQUIRE(nnz == 0 || (row_csc != nullptr && csr2csc != nullptr && grad_out != nullptr && edge != nullptr),
              "row_csc/csr2csc/grad_out/edge is NULL");
  const Pass p{colptr, row_csc, csr2csc, grad_out, edge, op == OP_ADD_RELU ? x : nullptr, row_scale, N, nnz, 0, grad_x};
  const int rc = run_pass<true>(__func__, dtype, op, p, K, workspace, workspace_bytes, psa::as_stream(stream));
  if (rc != PSA_OK) return rc;
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_edge_spmm_bw_edge(int dtype, int op, const int64_t* row, const int64_t* col, const void* grad_out,
                          const void* x, const void* edge, const float* row_scale, int64_t M, int64_t N, int64_t K,
                          int64_t nnz, void* grad_edge, psa_stream_t stream) {
  PSA_REQUIRE(dtype == PSA_F32 || dtype == PSA_BF16, "dtype must be PSA_F32 or PSA_BF16");
  PSA_REQUIRE(op == OP_MUL || op == OP_ADD || op == OP_ADD_RELU, "unknown op");
  PSA_REQUIRE(M >= 0 && N >= 0 && K >= 0 && nnz >= 0, "negative size");
  PSA_REQUIRE(nnz < (int64_t{1} << 38), "nnz too large");
  PSA_REQUIRE(K < (int64_t{1} << 24), "K too large");
  if (nnz == 0 || K == 0) return PSA_OK;
  PSA_REQUIRE(row != nullptr && grad_out != nullptr && grad_edge != nullptr, "row/grad_out/grad_edge is NULL");
  PSA_REQUIRE(op == OP_ADD || (col != nullptr && x != nullptr), "col/x is NULL");
  PSA_REQUIRE(op != OP_ADD_RELU || edge != nullptr, "edge is NULL");
  const void* xs = op == OP_ADD ? nullptr : x;
  const void* es = op == OP_ADD_RELU ? edge : nullptr;
  const int vec = vector_width(dtype, K, {grad_out, xs, es, grad_edge});
  const Geo g = geometry(K, vec, 0);
  hipStream_t s = psa::as_stream(stream);
  if (dtype == PSA_F32) {
    if (vec == 4) launch_grad<float, 4>(op, row, col, grad_out, xs, es, row_scale, g, nnz, grad_edge, s);
    else launch_grad<float, 1>(op, row, col, grad_out, xs, es, row_scale, g, nnz, grad_edge, s);
  } else {
    if (vec == 8) launch_grad<BF16, 8>(op, row, col, grad_out, xs, es, row_scale, g, nnz, grad_edge, s);
    else launch_grad<BF16, 1>(op, row, col, grad_out, xs, es, row_scale, g, nnz, grad_edge, s);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_edge_spmm_tile(int* chunk_waves, int* entry_lanes, int* tile_f32, int* tile_bf16) {
  PSA_REQUIRE(chunk_waves && entry_lanes && tile_f32 && tile_bf16, "NULL output");
  *chunk_waves = kChunkBlocks * kWaves;
  *entry_lanes = kEntryBlocks * kThreads;
  *tile_f32 = 64 * 4;
  *tile_bf16 = 64 * 8;
  return PSA_OK;
}

}  // extern "C"
