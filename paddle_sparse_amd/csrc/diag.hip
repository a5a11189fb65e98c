// Diagonal ops of a sorted CSR matrix for gfx950: remove_diag / set_diag /
// fill_diag (count pass -> count2ptr -> write pass) and get_diag.
//
// "The k-th diagonal" is the set of cells (r, r + k) inside the M x N matrix.
// Every row touches at most one diagonal cell, so the count pass is one lane
// per row with no atomics: a binary search of the row's sorted columns gives
// the first diagonal entry and their number (duplicates included).  The write
// pass is balanced by OUTPUT entries: a workgroup owns a fixed tile of the
// output, finds the rows the tile spans by a 64-ary wave search in the new
// rowptr, stages those rows' pointers in LDS (as ptr2ind_kernel does in
// convert.hip) and maps every output slot to its source entry or to the
// inserted diagonal value.  A hub row is split over as many tiles as it
// needs; no lane walks more than kPer entries.  Values move as opaque rows of
// `row_bytes` (16-byte pieces when the alignment allows), so every dtype and
// trailing shape takes the same kernels.
#include <initializer_list>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                   // output entries per lane in the write pass
constexpr int kTile = kThreads * kPer;    // output entries per workgroup
constexpr int kRows = 512;                // rows of a tile staged in LDS

struct alignas(16) B16 {
  uint64_t x, y;
};

__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t upper_bound(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool on_diag(int64_t r, int64_t M, int64_t N, int64_t k) {
  const int64_t c = r + k;
  return r >= 0 && r < M && c >= 0 && c < N;
}

// Largest r in [lo, hi) with ptr[r] <= p, given ptr[lo] <= p; called by a whole
// wave (64 probes per step: 4 dependent loads for 2^24 rows).
__device__ __forceinline__ int64_t wave_search(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t p) {
  const int lane = threadIdx.x & 63;
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t x = lo + lane * step;
    const bool ok = x < hi && ptr[x] <= p;
    const int cnt = __popcll(__ballot(ok));  // lanes [0, cnt) hold: ptr is non-decreasing
    const int64_t nhi = lo + cnt * step;
    lo += (cnt - 1) * step;
    hi = nhi < hi ? nhi : hi;
  }
  return lo;
}

// One lane per j in [0, max(M, N)): row j's diagonal entries [dpos[j], dpos[j] + cnt)
// and its new length; with colcount given, column j's count adjusted for row j - k
// (the only row that touches it).  Rows off the diagonal get dpos = their end.
__global__ void __launch_bounds__(kThreads)
diag_count_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t M, int64_t N,
                  int64_t k, int insert, const int64_t* __restrict__ colcount, int64_t* __restrict__ rowcount_out,
                  int64_t* __restrict__ colcount_out, int64_t* __restrict__ dpos) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (j < M) {
    const int64_t s = rowptr[j], e = rowptr[j + 1];
    int64_t lb = e, ub = e;
    const bool on = on_diag(j, M, N, k);
    if (on) {
      lb = lower_bound(col, s, e, j + k);
      ub = upper_bound(col, lb, e, j + k);
    }
    dpos[j] = lb;
    rowcount_out[j] = (e - s) - (ub - lb) + (insert && on ? 1 : 0);
  }
  if (colcount != nullptr && j < N) {
    const int64_t r = j - k;
    int64_t delta = 0;
    if (on_diag(r, M, N, k)) {
      const int64_t s = rowptr[r], e = rowptr[r + 1];
      const int64_t lb = lower_bound(col, s, e, j);
      delta = (insert ? 1 : 0) - (upper_bound(col, lb, e, j) - lb);
    }
    colcount_out[j] = colcount[j] + delta;
  }
}

struct RowMap {
  int64_t optr;  // first output slot of the row
  int64_t s;     // first input entry of the row
  int64_t a;     // entries kept before the diagonal
  int64_t d;     // input offset of the kept tail: src = s + q + d for q >= a + ins
};

__device__ __forceinline__ RowMap row_map(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rowptr_out,
                                          const int64_t* __restrict__ dpos, int64_t r, bool ins) {
  RowMap m;
  m.optr = rowptr_out[r];
  m.s = rowptr[r];
  const int64_t e = rowptr[r + 1];
  const int64_t olen = rowptr_out[r + 1] - m.optr;
  const int64_t dcnt = (e - m.s) - olen + (ins ? 1 : 0);
  m.a = dpos[r] - m.s;
  m.d = dcnt - (ins ? 1 : 0);
  return m;
}

// Output tile [p0, p0 + kTile): col_out, the gradient maps, then the value rows
// (chunks pieces of T each) through the per-slot source kept in LDS.
// src >= 0: input entry; src < 0: inserted value -1 - src (index along the diagonal).
template <typename T>
__global__ void __launch_bounds__(kThreads)
diag_write_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, const T* __restrict__ value,
                  int64_t chunks, int shift, const T* __restrict__ diag_values, int64_t M, int64_t N, int64_t k,
                  int insert, const int64_t* __restrict__ rowptr_out, int64_t nnz_out,
                  const int64_t* __restrict__ dpos, int64_t* __restrict__ col_out, T* __restrict__ value_out,
                  int64_t* __restrict__ out_pos, int64_t* __restrict__ diag_pos) {
  __shared__ int64_t s_optr[kRows + 1];
  __shared__ int64_t s_s[kRows], s_a[kRows], s_d[kRows];
  __shared__ int64_t s_src[kTile];
  __shared__ int64_t s_bounds[2];
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const int64_t p1 = nnz_out - p0 < kTile ? nnz_out : p0 + kTile;
  const int wave = threadIdx.x >> 6;
  if (wave < 2) {  // rows of the tile's first and last slot
    const int64_t r = wave_search(rowptr_out, 0, M, wave == 0 ? p0 : p1 - 1);
    if ((threadIdx.x & 63) == 0) s_bounds[wave] = r;
  }
  __syncthreads();
  const int64_t r_lo = s_bounds[0], r_hi = s_bounds[1];
  const int64_t nr = r_hi - r_lo + 1;
  const bool staged = nr <= kRows;  // else: a run of empty rows; search rowptr_out in global memory
  if (staged) {
    for (int i = threadIdx.x; i <= nr; i += kThreads) {
      const int64_t r = r_lo + i;
      if (i == nr) {
        s_optr[i] = rowptr_out[r];
      } else {
        const RowMap m = row_map(rowptr, rowptr_out, dpos, r, insert && on_diag(r, M, N, k));
        s_optr[i] = m.optr;
        s_s[i] = m.s;
        s_a[i] = m.a;
        s_d[i] = m.d;
      }
    }
  }
  __syncthreads();
  const int64_t start = k < 0 ? -k : 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int li = j * kThreads + threadIdx.x;
    const int64_t p = p0 + li;
    if (p >= p1) break;
    int64_t r;
    RowMap m;
    if (staged) {
      int lo = 0, hi = static_cast<int>(nr);  // largest i with s_optr[i] <= p
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_optr[mid] <= p) lo = mid;
        else hi = mid;
      }
      r = r_lo + lo;
      m.optr = s_optr[lo];
      m.s = s_s[lo];
      m.a = s_a[lo];
      m.d = s_d[lo];
    } else {
      r = upper_bound(rowptr_out, r_lo, r_hi + 1, p) - 1;
      m = row_map(rowptr, rowptr_out, dpos, r, insert && on_diag(r, M, N, k));
    }
    const bool ins = insert && on_diag(r, M, N, k);
    const int64_t q = p - m.optr;
    int64_t src;
    if (q < m.a) src = m.s + q;
    else if (ins && q == m.a) src = -1 - (r - start);
    else src = m.s + q + m.d;
    if (src >= 0) {
      col_out[p] = col[src];
      if (out_pos != nullptr) out_pos[src] = p;
    } else {
      col_out[p] = r + k;
      if (diag_pos != nullptr) diag_pos[-1 - src] = p;
    }
    s_src[li] = src;
  }
  if (value_out == nullptr) return;  // block-uniform
  __syncthreads();
  const int64_t total = (p1 - p0) * chunks;
  for (int64_t g = threadIdx.x; g < total; g += kThreads) {
    int64_t i, c;
    if (shift >= 0) {
      i = g >> shift;
      c = g & (chunks - 1);
    } else {
      i = g / chunks;
      c = g - i * chunks;
    }
    const int64_t src = s_src[i];
    value_out[(p0 + i) * chunks + c] = src >= 0 ? value[src * chunks + c] : diag_values[(-1 - src) * chunks + c];
  }
}

__global__ void __launch_bounds__(kThreads)
fill_i64_kernel(int64_t* __restrict__ p, int64_t n, int64_t v) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) p[i] = v;
}

// One lane per main-diagonal row r < min(M, N): the LAST stored (r, r) entry
// (storage order, as upstream's out[row[mask]] = value[mask] leaves it), or zero.
template <typename T>
__global__ void __launch_bounds__(kThreads)
get_diag_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, const T* __restrict__ value,
                int64_t chunks, int64_t D, T* __restrict__ out, float* __restrict__ out_ones,
                int64_t* __restrict__ pos_out) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= D) return;
  const int64_t s = rowptr[r], e = rowptr[r + 1];
  const int64_t lb = lower_bound(col, s, e, r);
  const int64_t ub = upper_bound(col, lb, e, r);
  const int64_t pos = ub > lb ? ub - 1 : -1;
  if (pos_out != nullptr) pos_out[r] = pos;
  if (value == nullptr) {
    out_ones[r] = pos >= 0 ? 1.0f : 0.0f;
    return;
  }
  for (int64_t c = 0; c < chunks; ++c) out[r * chunks + c] = pos >= 0 ? value[pos * chunks + c] : T{};
}

// out[i] = map[i] >= 0 ? src[map[i]] : 0, row by row.
template <typename T>
__global__ void __launch_bounds__(kThreads)
gather_or_zero_kernel(const T* __restrict__ src, const int64_t* __restrict__ map, int64_t n, int64_t chunks,
                      int shift, T* __restrict__ out) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= n * chunks) return;
  const int64_t i = shift >= 0 ? g >> shift : g / chunks;
  const int64_t c = g - i * chunks;
  const int64_t m = map[i];
  out[g] = m >= 0 ? src[m * chunks + c] : T{};
}

// out[pos[i]] = src[i] for pos[i] >= 0 (distinct positions), row by row.
template <typename T>
__global__ void __launch_bounds__(kThreads)
scatter_rows_kernel(const T* __restrict__ src, const int64_t* __restrict__ pos, int64_t n, int64_t chunks,
                    int shift, T* __restrict__ out) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= n * chunks) return;
  const int64_t i = shift >= 0 ? g >> shift : g / chunks;
  const int64_t c = g - i * chunks;
  const int64_t m = pos[i];
  if (m >= 0) out[m * chunks + c] = src[g];
}

// Calls f(T{}) with the widest piece type T (16, 8, 4, 2 or 1 bytes) that
// divides row_bytes and to which every non-NULL pointer is aligned.
template <typename F>
int with_piece(int64_t row_bytes, std::initializer_list<const void*> ptrs, F&& f) {
  auto fits = [&](int64_t a) {
    if (row_bytes % a != 0) return false;
    for (const void* p : ptrs)
      if (p != nullptr && !psa::aligned(p, static_cast<size_t>(a))) return false;
    return true;
  };
  if (fits(16)) return f(B16{});
  if (fits(8)) return f(uint64_t{});
  if (fits(4)) return f(uint32_t{});
  if (fits(2)) return f(uint16_t{});
  return f(uint8_t{});
}

int shift_of(int64_t chunks) {
  if (chunks <= 0 || (chunks & (chunks - 1)) != 0) return -1;
  int s = 0;
  while ((int64_t{1} << s) < chunks) ++s;
  return s;
}

// k outside (-M, N) has no diagonal cell; clamping keeps r + k well away from overflow.
int64_t clamp_k(int64_t k, int64_t M, int64_t N) {
  if (k > N) return N;
  if (k < -M) return -M;
  return k;
}

// {position of every row's diagonal entry [M] (psa_diag_write reads it), scratch of the row-count scan}
struct DiagWs {
  int64_t* dpos;
  char* scan;
  size_t scan_bytes, bytes;
};

DiagWs diag_layout(void* workspace, int64_t M) {
  psa::Carver c(workspace);
  DiagWs w;
  w.dpos = c.take<int64_t>(static_cast<size_t>(M > 0 ? M : 1), 16);
  w.scan_bytes = psa_count2ptr_workspace_bytes(M);
  w.scan = c.take<char>(w.scan_bytes, 1);
  w.bytes = c.off;
  return w;
}

}  // namespace

extern "C" {

size_t psa_diag_workspace_bytes(int64_t M) {
  return diag_layout(nullptr, M).bytes;
}

int psa_diag_count(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, int64_t k, int insert,
                   const int64_t* colcount, int64_t* rowcount_out, int64_t* rowptr_out, int64_t* colcount_out,
                   void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && N >= 0, "negative size");
  PSA_REQUIRE(rowptr != nullptr && rowptr_out != nullptr, "NULL pointer");
  PSA_REQUIRE(M == 0 || rowcount_out != nullptr, "rowcount_out is NULL");
  PSA_REQUIRE(colcount == nullptr || N == 0 || colcount_out != nullptr, "colcount_out is NULL");
  const DiagWs w = diag_layout(workspace, M);
  if (workspace == nullptr || workspace_bytes < w.bytes) {
    psa::set_error("psa_diag_count: workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  hipStream_t s = psa::as_stream(stream);
  k = clamp_k(k, M, N);
  const int64_t lanes = M > N ? M : (colcount != nullptr ? N : M);
  if (lanes > 0) {
    const int64_t blocks = psa::ceil_div(lanes, kThreads);
    PSA_REQUIRE(blocks <= 0x7fffffff, "M too large for one launch");
    hipLaunchKernelGGL(diag_count_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, rowptr, col,
                       M, N, k, insert ? 1 : 0, colcount, rowcount_out, colcount_out,
                       w.dpos);
    PSA_LAUNCH_CHECK();
  }
  return psa_count2ptr(rowcount_out, M, rowptr_out, w.scan, w.scan_bytes, stream);
}

int psa_diag_write(const int64_t* rowptr, const int64_t* col, const void* value, int64_t row_bytes,
                   const void* diag_values, int64_t M, int64_t N, int64_t k, int insert, int64_t nnz,
                   const int64_t* rowptr_out, int64_t nnz_out, const void* workspace, int64_t* col_out,
                   void* value_out, int64_t* out_pos, int64_t* diag_pos, psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && N >= 0 && nnz >= 0 && nnz_out >= 0 && row_bytes >= 0, "negative size");
  PSA_REQUIRE(rowptr != nullptr && rowptr_out != nullptr && workspace != nullptr, "NULL pointer");
  PSA_REQUIRE(nnz == 0 || col != nullptr, "col is NULL");
  PSA_REQUIRE(nnz_out == 0 || col_out != nullptr, "col_out is NULL");
  hipStream_t s = psa::as_stream(stream);
  k = clamp_k(k, M, N);
  // value_out decides whether values move (value itself is NULL for an empty matrix)
  const bool has_value = value_out != nullptr && row_bytes > 0;
  const int64_t nd = k >= 0 ? (M < N - k ? M : N - k) : (M + k < N ? M + k : N);
  PSA_REQUIRE(!has_value || nnz == 0 || value != nullptr, "value is NULL");
  PSA_REQUIRE(!has_value || !insert || nd <= 0 || diag_values != nullptr, "diag_values is NULL");
  if (out_pos != nullptr && nnz > 0) {  // removed entries keep -1
    int64_t blocks = psa::ceil_div(nnz, kThreads);
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(fill_i64_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, out_pos, nnz,
                       int64_t{-1});
    PSA_LAUNCH_CHECK();
  }
  if (nnz_out == 0) return PSA_OK;
  const int64_t blocks = psa::ceil_div(nnz_out, kTile);
  PSA_REQUIRE(blocks <= 0x7fffffff, "nnz_out too large for one launch");
  const int64_t* dpos = static_cast<const int64_t*>(workspace);
  return with_piece(has_value ? row_bytes : 1, {value, diag_values, value_out}, [&](auto piece) {
    using T = decltype(piece);
    const int64_t chunks = has_value ? row_bytes / static_cast<int64_t>(sizeof(T)) : 0;
    hipLaunchKernelGGL((diag_write_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, rowptr,
                       col, static_cast<const T*>(value), chunks, shift_of(chunks),
                       static_cast<const T*>(diag_values), M, N, k, insert ? 1 : 0, rowptr_out, nnz_out, dpos,
                       col_out, has_value ? static_cast<T*>(value_out) : nullptr, out_pos, diag_pos);
    PSA_LAUNCH_CHECK();
    return PSA_OK;
  });
}

int psa_get_diag(const int64_t* rowptr, const int64_t* col, const void* value, int64_t row_bytes, int64_t M,
                 int64_t N, void* out, int64_t* pos_out, psa_stream_t stream) {
  PSA_REQUIRE(M >= 0 && N >= 0 && row_bytes >= 0, "negative size");
  const int64_t D = M < N ? M : N;
  if (D == 0 || (value != nullptr && row_bytes == 0 && pos_out == nullptr)) return PSA_OK;
  PSA_REQUIRE(rowptr != nullptr && out != nullptr, "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  const int64_t blocks = psa::ceil_div(D, kThreads);
  PSA_REQUIRE(blocks <= 0x7fffffff, "M too large for one launch");
  return with_piece(value != nullptr && row_bytes > 0 ? row_bytes : 1, {value, out}, [&](auto piece) {
    using T = decltype(piece);
    const int64_t chunks = value != nullptr ? row_bytes / static_cast<int64_t>(sizeof(T)) : 0;
    hipLaunchKernelGGL((get_diag_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, rowptr,
                       col, static_cast<const T*>(value), chunks, D, static_cast<T*>(out),
                       static_cast<float*>(out), pos_out);
    PSA_LAUNCH_CHECK();
    return PSA_OK;
  });
}

int psa_diag_gather(const void* src, const int64_t* map, int64_t n, int64_t row_bytes, void* out,
                    psa_stream_t stream) {
  PSA_REQUIRE(n >= 0 && row_bytes >= 0, "negative size");
  if (n == 0 || row_bytes == 0) return PSA_OK;
  PSA_REQUIRE(src && map && out, "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  return with_piece(row_bytes, {src, out}, [&](auto piece) {
    using T = decltype(piece);
    const int64_t chunks = row_bytes / static_cast<int64_t>(sizeof(T));
    const int64_t blocks = psa::ceil_div(n * chunks, kThreads);
    PSA_REQUIRE(blocks <= 0x7fffffff, "too many elements for one launch");
    hipLaunchKernelGGL((gather_or_zero_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s,
                       static_cast<const T*>(src), map, n, chunks, shift_of(chunks), static_cast<T*>(out));
    PSA_LAUNCH_CHECK();
    return PSA_OK;
  });
}

int psa_diag_scatter(const void* src, const int64_t* pos, int64_t n, int64_t row_bytes, void* out,
                     psa_stream_t stream) {
  PSA_REQUIRE(n >= 0 && row_bytes >= 0, "negative size");
  if (n == 0 || row_bytes == 0) return PSA_OK;
  PSA_REQUIRE(src && pos && out, "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  return with_piece(row_bytes, {src, out}, [&](auto piece) {
    using T = decltype(piece);
    const int64_t chunks = row_bytes / static_cast<int64_t>(sizeof(T));
    const int64_t blocks = psa::ceil_div(n * chunks, kThreads);
    PSA_REQUIRE(blocks <= 0x7fffffff, "too many elements for one launch");
    hipLaunchKernelGGL((scatter_rows_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s,
                       static_cast<const T*>(src), pos, n, chunks, shift_of(chunks), static_cast<T*>(out));
    PSA_LAUNCH_CHECK();
    return PSA_OK;
  });
}

}  // extern "C"
