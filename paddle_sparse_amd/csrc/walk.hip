// GraphSAINT's random-walk sampler on a sorted CSR matrix for gfx950:
// random_walk (torch_sparse rw.py) and saint_subgraph (torch_sparse saint.py).
//
// random_walk: ONE launch runs every step, one lane per walk, the current node
// in a register.  A step is two dependent random reads (the rowptr pair, then
// col) and the draw of rng.h with stream = walk n, draw = step l, so step 0 of
// walk n picks the edge sample_adj(start, 1, replace=True, seed) picks for
// subset row n.  A node without entries keeps the walk where it is.  The walk
// rows are written either one 8-byte store per step or, by default, in bursts
// of kBuf steps held in registers (vmcnt counts stores with loads, so a store
// per step puts its completion on the next step's load wait).
//
// saint_subgraph: the induced subgraph of node_idx, as a stream compaction over
// the concatenated candidate list (every stored entry of every selected row, in
// selection order):
//   init + assoc    assoc[node_idx[i]] = max i (the last duplicate wins: one
//                   atomicMax per i), flags: out of range / decreasing
//   degree          counts[i] = degree of node_idx[i], flag: duplicates;
//                   psa_count2ptr -> in_ptr (C = in_ptr[S] candidates)
//   tile count      a fixed grid of kBlocks workgroups splits [0, C) evenly (C
//                   is read on the device, so no host read sizes the grid); a
//                   tile finds the rows it spans by a wave search in in_ptr and
//                   stages them in LDS as diag.hip's write pass does; candidate
//                   p of row i is entry e = rowptr[node_idx[i]] + p - in_ptr[i],
//                   kept when assoc[col[e]] >= 0.  A hub row spans many tiles.
//   psa_count2ptr of the block counts -> info = {nnz', flags}: THE host read
//   write           the same enumeration with an in-block scan: row', col' =
//                   assoc[col[e]], edge_index = e, in candidate order; rowptr'
//                   from row' (psa_ind2ptr).
// Candidate order is (row, col') order unless node_idx decreases somewhere
// (flag bit 2); only then does the caller re-sort.
#include "common.h"
#include "rng.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBuf = 16;                 // steps per burst of the buffered walk: one 128-byte line of a row
constexpr int kPer = 4;                  // candidates per lane per tile
constexpr int kTile = kThreads * kPer;   // candidates per tile
constexpr int kRows = 512;               // rows of a tile staged in LDS
constexpr int kBlocks = 2048;            // workgroups of the two candidate passes

int g_walk_variant = 0;

// ---- random_walk ----------------------------------------------------------------

// WALKS independent walks per lane (walk g + w * lanes), BUF steps per burst of
// stores (1: a store per step).  Walk n's row of out starts at n * (L + 1).
template <int WALKS, int BUF>
__global__ void __launch_bounds__(kThreads)
random_walk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                   const int64_t* __restrict__ start, int64_t S, int64_t L, int64_t N, uint64_t seed,
                   int64_t* __restrict__ out, unsigned long long* __restrict__ flags) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  int64_t cur[WALKS], row[WALKS];
  uint64_t stream[WALKS];
  bool live[WALKS];
#pragma unroll
  for (int w = 0; w < WALKS; ++w) {
    const int64_t n = g + w * lanes;
    live[w] = n < S;
    cur[w] = live[w] ? start[n] : 0;
    if (live[w] && (cur[w] < 0 || cur[w] >= N)) {
      atomicOr(flags, 1ull);
      live[w] = false;
    }
    row[w] = n * (L + 1);
    stream[w] = psa::rand_stream(seed, n);
    if (live[w]) out[row[w]] = cur[w];
  }
  for (int64_t l0 = 0; l0 < L; l0 += BUF) {
    int64_t buf[WALKS][BUF];
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      const int64_t l = l0 + j;
      if (l < L) {  // uniform across the grid
        int64_t s[WALKS], deg[WALKS];
#pragma unroll
        for (int w = 0; w < WALKS; ++w) {
          s[w] = live[w] ? rowptr[cur[w]] : 0;
          deg[w] = live[w] ? rowptr[cur[w] + 1] - s[w] : 0;
        }
#pragma unroll
        for (int w = 0; w < WALKS; ++w) {
          if (deg[w] > 0) cur[w] = col[s[w] + psa::rand_draw(stream[w], l, deg[w])];
          buf[w][j] = cur[w];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      if (l0 + j < L) {
#pragma unroll
        for (int w = 0; w < WALKS; ++w)
          if (live[w]) out[row[w] + l0 + j + 1] = buf[w][j];
      }
    }
  }
}

// ---- saint_subgraph ---------------------------------------------------------------

// Largest r in [lo, hi) with ptr[r] <= p, given ptr[lo] <= p; called by a whole wave.
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

// Largest r in [lo, hi) with ptr[r] <= p (ptr[lo] <= p), one lane.
__device__ __forceinline__ int64_t last_le(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t p) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads)
saint_init_kernel(int64_t* __restrict__ assoc, int64_t N, unsigned long long* __restrict__ info) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g < 2) info[g] = 0;
  for (int64_t i = g; i < N; i += stride) assoc[i] = -1;
}

// flags: bit 0 = a node outside [0, N), bit 2 = node_idx decreases somewhere.
__global__ void __launch_bounds__(kThreads)
saint_assoc_kernel(const int64_t* __restrict__ node_idx, int64_t S, int64_t N, long long* __restrict__ assoc,
                   unsigned long long* __restrict__ flags) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t v = node_idx[i];
  if (v < 0 || v >= N) {
    atomicOr(flags, 1ull);
    return;
  }
  __hip_atomic_fetch_max(assoc + v, static_cast<long long>(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i > 0 && node_idx[i - 1] > v) atomicOr(flags, 4ull);
}

// counts[i] = degree of node_idx[i] (0 outside the matrix); flags bit 1 = a duplicate.
__global__ void __launch_bounds__(kThreads)
saint_degree_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ node_idx, int64_t S,
                    int64_t N, const int64_t* __restrict__ assoc, int64_t* __restrict__ counts,
                    unsigned long long* __restrict__ flags) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t v = node_idx[i];
  if (v < 0 || v >= N) {
    counts[i] = 0;
    return;
  }
  counts[i] = rowptr[v + 1] - rowptr[v];
  if (assoc[v] != i) atomicOr(flags, 2ull);
}

// Candidates of tile [p0, p1) of this block's range: the tile's rows staged in LDS
// (or searched in global memory when more than kRows rows, i.e. a run of empty
// rows, fall into it), then per lane the kPer candidates li = j * kThreads + tid:
// keep bit, and for a kept one its row and new column; e = source entry.
struct Tile {
  int64_t r_lo, nr;
  bool staged;
};

__device__ __forceinline__ Tile stage_tile(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ node_idx,
                                           int64_t S, int64_t N, const int64_t* __restrict__ in_ptr, int64_t p0,
                                           int64_t p1, int64_t* s_ptr, int64_t* s_base, int64_t* s_bounds) {
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // the previous tile's readers of s_ptr / s_base are done
  if (wave < 2) {
    const int64_t r = wave_search(in_ptr, 0, S, wave == 0 ? p0 : p1 - 1);
    if ((threadIdx.x & 63) == 0) s_bounds[wave] = r;
  }
  __syncthreads();
  Tile t;
  t.r_lo = s_bounds[0];
  t.nr = s_bounds[1] - t.r_lo + 1;
  t.staged = t.nr <= kRows;
  if (t.staged) {
    for (int i = threadIdx.x; i < t.nr; i += kThreads) {
      const int64_t r = t.r_lo + i;
      const int64_t q = in_ptr[r], v = node_idx[r];
      s_ptr[i] = q;
      s_base[i] = v >= 0 && v < N ? rowptr[v] - q : 0;  // a node outside has no candidates
    }
  }
  __syncthreads();
  return t;
}

__device__ __forceinline__ bool candidate(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                          const int64_t* __restrict__ node_idx, const int64_t* __restrict__ in_ptr,
                                          const int64_t* __restrict__ assoc, const Tile& t, const int64_t* s_ptr,
                                          const int64_t* s_base, int64_t p, int64_t* r_out, int64_t* c_out,
                                          int64_t* e_out) {
  int64_t r, base;
  if (t.staged) {
    int lo = 0, hi = static_cast<int>(t.nr);
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_ptr[mid] <= p) lo = mid;
      else hi = mid;
    }
    r = t.r_lo + lo;
    base = s_base[lo];
  } else {
    r = last_le(in_ptr, t.r_lo, t.r_lo + t.nr, p);
    base = rowptr[node_idx[r]] - in_ptr[r];
  }
  const int64_t e = p + base;
  const int64_t a = assoc[col[e]];
  *r_out = r;
  *c_out = a;
  *e_out = e;
  return a >= 0;
}

__device__ __forceinline__ void block_range(const int64_t* __restrict__ in_ptr, int64_t S, int64_t* lo, int64_t* hi) {
  const int64_t C = in_ptr[S];
  *lo = C / kBlocks * blockIdx.x + (C % kBlocks) * blockIdx.x / kBlocks;
  *hi = C / kBlocks * (blockIdx.x + 1) + (C % kBlocks) * (blockIdx.x + 1) / kBlocks;
}

__global__ void __launch_bounds__(kThreads)
saint_count_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                   const int64_t* __restrict__ node_idx, int64_t S, int64_t N, const int64_t* __restrict__ in_ptr,
                   const int64_t* __restrict__ assoc, int64_t* __restrict__ block_counts) {
  __shared__ int64_t s_ptr[kRows], s_base[kRows], s_bounds[2];
  __shared__ int s_wave[kWaves];
  int64_t lo, hi;
  block_range(in_ptr, S, &lo, &hi);
  int kept = 0;
  for (int64_t p0 = lo; p0 < hi; p0 += kTile) {
    const int64_t p1 = hi - p0 < kTile ? hi : p0 + kTile;
    const Tile t = stage_tile(rowptr, node_idx, S, N, in_ptr, p0, p1, s_ptr, s_base, s_bounds);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t p = p0 + j * kThreads + threadIdx.x;
      int64_t r, c, e;
      if (p < p1 && candidate(rowptr, col, node_idx, in_ptr, assoc, t, s_ptr, s_base, p, &r, &c, &e)) ++kept;
    }
  }
  for (int off = 32; off > 0; off >>= 1) kept += __shfl_down(kept, off);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += s_wave[w];
    block_counts[blockIdx.x] = sum;
  }
}

__global__ void saint_info_kernel(const int64_t* __restrict__ block_ptr, int64_t* __restrict__ info) {
  info[0] = block_ptr[kBlocks];
}

__global__ void __launch_bounds__(kThreads)
saint_write_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                   const int64_t* __restrict__ node_idx, int64_t S, int64_t N, const int64_t* __restrict__ in_ptr,
                   const int64_t* __restrict__ assoc, const int64_t* __restrict__ block_ptr,
                   int64_t* __restrict__ row_out, int64_t* __restrict__ col_out, int64_t* __restrict__ edge_out) {
  __shared__ int64_t s_ptr[kRows], s_base[kRows], s_bounds[2];
  __shared__ int s_wave[2][kWaves];
  int64_t lo, hi;
  block_range(in_ptr, S, &lo, &hi);
  int64_t q0 = block_ptr[blockIdx.x];  // output slot of the next kept candidate
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int flip = 0;
  for (int64_t p0 = lo; p0 < hi; p0 += kTile) {
    const int64_t p1 = hi - p0 < kTile ? hi : p0 + kTile;
    const Tile t = stage_tile(rowptr, node_idx, S, N, in_ptr, p0, p1, s_ptr, s_base, s_bounds);
    for (int j = 0; j < kPer; ++j) {
      const int64_t p = p0 + j * kThreads + threadIdx.x;
      int64_t r = 0, c = 0, e = 0;
      const bool keep = p < p1 && candidate(rowptr, col, node_idx, in_ptr, assoc, t, s_ptr, s_base, p, &r, &c, &e);
      const uint64_t mask = __ballot(keep);
      if (lane == 0) s_wave[flip][wave] = __popcll(mask);
      __syncthreads();
      int64_t before = q0, total = 0;
      for (int w = 0; w < kWaves; ++w) {
        const int n = s_wave[flip][w];
        if (w < wave) before += n;
        total += n;
      }
      flip ^= 1;  // the next sub-tile writes the other copy: one barrier per sub-tile
      if (keep) {
        const int64_t q = before + __popcll(mask & ((1ull << lane) - 1));
        row_out[q] = r;
        col_out[q] = c;
        edge_out[q] = e;
      }
      q0 += total;
    }
  }
}

int grid_for(int64_t n, unsigned* blocks) {
  const int64_t b = psa::ceil_div(n > 0 ? n : 1, kThreads);
  if (b > 0x7fffffff) return 0;
  *blocks = static_cast<unsigned>(b);
  return 1;
}

// workspace: assoc int64[N] | counts int64[S] | in_ptr int64[S+1] | block_counts int64[kBlocks]
//            | block_ptr int64[kBlocks+1] | count2ptr scratch (max of S and kBlocks)
struct SaintWs {
  int64_t *assoc, *counts, *in_ptr, *block_counts, *block_ptr;
  void* scan;
  size_t scan_bytes;
};

size_t saint_layout(int64_t S, int64_t N, char* base, SaintWs* ws) {
  const int64_t n_scan = S > kBlocks ? S : kBlocks;
  psa::Carver c(base);
  SaintWs w;
  w.assoc = c.take<int64_t>(static_cast<size_t>(N > 0 ? N : 1), 16);
  w.counts = c.take<int64_t>(static_cast<size_t>(S > 0 ? S : 1), 16);
  w.in_ptr = c.take<int64_t>(static_cast<size_t>(S + 1), 16);
  w.block_counts = c.take<int64_t>(kBlocks, 16);
  w.block_ptr = c.take<int64_t>(kBlocks + 1, 16);
  w.scan_bytes = psa_count2ptr_workspace_bytes(n_scan);
  w.scan = c.take<char>(w.scan_bytes, 16);
  if (ws) *ws = w;
  return c.off;
}

}  // namespace

extern "C" {

int psa_random_walk_set_variant(int variant) {
  const int prev = g_walk_variant;
  g_walk_variant = variant;
  return prev;
}

int psa_random_walk(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* start, int64_t S,
                    int64_t walk_length, uint64_t seed, int64_t* out, int64_t* flags, psa_stream_t stream) {
  PSA_REQUIRE(N >= 0 && S >= 0 && walk_length >= 0, "negative size");
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && start && out && flags, "NULL pointer");
  PSA_REQUIRE(walk_length < INT64_MAX / S - 1, "output too large");
  hipStream_t s = psa::as_stream(stream);
  const int v = g_walk_variant;
  const int walks = (v == 3 || v == 4) ? 2 : 1;
  unsigned blocks;
  PSA_REQUIRE(grid_for(psa::ceil_div(S, walks), &blocks), "too many walks for one launch");
  auto* f = reinterpret_cast<unsigned long long*>(flags);
  if (v == 1) {
    hipLaunchKernelGGL((random_walk_kernel<1, 1>), dim3(blocks), dim3(kThreads), 0, s, rowptr, col, start, S,
                       walk_length, N, seed, out, f);
  } else if (v == 3) {
    hipLaunchKernelGGL((random_walk_kernel<2, 1>), dim3(blocks), dim3(kThreads), 0, s, rowptr, col, start, S,
                       walk_length, N, seed, out, f);
  } else if (v == 4) {
    hipLaunchKernelGGL((random_walk_kernel<2, kBuf>), dim3(blocks), dim3(kThreads), 0, s, rowptr, col, start, S,
                       walk_length, N, seed, out, f);
  } else {  // 0 (default) and 2
    hipLaunchKernelGGL((random_walk_kernel<1, kBuf>), dim3(blocks), dim3(kThreads), 0, s, rowptr, col, start, S,
                       walk_length, N, seed, out, f);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

size_t psa_saint_workspace_bytes(int64_t S, int64_t N) {
  return saint_layout(S < 0 ? 0 : S, N < 0 ? 0 : N, nullptr, nullptr);
}

int psa_saint_count(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* node_idx, int64_t S,
                    void* workspace, size_t workspace_bytes, int64_t* info, psa_stream_t stream) {
  PSA_REQUIRE(N >= 0 && S >= 0, "negative size");
  PSA_REQUIRE(rowptr && info && (node_idx || S == 0), "NULL pointer");
  if (workspace == nullptr || workspace_bytes < psa_saint_workspace_bytes(S, N)) {
    psa::set_error("psa_saint_count: workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  hipStream_t s = psa::as_stream(stream);
  SaintWs ws;
  saint_layout(S, N, static_cast<char*>(workspace), &ws);
  auto* flags = reinterpret_cast<unsigned long long*>(info + 1);
  unsigned blocks;
  PSA_REQUIRE(grid_for(N, &blocks), "N too large for one launch");
  blocks = blocks > 8192 ? 8192 : blocks;
  hipLaunchKernelGGL(saint_init_kernel, dim3(blocks), dim3(kThreads), 0, s, ws.assoc, N,
                     reinterpret_cast<unsigned long long*>(info));
  PSA_LAUNCH_CHECK();
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(col != nullptr, "col is NULL");
  PSA_REQUIRE(grid_for(S, &blocks), "node_idx too large for one launch");
  hipLaunchKernelGGL(saint_assoc_kernel, dim3(blocks), dim3(kThreads), 0, s, node_idx, S, N,
                     reinterpret_cast<long long*>(ws.assoc), flags);
  hipLaunchKernelGGL(saint_degree_kernel, dim3(blocks), dim3(kThreads), 0, s, rowptr, node_idx, S, N, ws.assoc,
                     ws.counts, flags);
  PSA_LAUNCH_CHECK();
  int st = psa_count2ptr(ws.counts, S, ws.in_ptr, ws.scan, ws.scan_bytes, stream);
  if (st != PSA_OK) return st;
  hipLaunchKernelGGL(saint_count_kernel, dim3(kBlocks), dim3(kThreads), 0, s, rowptr, col, node_idx, S, N,
                     ws.in_ptr, ws.assoc, ws.block_counts);
  PSA_LAUNCH_CHECK();
  st = psa_count2ptr(ws.block_counts, kBlocks, ws.block_ptr, ws.scan, ws.scan_bytes, stream);
  if (st != PSA_OK) return st;
  hipLaunchKernelGGL(saint_info_kernel, dim3(1), dim3(1), 0, s, ws.block_ptr, info);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_saint_write(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* node_idx, int64_t S,
                    const void* workspace, int64_t nnz_out, int64_t* rowptr_out, int64_t* row_out,
                    int64_t* col_out, int64_t* edge_out, psa_stream_t stream) {
  PSA_REQUIRE(N >= 0 && S >= 0 && nnz_out >= 0, "negative size");
  PSA_REQUIRE(rowptr_out != nullptr, "rowptr_out is NULL");
  PSA_REQUIRE(nnz_out == 0 || (rowptr && col && node_idx && workspace && row_out && col_out && edge_out),
              "NULL pointer");
  if (nnz_out > 0) {
    SaintWs ws;
    saint_layout(S, N, static_cast<char*>(const_cast<void*>(workspace)), &ws);
    hipLaunchKernelGGL(saint_write_kernel, dim3(kBlocks), dim3(kThreads), 0, psa::as_stream(stream), rowptr, col,
                       node_idx, S, N, ws.in_ptr, ws.assoc, ws.block_ptr, row_out, col_out, edge_out);
    PSA_LAUNCH_CHECK();
  }
  return psa_ind2ptr(row_out, nnz_out, S, rowptr_out, stream);
}

}  // extern "C"
