// gfx950 only.
// reverse_cuthill_mckee (torch_sparse bandwidth.py, which copies to the host and calls
// scipy): the Cuthill-McKee order of a square sorted CSR pattern, built on the device.
//
// Definition: deg[i] = rowptr[i+1] - rowptr[i]; components in the order of
// their seed, the unvisited node with the smallest (deg, id); inside a component a
// breadth-first search whose level is ordered by (position of the earliest-placed
// parent, deg, id).  perm is that order reversed.
//
// Device state: rank int32[N] (position in the order, kUnseen before), claim int32[N]
// (smallest parent position that reached the node), order int32[N], seeds int64[N] (the
// stable psa_index_sort of deg: (deg, id) order) and the caller's state block.  The
// degree-0 nodes are the first n0 seeds and take the positions 0..n0-1 in one launch.
//
// Two level paths produce the same bits:
//   small   one workgroup runs level after level (and starts the next component from
//           seeds) until all is placed or a level has more than the capacity of
//           candidate edges / frontier rows; that level is left untouched for
//   large   a fixed launch sequence over the level's candidate list: frontier degrees ->
//           psa_count2ptr -> claim (atomicMin) -> count kept -> psa_count2ptr over the
//           tiles -> [host read of the count] -> write keys in candidate order ->
//           psa_sort_pairs_u32 (stable) -> place.
// Phases inside the small kernel are ordered by __syncthreads alone; no workgroup of
// this file waits for another one.  Every loop is bounded by N or nnz.
#include "coalesce_internal.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;            // large path
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;                  // candidates per lane per tile
constexpr int kTile = kThreads * kPer;   // candidates per workgroup of the large path
constexpr int kSmallThreads = 1024;      // small path: one workgroup
constexpr int kSmallWaves = kSmallThreads / 64;
constexpr int kSmallCap = 4096;          // candidate edges of a level (LDS: 12 bytes each)
constexpr int kSmallRows = 2048;         // frontier rows of a level (LDS: 4 bytes each)
constexpr int kSmallCapTest = 8;         // variant 2
constexpr int32_t kUnseen = 0x7fffffff;

// the caller's state block, int64[PSA_RCM_STATE_WORDS]
enum { kPlaced = 0, kLo, kHi, kNextSeed, kStatus, kCand, kNew, kNextCand, kFault, kSmallLevels, kWords };
static_assert(kWords <= PSA_RCM_STATE_WORDS, "state block");

int g_rcm_variant = 0;

int small_cap() { return g_rcm_variant == 1 ? 0 : g_rcm_variant == 2 ? kSmallCapTest : kSmallCap; }

__device__ __forceinline__ int32_t ld32(const int32_t* p) {
  // L2-served: the line may sit in this CU's L1 from before an atomic or a store of another wave
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads)
rcm_init_kernel(const int64_t* __restrict__ rowptr, int64_t N, int64_t* __restrict__ deg, int32_t* __restrict__ rank,
                int32_t* __restrict__ claim) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < N; i += stride) {
    deg[i] = rowptr[i + 1] - rowptr[i];
    rank[i] = kUnseen;
    claim[i] = kUnseen;
  }
}

// The degree-0 nodes in closed form, and the state block.
__global__ void __launch_bounds__(kThreads)
rcm_isolated_kernel(const int64_t* __restrict__ seeds, int64_t n0, int64_t N, int32_t* __restrict__ rank,
                    int32_t* __restrict__ order, int64_t* __restrict__ state, const uint32_t* __restrict__ fault) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  for (int64_t i = g; i < n0; i += stride) {
    const int64_t s = seeds[i];
    if (static_cast<uint64_t>(s) >= static_cast<uint64_t>(N)) continue;  // a faulted sort: state[kFault] says so
    order[i] = static_cast<int32_t>(s);
    rank[s] = static_cast<int32_t>(i);
  }
  if (g < PSA_RCM_STATE_WORDS) {
    int64_t v = 0;
    if (g == kPlaced || g == kLo || g == kHi || g == kNextSeed) v = n0;
    if (g == kStatus) v = PSA_RCM_HANDOVER;
    if (g == kFault) v = fault != nullptr && *fault != 0u ? 1 : 0;
    state[g] = v;
  }
}

// ---- small path ---------------------------------------------------------------------

__device__ __forceinline__ int64_t small_sum(int64_t v, int64_t* s_sum) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();  // the previous sum's readers are done
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t t = 0;
  for (int w = 0; w < kSmallWaves; ++w) t += s_sum[w];
  return t;
}

__device__ __forceinline__ int small_excl_scan(int v, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int n = __shfl_up(inc, off);
    if (lane >= off) inc += n;
  }
  __syncthreads();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  return before + inc - v;
}

__global__ void __launch_bounds__(kSmallThreads)
rcm_small_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                 const int64_t* __restrict__ seeds, int32_t* rank, int32_t* claim, int32_t* order,
                 int64_t* __restrict__ state, int cap, int64_t dstride) {
  __shared__ uint64_t s_key[kSmallCap];
  __shared__ uint32_t s_id[kSmallCap];
  __shared__ int32_t s_ptr[kSmallRows + 1];
  __shared__ int64_t s_sum[kSmallWaves];
  __shared__ int s_wave[kSmallWaves];
  __shared__ int s_first, s_cnt;
  const int tid = threadIdx.x;
  if (state[kFault] != 0) return;  // seeds cannot be trusted
  int64_t placed = state[kPlaced], lo = state[kLo], hi = state[kHi], next_seed = state[kNextSeed];
  int64_t levels = 0, cand = 0, status = PSA_RCM_DONE;
  // a turn places a node, or finds the level empty and the next turn places a seed
  for (int64_t turn = 0; turn <= 2 * N + 1; ++turn) {
    if (lo == hi) {  // the component is complete
      if (placed >= N) break;
      int f = kUnseen;
      while (next_seed < N) {  // chunks of the (deg, id) list; next_seed only grows: N steps in all
        __syncthreads();
        if (tid == 0) s_first = kUnseen;
        __syncthreads();
        const int64_t i = next_seed + tid;
        if (i < N && ld32(rank + seeds[i]) == kUnseen) atomicMin(&s_first, tid);
        __syncthreads();
        f = s_first;
        if (f != kUnseen) break;
        next_seed += kSmallThreads;
      }
      if (f == kUnseen) break;  // placed < N leaves an unseen node: not reached
      next_seed += f;
      const int64_t s = seeds[next_seed];
      if (tid == 0) {
        order[placed] = static_cast<int32_t>(s);
        rank[s] = static_cast<int32_t>(placed);
      }
      lo = placed;
      hi = ++placed;
      ++next_seed;
      __syncthreads();
      continue;
    }
    const int64_t F = hi - lo;
    int64_t mine = 0;
    for (int64_t i = tid; i < F; i += kSmallThreads) {
      const int64_t v = ld32(order + lo + i);
      mine += rowptr[v + 1] - rowptr[v];
    }
    const int64_t C64 = small_sum(mine, s_sum);
    if (F > kSmallRows || C64 > cap) {  // untouched, for the large path
      cand = C64;
      status = PSA_RCM_HANDOVER;
      break;
    }
    const int C = static_cast<int>(C64), Fi = static_cast<int>(F);
    {  // s_ptr: exclusive scan of the frontier's degrees, two rows per thread
      int d[2];
      for (int k = 0; k < 2; ++k) {
        const int i = 2 * tid + k;
        d[k] = 0;
        if (i < Fi) {
          const int64_t v = ld32(order + lo + i);
          d[k] = static_cast<int>(rowptr[v + 1] - rowptr[v]);
        }
      }
      const int base = small_excl_scan(d[0] + d[1], s_wave);
      if (2 * tid < Fi) s_ptr[2 * tid] = base;
      if (2 * tid + 1 < Fi) s_ptr[2 * tid + 1] = base + d[0];
      if (tid == 0) {
        s_ptr[Fi] = C;
        s_cnt = 0;
      }
    }
    __syncthreads();
    // enumerate and claim: s_id = child, s_key = parent (local) for the next phase
    for (int p = tid; p < C; p += kSmallThreads) {
      int l = 0, h = Fi;
      while (h - l > 1) {
        const int mid = (l + h) >> 1;
        if (s_ptr[mid] <= p) l = mid;
        else h = mid;
      }
      const int64_t e = rowptr[ld32(order + lo + l)] + (p - s_ptr[l]);
      const int64_t c = col[e];
      const bool ok = static_cast<uint64_t>(c) < static_cast<uint64_t>(N);
      s_id[p] = ok ? static_cast<uint32_t>(c) : 0xffffffffu;
      s_key[p] = static_cast<uint64_t>(l);
      if (ok && ld32(rank + c) == kUnseen) atomicMin(claim + c, static_cast<int32_t>(lo + l));
    }
    __syncthreads();
    int P = 1;
    while (P < C) P <<= 1;
    for (int p = tid; p < P; p += kSmallThreads) {
      uint64_t key = ~uint64_t{0};
      if (p < C) {
        const int l = static_cast<int>(s_key[p]);
        const uint32_t c = s_id[p];
        bool keep = c != 0xffffffffu && ld32(rank + c) == kUnseen && ld32(claim + c) == lo + l;
        if (keep && p > s_ptr[l]) {  // the first of its duplicates in the (sorted) row
          const int64_t e = rowptr[ld32(order + lo + l)] + (p - s_ptr[l]);
          keep = col[e - 1] != static_cast<int64_t>(c);
        }
        if (keep) {
          key = static_cast<uint64_t>(l) * static_cast<uint64_t>(dstride) +
                static_cast<uint64_t>(rowptr[c + 1] - rowptr[c]);
          atomicAdd(&s_cnt, 1);
        } else {
          s_id[p] = 0xffffffffu;
        }
      } else {
        s_id[p] = 0xffffffffu;
      }
      s_key[p] = key;
    }
    __syncthreads();
    // bitonic sort of (key, id), ascending; the dropped candidates sink to the end
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < P; t += kSmallThreads) {
          const int u = t ^ j;
          if (u > t) {
            const uint64_t ka = s_key[t], kb = s_key[u];
            const uint32_t ia = s_id[t], ib = s_id[u];
            const bool gt = ka > kb || (ka == kb && ia > ib);
            if (gt == ((t & k) == 0)) {
              s_key[t] = kb;
              s_key[u] = ka;
              s_id[t] = ib;
              s_id[u] = ia;
            }
          }
        }
        __syncthreads();
      }
    }
    const int n_new = s_cnt;
    if (hi + n_new > N) {  // rows not sorted (a duplicate kept twice): stop before order overflows
      status = PSA_RCM_BAD_INPUT;
      break;
    }
    for (int t = tid; t < n_new; t += kSmallThreads) {
      const uint32_t c = s_id[t];
      order[hi + t] = static_cast<int32_t>(c);
      rank[c] = static_cast<int32_t>(hi + t);
    }
    placed += n_new;
    lo = hi;
    hi += n_new;
    ++levels;
    __syncthreads();
  }
  if (tid == 0) {
    state[kPlaced] = placed;
    state[kLo] = lo;
    state[kHi] = hi;
    state[kNextSeed] = next_seed;
    state[kStatus] = status;
    state[kCand] = cand;
    state[kSmallLevels] += levels;
  }
}

// ---- large path -----------------------------------------------------------------------

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

__global__ void __launch_bounds__(kThreads)
rcm_frontier_deg_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ order, int64_t lo, int64_t F,
                        int64_t* __restrict__ counts, int64_t* __restrict__ state) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i == 0) state[kNextCand] = 0;
  if (i >= F) return;
  const int64_t v = order[lo + i];
  counts[i] = rowptr[v + 1] - rowptr[v];
}

// The tile [p0, p1) of the level's candidates: its frontier rows staged in LDS.  Every
// frontier node has an entry (the degree-0 nodes were placed up front and are never
// claimed), so fptr increases strictly and a tile touches at most kTile rows.
struct Tile {
  int64_t p0, p1, r_lo;
  int nr;
};

__device__ __forceinline__ bool stage_tile(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ order,
                                           int64_t lo, int64_t F, const int64_t* __restrict__ fptr, int64_t* s_ptr,
                                           int64_t* s_base, int64_t* s_bounds, Tile* t) {
  const int64_t C = fptr[F];
  t->p0 = static_cast<int64_t>(blockIdx.x) * kTile;
  if (t->p0 >= C) return false;  // block-uniform
  t->p1 = C - t->p0 < kTile ? C : t->p0 + kTile;
  const int wave = threadIdx.x >> 6;
  if (wave < 2) {
    const int64_t r = wave_search(fptr, 0, F, wave == 0 ? t->p0 : t->p1 - 1);
    if ((threadIdx.x & 63) == 0) s_bounds[wave] = r;
  }
  __syncthreads();
  t->r_lo = s_bounds[0];
  const int64_t nr = s_bounds[1] - t->r_lo + 1;
  t->nr = static_cast<int>(nr < kTile ? nr : kTile);
  for (int i = threadIdx.x; i < t->nr; i += kThreads) {
    const int64_t q = fptr[t->r_lo + i];
    s_ptr[i] = q;
    s_base[i] = rowptr[order[lo + t->r_lo + i]] - q;
  }
  __syncthreads();
  return true;
}

// candidate p: its frontier row r (local to the level), entry e, child; false for a column outside the matrix
__device__ __forceinline__ bool candidate(const int64_t* __restrict__ col, int64_t N, const Tile& t,
                                          const int64_t* s_ptr, const int64_t* s_base, int64_t p, int64_t* r,
                                          int64_t* e, bool* row_start, int64_t* child) {
  int l = 0, h = t.nr;
  while (h - l > 1) {
    const int mid = (l + h) >> 1;
    if (s_ptr[mid] <= p) l = mid;
    else h = mid;
  }
  *r = t.r_lo + l;
  *e = p + s_base[l];
  *row_start = p == s_ptr[l];
  *child = col[*e];
  return static_cast<uint64_t>(*child) < static_cast<uint64_t>(N);
}

__global__ void __launch_bounds__(kThreads)
rcm_claim_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                 const int32_t* __restrict__ order, int64_t lo, int64_t F, const int64_t* __restrict__ fptr,
                 const int32_t* __restrict__ rank, int32_t* __restrict__ claim) {
  __shared__ int64_t s_ptr[kTile], s_base[kTile], s_bounds[2];
  Tile t;
  if (!stage_tile(rowptr, order, lo, F, fptr, s_ptr, s_base, s_bounds, &t)) return;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t p = t.p0 + j * kThreads + threadIdx.x;
    int64_t r, e, c;
    bool first;
    if (p < t.p1 && candidate(col, N, t, s_ptr, s_base, p, &r, &e, &first, &c) && rank[c] == kUnseen)
      atomicMin(claim + c, static_cast<int32_t>(lo + r));
  }
}

__device__ __forceinline__ bool kept(const int64_t* __restrict__ col, int64_t N, const Tile& t, const int64_t* s_ptr,
                                     const int64_t* s_base, int64_t lo, const int32_t* __restrict__ rank,
                                     const int32_t* __restrict__ claim, int64_t p, int64_t* r, int64_t* c) {
  int64_t e;
  bool first;
  if (p >= t.p1 || !candidate(col, N, t, s_ptr, s_base, p, r, &e, &first, c)) return false;
  if (rank[*c] != kUnseen || claim[*c] != lo + *r) return false;
  return first || col[e - 1] != *c;  // the first of its duplicates in the (sorted) row
}

// tile_counts[b] = kept candidates of tile b; state[kNextCand] += their degrees
__global__ void __launch_bounds__(kThreads)
rcm_count_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                 const int32_t* __restrict__ order, int64_t lo, int64_t F, const int64_t* __restrict__ fptr,
                 const int32_t* __restrict__ rank, const int32_t* __restrict__ claim,
                 int64_t* __restrict__ tile_counts, int64_t* __restrict__ state) {
  __shared__ int64_t s_ptr[kTile], s_base[kTile], s_bounds[2];
  __shared__ int64_t s_n[kWaves], s_d[kWaves];
  Tile t;
  if (!stage_tile(rowptr, order, lo, F, fptr, s_ptr, s_base, s_bounds, &t)) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = 0;
    return;
  }
  int64_t n = 0, d = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    int64_t r, c;
    if (kept(col, N, t, s_ptr, s_base, lo, rank, claim, t.p0 + j * kThreads + threadIdx.x, &r, &c)) {
      ++n;
      d += rowptr[c + 1] - rowptr[c];
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    n += __shfl_down(n, off);
    d += __shfl_down(d, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_n[threadIdx.x >> 6] = n;
    s_d[threadIdx.x >> 6] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) {
      n += s_n[w];
      d += s_d[w];
    }
    tile_counts[blockIdx.x] = n;
    if (d != 0) atomicAdd(reinterpret_cast<unsigned long long*>(state + kNextCand), static_cast<unsigned long long>(d));
  }
}

__global__ void rcm_info_kernel(const int64_t* __restrict__ tile_ptr, int64_t tiles, int64_t* __restrict__ state) {
  state[kNew] = tile_ptr[tiles];
}

// keys / payload of the kept candidates, in candidate order = (parent, id) order
__global__ void __launch_bounds__(kThreads)
rcm_select_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                  const int32_t* __restrict__ order, int64_t lo, int64_t F, const int64_t* __restrict__ fptr,
                  const int32_t* __restrict__ rank, const int32_t* __restrict__ claim,
                  const int64_t* __restrict__ tile_ptr, int64_t n_new, int64_t dstride, int64_t* __restrict__ keys,
                  uint32_t* __restrict__ pay) {
  __shared__ int64_t s_ptr[kTile], s_base[kTile], s_bounds[2];
  __shared__ int s_wave[kPer][kWaves];
  Tile t;
  if (!stage_tile(rowptr, order, lo, F, fptr, s_ptr, s_base, s_bounds, &t)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bool keep[kPer];
  int64_t r[kPer], c[kPer];
  uint64_t mask[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    keep[j] = kept(col, N, t, s_ptr, s_base, lo, rank, claim, t.p0 + j * kThreads + threadIdx.x, &r[j], &c[j]);
    mask[j] = __ballot(keep[j]);
    if (lane == 0) s_wave[j][wave] = __popcll(mask[j]);
  }
  __syncthreads();
  int64_t q0 = tile_ptr[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    int before = 0, total = 0;
    for (int w = 0; w < kWaves; ++w) {
      const int n = s_wave[j][w];
      if (w < wave) before += n;
      total += n;
    }
    if (keep[j]) {
      const int64_t q = q0 + before + __popcll(mask[j] & ((1ull << lane) - 1));
      if (q < n_new) {
        keys[q] = r[j] * dstride + (rowptr[c[j] + 1] - rowptr[c[j]]);
        pay[q] = static_cast<uint32_t>(c[j]);
      }
    }
    q0 += total;
  }
}

__global__ void __launch_bounds__(kThreads)
rcm_place_kernel(const uint32_t* __restrict__ sorted, int64_t n_new, int64_t hi, int64_t N,
                 int32_t* __restrict__ order, int32_t* __restrict__ rank, int64_t* __restrict__ state,
                 const uint32_t* __restrict__ fault) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i == 0) {
    state[kPlaced] += n_new;
    state[kLo] = hi;
    state[kHi] = hi + n_new;
    state[kCand] = state[kNextCand];
    if (fault != nullptr && *fault != 0u) state[kFault] = 1;
  }
  if (i >= n_new) return;
  const uint32_t c = sorted[i];
  if (c >= static_cast<uint64_t>(N)) {  // a faulted sort stores no payload it can vouch for
    state[kFault] = 1;
    return;
  }
  order[hi + i] = static_cast<int32_t>(c);
  rank[c] = static_cast<int32_t>(hi + i);
}

__global__ void __launch_bounds__(kThreads)
rcm_reverse_kernel(const int32_t* __restrict__ order, int64_t N, int64_t* __restrict__ perm) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < N) perm[i] = order[N - 1 - i];
}

// workspace: buf int64[N] (deg, then the frontier's degrees) | seeds int64[N] | fptr int64[N+1] | keys int64[N]
//            | keys_out int64[N] | pay u32[N] | pay_out u32[N] | rank, claim, order int32[N] | tile_counts
//            int64[T] | tile_ptr int64[T+1] (T = tiles of nnz candidates) | count2ptr scratch | sort scratch
struct RcmWs {
  int64_t *buf, *seeds, *fptr, *keys, *keys_out, *tile_counts, *tile_ptr;
  uint32_t *pay, *pay_out;
  int32_t *rank, *claim, *order;
  void *scan, *sort;
  size_t scan_bytes, sort_bytes;
};

int64_t max_tiles(int64_t nnz) { return psa::ceil_div(nnz > 0 ? nnz : 1, kTile); }

size_t rcm_layout(int64_t N, int64_t nnz, char* base, RcmWs* ws) {
  const size_t n = static_cast<size_t>(N > 0 ? N : 1);
  const int64_t T = max_tiles(nnz);
  psa::Carver c(base);
  RcmWs w;
  w.buf = c.take<int64_t>(n, 256);
  w.seeds = c.take<int64_t>(n, 256);
  w.fptr = c.take<int64_t>(n + 1, 256);
  w.keys = c.take<int64_t>(n, 256);
  w.keys_out = c.take<int64_t>(n, 256);
  w.pay = c.take<uint32_t>(n, 256);
  w.pay_out = c.take<uint32_t>(n, 256);
  w.rank = c.take<int32_t>(n, 256);
  w.claim = c.take<int32_t>(n, 256);
  w.order = c.take<int32_t>(n, 256);
  w.tile_counts = c.take<int64_t>(static_cast<size_t>(T), 256);
  w.tile_ptr = c.take<int64_t>(static_cast<size_t>(T + 1), 256);
  w.scan_bytes = psa_count2ptr_workspace_bytes(N > T ? N : T);
  w.scan = c.take<char>(w.scan_bytes, 256);
  // the sort's scratch is not monotonic in n (smaller look-back tiles below 2^20 keys): a level of
  // any size up to N must fit, and psa_sort_pairs_u32 refuses a workspace that is too small
  const int64_t below = (int64_t{1} << 20) - 1;
  const size_t a = psa_index_sort_workspace_bytes(N, 2), b = psa_index_sort_workspace_bytes(N < below ? N : below, 2);
  w.sort_bytes = a > b ? a : b;
  w.sort = c.take<char>(w.sort_bytes, 256);
  if (ws) *ws = w;
  return c.off;
}

int rcm_args(const char* who, int64_t N, int64_t nnz, const void* workspace, size_t workspace_bytes, RcmWs* ws) {
  if (N < 1 || N >= (int64_t{1} << 31) || nnz < 0) {
    psa::set_error(std::string(who) + ": needs 1 <= N < 2^31 and nnz >= 0");
    return PSA_ERR_INVALID_ARG;
  }
  if (max_tiles(nnz) > 0x7fffffff) {
    psa::set_error(std::string(who) + ": nnz too large for one launch");
    return PSA_ERR_INVALID_ARG;
  }
  if (workspace == nullptr || workspace_bytes < rcm_layout(N, nnz, nullptr, nullptr)) {
    psa::set_error(std::string(who) + ": workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  rcm_layout(N, nnz, static_cast<char*>(const_cast<void*>(workspace)), ws);
  return PSA_OK;
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>(psa::ceil_div(n > 0 ? n : 1, kThreads)); }

}  // namespace

extern "C" {

int psa_rcm_set_variant(int variant) {
  const int prev = g_rcm_variant;
  g_rcm_variant = variant;
  return prev;
}

int64_t psa_rcm_small_capacity(void) { return small_cap(); }

int64_t psa_rcm_tile(void) { return kTile; }

size_t psa_rcm_workspace_bytes(int64_t N, int64_t nnz) {
  if (N < 1 || N >= (int64_t{1} << 31) || nnz < 0) return 0;
  return rcm_layout(N, nnz, nullptr, nullptr);
}

int psa_rcm_init(const int64_t* rowptr, int64_t N, int64_t nnz, int64_t n_empty, int64_t max_deg, void* workspace,
                 size_t workspace_bytes, int64_t* state, psa_stream_t stream) {
  RcmWs w;
  const int st = rcm_args(__func__, N, nnz, workspace, workspace_bytes, &w);
  if (st != PSA_OK) return st;
  PSA_REQUIRE(rowptr && state, "NULL pointer");
  PSA_REQUIRE(n_empty >= 0 && n_empty <= N && max_deg >= 0 && max_deg <= nnz, "row statistics out of range");
  hipStream_t s = psa::as_stream(stream);
  unsigned blocks = blocks_for(N);
  blocks = blocks > 8192 ? 8192 : blocks;
  hipLaunchKernelGGL(rcm_init_kernel, dim3(blocks), dim3(kThreads), 0, s, rowptr, N, w.buf, w.rank, w.claim);
  PSA_LAUNCH_CHECK();
  const int sorted = psa_index_sort(w.buf, N, max_deg + 1, nullptr, w.seeds, w.sort, w.sort_bytes, stream);
  if (sorted != PSA_OK) return sorted;
  blocks = blocks_for(n_empty > PSA_RCM_STATE_WORDS ? n_empty : PSA_RCM_STATE_WORDS);
  blocks = blocks > 8192 ? 8192 : blocks;
  hipLaunchKernelGGL(rcm_isolated_kernel, dim3(blocks), dim3(kThreads), 0, s, w.seeds, n_empty, N, w.rank, w.order,
                     state, psa::sort_fault_word(w.sort, N, max_deg + 1));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_rcm_small(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t max_deg,
                  void* workspace, size_t workspace_bytes, int64_t* state, psa_stream_t stream) {
  RcmWs w;
  const int st = rcm_args(__func__, N, nnz, workspace, workspace_bytes, &w);
  if (st != PSA_OK) return st;
  PSA_REQUIRE(rowptr && state && (col || nnz == 0), "NULL pointer");
  PSA_REQUIRE(max_deg >= 0 && max_deg <= nnz, "max_deg out of range");
  hipLaunchKernelGGL(rcm_small_kernel, dim3(1), dim3(kSmallThreads), 0, psa::as_stream(stream), rowptr, col, N,
                     w.seeds, w.rank, w.claim, w.order, state, small_cap(), max_deg + 1);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_rcm_level_count(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t level_lo,
                        int64_t level_hi, int64_t cand, void* workspace, size_t workspace_bytes, int64_t* state,
                        psa_stream_t stream) {
  RcmWs w;
  int st = rcm_args(__func__, N, nnz, workspace, workspace_bytes, &w);
  if (st != PSA_OK) return st;
  PSA_REQUIRE(rowptr && col && state, "NULL pointer");
  PSA_REQUIRE(level_lo >= 0 && level_lo < level_hi && level_hi <= N, "level out of range");
  PSA_REQUIRE(cand >= 1 && cand <= nnz, "candidate count out of range");
  hipStream_t s = psa::as_stream(stream);
  const int64_t F = level_hi - level_lo, tiles = psa::ceil_div(cand, kTile);
  hipLaunchKernelGGL(rcm_frontier_deg_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr, w.order, level_lo,
                     F, w.buf, state);
  PSA_LAUNCH_CHECK();
  st = psa_count2ptr(w.buf, F, w.fptr, w.scan, w.scan_bytes, stream);
  if (st != PSA_OK) return st;
  const dim3 grid(static_cast<unsigned>(tiles));
  hipLaunchKernelGGL(rcm_claim_kernel, grid, dim3(kThreads), 0, s, rowptr, col, N, w.order, level_lo, F, w.fptr,
                     w.rank, w.claim);
  hipLaunchKernelGGL(rcm_count_kernel, grid, dim3(kThreads), 0, s, rowptr, col, N, w.order, level_lo, F, w.fptr,
                     w.rank, w.claim, w.tile_counts, state);
  PSA_LAUNCH_CHECK();
  st = psa_count2ptr(w.tile_counts, tiles, w.tile_ptr, w.scan, w.scan_bytes, stream);
  if (st != PSA_OK) return st;
  hipLaunchKernelGGL(rcm_info_kernel, dim3(1), dim3(1), 0, s, w.tile_ptr, tiles, state);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_rcm_level_write(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t level_lo,
                        int64_t level_hi, int64_t cand, int64_t n_new, int64_t max_deg, void* workspace,
                        size_t workspace_bytes, int64_t* state, psa_stream_t stream) {
  RcmWs w;
  int st = rcm_args(__func__, N, nnz, workspace, workspace_bytes, &w);
  if (st != PSA_OK) return st;
  PSA_REQUIRE(rowptr && col && state, "NULL pointer");
  PSA_REQUIRE(level_lo >= 0 && level_lo < level_hi && level_hi <= N, "level out of range");
  PSA_REQUIRE(cand >= 1 && cand <= nnz && max_deg >= 1 && max_deg <= nnz, "candidate count or max_deg out of range");
  PSA_REQUIRE(n_new >= 0 && n_new <= N - level_hi && n_new <= cand,
              "more new nodes than unplaced ones (are the rows sorted?)");
  hipStream_t s = psa::as_stream(stream);
  const int64_t F = level_hi - level_lo, tiles = psa::ceil_div(cand, kTile), dstride = max_deg + 1;
  PSA_REQUIRE(dstride <= (int64_t{1} << 62) / F, "level key does not fit 62 bits");
  const uint32_t* fault = nullptr;
  if (n_new > 0) {
    hipLaunchKernelGGL(rcm_select_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kThreads), 0, s, rowptr, col, N,
                       w.order, level_lo, F, w.fptr, w.rank, w.claim, w.tile_ptr, n_new, dstride, w.keys, w.pay);
    PSA_LAUNCH_CHECK();
    st = psa_sort_pairs_u32(w.keys, w.pay, n_new, F * dstride, w.keys_out, w.pay_out, w.sort, w.sort_bytes, stream);
    if (st != PSA_OK) return st;
    fault = psa::sort_fault_word(w.sort, n_new, F * dstride);
  }
  hipLaunchKernelGGL(rcm_place_kernel, dim3(blocks_for(n_new)), dim3(kThreads), 0, s, w.pay_out, n_new, level_hi, N,
                     w.order, w.rank, state, fault);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_rcm_finish(int64_t N, int64_t nnz, const void* workspace, size_t workspace_bytes, int64_t* perm_out,
                   psa_stream_t stream) {
  RcmWs w;
  const int st = rcm_args(__func__, N, nnz, workspace, workspace_bytes, &w);
  if (st != PSA_OK) return st;
  PSA_REQUIRE(perm_out != nullptr, "perm_out is NULL");
  hipLaunchKernelGGL(rcm_reverse_kernel, dim3(blocks_for(N)), dim3(kThreads), 0, psa::as_stream(stream), w.order, N,
                     perm_out);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"
