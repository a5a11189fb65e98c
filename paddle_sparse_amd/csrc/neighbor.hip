// gfx950 only.
// neighbor_sample (torch_sparse neighbor_sample, the op behind PyG's NeighborLoader; CPU
// only upstream): multi-hop, layer-wise neighbour sampling of a square sorted CSR matrix
// with ONE relabel map for the whole call.
//
// n_id starts as the seeds; local id = position in n_id.  Hop l expands the nodes that
// hop l - 1 appended (the frontier, local ids [begin, end)), each node once per call.  A
// frontier node at local id i makes picks_of(deg, k_l, replace) picks by sample_adj's
// rules with the draws of rng.h on stream i, so one seed serves every hop.  Slot order
// within a hop is (frontier position, t); a picked column without a local id gets the
// next one in order of its first slot.
//
// Device state: local int32[N] in the caller's workspace (kUnseen, a local id >= 0, or
// -2 - p = provisional claim by slot p of the current hop), and the caller's state block.
//
//   init        fill local (fresh workspace only); one atomicMax(local[s], i) per seed,
//               re-read: local[s] != i -> duplicate flag; a seed outside -> flag, skipped
//   hop_count   (k < 0 only) frontier degrees; the caller scans them (psa_count2ptr) and
//               reads the slot count
//   hop_pick    one thread per slot p picks its entry e_raw[p] (k >= 0: p = f * k + t, the
//               grid covers the bound F * k and slots past a row's picks stay -1; k < 0:
//               a tile of kTile slots finds its rows by a wave search in the scanned
//               degrees and stages them in LDS, so a hub row spreads over many
//               workgroups), Floyd rows one thread per row (picks in registers up to
//               k = 32); every slot does one atomicMax(local[c], -2 - p): ids are >= 0
//               and stay, among claims the smallest slot wins whatever the arrival
//               order.  Then one word per slot,
//               valid << 32 | (local[c] == -2 - p), ONE psa_count2ptr over the words gives
//               both the edge position and the rank of every first pick, and
//               state = {E_l, new_l}: the host read
//   hop_write   id = end + rank[first slot] for a claimed column, n_id, (row', col', e);
//               local[c] = id in a pass of its own over the new nodes, so that the slot
//               pass never reads a word that another slot writes
//   reset       local[n_id[j]] = kUnseen for the touched entries: n stores instead of N
// No workgroup waits for another one; every loop is bounded by a degree, k or log2(F).
#include "common.h"
#include "rng.h"
#include "weighted_pick.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                  // slots per lane per tile (k < 0)
constexpr int kTile = kThreads * kPer;   // slots per workgroup (k < 0)
constexpr int kRows = 512;               // rows of a tile staged in LDS
constexpr int kFloydRegs = 32;           // largest fan-out whose Floyd picks stay in registers
constexpr int32_t kUnseen = INT32_MIN;
constexpr int64_t kMaxSlots = 0x7ffffff0;  // -2 - p must stay above kUnseen

// the caller's state block, int64[PSA_NEIGHBOR_STATE_WORDS]
enum { kEdges = 0, kNew, kFlags, kWords };
static_assert(kWords <= PSA_NEIGHBOR_STATE_WORDS, "state block");
constexpr unsigned long long kDupSeed = 1, kSeedOutside = 2, kColOutside = 4;

using psa::randint;

__device__ __forceinline__ int32_t ld32(const int32_t* p) {
  // L2-served: the line may sit in this CU's L1 from before an atomic of another wave
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void raise_flag(int64_t* state, unsigned long long bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(state + kFlags), bit);
}

__device__ inline int64_t picks_of(int64_t deg, int64_t k, int replace) {
  if (k < 0) return deg;
  if (replace) return deg > 0 ? k : 0;
  return deg < k ? deg : k;
}

// start and degree of frontier node v; a node outside the matrix (a bad seed: the flag is
// up and the call will raise) has no entries.
__device__ __forceinline__ void row_of(const int64_t* __restrict__ rowptr, int64_t N, int64_t v, int64_t* start,
                                       int64_t* deg) {
  if (static_cast<uint64_t>(v) >= static_cast<uint64_t>(N)) {
    *start = 0;
    *deg = 0;
    return;
  }
  *start = rowptr[v];
  *deg = rowptr[v + 1] - *start;
}

// Slot p picked entry e: claim its column.  Returns e, or -1 for a column outside [0, N).
__device__ __forceinline__ int64_t claim(const int64_t* __restrict__ col, int64_t N, int64_t e, int64_t p,
                                         int32_t* __restrict__ local, int64_t* __restrict__ state) {
  const int64_t c = col[e];
  if (static_cast<uint64_t>(c) >= static_cast<uint64_t>(N)) {
    raise_flag(state, kColOutside);
    return -1;
  }
  __hip_atomic_fetch_max(local + c, static_cast<int32_t>(-2 - p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return e;
}

__global__ void __launch_bounds__(kThreads)
neighbor_fill_kernel(int32_t* __restrict__ local, int64_t N) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < N; i += stride) local[i] = kUnseen;
}

__global__ void __launch_bounds__(kThreads)
neighbor_place_kernel(const int64_t* __restrict__ seeds, int64_t S, int64_t N, int32_t* __restrict__ local,
                      int64_t* __restrict__ state) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t s = seeds[i];
  if (static_cast<uint64_t>(s) >= static_cast<uint64_t>(N)) {
    raise_flag(state, kSeedOutside);
    return;
  }
  __hip_atomic_fetch_max(local + s, static_cast<int32_t>(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads)
neighbor_seed_check_kernel(const int64_t* __restrict__ seeds, int64_t S, int64_t N, const int32_t* __restrict__ local,
                           int64_t* __restrict__ state) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t s = seeds[i];
  if (static_cast<uint64_t>(s) >= static_cast<uint64_t>(N)) return;
  if (ld32(local + s) != static_cast<int32_t>(i)) raise_flag(state, kDupSeed);
}

__global__ void __launch_bounds__(kThreads)
neighbor_degree_kernel(const int64_t* __restrict__ rowptr, int64_t N, const int64_t* __restrict__ frontier, int64_t F,
                       int64_t* __restrict__ counts) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  counts[f] = deg;
}

// k >= 0, one thread per slot p = f * k + t of the bound F * k: every case except
// "without replacement, deg > k" (the Floyd rows, whose slots this kernel leaves alone).
__global__ void __launch_bounds__(kThreads)
neighbor_pick_slot_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                          const int64_t* __restrict__ frontier, int64_t begin, int64_t k, int replace, uint64_t seed,
                          int64_t cap, int32_t* __restrict__ local, int64_t* __restrict__ e_raw,
                          int64_t* __restrict__ state) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t f = p / k, t = p - f * k;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  if (!replace && deg > k) return;
  int64_t e = -1;
  if (t < picks_of(deg, k, replace)) {
    e = replace ? start + randint(seed, begin + f, t, deg) : start + t;
    e = claim(col, N, e, p, local, state);
  }
  e_raw[p] = e;
}

// Without replacement, deg > k: Floyd's walk exactly as sample_select_floyd_kernel does
// it, one thread per row.  k <= KMAX: the picks stay in registers (every index is static
// once the loops are unrolled), so a step does not wait for the previous step's store to
// come back from memory.
template <int KMAX>
__global__ void __launch_bounds__(kThreads)
neighbor_pick_floyd_reg_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                               const int64_t* __restrict__ frontier, int64_t F, int64_t begin, int64_t k,
                               uint64_t seed, int32_t* __restrict__ local, int64_t* __restrict__ e_raw,
                               int64_t* __restrict__ state) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  if (deg <= k) return;
  int64_t mine[KMAX];
  const uint64_t stream = psa::rand_stream(seed, begin + f);
#pragma unroll
  for (int t = 0; t < KMAX; ++t) {
    if (t < k) {
      const int64_t j = deg - k + t;  // > 0
      const int64_t pick = start + psa::rand_draw(stream, t, j);
      bool taken = false;
#pragma unroll
      for (int u = 0; u < t; ++u) taken |= mine[u] == pick;
      mine[t] = taken ? start + j : pick;
    }
  }
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < k) e_raw[f * k + t] = claim(col, N, mine[t], f * k + t, local, state);
}

// The same for k > kFloydRegs: the row's own slots double as the "already taken" set.
__global__ void __launch_bounds__(kThreads)
neighbor_pick_floyd_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                           const int64_t* __restrict__ frontier, int64_t F, int64_t begin, int64_t k, uint64_t seed,
                           int32_t* __restrict__ local, int64_t* __restrict__ e_raw, int64_t* __restrict__ state) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  if (deg <= k) return;
  int64_t* mine = e_raw + f * k;
  const uint64_t stream = psa::rand_stream(seed, begin + f);
  for (int64_t t = 0; t < k; ++t) {
    const int64_t j = deg - k + t;  // > 0
    int64_t pick = start + psa::rand_draw(stream, t, j);
    bool taken = false;
    for (int64_t u = 0; u < t && !taken; ++u) taken = mine[u] == pick;
    if (taken) pick = start + j;
    mine[t] = pick;
  }
  // claims after the walk: a column outside the matrix turns its slot into -1, which the
  // walk's comparisons must not see
  for (int64_t t = 0; t < k; ++t) mine[t] = claim(col, N, mine[t], f * k + t, local, state);
}

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

// k < 0: every stored entry of every frontier row, slot p = fptr[f] + t.  One tile of kTile
// slots per workgroup; its rows [r_lo, r_hi] come from two wave searches and are staged
// in LDS (searched in global memory when more than kRows rows, a run of empty rows, fall
// into the tile).
__global__ void __launch_bounds__(kThreads)
neighbor_pick_all_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                         const int64_t* __restrict__ frontier, int64_t F, const int64_t* __restrict__ fptr,
                         int64_t cap, int32_t* __restrict__ local, int64_t* __restrict__ e_raw,
                         int32_t* __restrict__ owner, int64_t* __restrict__ state) {
  __shared__ int64_t s_ptr[kRows], s_base[kRows], s_bounds[2];
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const int64_t p1 = cap - p0 < kTile ? cap : p0 + kTile;
  const int wave = threadIdx.x >> 6;
  if (wave < 2) {
    const int64_t r = wave_search(fptr, 0, F, wave == 0 ? p0 : p1 - 1);
    if ((threadIdx.x & 63) == 0) s_bounds[wave] = r;
  }
  __syncthreads();
  const int64_t r_lo = s_bounds[0], nr = s_bounds[1] - r_lo + 1;
  const bool staged = nr <= kRows;
  if (staged) {
    for (int i = threadIdx.x; i < nr; i += kThreads) {
      int64_t start, deg;
      row_of(rowptr, N, frontier[r_lo + i], &start, &deg);
      const int64_t q = fptr[r_lo + i];
      s_ptr[i] = q;
      s_base[i] = start - q;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t p = p0 + j * kThreads + threadIdx.x;
    if (p >= p1) continue;
    int64_t r, base;
    if (staged) {
      int lo = 0, hi = static_cast<int>(nr);
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_ptr[mid] <= p) lo = mid;
        else hi = mid;
      }
      r = r_lo + lo;
      base = s_base[lo];
    } else {
      int64_t lo = r_lo, hi = r_lo + nr;
      while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (fptr[mid] <= p) lo = mid;
        else hi = mid;
      }
      r = lo;
      base = rowptr[frontier[r]] - fptr[r];  // the row has slot p, so the node is inside
    }
    owner[p] = static_cast<int32_t>(r);
    e_raw[p] = claim(col, N, p + base, p, local, state);
  }
}

// word[p] = valid << 32 | first: one scan of the words yields the edge position (high
// half) and the rank among the first picks (low half) of every slot.
__global__ void __launch_bounds__(kThreads)
neighbor_flags_kernel(const int64_t* __restrict__ col, const int64_t* __restrict__ e_raw, int64_t cap,
                      const int32_t* __restrict__ local, int64_t* __restrict__ word) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t e = e_raw[p];
  int64_t w = 0;
  if (e >= 0) w = (int64_t{1} << 32) | (ld32(local + col[e]) == static_cast<int32_t>(-2 - p) ? 1 : 0);
  word[p] = w;
}

__global__ void neighbor_state_kernel(const int64_t* __restrict__ ptr, int64_t cap, int64_t* __restrict__ state) {
  const int64_t total = ptr[cap];
  state[kEdges] = total >> 32;
  state[kNew] = total & 0xffffffff;
}

__global__ void __launch_bounds__(kThreads)
neighbor_write_kernel(const int64_t* __restrict__ col, const int64_t* __restrict__ e_raw,
                      const int32_t* __restrict__ owner, const int64_t* __restrict__ ptr, int64_t cap, int64_t k,
                      int64_t begin, int64_t end, const int32_t* __restrict__ local, int64_t* __restrict__ n_id_new,
                      int64_t* __restrict__ row_out, int64_t* __restrict__ col_out, int64_t* __restrict__ edge_out) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t e = e_raw[p];
  if (e < 0) return;
  const int64_t c = col[e];
  const int32_t v = ld32(local + c);
  int64_t id = v;
  if (v < 0) {
    const int64_t first = -2 - static_cast<int64_t>(v);  // slot of the first pick of c
    const int64_t rank = ptr[first] & 0xffffffff;
    id = end + rank;
    if (first == p) n_id_new[rank] = c;
  }
  if (row_out == nullptr) return;  // the caller wants the node set only
  const int64_t q = ptr[p] >> 32;
  row_out[q] = begin + (k >= 0 ? p / k : static_cast<int64_t>(owner[p]));
  col_out[q] = id;
  edge_out[q] = e;
}

__global__ void __launch_bounds__(kThreads)
neighbor_finalise_kernel(const int64_t* __restrict__ n_id_new, int64_t n_new, int64_t end,
                         int32_t* __restrict__ local) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (j < n_new) local[n_id_new[j]] = static_cast<int32_t>(end + j);
}

// threads [0, n): listed nodes; threads [n, n + cap): the columns the slots of an
// abandoned hop claimed.
__global__ void __launch_bounds__(kThreads)
neighbor_reset_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t N, const int64_t* __restrict__ col,
                      const int64_t* __restrict__ e_raw, int64_t cap, int32_t* __restrict__ local) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g < n) {
    const int64_t v = ids[g];
    if (static_cast<uint64_t>(v) < static_cast<uint64_t>(N)) local[v] = kUnseen;
  } else if (g < n + cap) {
    const int64_t e = e_raw[g - n];
    if (e >= 0) local[col[e]] = kUnseen;
  }
}

unsigned blocks_for(int64_t n, int per = kThreads) {
  return static_cast<unsigned>(psa::ceil_div(n > 0 ? n : 1, per));
}

// hop scratch: e_raw int64[cap] | word int64[cap] | ptr int64[cap+1] | owner int32[cap] | count2ptr scratch
struct HopWs {
  int64_t *e_raw, *word, *ptr;
  int32_t* owner;
  void* scan;
  size_t scan_bytes;
};

size_t hop_layout(int64_t cap, char* base, HopWs* ws) {
  psa::Carver c(base);
  const size_t n = static_cast<size_t>(cap > 0 ? cap : 1);
  HopWs w;
  w.e_raw = c.take<int64_t>(n, 16);
  w.word = c.take<int64_t>(n, 16);
  w.ptr = c.take<int64_t>(n + 1, 16);
  w.owner = c.take<int32_t>(n, 16);
  w.scan_bytes = psa_count2ptr_workspace_bytes(static_cast<int64_t>(n));
  w.scan = c.take<char>(w.scan_bytes, 16);
  if (ws) *ws = w;
  return c.off;
}

bool in_range(int64_t N) { return N >= 0 && N < (int64_t{1} << 31); }

}  // namespace

extern "C" {

size_t psa_neighbor_workspace_bytes(int64_t N) {
  if (!in_range(N)) return 0;
  psa::Carver c(nullptr);  // one region: the label of every node, int32[N]
  c.take<int32_t>(static_cast<size_t>(N > 0 ? N : 1), 16);
  return c.off;
}

size_t psa_neighbor_hop_workspace_bytes(int64_t slots) {
  return slots >= 0 && slots <= kMaxSlots ? hop_layout(slots, nullptr, nullptr) : 0;
}

int psa_neighbor_init(const int64_t* seeds, int64_t S, int64_t N, int fresh, void* workspace, size_t workspace_bytes,
                      int64_t* state, psa_stream_t stream) {
  PSA_REQUIRE(in_range(N) && S >= 0 && S < (int64_t{1} << 31), "N and S must lie in [0, 2^31)");
  PSA_REQUIRE(state && (seeds || S == 0), "NULL pointer");
  if (workspace == nullptr || workspace_bytes < psa_neighbor_workspace_bytes(N)) {
    psa::set_error("psa_neighbor_init: workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  hipStream_t s = psa::as_stream(stream);
  auto* local = static_cast<int32_t*>(workspace);
  PSA_ZERO(state, sizeof(int64_t) * PSA_NEIGHBOR_STATE_WORDS, s);
  if (fresh && N > 0) {
    const unsigned blocks = blocks_for(N);
    hipLaunchKernelGGL(neighbor_fill_kernel, dim3(blocks > 8192 ? 8192 : blocks), dim3(kThreads), 0, s, local, N);
  }
  if (S > 0) {
    hipLaunchKernelGGL(neighbor_place_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, s, seeds, S, N, local, state);
    hipLaunchKernelGGL(neighbor_seed_check_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, s, seeds, S, N, local,
                       state);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_neighbor_hop_count(const int64_t* rowptr, int64_t N, const int64_t* frontier, int64_t F, int64_t* counts,
                           psa_stream_t stream) {
  PSA_REQUIRE(in_range(N) && F >= 0 && F < (int64_t{1} << 31), "N and F must lie in [0, 2^31)");
  if (F == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && frontier && counts, "NULL pointer");
  hipLaunchKernelGGL(neighbor_degree_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, psa::as_stream(stream), rowptr, N,
                     frontier, F, counts);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_neighbor_hop_pick(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* frontier, int64_t F,
                          const int64_t* frontier_ptr, int64_t begin, int64_t num_neighbors, int replace,
                          uint64_t seed, int64_t slots, void* workspace, void* hop_workspace,
                          size_t hop_workspace_bytes, int64_t* state, psa_stream_t stream) {
  const int64_t k = num_neighbors;
  PSA_REQUIRE(in_range(N) && F >= 1 && begin >= 0 && begin + F < (int64_t{1} << 31), "frontier out of range");
  PSA_REQUIRE(slots >= 1 && slots <= kMaxSlots, "slot count out of range");
  PSA_REQUIRE(k != 0 && (k < 0 || slots == F * k), "slots must be F * num_neighbors when num_neighbors >= 0");
  PSA_REQUIRE(rowptr && col && frontier && workspace && state && (k >= 0 || frontier_ptr), "NULL pointer");
  if (hop_workspace == nullptr || hop_workspace_bytes < psa_neighbor_hop_workspace_bytes(slots)) {
    psa::set_error("psa_neighbor_hop_pick: hop workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  hipStream_t s = psa::as_stream(stream);
  auto* local = static_cast<int32_t*>(workspace);
  HopWs w;
  hop_layout(slots, static_cast<char*>(hop_workspace), &w);
  if (k >= 0) {
    hipLaunchKernelGGL(neighbor_pick_slot_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, rowptr, col, N,
                       frontier, begin, k, replace, seed, slots, local, w.e_raw, state);
    if (!replace && k <= kFloydRegs)
      hipLaunchKernelGGL(neighbor_pick_floyd_reg_kernel<kFloydRegs>, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr,
                         col, N, frontier, F, begin, k, seed, local, w.e_raw, state);
    else if (!replace)
      hipLaunchKernelGGL(neighbor_pick_floyd_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr, col, N,
                         frontier, F, begin, k, seed, local, w.e_raw, state);
  } else {
    hipLaunchKernelGGL(neighbor_pick_all_kernel, dim3(blocks_for(slots, kTile)), dim3(kThreads), 0, s, rowptr, col, N,
                       frontier, F, frontier_ptr, slots, local, w.e_raw, w.owner, state);
  }
  hipLaunchKernelGGL(neighbor_flags_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, col, w.e_raw, slots, local,
                     w.word);
  PSA_LAUNCH_CHECK();
  const int st = psa_count2ptr(w.word, slots, w.ptr, w.scan, w.scan_bytes, stream);
  if (st != PSA_OK) return st;
  hipLaunchKernelGGL(neighbor_state_kernel, dim3(1), dim3(1), 0, s, w.ptr, slots, state);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_neighbor_hop_write(const int64_t* col, int64_t begin, int64_t end, int64_t num_neighbors, int64_t slots,
                           int64_t n_edges, int64_t n_new, void* workspace, const void* hop_workspace,
                           int64_t* n_id_new, int64_t* row_out, int64_t* col_out, int64_t* edge_out,
                           psa_stream_t stream) {
  PSA_REQUIRE(begin >= 0 && begin < end && num_neighbors != 0, "frontier out of range");
  PSA_REQUIRE(slots >= 1 && slots <= kMaxSlots, "slot count out of range");
  PSA_REQUIRE(n_edges >= 0 && n_edges <= slots && n_new >= 0 && n_new <= n_edges &&
                  end + n_new < (int64_t{1} << 31),
              "n_edges and n_new must be the values read after psa_neighbor_hop_pick");
  if (n_edges == 0) return PSA_OK;
  PSA_REQUIRE(col && workspace && hop_workspace && (n_id_new || n_new == 0), "NULL pointer");
  PSA_REQUIRE((row_out && col_out && edge_out) || (!row_out && !col_out && !edge_out),
              "row_out, col_out and edge_out are given together or not at all");
  hipStream_t s = psa::as_stream(stream);
  auto* local = static_cast<int32_t*>(workspace);
  HopWs w;
  hop_layout(slots, static_cast<char*>(const_cast<void*>(hop_workspace)), &w);
  hipLaunchKernelGGL(neighbor_write_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, col, w.e_raw, w.owner,
                     w.ptr, slots, num_neighbors, begin, end, local, n_id_new, row_out, col_out, edge_out);
  if (n_new > 0)
    hipLaunchKernelGGL(neighbor_finalise_kernel, dim3(blocks_for(n_new)), dim3(kThreads), 0, s, n_id_new, n_new, end,
                       local);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_neighbor_reset(const int64_t* ids, int64_t n, int64_t N, const int64_t* col, const void* hop_workspace,
                       int64_t slots, void* workspace, psa_stream_t stream) {
  PSA_REQUIRE(in_range(N) && n >= 0 && slots >= 0 && slots <= kMaxSlots, "size out of range");
  if (n + slots == 0) return PSA_OK;
  PSA_REQUIRE(workspace && (ids || n == 0) && ((col && hop_workspace) || slots == 0), "NULL pointer");
  HopWs w{};
  if (slots > 0) hop_layout(slots, static_cast<char*>(const_cast<void*>(hop_workspace)), &w);
  hipLaunchKernelGGL(neighbor_reset_kernel, dim3(blocks_for(n + slots)), dim3(kThreads), 0, psa::as_stream(stream),
                     ids, n, N, col, w.e_raw, slots, static_cast<int32_t*>(workspace));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"

// ---- weighted picks: psa_neighbor_hop_pick with every pick of a hop with
// num_neighbors >= 0 drawn in proportion to the entries' weights, from the row CDF `cum`.
// Only the pick kernels differ; claims, flags, the scan and psa_neighbor_hop_write are the
// chain above.  Without replacement one thread walks one frontier row (weighted_pick.h):
// slot f * k + t holds draw t, the slots past the row's picks hold -1; up to kWeightedRegs
// draws the taken positions and the gap masses stay in registers, beyond that the row's
// slots of e_raw hold the picks in draw order and its slots of `word` (written by the flags
// pass only afterwards) the ascending view.  Claims run after the walk.
namespace {

constexpr int kWeightedRegs = 32;   // largest fan-out walked in registers
constexpr int kWeightedSmall = 16;  // the instantiations for fan-outs up to 16 and up to 8: fewer registers,
constexpr int kWeightedTiny = 8;    // more waves in flight over the binary searches

struct StreamWords {  // the words of stream st for a fan-out of k: entry(t) is the uniform draw's word
  uint64_t st, k;
  __host__ __device__ uint64_t entry(int64_t t) const { return psa::mix64(st + static_cast<uint64_t>(t)); }
  __host__ __device__ uint64_t gap(int64_t t) const { return psa::mix64(st + k + static_cast<uint64_t>(t)); }
};

// KMAX > 0: k <= KMAX, walked in registers (a row of 2^31 entries or more takes the memory walk).
template <int KMAX>
__global__ void __launch_bounds__(kThreads)
neighbor_pick_weighted_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                              const double* __restrict__ cum, int64_t N, const int64_t* __restrict__ frontier,
                              int64_t F, int64_t begin, int64_t k, uint64_t seed, int32_t* __restrict__ local,
                              int64_t* __restrict__ e_raw, int64_t* __restrict__ sorted,
                              int64_t* __restrict__ state) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  int64_t* mine = e_raw + f * k;
  const StreamWords words{psa::rand_stream(seed, begin + f), static_cast<uint64_t>(k)};
  int64_t count = 0;
  if (deg > 0) {
    bool walked = false;
    if constexpr (KMAX > 0) {
      if (deg <= INT32_MAX) {
        count = psa::weighted_pick_without_small<KMAX>(cum + start, deg, k, words, mine);
        walked = true;
      }
    }
    if (!walked) count = psa::weighted_pick_without_large(cum + start, deg, k, words, sorted + f * k, mine);
  }
  for (int64_t t = 0; t < k; ++t)
    mine[t] = t < count ? claim(col, N, start + mine[t], f * k + t, local, state) : -1;
}

// With replacement: one thread per slot, the pick of the weighted walk and weighted sample_adj.
__global__ void __launch_bounds__(kThreads)
neighbor_pick_weighted_slot_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                   const double* __restrict__ cum, int64_t N, const int64_t* __restrict__ frontier,
                                   int64_t begin, int64_t k, uint64_t seed, int64_t cap, int32_t* __restrict__ local,
                                   int64_t* __restrict__ e_raw, int64_t* __restrict__ state) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t f = p / k, t = p - f * k;
  int64_t start, deg;
  row_of(rowptr, N, frontier[f], &start, &deg);
  int64_t e = -1;
  if (deg > 0) {
    const int64_t pick =
        psa::weighted_pick(cum + start, deg, psa::mix64(psa::rand_stream(seed, begin + f) + static_cast<uint64_t>(t)));
    if (pick >= 0) e = claim(col, N, start + pick, p, local, state);
  }
  e_raw[p] = e;
}

}  // namespace

extern "C" {

int64_t psa_weighted_pick_without_host(const double* cum, int64_t deg, int64_t k, const uint64_t* words_entry,
                                       const uint64_t* words_gap, int64_t* out) {
  if (cum == nullptr || words_entry == nullptr || words_gap == nullptr || out == nullptr || deg <= 0 || k <= 0) return 0;
  const psa::PickWordArrays words{words_entry, words_gap};
  int64_t count;
  if (k <= kWeightedTiny && deg <= INT32_MAX) {
    count = psa::weighted_pick_without_small<kWeightedTiny>(cum, deg, k, words, out);
  } else if (k <= kWeightedSmall && deg <= INT32_MAX) {
    count = psa::weighted_pick_without_small<kWeightedSmall>(cum, deg, k, words, out);
  } else if (k <= kWeightedRegs && deg <= INT32_MAX) {
    count = psa::weighted_pick_without_small<kWeightedRegs>(cum, deg, k, words, out);
  } else {
    int64_t* sorted = new int64_t[static_cast<size_t>(k)];
    count = psa::weighted_pick_without_large(cum, deg, k, words, sorted, out);
    delete[] sorted;
  }
  for (int64_t t = count; t < k; ++t) out[t] = -1;
  return count;
}

int psa_neighbor_hop_pick_weighted(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                                   const int64_t* frontier, int64_t F, const int64_t* frontier_ptr, int64_t begin,
                                   int64_t num_neighbors, int replace, uint64_t seed, int64_t slots, void* workspace,
                                   void* hop_workspace, size_t hop_workspace_bytes, int64_t* state,
                                   psa_stream_t stream) {
  const int64_t k = num_neighbors;
  (void)frontier_ptr;  // read by the unweighted entry point when num_neighbors < 0 only
  PSA_REQUIRE(in_range(N) && F >= 1 && begin >= 0 && begin + F < (int64_t{1} << 31), "frontier out of range");
  PSA_REQUIRE(slots >= 1 && slots <= kMaxSlots, "slot count out of range");
  PSA_REQUIRE(k >= 1 && slots == F * k, "num_neighbors must be >= 1 and slots F * num_neighbors");
  PSA_REQUIRE(rowptr && col && cum && frontier && workspace && state, "NULL pointer");
  if (hop_workspace == nullptr || hop_workspace_bytes < psa_neighbor_hop_workspace_bytes(slots)) {
    psa::set_error("psa_neighbor_hop_pick_weighted: hop workspace too small");
    return PSA_ERR_WORKSPACE;
  }
  hipStream_t s = psa::as_stream(stream);
  auto* local = static_cast<int32_t*>(workspace);
  HopWs w;
  hop_layout(slots, static_cast<char*>(hop_workspace), &w);
#define PSA_PICK_ROWS(KMAX)                                                                                      \
  hipLaunchKernelGGL(neighbor_pick_weighted_kernel<KMAX>, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr, col, \
                     cum, N, frontier, F, begin, k, seed, local, w.e_raw, w.word, state)
  if (replace)
    hipLaunchKernelGGL(neighbor_pick_weighted_slot_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, rowptr, col,
                       cum, N, frontier, begin, k, seed, slots, local, w.e_raw, state);
  else if (k <= kWeightedTiny) PSA_PICK_ROWS(kWeightedTiny);
  else if (k <= kWeightedSmall) PSA_PICK_ROWS(kWeightedSmall);
  else if (k <= kWeightedRegs) PSA_PICK_ROWS(kWeightedRegs);
  else PSA_PICK_ROWS(0);
#undef PSA_PICK_ROWS
  hipLaunchKernelGGL(neighbor_flags_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, col, w.e_raw, slots, local,
                     w.word);
  PSA_LAUNCH_CHECK();
  const int st = psa_count2ptr(w.word, slots, w.ptr, w.scan, w.scan_bytes, stream);
  if (st != PSA_OK) return st;
  hipLaunchKernelGGL(neighbor_state_kernel, dim3(1), dim3(1), 0, s, w.ptr, slots, state);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"
