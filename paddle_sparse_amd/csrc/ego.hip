// gfx950 only.
// ego_k_hop_sample (torch_sparse ego_k_hop_sample_adj, the op behind PyG's ShaDowKHopSampler):
// every seed gets a k-hop neighbourhood of its own and the subgraphs induced on them come
// back as one block-diagonal matrix.
//
// Walk list: one global sequence of entries, entry i < S is seed i and belongs to ego i.
// Hop l expands EVERY entry of hop l - 1, duplicates included; a child belongs to its
// parent's ego.  The parent at walk index i holding node v makes sample_adj's picks for
// (deg(v), k, replace) on stream i of `seed`.  k >= 0: the hop has F * k slots, slot
// f * k + t is pick t of parent f, a slot past its parent's picks (or of an empty parent) is
// empty: node -1, and it stays empty in later hops.  k < 0: the slots are the entries of the
// parents' rows in (parent, storage) order, all valid.
//
// Every slot writes three words: node (or -1), ego, and the sort key ego * N + node.  An
// empty slot takes the key of its ego's seed, a key that entry `ego` of the walk list holds
// already, so that the distinct keys are exactly the node sets and nothing is compacted or
// cut off.  No relabel map: the caller sorts the keys, takes the distinct ones (n_id, and
// the ego of every local row) and builds ptr with psa_ind2ptr.
//
//   init          node, ego, key of the seeds; a seed outside [0, N) raises a flag and is empty
//   hop_count     (k < 0 only) the parents' degrees; the caller scans them (psa_count2ptr) and
//                 reads the slot count
//   hop_pick      k >= 0: one thread per slot (all entries, or draws with replacement); Floyd
//                 rows (no replacement, deg > k) one thread per parent in a launch of their
//                 own, picks in registers up to k = 32, in the row's own node slots above.
//                 k < 0: one thread per slot, the parent found by a search in the scanned degrees
//   induce_count  root[g] = position of (g, seeds[g]); counts[r] = matches of local row r
//   induce_write  the same traversal, (col', e) placed by ballot and prefix popcount
//
// Induce: local row r = (g, v) intersects the adjacency row of v (deg entries, ascending,
// equal columns allowed) with its ego's list n_id[ptr[g], ptr[g+1]) (n_g nodes, ascending,
// distinct).  The shorter side probes the longer by binary search, TIE: THE ROW PROBES
// (deg <= n_g).  Each lane's probe elements ascend, so a search resumes where the last one
// ended.  When the list probes the row a hit is the lower bound and the whole run of equal
// columns is emitted in storage order; either direction emits the same entries in storage
// order.  A probe side of at most T elements is run by a group of 8 lanes (8 rows per wave);
// longer ones are deferred by a ballot and run by the whole wave afterwards, one at a time.
// Inside a pass lane l takes probe elements l, l + W, ...; the W elements of one step are
// placed by a ballot and a prefix popcount (a prefix sum over the lanes when a run is longer
// than one), so the order inside a row is the traversal's.  No workgroup waits for another,
// no atomics except the flag word, no search leaves the ego's segment; every loop is
// bounded by k, a degree or a log.
#include <atomic>

#include "common.h"
#include "rng.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / psa::kWave;
constexpr int kGroup = 8;
constexpr int kRowsPerWave = psa::kWave / kGroup;
constexpr int kFloydRegs = 32;
constexpr int64_t kMaxSlots = 0x7ffffff0;
constexpr int64_t kMaxBlocks = 65536;
constexpr unsigned long long kSeedOutside = PSA_EGO_SEED_OUTSIDE, kColOutside = PSA_EGO_COL_OUTSIDE;

std::atomic<int> g_threshold{32};  // probe sides LONGER than this take the whole wave

__device__ __forceinline__ void raise_flag(int64_t* flags, unsigned long long bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(flags), bit);
}

__device__ __forceinline__ int64_t picks_of(int64_t deg, int64_t k, int replace) {
  if (replace) return deg > 0 ? k : 0;
  return deg < k ? deg : k;
}

// start and degree of the row of node v; an empty entry (-1) has no entries
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

// the node that stands in for an empty slot of ego g: its seed (0 for a seed outside: the flag is up)
__device__ __forceinline__ int64_t seed_of(const int64_t* __restrict__ seeds, int64_t N, int64_t g) {
  const int64_t s = seeds[g];
  return static_cast<uint64_t>(s) < static_cast<uint64_t>(N) ? s : 0;
}

// Slot p of ego g picked entry e (or none: e < 0): node and key of the slot.
__device__ __forceinline__ void emit(const int64_t* __restrict__ col, const int64_t* __restrict__ seeds, int64_t N,
                                     int64_t e, int64_t g, int64_t p, int64_t* __restrict__ node_out,
                                     int64_t* __restrict__ key_out, int64_t* __restrict__ flags) {
  int64_t c = -1;
  if (e >= 0) {
    c = col[e];
    if (static_cast<uint64_t>(c) >= static_cast<uint64_t>(N)) {
      raise_flag(flags, kColOutside);
      c = -1;
    }
  }
  node_out[p] = c;
  key_out[p] = g * N + (c >= 0 ? c : seed_of(seeds, N, g));
}

__global__ void __launch_bounds__(kThreads)
ego_init_kernel(const int64_t* __restrict__ seeds, int64_t S, int64_t N, int64_t* __restrict__ node_out,
                int32_t* __restrict__ ego_out, int64_t* __restrict__ key_out, int64_t* __restrict__ flags) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= S) return;
  const int64_t s = seeds[i];
  const bool ok = static_cast<uint64_t>(s) < static_cast<uint64_t>(N);
  if (!ok) raise_flag(flags, kSeedOutside);
  node_out[i] = ok ? s : -1;
  ego_out[i] = static_cast<int32_t>(i);
  key_out[i] = i * N + (ok ? s : 0);
}

// k >= 0, one thread per slot p = f * k + t: the ego of every slot, and node and key of every
// case except "without replacement, deg > k" (the Floyd rows).
__global__ void __launch_bounds__(kThreads)
ego_pick_slot_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                     const int64_t* __restrict__ seeds, const int64_t* __restrict__ pnode,
                     const int32_t* __restrict__ pego, int64_t begin, int64_t k, int replace, uint64_t seed,
                     int64_t cap, int64_t* __restrict__ node_out, int32_t* __restrict__ ego_out,
                     int64_t* __restrict__ key_out, int64_t* __restrict__ flags) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t f = p / k, t = p - f * k;
  const int32_t g = pego[f];
  ego_out[p] = g;
  int64_t start, deg;
  row_of(rowptr, N, pnode[f], &start, &deg);
  if (!replace && deg > k) return;
  int64_t e = -1;
  if (t < picks_of(deg, k, replace)) e = replace ? start + psa::randint(seed, begin + f, t, deg) : start + t;
  emit(col, seeds, N, e, g, p, node_out, key_out, flags);
}

// Without replacement, deg > k: Floyd's walk as sample_adj does it, one thread per parent,
// the picks in registers.
template <int KMAX>
__global__ void __launch_bounds__(kThreads)
ego_pick_floyd_reg_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                          const int64_t* __restrict__ seeds, const int64_t* __restrict__ pnode,
                          const int32_t* __restrict__ pego, int64_t F, int64_t begin, int64_t k, uint64_t seed,
                          int64_t* __restrict__ node_out, int64_t* __restrict__ key_out,
                          int64_t* __restrict__ flags) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, pnode[f], &start, &deg);
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
  const int32_t g = pego[f];
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < k) emit(col, seeds, N, mine[t], g, f * k + t, node_out, key_out, flags);
}

// The same for k > kFloydRegs: the parent's own node slots hold the picked entries during the walk.
__global__ void __launch_bounds__(kThreads)
ego_pick_floyd_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                      const int64_t* __restrict__ seeds, const int64_t* __restrict__ pnode,
                      const int32_t* __restrict__ pego, int64_t F, int64_t begin, int64_t k, uint64_t seed,
                      int64_t* __restrict__ node_out, int64_t* __restrict__ key_out, int64_t* __restrict__ flags) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, pnode[f], &start, &deg);
  if (deg <= k) return;
  int64_t* mine = node_out + f * k;
  const uint64_t stream = psa::rand_stream(seed, begin + f);
  for (int64_t t = 0; t < k; ++t) {
    const int64_t j = deg - k + t;  // > 0
    int64_t pick = start + psa::rand_draw(stream, t, j);
    bool taken = false;
    for (int64_t u = 0; u < t && !taken; ++u) taken = mine[u] == pick;
    if (taken) pick = start + j;
    mine[t] = pick;
  }
  // entries become nodes after the walk, whose comparisons must see entries only
  const int32_t g = pego[f];
  for (int64_t t = 0; t < k; ++t) emit(col, seeds, N, mine[t], g, f * k + t, node_out, key_out, flags);
}

// k < 0: slot p is entry p - pptr[r] of the row of parent r, r = the largest index with pptr[r] <= p.
__global__ void __launch_bounds__(kThreads)
ego_pick_all_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N,
                    const int64_t* __restrict__ seeds, const int64_t* __restrict__ pnode,
                    const int32_t* __restrict__ pego, int64_t F, const int64_t* __restrict__ pptr, int64_t cap,
                    int64_t* __restrict__ node_out, int32_t* __restrict__ ego_out, int64_t* __restrict__ key_out,
                    int64_t* __restrict__ flags) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  int64_t lo = 0, hi = F;  // pptr[0] = 0 <= p < cap = pptr[F]
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  const int32_t g = pego[lo];
  ego_out[p] = g;
  int64_t start, deg;
  row_of(rowptr, N, pnode[lo], &start, &deg);
  const int64_t t = p - pptr[lo];
  emit(col, seeds, N, t < deg ? start + t : -1, g, p, node_out, key_out, flags);
}

__global__ void __launch_bounds__(kThreads)
ego_degree_kernel(const int64_t* __restrict__ rowptr, int64_t N, const int64_t* __restrict__ pnode, int64_t F,
                  int64_t* __restrict__ counts) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(rowptr, N, pnode[f], &start, &deg);
  counts[f] = deg;
}

__global__ void __launch_bounds__(kThreads)
ego_root_kernel(const int64_t* __restrict__ n_id, const int64_t* __restrict__ ptr, const int64_t* __restrict__ seeds,
                int64_t S, int64_t* __restrict__ root) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= S) return;
  const int64_t s = seeds[g], end = ptr[g + 1];
  int64_t lo = ptr[g], hi = end;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (n_id[mid] < s) lo = mid + 1;
    else hi = mid;
  }
  root[g] = lo < end && n_id[lo] == s ? lo : -1;
}

__global__ void ego_total_kernel(const int64_t* __restrict__ rowptr_out, int64_t n, const int64_t* __restrict__ flags,
                                 int64_t* __restrict__ state) {
  state[0] = rowptr_out[n];
  state[1] = *flags;
}

// One local row as its probe and search sides see it.
struct Row {
  const int64_t* pidx;  // probe side
  const int64_t* sidx;  // searched side
  int64_t np, ns;
  int64_t e0;     // storage position of the adjacency row's first entry
  int64_t c0;     // ptr[g]: local id of the ego's first node
  int64_t out0;   // rowptr'[r] (write pass)
  int row_probes;
};

template <int W>
__device__ __forceinline__ int64_t group_sum(int64_t x) {
#pragma unroll
  for (int off = 1; off < W; off <<= 1) x += __shfl_xor(static_cast<long long>(x), off);
  return x;
}

// Steps [0, steps) of a row on W lanes, lane l of the group taking probe elements l, l + W, ...
// `steps` is uniform over the wave (the ballots and shuffles are reached by every lane); a lane
// past its row's probe side has no element.  Returns this lane's matches (the count pass folds them).
template <int W, bool WRITE>
__device__ __forceinline__ int64_t traverse(const Row& row, int64_t steps, int lane, int64_t* __restrict__ col_out,
                                            int64_t* __restrict__ e_out) {
  const int l = lane & (W - 1);
  int64_t lo = 0, mine = 0, done = 0;
  for (int64_t step = 0; step < steps; ++step) {
    const int64_t i = step * W + l;
    int64_t cnt = 0;
    if (i < row.np) {
      const int64_t k = row.pidx[i];
      int64_t hi = row.ns;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row.sidx[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      if (lo < row.ns && row.sidx[lo] == k) {
        cnt = 1;
        if (!row.row_probes)  // the run of equal columns that starts at the lower bound
          while (lo + cnt < row.ns && row.sidx[lo + cnt] == k) ++cnt;
      }
    }
    if constexpr (!WRITE) {
      mine += cnt;
    } else {
      const unsigned long long hits = __ballot(cnt > 0);
      int64_t before, total;
      if (__ballot(cnt > 1) == 0) {
        const unsigned long long bits = W == 64 ? hits : (hits >> (lane & ~(W - 1))) & ((1ull << (W & 63)) - 1);
        before = __popcll(bits & ((1ull << l) - 1));
        total = __popcll(bits);
      } else {
        int64_t incl = cnt;
#pragma unroll
        for (int off = 1; off < W; off <<= 1) {
          const int64_t up = __shfl_up(static_cast<long long>(incl), off, W);
          if (l >= off) incl += up;
        }
        before = incl - cnt;
        total = __shfl(static_cast<long long>(incl), W - 1, W);
      }
      const int64_t q = row.out0 + done + before;
      if (cnt > 0 && row.row_probes) {
        col_out[q] = row.c0 + lo;
        e_out[q] = row.e0 + i;
      } else {
        for (int64_t j = 0; j < cnt; ++j) {
          col_out[q + j] = row.c0 + i;
          e_out[q + j] = row.e0 + lo + j;
        }
      }
      done += total;
    }
  }
  return mine;
}

__device__ __forceinline__ int64_t bcast(int64_t x, int src) {
  return static_cast<int64_t>(__shfl(static_cast<long long>(x), src));
}

template <typename P>
__device__ __forceinline__ P* bcast_ptr(P* p, int src) {
  return reinterpret_cast<P*>(__shfl(static_cast<long long>(reinterpret_cast<uintptr_t>(p)), src));
}

template <bool WRITE>
__global__ void __launch_bounds__(kThreads)
ego_induce_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, const int64_t* __restrict__ n_id,
                  const int64_t* __restrict__ ego_of, const int64_t* __restrict__ ptr, int64_t n, int64_t S,
                  int64_t N, int64_t T, const int64_t* __restrict__ rowptr_out, int64_t* __restrict__ counts,
                  int64_t* __restrict__ col_out, int64_t* __restrict__ e_out) {
  const int lane = threadIdx.x & (psa::kWave - 1);
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t tiles = (n + kRowsPerWave - 1) / kRowsPerWave;
  for (int64_t tile = wave; tile < tiles; tile += waves) {  // wave-uniform
    const int64_t r = tile * kRowsPerWave + (lane >> 3);
    Row row{nullptr, nullptr, 0, 0, 0, 0, 0, 1};
    if (r < n) {
      const int64_t g = ego_of[r], v = n_id[r];
      // the sorted keys put both inside; a row whose words are not is left empty
      if (static_cast<uint64_t>(g) < static_cast<uint64_t>(S) && static_cast<uint64_t>(v) < static_cast<uint64_t>(N)) {
        const int64_t start = rowptr[v], deg = rowptr[v + 1] - start;
        const int64_t first = ptr[g], ng = ptr[g + 1] - first;
        row.row_probes = deg <= ng;
        row.pidx = row.row_probes ? col + start : n_id + first;
        row.sidx = row.row_probes ? n_id + first : col + start;
        row.np = row.row_probes ? deg : ng;
        row.ns = row.row_probes ? ng : deg;
        row.e0 = start;
        row.c0 = first;
        if constexpr (WRITE) row.out0 = rowptr_out[r];
      }
    }
    const bool deferred = row.np > T;
    Row now = row;
    if (deferred) now.np = 0;
    int64_t longest = now.np;  // the wave's longest short probe side: a uniform step count
#pragma unroll
    for (int off = kGroup; off < psa::kWave; off <<= 1) {
      const int64_t other = __shfl_xor(static_cast<long long>(longest), off);
      longest = other > longest ? other : longest;
    }
    int64_t mine = traverse<kGroup, WRITE>(now, (longest + kGroup - 1) / kGroup, lane, col_out, e_out);
    if constexpr (!WRITE) {
      mine = group_sum<kGroup>(mine);
      if ((lane & (kGroup - 1)) == 0 && r < n && !deferred) counts[r] = mine;
    }
    unsigned long long todo = __ballot(deferred);
    while (todo) {  // the wave's long rows, one at a time, in row order
      const int src = __ffsll(todo) - 1;  // first lane of the group
      todo &= ~(0xffull << src);
      Row big;
      big.pidx = bcast_ptr(row.pidx, src);
      big.sidx = bcast_ptr(row.sidx, src);
      big.np = bcast(row.np, src);
      big.ns = bcast(row.ns, src);
      big.e0 = bcast(row.e0, src);
      big.c0 = bcast(row.c0, src);
      big.out0 = bcast(row.out0, src);
      big.row_probes = __shfl(row.row_probes, src);
      int64_t m = traverse<psa::kWave, WRITE>(big, (big.np + psa::kWave - 1) / psa::kWave, lane, col_out, e_out);
      if constexpr (!WRITE) {
        m = group_sum<psa::kWave>(m);
        if (lane == 0) counts[tile * kRowsPerWave + (src >> 3)] = m;
      }
    }
  }
}

unsigned blocks_for(int64_t n, int per = kThreads) {
  return static_cast<unsigned>(psa::ceil_div(n > 0 ? n : 1, per));
}

unsigned induce_blocks(int64_t n) {
  const int64_t blocks = psa::ceil_div(psa::ceil_div(n, kRowsPerWave), kWavesPerBlock);
  return static_cast<unsigned>(blocks > kMaxBlocks ? kMaxBlocks : blocks);
}

bool key_range(int64_t S, int64_t N) {
  if (S < 0 || N < 0 || S >= (int64_t{1} << 31)) return false;
  return static_cast<unsigned __int128>(S) * static_cast<unsigned __int128>(N) < (static_cast<unsigned __int128>(1) << 62);
}

}  // namespace

extern "C" {

int psa_ego_set_threshold(int threshold) {
  if (threshold < 1) threshold = 1;
  return g_threshold.exchange(threshold);
}

int psa_ego_init(const int64_t* seeds, int64_t S, int64_t N, int64_t* node_out, int32_t* ego_out, int64_t* key_out,
                 int64_t out_count, int64_t* flags, psa_stream_t stream) {
  PSA_REQUIRE(key_range(S, N), "S must lie in [0, 2^31) and S * N below 2^62");
  PSA_REQUIRE(out_count >= S, "node_out, ego_out and key_out must hold S elements");
  PSA_REQUIRE(flags, "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  PSA_ZERO(flags, sizeof(int64_t), s);
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(seeds && node_out && ego_out && key_out, "NULL pointer");
  hipLaunchKernelGGL(ego_init_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, s, seeds, S, N, node_out, ego_out,
                     key_out, flags);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ego_hop_count(const int64_t* rowptr, int64_t N, const int64_t* parent_node, int64_t F, int64_t* counts,
                      int64_t counts_count, psa_stream_t stream) {
  PSA_REQUIRE(N >= 0 && F >= 0 && F <= kMaxSlots, "size out of range");
  PSA_REQUIRE(counts_count >= F, "counts must hold F elements");
  if (F == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && parent_node && counts, "NULL pointer");
  hipLaunchKernelGGL(ego_degree_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, psa::as_stream(stream), rowptr, N,
                     parent_node, F, counts);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ego_hop_pick(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* seeds, int64_t S,
                     const int64_t* parent_node, const int32_t* parent_ego, int64_t F, const int64_t* parent_ptr,
                     int64_t begin, int64_t num_neighbors, int replace, uint64_t seed, int64_t slots,
                     int64_t* node_out, int32_t* ego_out, int64_t* key_out, int64_t out_count, int64_t* flags,
                     psa_stream_t stream) {
  const int64_t k = num_neighbors;
  PSA_REQUIRE(key_range(S, N) && F >= 1 && F <= kMaxSlots && begin >= 0, "size out of range");
  PSA_REQUIRE(slots >= 1 && slots <= kMaxSlots, "slot count out of range");
  PSA_REQUIRE(k != 0 && (k < 0 || slots == F * k), "slots must be F * num_neighbors when num_neighbors >= 0");
  PSA_REQUIRE(out_count >= slots, "node_out, ego_out and key_out must hold `slots` elements");
  PSA_REQUIRE(rowptr && col && seeds && parent_node && parent_ego && node_out && ego_out && key_out && flags &&
                  (k >= 0 || parent_ptr),
              "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  if (k >= 0) {
    hipLaunchKernelGGL(ego_pick_slot_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, rowptr, col, N, seeds,
                       parent_node, parent_ego, begin, k, replace, seed, slots, node_out, ego_out, key_out, flags);
    if (!replace && k <= kFloydRegs)
      hipLaunchKernelGGL(ego_pick_floyd_reg_kernel<kFloydRegs>, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr, col,
                         N, seeds, parent_node, parent_ego, F, begin, k, seed, node_out, key_out, flags);
    else if (!replace)
      hipLaunchKernelGGL(ego_pick_floyd_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, s, rowptr, col, N, seeds,
                         parent_node, parent_ego, F, begin, k, seed, node_out, key_out, flags);
  } else {
    hipLaunchKernelGGL(ego_pick_all_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, rowptr, col, N, seeds,
                       parent_node, parent_ego, F, parent_ptr, slots, node_out, ego_out, key_out, flags);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ego_induce_count(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* seeds, int64_t S,
                         const int64_t* n_id, const int64_t* ego_of, const int64_t* ptr, int64_t n, int64_t* root,
                         int64_t root_count, int64_t* counts, int64_t counts_count, psa_stream_t stream) {
  PSA_REQUIRE(key_range(S, N) && n >= 0 && n < (int64_t{1} << 31), "size out of range");
  PSA_REQUIRE(root_count >= S && counts_count >= n, "root must hold S elements and counts n");
  if (S == 0 && n == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && (seeds || S == 0) && ptr && (root || S == 0), "NULL pointer");
  // col is read for rows with entries only: a matrix without entries may pass NULL
  PSA_REQUIRE(n == 0 || (n_id && ego_of && counts), "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  if (S > 0)
    hipLaunchKernelGGL(ego_root_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, s, n_id, ptr, seeds, S, root);
  if (n > 0)
    hipLaunchKernelGGL(ego_induce_kernel<false>, dim3(induce_blocks(n)), dim3(kThreads), 0, s, rowptr, col, n_id,
                       ego_of, ptr, n, S, N, static_cast<int64_t>(g_threshold.load()), nullptr, counts, nullptr,
                       nullptr);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ego_total(const int64_t* rowptr_out, int64_t n, const int64_t* flags, int64_t* state, psa_stream_t stream) {
  PSA_REQUIRE(n >= 0 && rowptr_out && flags && state, "NULL pointer or negative size");
  hipLaunchKernelGGL(ego_total_kernel, dim3(1), dim3(1), 0, psa::as_stream(stream), rowptr_out, n, flags, state);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ego_induce_write(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t S, const int64_t* n_id,
                         const int64_t* ego_of, const int64_t* ptr, int64_t n, const int64_t* rowptr_out,
                         int64_t nnz_out, int64_t* col_out, int64_t* edge_out, int64_t out_count,
                         psa_stream_t stream) {
  PSA_REQUIRE(key_range(S, N) && n >= 0 && n < (int64_t{1} << 31) && nnz_out >= 0, "size out of range");
  PSA_REQUIRE(out_count >= nnz_out, "col_out and edge_out must hold nnz_out elements");
  if (n == 0 || nnz_out == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && col && n_id && ego_of && ptr && rowptr_out && col_out && edge_out, "NULL pointer");
  hipLaunchKernelGGL(ego_induce_kernel<true>, dim3(induce_blocks(n)), dim3(kThreads), 0, psa::as_stream(stream), rowptr,
                     col, n_id, ego_of, ptr, n, S, N, static_cast<int64_t>(g_threshold.load()), rowptr_out, nullptr,
                     col_out, edge_out);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

}  // extern "C"
