// gfx950 only.
// temporal_neighbor_sample (torch_sparse hetero_temporal_neighbor_sample on one node type, the
// op behind PyG's NeighborLoader(time_attr=...)): per-seed sampling in which ego g only ever
// takes entries whose time is <= seed_time[g], and the SAMPLED entries come back as one
// block-diagonal matrix.
//
// The matrix comes with an EdgeTimeOrder: order[rowptr[v] .. rowptr[v+1]) are the storage
// positions of row v ascending by (time, position) and sorted_time their times.  The eligible
// set of (v, T) is therefore a prefix of the row's segment, c entries long, found by one
// upper-bound search; a pick is a rank in [0, c) and one load of `order`.  The rules that turn
// (c, k, replace, strategy, stream) into ranks are temporal_pick.h, shared with the host export.
//
// Walk list, streams and slot numbering are ego.hip's: entry i < S is seed i of ego i, hop l
// expands every entry of hop l - 1, the parent at walk index i draws on stream i, a hop with
// k >= 0 has F * k slots and a slot past its parent's picks is empty for good.  Every slot
// writes node (or -1), ego, the node key ego * N + node (an empty slot: its ego's seed, a key
// entry `ego` holds already) and the edge key ego * nnz + e (an empty slot: the sentinel
// S * nnz, the largest key, dropped after the unique pass).
//
//   hop_count  (k < 0 only) c of every parent; the caller scans them and reads the slot count
//   hop_pick   k >= 0: one thread per slot; Floyd parents (uniform, no replacement, c > k) one
//              thread per parent in a launch of their own, ranks in registers up to k = 32, in
//              the parent's own node slots above.  k < 0: one thread per slot, the parent found
//              by a search in the scanned counts
//   total      {distinct edge keys, the sort's fault word, flags} in one buffer: one host read
//   finish     root[g]; one thread per distinct edge key (g, e): v by a search in rowptr, row'
//              and col' by two lower-bound searches inside n_id[ptr[g], ptr[g+1])
//
// Grids are sized from the work and not capped: a hop stays below 2^31 - 16 slots, so a launch
// has fewer than 2^23 workgroups and no thread takes a second trip.  No atomics except the
// flag word, no workgroup waits for another, every loop is bounded by k or a log; every index
// read from memory is checked against its array before it is used as one.
#include "common.h"
#include "temporal_pick.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFloydRegs = 32;
constexpr int64_t kMaxSlots = 0x7ffffff0;
constexpr unsigned long long kColOutside = PSA_EGO_COL_OUTSIDE, kBadIndex = PSA_TEMPORAL_BAD_INDEX;

__device__ __forceinline__ void raise_flag(int64_t* flags, unsigned long long bit) {
  atomicOr(reinterpret_cast<unsigned long long*>(flags), bit);
}

struct Graph {
  const int64_t* __restrict__ rowptr;
  const int64_t* __restrict__ col;
  const int64_t* __restrict__ order;
  const int64_t* __restrict__ sorted_time;
  const int64_t* __restrict__ seeds;
  const int64_t* __restrict__ seed_time;
  int64_t N, nnz, S;
};

// start and degree of the row of node v; an empty entry (-1) has none.  A row that leaves
// [0, nnz) is treated as empty and flagged.
__device__ __forceinline__ void row_of(const Graph& G, int64_t v, int64_t* start, int64_t* deg, int64_t* flags) {
  *start = 0;
  *deg = 0;
  if (static_cast<uint64_t>(v) >= static_cast<uint64_t>(G.N)) return;
  const int64_t a = G.rowptr[v], b = G.rowptr[v + 1];
  if (a < 0 || b < a || b > G.nnz) {
    raise_flag(flags, kBadIndex);
    return;
  }
  *start = a;
  *deg = b - a;
}

// eligible entries of parent (v, g)
__device__ __forceinline__ int64_t eligible(const Graph& G, int64_t start, int64_t deg, int32_t g) {
  return deg > 0 ? psa::temporal_count(G.sorted_time, start, deg, G.seed_time[g]) : 0;
}

__device__ __forceinline__ int64_t seed_of(const Graph& G, int64_t g) {
  const int64_t s = G.seeds[g];
  return static_cast<uint64_t>(s) < static_cast<uint64_t>(G.N) ? s : 0;
}

// Slot p of ego g took the entry at position `at` of `order` (none: at < 0).
__device__ __forceinline__ void emit(const Graph& G, int64_t at, int64_t g, int64_t p, int64_t* __restrict__ node_out,
                                     int64_t* __restrict__ key_out, int64_t* __restrict__ ekey_out,
                                     int64_t* __restrict__ flags) {
  int64_t e = -1, c = -1;
  if (at >= 0) {
    e = G.order[at];
    if (static_cast<uint64_t>(e) >= static_cast<uint64_t>(G.nnz)) {
      raise_flag(flags, kBadIndex);
      e = -1;
    }
  }
  if (e >= 0) {
    c = G.col[e];
    if (static_cast<uint64_t>(c) >= static_cast<uint64_t>(G.N)) {
      raise_flag(flags, kColOutside);
      c = -1;
      e = -1;
    }
  }
  node_out[p] = c;
  key_out[p] = g * G.N + (c >= 0 ? c : seed_of(G, g));
  ekey_out[p] = e >= 0 ? g * G.nnz + e : G.S * G.nnz;
}

__global__ void __launch_bounds__(kThreads)
temporal_count_kernel(Graph G, const int64_t* __restrict__ pnode, const int32_t* __restrict__ pego, int64_t F,
                      int64_t* __restrict__ counts, int64_t* __restrict__ flags) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  int64_t start, deg;
  row_of(G, pnode[f], &start, &deg, flags);
  counts[f] = eligible(G, start, deg, pego[f]);
}

// k >= 0, one thread per slot p = f * k + t: the ego of every slot, and node and keys of every
// parent that is not a Floyd parent.
__global__ void __launch_bounds__(kThreads)
temporal_pick_slot_kernel(Graph G, const int64_t* __restrict__ pnode, const int32_t* __restrict__ pego, int64_t begin,
                          int64_t k, int replace, int strategy, uint64_t seed, int64_t cap,
                          int64_t* __restrict__ node_out, int32_t* __restrict__ ego_out, int64_t* __restrict__ key_out,
                          int64_t* __restrict__ ekey_out, int64_t* __restrict__ flags) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  const int64_t f = p / k, t = p - f * k;
  const int32_t g = pego[f];
  ego_out[p] = g;
  int64_t start, deg;
  row_of(G, pnode[f], &start, &deg, flags);
  const int64_t c = eligible(G, start, deg, g);
  if (psa::temporal_is_floyd(c, k, replace, strategy)) return;
  int64_t at = -1;
  if (t < psa::temporal_picks_of(c, k, replace, strategy))
    at = start + psa::temporal_slot_rank(c, replace, strategy, psa::temporal_stream(seed, begin + f), t);
  emit(G, at, g, p, node_out, key_out, ekey_out, flags);
}

// Floyd parents, one thread each, the ranks in registers.
template <int KMAX>
__global__ void __launch_bounds__(kThreads)
temporal_pick_floyd_reg_kernel(Graph G, const int64_t* __restrict__ pnode, const int32_t* __restrict__ pego, int64_t F,
                               int64_t begin, int64_t k, uint64_t seed, int64_t* __restrict__ node_out,
                               int64_t* __restrict__ key_out, int64_t* __restrict__ ekey_out,
                               int64_t* __restrict__ flags) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  const int32_t g = pego[f];
  int64_t start, deg;
  row_of(G, pnode[f], &start, &deg, flags);
  const int64_t c = eligible(G, start, deg, g);
  if (c <= k) return;
  int64_t mine[KMAX];
  psa::temporal_floyd_small<KMAX>(c, k, psa::temporal_stream(seed, begin + f), mine);
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < k) emit(G, start + mine[t], g, f * k + t, node_out, key_out, ekey_out, flags);
}

// The same for k > kFloydRegs: the parent's own node slots hold the ranks during the walk.
__global__ void __launch_bounds__(kThreads)
temporal_pick_floyd_kernel(Graph G, const int64_t* __restrict__ pnode, const int32_t* __restrict__ pego, int64_t F,
                           int64_t begin, int64_t k, uint64_t seed, int64_t* __restrict__ node_out,
                           int64_t* __restrict__ key_out, int64_t* __restrict__ ekey_out, int64_t* __restrict__ flags) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  const int32_t g = pego[f];
  int64_t start, deg;
  row_of(G, pnode[f], &start, &deg, flags);
  const int64_t c = eligible(G, start, deg, g);
  if (c <= k) return;
  int64_t* mine = node_out + f * k;
  psa::temporal_floyd_large(c, k, psa::temporal_stream(seed, begin + f), mine);
  // ranks become nodes after the walk, whose comparisons must see ranks only
  for (int64_t t = 0; t < k; ++t) emit(G, start + mine[t], g, f * k + t, node_out, key_out, ekey_out, flags);
}

// k < 0: slot p is rank p - pptr[r] of parent r, r = the largest index with pptr[r] <= p.
__global__ void __launch_bounds__(kThreads)
temporal_pick_all_kernel(Graph G, const int64_t* __restrict__ pnode, const int32_t* __restrict__ pego, int64_t F,
                         const int64_t* __restrict__ pptr, int64_t cap, int64_t* __restrict__ node_out,
                         int32_t* __restrict__ ego_out, int64_t* __restrict__ key_out, int64_t* __restrict__ ekey_out,
                         int64_t* __restrict__ flags) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= cap) return;
  int64_t lo = 0, hi = F;  // pptr[0] = 0 <= p < cap = pptr[F]
  for (int i = 0; i < 64 && hi - lo > 1; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  const int32_t g = pego[lo];
  ego_out[p] = g;
  int64_t start, deg;
  row_of(G, pnode[lo], &start, &deg, flags);
  const int64_t t = p - pptr[lo];
  // the scanned counts were taken from this very row: t < c <= deg unless they were not
  emit(G, t >= 0 && t < deg ? start + t : -1, g, p, node_out, key_out, ekey_out, flags);
}

__global__ void temporal_total_kernel(const int64_t* __restrict__ count_words, const int64_t* __restrict__ flags,
                                      int64_t* __restrict__ state) {
  state[0] = count_words[0];
  state[1] = count_words[1];
  state[2] = *flags;
}

// position of x in the ascending list[lo0, hi0), or -1
__device__ __forceinline__ int64_t find(const int64_t* __restrict__ list, int64_t lo0, int64_t hi0, int64_t x) {
  int64_t lo = lo0, hi = hi0;
  for (int i = 0; i < 64 && lo < hi; ++i) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < hi0 && list[lo] == x ? lo : -1;
}

__global__ void __launch_bounds__(kThreads)
temporal_root_kernel(const int64_t* __restrict__ n_id, const int64_t* __restrict__ ptr, int64_t n,
                     const int64_t* __restrict__ seeds, int64_t S, int64_t* __restrict__ root) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (g >= S) return;
  const int64_t first = ptr[g], end = ptr[g + 1];
  root[g] = first >= 0 && first <= end && end <= n ? find(n_id, first, end, seeds[g]) : -1;
}

// One thread per distinct edge key (g, e), q < m: the sentinel sorts behind them.
__global__ void __launch_bounds__(kThreads)
temporal_finish_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N, int64_t nnz,
                       int64_t S, const int64_t* __restrict__ key_ego, const int64_t* __restrict__ key_edge, int64_t m,
                       const int64_t* __restrict__ n_id, const int64_t* __restrict__ ptr, int64_t n,
                       int64_t* __restrict__ row_out, int64_t* __restrict__ col_out, int64_t* __restrict__ edge_out,
                       int64_t* __restrict__ flags) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= m) return;
  const int64_t g = key_ego[q], e = key_edge[q];
  int64_t r = -1, c = -1;
  if (static_cast<uint64_t>(g) < static_cast<uint64_t>(S) && static_cast<uint64_t>(e) < static_cast<uint64_t>(nnz)) {
    int64_t lo = 0, hi = N;  // the row of e: the largest v with rowptr[v] <= e (rowptr[0] = 0)
    for (int i = 0; i < 64 && hi - lo > 1; ++i) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (rowptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    const int64_t first = ptr[g], end = ptr[g + 1];
    if (first >= 0 && first <= end && end <= n) {
      r = find(n_id, first, end, lo);
      c = find(n_id, first, end, col[e]);  // a column outside [0, N) is no node of the set
    }
  }
  if (r < 0 || c < 0) {  // the pick kernels emitted both nodes: never, unless the inputs changed under the op
    raise_flag(flags, kBadIndex);
    r = c = 0;
  }
  row_out[q] = r;
  col_out[q] = c;
  edge_out[q] = e;
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>(psa::ceil_div(n > 0 ? n : 1, kThreads)); }

bool key_range(int64_t S, int64_t N, int64_t nnz) {
  if (S < 0 || N < 0 || nnz < 0 || S >= (int64_t{1} << 31)) return false;
  const unsigned __int128 lim = static_cast<unsigned __int128>(1) << 62, s = static_cast<unsigned __int128>(S);
  return s * static_cast<unsigned __int128>(N) < lim && s * static_cast<unsigned __int128>(nnz) < lim;
}

}  // namespace

extern "C" {

int psa_temporal_hop_count(const int64_t* rowptr, const int64_t* sorted_time, int64_t N, int64_t nnz,
                           const int64_t* seed_time, int64_t S, const int64_t* parent_node, const int32_t* parent_ego,
                           int64_t F, int64_t* counts, int64_t counts_count, int64_t* flags, psa_stream_t stream) {
  PSA_REQUIRE(key_range(S, N, nnz) && F >= 0 && F <= kMaxSlots, "size out of range");
  PSA_REQUIRE(counts_count >= F, "counts must hold F elements");
  if (F == 0) return PSA_OK;
  PSA_REQUIRE(rowptr && seed_time && parent_node && parent_ego && counts && flags && (sorted_time || nnz == 0),
              "NULL pointer");
  const Graph G{rowptr, nullptr, nullptr, sorted_time, nullptr, seed_time, N, nnz, S};
  hipLaunchKernelGGL(temporal_count_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, psa::as_stream(stream), G,
                     parent_node, parent_ego, F, counts, flags);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_temporal_hop_pick(const int64_t* rowptr, const int64_t* col, const int64_t* order, const int64_t* sorted_time,
                          int64_t N, int64_t nnz, const int64_t* seeds, const int64_t* seed_time, int64_t S,
                          const int64_t* parent_node, const int32_t* parent_ego, int64_t F, const int64_t* parent_ptr,
                          int64_t begin, int64_t num_neighbors, int replace, int strategy, uint64_t seed, int64_t slots,
                          int64_t* node_out, int32_t* ego_out, int64_t* key_out, int64_t* edge_key_out,
                          int64_t out_count, int64_t* flags, psa_stream_t stream) {
  const int64_t k = num_neighbors;
  PSA_REQUIRE(key_range(S, N, nnz) && nnz >= 1 && F >= 1 && F <= kMaxSlots && begin >= 0, "size out of range");
  PSA_REQUIRE(slots >= 1 && slots <= kMaxSlots, "slot count out of range");
  PSA_REQUIRE(k != 0 && (k < 0 || slots == F * k), "slots must be F * num_neighbors when num_neighbors >= 0");
  PSA_REQUIRE(strategy == psa::kTemporalUniform || (strategy == psa::kTemporalLast && !replace),
              "strategy must be 0 (uniform) or 1 (last, without replacement)");
  PSA_REQUIRE(out_count >= slots, "node_out, ego_out, key_out and edge_key_out must hold `slots` elements");
  PSA_REQUIRE(rowptr && col && order && sorted_time && seeds && seed_time && parent_node && parent_ego && node_out &&
                  ego_out && key_out && edge_key_out && flags && (k >= 0 || parent_ptr),
              "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  const Graph G{rowptr, col, order, sorted_time, seeds, seed_time, N, nnz, S};
  if (k >= 0) {
    hipLaunchKernelGGL(temporal_pick_slot_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, G, parent_node,
                       parent_ego, begin, k, replace, strategy, seed, slots, node_out, ego_out, key_out, edge_key_out,
                       flags);
    const bool floyd = strategy == psa::kTemporalUniform && !replace;
    if (floyd && k <= kFloydRegs)
      hipLaunchKernelGGL(temporal_pick_floyd_reg_kernel<kFloydRegs>, dim3(blocks_for(F)), dim3(kThreads), 0, s, G,
                         parent_node, parent_ego, F, begin, k, seed, node_out, key_out, edge_key_out, flags);
    else if (floyd)
      hipLaunchKernelGGL(temporal_pick_floyd_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, s, G, parent_node,
                         parent_ego, F, begin, k, seed, node_out, key_out, edge_key_out, flags);
  } else {
    hipLaunchKernelGGL(temporal_pick_all_kernel, dim3(blocks_for(slots)), dim3(kThreads), 0, s, G, parent_node,
                       parent_ego, F, parent_ptr, slots, node_out, ego_out, key_out, edge_key_out, flags);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_temporal_total(const int64_t* count_words, const int64_t* flags, int64_t* state, psa_stream_t stream) {
  PSA_REQUIRE(count_words && flags && state, "NULL pointer");
  hipLaunchKernelGGL(temporal_total_kernel, dim3(1), dim3(1), 0, psa::as_stream(stream), count_words, flags, state);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_temporal_finish(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, const int64_t* seeds,
                        int64_t S, const int64_t* key_ego, const int64_t* key_edge, int64_t m, const int64_t* n_id,
                        const int64_t* ptr, int64_t n, int64_t* root, int64_t root_count, int64_t* row_out,
                        int64_t* col_out, int64_t* edge_out, int64_t out_count, int64_t* flags, psa_stream_t stream) {
  PSA_REQUIRE(key_range(S, N, nnz) && n >= 0 && n < (int64_t{1} << 31) && m >= 0, "size out of range");
  PSA_REQUIRE(root_count >= S && out_count >= m, "root must hold S elements, the entry outputs m");
  if (S == 0) return PSA_OK;
  PSA_REQUIRE(seeds && ptr && root && flags && (n_id || n == 0), "NULL pointer");
  hipStream_t s = psa::as_stream(stream);
  hipLaunchKernelGGL(temporal_root_kernel, dim3(blocks_for(S)), dim3(kThreads), 0, s, n_id, ptr, n, seeds, S, root);
  if (m > 0) {
    PSA_REQUIRE(rowptr && col && key_ego && key_edge && n_id && row_out && col_out && edge_out && N >= 1,
                "NULL pointer");
    hipLaunchKernelGGL(temporal_finish_kernel, dim3(blocks_for(m)), dim3(kThreads), 0, s, rowptr, col, N, nnz, S,
                       key_ego, key_edge, m, n_id, ptr, n, row_out, col_out, edge_out, flags);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int64_t psa_temporal_pick_host(const int64_t* sorted_time, int64_t start, int64_t deg, int64_t bound, int64_t k,
                               int replace, int strategy, uint64_t seed, int64_t stream_index, int64_t* ranks,
                               int64_t ranks_count) {
  if (start < 0 || deg < 0 || (deg > 0 && !sorted_time) || ranks_count < 0 || (ranks_count > 0 && !ranks)) return -1;
  if (strategy != psa::kTemporalUniform && !(strategy == psa::kTemporalLast && !replace)) return -1;
  const int64_t c = deg > 0 ? psa::temporal_count(sorted_time, start, deg, bound) : 0;
  const int64_t count = k < 0 ? c : psa::temporal_picks_of(c, k, replace, strategy);
  if (count > ranks_count) return -1;
  if (k < 0) {
    for (int64_t t = 0; t < c; ++t) ranks[t] = t;
    return count;
  }
  const uint64_t stream = psa::temporal_stream(seed, stream_index);
  if (!psa::temporal_is_floyd(c, k, replace, strategy)) {
    for (int64_t t = 0; t < count; ++t) ranks[t] = psa::temporal_slot_rank(c, replace, strategy, stream, t);
  } else if (k <= kFloydRegs) {  // the two walks the kernels run, chosen as they choose
    int64_t mine[kFloydRegs];
    psa::temporal_floyd_small<kFloydRegs>(c, k, stream, mine);
    for (int64_t t = 0; t < k; ++t) ranks[t] = mine[t];
  } else {
    psa::temporal_floyd_large(c, k, stream, ranks);
  }
  return count;
}

}  // extern "C"
