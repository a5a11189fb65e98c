// Approximate personalised PageRank by forward push, for gfx950 (ppr_step.h states the round,
// the fixed point, the work bound and the table; the host export below runs the same steps).
//
// ONE WORKGROUP RUNS ONE SOURCE from its first round to its last: no workgroup waits on
// another, and every loop has its bound before it starts (max_rounds rounds, cap slots, cap
// probes, the entries of a chunk, 64 halvings).  256 lanes.
//
// The table of cap slots (key, r, p, s: 32 bytes a slot) is the source's slab in global
// memory, or, in the second build of the same template, lives in LDS for the whole run and is
// copied to the slab once at the end.  LDS budget: the 160 KB of a gfx950 CU, of which the
// chunk below takes 27 KB; that leaves room for cap <= 4096 (128 KB), kPprLdsCap.  Both are
// dynamic LDS (above 64 KB the function attribute is needed).  In global memory every access
// to the table is an agent-scope atomic load, store, compare-and-swap or add, so no lane reads
// a line that the L1 kept from before another lane's atomic; in LDS the same calls are ds
// instructions.  The workgroup clears its key, r and s arrays before it starts; p of a slot
// is zeroed by the lane that claims it.
//
// A round.
//   1  SPLIT: the lanes stride over the slots.  An active slot is split where it lies:
//      p += keep, r = rem, s = share.  The snapshot of the whole round is thereby taken before
//      any entry of the round is added; s != 0 now says "push pending".  The number of active
//      slots decides whether the run goes on, the number of pending ones how chunks are filled.
//   2  CHUNKS: pending slots are compacted into an LDS chunk (row begin, share, degree) and
//      their s cleared.  A round whose pending slots fit one chunk fills it in one sweep of
//      the table; a larger one sweeps CHUNK / 2 slots at a time and runs the chunk as soon as
//      it is more than half full.  The chunk's degrees get an exclusive scan in LDS.
//   3  ENTRIES: lanes take entries, not nodes.  Lane t handles entries t, t + 256, ... of the
//      chunk, finds the owning node by binary search in the scanned degrees and adds its share
//      to the column's slot (ppr_add: 64-bit CAS on the key, linear probing, a 64-bit integer
//      add that returns nothing).  A row of 100 000 entries is spread over the whole workgroup;
//      a thousand rows of 3 entries keep every lane busy.
// Workgroup barriers separate 1 from 2, a chunk's fill from its entries, and the rounds.
//
// Integer adds commute, so r and p of every node are the same bits under any schedule; which
// slot a node got is not, and nothing exposes it: psa_ppr_write compacts a slab's entries with
// a positive value into (slot-in-batch * N + node, value / 2^48 as a double), which the caller
// sorts by key.
#include <initializer_list>
#include <vector>

#include "common.h"
#include "ppr_step.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsChunk = 1024;        // chunk capacity of the LDS build
constexpr int kGlobalChunk = 2048;     // and of the global build (48 KB: three workgroups a CU)
constexpr int64_t kPprLdsCap = 4096;   // largest table the LDS build holds
constexpr int kInfoFields = 8;

// Agent-scope (global build) or workgroup-scope (LDS build) atomics: the device's memory policy.
template <int SCOPE>
struct PprDevMem {
  static __device__ inline int64_t load(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ inline uint64_t load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ inline void store(int64_t* p, int64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
  static __device__ inline void store(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
  static __device__ inline int64_t cas(int64_t* p, int64_t expect, int64_t v) {
    __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return expect;  // the value found
  }
  static __device__ inline void add(uint64_t* p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE); }
};

template <int CHUNK>
struct PprChunk {
  int64_t begin[CHUNK];     // first storage position of the node's row
  uint64_t share[CHUNK];    // what every entry of it receives
  int64_t scan[CHUNK + 1];  // degrees, then their exclusive scan; scan[n] = entries of the chunk
  int64_t part[kThreads];   // the scan's per-lane sums
  int n;                    // nodes in the chunk
  int pending;              // slots with a push pending this round
  int active;               // slots split this round (pending + dangling)
  unsigned long long flags, pushes, edges, count_p, count_r, touched;
};

// Exclusive scan of ch.scan[0 .. n) in place, ch.scan[n] = total.  All lanes call it.
template <int CHUNK>
__device__ void chunk_scan(PprChunk<CHUNK>& ch, int n) {
  constexpr int PER = CHUNK / kThreads;
  const int t = threadIdx.x;
  int64_t v[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = t * PER + k;
    v[k] = i < n ? ch.scan[i] : 0;
    sum += v[k];
  }
  ch.part[t] = sum;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const int64_t below = t >= off ? ch.part[t - off] : 0;
    __syncthreads();
    ch.part[t] += below;
    __syncthreads();
  }
  int64_t run = ch.part[t] - sum;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = t * PER + k;
    if (i < n) ch.scan[i] = run;
    run += v[k];
  }
  if (t == kThreads - 1) ch.scan[n] = ch.part[t];
  __syncthreads();
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads)
ppr_push_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N, int64_t nnz,
                const int64_t* __restrict__ source, int64_t nsrc, int64_t cap, uint64_t alpha_q, uint64_t eps_q,
                int64_t max_rounds, int64_t* table_key, uint64_t* table_r, uint64_t* table_p, uint64_t* table_s,
                int64_t* __restrict__ info) {
  constexpr int CHUNK = LDS ? kLdsChunk : kGlobalChunk;
  using M = PprDevMem<LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT>;
  using Chunk = PprChunk<CHUNK>;
  extern __shared__ __align__(16) unsigned char smem[];
  Chunk& ch = *reinterpret_cast<Chunk*>(smem);

  const int tid = threadIdx.x;
  const int64_t me = blockIdx.x;
  int64_t* const slab_key = table_key + me * cap;
  uint64_t* const slab_r = table_r + me * cap;
  uint64_t* const slab_p = table_p + me * cap;
  uint64_t* const slab_s = table_s + me * cap;
  int64_t* key = slab_key;
  uint64_t *r = slab_r, *p = slab_p, *s = slab_s;
  if (LDS) {
    key = reinterpret_cast<int64_t*>(smem + sizeof(Chunk));
    r = reinterpret_cast<uint64_t*>(key + cap);
    p = r + cap;
    s = p + cap;
  }

  for (int64_t j = tid; j < cap; j += kThreads) {
    M::store(key + j, psa::kPprEmpty);
    M::store(r + j, 0);
    M::store(s + j, 0);
  }
  if (tid == 0) {
    ch.flags = LDS ? psa::kPprInLds : 0;
    ch.pushes = ch.edges = ch.count_p = ch.count_r = ch.touched = 0;
  }
  __syncthreads();
  if (tid == 0) {
    const int64_t src = source[me];
    if (src >= 0 && src < N) {
      const int64_t slot = psa::ppr_hash(src, cap);
      M::store(key + slot, src);
      M::store(r + slot, psa::kPprOne);
      M::store(p + slot, 0);
      M::store(s + slot, 0);
    } else {
      ch.flags |= psa::kPprBadIndex;
    }
  }

  int64_t flags = 0, rounds = 0;
  unsigned long long pushes = 0, edges = 0;
  for (int64_t round = 0; round < max_rounds; ++round) {
    if (tid == 0) ch.pending = ch.active = 0;
    __syncthreads();

    // 1  split every active slot where it lies
    int my_active = 0, my_pending = 0;
    for (int64_t j = tid; j < cap; j += kThreads) {
      const int64_t u = M::load(key + j);
      if (u == psa::kPprEmpty) continue;
      const uint64_t x = M::load(r + j);
      if (x == 0) continue;
      int64_t begin;
      const int64_t deg = psa::ppr_row(rowptr, nnz, u, &begin, &flags);
      if (!psa::ppr_active(x, deg, eps_q)) continue;
      const psa::PprSplit sp = psa::ppr_split(x, deg, alpha_q);
      M::store(p + j, M::load(p + j) + sp.keep);
      M::store(r + j, sp.rem);
      M::store(s + j, sp.share);
      ++my_active;
      my_pending += sp.share != 0;
      edges += static_cast<unsigned long long>(deg);
    }
    pushes += my_active;
    if (my_active) atomicAdd(&ch.active, my_active);
    if (my_pending) atomicAdd(&ch.pending, my_pending);
    __syncthreads();
    const int active = ch.active, pending = ch.pending;
    if (active == 0) break;  // the same value in every lane
    ++rounds;

    // 2, 3  chunks of pending slots, their entries
    const bool one_sweep = pending <= CHUNK;
    const int64_t span = one_sweep ? cap : CHUNK / 2;
    int64_t base = 0;
    while (pending > 0 && base < cap) {
      __syncthreads();
      if (tid == 0) ch.n = 0;
      __syncthreads();
      int n = 0;
      do {
        const int64_t end = cap - base < span ? cap : base + span;
        for (int64_t j = base + tid; j < end; j += kThreads) {
          const uint64_t share = M::load(s + j);
          if (share == 0) continue;
          const int idx = atomicAdd(&ch.n, 1);
          if (idx >= CHUNK) {  // cannot happen: pending counted them
            flags |= psa::kPprBadIndex;
            continue;
          }
          int64_t begin;
          ch.scan[idx] = psa::ppr_row(rowptr, nnz, M::load(key + j), &begin, &flags);
          ch.begin[idx] = begin;
          ch.share[idx] = share;
          M::store(s + j, 0);
        }
        base = end;
        __syncthreads();
        n = ch.n < CHUNK ? ch.n : CHUNK;
        __syncthreads();
      } while (!one_sweep && base < cap && n + span <= CHUNK);
      if (n == 0) continue;
      chunk_scan(ch, n);
      const int64_t total = ch.scan[n];
      for (int64_t e = tid; e < total; e += kThreads) {
        const int i = psa::ppr_owner(ch.scan, n, e);
        const int64_t v = col[ch.begin[i] + (e - ch.scan[i])];
        flags |= psa::ppr_add<M>(key, r, p, s, cap, N, v, ch.share[i]);
      }
    }
    __syncthreads();
  }
  __syncthreads();

  // the counts, and the LDS table's one trip to its slab
  unsigned long long count_p = 0, count_r = 0, touched = 0;
  for (int64_t j = tid; j < cap; j += kThreads) {
    const int64_t u = M::load(key + j);
    const uint64_t rv = M::load(r + j);
    const uint64_t pv = u != psa::kPprEmpty ? M::load(p + j) : 0;
    if (LDS) {
      slab_key[j] = u;
      slab_r[j] = rv;
      slab_p[j] = pv;
      slab_s[j] = 0;
    }
    touched += u != psa::kPprEmpty;
    count_p += pv != 0;
    count_r += rv != 0;
  }
  if (flags) atomicOr(&ch.flags, static_cast<unsigned long long>(flags));
  if (pushes) atomicAdd(&ch.pushes, pushes);
  if (edges) atomicAdd(&ch.edges, edges);
  if (count_p) atomicAdd(&ch.count_p, count_p);
  if (count_r) atomicAdd(&ch.count_r, count_r);
  if (touched) atomicAdd(&ch.touched, touched);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long f[kInfoFields] = {ch.count_p, ch.count_r, static_cast<unsigned long long>(rounds),
                                               ch.flags,   ch.pushes,  ch.edges,
                                               ch.touched, 0};
    for (int k = 0; k < kInfoFields; ++k) info[k * nsrc + me] = static_cast<int64_t>(f[k]);
  }
}

// One workgroup per slab: the entries with a key and a positive value, in any order inside
// [ptr[i], ptr[i + 1]).  A slab whose range does not lie in [0, n_out] writes nothing, and no
// entry is written past its slab's range.
__global__ void __launch_bounds__(kThreads)
ppr_write_kernel(const int64_t* __restrict__ table_key, const uint64_t* __restrict__ table_val, int64_t cap, int64_t N,
                 const int64_t* __restrict__ ptr, int64_t n_out, int64_t* __restrict__ key_out,
                 double* __restrict__ val_out) {
  __shared__ unsigned long long cursor;
  const int64_t me = blockIdx.x;
  const int64_t b = ptr[me], e = ptr[me + 1];
  if (!(0 <= b && b <= e && e <= n_out)) return;
  if (threadIdx.x == 0) cursor = 0;
  __syncthreads();
  for (int64_t j = threadIdx.x; j < cap; j += kThreads) {
    const int64_t u = table_key[me * cap + j];
    const uint64_t v = table_val[me * cap + j];
    if (u < 0 || u >= N || v == 0) continue;
    const int64_t pos = b + static_cast<int64_t>(atomicAdd(&cursor, 1ull));
    if (pos >= e) continue;
    key_out[pos] = me * N + u;
    val_out[pos] = static_cast<double>(v) * 0x1p-48;
  }
}

bool power_of_two(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

// The argument checks the entry points share: 1 = run, 0 = nothing to do, < 0 = refused.
int check_args(const char* fn, std::initializer_list<int64_t> sizes, int64_t cap, int64_t count,
               std::initializer_list<const void*> ptrs) {
  const char* msg = nullptr;
  for (int64_t x : sizes)
    if (x < 0) msg = "negative size";
  if (!msg && !power_of_two(cap)) msg = "cap must be a power of two";
  if (!msg && count == 0) return 0;
  if (!msg)
    for (const void* p : ptrs)
      if (!p) msg = "NULL pointer";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

bool quanta_ok(uint64_t alpha_q, uint64_t eps_q) {
  return alpha_q >= (1ull << 16) && alpha_q <= (1ull << 32) - (1ull << 16) && eps_q >= (1ull << 16) &&
         eps_q <= psa::kPprOne;
}

}  // namespace

extern "C" {

int64_t psa_ppr_lds_cap(void) { return kPprLdsCap; }

int psa_ppr_push(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, const int64_t* source, int64_t nsrc,
                 int64_t cap, uint64_t alpha_q, uint64_t eps_q, int64_t max_rounds, int64_t* table_key,
                 uint64_t* table_r, uint64_t* table_p, uint64_t* table_s, int64_t* info, psa_stream_t stream) {
  const int go = check_args(__func__, {N, nnz, nsrc, max_rounds}, cap, nsrc,
                            {rowptr, source, table_key, table_r, table_p, table_s, info, nnz > 0 ? col : rowptr});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  PSA_REQUIRE(quanta_ok(alpha_q, eps_q), "alpha_q must lie in [2^16, 2^32 - 2^16] and eps_q in [2^16, 2^48]");
  PSA_REQUIRE(nsrc <= 0x7fffffff, "too many sources for one launch");
  const dim3 grid(static_cast<unsigned>(nsrc)), block(kThreads);
  if (cap <= kPprLdsCap) {
    const size_t lds = sizeof(PprChunk<kLdsChunk>) + static_cast<size_t>(cap) * 32;
    PSA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ppr_push_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL(ppr_push_kernel<true>, grid, block, lds, psa::as_stream(stream), rowptr, col, N, nnz, source,
                       nsrc, cap, alpha_q, eps_q, max_rounds, table_key, table_r, table_p, table_s, info);
  } else {
    hipLaunchKernelGGL(ppr_push_kernel<false>, grid, block, sizeof(PprChunk<kGlobalChunk>), psa::as_stream(stream),
                       rowptr, col, N, nnz, source, nsrc, cap, alpha_q, eps_q, max_rounds, table_key, table_r, table_p,
                       table_s, info);
  }
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ppr_write(const int64_t* table_key, const uint64_t* table_val, int64_t nslab, int64_t cap, int64_t N,
                  const int64_t* ptr, int64_t n_out, int64_t* key_out, double* val_out, psa_stream_t stream) {
  const int go = check_args(__func__, {nslab, N, n_out}, cap, nslab < n_out ? nslab : n_out,
                            {table_key, table_val, ptr, key_out, val_out});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  PSA_REQUIRE(nslab <= 0x7fffffff, "too many slabs for one launch");
  hipLaunchKernelGGL(ppr_write_kernel, dim3(static_cast<unsigned>(nslab)), dim3(kThreads), 0, psa::as_stream(stream),
                     table_key, table_val, cap, N, ptr, n_out, key_out, val_out);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_ppr_host(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, const int64_t* source, int64_t nsrc,
                 int64_t cap, uint64_t alpha_q, uint64_t eps_q, int64_t max_rounds, int64_t* table_key,
                 uint64_t* table_r, uint64_t* table_p, uint64_t* table_s, int64_t* info) {
  using M = psa::PprHostMem;
  const int go = check_args(__func__, {N, nnz, nsrc, max_rounds}, cap, nsrc,
                            {rowptr, source, table_key, table_r, table_p, table_s, info, nnz > 0 ? col : rowptr});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  PSA_REQUIRE(quanta_ok(alpha_q, eps_q), "alpha_q must lie in [2^16, 2^32 - 2^16] and eps_q in [2^16, 2^48]");
  std::vector<int64_t> begin(kLdsChunk), scan(kLdsChunk + 1);
  std::vector<uint64_t> share(kLdsChunk);
  for (int64_t me = 0; me < nsrc; ++me) {
    int64_t* key = table_key + me * cap;
    uint64_t *r = table_r + me * cap, *p = table_p + me * cap, *s = table_s + me * cap;
    int64_t flags = 0, rounds = 0, pushes = 0, edges = 0;
    for (int64_t j = 0; j < cap; ++j) key[j] = psa::kPprEmpty, r[j] = 0, s[j] = 0;
    const int64_t src = source[me];
    if (src >= 0 && src < N) {
      const int64_t slot = psa::ppr_hash(src, cap);
      key[slot] = src, r[slot] = psa::kPprOne, p[slot] = 0, s[slot] = 0;
    } else {
      flags |= psa::kPprBadIndex;
    }
    for (int64_t round = 0; round < max_rounds; ++round) {
      int64_t active = 0;
      for (int64_t j = 0; j < cap; ++j) {
        if (key[j] == psa::kPprEmpty || r[j] == 0) continue;
        int64_t b;
        const int64_t deg = psa::ppr_row(rowptr, nnz, key[j], &b, &flags);
        if (!psa::ppr_active(r[j], deg, eps_q)) continue;
        const psa::PprSplit sp = psa::ppr_split(r[j], deg, alpha_q);
        p[j] += sp.keep, r[j] = sp.rem, s[j] = sp.share;
        ++active, edges += deg;
      }
      if (active == 0) break;
      ++rounds, pushes += active;
      for (int64_t base = 0; base < cap;) {  // the kernel's chunks: compact, scan, entries
        int n = 0;
        for (; base < cap && n < kLdsChunk; ++base) {
          if (s[base] == 0) continue;
          scan[n] = psa::ppr_row(rowptr, nnz, key[base], &begin[n], &flags);
          share[n++] = s[base];
          s[base] = 0;
        }
        int64_t total = 0;
        for (int i = 0; i < n; ++i) {
          const int64_t deg = scan[i];
          scan[i] = total, total += deg;
        }
        scan[n] = total;
        for (int64_t e = 0; e < total; ++e) {
          const int i = psa::ppr_owner(scan.data(), n, e);
          flags |= psa::ppr_add<M>(key, r, p, s, cap, N, col[begin[i] + (e - scan[i])], share[i]);
        }
      }
    }
    int64_t count_p = 0, count_r = 0, touched = 0;
    for (int64_t j = 0; j < cap; ++j) {
      if (key[j] == psa::kPprEmpty) p[j] = 0;
      s[j] = 0;
      touched += key[j] != psa::kPprEmpty, count_p += p[j] != 0, count_r += r[j] != 0;
    }
    const int64_t f[kInfoFields] = {count_p, count_r, rounds, flags, pushes, edges, touched, 0};
    for (int k = 0; k < kInfoFields; ++k) info[k * nsrc + me] = f[k];
  }
  return PSA_OK;
}

}  // extern "C"
