// node2vec (p, q) random walks on a sorted CSR matrix for gfx950: the second-order walk of
// Grover & Leskovec, uniform or edge-weighted (pi ~ alpha_pq * w), with edge ids.
//
// The launch shape is weighted.hip's walk: one lane per walk, the node in a register, bursts
// of stores.  The step is node2vec_step.h: propose an entry as the plain walk would, accept
// it by an integer compare against the threshold of its class, at most max_tries times.
// What the step needs of the previous node t (t itself and the bounds of its row, for the
// search "does row t store x") is what the lane loaded one step earlier, so it stays in
// registers and row t's lines are the ones the walk has just read.
//
// Every loop is bounded before it starts: walk_length steps, max_tries tries, 64 halvings.
// No atomics on the output, no workspace, no waiting on another workgroup.
//
// psa_node2vec_walk_host runs the same step serially on host arrays.
#include "common.h"
#include "node2vec_step.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBuf = 16;      // steps per burst of stores, as weighted.hip
constexpr int kBufEdges = 8;  // with edge ids two rows are buffered: half the steps each

template <bool WEIGHTED, bool EDGES, int BUF>
__global__ void __launch_bounds__(kThreads)
node2vec_walk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                     const double* __restrict__ cum, const int64_t* __restrict__ start, int64_t S, int64_t L,
                     int64_t N, uint64_t seed, uint64_t thr0, uint64_t thr1, uint64_t thr2, int max_tries,
                     int64_t* __restrict__ out, int64_t* __restrict__ edge_out,
                     unsigned long long* __restrict__ flags) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  bool live = n < S;
  int64_t cur = live ? start[n] : 0;
  if (live && (cur < 0 || cur >= N)) {
    atomicOr(flags, 1ull);
    live = false;
  }
  const int64_t row = n * (L + 1), erow = n * L;
  const uint64_t stream = psa::rand_stream(seed, n);
  if (live) out[row] = cur;
  int64_t t = -1, ts = 0, te = 0;  // the previous node and its row
  for (int64_t l0 = 0; l0 < L; l0 += BUF) {
    int64_t buf[BUF], ebuf[EDGES ? BUF : 1];
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      const int64_t l = l0 + j;
      if (l < L) {  // uniform across the grid
        const int64_t s = live ? rowptr[cur] : 0;
        const int64_t deg = live ? rowptr[cur + 1] - s : 0;
        int64_t x = cur;
        const int64_t e =
            psa::node2vec_step<WEIGHTED>(col, cum, s, deg, t, ts, te, stream, l, thr0, thr1, thr2, max_tries, &x);
        t = cur, ts = s, te = s + deg;
        cur = x;
        buf[j] = cur;
        if (EDGES) ebuf[j] = e;
      }
    }
#pragma unroll
    for (int j = 0; j < BUF; ++j) {
      if (l0 + j < L && live) {
        out[row + l0 + j + 1] = buf[j];
        if (EDGES) edge_out[erow + l0 + j] = ebuf[j];
      }
    }
  }
}

template <bool WEIGHTED>
void walk_host(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N, const int64_t* start,
               int64_t S, int64_t L, uint64_t seed, uint64_t thr0, uint64_t thr1, uint64_t thr2, int max_tries,
               int64_t* out, int64_t* edge_out, int64_t* flags) {
  for (int64_t n = 0; n < S; ++n) {
    int64_t cur = start[n];
    if (cur < 0 || cur >= N) {
      *flags |= 1;
      continue;
    }
    const uint64_t stream = psa::rand_stream(seed, n);
    out[n * (L + 1)] = cur;
    int64_t t = -1, ts = 0, te = 0;
    for (int64_t l = 0; l < L; ++l) {
      const int64_t s = rowptr[cur], deg = rowptr[cur + 1] - s;
      int64_t x = cur;
      const int64_t e =
          psa::node2vec_step<WEIGHTED>(col, cum, s, deg, t, ts, te, stream, l, thr0, thr1, thr2, max_tries, &x);
      t = cur, ts = s, te = s + deg;
      cur = x;
      out[n * (L + 1) + l + 1] = cur;
      if (edge_out) edge_out[n * L + l] = e;
    }
  }
}

// The argument checks the two entry points share: 1 = run, 0 = nothing to do, < 0 = refused.
int check_args(const char* fn, const void* rowptr, const void* start, const void* out, const void* flags, int64_t N,
               int64_t S, int64_t L, uint64_t thr0, uint64_t thr1, uint64_t thr2, int max_tries) {
  const char* msg = nullptr;
  if (N < 0 || S < 0 || L < 0) msg = "negative size";
  else if (max_tries < 1 || max_tries > psa::kNode2vecMaxTries) msg = "max_tries outside [1, 32768]";
  else if (thr0 > psa::kNode2vecOne || thr1 > psa::kNode2vecOne || thr2 > psa::kNode2vecOne)
    msg = "a threshold above 2^53";
  else if (S == 0) return 0;
  else if (!rowptr || !start || !out || !flags) msg = "NULL pointer";
  else if (L >= INT64_MAX / S - 1) msg = "output too large";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

}  // namespace

extern "C" {

int psa_node2vec_walk(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N, const int64_t* start,
                      int64_t S, int64_t walk_length, uint64_t seed, uint64_t thr0, uint64_t thr1, uint64_t thr2,
                      int max_tries, int64_t* out, int64_t* edge_out, int64_t* flags, psa_stream_t stream) {
  const int go = check_args(__func__, rowptr, start, out, flags, N, S, walk_length, thr0, thr1, thr2, max_tries);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t b = psa::ceil_div(S, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many walks for one launch");
  const dim3 blocks(static_cast<unsigned>(b));
  hipStream_t s = psa::as_stream(stream);
  auto* f = reinterpret_cast<unsigned long long*>(flags);
#define PSA_WALK(W, E, B)                                                                                     \
  hipLaunchKernelGGL((node2vec_walk_kernel<W, E, B>), blocks, dim3(kThreads), 0, s, rowptr, col, cum, start, \
                     S, walk_length, N, seed, thr0, thr1, thr2, max_tries, out, edge_out, f)
  if (cum && edge_out) PSA_WALK(true, true, kBufEdges);
  else if (cum) PSA_WALK(true, false, kBuf);
  else if (edge_out) PSA_WALK(false, true, kBufEdges);
  else PSA_WALK(false, false, kBuf);
#undef PSA_WALK
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_node2vec_walk_host(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                           const int64_t* start, int64_t S, int64_t walk_length, uint64_t seed, uint64_t thr0,
                           uint64_t thr1, uint64_t thr2, int max_tries, int64_t* out, int64_t* edge_out,
                           int64_t* flags) {
  const int go = check_args(__func__, rowptr, start, out, flags, N, S, walk_length, thr0, thr1, thr2, max_tries);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  if (cum)
    walk_host<true>(rowptr, col, cum, N, start, S, walk_length, seed, thr0, thr1, thr2, max_tries, out, edge_out, flags);
  else
    walk_host<false>(rowptr, col, cum, N, start, S, walk_length, seed, thr0, thr1, thr2, max_tries, out, edge_out, flags);
  return PSA_OK;
}

}  // extern "C"
