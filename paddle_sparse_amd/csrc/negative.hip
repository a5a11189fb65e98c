// Edge lookup and exact negative sampling on a CSR matrix sorted by (row, col), for gfx950: the
// link-prediction half that the scores of intersect.hip lack.  "Is (u, v) stored, and where?"
// is one lower-bound search in row u; a negative sample is that search inside a bounded
// rejection loop over proposals from the counter-based stream of rng.h (edge_lookup.h states
// both steps, and the host exports below run the same text).
//
// Both kernels run one lane per query or sample.  A lookup is about log2(deg) dependent 8-byte
// loads from one row, so the lanes of a wave walk unrelated rows and nothing is worth staging;
// the queries, the given rows and the outputs are read and written coalesced.  The grid covers
// the count and is not capped.  No workspace, no atomics on the outputs, no waiting on another
// workgroup; the one atomic is the OR into flags.  Every output element is written on every
// path (-1 where there is no answer), so an output buffer may hold anything before the call.
#include "common.h"
#include "edge_lookup.h"

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads)
edge_lookup_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t M, int64_t N,
                   const int64_t* __restrict__ row_q, const int64_t* __restrict__ col_q, int64_t Q,
                   int64_t* __restrict__ pos_out, unsigned long long* __restrict__ flags) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= Q) return;
  int64_t flag = 0;
  pos_out[q] = psa::edge_lookup_one(rowptr, col, M, N, row_q[q], col_q[q], &flag);
  if (flag) atomicOr(flags, static_cast<unsigned long long>(flag));
}

template <bool GIVEN_ROWS>
__global__ void __launch_bounds__(kThreads)
negative_sample_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t M, int64_t N,
                       const int64_t* __restrict__ src, int64_t count, int64_t k, bool no_self_loops, int max_tries,
                       uint64_t seed, int64_t* __restrict__ row_out, int64_t* __restrict__ col_out,
                       unsigned long long* __restrict__ flags) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= count) return;
  int64_t flag = 0, r = -1;
  const int64_t given = GIVEN_ROWS ? src[i / k] : 0;
  col_out[i] = psa::negative_try_loop<GIVEN_ROWS>(rowptr, col, M, N, given, i, no_self_loops, max_tries, seed, &r,
                                                  &flag);
  if (!GIVEN_ROWS) row_out[i] = r;
  if (flag) atomicOr(flags, static_cast<unsigned long long>(flag));
}

// The argument checks the entry points share: 1 = run, 0 = nothing to do, < 0 = refused.
int check_lookup(const char* fn, const void* rowptr, const void* row_q, const void* col_q, const void* pos_out,
                 const void* flags, int64_t M, int64_t N, int64_t Q) {
  const char* msg = nullptr;
  if (M < 0 || N < 0 || Q < 0) msg = "negative size";
  else if (Q == 0) return 0;
  else if (!rowptr || !row_q || !col_q || !pos_out || !flags) msg = "NULL pointer";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

int check_sample(const char* fn, const void* rowptr, const void* src, const void* row_out, const void* col_out,
                 const void* flags, int64_t M, int64_t N, int64_t S, int64_t k, int no_self_loops, int max_tries) {
  const char* msg = nullptr;
  if (M < 0 || N < 0 || S < 0) msg = "negative size";
  else if (k < 1) msg = "k must be >= 1";
  else if (max_tries < 1 || max_tries > psa::kNegativeMaxTries) msg = "max_tries outside [1, 32768]";
  else if (S > INT64_MAX / k) msg = "S * k overflows";
  else if (no_self_loops && M != N) msg = "no_self_loops needs a square matrix";
  else if (S == 0) return 0;
  else if (!rowptr || !col_out || !flags || (!src && !row_out)) msg = "NULL pointer";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

}  // namespace

extern "C" {

int psa_edge_lookup(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* row_q,
                    const int64_t* col_q, int64_t Q, int64_t* pos_out, int64_t* flags, psa_stream_t stream) {
  const int go = check_lookup(__func__, rowptr, row_q, col_q, pos_out, flags, M, N, Q);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t b = psa::ceil_div(Q, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many queries for one launch");
  hipLaunchKernelGGL(edge_lookup_kernel, dim3(static_cast<unsigned>(b)), dim3(kThreads), 0, psa::as_stream(stream),
                     rowptr, col, M, N, row_q, col_q, Q, pos_out, reinterpret_cast<unsigned long long*>(flags));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_edge_lookup_host(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* row_q,
                         const int64_t* col_q, int64_t Q, int64_t* pos_out, int64_t* flags) {
  const int go = check_lookup(__func__, rowptr, row_q, col_q, pos_out, flags, M, N, Q);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  for (int64_t q = 0; q < Q; ++q) pos_out[q] = psa::edge_lookup_one(rowptr, col, M, N, row_q[q], col_q[q], flags);
  return PSA_OK;
}

int psa_negative_sample(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* src, int64_t S,
                        int64_t k, int no_self_loops, int max_tries, uint64_t seed, int64_t* row_out, int64_t* col_out,
                        int64_t* flags, psa_stream_t stream) {
  const int go = check_sample(__func__, rowptr, src, row_out, col_out, flags, M, N, S, k, no_self_loops, max_tries);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t count = S * k, b = psa::ceil_div(count, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many samples for one launch");
  const dim3 blocks(static_cast<unsigned>(b));
  hipStream_t s = psa::as_stream(stream);
  auto* f = reinterpret_cast<unsigned long long*>(flags);
  if (src)
    hipLaunchKernelGGL(negative_sample_kernel<true>, blocks, dim3(kThreads), 0, s, rowptr, col, M, N, src, count, k,
                       no_self_loops != 0, max_tries, seed, row_out, col_out, f);
  else
    hipLaunchKernelGGL(negative_sample_kernel<false>, blocks, dim3(kThreads), 0, s, rowptr, col, M, N, src, count, k,
                       no_self_loops != 0, max_tries, seed, row_out, col_out, f);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_negative_sample_host(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* src,
                             int64_t S, int64_t k, int no_self_loops, int max_tries, uint64_t seed, int64_t* row_out,
                             int64_t* col_out, int64_t* flags) {
  const int go = check_sample(__func__, rowptr, src, row_out, col_out, flags, M, N, S, k, no_self_loops, max_tries);
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  for (int64_t i = 0; i < S * k; ++i) {
    int64_t r = -1;
    if (src) {
      col_out[i] = psa::negative_try_loop<true>(rowptr, col, M, N, src[i / k], i, no_self_loops != 0, max_tries, seed,
                                                &r, flags);
    } else {
      col_out[i] = psa::negative_try_loop<false>(rowptr, col, M, N, 0, i, no_self_loops != 0, max_tries, seed, &r,
                                                 flags);
      row_out[i] = r;
    }
  }
  return PSA_OK;
}

}  // extern "C"
