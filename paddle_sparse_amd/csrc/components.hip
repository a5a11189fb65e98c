// Weakly connected components of a square sparse matrix, for gfx950: a lock-free union-find
// over the stored entries (union_find.h states the steps and why no interleaving of lanes can
// break them; the host export below runs the same text).  Three launches on one stream, none of
// them repeated: the number of launches depends on neither the diameter nor the data.
//
//   init     one lane per node: parent[v] = the first stored column of row v if it is a
//            smaller node, else v.
//   hook     one lane per stored entry over the COO pair (row[e], col[e]): coalesced reads, a
//            hub row is no special case.  An entry with an end outside [0, N) raises the flag
//            bit and joins nothing.
//   flatten  one lane per node: root[v] = the root of v, is_root[v] = (root[v] == v).
//
// The root of a component is its smallest node, whatever the schedule: a link always points
// the larger root at the smaller.  The caller ranks the roots (count2ptr over is_root) and
// gathers the labels.  256 lanes per workgroup; each grid covers its count and is not capped.
// No workspace: parent, root, is_root and flags are the caller's; every element of the first
// three is written on every path, flags is only ever OR-ed into.  No lane waits on another.
#include <initializer_list>

#include "common.h"
#include "union_find.h"

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads)
components_init_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N, int64_t nnz,
                       int64_t* __restrict__ parent) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (v >= N) return;
  parent[v] = psa::uf_first_parent(rowptr, col, nnz, v);
}

__global__ void __launch_bounds__(kThreads)
components_hook_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t nnz, int64_t N,
                       int64_t* parent, unsigned long long* __restrict__ flags) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= nnz) return;
  const int64_t flag = psa::uf_hook(parent, N, row[e], col[e]);
  if (flag) atomicOr(flags, static_cast<unsigned long long>(flag));
}

__global__ void __launch_bounds__(kThreads)
components_flatten_kernel(int64_t* parent, int64_t N, int64_t* __restrict__ root, int64_t* __restrict__ is_root) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (v >= N) return;
  const int64_t r = psa::uf_find(parent, v);
  root[v] = r;
  is_root[v] = r == v;
}

// The argument checks the entry points share: 1 = run, 0 = nothing to do, < 0 = refused.
// `count` is what the lanes run over; the pointers are those the call reads or writes.
int check_args(const char* fn, int64_t N, int64_t nnz, int64_t count, std::initializer_list<const void*> ptrs) {
  const char* msg = nullptr;
  if (N < 0 || nnz < 0) msg = "negative size";
  else if (count == 0) return 0;
  else
    for (const void* p : ptrs)
      if (!p) msg = "NULL pointer";
  if (!msg) return 1;
  psa::set_error(std::string(fn) + ": " + msg);
  return -1;
}

}  // namespace

extern "C" {

int psa_components_init(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t* parent,
                        psa_stream_t stream) {
  // col is read only where a row is not empty: it may be NULL when nothing is stored
  const int go = check_args(__func__, N, nnz, N, {rowptr, parent, nnz > 0 ? col : parent});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t b = psa::ceil_div(N, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many nodes for one launch");
  hipLaunchKernelGGL(components_init_kernel, dim3(static_cast<unsigned>(b)), dim3(kThreads), 0, psa::as_stream(stream),
                     rowptr, col, N, nnz, parent);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_components_hook(const int64_t* row, const int64_t* col, int64_t nnz, int64_t N, int64_t* parent, int64_t* flags,
                        psa_stream_t stream) {
  const int go = check_args(__func__, N, nnz, nnz, {row, col, flags, N > 0 ? parent : flags});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t b = psa::ceil_div(nnz, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many entries for one launch");
  hipLaunchKernelGGL(components_hook_kernel, dim3(static_cast<unsigned>(b)), dim3(kThreads), 0, psa::as_stream(stream),
                     row, col, nnz, N, parent, reinterpret_cast<unsigned long long*>(flags));
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_components_flatten(int64_t* parent, int64_t N, int64_t* root, int64_t* is_root, psa_stream_t stream) {
  const int go = check_args(__func__, N, 0, N, {parent, root, is_root});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  const int64_t b = psa::ceil_div(N, kThreads);
  PSA_REQUIRE(b <= 0x7fffffff, "too many nodes for one launch");
  hipLaunchKernelGGL(components_flatten_kernel, dim3(static_cast<unsigned>(b)), dim3(kThreads), 0,
                     psa::as_stream(stream), parent, N, root, is_root);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

int psa_components_host(const int64_t* rowptr, const int64_t* row, const int64_t* col, int64_t N, int64_t nnz,
                        int64_t* parent, int64_t* root, int64_t* is_root, int64_t* flags) {
  const int go = check_args(__func__, N, nnz, N + nnz,
                            {flags, N > 0 ? rowptr : flags, N > 0 ? parent : flags, N > 0 ? root : flags,
                             N > 0 ? is_root : flags, nnz > 0 ? row : flags, nnz > 0 ? col : flags});
  if (go <= 0) return go < 0 ? PSA_ERR_INVALID_ARG : PSA_OK;
  for (int64_t v = 0; v < N; ++v) parent[v] = psa::uf_first_parent(rowptr, col, nnz, v);
  for (int64_t e = 0; e < nnz; ++e) *flags |= psa::uf_hook(parent, N, row[e], col[e]);
  for (int64_t v = 0; v < N; ++v) {
    root[v] = psa::uf_find(parent, v);
    is_root[v] = root[v] == v;
  }
  return PSA_OK;
}

}  // extern "C"
