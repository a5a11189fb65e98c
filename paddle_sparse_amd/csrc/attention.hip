// Fused sparse attention, fp32: the entry points over attention_kernels.h (the plan is there), and what exists
// once for both formats.
//
//   psa_attention_fw / _bw_entries                  attention_fw / attention_bw
//   psa_attention_dropout_fw / _bw_entries          the same with the mask (A::kDrop)
//   psa_gat_attention_fw / _bw_entries              gat_fw / gat_bw (A::kGat)
//   psa_attention_workspace_bytes                   the long-row workspace of either format: the partials are fp32
//   psa_attention_dropout_mask                      keep [nnz, H] as bytes, for the unfused chain
#include "attention_kernels.h"

namespace {

// mask[e * H + h] = keep(e, h): the mask of the dropout forms as bytes, for the chain with the same mask.
__global__ void __launch_bounds__(kThreads)
attn_dropout_mask_kernel(int64_t total, int64_t H, uint64_t seed, uint32_t T, unsigned char* __restrict__ mask) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; t < total; t += step) {
    const int64_t e = t / H;
    mask[t] = psa::keep_of(psa::rand_stream(seed, e), t - e * H, T) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

size_t psa_attention_workspace_bytes(int64_t nnz, int64_t H, int64_t F) {
  if (nnz <= psa::kLongRow || H <= 0 || F <= 0) return 0;  // no row can be long
  return long_layout(nullptr, nnz, H, F, true).bytes;
}

int psa_attention_fw(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                     const float* bias, int64_t bias_heads, float scale, int64_t M, int64_t N, int64_t H, int64_t K,
                     int64_t F, int64_t nnz, float* out, float* stat, void* workspace, size_t workspace_bytes,
                     psa_stream_t stream) {
  return attention_fw<FwArgs<Fp32>>("psa_attention_fw", psa::Drop{}, PSA_F32, rowptr, col, q, k, v, bias, bias_heads,
                                    scale, M, N, H, K, F, nnz, out, stat, workspace, workspace_bytes, stream);
}

int psa_attention_bw_entries(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                             const float* bias, int64_t bias_heads, float scale, const float* grad_out,
                             const float* out, const float* stat, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F,
                             int64_t nnz, float* p, float* ds, void* workspace, size_t workspace_bytes,
                             psa_stream_t stream) {
  return attention_bw<BwArgs<Fp32>>("psa_attention_bw_entries", psa::Drop{}, PSA_F32, rowptr, col, q, k, v, bias,
                                    bias_heads, scale, grad_out, out, stat, M, N, H, K, F, nnz, p, ds, workspace,
                                    workspace_bytes, stream);
}

int psa_attention_dropout_fw(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                             const float* bias, int64_t bias_heads, float scale, double dropout_p, uint64_t seed,
                             int64_t M, int64_t N, int64_t H, int64_t K, int64_t F, int64_t nnz, float* out,
                             float* stat, void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_attention_dropout_fw", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  return attention_fw<FwDropArgs<Fp32>>("psa_attention_dropout_fw", drop, PSA_F32, rowptr, col, q, k, v, bias,
                                        bias_heads, scale, M, N, H, K, F, nnz, out, stat, workspace, workspace_bytes,
                                        stream);
}

int psa_attention_dropout_bw_entries(const int64_t* rowptr, const int64_t* col, const float* q, const float* k,
                                     const float* v, const float* bias, int64_t bias_heads, float scale,
                                     double dropout_p, uint64_t seed, const float* grad_out, const float* out,
                                     const float* stat, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F,
                                     int64_t nnz, float* p, float* ds, void* workspace, size_t workspace_bytes,
                                     psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_attention_dropout_bw_entries", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  return attention_bw<BwDropArgs<Fp32>>("psa_attention_dropout_bw_entries", drop, PSA_F32, rowptr, col, q, k, v, bias,
                                        bias_heads, scale, grad_out, out, stat, M, N, H, K, F, nnz, p, ds, workspace,
                                        workspace_bytes, stream);
}

int psa_attention_dropout_mask(int64_t nnz, int64_t H, double dropout_p, uint64_t seed, uint8_t* mask,
                               psa_stream_t stream) {
  PSA_REQUIRE(nnz >= 0 && H >= 1, "nnz must be at least 0 and H at least 1");
  PSA_REQUIRE(nnz < (int64_t{1} << 38) && H < (int64_t{1} << 24), "nnz or H too large");
  psa::Drop drop;
  if (!psa::make_drop("psa_attention_dropout_mask", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  if (nnz == 0) return PSA_OK;
  PSA_REQUIRE(mask, "NULL pointer");
  const int64_t total = nnz * H;
  const int64_t blocks = psa::ceil_div(total, kThreads);
  hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3(static_cast<unsigned>(blocks > 65536 ? 65536 : blocks)),
                     dim3(kThreads), 0, psa::as_stream(stream), total, H, seed, drop.T, mask);
  PSA_LAUNCH_CHECK();
  return PSA_OK;
}

// dropout_p == 0 takes the maskless instantiations: the same bits (every entry kept, times 1) without the draws.
int psa_gat_attention_fw(const int64_t* rowptr, const int64_t* col, const float* a_row, const float* a_col,
                         const float* v, const float* bias, int64_t bias_heads, float negative_slope, double dropout_p,
                         uint64_t seed, int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, float* out,
                         float* stat, void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_gat_attention_fw", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  if (dropout_p == 0.0) {
    return gat_fw<Fp32, false>("psa_gat_attention_fw", drop, PSA_F32, rowptr, col, a_row, a_col, v, bias, bias_heads,
                               negative_slope, M, N, H, F, nnz, out, stat, workspace, workspace_bytes, stream);
  }
  return gat_fw<Fp32, true>("psa_gat_attention_fw", drop, PSA_F32, rowptr, col, a_row, a_col, v, bias, bias_heads,
                            negative_slope, M, N, H, F, nnz, out, stat, workspace, workspace_bytes, stream);
}

int psa_gat_attention_bw_entries(const int64_t* rowptr, const int64_t* col, const float* a_row, const float* a_col,
                                 const float* v, const float* bias, int64_t bias_heads, float negative_slope,
                                 double dropout_p, uint64_t seed, const float* grad_out, const float* out,
                                 const float* stat, int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, float* p,
                                 float* dz, void* workspace, size_t workspace_bytes, psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_gat_attention_bw_entries", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  if (dropout_p == 0.0) {
    return gat_bw<Fp32, false>("psa_gat_attention_bw_entries", drop, PSA_F32, rowptr, col, a_row, a_col, v, bias,
                               bias_heads, negative_slope, grad_out, out, stat, M, N, H, F, nnz, p, dz, workspace,
                               workspace_bytes, stream);
  }
  return gat_bw<Fp32, true>("psa_gat_attention_bw_entries", drop, PSA_F32, rowptr, col, a_row, a_col, v, bias,
                            bias_heads, negative_slope, grad_out, out, stat, M, N, H, F, nnz, p, dz, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
