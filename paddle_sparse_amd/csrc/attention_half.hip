// Fused sparse attention with two-byte dense operands (bf16): the entry points over attention_kernels.h (the
// plan and what bf16 changes in it are there).  dtype: PSA_BF16 is served.
//
//   psa_attention_half_fw / _bw_entries             attention_fw / attention_bw
//   psa_attention_half_dropout_fw / _bw_entries     the same with the mask (A::kDrop)
//   psa_gat_attention_half_fw / _bw_entries         gat_fw / gat_bw (A::kGat)
#include "attention_kernels.h"

extern "C" {

int psa_attention_half_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                          const void* v, const float* bias, int64_t bias_heads, float scale, int64_t M, int64_t N,
                          int64_t H, int64_t K, int64_t F, int64_t nnz, void* out, float* stat, void* workspace,
                          size_t workspace_bytes, psa_stream_t stream) {
  return attention_fw<FwArgs<Bf16>>("psa_attention_half_fw", psa::Drop{}, dtype, rowptr, col, q, k, v, bias, bias_heads,
                                    scale, M, N, H, K, F, nnz, out, stat, workspace, workspace_bytes, stream);
}

int psa_attention_half_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                                  const void* v, const float* bias, int64_t bias_heads, float scale,
                                  const void* grad_out, const void* out, const float* stat, int64_t M, int64_t N,
                                  int64_t H, int64_t K, int64_t F, int64_t nnz, float* p, float* ds, void* workspace,
                                  size_t workspace_bytes, psa_stream_t stream) {
  return attention_bw<BwArgs<Bf16>>("psa_attention_half_bw_entries", psa::Drop{}, dtype, rowptr, col, q, k, v, bias,
                                    bias_heads, scale, grad_out, out, stat, M, N, H, K, F, nnz, p, ds, workspace,
                                    workspace_bytes, stream);
}

int psa_attention_half_dropout_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                                  const void* v, const float* bias, int64_t bias_heads, float scale, double dropout_p,
                                  uint64_t seed, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F, int64_t nnz,
                                  void* out, float* stat, void* workspace, size_t workspace_bytes,
                                  psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_attention_half_dropout_fw", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  return attention_fw<FwDropArgs<Bf16>>("psa_attention_half_dropout_fw", drop, dtype, rowptr, col, q, k, v, bias,
                                        bias_heads, scale, M, N, H, K, F, nnz, out, stat, workspace, workspace_bytes,
                                        stream);
}

int psa_attention_half_dropout_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* q,
                                          const void* k, const void* v, const float* bias, int64_t bias_heads,
                                          float scale, double dropout_p, uint64_t seed, const void* grad_out,
                                          const void* out, const float* stat, int64_t M, int64_t N, int64_t H,
                                          int64_t K, int64_t F, int64_t nnz, float* p, float* ds, void* workspace,
                                          size_t workspace_bytes, psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_attention_half_dropout_bw_entries", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  return attention_bw<BwDropArgs<Bf16>>("psa_attention_half_dropout_bw_entries", drop, dtype, rowptr, col, q, k, v,
                                        bias, bias_heads, scale, grad_out, out, stat, M, N, H, K, F, nnz, p, ds,
                                        workspace, workspace_bytes, stream);
}

// dropout_p == 0 takes the maskless instantiations: the same bits (every entry kept, times 1) without the draws.
int psa_gat_attention_half_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* a_row,
                              const void* a_col, const void* v, const float* bias, int64_t bias_heads,
                              float negative_slope, double dropout_p, uint64_t seed, int64_t M, int64_t N, int64_t H,
                              int64_t F, int64_t nnz, void* out, float* stat, void* workspace, size_t workspace_bytes,
                              psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_gat_attention_half_fw", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  if (dropout_p == 0.0) {
    return gat_fw<Bf16, false>("psa_gat_attention_half_fw", drop, dtype, rowptr, col, a_row, a_col, v, bias, bias_heads,
                               negative_slope, M, N, H, F, nnz, out, stat, workspace, workspace_bytes, stream);
  }
  return gat_fw<Bf16, true>("psa_gat_attention_half_fw", drop, dtype, rowptr, col, a_row, a_col, v, bias, bias_heads,
                            negative_slope, M, N, H, F, nnz, out, stat, workspace, workspace_bytes, stream);
}

int psa_gat_attention_half_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* a_row,
                                      const void* a_col, const void* v, const float* bias, int64_t bias_heads,
                                      float negative_slope, double dropout_p, uint64_t seed, const void* grad_out,
                                      const void* out, const float* stat, int64_t M, int64_t N, int64_t H, int64_t F,
                                      int64_t nnz, float* p, float* dz, void* workspace, size_t workspace_bytes,
                                      psa_stream_t stream) {
  psa::Drop drop;
  if (!psa::make_drop("psa_gat_attention_half_bw_entries", dropout_p, seed, &drop)) return PSA_ERR_INVALID_ARG;
  if (dropout_p == 0.0) {
    return gat_bw<Bf16, false>("psa_gat_attention_half_bw_entries", drop, dtype, rowptr, col, a_row, a_col, v, bias,
                               bias_heads, negative_slope, grad_out, out, stat, M, N, H, F, nnz, p, dz, workspace,
                               workspace_bytes, stream);
  }
  return gat_bw<Bf16, true>("psa_gat_attention_half_bw_entries", drop, dtype, rowptr, col, a_row, a_col, v, bias,
                            bias_heads, negative_slope, grad_out, out, stat, M, N, H, F, nnz, p, dz, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
