/*
 * paddle_sparse_hip.h — C-ABI of the MI355X (gfx950) sparse-op core.
 *
 * This is the drop-in boundary: the entry points a Paddle custom-op shim
 * (PD_BUILD_OP) binds in place of the reference's
 * csrc/cpu + csrc/cuda kernels.  Plain pointers and sizes only; no framework
 * types.  All pointers are DEVICE pointers (hipMalloc'd or framework-owned
 * HBM) unless a parameter says "host".  Every call enqueues work on `stream`
 * (a hipStream_t passed as void*) and returns without synchronising, exactly
 * like the reference's CUDA launchers (csrc/cuda/convert_cuda.cu:34-38).
 * Outputs are caller-allocated (the shim allocates them with the framework's
 * allocator, as the reference does with paddle::empty).
 *
 * Return value: PSA_OK (0) or a psa_status error; psa_last_error() gives the
 * message the shim should PD_THROW (reference errors are C++ exceptions,
 * csrc/cpu/utils.h:6-9).
 *
 * Index dtype is int64 everywhere (reference asserts it:
 * paddle_sparse/storage.py:61,94,101).  `reduce` strings of the Python API
 * ("sum"/"add"/"mean"/"min"/"max", paddle_sparse/testing.py:10) map to
 * psa_reduce.
 */
#ifndef PADDLE_SPARSE_HIP_H_
#define PADDLE_SPARSE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSA_ABI_VERSION 1

typedef void* psa_stream_t; /* hipStream_t */

typedef enum psa_status {
  PSA_OK = 0,
  PSA_ERR_INVALID_ARG = 1, /* bad pointer / size / enum */
  PSA_ERR_HIP = 2,         /* a HIP runtime call failed */
  PSA_ERR_WORKSPACE = 3,   /* workspace too small */
  PSA_ERR_UNSUPPORTED = 4  /* dtype / shape not supported by this build */
} psa_status;

typedef enum psa_reduce {
  PSA_SUM = 0, /* "sum" and "add" */
  PSA_MEAN = 1,
  PSA_MIN = 2,
  PSA_MAX = 3
} psa_reduce;

/* Value dtypes accepted by the dtype-generic entry points (gather, segment
 * reduce, coalesce).  SpMM is fp32 (the north-star dtype). */
typedef enum psa_dtype {
  PSA_F32 = 0,
  PSA_F64 = 1,
  PSA_I32 = 2,
  PSA_I64 = 3,
  PSA_F16 = 4,
  PSA_BF16 = 5
} psa_dtype;

/* ---- library ---------------------------------------------------------- */

/* Message of the last failing call on this host thread ("" if none). */
const char* psa_last_error(void);

/* PSA_ABI_VERSION the library was built with. */
int psa_abi_version(void);

/* Replaces sparse_cuda_version (csrc/version.cpp:14-22).  Always -1 on the
 * HIP build so that paddle_sparse/__init__.py:18-32 skips its CUDA-major
 * check. */
int64_t psa_sparse_cuda_version(void);

/* ---- index conversion (bit-exact) ------------------------------------- */

/* Replaces ind2ptr (csrc/convert.cpp:13-23 -> csrc/cuda/convert_cuda.cu:6-40,
 * CPU text csrc/cpu/convert_cpu.cpp:6-30).
 * ind: int64[numel], sorted ascending, values in [0, M).  out: int64[M+1],
 * out[r] = #{e : ind[e] < r}.  numel == 0 -> out is all zeros. */
int psa_ind2ptr(const int64_t* ind, int64_t numel, int64_t M, int64_t* out,
                psa_stream_t stream);

/* Replaces ptr2ind (csrc/convert.cpp:46-56 -> csrc/cuda/convert_cuda.cu:42-68,
 * CPU text csrc/cpu/convert_cpu.cpp:32-48).
 * ptr: int64[M+1], non-decreasing, ptr[0] >= 0, ptr[M] <= E.  out: int64[E];
 * out[e] = r for ptr[r] <= e < ptr[r+1].  Entries outside [ptr[0], ptr[M])
 * are left untouched (as in the reference). */
int psa_ptr2ind(const int64_t* ptr, int64_t M, int64_t E, int64_t* out,
                psa_stream_t stream);

/* ---- SpMM (CSR x dense), fp32 ------------------------------------------ */

/* out[i,:] = REDUCE_{e in [rowptr[i], rowptr[i+1])} w_e * mat[col[e], :]
 * with w_e = value[e], or 1 when value == NULL.
 *   PSA_SUM : plain sum.
 *   PSA_MEAN: sum / max(deg_i, 1).
 *   PSA_MIN/PSA_MAX: element-wise over k; arg_out[i,k] = e of the first
 *     winner in edge order; empty row -> out = 0, arg_out = nnz (sentinel).
 * Not in the reference tree (README.md:47-50 "Support later"); semantics are
 * upstream pytorch_sparse spmm (README.md:267-306 holds the API and one KAT).
 *
 * rowptr int64[M+1], col int64[nnz] (values in [0, N)), value f32[nnz] or
 * NULL, mat f32[N,K] row-major, out f32[M,K], arg_out int64[M,K] (MIN/MAX;
 * ignored for SUM/MEAN).  arg_out may be NULL for MIN/MAX too: it is then not
 * stored — 2 GB fewer writes at M = 2 M, K = 128; with arg_bytes NULL as well
 * the winners are not even tracked: 2.15 -> 1.60 ms, the sum's time — which is
 * what a caller wants that needs `out` only (inference), or whose backward
 * reads arg_bytes alone (complete when no row has more than 128 entries).
 * nnz is passed explicitly because rowptr lives on the device.
 *
 * arg_bytes: uint8[M,K] or NULL (MIN/MAX only, needs K % 4 == 0): arg_out once
 * more as the winner's index INSIDE its row, one byte per element (index mod
 * 128; bit 7 marks rows of more than 128 edges, where equal bytes name a
 * candidate that the backward checks against arg_out) — the form
 * psa_spmm_minmax_bw_csc reads.  The
 * forward has it in registers, so writing it here (0.26 GB at M = 2 M, K = 128)
 * saves the backward a pass that re-reads all of arg_out (2 GB).  With
 * arg_out == NULL the bytes must come from the kernel itself (K % 4 == 0 and
 * K <= 256); other K tiles return PSA_ERR_INVALID_ARG then.
 *
 * workspace (psa_spmm_workspace_bytes(reduce, K, nnz) bytes, 16-byte aligned)
 * enables the long-row path: rows with more than 128 edges are split into
 * 128-edge chunks reduced by separate wavefronts and folded in chunk order
 * (deterministic).  workspace == NULL keeps every row on one wavefront — same
 * results, but a power-law graph then waits for its longest row. */
size_t psa_spmm_workspace_bytes(int reduce, int64_t K, int64_t nnz);
int psa_spmm(int reduce, const int64_t* rowptr, const int64_t* col,
             const float* value, const float* mat, int64_t M, int64_t N,
             int64_t K, int64_t nnz, float* out, int64_t* arg_out,
             uint8_t* arg_bytes, void* workspace, size_t workspace_bytes,
             psa_stream_t stream);

/* psa_spmm with the COO row ids beside the CSR pointer: row int64[nnz] is what
 * SparseStorage.row() holds (paddle_sparse/storage.py:195-206), row[e] = r for
 * rowptr[r] <= e < rowptr[r+1]; NULL = not at hand (derived from rowptr into
 * the workspace when a kernel wants it — one psa_ptr2ind pass).  The
 * edge-balanced kernels read it: their unit of work is a range of consecutive
 * edges whatever rows they belong to, each lane group keeps the running
 * reduction of the current row in registers and stores a row when the id
 * changes; rows that cross a range boundary are folded in range order by a
 * second launch (deterministic), rows without edges are zero-filled from
 * rowptr by extra workgroups of the same launch.  That removes the per-row
 * rowptr -> col -> gather dependency chain which bounds the one-wave-per-row
 * kernels on power-law graphs.  Same results contract as psa_spmm (sums are
 * taken in edge order inside a range, so sum / mean may differ from the
 * row-wave kernels in the last bits; min / max / arg_out are identical).
 * ldo: floats between consecutive rows of `out` (0 = K): out may be a K-column
 * slice of a wider row-major matrix, so a product computed slice by slice
 * (the feature-sliced multi-GPU exchange) lands in place with no concatenation.
 * arg_out / arg_bytes, when given, stay dense [M, K].
 * hot_rows / num_hot (PSA_SPMM_EDGE_RANGES only; NULL / 0 = off): a compact
 * copy f32[num_hot, K] of the most referenced rows of mat.  Column ids in
 * [N, N + num_hot) then name row id - N of that copy instead of a row of mat.
 * Hub columns of a power-law graph draw a large share of all gathers to a few
 * rows of mat; where those rows sit at addresses that fall on few memory
 * channels (R-MAT as generated: hubs at ids with few bits set) the gather runs
 * at 3.7 TB/s instead of 5; from a compact copy — consecutive addresses, a few
 * MB that stay cache resident — R-MAT scale 21 goes 2.03 -> 1.43 ms.  The caller
 * keeps, per matrix, the list of hot columns and the redirected col array
 * (paddle_sparse_amd/storage.py::_hot_columns), and per call gathers the hot
 * rows of the current mat with psa_gather_rows (13 us for 65 536 rows).
 * arg_width: bytes per entry of arg_bytes, 1 (as psa_spmm) or 2 — (index in the
 * row) & 0xffff, exact up to 65 535 entries per row; see psa_spmm_minmax_bw_csc. */
typedef enum psa_spmm_algo {
  PSA_SPMM_AUTO = 0,        /* today: PSA_SPMM_ROW_WAVES */
  PSA_SPMM_ROW_WAVES = 1,   /* one wavefront per CSR row (+ the long-row chunks) */
  PSA_SPMM_EDGE_RANGES = 2  /* edge-balanced; shapes it does not serve (K % 4 != 0,
                               no workspace, ids beyond 31 bits) fall back to 1 */
} psa_spmm_algo;
int psa_spmm_coo(int reduce, const int64_t* rowptr, const int64_t* row,
                 const int64_t* col, const float* value, const float* mat,
                 const float* hot_rows, int64_t num_hot,
                 int64_t M, int64_t N, int64_t K, int64_t nnz, float* out,
                 int64_t ldo, int64_t* arg_out, void* arg_bytes, int arg_width,
                 int algo, void* workspace, size_t workspace_bytes,
                 psa_stream_t stream);

/* psa_spmm with half-width dense operands: mat and out are fp16 (PSA_F16) or
 * bf16 (PSA_BF16) [N, K] / [M, K] row-major, every product and sum is fp32 and
 * the result is rounded to the 2-byte type once, on store (round to nearest
 * even).  The reference parametrises its tests over float16 / bfloat16 / float32
 * / float64 values (paddle_sparse/testing.py:12-21).  value: fp32[nnz]
 * (value_dtype = PSA_F32), or `dtype`[nnz] (value_dtype = dtype), or NULL.
 * arg_out int64[M, K] or NULL (MIN / MAX).  The gathered rows are half as wide:
 * 2 M x 2 M, 20 M entries, K = 128 moves 6.4 GB instead of 11.5 GB.
 * Needs K % 8 == 0 and 16-byte aligned mat / out (PSA_ERR_UNSUPPORTED
 * otherwise: callers widen to fp32 and use psa_spmm).  One wavefront per row,
 * rows of any length on their own wave (no long-row scratch, no workspace).
 * N IS A CONTRACT, not a hint: it must be the number of rows of mat and bound every
 * column id (0 <= col[e] < N).  When N * K * 2 < 2^32 the kernels address mat with
 * 32-bit byte offsets built from the low 32 bits of col; a stale or short N gives
 * wrong gathers without any error (index values are never validated, as in the
 * reference: csrc/cpu/convert_cpu.cpp:19-27). */
int psa_spmm_half(int reduce, int dtype, const int64_t* rowptr,
                  const int64_t* col, const void* value, int value_dtype,
                  const void* mat, int64_t M, int64_t N, int64_t K, int64_t nnz,
                  void* out, int64_t* arg_out, psa_stream_t stream);

/* psa_spmm_half with the COO row ids, the kernel family and the hub-row copy of
 * psa_spmm_coo: on a power-law graph the one-wave-per-row kernel above waits for
 * its longest row (R-MAT scale 21, bf16, K = 128: 2.3 ms); the edge-range kernels
 * are the same code for 16-byte lanes of 8 two-byte elements.  value: fp32[nnz]
 * or NULL.  hot_rows: [num_hot, K] in mat's type.  algo != PSA_SPMM_EDGE_RANGES,
 * or a shape the edge ranges do not serve (K % 8 != 0, no workspace): forwards to
 * psa_spmm_half (hot_rows must then be NULL).  workspace:
 * psa_spmm_half_workspace_bytes(reduce, K, nnz) bytes, 16-byte aligned.  Sums are
 * taken in edge order inside a range, rows that cross ranges are folded from fp32
 * partials: sum / mean may differ from psa_spmm_half in the last bit of the
 * 2-byte result; min / max / arg_out are identical.  arg_bytes / arg_width (MIN / MAX): the
 * row-local form of arg_out as in psa_spmm_coo ([M, K] entries of 1 or 2 bytes, or NULL) — what the
 * half-width masked pass over the CSC view reads (psa_spmm_half_minmax_bw_csc), so that min / max
 * training on a power-law matrix needs neither an int64 arg_out nor fp32 copies of the operands. */
size_t psa_spmm_half_workspace_bytes(int reduce, int64_t K, int64_t nnz);
int psa_spmm_half_coo(int reduce, int dtype, const int64_t* rowptr,
                      const int64_t* row, const int64_t* col, const float* value,
                      const void* mat, const void* hot_rows, int64_t num_hot,
                      int64_t M, int64_t N, int64_t K, int64_t nnz, void* out,
                      int64_t* arg_out, void* arg_bytes, int arg_width, int algo,
                      void* workspace, size_t workspace_bytes, psa_stream_t stream);

/* sum / mean backward with BOTH gradients in one pass over the CSC view, half-width dense
 * operands (the fp32 form is psa_spmm_sum_bw_csc): mat f16/bf16 [N, K] (the forward's dense
 * operand), grad f16/bf16 [M, K], grad_mat f16/bf16 [N, K] out (fp32 sums, one rounding),
 * grad_value_csc f32[nnz] out in CSC order or NULL.  weight_csc: f32[nnz] = value[csr2csc] (CSC
 * order: psa_permute_apply_u32 / psa_transpose_weights) or NULL (weights 1); row_scale f32[M] or
 * NULL multiplies both gradients per entry (mean: 1 / max(deg(r), 1)).  One wave per column; with a
 * workspace of psa_spmm_half_bw_csc_workspace_bytes(K, nnz) bytes, columns above 128 entries (the hub
 * rows of a power-law matrix) are cut into 128-entry chunks with a wave each, whose fp32 partials are
 * added in chunk order (workspace NULL: every column on its one wave, whatever its length).
 * K % 8 == 0, K <= 512 (the dot <mat[c, :], grad[r, :]> needs the whole row in one tile), else
 * PSA_ERR_UNSUPPORTED.  The dtype list the reference parametrises over: paddle_sparse/testing.py:12-21. */
size_t psa_spmm_half_bw_csc_workspace_bytes(int64_t K, int64_t nnz);

/* psa_spmm_half that also leaves the row-local form of arg_out behind (min / max; arg_bytes: [M, K]
 * entries of arg_width bytes as in psa_spmm_coo, or NULL; arg_out and arg_bytes are both optional). */
int psa_spmm_half_arg(int reduce, int dtype, const int64_t* rowptr, const int64_t* col, const void* value,
                      int value_dtype, const void* mat, int64_t M, int64_t N, int64_t K, int64_t nnz, void* out,
                      int64_t* arg_out, void* arg_bytes, int arg_width, psa_stream_t stream);

/* min / max backward over the CSC view with half-width dense operands, both gradients in one pass (the
 * fp32 form is psa_spmm_minmax_bw_csc in its exact arg_bytes forms): an entry's term counts for column k
 * only where arg_bytes[r, k] equals the entry's tag (psa_csc_edge_tags, same width).  arg_bytes must be
 * exact (one byte: no row above 128 entries; two: none above 65 535).  weight_csc: f32[nnz] value[csr2csc]
 * or NULL; grad_value_csc f32[nnz] in CSC order or NULL; grad_mat in grad's dtype.  K % 8 == 0, K <= 512.
 * workspace: as for psa_spmm_half_sum_bw_csc (long columns in chunks), or NULL. */
int psa_spmm_half_minmax_bw_csc(int dtype, const int64_t* colptr, const int64_t* row_csc, const void* tag,
                                const float* weight_csc, const void* mat, const void* grad, const void* arg_bytes,
                                int arg_width, int64_t M, int64_t N, int64_t K, int64_t nnz, float* grad_value_csc,
                                void* grad_mat, void* workspace, size_t workspace_bytes, psa_stream_t stream);

int psa_spmm_half_sum_bw_csc(int dtype, const int64_t* colptr, const int64_t* row_csc, const float* weight_csc,
                             const float* row_scale, const void* mat, const void* grad, int64_t M, int64_t N,
                             int64_t K, int64_t nnz, float* grad_value_csc, void* grad_mat, void* workspace,
                             size_t workspace_bytes, psa_stream_t stream);

/* Test/bench hook: 0 = default (one row per wave), 1 = several rows per wave for
 * K <= 128, 2 = one row per wave with 8 gather steps in flight, 3 = default
 * without the XCD mixing of the row blocks, 4 = default with 64-bit addressing of the
 * dense operands forced (the form operands of 4 GiB and more take).  Returns the previous value. */
int psa_spmm_half_set_variant(int variant);

/* Row-length statistics of a CSR pointer, for choosing psa_spmm_algo once per
 * matrix (the caller reads the four words back and keeps the answer with the
 * matrix, like the reference keeps rowcount: paddle_sparse/storage.py:373-381).
 * stats int64[4] (device) = { rows without entries, rows with 1 or 2 entries,
 * rows with more than 128 entries, longest row }.  One wave per row is the
 * faster forward while most rows hold a handful of entries or more (uniform
 * 2 M x 2 M, 20 M entries, K = 128: 1.67 ms against 2.02 ms); edge ranges win
 * once empty and 1-2-entry rows dominate (R-MAT degrees, hub ids spread over the
 * address space: 1.51 ms against 1.89 ms). */
int psa_csr_row_stats(const int64_t* rowptr, int64_t M, int64_t* stats,
                      psa_stream_t stream);

/* ---- SpMM backward (fp32) ------------------------------------------------ */

/* grad wrt the sparse values for sum/mean (upstream spmm_value_bw):
 * out[e] = sum_k mat[col[e],k] * grad[row(e),k], divided by max(deg(row(e)),1)
 * for PSA_MEAN.  row(e) is implied by rowptr (one wave per CSR row), so the
 * upstream `row` argument is not needed.  out: f32[nnz].  workspace
 * (psa_spmm_value_bw_workspace_bytes(nnz) bytes, or NULL) holds the work list
 * of the long-row path, as for psa_spmm. */
size_t psa_spmm_value_bw_workspace_bytes(int64_t nnz);
int psa_spmm_value_bw(int reduce, const int64_t* rowptr, const int64_t* col,
                      const float* mat, const float* grad, int64_t M, int64_t K,
                      int64_t nnz, float* out, void* workspace,
                      size_t workspace_bytes, psa_stream_t stream);

/* CSC-ordered edge weights for grad wrt the dense operand (sum/mean):
 * out[j] = (value ? value[csr2csc[j]] : 1) / (mean ? max(deg(row_csc[j]),1) : 1)
 * with row_csc = row[csr2csc].  gB = psa_spmm(PSA_SUM, colptr, row_csc, out,
 * gOut) — upstream torch_sparse/matmul.py spmm_sum/spmm_mean backward. */
int psa_transpose_weights(const float* value, const int64_t* csr2csc,
                          const int64_t* row_csc, const int64_t* rowptr,
                          int64_t nnz, int mean, float* out,
                          psa_stream_t stream);

/* min/max backward through arg_out (entries == nnz are masked):
 *   grad_value[arg] += mat[col[arg],k] * grad[i,k]   (f32[nnz], or NULL)
 *   grad_mat[col[arg],k] += w_arg * grad[i,k]        (f32[N,K], or NULL)
 * Both outputs are zero-filled by the call; accumulation uses float atomics
 * (summation order is not fixed; results agree to fp32 rounding). */
int psa_spmm_minmax_bw(const int64_t* col, const float* value, const float* mat,
                       const float* grad, const int64_t* arg_out, int64_t M,
                       int64_t N, int64_t K, int64_t nnz, float* grad_value,
                       float* grad_mat, psa_stream_t stream);

/* min/max backward WITHOUT atomics, in one pass over the CSC view of the
 * matrix (the caches storage.py:425-434 / tensor.py:254-257 already keep for
 * the sum/mean backward).  For column c and each stored entry e = (r, c):
 *   grad_mat[c, k]  += w_e * grad[r, k]        where arg_out[r, k] == e
 *   grad_value_csc[j] = sum of mat[c, k] * grad[r, k] over those k   (j = CSC
 *                       position of e, i.e. e = csr2csc[j])
 * Scattered float atomics run at ~20-50 G adds/s on this chip whatever their
 * shape (256 M of them at M = 2 M, K = 128: 5 ms); this pass is a gather like
 * the forward, every output element is written once and sums run in CSC edge
 * order (reproducible bit for bit).
 *
 * tag: uint8[nnz] from psa_csc_edge_tags (depends on the sparsity structure
 * only: cache it with csr2csc).  value: f32[nnz] in CSR order, or NULL.
 * arg_bytes: what psa_spmm left behind (see there), or NULL — the call then
 * derives it from arg_out itself in a first pass.  arg_out may be NULL when
 * arg_bytes is given and no row has more than 128 entries (entries of longer
 * rows need the exact test against arg_out; without it they count as no hit).
 * grad_value_csc: f32[nnz] or NULL (then mat may be NULL too); it is written in
 * CSC order, contiguously — psa_gather_rows(grad_value_csc, csc2csr, nnz, 4, ..)
 * puts it into the CSR order the API returns (a 4-byte scatter from inside the
 * pass costs more than that gather).
 * workspace: psa_spmm_minmax_bw_csc_workspace_bytes(M, K, nnz) bytes, 16-byte
 * aligned (arg_out compressed to its row-local form + long-column scratch).
 * Returns PSA_ERR_UNSUPPORTED unless K % 4 == 0 and K <= 256 (callers then
 * use psa_spmm_minmax_bw).
 *
 * arg_width (1 or 2): bytes per entry of arg_bytes and of tag — the width
 * psa_spmm_coo wrote and psa_csc_edge_tags was asked for.  Width 2 holds
 * (index in the row) & 0xffff: exact for rows of up to 65 535 entries (0xffff, like 0xff in the one-byte form, says "no winner": empty row, or no product beat the init), so on a
 * power-law graph (R-MAT scale 21: longest row 41 677) the forward stores
 * 2 bytes per element instead of 8 + 1 and this pass needs no arg_out.
 *
 * hot_grad f32[num_hot, K] / hot_bytes [num_hot, K] entries / num_hot (NULL,
 * NULL, 0 = off): compact copies of the most referenced rows of grad and of
 * arg_bytes.  Ids in [M, M + num_hot) in row_csc then name row id - M of the
 * copies (the hub rows of a power-law graph, as hot_rows of psa_spmm_coo;
 * R-MAT scale 21 as generated: the pass runs 1.9 ms faster with the hubs'
 * rows relabelled away from their crowded addresses).  Needs the two-byte
 * arg_bytes (arg_width 2, arg_out NULL): a matrix whose rows all fit the
 * one-byte form has no hub rows to speak of. */
int psa_csc_edge_tags(const int64_t* rowptr, const int64_t* row_csc,
                      const int64_t* csr2csc, int64_t nnz, void* tag,
                      int width, psa_stream_t stream);
size_t psa_spmm_minmax_bw_csc_workspace_bytes(int64_t M, int64_t K, int64_t nnz);
int psa_spmm_minmax_bw_csc(const int64_t* rowptr, const int64_t* colptr,
                           const int64_t* row_csc, const int64_t* csr2csc,
                           const void* tag, const float* value,
                           const float* mat, const float* grad,
                           const int64_t* arg_out, const void* arg_bytes,
                           int arg_width, const float* hot_grad,
                           const void* hot_bytes, int64_t num_hot,
                           int64_t M, int64_t N,
                           int64_t K, int64_t nnz, float* grad_value_csc,
                           float* grad_mat, void* workspace,
                           size_t workspace_bytes, psa_stream_t stream);

/* Gradient wrt the dense operand of spmm_min / spmm_max for a FIXED adjacency on a
 * power-law matrix: the edge-range kernels of psa_spmm_coo over the CSC view, with
 * the term of an entry counted only where the forward's row-local arg_out names it
 *   grad_mat[c, k] = sum over entries e = (r, c) with arg_bytes[r, k] == tag[e] of
 *                    weight_csc[e] * grad[r, k]
 * (two gathers per entry: the row of grad and its row of arg_bytes).  No
 * grad_value: callers that train the edge values use psa_spmm_minmax_bw_csc.
 * col_csc: int64[nnz], the column of every CSC-ordered entry (the COO row ids of
 * the view), or NULL (derived from colptr into the workspace).  row_csc, tag,
 * arg_bytes / arg_width, hot_grad / hot_bytes / num_hot: as psa_spmm_minmax_bw_csc;
 * arg_bytes must be exact (one byte: no row above 128 entries; two bytes: none above
 * 65 535).  weight_csc: f32[nnz] = value[csr2csc] (psa_transpose_weights) or NULL
 * (weights 1).  Sums run in entry order inside a range and range by range for
 * columns that cross ranges: deterministic, last bits may differ from
 * psa_spmm_minmax_bw_csc.  R-MAT scale 21, K = 128: 2.7 -> 2.0 ms.
 * workspace: psa_spmm_minmax_bw_eb_workspace_bytes(K, nnz) bytes, 16-byte aligned.
 * PSA_ERR_UNSUPPORTED unless K % 4 == 0 and every id fits 31 bits. */
size_t psa_spmm_minmax_bw_eb_workspace_bytes(int64_t K, int64_t nnz);
int psa_spmm_minmax_bw_eb(const int64_t* colptr, const int64_t* col_csc,
                          const int64_t* row_csc, const void* tag,
                          const float* weight_csc, const float* grad,
                          const void* arg_bytes, int arg_width,
                          const float* hot_grad, const void* hot_bytes,
                          int64_t num_hot, int64_t M, int64_t N, int64_t K,
                          int64_t nnz, float* grad_mat, void* workspace,
                          size_t workspace_bytes, psa_stream_t stream);

/* sum backward with BOTH gradients in one pass over the CSC view (trainable
 * edge values): for column c and each stored entry e = (r, c)
 *   grad_mat[c, :] += value[e] * grad[r, :]      (value NULL: weights 1)
 *   grad_value_csc[j] = <mat[c, :], grad[r, :]>   (j = CSC position of e)
 * The gathered grad row serves both, mat[c, :] is the column's own row, and
 * value is read through csr2csc — so the separate psa_spmm_value_bw (a second
 * full gather, of mat rows) and psa_transpose_weights passes are not needed.
 * csr2csc = NULL: `value` is in CSC order already (value[csr2csc], e.g. from
 * psa_permute_apply_u32: 0.12 ms at 20 M entries) and is read as a stream — the
 * nnz dependent 4-byte reads value[csr2csc[j]] were 18 % of this pass's memory
 * requests (profiles/r03_pmc_backward.json).  psa_spmm_minmax_bw_csc takes the
 * same convention when arg_out is NULL (the exact arg_bytes forms).
 * row_scale: f32[M] or NULL; with it both gradients carry the factor
 * row_scale[r] (mean: 1 / max(deg(r), 1), folded in per edge instead of a
 * pre-scaling pass over grad).
 * grad_value_csc: f32[nnz] in CSC order or NULL (CSR order: psa_gather_rows
 * through csc2csr, as above).  hot_grad f32[num_hot, K] / num_hot (NULL / 0 =
 * off): compact copy of the most referenced rows of grad; ids in
 * [M, M + num_hot) in row_csc name its rows (row_scale then has M + num_hot
 * entries, the copies' scales at the end).  M = rows of grad.  workspace:
 * psa_spmm_sum_bw_csc_workspace_bytes(K, nnz) bytes, 16-byte aligned.
 * PSA_ERR_UNSUPPORTED unless K % 4 == 0 and K <= 256. */
size_t psa_spmm_sum_bw_csc_workspace_bytes(int64_t K, int64_t nnz);
int psa_spmm_sum_bw_csc(const int64_t* colptr, const int64_t* row_csc,
                        const int64_t* csr2csc, const float* value,
                        const float* row_scale, const float* mat,
                        const float* grad, const float* hot_grad,
                        int64_t num_hot, int64_t M, int64_t N,
                        int64_t K, int64_t nnz, float* grad_value_csc,
                        float* grad_mat, void* workspace,
                        size_t workspace_bytes, psa_stream_t stream);

/* Test/bench hook: choose the SpMM kernel variant for subsequent psa_spmm
 * calls of this process (0 = auto).  Returns the previous value.  Variants
 * compute identical results up to fp32 summation order; listed in DESIGN.md. */
int psa_spmm_set_variant(int variant);

/* ---- index_sort: stable LSD radix sort (bit-exact permutation) ----------- */

/* Replaces index_sort (paddle_sparse/utils.py:14-23: `inputs.argsort()`),
 * whose call sites are the constructor sort (storage.py:164-169), csr2csc
 * (storage.py:430-432) and csc2csr (storage.py:444-445).
 * keys: int64[n], values in [0, max_value) — max_value is the hint the
 * reference signature already carries (M*N); it selects the number of 8-bit
 * passes.  perm_out: int64[n], the STABLE sorting permutation
 * (== numpy argsort(kind="stable")); sorted_out: int64[n] or NULL.
 * keys is not modified.  workspace: psa_index_sort_workspace_bytes(n,
 * max_value) bytes of device memory, 16-byte aligned.  n < 2^31. */
size_t psa_index_sort_workspace_bytes(int64_t n, int64_t max_value);
int psa_index_sort(const int64_t* keys, int64_t n, int64_t max_value,
                   int64_t* sorted_out, int64_t* perm_out, void* workspace,
                   size_t workspace_bytes, psa_stream_t stream);

/* Diagnostic (synchronises the stream): 0 if the last psa_index_sort /
 * psa_sort_pairs_u32 that used `workspace` (same n, max_value) finished every
 * inter-workgroup wait normally, 1 if a bounded spin of the look-back gave up
 * (never expected; results are then invalid), -1 if the flag could not be read.
 * A sort never hands back a wrong order unmarked (the reference's argsort cannot,
 * storage.py:164-169): once a wait gave up, the last pass stores -1 over its share
 * of perm_out / sorted_out instead of positions.  Callers with no host read behind
 * the sort (the SparseStorage constructor, csr2csc) call this and raise. */
int psa_index_sort_status(const void* workspace, int64_t n, int64_t max_value,
                          psa_stream_t stream);

/* Same sort carrying a caller-defined 4-byte payload per key instead of the
 * permutation: payload_out[i] = payload[perm[i]] (any 4-byte dtype: fp32 /
 * int32 values of a COO matrix).  Lets coalesce (storage.py:164-169 + :471)
 * keep `value[perm]` a sequential stream instead of a random gather.
 * sorted_out is required.  Workspace as psa_index_sort. */
int psa_sort_pairs_u32(const int64_t* keys, const void* payload, int64_t n,
                       int64_t max_value, int64_t* sorted_out, void* payload_out,
                       void* workspace, size_t workspace_bytes, psa_stream_t stream);

/* psa_sort_pairs_u32 on a BIT FIELD of the keys: stable order by
 * (keys[i] >> first_bit), which must be < max_value; the bits below first_bit
 * are not looked at and travel inside the key.  With keys packed as
 * (hi << 32) | lo this orders by `hi` alone in ceil(log2(max_value) / 8) passes
 * while `lo` comes along for free — e.g. products grouped by output column
 * (lo) brought into (row, col) order by ONE sort on the row field.  Workspace:
 * psa_index_sort_workspace_bytes(n, max_value). */
int psa_sort_pairs_u32_field(const int64_t* keys, const void* payload, int64_t n,
                             int first_bit, int64_t max_value,
                             int64_t* sorted_out, void* payload_out,
                             void* workspace, size_t workspace_bytes,
                             psa_stream_t stream);

/* Stable merge of two SORTED key arrays: merged_out[na + nb] is what a stable
 * sort of the concatenation [a; b] would give (a's entry first on equal keys)
 * — the "cat, then argsort" of add.py:30-47, mul.py:57-73 and tensor.py:415-451
 * when both halves are sorted already, in one streaming launch (merge path)
 * instead of ceil(bits / 8) radix passes.  source_out (or NULL) receives the index into
 * the concatenation every merged key came from (i for a[i], na + j for b[j]) —
 * the permutation psa_index_sort would return; payload_out (or NULL; then
 * payload_a / payload_b are ignored) receives the 4-byte payloads in merged
 * order.  Unsorted inputs give an unspecified (memory-safe) order. */
int psa_merge_sorted(const int64_t* a, int64_t na, const int64_t* b, int64_t nb,
                     const void* payload_a, const void* payload_b,
                     int64_t* merged_out, int64_t* source_out, void* payload_out,
                     psa_stream_t stream);

/* Small inputs (n <= psa_coalesce_small_max(), 40960): the sort by (row, col)
 * AND the run-length structure of a coalesce (storage.py:158-171 + 455-470) in
 * one launch of one workgroup — at BASELINE config 1 (10 k entries) the
 * multi-launch chain is pure launch latency.  Outputs are sized for the worst
 * case: out_row / out_col / perm int64[n], ptr int64[n + 1]; on return
 * count_out[0] (device) = number of distinct (row, col), out_row/out_col[0:count]
 * the sorted distinct pairs, ptr[0:count + 1] the run starts in sorted order,
 * perm the stable sorting permutation (same bits as psa_index_sort).
 * workspace: psa_coalesce_small_workspace_bytes(n) bytes, 16-byte aligned. */
int64_t psa_coalesce_small_max(void);
size_t psa_coalesce_small_workspace_bytes(int64_t n);
int psa_coalesce_small(const int64_t* row, const int64_t* col, int64_t n,
                       int64_t M, int64_t N, int64_t* out_row, int64_t* out_col,
                       int64_t* ptr, int64_t* perm, int64_t* count_out,
                       void* workspace, size_t workspace_bytes,
                       psa_stream_t stream);

/* ---- coalesce(index, value, m, n, op) in two calls -------------------------
 * What the reference's user gets from ONE call (paddle_sparse/coalesce.py:25-29
 * = SparseStorage(is_sorted=False) storage.py:158-171 + storage.coalesce
 * storage.py:454-486), with the one host read the dynamic output size needs:
 *
 *   psa_coalesce_count(...)          keys row * N + col, stable sort, run count
 *   host reads status[0] (= count)   <- the only synchronisation
 *   psa_coalesce_write(...)          [2, count] index + reduced values
 *
 * status = the first two int64 words of the workspace: status[0] = number of
 * distinct (row, col) pairs; status[1] = flags, bit 0: some row/col lies outside
 * [0, M) x [0, N) (the reference asserts this, storage.py:78-91: raise, the
 * outputs are unspecified then), bit 1: the input was not sorted by (row, col),
 * bit 2: an inter-workgroup wait of the sort gave up (never expected; the outputs
 * are invalid — the same word psa_index_sort_status reads).
 * psa_coalesce_write takes the count from the device, so a caller may also
 * allocate worst-case outputs (n rows), enqueue both calls back to back and read
 * the status afterwards (count < 0 in the call = "not read yet").
 *
 * value: [n, D] of `dtype` (psa_dtype) or NULL; fp32 / int32 scalars (D = 1) ride
 * through the sort as its payload.  index_out: int64[2 * rows] with rows >= count,
 * filled as the contiguous [2, count] index (row' then col'); value_out [rows, D].
 * n <= 10240 runs as one workgroup whose radix sort stays in the LDS (two
 * launches in all); larger inputs use psa_index_sort / psa_sort_pairs_u32,
 * psa_unique_* and psa_segment_reduce.  transpose(index, value, m, n)
 * (paddle_sparse/transpose.py:41-65) is the same two calls with row/col and M/N
 * swapped.  workspace: psa_coalesce_workspace_bytes(n, M, N) bytes, 16-byte
 * aligned, untouched between the two calls.
 * Non-finite values (every form of the chain, psa_coalesce_small_fused included):
 * min / max give NaN for an entry whose duplicates hold one, at any position; sum /
 * mean are IEEE (+inf and -inf together give NaN); the sign of a zero min / max on
 * a +0 / -0 tie is unspecified. */
size_t psa_coalesce_workspace_bytes(int64_t n, int64_t M, int64_t N);
int psa_coalesce_count(const int64_t* row, const int64_t* col, const void* value,
                       int dtype, int64_t D, int64_t n, int64_t M, int64_t N,
                       void* workspace, size_t workspace_bytes,
                       psa_stream_t stream);
int psa_coalesce_write(const void* value, int dtype, int64_t D, int64_t n,
                       int64_t M, int64_t N, int reduce, int64_t count,
                       const void* workspace, int64_t* index_out,
                       void* value_out, psa_stream_t stream);

/* The whole coalesce in ONE launch, for n <= psa_coalesce_small_max_fused() (10 240)
 * entries with no values or fp32 / int32 scalar values (BASELINE config 1): the
 * one-workgroup LDS sort of the chain above also writes the contiguous [2, count]
 * index into index_out (int64[2 n] capacity) and reduces every run of values into
 * value_out ([n] capacity).  status int64[2] (device) = {count, flags} as above;
 * the caller reads it once after the launch.  No workspace. */
int psa_coalesce_small_max_fused(void);
int psa_coalesce_small_fused(const int64_t* row, const int64_t* col,
                             const void* value, int dtype, int64_t n, int64_t M,
                             int64_t N, int reduce, int64_t* index_out,
                             void* value_out, int64_t* status,
                             psa_stream_t stream);

/* psa_make_keys for (row, col) with the reference's range assertions folded in:
 * keys[i] = row[i] * N + col[i]; status int64[4] (device): status[1] gets bit 0
 * when some row/col lies outside [0, M) x [0, N), bit 1 when keys[i] < keys[i-1]
 * for some i (storage.py:163); status[0] is zeroed, status[2..3] are scratch. */
int psa_make_keys_checked(const int64_t* row, const int64_t* col, int64_t n,
                          int64_t M, int64_t N, int64_t* keys, int64_t* status,
                          psa_stream_t stream);

/* ---- a 4-byte array through a FIXED permutation, planned ---------------------- */

/* dst[i] = src[perm[i]] for 4-byte elements, n < 2^31, as two streaming passes over a plan
 * built once per permutation (csrc/permute.hip) instead of n dependent 4-byte reads: the
 * value[csr2csc] gathers of tensor.py:254-257 / transpose.py:19-22 and the way of grad_value
 * from CSC back to CSR order.  T = psa_permute_tile() (32 768).
 * Plan (structure only, 8 bytes per element), with dest = the INVERSE of perm (dest[s] = where
 * source s goes), tile(s) = s / T, block(s) = dest[s] / T:
 *   perm_ts  = stable sorting permutation of the keys tile(s) * ceil(n / T) + block(s)
 *   perm_mid = stable sorting permutation of block(s);  gslot = its inverse
 *   psa_permute_plan_pack(perm_ts, gslot, perm_mid, dest, n, sl, gs, lo):
 *     sl: uint16[n], gs: int32[n], lo: uint16[n]
 * psa_permute_apply_u32: mid = scratch of n 4-byte elements; src, mid, dst distinct. */
int64_t psa_permute_tile(void);
int psa_permute_plan_pack(const int64_t* perm_ts, const int64_t* gslot, const int64_t* perm_mid,
                          const int64_t* dest, int64_t n, void* sl, void* gs, void* lo, psa_stream_t stream);
int psa_permute_apply_u32(const void* src, const void* sl, const void* gs, const void* lo, int64_t n, void* mid,
                          void* dst, psa_stream_t stream);

/* Test/bench hook: scatter kernel variant of psa_index_sort for this process
 * (0 = production: single-sweep passes with decoupled look-back, 512 threads x
 * 16 keys; 5 = the same with 1024 x 8; 1-4, 7 = histogram / scan / scatter
 * per pass with 2048-key LDS tile, direct per-lane stores, 4096- / 8192-key
 * tiles).  Returns the previous value.  All variants produce the same bits. */
int psa_sort_set_variant(int variant);

/* Test hook: polls a look-back wait of the single-sweep passes may spend on a word that is
 * not ready before it gives up and raises the fault word (production: 2^22; 0 makes every
 * wait that does not succeed at once give up; negative restores the default).  Returns the
 * previous value. */
int64_t psa_sort_set_spin_limit(int64_t limit);

/* keys[i] = a[i] * mul + b[i]  (storage.py:159-162 key = row*N + col,
 * storage.py:430 key = M*col + row).  If unsorted_flag != NULL, *unsorted_flag
 * (device int32, caller-zeroed) is set to 1 when some keys[i] < keys[i-1]
 * (the reference's sortedness test, storage.py:163). */
int psa_make_keys(const int64_t* a, const int64_t* b, int64_t mul, int64_t n,
                  int64_t* keys, int32_t* unsorted_flag, psa_stream_t stream);

/* The inverse of psa_make_keys on a (sorted) key stream: hi[i] = keys[i] / div,
 * lo[i] = keys[i] % div; either output may be NULL.  Replaces the row[perm] /
 * col[perm] gathers after a sort (storage.py:166-168, tensor.py:254-257,
 * transpose.py:14-16) with one sequential pass: the sorted keys already hold
 * both indices. */
int psa_split_keys(const int64_t* keys, int64_t n, int64_t div, int64_t* hi,
                   int64_t* lo, psa_stream_t stream);

/* out[i, :] = src[perm[i], :] for rows of row_bytes bytes (any dtype):
 * the `x[perm]` gathers of storage.py:166-169, transpose.py:14-22,
 * tensor.py:252-257. */
int psa_gather_rows(const void* src, const int64_t* perm, int64_t n,
                    int64_t row_bytes, void* out, psa_stream_t stream);

/* psa_gather_rows on a column window of the source rows: out[i, :] = the
 * width_bytes bytes at offset_bytes of row perm[i] of src, whose rows are
 * src_row_bytes apart; out is dense [n, width_bytes].  Packs the rows (and the
 * feature slice) of the dense operand another rank asked for into its send
 * buffer (row-partitioned SpMM, halo exchange: paddle_sparse_amd/distributed.py). */
int psa_gather_rows_window(const void* src, int64_t src_row_bytes,
                           int64_t offset_bytes, int64_t width_bytes,
                           const int64_t* perm, int64_t n, void* out,
                           psa_stream_t stream);

/* inv[perm[i]] = i.  Same result as the reference's second sort in csc2csr
 * (storage.py:444-445 sorts a permutation to invert it), in one pass. */
int psa_invert_permutation(const int64_t* perm, int64_t n, int64_t* inv,
                           psa_stream_t stream);

/* out[b] = #{i : index[i] == b} for b in [0, size): colcount
 * (storage.py:414-418, scatter_add of ones).  out: int64[size]. */
int psa_bincount(const int64_t* index, int64_t n, int64_t size, int64_t* out,
                 psa_stream_t stream);

/* ptr_out[0] = 0, ptr_out[i+1] = counts[0] + ... + counts[i]: colptr from
 * colcount (storage.py:397-398, zeros + cumsum).  ptr_out: int64[n+1]. */
size_t psa_count2ptr_workspace_bytes(int64_t n);
int psa_count2ptr(const int64_t* counts, int64_t n, int64_t* ptr_out,
                  void* workspace, size_t workspace_bytes, psa_stream_t stream);

/* ---- coalesce on sorted keys (storage.py:454-486) ------------------------ */

/* Phase 1: *count_out (device int64) = number of distinct values in
 * sorted_keys[n] (the reference's mask.sum(); mask.all() <=> count == n).
 * workspace: psa_unique_workspace_bytes(n) bytes; it carries per-block
 * offsets into phase 2 and must stay untouched in between. */
size_t psa_unique_workspace_bytes(int64_t n);
int psa_unique_count(const int64_t* sorted_keys, int64_t n, void* workspace,
                     size_t workspace_bytes, int64_t* count_out,
                     psa_stream_t stream);
/* psa_unique_count on the output of psa_index_sort / psa_sort_pairs_u32, folding in
 * the sort's look-back diagnostic: count_out int64[2] (device) = {count, fault},
 * fault != 0 when a bounded inter-workgroup wait of a radix pass gave up (never
 * expected; the order is then invalid).  sort_workspace / sort_max_value: what the
 * sort was called with (its workspace must still be alive); n is the same n.
 * The caller reads both words in its one host read of the count. */
int psa_unique_count_after_sort(const int64_t* sorted_keys, int64_t n,
                                void* workspace, size_t workspace_bytes,
                                const void* sort_workspace, int64_t sort_max_value,
                                int64_t* count_out, psa_stream_t stream);

/* Phase 2 (after the caller has read the count and sized the outputs):
 * ptr_out int64[count+1] = start of every run of equal keys, ptr_out[count]
 * = n (the reference's `ptr`, storage.py:467-470); row_out/col_out
 * int64[count] = key / N, key % N of each distinct key (the reference's
 * row[mask], col[mask], storage.py:462-463).  Any of ptr_out or the
 * (row_out, col_out) pair may be NULL.  count: the device scalar written by
 * phase 1. */
int psa_unique_write(const int64_t* sorted_keys, int64_t n, int64_t N,
                     const void* workspace, const int64_t* count,
                     int64_t* ptr_out, int64_t* row_out, int64_t* col_out,
                     psa_stream_t stream);

/* psa_unique_write (packed index, no ptr) and psa_segment_reduce in ONE launch, for 4-byte values
 * (PSA_F32 / PSA_I32) that are in SORTED order already — they rode the sort as its payload
 * (psa_sort_pairs_u32) or the input was sorted: index_out int64[2 * count] = the distinct rows, then the
 * distinct columns (the [2, nnz'] index of coalesce.py:29); value_out[count] = the reduction of every run
 * of equal keys, taken sequentially in run order (psa_segment_reduce's order and bits).  The thread that
 * writes a pair reduces its run: meant for inputs whose runs are short (count * 32 > n); a heavily
 * duplicated input is better served by psa_unique_write + psa_segment_reduce, whose reducer then takes a
 * wave per run.  Other dtypes: PSA_ERR_UNSUPPORTED.  Non-finite values as psa_segment_reduce: NaN
 * propagates through min / max from any position of a run, sum / mean are IEEE. */
int psa_unique_write_reduce(int reduce, int dtype, const int64_t* sorted_keys, int64_t n, int64_t N,
                            const void* workspace, const int64_t* count, int64_t* index_out,
                            const void* payload, void* value_out, psa_stream_t stream);

/* out[s, :] = REDUCE_{i in [ptr[s], ptr[s+1])} src[perm ? perm[i] : i, :]
 * for src rows of D elements of `dtype` (psa_dtype).  Stands in for
 * paddle_scatter.segment_csr at storage.py:471 (with perm = the sort
 * permutation, so value[perm] is never materialised), reduce.py:51 and
 * tensor.py:437.  Semantics = pytorch_scatter segment_csr: empty segment ->
 * 0, mean = sum / count (floor division for integer dtypes), min/max values
 * only.  Sums run in segment order.  n_hint = ptr[nseg] if known (selects the
 * wave-per-segment kernel for long segments), else 0.
 * Non-finite values, whichever kernel runs: min / max give NaN for a segment
 * that holds a NaN in that column, at any position; sum / mean are IEEE (+inf
 * and -inf in one segment give NaN); an empty segment gives 0; the sign of a
 * zero min / max on a +0 / -0 tie is unspecified. */
int psa_segment_reduce(int reduce, int dtype, const void* src,
                       const int64_t* perm, const int64_t* ptr, int64_t nseg,
                       int64_t D, int64_t n_hint, void* out,
                       psa_stream_t stream);

/* out[index[i], :] = REDUCE over i of src[i, :]; src [n, D] of `dtype`
 * (f32/f64/i32/i64), out [dim_size, D].  Stands in for
 * paddle_scatter.scatter at reduce.py:40-42 (reduce over dim 0, index = col).
 * Rows no index points at are 0; mean = sum / count (floor for integers).
 * workspace (psa_scatter_workspace_bytes(dim_size) bytes) is needed for
 * mean/min/max.  Float sums use atomics: order not fixed.
 * Non-finite values: min / max give NaN for a row that receives one (the float
 * min / max atomics drop NaN; a pass of plain stores after them writes it); sum /
 * mean are IEEE; a row nothing points at gives 0 whatever the reduction; the
 * sign of a zero min / max on a +0 / -0 tie is unspecified. */
size_t psa_scatter_workspace_bytes(int64_t dim_size);
int psa_scatter_reduce(int reduce, int dtype, const void* src,
                       const int64_t* index, int64_t n, int64_t D,
                       int64_t dim_size, void* out, void* workspace,
                       size_t workspace_bytes, psa_stream_t stream);

/* ---- spspmm: C = A @ B with both operands sparse (README.md:308-353) -------
 * The reference documents `spspmm(indexA, valueA, indexB, valueB, m, k, n)` but
 * ships no kernel for it.  Here it is expand / sort / compress on the path's
 * own kernels: psa_spspmm_count -> psa_count2ptr (product offsets) ->
 * psa_ptr2ind (owner A entry of every product) -> psa_spspmm_expand ->
 * psa_sort_pairs_u32 | psa_index_sort -> psa_unique_* -> psa_segment_reduce.
 *
 * counts[e] = entries stored in B's row colA[e] (A entries in storage order). */
int psa_spspmm_count(const int64_t* colA, int64_t nnzA, const int64_t* rowptrB,
                     int64_t* counts, psa_stream_t stream);

/* For product p in [0, total): e = owner[p], q = rowptrB[colA[e]] + p -
 * offsets[e]; keys[p] = rowA[e] * n + colB[q]; vals[p] = valA[e] * valB[q]
 * (a NULL value array counts as ones; vals may be NULL).  With n < 0 the key
 * is packed instead: keys[p] = (colB[q] << 32) | rowA[e] — the form used when
 * the walk runs over the CSC views of both operands (outer = entries of B by
 * column, inner = a column of A), so that products come out grouped by output
 * column and ONE stable sort on the row field (psa_sort_pairs_u32_field, half
 * the passes of a sort on row * n + col) finishes the order.  dtype: f32, f64,
 * i32 or i64.  Products of one C entry keep the order in which a sequential
 * row-by-row product meets them, so a stable sort + psa_segment_reduce's
 * in-order kernel (runs averaging < 32 products) reproduces that sum bit for
 * bit. */
int psa_spspmm_expand(int dtype, const int64_t* rowA, const int64_t* colA,
                      const void* valA, const int64_t* rowptrB, const int64_t* colB,
                      const void* valB, const int64_t* offsets, const int64_t* owner,
                      int64_t total, int64_t n, int64_t* keys, void* vals,
                      psa_stream_t stream);

/* ---- sample_adj on the GPU ------------------------------------------------
 * Replaces sample_adj (csrc/sample.cpp:8-24, which throws for GPU tensors;
 * CPU text csrc/cpu/sample_cpu.cpp:9-148).  The op is a chain, because its
 * output sizes are data dependent (two host reads: E and the new-node count):
 *
 *   psa_sample_count  -> psa_count2ptr (out_rowptr; E = out_rowptr[S])
 *   psa_ptr2ind(out_rowptr) -> owner;  psa_sample_select -> e_raw[E]
 *   psa_relabel_mark -> flags;  psa_count2ptr(flags) -> rank; new = rank[E]
 *   psa_relabel_finish -> n_id[S + new], keys[E] = i * n_out + new column id
 *   psa_index_sort(keys) -> out_col = keys % n_out, out_e_id = e_raw[perm]
 *
 * Conventions where the CPU text leaves the order open: picks of one row are
 * taken in draw order (sample_cpu.cpp:108 iterates an unordered_set), and
 * equal new column ids inside a row keep that order (the reference's std::sort
 * at :134-140 is not stable).  num_neighbors < 0 (no sampling) involves
 * neither, apart from multi-edges.
 *
 * Random draws are counter based: draw t of subset row i is a function of
 * (seed, i, t) alone (oracle/sample_oracle.c restates it), in place of the
 * reference's framework-global generator.
 *
 * counts[i] = picks of subset row i: deg if num_neighbors < 0; num_neighbors if
 * replace and deg > 0; min(deg, num_neighbors) otherwise. */
int psa_sample_count(const int64_t* rowptr, const int64_t* idx, int64_t S,
                     int64_t num_neighbors, int replace, int64_t* counts,
                     psa_stream_t stream);

/* e_raw[p] = edge picked by slot p (p = out_rowptr[i] + t, i = owner[p]). */
int psa_sample_select(const int64_t* rowptr, const int64_t* idx, int64_t S,
                      const int64_t* out_rowptr, const int64_t* owner, int64_t E,
                      int64_t num_neighbors, int replace, uint64_t seed,
                      int64_t* e_raw, psa_stream_t stream);

/* newid: int64[num_nodes] scratch (filled by the call).  Afterwards newid[c] =
 * position of c in idx (the last one for duplicates, as the CPU map does) for
 * subset nodes, -2 - (first slot that picked c) for other picked nodes.
 * flags[p] = 1 when slot p is that first pick, else 0 (int64[E]). */
int psa_relabel_mark(const int64_t* idx, int64_t S, const int64_t* col,
                     const int64_t* e_raw, int64_t E, int64_t num_nodes,
                     int64_t* newid, int64_t* flags, psa_stream_t stream);

/* rank = exclusive scan of flags (psa_count2ptr); n_out = S + rank[E].
 * n_id[0:S] = idx, n_id[S + rank[p]] = node first picked at slot p;
 * keys[p] = owner[p] * n_out + (new id of slot p's node). */
int psa_relabel_finish(const int64_t* idx, int64_t S, const int64_t* col,
                       const int64_t* e_raw, int64_t E, const int64_t* newid,
                       const int64_t* rank, const int64_t* owner, int64_t n_out,
                       int64_t* n_id, int64_t* keys, psa_stream_t stream);

/* ---- diagonal ops (torch_sparse/diag.py: remove_diag / set_diag / fill_diag / get_diag)
 * on a SORTED CSR matrix (rowptr int64[M+1], col int64[nnz]).  The k-th diagonal is
 * the cells (r, r + k) inside M x N; k outside (-M, N) has none.  Two calls and ONE
 * host read, as the coalesce chain:
 *   psa_diag_count(...)   new row lengths -> rowcount_out, rowptr_out (psa_count2ptr);
 *                         nnz_out = rowptr_out[M] is the one value the caller reads back
 *   psa_diag_write(...)   col_out int64[nnz_out], value_out [nnz_out, row_bytes]
 * insert = 0: remove_diag (every stored (r, r + k) entry goes, duplicates included);
 * insert = 1: set_diag (the same, then one entry per diagonal cell at its sorted place,
 * value row diag_values[r - max(-k, 0)]).  Kept entries keep their order and bytes.
 * colcount (int64[N] or NULL): the input's column counts; colcount_out then gets them
 * adjusted for the removed / inserted entries.  workspace: psa_diag_workspace_bytes(M)
 * bytes, 16-byte aligned; psa_diag_write reads what psa_diag_count left there.
 * Deterministic, no atomics; the write pass is balanced by output entries. */
size_t psa_diag_workspace_bytes(int64_t M);
int psa_diag_count(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, int64_t k, int insert,
                   const int64_t* colcount, int64_t* rowcount_out, int64_t* rowptr_out, int64_t* colcount_out,
                   void* workspace, size_t workspace_bytes, psa_stream_t stream);
/* value: [nnz, row_bytes] of any dtype; value_out NULL (or row_bytes 0) for a value-less
 * matrix.  value may be NULL when nnz is 0, diag_values when num_diag is 0.
 * Gradient maps, each optional (NULL): out_pos int64[nnz] = output slot of every input
 * entry, -1 for a removed one; diag_pos int64[num_diag] = output slot of every inserted
 * entry.  The backward of the value path is psa_diag_gather through them. */
int psa_diag_write(const int64_t* rowptr, const int64_t* col, const void* value, int64_t row_bytes,
                   const void* diag_values, int64_t M, int64_t N, int64_t k, int insert, int64_t nnz,
                   const int64_t* rowptr_out, int64_t nnz_out, const void* workspace, int64_t* col_out,
                   void* value_out, int64_t* out_pos, int64_t* diag_pos, psa_stream_t stream);

/* get_diag: out [min(M, N), row_bytes] = the value row of the LAST stored (r, r) entry of
 * row r (storage order), zero bytes where there is none.  value NULL: out is
 * f32[min(M, N)] of 1.0 / 0.0 (so a valued matrix passes a non-NULL value: nnz > 0).  pos_out (int64[min(M, N)] or NULL): that entry's
 * position, -1 for none (the backward: psa_diag_scatter into zeros). */
int psa_get_diag(const int64_t* rowptr, const int64_t* col, const void* value, int64_t row_bytes, int64_t M,
                 int64_t N, void* out, int64_t* pos_out, psa_stream_t stream);

/* out[i, :] = map[i] >= 0 ? src[map[i], :] : 0, rows of row_bytes bytes. */
int psa_diag_gather(const void* src, const int64_t* map, int64_t n, int64_t row_bytes, void* out,
                    psa_stream_t stream);
/* out[pos[i], :] = src[i, :] for every pos[i] >= 0 (distinct); other rows of out untouched. */
int psa_diag_scatter(const void* src, const int64_t* pos, int64_t n, int64_t row_bytes, void* out,
                     psa_stream_t stream);

/* ---- GraphSAINT random-walk sampler (torch_sparse rw.py / saint.py) on a SQUARE N x N
 * sorted CSR matrix (rowptr int64[N+1], col int64[nnz]).
 *
 * random_walk: out int64[S, walk_length + 1], row n = the walk from start[n] (int64[S]):
 * out[n, 0] = start[n]; at step l (0-based) from node c with d = rowptr[c+1] - rowptr[c]
 * entries, the next node is col[rowptr[c] + randint(seed, n, l, d)] when d > 0 and c
 * itself when d == 0 (a walk stays at a node without entries).  randint is the draw of
 * psa_sample_select (stream n, draw l), so step 0 of walk n picks the edge
 * psa_sample_select picks for subset row n with num_neighbors = 1, replace = 1.  Duplicate
 * entries are separate choices.  flags: int64[1], zeroed by the caller; bit 0 is set when a
 * start lies outside [0, N) (that walk's row is then left unwritten).  One launch, no
 * atomics on the output; deterministic. */
int psa_random_walk(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* start, int64_t S,
                    int64_t walk_length, uint64_t seed, int64_t* out, int64_t* flags, psa_stream_t stream);
/* Test/bench hook: the store scheme of psa_random_walk for this process (0 = default =
 * 2; 1 = one 8-byte store per step, 2 = bursts of 16 steps held in registers, 3 / 4 =
 * 1 / 2 with two walks per lane).  Returns the previous value.  All produce the same bits. */
int psa_random_walk_set_variant(int variant);

/* ---- edge-weighted sampling: the row CDF, the weighted walk, weighted sample_adj picks.
 *
 * row CDF of a CSR matrix with N rows: for every row [s, t) = [rowptr[r], rowptr[r+1]),
 * cum[s] = w[s] and cum[e] = fl(cum[e-1] + w[e]) in float64, STRICTLY left to right and
 * afresh in each row: cum equals numpy's cumsum of the row bit for bit, is non-decreasing
 * for weights >= 0, and cum[e] == cum[e-1] exactly where w[e] == 0.  w, cum: double[nnz]
 * (distinct buffers).  flags: int64[1], zeroed by the caller; bit 0 = a weight < 0 (-0.0
 * counts as 0), bit 1 = a NaN or infinite weight, bit 2 = the total of a row of finite
 * weights overflowed to infinity.  cum is only meaningful when flags stays 0.  One launch,
 * no workspace, no atomics on floats; capturable. */
int psa_row_cdf(const int64_t* rowptr, const double* w, int64_t N, double* cum, int64_t* flags,
                psa_stream_t stream);

/* The weighted pick, on the host (the kernels run the same text, csrc/weighted_pick.h).
 * cum[0 .. deg) is one row of the row CDF, r the random word of a draw: mix64(stream + t),
 * the word the uniform draw turns into an index.  total = cum[deg-1]; u = (r >> 11) * 2^-53;
 * target = u * total, one rounded multiply; the pick is the smallest e with cum[e] > target,
 * or, when there is none (a subnormal total whose product rounded up to it), the smallest
 * e with cum[e] == total.  Either way the picked entry has a positive weight.  Returns the
 * index in [0, deg), or -1 for no pick: deg <= 0, a NULL cum, or a total that is not
 * positive. */
int64_t psa_weighted_pick_host(const double* cum, int64_t deg, uint64_t r);

/* Successive weighted picks WITHOUT replacement from one row of the row CDF, on the host
 * (the kernels of psa_neighbor_hop_pick_weighted run the same text, csrc/weighted_pick.h).
 * The positions taken so far, ascending, cut the row into gaps; the mass of a gap is the
 * difference of cum at its two ends (0.0 below the row's first entry), exactly 0 when it
 * holds no entry of positive weight.  Draw t: T = the masses summed left to right; the
 * draws end when T is not positive; the gap is the first whose running sum exceeds
 * u1 * T, u1 = (words_gap[t] >> 11) * 2^-53 (no word at draw 0: there is one gap; when
 * the product rounded up to T, the last gap of positive mass); the entry is the smallest e
 * in the gap with cum[e] > base + u * mass, u from words_entry[t], base = cum just below
 * the gap (one rounded multiply, one rounded add; when there is none, the smallest e with
 * cum[e] equal to the gap's last cum).  Draw 0 is psa_weighted_pick_host(cum, deg,
 * words_entry[0]).  The kernels use words_entry[t] = mix64(stream + t) and words_gap[t] =
 * mix64(stream + k + t).  out: int64[k], the picks in draw order as indices in [0, deg),
 * -1 past the last pick.  Returns the number of picks = min(k, entries of positive
 * weight), all distinct; 0 for a NULL pointer, deg <= 0 or k <= 0.  Row totals so large
 * that the sum of the gap masses overflows are not supported. */
int64_t psa_weighted_pick_without_host(const double* cum, int64_t deg, int64_t k, const uint64_t* words_entry,
                                       const uint64_t* words_gap, int64_t* out);

/* The walk of the random-walk sampler above with the step's entry chosen by the weighted
 * pick: at step l, walk n at node c with d > 0 entries takes entry e = rowptr[c] + pick of
 * (cum + rowptr[c], d, mix64(stream n + l)) and moves to col[e]; it stays at c when d == 0
 * or the row's total is zero.  cum: the row CDF of the matrix's weights, or NULL for the
 * uniform draw, and then out equals the plain random walk's bit for bit.  edge_out:
 * int64[S, walk_length] or NULL; edge_out[n, l] = e, the storage position of the entry
 * taken, or -1 where the walk stayed.  flags as for the plain walk.  One launch. */
int psa_random_walk_weighted(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                             const int64_t* start, int64_t S, int64_t walk_length, uint64_t seed, int64_t* out,
                             int64_t* edge_out, int64_t* flags, psa_stream_t stream);

/* ---- node2vec (p, q) walks: the second-order bias on the walks above, uniform (cum NULL)
 * or weighted (cum = the row CDF).
 *
 * Walk n (stream = rand_stream(seed, n)) at node v at step l, having arrived from t, stays
 * (node v, edge id -1) when row v is empty or, weighted, its total is not positive.  Else it
 * makes tries j = 0 .. max_tries - 1: c = stream + l + (j << 32) mod 2^64; the proposal is
 * the entry e the plain step takes for the word mix64(c) (rowptr[v] + high half of
 * word * deg, or the weighted pick), x = col[e].  At l == 0 the first proposal is taken.  At
 * l > 0 its class is 0 if x == t, else 1 if row t stores a column equal to x (lower-bound
 * binary search in the sorted row, at most 64 halvings), else 2, and it is accepted when
 * (mix64(c + 2^63) >> 11) < thr<class>.  When no try is accepted the last proposal is
 * taken.  Then t = v, v = x.  thr0/1/2 <= 2^53 (2^53: always accept; 0: never); the caller
 * makes them from 1/p, 1, 1/q.  With all three at 2^53 the walks are those of
 * psa_random_walk_weighted bit for bit.  out, edge_out, flags as there.  One launch, no
 * workspace, every loop bounded; capturable.  PSA_ERR_INVALID_ARG for a NULL rowptr, start,
 * out or flags (S > 0), a negative size, max_tries outside [1, 32768] or a threshold
 * above 2^53. */
int psa_node2vec_walk(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N, const int64_t* start,
                      int64_t S, int64_t walk_length, uint64_t seed, uint64_t thr0, uint64_t thr1, uint64_t thr2,
                      int max_tries, int64_t* out, int64_t* edge_out, int64_t* flags, psa_stream_t stream);
/* The same walks run serially on HOST arrays by the same step (csrc/node2vec_step.h): the
 * step can be checked without a GPU. */
int psa_node2vec_walk_host(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                           const int64_t* start, int64_t S, int64_t walk_length, uint64_t seed, uint64_t thr0,
                           uint64_t thr1, uint64_t thr2, int max_tries, int64_t* out, int64_t* edge_out,
                           int64_t* flags);

/* ---- edge lookup and exact negative sampling on a CSR matrix of M rows and N columns sorted
 * by (row, col); duplicated entries allowed (csrc/negative.hip, csrc/edge_lookup.h).
 *
 * psa_edge_lookup: pos_out[q] = the storage position of the FIRST entry (row_q[q], col_q[q]):
 * a lower-bound binary search for col_q[q] in col[rowptr[r] .. rowptr[r + 1]), at most 64
 * halvings; -1 when the entry is not stored; -1 with flags bit 0 (value 1) when the pair lies
 * outside M x N (nothing is read through it).  One launch, one lane per query, no workspace;
 * flags (int64[1], zeroed by the caller) is only ever OR-ed into; every pos_out[q] is written.
 *
 * psa_negative_sample draws S * k samples.  Sample i: stream = rand_stream(seed, i) =
 * mix64(seed ^ mix64(i)), mix64 the finaliser of splitmix64 (csrc/rng.h).  Try j = 0 ..
 * max_tries - 1 uses c = stream + j mod 2^64.  The column proposal is cc = high half of the
 * 128-bit product mix64(c) * N.  With src == NULL (global mode) the row proposal is r = high
 * half of mix64(c + 2^63) * M; with src (int64[S], structured mode) r = src[i / k].  The try
 * is accepted iff !(no_self_loops && r == cc) and the search above does not find cc in row r.
 * The first accepted try is the result: col_out[i] = cc and, in global mode, row_out[i] = r
 * (row_out is not touched in structured mode and may be NULL).  When no try is accepted the
 * result is -1 (both outputs) and flags bit 1 (value 2) is raised; with M == 0 or N == 0
 * every sample fails that way and nothing of the matrix is read.  A given row outside [0, M):
 * -1 with flags bit 0, nothing read through it.  Draws are with replacement across samples.
 * One launch, one lane per sample, no workspace, every loop bounded; capturable.
 *
 * PSA_ERR_INVALID_ARG: a negative size, k < 1, max_tries outside [1, 32768], S * k
 * overflowing, no_self_loops with M != N, or (with a non-zero count) a NULL rowptr, query,
 * output or flags pointer.  A zero count returns PSA_OK and touches nothing.
 *
 * The _host forms run the same steps serially on HOST arrays: every result can be checked
 * without a GPU. */
int psa_edge_lookup(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* row_q,
                    const int64_t* col_q, int64_t Q, int64_t* pos_out, int64_t* flags, psa_stream_t stream);
int psa_edge_lookup_host(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* row_q,
                         const int64_t* col_q, int64_t Q, int64_t* pos_out, int64_t* flags);
int psa_negative_sample(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* src, int64_t S,
                        int64_t k, int no_self_loops, int max_tries, uint64_t seed, int64_t* row_out, int64_t* col_out,
                        int64_t* flags, psa_stream_t stream);
int psa_negative_sample_host(const int64_t* rowptr, const int64_t* col, int64_t M, int64_t N, const int64_t* src,
                             int64_t S, int64_t k, int no_self_loops, int max_tries, uint64_t seed, int64_t* row_out,
                             int64_t* col_out, int64_t* flags);

/* ---- weakly connected components of an N x N matrix: a lock-free union-find over the stored
 * entries (csrc/components.hip, csrc/union_find.h).  Every stored entry (u, v) joins u and v,
 * whatever its direction or value; self loops and duplicates change nothing; the entries need
 * no order beyond row[] being the expansion of rowptr[].  Three launches on one stream:
 *
 *   psa_components_init     parent[v] = c when row v is not empty and its first stored column
 *                           c = col[rowptr[v]] satisfies 0 <= c < v, else v.  A rowptr[v]
 *                           outside [0, nnz) reads nothing and gives v.
 *   psa_components_hook     one lane per entry e: joins row[e] and col[e] in parent (int64[N]
 *                           as init left it): the larger of the two roots becomes, by one
 *                           64-bit compare-and-swap, a child of the smaller; a lost race goes
 *                           on from the value the swap returned.  An entry with an end outside
 *                           [0, N) joins nothing and raises flags bit 0 (value 1); flags
 *                           (int64[1], zeroed by the caller) is only ever OR-ed into.
 *   psa_components_flatten  root[v] = the root of v's tree, which after hook is the smallest
 *                           node of v's component under any schedule; is_root[v] = (root[v] ==
 *                           v) as 0 / 1.  parent is compressed along the way.
 *
 * The caller ranks the roots: with rank = the exclusive prefix sum of is_root (psa_count2ptr),
 * rank[N] is the number of components and rank[root[v]] the label of v, the number of
 * components whose smallest node is below that of v's.  parent, root and is_root are int64[N];
 * every element is written on every path.  No workspace, no lane waits on another, every loop
 * is bounded (union_find.h gives the bounds); each grid covers its count, 256 lanes per
 * workgroup.  The result is deterministic although the order of the links is not.
 *
 * PSA_ERR_INVALID_ARG: a negative size, more than 2^31 - 1 workgroups, or (with a non-zero
 * count: N for init and flatten, nnz for hook) a NULL pointer among those the call uses; col
 * may be NULL for init when nnz == 0.  A zero count returns PSA_OK and touches nothing.
 *
 * psa_components_host runs init, hook and flatten serially on HOST arrays by the same steps:
 * the result can be checked without a GPU. */
int psa_components_init(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t* parent,
                        psa_stream_t stream);
int psa_components_hook(const int64_t* row, const int64_t* col, int64_t nnz, int64_t N, int64_t* parent, int64_t* flags,
                        psa_stream_t stream);
int psa_components_flatten(int64_t* parent, int64_t N, int64_t* root, int64_t* is_root, psa_stream_t stream);
int psa_components_host(const int64_t* rowptr, const int64_t* row, const int64_t* col, int64_t N, int64_t nnz,
                        int64_t* parent, int64_t* root, int64_t* is_root, int64_t* flags);

/* The count and select steps of the sample_adj chain for weighted picks; every other step
 * of the chain is shared.  counts[i] = deg for num_neighbors < 0; with replace,
 * num_neighbors when the row's total is > 0 and 0 otherwise.  Slot t of subset row i takes
 * entry rowptr[idx[i]] + pick of stream i, draw t (entry rowptr[idx[i]] + t for
 * num_neighbors < 0).  Weighted picks WITHOUT replacement (num_neighbors >= 0 and replace
 * == 0) are refused with PSA_ERR_INVALID_ARG: successive weighted draws need a per-row
 * removal structure that these entry points do not have. */
int psa_sample_count_weighted(const int64_t* rowptr, const double* cum, const int64_t* idx, int64_t S,
                              int64_t num_neighbors, int replace, int64_t* counts, psa_stream_t stream);
int psa_sample_select_weighted(const int64_t* rowptr, const double* cum, const int64_t* idx, int64_t S,
                               const int64_t* out_rowptr, const int64_t* owner, int64_t E, int64_t num_neighbors,
                               int replace, uint64_t seed, int64_t* e_raw, psa_stream_t stream);

/* saint_subgraph: the subgraph induced by node_idx (int64[S], any order, duplicates
 * allowed).  assoc[node_idx[i]] = i (the last duplicate wins); for every i in order and
 * every entry e of row node_idx[i] with assoc[col[e]] >= 0, the candidate order emits
 * (row' = i, col' = assoc[col[e]], edge = e).  Two calls and ONE host read:
 *   psa_saint_count(...)   info int64[2] = {nnz', flags} on the device: the host read
 *   psa_saint_write(...)   row_out, col_out, edge_out int64[nnz'] in candidate order,
 *                          rowptr_out int64[S+1]
 * flags: bit 0 = a node_idx entry outside [0, N) (the output is then meaningless), bit 1 =
 * node_idx has duplicates, bit 2 = node_idx decreases somewhere.  Without bit 2 the
 * candidate order is sorted by (row', col'); with it the caller re-sorts (stable) by
 * (row', col').  workspace: psa_saint_workspace_bytes(S, N) bytes, 16-byte aligned, kept
 * between the two calls.  Deterministic; hub rows are split across workgroups. */
size_t psa_saint_workspace_bytes(int64_t S, int64_t N);
int psa_saint_count(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* node_idx, int64_t S,
                    void* workspace, size_t workspace_bytes, int64_t* info, psa_stream_t stream);
int psa_saint_write(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* node_idx, int64_t S,
                    const void* workspace, int64_t nnz_out, int64_t* rowptr_out, int64_t* row_out,
                    int64_t* col_out, int64_t* edge_out, psa_stream_t stream);

/* ---- reverse_cuthill_mckee (torch_sparse bandwidth.py) on the pattern of a SQUARE N x N
 * CSR matrix with sorted rows (rowptr int64[N+1], col int64[nnz]); values are never read.
 *
 * deg[i] = rowptr[i+1] - rowptr[i] (stored duplicates and a stored diagonal count).  The
 * Cuthill-McKee order is built one component at a time: the seed of the next component is
 * the unvisited node with the smallest (deg, id); from the seed, nodes are taken in order
 * and each appends its not-yet-visited neighbours sorted by (deg, id), once.  The kernels
 * build it level by level: the nodes found by one breadth-first level are ordered by
 * (position of their earliest-placed parent, deg, id), which is the same order.  perm is
 * that order reversed.  On a non-symmetric pattern the rules run over the stored entries.
 *
 * The level loop belongs to the caller (paddle_sparse_amd/ops.py::reverse_cuthill_mckee):
 *   psa_csr_row_stats            -> n_empty (rows without entries), max_deg   [host read]
 *   psa_rcm_init(...)            degrees, seeds = stable psa_index_sort of deg = (deg, id)
 *                                order, the n_empty degree-0 nodes at positions 0..n_empty-1
 *   repeat
 *     psa_rcm_small(...)         ONE workgroup runs level after level, starting the next
 *                                component from seeds whenever a level comes back empty,
 *                                until all N nodes are placed (status PSA_RCM_DONE) or a
 *                                level has more than psa_rcm_small_capacity() candidate
 *                                edges (or more than 2048 frontier nodes): that level is
 *                                left untouched, status PSA_RCM_HANDOVER    [host read of state]
 *     while the level [level_lo, level_hi) with `cand` candidate edges is too large:
 *       psa_rcm_level_count(...) frontier degrees -> psa_count2ptr; tiles of psa_rcm_tile()
 *                                candidates (a long row spans several workgroups) claim
 *                                every unseen child for the smallest parent position
 *                                (atomicMin: order-independent) and count the candidates
 *                                whose parent won and that are the first of their
 *                                duplicates -> state[NEW], state[NEXT_CAND] [host read of state]
 *       psa_rcm_level_write(...) keys parent_local * (max_deg + 1) + deg and the child ids
 *                                in candidate order ((parent, id) order), a stable
 *                                psa_sort_pairs_u32, then order / rank; the level becomes
 *                                [level_hi, level_hi + n_new) with state[NEXT_CAND] candidates
 *   psa_rcm_finish(...)          perm_out int64[N] = the order reversed
 * Which path served a level does not change a bit of the result.  No launch waits for
 * another workgroup (the radix sort's own look-back aside; its fault word is folded into
 * state[FAULT]); every loop is bounded by N or nnz.
 *
 * state: int64[PSA_RCM_STATE_WORDS] on the device, written by psa_rcm_init, =
 *   { placed, level_lo, level_hi, next_seed, status, cand (candidate edges of the level),
 *     NEW (nodes the counted level adds), NEXT_CAND (their candidate edges), FAULT (a radix
 *     pass gave up: the result is invalid), levels served by psa_rcm_small so far, ... }.
 * workspace: psa_rcm_workspace_bytes(N, nnz) bytes (0 when N is outside [1, 2^31)), 16-byte
 * aligned, kept from psa_rcm_init to psa_rcm_finish; it includes the scan and sort scratch.
 * n_empty and max_deg are words 0 and 3 of psa_csr_row_stats.  1 <= N < 2^31. */
#define PSA_RCM_STATE_WORDS 16
#define PSA_RCM_DONE 0
#define PSA_RCM_HANDOVER 1
#define PSA_RCM_BAD_INPUT 2 /* more nodes found than exist: the rows are not sorted */
size_t psa_rcm_workspace_bytes(int64_t N, int64_t nnz);
int psa_rcm_init(const int64_t* rowptr, int64_t N, int64_t nnz, int64_t n_empty, int64_t max_deg, void* workspace,
                 size_t workspace_bytes, int64_t* state, psa_stream_t stream);
int psa_rcm_small(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t max_deg,
                  void* workspace, size_t workspace_bytes, int64_t* state, psa_stream_t stream);
/* level_lo, level_hi, cand: the values of the last host read of state (1 <= cand <= nnz). */
int psa_rcm_level_count(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t level_lo,
                        int64_t level_hi, int64_t cand, void* workspace, size_t workspace_bytes, int64_t* state,
                        psa_stream_t stream);
/* n_new: state[NEW] as read after psa_rcm_level_count of the same level (0 allowed: the
 * level found nothing, the component is complete and psa_rcm_small starts the next). */
int psa_rcm_level_write(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t level_lo,
                        int64_t level_hi, int64_t cand, int64_t n_new, int64_t max_deg, void* workspace,
                        size_t workspace_bytes, int64_t* state, psa_stream_t stream);
int psa_rcm_finish(int64_t N, int64_t nnz, const void* workspace, size_t workspace_bytes, int64_t* perm_out,
                   psa_stream_t stream);
/* Candidate edges of a level that psa_rcm_small takes under the current variant (4096 by
 * default), and the candidates per workgroup of the large path (1024). */
int64_t psa_rcm_small_capacity(void);
int64_t psa_rcm_tile(void);
/* Test/bench hook: 0 = default, 1 = every level through the large path (capacity 0: the
 * small launch only starts components), 2 = the small path with a capacity of 8 candidate
 * edges, so that both paths and the hand-over in each direction happen at tiny sizes.
 * Returns the previous value.  All produce the same bits. */
int psa_rcm_set_variant(int variant);

/* ---- neighbor_sample (torch_sparse neighbor_sample, CPU only upstream): multi-hop,
 * layer-wise neighbour sampling of a SQUARE N x N CSR matrix with sorted rows, with one
 * relabel map for the whole call.
 *
 * n_id starts as the seeds (distinct, inside [0, N)); local id = position in n_id.  Hop l
 * expands the frontier, the nodes appended during hop l - 1 (hop 1: the seeds), local ids
 * [begin, end); every node is expanded at most once per call.  A frontier node at local id
 * i with deg stored entries makes the picks of psa_sample_count / psa_sample_select for
 * (deg, num_neighbors, replace).  Random-stream contract: draw t of the node at LOCAL ID i
 * is randint(seed, i, t, .) of psa_sample_select (stream i, draw t; Floyd's walk draws
 * randint(seed, i, t, deg - k + t)), whatever the hop: local ids are unique across hops, so
 * one seed serves all of them, and hop 1 makes the picks of sample_adj(seeds, k, replace,
 * seed).  Slot order within a hop is (frontier position, t).  A picked column without a
 * local id gets the next one in order of its first slot and is appended to n_id; one that
 * has a local id (a seed, a node of an earlier or of the same hop) keeps it.  Every slot
 * emits (row' = i, col' = local id of the column, e = position in the matrix's storage).
 *
 * The hop loop belongs to the caller (paddle_sparse_amd/ops.py::neighbor_sample):
 *   psa_neighbor_init(...)        fill the map when `fresh`; place and check the seeds
 *   per hop with num_neighbors != 0 and a non-empty frontier:
 *     num_neighbors < 0 only: psa_neighbor_hop_count -> psa_count2ptr -> frontier_ptr,
 *                                 slots = frontier_ptr[F]                  [host read]
 *     num_neighbors >= 0:         slots = F * num_neighbors, the bound the grid covers
 *     psa_neighbor_hop_pick(...)  picks, one atomicMax claim per slot (the smallest slot
 *                                 wins whatever the arrival order), one scan;
 *                                 state = {E_l, new_l, flags}              [host read]
 *     psa_neighbor_hop_write(...) n_id_new int64[new_l] (the next frontier, local ids
 *                                 [end, end + new_l)), row_out / col_out / edge_out
 *                                 int64[E_l] in slot order, the map finalised
 *   psa_neighbor_reset(...)       map[n_id[j]] = unseen: the workspace is clean again
 *   the caller sorts (stable) by row' * n + col' with psa_index_sort and builds rowptr'
 *   with psa_ind2ptr.
 * state: int64[PSA_NEIGHBOR_STATE_WORDS] on the device, zeroed by psa_neighbor_init;
 * state[2] collects PSA_NEIGHBOR_DUP_SEED, PSA_NEIGHBOR_SEED_OUTSIDE (such a seed is
 * skipped and has no entries) and PSA_NEIGHBOR_COL_OUTSIDE (a stored column outside
 * [0, N): its slot is dropped); with a flag up the call must end with psa_neighbor_reset
 * over the seeds, the nodes appended so far AND the slots of the hop just picked (its
 * claims are in the map).
 * workspace: psa_neighbor_workspace_bytes(N) bytes, 16-byte aligned: the map int32[N].  It
 * may be kept between calls: after psa_neighbor_reset it is clean and the next
 * psa_neighbor_init takes fresh = 0, so nothing sized N runs per call.
 * hop_workspace: psa_neighbor_hop_workspace_bytes(slots) bytes, 16-byte aligned, kept
 * from psa_neighbor_hop_pick to psa_neighbor_hop_write (or the reset of an abandoned hop).
 * N, the node count and slots stay below 2^31 (the size functions return 0 otherwise).
 * Deterministic; no launch waits for another workgroup; not capturable in a graph. */
#define PSA_NEIGHBOR_STATE_WORDS 8
#define PSA_NEIGHBOR_DUP_SEED 1
#define PSA_NEIGHBOR_SEED_OUTSIDE 2
#define PSA_NEIGHBOR_COL_OUTSIDE 4
size_t psa_neighbor_workspace_bytes(int64_t N);
size_t psa_neighbor_hop_workspace_bytes(int64_t slots);
int psa_neighbor_init(const int64_t* seeds, int64_t S, int64_t N, int fresh, void* workspace, size_t workspace_bytes,
                      int64_t* state, psa_stream_t stream);
/* counts[f] = stored entries of frontier node f (0 for a node outside the matrix). */
int psa_neighbor_hop_count(const int64_t* rowptr, int64_t N, const int64_t* frontier, int64_t F, int64_t* counts,
                           psa_stream_t stream);
/* frontier: int64[F], the nodes at local ids [begin, begin + F); frontier_ptr: int64[F+1],
 * read when num_neighbors < 0 only (NULL otherwise); num_neighbors != 0, F >= 1, slots >= 1. */
int psa_neighbor_hop_pick(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* frontier, int64_t F,
                          const int64_t* frontier_ptr, int64_t begin, int64_t num_neighbors, int replace,
                          uint64_t seed, int64_t slots, void* workspace, void* hop_workspace,
                          size_t hop_workspace_bytes, int64_t* state, psa_stream_t stream);
/* psa_neighbor_hop_pick for a hop with num_neighbors >= 1 whose picks are weighted: cum is
 * the row CDF of the matrix's weights (psa_row_cdf, double[nnz]).  replace = 1: slot t of
 * the node at local id i takes the entry psa_weighted_pick_host finds with the word
 * mix64(stream i + t), as weighted sample_adj and the weighted walk do; replace = 0: the
 * node's picks are those of psa_weighted_pick_without_host with the words of stream i,
 * slot f * num_neighbors + t holding draw t.  A row makes min(num_neighbors, entries of
 * positive weight) picks without replacement and none at all when its total is zero; the
 * remaining slots stay empty.  Same workspaces, state and follow-up
 * (psa_neighbor_hop_write with the same num_neighbors) as psa_neighbor_hop_pick;
 * frontier_ptr is not read.  num_neighbors < 0 takes every entry whatever its weight: that
 * hop goes through psa_neighbor_hop_pick.  Cost without replacement: one thread per
 * frontier node, O(num_neighbors^2) gap work and num_neighbors binary searches per node. */
int psa_neighbor_hop_pick_weighted(const int64_t* rowptr, const int64_t* col, const double* cum, int64_t N,
                                   const int64_t* frontier, int64_t F, const int64_t* frontier_ptr, int64_t begin,
                                   int64_t num_neighbors, int replace, uint64_t seed, int64_t slots, void* workspace,
                                   void* hop_workspace, size_t hop_workspace_bytes, int64_t* state,
                                   psa_stream_t stream);
/* n_edges, n_new: state[0], state[1] as read after psa_neighbor_hop_pick of the same hop.
 * row_out, col_out and edge_out may be NULL together: only n_id_new and the map are then
 * written (a caller that wants the node set alone). */
int psa_neighbor_hop_write(const int64_t* col, int64_t begin, int64_t end, int64_t num_neighbors, int64_t slots,
                           int64_t n_edges, int64_t n_new, void* workspace, const void* hop_workspace,
                           int64_t* n_id_new, int64_t* row_out, int64_t* col_out, int64_t* edge_out,
                           psa_stream_t stream);
/* ids: int64[n] nodes whose map entries are cleared (entries outside [0, N) are skipped);
 * slots > 0: also the columns claimed by the slots of the hop held in hop_workspace. */
int psa_neighbor_reset(const int64_t* ids, int64_t n, int64_t N, const int64_t* col, const void* hop_workspace,
                       int64_t slots, void* workspace, psa_stream_t stream);

/* ---- segmented softmax of stored values (the attention path: softmax over the entries of
 * every row or column of a sparse matrix), fp32.  src, out: [n, D] row-major (D = 1 for
 * scalar values), any 4-byte alignment; indptr int64[nseg + 1] with indptr[nseg] <= n.
 * For every segment s and column h < D
 *   out[j, h] = exp(src[j, h] - m[s, h]) / sum_{j' in s} exp(src[j', h] - m[s, h]),
 * m = the segment's maximum.  perm (int64[n] or NULL): the entry at position j of the
 * segment order is src[perm[j]] and its result goes to out[perm[j]] (softmax over the
 * columns of a CSR matrix: indptr = colptr, perm = csr2csc, nothing is transposed).
 * Non-finite values as torch.softmax on the dense row: a group with a NaN, a +inf or
 * nothing but -inf is NaN throughout; -inf among finite entries gives exactly 0.  An
 * empty segment writes nothing.
 * Backward, from the saved output y and the upstream gradient grad (same layout and perm
 * rule; src is not read):
 *   grad_src[j, h] = y[j, h] * (grad[j, h] - sum_{j' in s} y[j', h] * grad[j', h]).
 * One group of 8..64 lanes per segment; segments above 128 entries run as 128-entry
 * chunks whose partials are folded in chunk order.  No float atomics, no host read:
 * bitwise reproducible and capturable.  workspace: psa_segment_softmax_workspace_bytes(n, D)
 * bytes, 16-byte aligned (0 bytes, NULL allowed, when n <= 128). */
size_t psa_segment_softmax_workspace_bytes(int64_t n, int64_t D);
int psa_segment_softmax(const float* src, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t D,
                        int64_t n, float* out, void* workspace, size_t workspace_bytes, psa_stream_t stream);
int psa_segment_softmax_bw(const float* y, const float* grad, const int64_t* perm, const int64_t* indptr, int64_t nseg,
                           int64_t D, int64_t n, float* grad_src, void* workspace, size_t workspace_bytes,
                           psa_stream_t stream);

/* ---- multi-head attention ends: SpMM over per-head values and sddmm per head, fp32.
 * (rowptr int64[M + 1], col int64[nnz]) is a CSR pattern with col[e] in [0, N); all dense
 * arrays are row-major and contiguous.
 *   psa_spmm_heads   value [nnz, H], mat [N, H, F]:
 *                    out[r, h, f] = sum_{e in row r} value[e, h] * mat[col[e], h, f], out [M, H, F].
 *                    out is fully written; a row without entries is 0.  A stored 0 is not
 *                    skipped (0 * inf = NaN).
 *   psa_sddmm_heads  x [M, H, K], y [N, H, K]: out[e, h] = <x[row(e), h, :], y[col[e], h, :]>,
 *                    out [nnz, H].  Also the gradient of psa_spmm_heads wrt value (x = grad_out,
 *                    y = mat, K = F); the gradients wrt the dense operands are psa_spmm_heads
 *                    over the CSR and the CSC view.
 * One wave per row; rows above 128 entries run as 128-entry chunks (psa_spmm_heads adds the
 * chunks' partial rows in chunk order).  16-byte gathers when F (K) % 4 == 0 and mat and out
 * (x and y) are 16-byte aligned, 4-byte loads otherwise: any 4-byte alignment is accepted.
 * Every address is formed in 64-bit arithmetic (no bound on N * H * F * 4).  No float atomics,
 * no host read: bitwise reproducible and capturable.  workspace: the matching
 * _workspace_bytes(...) bytes, 16-byte aligned (0 bytes, NULL allowed, when nnz <= 128). */
size_t psa_spmm_heads_workspace_bytes(int64_t nnz, int64_t H, int64_t F);
int psa_spmm_heads(const int64_t* rowptr, const int64_t* col, const float* value, const float* mat, int64_t M,
                   int64_t N, int64_t H, int64_t F, int64_t nnz, float* out, void* workspace,
                   size_t workspace_bytes, psa_stream_t stream);
size_t psa_sddmm_heads_workspace_bytes(int64_t nnz);
int psa_sddmm_heads(const int64_t* rowptr, const int64_t* col, const float* x, const float* y, int64_t M, int64_t H,
                    int64_t K, int64_t nnz, float* out, void* workspace, size_t workspace_bytes,
                    psa_stream_t stream);

/* ---- fused sparse attention: sddmm + row softmax + SpMM in one pass per row, fp32.  Pattern and
 * layouts as above: q [M, H, K], k [N, H, K], v [N, H, F]; bias NULL, or [nnz] (bias_heads = 1,
 * shared by the heads) or [nnz, H] (bias_heads = H); H, K, F >= 1.
 *   s[e, h]      = scale * <q[row(e), h, :], k[col[e], h, :]> (+ bias)
 *   p[e, h]      = exp(s[e, h] - m[r, h]) / l[r, h],  m = the row's maximum of s[., h],
 *                  l = sum over the row of exp(s - m)
 *   out[r, h, :] = sum_{e in row r} p[e, h] * v[col[e], h, :]
 *   psa_attention_fw          writes out [M, H, F] and stat [M, H, 2] = {m, l} (the pair, not m + log l),
 *                             both fully; nothing per entry is written.  A row without entries gives
 *                             out = 0 and stat = {-inf, 0}.
 *   psa_attention_bw_entries  the per-entry half of the backward: with delta[r, h] =
 *                             <grad_out[r, h, :], out[r, h, :]> and dP[e, h] = <grad_out[row(e), h, :],
 *                             v[col[e], h, :]> it recomputes s and writes p [nnz, H] and
 *                             ds [nnz, H] = p * (dP - delta); a row without entries writes nothing.
 *                             The gradients are psa_spmm_heads calls: grad_q = scale * (ds, k) over
 *                             the CSR view, grad_k = scale * (ds, q) and grad_v = (p, grad_out) over the
 *                             CSC view, grad_bias = ds (summed over the heads for bias_heads = 1).
 * Non-finite values as psa_segment_softmax and psa_spmm_heads: a row and head whose scores hold a NaN,
 * a +inf or nothing but -inf is NaN in out[r, h, :]; -inf among finite scores has weight exactly 0; no
 * zero skipping (0 * inf = NaN).
 * One wave per row with a running {m, l} per head (online softmax); rows above 128 entries run as
 * 128-entry chunks whose {m, l, partial row} are merged in chunk order.  16-byte gathers when
 * K % 4 == 0, F % 4 == 0 and q, k, v, out (and grad_out) are 16-byte aligned, 4-byte loads otherwise:
 * any 4-byte alignment is accepted.  Every address is formed in 64-bit arithmetic.  exp is expf.  No
 * float atomics, no host read: bitwise reproducible and capturable.  workspace, 16-byte aligned (0
 * bytes, NULL allowed, when nnz <= 128): psa_attention_workspace_bytes(nnz, H, F) bytes for the
 * forward; the backward needs no more than the same call gives. */
size_t psa_attention_workspace_bytes(int64_t nnz, int64_t H, int64_t F);
int psa_attention_fw(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                     const float* bias, int64_t bias_heads, float scale, int64_t M, int64_t N, int64_t H, int64_t K,
                     int64_t F, int64_t nnz, float* out, float* stat, void* workspace, size_t workspace_bytes,
                     psa_stream_t stream);
int psa_attention_bw_entries(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                             const float* bias, int64_t bias_heads, float scale, const float* grad_out,
                             const float* out, const float* stat, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F,
                             int64_t nnz, float* p, float* ds, void* workspace, size_t workspace_bytes,
                             psa_stream_t stream);

/* ---- fused sparse attention with two-byte dense operands.  dtype names the format of q, k, v, out and
 * grad_out: PSA_BF16 is served, any other code is PSA_ERR_INVALID_ARG.  Semantics, layouts, the
 * non-finite rule, the long-row plan and the workspace (psa_attention_workspace_bytes(nnz, H, F): the
 * partials stay fp32) are those of psa_attention_fw / psa_attention_bw_entries.  bias, stat, p and ds are
 * fp32; every product, the scores, the softmax and the accumulators are fp32 and a bf16 result is
 * rounded once (nearest even) where it is written: out = round(acc / l).
 *   psa_attention_half_bw_entries  forms delta from the saved, rounded out.
 *   psa_spmm_heads_half            value fp32 [nnz, H], mat [N, H, F]:
 *                                  out[r, h, f] = round(alpha * sum_{e in row r} value[e, h] * mat[col[e], h, f]),
 *                                  out [M, H, F] fully written; psa_spmm_heads' plan and workspace
 *                                  (psa_spmm_heads_workspace_bytes(nnz, H, F)).  The gradients of the
 *                                  attention: grad_q = (ds, k) with alpha = scale over the CSR view,
 *                                  grad_k = (ds, q) with alpha = scale and grad_v = (p, grad_out) with
 *                                  alpha = 1 over the CSC view.
 * 16-byte gathers of 8 elements when K % 8 == 0, F % 8 == 0 (psa_spmm_heads_half: F % 8 == 0) and the
 * two-byte operands are 16-byte aligned, 2-byte loads otherwise: any 2-byte alignment is accepted. */
int psa_attention_half_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                          const void* v, const float* bias, int64_t bias_heads, float scale, int64_t M, int64_t N,
                          int64_t H, int64_t K, int64_t F, int64_t nnz, void* out, float* stat, void* workspace,
                          size_t workspace_bytes, psa_stream_t stream);
int psa_attention_half_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                                  const void* v, const float* bias, int64_t bias_heads, float scale,
                                  const void* grad_out, const void* out, const float* stat, int64_t M, int64_t N,
                                  int64_t H, int64_t K, int64_t F, int64_t nnz, float* p, float* ds, void* workspace,
                                  size_t workspace_bytes, psa_stream_t stream);
int psa_spmm_heads_half(int dtype, const int64_t* rowptr, const int64_t* col, const float* value, const void* mat,
                        float alpha, int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, void* out,
                        void* workspace, size_t workspace_bytes, psa_stream_t stream);

/* ---- fused sparse attention with dropout of the attention weights, fp32 and two-byte operands: the
 * four entry points above with `double dropout_p, uint64_t seed` after scale.  Everything not said
 * here is as there: s, p = softmax_row(s) and stat = {m, l} do not change (dropout comes after the
 * softmax), nor do the layouts, the forms, the long-row plan and the workspace
 * (psa_attention_workspace_bytes).
 *   T          = floor(dropout_p * 2^24)                     (in double; 0 <= dropout_p < 1, anything
 *                                                             else, NaN included, is PSA_ERR_INVALID_ARG)
 *   r(e, h)    = mix64(rand_stream(seed, e) + h)             (csrc/rng.h; e = position of the entry in
 *                                                             CSR order, h = absolute head, uint64 wrap)
 *   keep(e, h) = (r(e, h) >> 40) >= T
 *   inv_keep   = float32(1 / (1 - dropout_p))
 *   out[r, h, :] = inv_keep * sum_{e in row r} keep(e, h) * p[e, h] * v[col[e], h, :]
 * The mask depends on (seed, e, h) only: not on head blocks, chunks, the load width, the dtype or
 * forward versus backward, so the fp32 and bf16 entry points drop the same entries for one seed and
 * a host restatement reproduces it bit for bit.  It is evaluated once per (entry, head) and never
 * stored; the seed is a launch argument, so a captured graph replays the same mask.  keep multiplies
 * the weight inside the sum (exact); inv_keep is applied once per output element after the division
 * by l, in fp32 (bf16: before the one rounding), by the row kernel and by the long-row combine.
 * dropout_p = 0 keeps everything and multiplies by 1: the bits of the plain entry points.
 *   psa_attention_dropout_bw_entries  with D = keep * inv_keep: dP = D * <grad_out, v>, delta =
 *                                     <grad_out, out> (out carries D), ds = p * (dP - delta), and
 *                                     p * D is written where p was, so that grad_v = (p, grad_out)
 *                                     over the CSC view needs nothing else.
 * Non-finite values by plain IEEE arithmetic: a dropped entry has weight exactly 0 and 0 against an
 * inf in v is NaN (no zero skipping); a NaN score poisons l whether or not its entry is dropped.
 *   psa_attention_dropout_mask        mask[e * H + h] = keep(e, h) as bytes (0 / 1), [nnz, H], fully
 *                                     written: the same mask for the unfused chain. */
int psa_attention_dropout_fw(const int64_t* rowptr, const int64_t* col, const float* q, const float* k, const float* v,
                             const float* bias, int64_t bias_heads, float scale, double dropout_p, uint64_t seed,
                             int64_t M, int64_t N, int64_t H, int64_t K, int64_t F, int64_t nnz, float* out,
                             float* stat, void* workspace, size_t workspace_bytes, psa_stream_t stream);
int psa_attention_dropout_bw_entries(const int64_t* rowptr, const int64_t* col, const float* q, const float* k,
                                     const float* v, const float* bias, int64_t bias_heads, float scale,
                                     double dropout_p, uint64_t seed, const float* grad_out, const float* out,
                                     const float* stat, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F,
                                     int64_t nnz, float* p, float* ds, void* workspace, size_t workspace_bytes,
                                     psa_stream_t stream);
int psa_attention_half_dropout_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* q, const void* k,
                                  const void* v, const float* bias, int64_t bias_heads, float scale, double dropout_p,
                                  uint64_t seed, int64_t M, int64_t N, int64_t H, int64_t K, int64_t F, int64_t nnz,
                                  void* out, float* stat, void* workspace, size_t workspace_bytes,
                                  psa_stream_t stream);
int psa_attention_half_dropout_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* q,
                                          const void* k, const void* v, const float* bias, int64_t bias_heads,
                                          float scale, double dropout_p, uint64_t seed, const void* grad_out,
                                          const void* out, const float* stat, int64_t M, int64_t N, int64_t H,
                                          int64_t K, int64_t F, int64_t nnz, float* p, float* ds, void* workspace,
                                          size_t workspace_bytes, psa_stream_t stream);
int psa_attention_dropout_mask(int64_t nnz, int64_t H, double dropout_p, uint64_t seed, uint8_t* mask,
                               psa_stream_t stream);

/* ---- fused GAT attention: the additive scores of a graph attention layer through the one-pass
 * kernels above, fp32 and two-byte operands.  Pattern, v [N, H, F], bias (NULL, [nnz] with
 * bias_heads = 1 or [nnz, H] with bias_heads = H), out, stat, the forms, the long-row plan and the
 * workspace (psa_attention_workspace_bytes(nnz, H, F); 0 bytes, NULL allowed, when nnz <= 128) are
 * those of psa_attention_fw / psa_attention_bw_entries; a_row [M, H] and a_col [N, H] hold one scalar
 * per node and head and take the place of q and k; H, F >= 1.
 *   z[e, h]      = (a_row[row(e), h] + a_col[col[e], h]) (+ bias)        (two rounded additions, the
 *                                                                        second skipped without a bias)
 *   s[e, h]      = z > 0 ? z : negative_slope * z                        (one rounded product; z == 0
 *                                                                        and a NaN take the slope branch)
 *   p, stat      = the row softmax of s and its {m, l}, as psa_attention_fw (of s after the activation)
 *   out[r, h, :] = inv_keep * sum_{e in row r} keep(e, h) * p[e, h] * v[col[e], h, :]
 * The dropout arguments are always present: T, keep(e, h) and inv_keep are those of
 * psa_attention_dropout_fw (the same entries dropped for the same seed, psa_attention_dropout_mask
 * gives the mask); dropout_p = 0 keeps everything and multiplies by 1, the bits of the maskless
 * computation, and the seed is then ignored.  No contraction in z and s, so the backward recomputes
 * the same bits.  negative_slope must be finite (else PSA_ERR_INVALID_ARG); it may be 0 or negative.
 *   psa_gat_attention_bw_entries  with D = keep * inv_keep (1 without dropout), delta = <grad_out, out>
 *                                 and dP = <grad_out[row(e), h, :], v[col[e], h, :]>: writes
 *                                 p * D [nnz, H] and dz [nnz, H] = p * (D * dP - delta) *
 *                                 (z > 0 ? 1 : negative_slope); a row without entries writes
 *                                 nothing.  grad_a_row is the sum of dz over the entries of a row,
 *                                 grad_a_col over those of a column, grad_v = (p, grad_out) over the CSC
 *                                 view (psa_spmm_heads), grad_bias = dz (summed over the heads for
 *                                 bias_heads = 1).
 * Non-finite values by plain IEEE arithmetic, as psa_attention_fw: a NaN, a +inf or nothing but -inf
 * among the scores of a row and head is NaN in out[r, h, :]; -inf among finite scores has weight
 * exactly 0.  A -inf bias therefore masks its entry for negative_slope > 0; with negative_slope == 0
 * it gives 0 * -inf = NaN and poisons its row and head (not special-cased).
 * a_row and a_col are read with element loads at any element alignment; the 16-byte form of v, out
 * (and grad_out) needs F % 4 == 0 (two-byte operands: F % 8 == 0) and 16-byte alignment of those
 * three, any element alignment is served otherwise.  Every address is formed in 64-bit arithmetic.
 * No float atomics, no host read: bitwise reproducible and capturable.
 *   psa_gat_attention_half_*      dtype names the format of a_row, a_col, v, out and grad_out
 *                                 (PSA_BF16 is served): half-width loads, every sum, the activation,
 *                                 the softmax and stat fp32, out rounded once; bias, p and dz fp32. */
int psa_gat_attention_fw(const int64_t* rowptr, const int64_t* col, const float* a_row, const float* a_col,
                         const float* v, const float* bias, int64_t bias_heads, float negative_slope, double dropout_p,
                         uint64_t seed, int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, float* out,
                         float* stat, void* workspace, size_t workspace_bytes, psa_stream_t stream);
int psa_gat_attention_bw_entries(const int64_t* rowptr, const int64_t* col, const float* a_row, const float* a_col,
                                 const float* v, const float* bias, int64_t bias_heads, float negative_slope,
                                 double dropout_p, uint64_t seed, const float* grad_out, const float* out,
                                 const float* stat, int64_t M, int64_t N, int64_t H, int64_t F, int64_t nnz, float* p,
                                 float* dz, void* workspace, size_t workspace_bytes, psa_stream_t stream);
int psa_gat_attention_half_fw(int dtype, const int64_t* rowptr, const int64_t* col, const void* a_row,
                              const void* a_col, const void* v, const float* bias, int64_t bias_heads,
                              float negative_slope, double dropout_p, uint64_t seed, int64_t M, int64_t N, int64_t H,
                              int64_t F, int64_t nnz, void* out, float* stat, void* workspace, size_t workspace_bytes,
                              psa_stream_t stream);
int psa_gat_attention_half_bw_entries(int dtype, const int64_t* rowptr, const int64_t* col, const void* a_row,
                                      const void* a_col, const void* v, const float* bias, int64_t bias_heads,
                                      float negative_slope, double dropout_p, uint64_t seed, const void* grad_out,
                                      const void* out, const float* stat, int64_t M, int64_t N, int64_t H, int64_t F,
                                      int64_t nnz, float* p, float* dz, void* workspace, size_t workspace_bytes,
                                      psa_stream_t stream);

/* ---- pair intersection: the sampled sparse x sparse product, its gradients, common neighbours.
 * (x_ptr int64[x_lists + 1], x_idx, x_val) and (y_ptr int64[y_lists + 1], y_idx, y_val) are two
 * families of lists in CSR form — a CSR view, or a CSC view read as "the lists of the columns";
 * every list ascending and free of duplicates.  For every pair p in [0, P):
 *   out[p] = sum over k in X[pair_x[p]] n Y[pair_y[p]] of x_val * y_val * weight[k]
 * A NULL value array counts as ones; a NULL weight counts as ones, otherwise it is read at the common
 * index k (the caller keeps every index value inside it; without a weight index values are only
 * compared, as int64, and may lie above 2^32).  dtype: PSA_F32, PSA_F64 (values, weight, out) or
 * PSA_I64, the counting form: x_val, y_val and weight must be NULL and out[p] = |X n Y| as int64.
 * A stored 0 is not skipped (0 * inf = NaN), as in psa_spmm_heads.  A pair index outside
 * [0, x_lists) / [0, y_lists) reads nothing and writes 0: the pair list is never taken on trust.
 * Pairs are independent: any order, duplicates allowed.  out is fully written.  P == 0 launches
 * nothing; NULL required pointers, negative sizes, another dtype, and values or a weight with
 * PSA_I64 return PSA_ERR_INVALID_ARG.
 * The shorter list of a pair is the probe list (tie: X) and each of its elements is binary-searched
 * in the other.  A probe list of at most 32 elements is run by 8 lanes (8 pairs per wave, lane l
 * takes elements l, l + 8, ...), a longer one by a whole wave after the wave's short pairs (lane l
 * takes l, l + 64, ...).  Each lane adds its terms (x_val * y_val) * weight[k] in probe order from 0,
 * every multiply and add rounded on its own (no FMA); the 8 or 64 partials are folded by the xor
 * butterfly 1, 2, 4, ...  The sum order is a function of the two list lengths alone.  Every address
 * is formed in 64-bit arithmetic and the grid strides over the pairs, so P is unbounded.  No
 * workspace, no atomics, no host read: bitwise reproducible and capturable. */
int psa_pair_intersect(int dtype, const int64_t* x_ptr, const int64_t* x_idx, const void* x_val, int64_t x_lists,
                       const int64_t* y_ptr, const int64_t* y_idx, const void* y_val, int64_t y_lists,
                       const void* weight, const int64_t* pair_x, const int64_t* pair_y, int64_t P, void* out,
                       psa_stream_t stream);

/* ---- ego_k_hop_sample (torch_sparse ego_k_hop_sample_adj, the op behind PyG's
 * ShaDowKHopSampler): every seed gets a k-hop neighbourhood of its own in a SQUARE N x N CSR
 * matrix with sorted rows, and the subgraphs induced on the neighbourhoods come back as one
 * block-diagonal matrix.  Seeds may repeat: every position of `seeds` is an ego of its own.
 *
 * Walk list: one global sequence of entries; entries [0, S) are the seeds and entry i belongs
 * to ego i.  Hop l expands every entry of hop l - 1, duplicates included, and a child belongs
 * to its parent's ego.  The parent at walk index i that holds node v makes the picks of
 * psa_sample_count / psa_sample_select for (deg(v), num_neighbors, replace) with the draws of
 * STREAM i (draw t is randint(seed, i, t, .); Floyd's walk draws randint(seed, i, t,
 * deg - k + t)), so hop 1 of ego i makes the picks of sample_adj(seeds, k_1, replace, seed)
 * for row i.  num_neighbors >= 0: the hop has slots = F * num_neighbors, slot f * k + t is
 * pick t of parent f; a slot past its parent's picks, or of an empty parent, is empty (node
 * -1), keeps its index and stays empty in later hops: the caller knows the numbering without
 * a read.  num_neighbors < 0: the slots are the stored entries of the parents' rows in
 * (parent, storage) order, slots = parent_ptr[F].
 * Every slot writes node (or -1), ego, and key = ego * N + node; an empty slot writes the key
 * of its ego's seed, which entry `ego` holds already, so the distinct keys are exactly the
 * node sets.  There is no relabel map and no workspace.
 *
 * The hop loop belongs to the caller (paddle_sparse_amd/ops.py::ego_k_hop_sample):
 *   psa_ego_init(...)             walk entries [0, S); zeroes the flag word
 *   per hop with num_neighbors != 0:
 *     num_neighbors < 0 only:     psa_ego_hop_count -> psa_count2ptr -> parent_ptr,
 *                                 slots = parent_ptr[F]                          [host read]
 *     psa_ego_hop_pick(...)       node, ego, key of the hop's slots
 *   psa_index_sort over all keys (bound S * N), psa_unique_count_after_sort / psa_unique_write:
 *   n, n_id = key % N, ego_of = key / N                                        [host read]
 *   psa_ind2ptr(ego_of) -> ptr int64[S + 1]
 *   psa_ego_induce_count(...)     root[g] = position in n_id of (g, seeds[g]) (-1 for a seed
 *                                 outside); counts[r] = entries (v, c) of the matrix, v = n_id[r],
 *                                 with c in the node set of ego_of[r]
 *   psa_count2ptr(counts) -> rowptr' ; psa_ego_total: state = {rowptr'[n], flags}  [host read]
 *   psa_ego_induce_write(...)     col_out[q] = ptr[g] + rank of c in ego g's set, edge_out[q] =
 *                                 the entry's storage position; q ascends in storage order
 *                                 from rowptr'[r], stored duplicates kept, so the result is
 *                                 sorted by (row', col') without a sort
 * Induce passes: the shorter of (row, ego list) probes the longer by binary search, tie: the
 * row probes.  A probe side of at most T = 32 elements (psa_ego_set_threshold) is run by 8
 * lanes, 8 rows per wave; longer ones by the whole wave after the wave's short rows.  Both
 * directions and every T give the same bits.
 * flags: one int64 on the device; PSA_EGO_SEED_OUTSIDE (such a seed is an empty entry) and
 * PSA_EGO_COL_OUTSIDE (a stored column outside [0, N): its slot is empty).
 * Buffers are plain typed arrays of the caller; every entry point takes their element count
 * and returns PSA_ERR_INVALID_ARG when one is short.  S and slots stay below 2^31 (slots
 * <= 2^31 - 16), S * N below 2^62, n below 2^31.  Deterministic; no atomics except the flag
 * word; no launch waits for another workgroup; not capturable in a graph (sizes depend on the
 * data). */
#define PSA_EGO_SEED_OUTSIDE 1
#define PSA_EGO_COL_OUTSIDE 2
/* Test/bench hook: T, the longest probe side that a group of 8 lanes runs (default 32, at
 * least 1).  Returns the previous value.  Every value produces the same bits. */
int psa_ego_set_threshold(int threshold);
/* node_out int64, ego_out int32, key_out int64: out_count >= S elements each. */
int psa_ego_init(const int64_t* seeds, int64_t S, int64_t N, int64_t* node_out, int32_t* ego_out, int64_t* key_out,
                 int64_t out_count, int64_t* flags, psa_stream_t stream);
/* counts[f] = stored entries of the row of parent_node[f] (0 for an empty entry). */
int psa_ego_hop_count(const int64_t* rowptr, int64_t N, const int64_t* parent_node, int64_t F, int64_t* counts,
                      int64_t counts_count, psa_stream_t stream);
/* parent_node / parent_ego: the F entries of the previous hop, walk indices [begin, begin + F);
 * parent_ptr int64[F + 1]: read when num_neighbors < 0 only (NULL otherwise). */
int psa_ego_hop_pick(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* seeds, int64_t S,
                     const int64_t* parent_node, const int32_t* parent_ego, int64_t F, const int64_t* parent_ptr,
                     int64_t begin, int64_t num_neighbors, int replace, uint64_t seed, int64_t slots,
                     int64_t* node_out, int32_t* ego_out, int64_t* key_out, int64_t out_count, int64_t* flags,
                     psa_stream_t stream);
/* root int64[S], counts int64[n]; col may be NULL for a matrix without entries. */
int psa_ego_induce_count(const int64_t* rowptr, const int64_t* col, int64_t N, const int64_t* seeds, int64_t S,
                         const int64_t* n_id, const int64_t* ego_of, const int64_t* ptr, int64_t n, int64_t* root,
                         int64_t root_count, int64_t* counts, int64_t counts_count, psa_stream_t stream);
/* state int64[2] = {rowptr_out[n], *flags}: one host read serves both. */
int psa_ego_total(const int64_t* rowptr_out, int64_t n, const int64_t* flags, int64_t* state, psa_stream_t stream);
int psa_ego_induce_write(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t S, const int64_t* n_id,
                         const int64_t* ego_of, const int64_t* ptr, int64_t n, const int64_t* rowptr_out,
                         int64_t nnz_out, int64_t* col_out, int64_t* edge_out, int64_t out_count,
                         psa_stream_t stream);

/* ---- temporal_neighbor_sample (torch_sparse hetero_temporal_neighbor_sample on one node type,
 * the op behind PyG's NeighborLoader(time_attr=...)) ----
 * Per-seed sampling under a time bound: ego g takes entries with time <= seed_time[g] only,
 * and the SAMPLED entries of all egos come back as one block-diagonal matrix.
 *
 * The matrix comes with a time order (paddle_sparse_amd/temporal.py::EdgeTimeOrder): order
 * int64[nnz] holds, inside every row, the storage positions ascending by (time, position), and
 * sorted_time int64[nnz] their times.  The eligible set of a parent holding node v in ego g is
 * the prefix of row v's segment with sorted_time <= seed_time[g]; c is its length (one
 * upper-bound search) and a pick is a rank in [0, c), i.e. the entry order[rowptr[v] + rank].
 *
 * Walk list, streams and slot numbering are ego_k_hop_sample's (above): psa_ego_init writes
 * the seeds, hop l expands every entry of hop l - 1, the parent at walk index i draws on
 * stream i of `seed`, a hop with k >= 0 has F * k slots and a slot past its parent's picks is
 * empty for good.  Ranks of a parent (csrc/temporal_pick.h):
 *   k < 0                          0 .. c-1
 *   strategy 1 (last)              c-1, c-2, ..., c-min(k, c)
 *   strategy 0, replace            randint(seed, i, t, c) for t < k; none when c == 0
 *   strategy 0, no replace, c <= k 0 .. c-1
 *   strategy 0, no replace, c > k  the exact Floyd walk: j = c - k + t, r = randint(seed, i, t,
 *                                  j + 1), pick = r was picked before ? j : r
 * Every slot writes node (or -1), ego, key = ego * N + node (an empty slot: the key of its
 * ego's seed) and edge key = ego * nnz + e (an empty slot: the sentinel S * nnz).
 *
 * The hop loop belongs to the caller (paddle_sparse_amd/ops.py::temporal_neighbor_sample):
 *   psa_ego_init(...)                 walk entries [0, S); zeroes the flag word
 *   per hop with num_neighbors != 0:
 *     num_neighbors < 0 only:         psa_temporal_hop_count -> psa_count2ptr -> parent_ptr,
 *                                     slots = parent_ptr[F]                        [host read]
 *     psa_temporal_hop_pick(...)      node, ego, key, edge key of the hop's slots
 *   node keys: psa_index_sort, psa_unique_* -> n, n_id, ego_of; psa_ind2ptr -> ptr  [host read]
 *   edge keys (one sentinel appended): psa_index_sort, psa_unique_count_after_sort,
 *   psa_temporal_total: state = {distinct keys, sort fault word, flags}            [host read]
 *   psa_unique_write -> key_ego, key_edge; the sentinel is the last distinct key: m = count - 1
 *   psa_temporal_finish(...)          root[g]; row', col', e_id of the m entries, which are in
 *                                     (row', col') order already; psa_ind2ptr(row') -> rowptr'
 * flags: one int64 on the device; PSA_EGO_SEED_OUTSIDE, PSA_EGO_COL_OUTSIDE (raised where the
 * pick reads the column: its slot is empty) and PSA_TEMPORAL_BAD_INDEX (rowptr, order, or the
 * keys do not describe the matrix: the slot or entry is neutralised, nothing is read or
 * written out of bounds).  S < 2^31, slots <= 2^31 - 16, S * N and S * nnz below 2^62.
 * Deterministic; no atomics except the flag word; no launch waits for another workgroup;
 * grids are sized from the work and not capped; not capturable in a graph. */
#define PSA_TEMPORAL_BAD_INDEX 4
/* counts[f] = eligible entries of parent f (0 for an empty entry). */
int psa_temporal_hop_count(const int64_t* rowptr, const int64_t* sorted_time, int64_t N, int64_t nnz,
                           const int64_t* seed_time, int64_t S, const int64_t* parent_node, const int32_t* parent_ego,
                           int64_t F, int64_t* counts, int64_t counts_count, int64_t* flags, psa_stream_t stream);
/* strategy: 0 uniform, 1 last (replace must be 0).  parent_ptr int64[F + 1]: read when
 * num_neighbors < 0 only.  The four outputs hold out_count >= slots elements each. */
int psa_temporal_hop_pick(const int64_t* rowptr, const int64_t* col, const int64_t* order, const int64_t* sorted_time,
                          int64_t N, int64_t nnz, const int64_t* seeds, const int64_t* seed_time, int64_t S,
                          const int64_t* parent_node, const int32_t* parent_ego, int64_t F, const int64_t* parent_ptr,
                          int64_t begin, int64_t num_neighbors, int replace, int strategy, uint64_t seed, int64_t slots,
                          int64_t* node_out, int32_t* ego_out, int64_t* key_out, int64_t* edge_key_out,
                          int64_t out_count, int64_t* flags, psa_stream_t stream);
/* state int64[3] = {count_words[0], count_words[1], *flags}: one host read serves all three. */
int psa_temporal_total(const int64_t* count_words, const int64_t* flags, int64_t* state, psa_stream_t stream);
/* key_ego / key_edge int64[m]: the distinct edge keys split by nnz, ascending.  root int64[S];
 * row_out, col_out, edge_out int64[m]. */
int psa_temporal_finish(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, const int64_t* seeds,
                        int64_t S, const int64_t* key_ego, const int64_t* key_edge, int64_t m, const int64_t* n_id,
                        const int64_t* ptr, int64_t n, int64_t* root, int64_t root_count, int64_t* row_out,
                        int64_t* col_out, int64_t* edge_out, int64_t out_count, int64_t* flags, psa_stream_t stream);
/* Host only (tests): the ranks of one parent on stream `stream_index`, by the text the kernels
 * run, into ranks[0 .. count); returns count, or -1 for bad arguments or ranks_count < count. */
int64_t psa_temporal_pick_host(const int64_t* sorted_time, int64_t start, int64_t deg, int64_t bound, int64_t k,
                               int replace, int strategy, uint64_t seed, int64_t stream_index, int64_t* ranks,
                               int64_t ranks_count);

/* ---- segment_topk: keep the k greatest entries of every segment (csrc/topk.hip,
 * csrc/topk_select.h).  A selection by value, not a sort: nothing is reordered.
 *
 * Segment s holds the positions j in [indptr[s], indptr[s + 1]); its element is
 * x_j = value[perm ? perm[j] : j].  value is `dtype`[n] (PSA_F32, PSA_F64, PSA_I32, PSA_I64,
 * PSA_F16 or PSA_BF16), indptr int64[nseg + 1]; perm (int64[n], may be NULL) is trusted to be a
 * permutation of [0, n): with the csr2csc of a CSR matrix and its colptr the segments are the
 * columns, and nothing is transposed.
 *
 * Key.  Every element maps to an unsigned key of 32 bits (fp32, fp16, bf16, int32) or 64 bits
 * (fp64, int64) that preserves the value order.  Every NaN, whatever its sign or payload, maps
 * to the single greatest key (torch.topk's rule for both directions); -0.0 and +0.0 map to one
 * key; with largest == 0 the key is complemented, so the rule below only ever keeps the k
 * greatest keys (NaN is then the least wanted).
 *
 * Rule.  Entry j of segment s is kept iff
 *   #{j' in s : key(j') > key(j)} + #{j' in s : key(j') == key(j), j' < j} < k_s,
 * so exactly min(max(k_s, 0), len_s) entries are kept and ties go to the earlier position in
 * segment order.  k_s = k_seg[s] when k_seg (int64[nseg]) is given, the scalar k otherwise;
 * k_s <= 0 keeps nothing.  The result is a pure function of the input and repeats bit for bit.
 *
 * Output.  keep[perm ? perm[j] : j] = 1 or 0 (uint8[n], in storage order).  Every position
 * inside a valid segment is written and nothing else is.  A segment whose bounds do not satisfy
 * 0 <= begin <= end <= n reads nothing and writes nothing.
 *
 * Two launches at most, no workspace, no host read, capturable: groups of 8 .. 64 lanes rank
 * the segments of up to 64 entries in registers; workgroups find the threshold of the longer
 * ones by an MSB-first radix select with 8-bit digits, their keys in LDS up to 4096 entries and
 * read again from global memory by every pass above.
 *
 * PSA_ERR_INVALID_ARG: a negative size, an unknown dtype, more than 2^31 - 1 workgroups, or,
 * with n > 0 and nseg > 0, a NULL value, indptr or keep.  nseg == 0 or n == 0 returns PSA_OK
 * and touches nothing.
 *
 * psa_segment_topk_host runs the same steps (key mapping, digit passes, ordered write)
 * serially on HOST arrays: every result can be checked without a GPU. */
int psa_segment_topk(const void* value, int dtype, const int64_t* perm, const int64_t* indptr, int64_t nseg, int64_t n,
                     int64_t k, const int64_t* k_seg, int largest, uint8_t* keep, psa_stream_t stream);
int psa_segment_topk_host(const void* value, int dtype, const int64_t* perm, const int64_t* indptr, int64_t nseg,
                          int64_t n, int64_t k, const int64_t* k_seg, int largest, uint8_t* keep);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* PADDLE_SPARSE_HIP_H_ */
