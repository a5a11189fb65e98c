"""attention — sddmm, the row softmax and the aggregation of an attention layer (GAT, graph
transformers) as one op:

    s[e, h]      = scale * <q[row(e), h], k[col(e), h]>  (+ the stored value of e with bias=True)
    p[., h]      = softmax of s[., h] over the entries of each row
    out[r, h, :] = sum over the entries of row r of p[e, h] * v[col(e), h, :]

It computes what `sddmm(A, q, k).softmax(dim=1) @ v` computes, in one pass per row with a running
maximum and sum (csrc/attention.hip: psa_attention_fw), and writes nothing per entry: autograd
keeps q, k, v, the output and {max, sum} per row and head, where the chain keeps two [nnz, H]
tensors.  The backward recomputes the scores (psa_attention_bw_entries) and takes the gradients
from psa_spmm_heads over the CSR and the CSC view.  The chain of the three ops stays as it is.

Non-finite values: a row and head whose scores hold a NaN, a +inf or nothing but -inf is NaN in
out[r, h, :]; a -inf score among finite ones has weight exactly 0 (a mask); weight 0 against an
inf in v is NaN (no zero skipping); a row without entries gives 0.

q, k, v are float32 or bfloat16 (all three alike).  With bfloat16 operands the gathers are half-width
(csrc/attention_half.hip), every product, the scores, the softmax and the sums stay fp32, and out and
the gradients of q, k, v come back in bfloat16, each rounded once (the gradients from
csrc/spmm_heads_half.hip, with `scale` applied before the rounding); the bias, {max, sum} and the
gradient of the bias stay fp32.

Attention dropout (dropout_p, seed) happens inside the same kernels, after the softmax: see attention() below.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .tensor import SparseTensor


def attention(src: SparseTensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float = 1.0,
              bias: bool = False, dropout_p: float = 0.0, seed: Optional[int] = None) -> torch.Tensor:
    """Dense [M, H, F] from q [M, H, K], k [N, H, K] and v [N, H, F], all float32 or all bfloat16 (the result has
    their dtype), over the pattern of `src`; 2-D q [M, K], k [N, K], v [N, F] are one head and give [M, F].
    With bias=False the stored values of `src` are NOT read; with bias=True they must be fp32 [nnz] (shared by the
    heads) or [nnz, H], for either dtype of q, k, v, and are added to the scaled scores (-inf masks an entry).  Differentiable in q, k, v and, when they are tracked,
    the values; `scale` is a Python float.

    dropout_p (a Python float, 0 <= dropout_p < 1; anything else, NaN included, is a ValueError) drops attention
    weights after the softmax, inside the fused kernels: with T = floor(dropout_p * 2^24), an entry e (its position
    in CSR order) is kept for head h when the top 24 bits of a counter-based draw of (seed, e, h) are >= T, and
    out[r, h, :] = float32(1 / (1 - dropout_p)) * sum of keep * p * v.  The mask depends on (seed, e, h) only, not
    on the dtype or the shapes' route through the kernels; ops.attention_dropout_mask gives it to the unfused chain.
    The backward recomputes it: nothing with nnz rows is saved.  seed is an int in [0, 2^64) (other types: TypeError,
    other ranges: ValueError); seed=None draws one from torch's CPU default generator, so torch.manual_seed
    reproduces a run, without a device read or a sync.  The seed is a launch argument: a captured graph replays the
    SAME mask at every replay; give each replayed step its own graph or seed if that is not wanted.
    dropout_p == 0.0 is the op without dropout, bit for bit; the seed is then ignored."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"attention: {name} must be a torch.Tensor")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"attention: {name} must be float32 or bfloat16 (got {t.dtype})")
        if t.dim() not in (2, 3):
            raise ValueError(f"attention: {name} must be 2-D, or 3-D [rows, H, width]")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"attention: q, k, v must share one dtype (got {q.dtype}, {k.dtype}, {v.dtype})")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise TypeError("attention: scale must be a float")
    if not isinstance(bias, bool):
        raise TypeError("attention: bias must be a bool (the bias itself is the stored values of src)")
    dropout_p, seed = ops._dropout_args(dropout_p, seed)
    M, N = src.sparse_size(0), src.sparse_size(1)
    if not (q.dim() == k.dim() == v.dim()) or q.shape[0] != M or k.shape[0] != N or v.shape[0] != N \
            or q.shape[1:] != k.shape[1:] or (q.dim() == 3 and v.shape[1] != q.shape[1]):
        raise ValueError(f"attention: q, k, v must be [{M}, K], [{N}, K], [{N}, F] or [{M}, H, K], [{N}, H, K], "
                         f"[{N}, H, F] (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    st = src.storage
    value = None
    if bias:
        value = st.value()
        nnz, H = st.col().numel(), (q.shape[1] if q.dim() == 3 else 1)
        if value is None:
            raise ValueError("attention: bias=True needs stored values")
        if value.dtype != torch.float32:
            raise TypeError(f"attention: bias=True takes float32 values (got {value.dtype})")
        if value.shape not in ((nnz,), (nnz, H)):
            raise ValueError(f"attention: bias=True takes values [{nnz}] or [{nnz}, {H}] (got {tuple(value.shape)})")

    def csc():  # asked for by the backward of k and v only
        csr2csc = st.csr2csc()
        return st.colptr(), st._row_in_csc_order(), csr2csc

    return ops.attention(st.rowptr(), st.col(), q, k, v, bias=value, scale=float(scale), csc=csc, dropout_p=dropout_p,
                         seed=seed)


SparseTensor.attention = lambda self, q, k, v, scale=1.0, bias=False, dropout_p=0.0, seed=None: \
    attention(self, q, k, v, scale, bias, dropout_p, seed)
