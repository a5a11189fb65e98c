"""gat_attention — the aggregation of a GAT layer as one op: additive scores, LeakyReLU, the row
softmax and the sum over the neighbours,

    z[e, h]      = a_row[row(e), h] + a_col[col(e), h]  (+ the stored value of e with bias=True)
    s[e, h]      = z if z > 0 else negative_slope * z
    p[., h]      = softmax of s[., h] over the entries of each row
    out[r, h, :] = sum over the entries of row r of p[e, h] * v[col(e), h, :]

with a_row = (h W · a_l) and a_col = (h W · a_r) one scalar per node and head.  It runs in the
kernels of `attention` (csrc/attention.hip, csrc/attention_half.hip) with the dot product replaced
by the sum: one pass per row, nothing written per entry, autograd keeps a_row, a_col, v, the output
and {max, sum} per row and head.  The edge term of GAT layers with edge features is the bias: it is
added inside the activation.

Non-finite values as `attention`.  A -inf stored value masks its entry for negative_slope > 0; with
negative_slope == 0 it is 0 * -inf = NaN and poisons its row and head.

Dtypes, dropout and the seed as `attention`: a_row, a_col, v all float32 or all bfloat16, the same
mask for the same (dropout_p, seed).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .tensor import SparseTensor


def gat_attention(src: SparseTensor, a_row: torch.Tensor, a_col: torch.Tensor, v: torch.Tensor,
                  negative_slope: float = 0.2, bias: bool = False, dropout_p: float = 0.0,
                  seed: Optional[int] = None) -> torch.Tensor:
    """Dense [M, H, F] from a_row [M, H], a_col [N, H] and v [N, H, F], all float32 or all bfloat16 (the result has
    their dtype), over the pattern of `src`; a_row [M], a_col [N], v [N, F] are one head and give [M, F].
    With bias=False the stored values of `src` are NOT read; with bias=True they must be fp32 [nnz] (shared by the
    heads) or [nnz, H] and are added to a_row + a_col before the activation.  Differentiable in a_row, a_col, v and,
    when they are tracked, the values.  negative_slope is a finite Python number (a bool or another type is a
    TypeError, NaN or inf a ValueError); dropout_p and seed as SparseTensor.attention."""
    for name, t in (("a_row", a_row), ("a_col", a_col), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"gat_attention: {name} must be a torch.Tensor")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"gat_attention: {name} must be float32 or bfloat16 (got {t.dtype})")
    if not (a_row.dtype == a_col.dtype == v.dtype):
        raise TypeError(f"gat_attention: a_row, a_col, v must share one dtype (got {a_row.dtype}, {a_col.dtype}, "
                        f"{v.dtype})")
    negative_slope = ops._slope_arg(negative_slope)
    if not isinstance(bias, bool):
        raise TypeError("gat_attention: bias must be a bool (the bias itself is the stored values of src)")
    dropout_p, seed = ops._dropout_args(dropout_p, seed, "gat_attention")
    M, N = src.sparse_size(0), src.sparse_size(1)
    heads = v.dim() == 3
    if v.dim() not in (2, 3) or a_row.dim() != v.dim() - 1 or a_col.dim() != v.dim() - 1 or a_row.shape[0] != M \
            or a_col.shape[0] != N or v.shape[0] != N \
            or (heads and not (a_row.shape[1] == a_col.shape[1] == v.shape[1])):
        raise ValueError(f"gat_attention: a_row, a_col, v must be [{M}], [{N}], [{N}, F] or [{M}, H], [{N}, H], "
                         f"[{N}, H, F] (got {tuple(a_row.shape)}, {tuple(a_col.shape)}, {tuple(v.shape)})")
    st = src.storage
    value = None
    if bias:
        value = st.value()
        nnz, H = st.col().numel(), (v.shape[1] if heads else 1)
        if value is None:
            raise ValueError("gat_attention: bias=True needs stored values")
        if value.dtype != torch.float32:
            raise TypeError(f"gat_attention: bias=True takes float32 values (got {value.dtype})")
        if value.shape not in ((nnz,), (nnz, H)):
            raise ValueError(f"gat_attention: bias=True takes values [{nnz}] or [{nnz}, {H}] "
                             f"(got {tuple(value.shape)})")

    def csc():  # asked for by the backward of a_col and v only
        csr2csc = st.csr2csc()
        return st.colptr(), st._row_in_csc_order(), csr2csc

    return ops.gat_attention(st.rowptr(), st.col(), a_row, a_col, v, bias=value, negative_slope=negative_slope, csc=csc,
                             dropout_p=dropout_p, seed=seed)


SparseTensor.gat_attention = lambda self, a_row, a_col, v, negative_slope=0.2, bias=False, dropout_p=0.0, seed=None: \
    gat_attention(self, a_row, a_col, v, negative_slope, bias, dropout_p, seed)
