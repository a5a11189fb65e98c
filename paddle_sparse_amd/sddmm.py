"""sddmm — the per-entry score <x[row], y[col]> of a sparse pattern (sampled dense-dense
matrix product): the first half of an attention layer, softmax (softmax.py) and SpMM
(matmul.py) being the rest.

The kernel is the one behind the gradient of SpMM wrt its values (psa_spmm_value_bw:
one wave per row, the row of x kept in registers, hub rows in 128-entry chunks); the
two gradients are SpMMs over the CSR and the CSC view, as in matmul.py.

With heads — x [M, H, K], y [N, H, K] — the scores are [nnz, H], one dot per head, from
psa_sddmm_heads (csrc/spmm_heads.hip: the same plan with the dot segmented per head); the
gradients are psa_spmm_heads over the same two views.
"""
from __future__ import annotations

import torch

from . import ops
from .tensor import SparseTensor


def sddmm(src: SparseTensor, x: torch.Tensor, y: torch.Tensor) -> SparseTensor:
    """Same pattern as `src`; values[e] = <x[row(e)], y[col(e)]> with x fp32 [M, K] and y fp32
    [N, K], or values[e, h] = <x[row(e), h], y[col(e), h]> with x fp32 [M, H, K] and y fp32
    [N, H, K].  The existing values of `src` are NOT read (multiply afterwards if they are
    wanted).  Differentiable in x and y."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"sddmm: {name} must be a torch.Tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"sddmm: {name} must be float32 (got {t.dtype})")
        if t.dim() not in (2, 3):
            raise ValueError(f"sddmm: {name} must be 2-D, or 3-D [rows, H, K]")
    M, N = src.sparse_size(0), src.sparse_size(1)
    if x.dim() != y.dim() or x.shape[0] != M or y.shape[0] != N or x.shape[1:] != y.shape[1:]:
        raise ValueError(f"sddmm: x must be [{M}, K] and y [{N}, K], or [{M}, H, K] and [{N}, H, K] "
                         f"(got {tuple(x.shape)}, {tuple(y.shape)})")
    st = src.storage

    def csc():  # asked for by the backward of y only
        csr2csc = st.csr2csc()
        return st.colptr(), st._row_in_csc_order(), csr2csc

    return src.set_value(ops.sddmm(st.rowptr(), st.col(), x, y, csc=csc), layout="coo")


SparseTensor.sddmm = lambda self, x, y: sddmm(self, x, y)
