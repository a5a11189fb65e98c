"""remove_diag / set_diag / fill_diag / get_diag — torch_sparse/diag.py (the
reference's README lists them as not yet supported).

The k-th diagonal is the set of cells (r, r + k) inside the M x N matrix.  The
three rewriting ops are one HIP chain over the sorted CSR form (csrc/diag.hip):

    psa_diag_count   new row lengths (binary search per row) -> rowptr'   ONE host read: nnz'
    psa_diag_write   col' and value rows, balanced by output entries, no re-sort

Upstream builds masks over every entry, indexes with them and rebuilds the
storage from COO; here the result comes out sorted with rowptr and rowcount in
hand, and colcount carried over (adjusted) when the input had it.  The value
path is differentiable: the backward is a HIP gather through the output
position of every kept entry (zero for a removed one) and of every inserted one.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import ops
from .storage import SparseStorage
from .tensor import SparseTensor


def num_diag(M: int, N: int, k: int = 0) -> int:
    """Cells of the k-th diagonal inside an M x N matrix."""
    return ops.diag_extent(M, N, k)[1]


def diag_start(k: int = 0) -> int:
    """First row of the k-th diagonal."""
    return max(-k, 0)


class _DiagWrite(torch.autograd.Function):
    """psa_diag_write with the gradient maps: value' = kept values with the diagonal
    values spliced in; grad(value) = grad'[out_pos] (0 where removed), grad(diag) =
    grad'[diag_pos]."""

    @staticmethod
    def forward(ctx, value, diag_values, plan, rowptr, col):
        col_out, value_out, out_pos, diag_pos = ops.diag_write(plan, rowptr, col, value, diag_values, want_maps=True)
        ctx.save_for_backward(out_pos, diag_pos)
        ctx.mark_non_differentiable(col_out)
        return col_out, value_out

    @staticmethod
    def backward(ctx, _grad_col, grad):
        out_pos, diag_pos = ctx.saved_tensors
        grad = grad.contiguous()
        g_value = ops.diag_gather(grad, out_pos) if ctx.needs_input_grad[0] else None
        g_diag = ops.diag_gather(grad, diag_pos) if ctx.needs_input_grad[1] and diag_pos is not None else None
        return g_value, g_diag, None, None, None


class _GetDiag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, rowptr, col, M, N):
        out, pos = ops.get_diag(rowptr, col, value, M, N, want_pos=True)
        ctx.save_for_backward(pos)
        ctx.nnz = value.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad):
        (pos,) = ctx.saved_tensors
        return ops.diag_scatter(grad.contiguous(), pos, ctx.nnz), None, None, None, None


def _rewrite(src: SparseTensor, k: int, insert: bool, diag_values: Optional[torch.Tensor]) -> SparseTensor:
    st = src.storage
    M, N = st.sparse_sizes()
    rowptr, col, value = st.rowptr(), st.col(), st.value()
    plan = ops.diag_count(rowptr, col, M, N, k, insert, st._colcount)
    if value is not None and (ops.needs_grad(value) or ops.needs_grad(diag_values)):
        col_out, value_out = _DiagWrite.apply(value, diag_values, plan, rowptr, col)
    else:
        col_out, value_out, _, _ = ops.diag_write(plan, rowptr, col, value, diag_values)
    # rowptr / rowcount from the kernels, colcount adjusted; the CSC caches are rebuilt lazily
    return src.from_storage(SparseStorage(row=None, rowptr=plan.rowptr, col=col_out, value=value_out,
                                          sparse_sizes=(M, N), rowcount=plan.rowcount, colcount=plan.colcount,
                                          is_sorted=True, trust_data=True))


def _diag_rows(value: torch.Tensor, values, rows: int) -> torch.Tensor:
    """values broadcast to [rows, *value.shape[1:]] in value's dtype (ones for None)."""
    shape = (rows,) + tuple(value.shape[1:])
    if values is None:
        return torch.ones(shape, dtype=value.dtype, device=value.device)
    if not isinstance(values, torch.Tensor):
        return value.new_full(shape, values)
    return values.to(device=value.device, dtype=value.dtype).expand(shape).contiguous()


def remove_diag(src: SparseTensor, k: int = 0) -> SparseTensor:
    """Drops every stored (r, r + k) entry, duplicates included."""
    return _rewrite(src, int(k), False, None)


def set_diag(src: SparseTensor, values: Optional[torch.Tensor] = None, k: int = 0) -> SparseTensor:
    """remove_diag, then exactly one entry at every cell of the k-th diagonal, with
    `values` (broadcast to [num_diag, *], cast to the value dtype; ones when None).
    A value-less matrix gives a value-less result."""
    k = int(k)
    value = src.storage.value()
    diag_values = None
    if value is not None:
        diag_values = _diag_rows(value, values, num_diag(src.size(0), src.size(1), k))
    return _rewrite(src, k, True, diag_values)


def fill_diag(src: SparseTensor, fill_value: Union[float, int, torch.Tensor], k: int = 0) -> SparseTensor:
    """set_diag with every diagonal value equal to fill_value."""
    value = src.storage.value()
    if value is None:
        return set_diag(src, None, k)
    return set_diag(src, _diag_rows(value, fill_value, num_diag(src.size(0), src.size(1), int(k))), k)


def get_diag(src: SparseTensor) -> torch.Tensor:
    """The main diagonal as a dense [min(M, N), *value.shape[1:]] tensor: the last stored
    (r, r) entry of every row, zero where none is stored (float32 ones for a value-less
    matrix)."""
    st = src.storage
    M, N = st.sparse_sizes()
    value = st.value()
    if ops.needs_grad(value):
        return _GetDiag.apply(value, st.rowptr(), st.col(), M, N)
    return ops.get_diag(st.rowptr(), st.col(), value, M, N)[0]


SparseTensor.remove_diag = lambda self, k=0: remove_diag(self, k)
SparseTensor.set_diag = lambda self, values=None, k=0: set_diag(self, values, k)
SparseTensor.fill_diag = lambda self, fill_value, k=0: fill_diag(self, fill_value, k)
SparseTensor.get_diag = lambda self: get_diag(self)
