"""The linear map of heterogeneous and relational layers: one weight matrix per type, one launch.

    out = ps.segment_matmul(x, ptr, weight)                      # rows sorted by type, ptr int64[T + 1]
    msg = ps.segment_matmul(x, ptr, weight, index=col_by_type)   # RGCN messages: x[col] is never materialised
    out = ps.typed_matmul(x, type, weight)                       # HeteroLinear on unsorted types, rows in x's order

out[r] = x_row(r) @ weight[t] for ptr[t] <= r < ptr[t + 1], x_row(r) = x[index[r]] or x[r]; weight is [T, K, F];
float32 or bfloat16 (fp32 sums, one rounding).  The kernels are csrc/segment_matmul.hip (MFMA); the raw ops are
ops.segment_matmul and ops.segment_matmul_bw_weight.  Both gradients come from the same kernels:

    grad_weight[t] = sum over the rows of segment t of x_row(r)^T (outer) grad_row(r)   (ops.segment_matmul_bw_weight)
    grad_x_row(r)  = grad_row(r) @ weight[t]^T                                          (the forward with trans_w)

Without `index` the second line is grad_x itself.  With a gather `index` (not injective) the [R, K] row gradients
are summed into [Nx, K] by the package's ops.scatter; for bfloat16 the operands of that product are widened to
float32, so the row gradients are float32 for the sum and rounded once after it.  typed_matmul's index is a
permutation, which serves as out_index of both products, so nothing is summed.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


class _SegmentMatmul(torch.autograd.Function):
    """index is None, a gather (permuted = False), or a permutation that also places the output rows (permuted)."""

    @staticmethod
    def forward(ctx, x, weight, ptr, index, permuted: bool):
        ctx.permuted = permuted
        ctx.save_for_backward(x, weight, ptr, index)
        return ops.segment_matmul(x, ptr, weight, index=index, out_index=index if permuted else None)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, ptr, index = ctx.saved_tensors
        g = grad_out.contiguous()
        place = index if ctx.permuted else None
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            # grad_row(r) @ weight[t]^T; row r of the result belongs to x[r], or to x[index[r]]
            if index is None or ctx.permuted:
                grad_x = ops.segment_matmul(g, ptr, weight, index=place, out_index=place, trans_w=True)
            else:
                # a gather: the row gradients are summed per row of x.  bfloat16 operands are widened (exactly) in
                # front of the product, so the rows stay float32 until the one rounding behind the sum
                rows = ops.segment_matmul(g.to(torch.float32), ptr, weight.to(torch.float32), trans_w=True)
                grad_x = ops.scatter(rows, index, x.shape[0], "sum").to(x.dtype)
        if ctx.needs_input_grad[1]:
            grad_w = ops.segment_matmul_bw_weight(x, ptr, g, index=index, out_index=place)
        return grad_x, grad_w, None, None, None


def _operands(x: torch.Tensor, weight: torch.Tensor):
    ops._gpu(x, "x")
    ops._gpu(weight, "weight")
    if x.dim() != 2 or weight.dim() != 3 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"x must be [Nx, K] and weight [T, K, F] (got {tuple(x.shape)} and {tuple(weight.shape)})")
    return x.contiguous(), weight.contiguous()


def segment_matmul(x: torch.Tensor, ptr: torch.Tensor, weight: torch.Tensor, index: Optional[torch.Tensor] = None,
                   trust_data: bool = True) -> torch.Tensor:
    """out [R, F] with out[r] = x_row(r) @ weight[t] for ptr[t] <= r < ptr[t + 1]; x_row(r) = x[index[r]] (index
    int64[R], any gather) or x[r].  x [Nx, K] and weight [T, K, F] are float32 or bfloat16; bfloat16 sums in float32
    and rounds once.  Differentiable in x and weight; with `index` the row gradients of bfloat16 operands are
    formed and summed into x's rows in float32 and rounded once after the sum.  ptr (and index) are trusted: no
    host read, capturable.  trust_data=False checks them first (one host read): ptr must run from 0 to R without
    decreasing, index must stay inside [0, Nx)."""
    x, weight = _operands(x, weight)
    ptr = ops._index(ptr, "ptr")
    index = None if index is None else ops._index(index, "index")
    if ptr.numel() != weight.shape[0] + 1:
        raise ValueError(f"ptr must be int64[T + 1] with T = {weight.shape[0]} (got {ptr.numel()} elements)")
    if not trust_data:
        R = x.shape[0] if index is None else index.numel()
        bad = (ptr[0] != 0) | (ptr[-1] != R) | (ptr[1:] < ptr[:-1]).any()
        if index is not None and R > 0:
            bad = bad | (index.min() < 0) | (index.max() >= x.shape[0])
        if bool(bad):
            raise ops.IndexRangeError("segment_matmul: ptr must run from 0 to R without decreasing and index must "
                                      "stay inside [0, Nx)")
    return _SegmentMatmul.apply(x, weight, ptr, index, False)


def typed_matmul(x: torch.Tensor, type: torch.Tensor, weight: torch.Tensor, trust_data: bool = False) -> torch.Tensor:
    """out [N, F] with out[i] = x[i] @ weight[type[i]], rows in the caller's order (PyG's HeteroLinear on unsorted
    types): one stable sort of `type`, a bincount, and ONE launch that gathers and places rows through the sorting
    permutation.  A type id outside [0, T) raises (one host read; trust_data=True skips it).  Differentiable in x and
    weight by the same two kernels through the same permutation."""
    x, weight = _operands(x, weight)
    type = ops._index(type, "type")
    T = weight.shape[0]
    if type.numel() != x.shape[0]:
        raise ValueError(f"type must have one entry per row of x ({x.shape[0]})")
    if not trust_data and type.numel() > 0 and bool((type.min() < 0) | (type.max() >= T)):
        raise ops.IndexRangeError(f"typed_matmul: a type id lies outside [0, {T})")
    _, perm = ops.index_sort(type, max_value=max(T, 1), check=True)
    ptr = ops.count2ptr(ops.bincount(type, T))
    return _SegmentMatmul.apply(x, weight, ptr, perm, True)
