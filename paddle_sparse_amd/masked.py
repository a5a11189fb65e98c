"""masked_spspmm — the sampled sparse x sparse product C = (A @ diag(w) @ B) at the entries of a mask —
with common_neighbors and triangle_count, on the pair-intersection kernel of csrc/intersect.hip.

    c = a.masked_matmul(b, mask)                    # c_ij = sum_k a_ik b_kj for every stored (i, j) of mask
    cn = adj.common_neighbors(u, v)                 # |N(u) n N(v)| for a batch of node pairs
    tri = adj.triangle_count()                      # triangles per node

Every entry of the result is one intersection of two sorted lists: row i of A with column j of B.
Nothing is expanded, sorted or compacted, there is no intermediate of unknown size and no host read, where
`a @ b` forms every partial product first (spspmm.py).  SparseStorage caches the three views the forward
and the two value gradients read (CSR, CSC, csr2csc), and the gradients are the same kernel again: with G
the gradient on the mask's pattern,

    grad a_ik = w_k * sum_j g_ij b_kj     rows of G  n rows of B,       at the entries of A
    grad b_kj = w_k * sum_i a_ik g_ij     columns of A n columns of G,  at the entries of B
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .tensor import SparseTensor

_FLOATS = (torch.float32, torch.float64)


def _host_read(t: torch.Tensor) -> list:
    """The one device-to-host read of this module (the range check of common_neighbors)."""
    return t.tolist()


def _values_dtype(who: str, **tensors) -> Optional[torch.dtype]:
    """The common dtype of the given values and weight (None: none given, the counting form)."""
    dtype = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch.Tensor")
        if t.dtype not in _FLOATS:
            raise TypeError(f"{who}: {name} must be float32 or float64 (got {t.dtype})")
        if t.dim() != 1:
            raise ValueError(f"{who}: {name} must be 1-D (got {tuple(t.shape)})")
        if dtype is not None and t.dtype != dtype:
            raise TypeError(f"{who}: mixed dtypes ({dtype}, {name} {t.dtype})")
        dtype = t.dtype
    return dtype


def _check_weight(who: str, weight: Optional[torch.Tensor], size: int) -> Optional[torch.Tensor]:
    if weight is None:
        return None
    if weight.numel() != size:
        raise ValueError(f"{who}: weight must have {size} entries, one per common index (got {weight.numel()})")
    if ops.needs_grad(weight):
        raise NotImplementedError(f"{who}: the gradient of weight is not implemented (the values' gradients are)")
    return weight.detach().contiguous()


def _in_csc_order(src: SparseTensor, value: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if value is None else ops._gather_rows_raw(value, src.storage.csr2csc())


class _MaskedSpspmm(torch.autograd.Function):
    """values of (a @ diag(w) @ b) on mask's pattern; the gradients of value_a and value_b by the same kernel."""

    @staticmethod
    def forward(ctx, value_a, value_b, a, b, mask, weight):
        ctx.save_for_backward(value_a, value_b)
        ctx.a, ctx.b, ctx.mask, ctx.weight = a, b, mask, weight
        return _forward(a, b, mask, weight, value_a, value_b)

    @staticmethod
    def backward(ctx, grad):
        value_a, value_b = ctx.saved_tensors
        a, b, mask, weight = ctx.a, ctx.b, ctx.mask, ctx.weight
        grad = grad.contiguous()
        grad_a = grad_b = None
        if value_a is not None and ctx.needs_input_grad[0]:
            rowptr_m, col_m, _ = mask.csr()
            rowptr_b, col_b, _ = b.csr()
            row_a, col_a, _ = a.coo()
            grad_a = ops.pair_intersect((rowptr_m, col_m, grad), (rowptr_b, col_b, value_b), row_a, col_a,
                                        dtype=grad.dtype)
            if weight is not None:
                grad_a = grad_a * ops._gather_rows_raw(weight, col_a)
        if value_b is not None and ctx.needs_input_grad[1]:
            colptr_a, row_a_csc, _ = _structure_csc(a)
            colptr_m, row_m_csc, _ = _structure_csc(mask)
            row_b, col_b, _ = b.coo()
            grad_b = ops.pair_intersect((colptr_a, row_a_csc, _in_csc_order(a, value_a)),
                                        (colptr_m, row_m_csc, _in_csc_order(mask, grad)), row_b, col_b,
                                        dtype=grad.dtype)
            if weight is not None:
                grad_b = grad_b * ops._gather_rows_raw(weight, row_b)
        return grad_a, grad_b, None, None, None, None


def _structure_csc(src: SparseTensor):
    st = src.storage
    st.csr2csc()  # first: it leaves colptr behind
    return st.colptr(), st._row_in_csc_order(), None


def _forward(a, b, mask, weight, value_a, value_b, dtype=None):
    rowptr_a, col_a, _ = a.csr()
    colptr_b, row_b_csc, _ = _structure_csc(b)
    row_m, col_m, _ = mask.coo()
    # b's values are gathered into CSC order by every call, not taken from the storage's memo: a captured graph
    # replays the gather with the call and so follows values that were overwritten in place
    return ops.pair_intersect((rowptr_a, col_a, value_a), (colptr_b, row_b_csc, _in_csc_order(b, value_b)),
                              row_m, col_m, weight, dtype=dtype)


def masked_spspmm(a: SparseTensor, b: SparseTensor, mask: SparseTensor,
                  weight: Optional[torch.Tensor] = None) -> SparseTensor:
    """C = (a @ diag(weight) @ b) computed only at the stored entries of `mask`: a SparseTensor with mask's
    pattern, sizes and order (it shares mask's index arrays and cached layouts) and the values
    c_ij = sum_k a_ik * weight_k * b_kj.  mask's own values are not read.  An entry of mask outside the
    product's pattern stores 0, it is not dropped.  A missing weight counts as ones; an operand without
    values counts as ones, and when neither operand has values and there is no weight the result is the
    int64 COUNT of common indices.  Otherwise values and weight share one dtype, float32 or float64, which
    is the result's.  `a` and `b` must be coalesced (sorted rows without duplicates: what the intersection
    assumes, not checked — as for spspmm), `mask` too when a gradient is asked for.  Differentiable in the
    values of a and b; a weight that requires grad raises NotImplementedError."""
    for name, t in (("a", a), ("b", b), ("mask", mask)):
        if not isinstance(t, SparseTensor):
            raise TypeError(f"masked_spspmm: {name} must be a SparseTensor")
    if a.size(1) != b.size(0):
        raise ValueError(f"masked_spspmm: inner sizes differ (a {a.sparse_sizes()}, b {b.sparse_sizes()})")
    if mask.sparse_sizes() != (a.size(0), b.size(1)):
        raise ValueError(f"masked_spspmm: mask must be {(a.size(0), b.size(1))} (got {mask.sparse_sizes()})")
    value_a, value_b = a.storage.value(), b.storage.value()
    dtype = _values_dtype("masked_spspmm", **{"a's values": value_a, "b's values": value_b, "weight": weight})
    weight = _check_weight("masked_spspmm", weight, a.size(1))
    if ops.needs_grad(value_a) or ops.needs_grad(value_b):
        value = _MaskedSpspmm.apply(value_a, value_b, a, b, mask, weight)
    else:
        value = _forward(a, b, mask, weight, value_a, value_b, dtype or torch.int64)
    return mask.set_value(value, layout="coo")


def common_neighbors(adj: SparseTensor, row: torch.Tensor, col: torch.Tensor, weight: Optional[torch.Tensor] = None,
                     trust_data: bool = False) -> torch.Tensor:
    """out[p] = sum over the common out-neighbours k of row[p] and col[p] of adj_{row[p], k} * adj_{col[p], k} *
    weight[k], for arbitrary query pairs (they need not be edges): int64 counts when adj has no values and
    there is no weight, the values' / weight's float dtype otherwise.  weight is one float per column of adj:
    1 / log(deg) gives Adamic-Adar, 1 / deg resource allocation (README).  adj must be coalesced.  The pairs
    are range-checked with one host read (IndexError); trust_data=True skips it, which makes the call
    capturable — the kernel writes 0 for a pair outside the matrix either way.  Not differentiable."""
    if not isinstance(adj, SparseTensor):
        raise TypeError("common_neighbors: adj must be a SparseTensor")
    for name, t in (("row", row), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise TypeError(f"common_neighbors: {name} must be an integer tensor")
        if t.dim() != 1:
            raise ValueError(f"common_neighbors: {name} must be 1-D")
    if row.numel() != col.numel():
        raise ValueError(f"common_neighbors: row and col differ in length ({row.numel()}, {col.numel()})")
    rowptr, idx, value = adj.csr()
    _values_dtype("common_neighbors", **{"adj's values": value, "weight": weight})
    if ops.needs_grad(value):
        raise NotImplementedError("common_neighbors is not differentiable (masked_spspmm is, in the values)")
    weight = _check_weight("common_neighbors", weight, adj.size(1))
    row, col = row.to(torch.int64).contiguous(), col.to(torch.int64).contiguous()
    if not trust_data and row.numel():
        ops._gpu(row, "row"), ops._gpu(col, "col")
        lo, hi = _host_read(torch.stack((torch.minimum(row.min(), col.min()), torch.maximum(row.max(), col.max()))))
        if lo < 0 or hi >= adj.size(0):
            raise IndexError(f"common_neighbors: node ids must lie in [0, {adj.size(0)}) (got {lo} .. {hi})")
    value = None if value is None else value.detach()
    return ops.pair_intersect((rowptr, idx, value), (rowptr, idx, value), row, col, weight)


def triangle_count(adj: SparseTensor) -> torch.Tensor:
    """int64[N]: the triangles every node of a symmetric, loop-free, coalesced adjacency lies in — the row sums
    of (A @ A) at the entries of A in counting form, halved (each triangle at a node is met through both of
    its edges there).  adj's values are not read."""
    if not isinstance(adj, SparseTensor):
        raise TypeError("triangle_count: adj must be a SparseTensor")
    if not adj.is_quadratic():
        raise ValueError(f"triangle_count needs a square matrix (got {adj.sparse_sizes()})")
    pattern = adj.set_value(None)
    return masked_spspmm(pattern, pattern, pattern).sum(dim=1) // 2


SparseTensor.masked_matmul = lambda self, other, mask, weight=None: masked_spspmm(self, other, mask, weight)
SparseTensor.common_neighbors = common_neighbors
SparseTensor.triangle_count = triangle_count
