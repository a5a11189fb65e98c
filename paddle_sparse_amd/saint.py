"""saint_subgraph — torch_sparse/saint.py (the reference's README lists it as not yet
supported): the subgraph induced by a node sample, GraphSAINT's mini-batch.

    node_idx = adj.random_walk(start, walk_length).view(-1).unique()
    sub, edge_index = adj.saint_subgraph(node_idx)

The structure comes from one HIP chain (csrc/walk.hip) with ONE host read: node i of
node_idx becomes row / column i (the last occurrence of a duplicated node), and every
stored entry between two selected nodes is kept, in selection order.  Unlike upstream,
whose result is marked sorted even when an unsorted node_idx leaves the columns out of
order, the result here is sorted by (row, col) (stable: ties keep selection order); a
non-decreasing node_idx, such as unique()'s output, is sorted already and is not
re-sorted.  edge_index holds the position in src's storage of every kept entry; the
values are value[edge_index], differentiable, with a deterministic backward.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import ops
from .storage import SparseStorage
from .tensor import SparseTensor


class _SaintValue(torch.autograd.Function):
    """value[edge_index]; grad(value) = the rows of grad' summed by edge id: a plain
    scatter when node_idx has no duplicates (every edge is kept at most once), otherwise a
    stable sort of the edge ids and a segment sum, so the result does not depend on
    scheduling."""

    @staticmethod
    def forward(ctx, value, edge_index, duplicates):
        ctx.save_for_backward(edge_index)
        ctx.duplicates, ctx.nnz = duplicates, value.shape[0]
        return ops._gather_rows_raw(value, edge_index)

    @staticmethod
    def backward(ctx, grad):
        (edge_index,) = ctx.saved_tensors
        grad = grad.contiguous()
        if ctx.duplicates and edge_index.numel() > 0:
            sorted_e, perm = ops.index_sort(edge_index, ctx.nnz, with_sorted_inputs=True, check=True)
            _, ptr, _, edges = ops.unique_sorted(sorted_e, ctx.nnz)
            grad = ops._segment_csr_raw(grad, ptr, "sum", perm)
            edge_index = edges
        return ops.diag_scatter(grad, edge_index, ctx.nnz), None, None


def saint_subgraph(src: SparseTensor, node_idx: torch.Tensor) -> Tuple[SparseTensor, torch.Tensor]:
    """(the [S, S] subgraph induced by node_idx, edge_index int64[nnz']): entry (i, j) of
    the result is src's entry (node_idx[i], node_idx[j]), duplicates kept; for a node that
    occurs more than once in node_idx, columns refer to its last occurrence.  node_idx may
    be of any integer dtype and order; a node outside the matrix raises IndexError."""
    if not src.is_quadratic():
        raise ValueError(f"saint_subgraph needs a square matrix (got {src.sparse_sizes()})")
    if not isinstance(node_idx, torch.Tensor) or node_idx.is_floating_point() or node_idx.is_complex() \
            or node_idx.dtype == torch.bool:
        raise TypeError("node_idx must be an integer tensor")
    if node_idx.dim() != 1:
        raise ValueError("node_idx must be 1-D")
    rowptr, col, value = src.csr()
    S = node_idx.numel()
    rowptr_out, row, col_out, edge_index, flags = ops.saint_subgraph(rowptr, col,
                                                                     node_idx.to(torch.int64).contiguous())
    if flags & ops.SAINT_UNSORTED and edge_index.numel() > 0:
        # rows are in order already (candidate order is row-major); sort the columns inside them
        keys, _ = ops.make_keys(row, col_out, S)
        keys, perm = ops.index_sort(keys, S * S, with_sorted_inputs=True, check=True)
        _, col_out = ops.split_keys(keys, S, want_hi=False)
        edge_index = ops._gather_rows_raw(edge_index, perm)
    if value is not None:
        if ops.needs_grad(value):
            value = _SaintValue.apply(value, edge_index, bool(flags & ops.SAINT_DUPLICATES))
        else:
            value = ops._gather_rows_raw(value, edge_index)
    out = src.from_storage(SparseStorage(row=row, rowptr=rowptr_out, col=col_out, value=value, sparse_sizes=(S, S),
                                         is_sorted=True, trust_data=True))
    return out, edge_index


SparseTensor.saint_subgraph = lambda self, node_idx: saint_subgraph(self, node_idx)
