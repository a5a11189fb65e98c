"""topk — keep the k largest (or smallest) stored entries of every row or column of a SparseTensor,
and segment_topk, the same selection over the segments of a pointer (TopKPooling: the k best node
scores of every graph of a batch, with the batch's `ptr`).

    knn = (adj @ adj).topk(8)                       # kNN-graph sparsification, per row
    gdc = diffusion.topk(64, dim=0)                 # GDC's sparsification="topk", per column
    att = pattern.topk(16, by=score.detach())       # prune an attention pattern by an external score
    perm = ps.segment_topk(score, batch_ptr, k)     # kept node positions, ascending

One HIP op (csrc/topk.hip: psa_segment_topk) marks the kept entries: dim = 1 runs over rowptr, dim = 0
over colptr with perm = csr2csc, so nothing is transposed and nothing is sorted.  The selection is by a
1-D key.  NaN counts as the greatest value in both directions (torch.topk's rule), -0.0 equals +0.0, and
of several equal values the earlier ones in the order of the row (column) are kept.  The kept entries
stay in storage order: the dense sorted [M, k] form of torch.topk is not built; a caller who wants the
at most k entries of a row in value order sorts them (ops.index_sort).
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import ops
from .storage import SparseStorage
from .tensor import SparseTensor


def _host_read(keep: torch.Tensor) -> torch.Tensor:
    """The one device-to-host read of this module: the number of kept entries sizes the result."""
    return torch.nonzero(keep).view(-1)


def _k(who: str, k, count: int, what: str):
    if isinstance(k, torch.Tensor):
        if k.dtype != torch.int64 or k.dim() != 1 or k.numel() != count:
            raise ValueError(f"{who}: a tensor k must be int64 with one entry per {what} ({count})")
        return k
    if not isinstance(k, int) or isinstance(k, bool):
        raise TypeError(f"{who}: k must be an int or an int64 tensor with one entry per {what}")
    return k


def topk(src: SparseTensor, k: Union[int, torch.Tensor], dim: int = 1, largest: bool = True,
         by: Optional[torch.Tensor] = None, return_e_id: bool = False):
    """The SparseTensor of src's sizes that holds, of every row (dim = 1 / -1) or column (dim = 0 / -2), the k
    stored entries with the largest (largest=False: smallest) values, in storage order (a sorted storage).  k is an
    int or an int64 tensor with one entry per row (column); k <= 0 keeps nothing of it.  The stored values select and
    must be 1-D; `by` (1-D, nnz elements in storage order) selects by an external score instead, and the matrix then
    keeps its own values of any shape.  Without values and without `by` all entries tie and the first k of every row
    (column) are kept.  NaN is the greatest value in both directions; ties go to the earlier entry.  The selection is
    not differentiable (`by` is detached); values that autograd tracks stay tracked through the gather, and a dropped
    entry gets the gradient 0.  return_e_id=True also returns the ascending storage positions of the kept entries.
    One host read per call (the kept total), so the op cannot be captured into a graph; ops.segment_topk can."""
    if not isinstance(src, SparseTensor):
        raise TypeError("topk: src must be a SparseTensor")
    if not isinstance(dim, int) or isinstance(dim, bool):
        raise TypeError("topk: dim must be an int")
    if dim < 0:
        dim += 2
    if dim not in (0, 1):
        raise ValueError("topk: dim must be 0 or 1 (-2 or -1)")
    st = src.storage
    value, nnz = st.value(), st.col().numel()
    k = _k("topk", k, src.sparse_size(dim ^ 1), "row" if dim == 1 else "column")
    if by is not None:
        if not isinstance(by, torch.Tensor) or by.dim() != 1 or by.numel() != nnz:
            raise ValueError(f"topk: by must be a 1-D tensor with one score per stored entry ({nnz})")
        key = by.detach()
    elif value is None:
        key = torch.zeros(nnz, dtype=torch.float32, device=st.col().device)
    elif value.dim() != 1:
        raise ValueError(f"topk: values of shape {tuple(value.shape)} do not order the entries; pass a 1-D score as by=")
    else:
        key = value.detach()
    if dim == 1:
        keep = ops.segment_topk(key, st.rowptr(), k, None, largest)
    else:
        perm = st.csr2csc()  # leaves colptr behind
        keep = ops.segment_topk(key, st.colptr(), k, perm, largest)
    e_id = _host_read(keep)
    count = st.rowcount() if dim == 1 else st.colcount()
    count = torch.minimum(count, k.clamp(min=0) if isinstance(k, torch.Tensor) else count.new_full((), max(k, 0)))
    row, col, _ = src.coo()
    storage = SparseStorage(row=row[e_id], col=col[e_id], value=None if value is None else value[e_id],
                            sparse_sizes=src.sparse_sizes(), rowcount=count if dim == 1 else None,
                            colcount=count if dim == 0 else None, is_sorted=True, trust_data=True)
    out = src.from_storage(storage)
    return (out, e_id) if return_e_id else out


def segment_topk(score: torch.Tensor, ptr: torch.Tensor, k: Union[int, torch.Tensor], largest: bool = True) -> torch.Tensor:
    """int64 positions, ascending, of the k largest (largest=False: smallest) of score[ptr[g] : ptr[g + 1]] for every
    segment g of ptr (int64[G + 1]): TopKPooling's `perm` from the node scores and the batch's ptr, with k an int or
    an int64[G] tensor such as ceil(ratio * n_g).  score is 1-D; it is detached.  Rule and limits as for topk.  One
    host read (the kept total)."""
    if not isinstance(score, torch.Tensor) or score.dim() != 1:
        raise ValueError("segment_topk: score must be a 1-D tensor")
    if not isinstance(ptr, torch.Tensor) or ptr.dim() != 1 or ptr.numel() < 1:
        raise ValueError("segment_topk: ptr must be a 1-D tensor with at least one element")
    k = _k("segment_topk", k, ptr.numel() - 1, "segment")
    return _host_read(ops.segment_topk(score, ptr, k, None, largest))


SparseTensor.topk = topk
