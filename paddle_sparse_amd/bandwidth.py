"""reverse_cuthill_mckee — torch_sparse/bandwidth.py (the reference's README lists it as not
yet supported): the bandwidth-reducing ordering of a square matrix and the matrix in it.

    out, perm = adj.reverse_cuthill_mckee()      # out == adj.permute(perm)
    y = (out @ x[perm])                          # == (adj @ x)[perm]

Upstream copies the matrix to the host and calls scipy's serial routine; here the ordering
is built on the GPU (csrc/rcm.hip).  It is scipy's algorithm with the ties fixed: the seed
of every component is the unvisited node with the smallest (degree, id) and every node
appends its unvisited neighbours in (degree, id) order, degree = stored entries of the row
(DESIGN 3.14).  scipy breaks degree ties among seeds by an unstable sort, so its perm may
differ; the bandwidths are within a few percent of each other in either direction.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .sample import permute
from .tensor import SparseTensor


def reverse_cuthill_mckee(src: SparseTensor, is_symmetric: Optional[bool] = None) -> Tuple[SparseTensor, torch.Tensor]:
    """(permute(src', perm), perm int64[N]) with src' = src when it is symmetric and
    src.to_symmetric() otherwise.  is_symmetric: True / False skip the symmetry check
    (src.is_symmetric(), a transpose and a comparison); None asks it.  The op has no
    gradient of its own: values flow through permute.  Not capturable in a graph: the
    launch sequence depends on the data (one host read per large level and per run of
    small ones)."""
    if not isinstance(src, SparseTensor):
        raise TypeError("src must be a SparseTensor")
    if is_symmetric is not None and not isinstance(is_symmetric, bool):
        raise TypeError(f"is_symmetric must be None or a bool (got {type(is_symmetric).__name__})")
    if not src.is_quadratic():
        raise ValueError(f"reverse_cuthill_mckee needs a square matrix (got {src.sparse_sizes()})")
    if is_symmetric is None:
        is_symmetric = src.is_symmetric()
    if not is_symmetric:
        src = src.to_symmetric()
    rowptr, col, _ = src.csr()
    perm = ops.reverse_cuthill_mckee(rowptr, col)
    return permute(src, perm), perm


SparseTensor.reverse_cuthill_mckee = lambda self, is_symmetric=None: reverse_cuthill_mckee(self, is_symmetric)
