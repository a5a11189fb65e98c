"""random_walk — torch_sparse/rw.py (the reference's README lists it as not yet supported).

One HIP launch runs every step of every walk (csrc/walk.hip), one lane per walk.  The
draws come from the counter-based stream of sample_adj (csrc/rng.h), selected by `seed`;
by default a fresh seed is taken from torch's global generator, so torch.manual_seed()
makes runs repeatable, as for sample_adj.

With `weighted` the step's entry is drawn in proportion to the stored values instead
(csrc/weighted.hip, weighted.EdgeCDF): the same random word, looked up in the row's CDF.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import ops
from .tensor import SparseTensor
from .weighted import EdgeCDF, resolve


def random_walk(src: SparseTensor, start: torch.Tensor, walk_length: int, seed: Optional[int] = None,
                weighted: Union[bool, EdgeCDF] = False, return_edge_ids: bool = False):
    """int64[len(start), walk_length + 1] random walks over the stored entries of a square
    matrix: row n starts at start[n]; each step moves to the column of an entry of the
    current row.  By default the entry is drawn uniformly (a duplicated entry counts as often
    as it is stored; values are ignored).

    weighted=True draws the entry in proportion to its value instead (1-D values >= 0; an
    entry of value zero is never taken, and a walk stays at a node whose values sum to zero).
    That builds the matrix's EdgeCDF on every call; pass an EdgeCDF built once to reuse it.
    return_edge_ids=True returns (walks, e_id): e_id int64[len(start), walk_length] holds the
    storage position of the entry taken at every step, -1 where the walk stayed.

    A node without entries keeps its walk where it is, as torch_cluster's random_walk
    does.  (torch_sparse's uniform kernel reads col[rowptr[cur]] on an empty row, which
    belongs to the next non-empty row.)

    Step 0 of walk n picks the edge that sample_adj(start, 1, replace=True, seed) picks
    for subset row n, with the same `weighted`.  start may be of any integer dtype; a start
    outside [0, N) raises IndexError."""
    if not src.is_quadratic():
        raise ValueError(f"random_walk needs a square matrix (got {src.sparse_sizes()})")
    if not isinstance(start, torch.Tensor) or start.is_floating_point() or start.is_complex() \
            or start.dtype == torch.bool:
        raise TypeError("start must be an integer tensor")
    if start.dim() != 1:
        raise ValueError("start must be 1-D")
    walk_length = int(walk_length)
    if walk_length < 0:
        raise ValueError("walk_length must be >= 0")
    if not isinstance(weighted, (bool, EdgeCDF)):
        raise TypeError("weighted must be a bool or an EdgeCDF")
    rowptr, col, _ = src.csr()
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    start = start.to(torch.int64).contiguous()
    if weighted is False and not return_edge_ids:
        return ops.random_walk(rowptr, col, start, walk_length, seed)
    return ops.random_walk_weighted(rowptr, col, resolve(src, weighted), start, walk_length, seed, return_edge_ids)


SparseTensor.random_walk = lambda self, start, walk_length, seed=None, weighted=False, return_edge_ids=False: \
    random_walk(self, start, walk_length, seed, weighted, return_edge_ids)
