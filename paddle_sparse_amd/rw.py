"""random_walk — torch_sparse/rw.py (the reference's README lists it as not yet supported).

One HIP launch runs every step of every walk (csrc/walk.hip), one lane per walk.  The
draws come from the counter-based stream of sample_adj (csrc/rng.h), selected by `seed`;
by default a fresh seed is taken from torch's global generator, so torch.manual_seed()
makes runs repeatable, as for sample_adj.

With `weighted` the step's entry is drawn in proportion to the stored values instead
(csrc/weighted.hip, weighted.EdgeCDF): the same random word, looked up in the row's CDF.

With `p` or `q` other than 1 the walk is node2vec's second-order walk (csrc/node2vec.hip):
the step's draw becomes a proposal, accepted with a chance that depends on where it leads
relative to the previous node; uniform or weighted alike.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import torch

from . import ops
from .tensor import SparseTensor
from .weighted import EdgeCDF, resolve


NODE2VEC_MAX_RATIO = 1024


def _node2vec_bias(p: float, q: float):
    """((thr0, thr1, thr2), max_tries) of the node2vec step for the return parameter p and the
    in-out parameter q: with a = (1/p, 1, 1/q) the chance to accept a proposal of class k is
    a[k] / max(a), as the integer thr[k] = int(a[k] / max(a) * 2^53); max_tries = 32 *
    ceil(max(a) / min(a)), after which the step takes its last proposal (chance < e^-32)."""
    p, q = float(p), float(q)
    for name, x in (("p", p), ("q", q)):
        if not (math.isfinite(x) and x > 0):
            raise ValueError(f"random_walk: {name} must be finite and > 0 (got {x})")
    a = (1.0 / p, 1.0, 1.0 / q)
    hi, lo = max(a), min(a)
    if hi / lo > NODE2VEC_MAX_RATIO:
        raise ValueError(f"random_walk: 1/p, 1 and 1/q may differ by a factor of {NODE2VEC_MAX_RATIO} at most "
                         f"(p = {p}, q = {q}: {hi / lo:.6g})")
    return tuple(int(x / hi * 2.0**53) for x in a), 32 * math.ceil(hi / lo)


def random_walk(src: SparseTensor, start: torch.Tensor, walk_length: int, seed: Optional[int] = None,
                weighted: Union[bool, EdgeCDF] = False, return_edge_ids: bool = False, p: float = 1.0,
                q: float = 1.0):
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

    p and q are node2vec's return and in-out parameters (finite, > 0; 1/p, 1 and 1/q within a
    factor of 1024 of each other).  With either other than 1, a step from v that arrived from t
    takes entry (v, x) with a chance in proportion to 1/p if x == t, 1 if t has an entry to x,
    1/q otherwise (times the entry's value when weighted): the plain step's draw is proposed
    and accepted with that chance over the largest of the three, at most 32 * ceil(largest /
    smallest) times, after which the last proposal is taken (a chance below e^-32).  "t has an
    entry to x" is the node2vec paper's d(t, x) = 1 and reads row t, the row the walk has just
    left; torch_cluster looks for t in row x instead.  On a symmetric matrix the two agree.
    With p == q == 1 the call is the first-order walk above, bit for bit.

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
    bias = None if p == 1 and q == 1 else _node2vec_bias(p, q)
    rowptr, col, _ = src.csr()
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    start = start.to(torch.int64).contiguous()
    if bias is not None:
        return ops.node2vec_walk(rowptr, col, resolve(src, weighted), start, walk_length, seed, bias[0], bias[1],
                                 return_edge_ids)
    if weighted is False and not return_edge_ids:
        return ops.random_walk(rowptr, col, start, walk_length, seed)
    return ops.random_walk_weighted(rowptr, col, resolve(src, weighted), start, walk_length, seed, return_edge_ids)


SparseTensor.random_walk = lambda self, start, walk_length, seed=None, weighted=False, return_edge_ids=False, \
    p=1.0, q=1.0: random_walk(self, start, walk_length, seed, weighted, return_edge_ids, p, q)
