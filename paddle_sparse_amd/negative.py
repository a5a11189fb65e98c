"""edge_ids, has_edge, negative_sampling, structured_negative_sampling — the lookup half of a
link-prediction step, on the kernels of csrc/negative.hip.

    e = adj.edge_ids(u, v)                               # where (u[q], v[q]) is stored, -1 where it is not
    m = adj.has_edge(u, v)
    row, col = adj.negative_sampling(num_neg)            # pairs that adj does not store
    tails = adj.structured_negative_sampling(row_pos)    # for every given source a column it has no entry to

A lookup is one lower-bound binary search in the query's row of the cached CSR view: no
linearised `row * N + col` key that overflows for hypersparse sizes.  A negative sample is that
search inside a bounded rejection loop on the device: every sample proposes pairs from its own
counter-based stream (csrc/rng.h, selected by `seed`; by default a fresh seed is taken from
torch's global generator, so torch.manual_seed() makes runs repeatable, as for random_walk) and
keeps the first one that is not stored.  One launch, no draw / lookup / mask round per retry
and no result of unknown size.

`adj` must be sorted by (row, col), as construction leaves it; duplicated entries are allowed.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .tensor import SparseTensor


def _host_read(t: torch.Tensor) -> int:
    """The one device-to-host read of this module (the range check of a lookup or of given sources)."""
    return int(t.item())


def _ids(who: str, **tensors):
    out = []
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise TypeError(f"{who}: {name} must be an integer tensor")
        if t.dim() != 1:
            raise ValueError(f"{who}: {name} must be 1-D")
        out.append(t)
    return out


def _adj(who: str, adj) -> SparseTensor:
    if not isinstance(adj, SparseTensor):
        raise TypeError(f"{who}: adj must be a SparseTensor")
    return adj


def _sampler_args(who: str, adj: SparseTensor, count: int, least: int, no_self_loops: bool, max_tries: int,
                  seed: Optional[int]):
    count, max_tries = int(count), int(max_tries)
    if count < least:
        raise ValueError(f"{who}: the number of samples must be >= {least} (got {count})")
    if not 1 <= max_tries <= ops.NEGATIVE_MAX_TRIES:
        raise ValueError(f"{who}: max_tries must lie in [1, {ops.NEGATIVE_MAX_TRIES}] (got {max_tries})")
    if no_self_loops and not adj.is_quadratic():
        raise ValueError(f"{who}: no_self_loops needs a square matrix (got {adj.sparse_sizes()})")
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    return count, max_tries, int(seed)


def edge_ids(adj: SparseTensor, row: torch.Tensor, col: torch.Tensor, trust_data: bool = False) -> torch.Tensor:
    """int64[Q]: for every query pair (row[q], col[q]) its position in the storage's order (the index into
    adj.storage.value(), row() and col()), or -1 where the entry is not stored; for a duplicated entry the
    first position.  row and col may be of any integer dtype.  A pair outside the matrix raises IndexError
    after one host read; trust_data=True skips the read, which makes the call capturable — the kernel writes
    -1 for such a pair either way."""
    adj = _adj("edge_ids", adj)
    row, col = _ids("edge_ids", row=row, col=col)
    if row.numel() != col.numel():
        raise ValueError(f"edge_ids: row and col differ in length ({row.numel()}, {col.numel()})")
    rowptr, idx, _ = adj.csr()
    pos, flags = ops.edge_lookup(rowptr, idx, adj.size(1), row.to(torch.int64), col.to(torch.int64))
    if not trust_data and pos.numel() and _host_read(flags) & ops.LOOKUP_RANGE:
        raise IndexError(f"edge_ids: a query pair lies outside the matrix {adj.sparse_sizes()}")
    return pos


def has_edge(adj: SparseTensor, row: torch.Tensor, col: torch.Tensor, trust_data: bool = False) -> torch.Tensor:
    """bool[Q]: whether (row[q], col[q]) is stored; arguments and errors as edge_ids."""
    return edge_ids(_adj("has_edge", adj), row, col, trust_data) >= 0


def negative_sampling(adj: SparseTensor, num_neg: int, no_self_loops: bool = False, max_tries: int = 64,
                      seed: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row, col), int64[num_neg] each: pairs drawn uniformly from the pairs of the M x N matrix that are not
    stored, with no_self_loops (square matrices only) from those off the diagonal.  Draws are with
    replacement: a pair may repeat (coalesce removes repeats).  Every sample makes at most max_tries (1 ..
    32768) proposals; one whose proposals were all refused is (-1, -1), with a chance of (share of refused
    pairs) ^ max_tries — filter with `row >= 0` on a dense matrix.  No host read; capturable with a seed."""
    adj = _adj("negative_sampling", adj)
    num_neg, max_tries, seed = _sampler_args("negative_sampling", adj, num_neg, 0, no_self_loops, max_tries, seed)
    rowptr, idx, _ = adj.csr()
    row, col, _ = ops.negative_sample(rowptr, idx, adj.size(1), None, num_neg, no_self_loops, max_tries, seed)
    return row, col


def structured_negative_sampling(adj: SparseTensor, src: torch.Tensor, num_neg_per_src: int = 1,
                                 no_self_loops: bool = False, max_tries: int = 64, seed: Optional[int] = None,
                                 trust_data: bool = False) -> torch.Tensor:
    """int64[len(src), num_neg_per_src]: for every given source s = src[n], columns c drawn uniformly from
    those with (s, c) not stored (and c != s with no_self_loops) — the "corrupt the tail" form, with src the
    rows of the positive edges.  Draws are with replacement; -1 where all max_tries proposals were refused
    (a full row always gives -1).  src may be of any integer dtype; a source outside [0, M) raises IndexError
    after one host read, which trust_data=True skips (capturable with a seed; the kernel writes -1 for that
    source either way)."""
    adj = _adj("structured_negative_sampling", adj)
    src, = _ids("structured_negative_sampling", src=src)
    k, max_tries, seed = _sampler_args("structured_negative_sampling", adj, num_neg_per_src, 1, no_self_loops,
                                       max_tries, seed)
    rowptr, idx, _ = adj.csr()
    col, flags = ops.negative_sample(rowptr, idx, adj.size(1), src.to(torch.int64), k, no_self_loops, max_tries, seed)
    if not trust_data and col.numel() and _host_read(flags) & ops.LOOKUP_RANGE:
        raise IndexError(f"structured_negative_sampling: a source lies outside [0, {adj.size(0)})")
    return col.view(src.numel(), k)


SparseTensor.edge_ids = edge_ids
SparseTensor.has_edge = has_edge
SparseTensor.negative_sampling = negative_sampling
SparseTensor.structured_negative_sampling = structured_negative_sampling
