"""neighbor_sample — torch_sparse's multi-hop, layer-wise neighbour sampler (the op behind
PyG's NeighborLoader; CPU only upstream), on the HIP chain of csrc/neighbor.hip.

    sub, n_id, e_id, (nodes_per_hop, edges_per_hop) = adj.neighbor_sample(seeds, [15, 10, 5])
    out = sub @ x[n_id]          # rows [0, len(seeds)) are the seeds' aggregates

n_id starts as the seeds, local id = position in n_id.  Hop l expands the nodes that hop
l - 1 appended, every node at most once per call; a node at local id i makes sample_adj's
picks (same rules, same draws, stream i of `seed`), a picked column without a local id
gets the next one in order of its first slot.  sub is the [n, n] matrix of all emitted
entries (row' = the expanded node, col' = the picked one), sorted by (row', col'), ties in
slot order; e_id is the position in src's storage of every entry, the values are
value[e_id], differentiable with a deterministic backward.  Row ids grow with the hop, so
hop l's entries are the contiguous range [E_1 + ... + E_{l-1}, E_1 + ... + E_l) of sub and
the rows from S + new_1 + ... + new_{L-1} on are empty: what per-layer trimming needs.
directed=False returns the subgraph induced by the same n_id (saint_subgraph) instead, with
edges_per_hop None.

weighted=cdf (an EdgeCDF of src; True builds one) draws the picks of every hop with a
fan-out >= 0 in proportion to the stored values (csrc/neighbor.hip): with
replace=True every slot is the weighted pick of weighted sample_adj; with replace=False a
node draws its entries one after the other, each in proportion to the weights that are
left (torch.multinomial(w, k, False)), and makes min(k, entries of positive weight) picks.
One hop, neighbor_sample(batch, [k], weighted=cdf), is the weighted sample_adj without
replacement.  A fan-out of -1 takes every entry whatever its weight.

One relabel map (int32 per node of src) serves the whole call; a NeighborSampler keeps it
between calls, clean, so that a call costs stores per sampled node and never per node.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import ops
from .saint import _SaintValue, saint_subgraph
from .storage import SparseStorage
from .tensor import SparseTensor
from .weighted import EdgeCDF, resolve


class NeighborSampler:
    """sampler(seeds, seed=None) = src.neighbor_sample(seeds, num_neighbors, replace, directed, seed, weighted),
    with the relabel map held between calls.  One sampler serves one stream at a time.
    weighted=True builds the EdgeCDF once, here: it holds the values as they are now."""

    def __init__(self, src: SparseTensor, num_neighbors: Sequence[int], replace: bool = False, directed: bool = True,
                 weighted: Union[bool, EdgeCDF, None] = None):
        if not src.is_quadratic():
            raise ValueError(f"neighbor_sample needs a square matrix (got {src.sparse_sizes()})")
        if isinstance(num_neighbors, (str, bytes)) or not isinstance(num_neighbors, (list, tuple)) \
                or any(isinstance(k, bool) or not isinstance(k, int) for k in num_neighbors):
            raise TypeError("num_neighbors must be a list of ints")
        if any(k < -1 for k in num_neighbors):
            raise ValueError(f"num_neighbors must be >= -1 (got {list(num_neighbors)})")
        self.src, self.num_neighbors = src, list(num_neighbors)
        self.replace, self.directed = bool(replace), bool(directed)
        if weighted is not None and not isinstance(weighted, (bool, EdgeCDF)):
            raise TypeError("weighted must be None, a bool or an EdgeCDF")
        self._cum = resolve(src, weighted)  # None: the uniform picks
        self._workspace = None  # made by the first call, on the matrix's device

    def __call__(self, seeds: torch.Tensor, seed: Optional[int] = None):
        if not isinstance(seeds, torch.Tensor) or seeds.is_floating_point() or seeds.is_complex() \
                or seeds.dtype == torch.bool:
            raise TypeError("seeds must be an integer tensor")
        if seeds.dim() != 1:
            raise ValueError("seeds must be 1-D")
        src = self.src
        rowptr, col, value = src.csr()
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        if self._workspace is None:
            self._workspace = ops.NeighborWorkspace(src.sparse_size(0), rowptr.device)
        if self._cum is None:
            n_id, rowptr_out, col_out, e_id, nodes_per_hop, edges_per_hop = ops.neighbor_sample(
                rowptr, col, seeds.to(torch.int64).contiguous(), self.num_neighbors, self.replace, seed,
                workspace=self._workspace, want_edges=self.directed)
        else:
            n_id, rowptr_out, col_out, e_id, nodes_per_hop, edges_per_hop = ops.neighbor_sample(
                rowptr, col, seeds.to(torch.int64).contiguous(), self.num_neighbors, self.replace, seed,
                workspace=self._workspace, want_edges=self.directed, cum=self._cum)
        if not self.directed:
            sub, e_id = saint_subgraph(src, n_id)
            return sub, n_id, e_id, (nodes_per_hop, None)
        if value is not None:
            if ops.needs_grad(value):
                # replace=False emits every edge at most once: a plain scatter; otherwise sort + segment sum
                value = _SaintValue.apply(value, e_id, self.replace)
            else:
                value = ops._gather_rows_raw(value, e_id)
        n = n_id.numel()
        sub = src.from_storage(SparseStorage(row=None, rowptr=rowptr_out, col=col_out, value=value, sparse_sizes=(n, n),
                                             is_sorted=True, trust_data=True))
        return sub, n_id, e_id, (nodes_per_hop, edges_per_hop)


def neighbor_sample(src: SparseTensor, seeds: torch.Tensor, num_neighbors: Sequence[int], replace: bool = False,
                    directed: bool = True, seed: Optional[int] = None, weighted: Union[bool, EdgeCDF, None] = None
                    ) -> Tuple[SparseTensor, torch.Tensor, torch.Tensor, Tuple[List[int], Optional[List[int]]]]:
    """(sub, n_id, e_id, (nodes_per_hop, edges_per_hop)) — see the module text.  seeds: 1-D,
    any integer dtype, distinct (ValueError) and inside the matrix (IndexError);
    num_neighbors: one fan-out per hop, -1 = every entry, [] = the seeds alone.  To take all
    entries pass -1, not a large k: a hop with k >= 0 is sized by (frontier nodes) * k.
    seed=None draws one from torch's CPU generator, as sample_adj does.  weighted: None, True
    (an EdgeCDF built for this call) or an EdgeCDF of src, as random_walk takes it."""
    return NeighborSampler(src, num_neighbors, replace, directed, weighted)(seeds, seed)


SparseTensor.neighbor_sample = neighbor_sample
