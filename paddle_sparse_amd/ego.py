"""ego_k_hop_sample — torch_sparse's ego_k_hop_sample_adj (the op behind PyG's
ShaDowKHopSampler), on the HIP kernels of csrc/ego.hip.

    sub, n_id, e_id, ptr, root = adj.ego_k_hop_sample(seeds, [10, 5])
    h = deep_gnn(sub, x[n_id])      # any depth: it runs on the ego nets, not on adj
    out = h[root]                   # one row per seed

Every position of `seeds` gets a k-hop neighbourhood of its own (duplicate seeds are egos of
their own), and what comes back is the subgraph induced on each neighbourhood, all S of them
as one block-diagonal matrix.

Walk list.  There is one global sequence of walk entries.  Entries 0 .. S-1 are the seeds and
entry i belongs to ego i.  Hop l expands every entry of hop l - 1; duplicates are kept
(upstream's rule: a node reached twice is expanded twice), and a child belongs to its
parent's ego.

Picks.  A parent at walk index i that holds node v makes sample_adj's picks for (deg(v), k_l,
replace) on stream i of `seed`: all entries when k_l < 0 or not replace and deg <= k_l;
randint(seed, i, t, deg) with replacement; otherwise Floyd's walk.

Numbering.  For k_l >= 0 hop l has exactly F_{l-1} * k_l slots and slot base_l + f * k_l + t
belongs to parent f and pick t.  A slot past its parent's pick count, or a slot of an empty
parent, is empty: it keeps its index, stays empty in later hops and contributes nothing, so
the host knows the numbering without a read.  For k_l < 0 the hop has the sum of the parents'
degrees as slots, all valid, in (parent, storage) order: one degree count, one scan and one
host read of the total.  k_l == 0 ends the sampling.  Hop 1 of ego i is thus exactly
sample_adj(seeds, k_1, replace, seed)'s picks for row i.

Node set.  Ego g's nodes are the distinct nodes of its non-empty walk entries in ascending
node id; n_id is the concatenation over the egos, ptr is int64[S+1] with ptr[g+1] - ptr[g] =
n_g, root[g] is the position in n_id of (g, seeds[g]); local id = position in n_id.

Subgraph.  sub is the [n, n] block-diagonal matrix: local row r (ego g, node v) holds every
stored entry (v, c) of adj with c in ego g's node set, at column ptr[g] + rank of c in the
set, stored duplicates kept in storage order.  adj's rows are column-sorted and local ids
ascend with the node id, so the entries are sorted by (row', col') as they are written; no
sort runs over them.  e_id is the storage position of every kept entry and the values are
value[e_id], differentiable with a deterministic backward (one edge may sit in several
egos: the gradient rows are summed in a fixed order).  adj and its caches are not modified.

Limits: S * N < 2^62, every hop below 2^31 - 16 slots and the walk list below 2^31 entries
(which bounds n); each is a ValueError, raised before anything is allocated where the
fan-outs alone decide it.  To take all entries pass -1, not a large k.  The result is a
function of (seed, inputs) only.  Not capturable in a graph: the sizes depend on the data.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .saint import _SaintValue
from .storage import SparseStorage
from .tensor import SparseTensor


def ego_k_hop_sample(src: SparseTensor, seeds: torch.Tensor, num_neighbors: Sequence[int], replace: bool = False,
                     seed: Optional[int] = None
                     ) -> Tuple[SparseTensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sub, n_id, e_id, ptr, root) — see the module text.  seeds: 1-D, any integer dtype, inside
    the matrix (IndexError), duplicates allowed; num_neighbors: one fan-out per hop, -1 = every
    entry, [] = each ego is its seed alone.  seed=None draws one from torch's CPU generator, as
    sample_adj does."""
    if not src.is_quadratic():
        raise ValueError(f"ego_k_hop_sample needs a square matrix (got {src.sparse_sizes()})")
    if isinstance(num_neighbors, (str, bytes)) or not isinstance(num_neighbors, (list, tuple)) \
            or any(isinstance(k, bool) or not isinstance(k, int) for k in num_neighbors):
        raise TypeError("num_neighbors must be a list of ints")
    if any(k < -1 for k in num_neighbors):
        raise ValueError(f"num_neighbors must be >= -1 (got {list(num_neighbors)})")
    if not isinstance(seeds, torch.Tensor) or seeds.is_floating_point() or seeds.is_complex() \
            or seeds.dtype == torch.bool:
        raise TypeError("seeds must be an integer tensor")
    if seeds.dim() != 1:
        raise ValueError("seeds must be 1-D")
    rowptr, col, value = src.csr()
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    n_id, ptr, root, rowptr_out, col_out, e_id = ops.ego_k_hop_sample(
        rowptr, col, seeds.to(torch.int64).contiguous(), list(num_neighbors), bool(replace), seed)
    if value is not None:
        if ops.needs_grad(value):
            value = _SaintValue.apply(value, e_id, True)  # an edge may sit in several egos: sort + segment sum
        else:
            value = ops._gather_rows_raw(value, e_id)
    n = n_id.numel()
    sub = src.from_storage(SparseStorage(row=None, rowptr=rowptr_out, col=col_out, value=value, sparse_sizes=(n, n),
                                         is_sorted=True, trust_data=True))
    return sub, n_id, e_id, ptr, root


SparseTensor.ego_k_hop_sample = ego_k_hop_sample
