"""temporal_neighbor_sample — per-seed neighbour sampling under a time bound (torch_sparse's
hetero_temporal_neighbor_sample on one node type, the op behind PyG's
NeighborLoader(time_attr=...)), on the HIP kernels of csrc/temporal.hip.

    order = EdgeTimeOrder(adj, edge_time=t)       # once per matrix
    sub, n_id, e_id, ptr, root = adj.temporal_neighbor_sample(seeds, seed_time, [10, 5], time=order)
    h = gnn(sub, x[n_id])
    out = h[root]                                 # one row per seed

Every position of `seeds` is an ego of its own with the bound T_g = seed_time[g], and nothing
ego g receives is newer than T_g: no entry of the seed's future reaches the model.

Time.  time_of(e) is edge_time[e] (e = storage position, CSR order), or node_time[col[e]] in
node mode.  An EdgeTimeOrder holds, inside every row, the storage positions ascending by
(time_of(e), e) (`order`) and their times (`sorted_time`).  The entries of a row are stored by
column, so the eligible ones are scattered over it; in the index they are a prefix, found by
one upper-bound search, where a scan would cost the degree of every hub a walk reaches, per
parent and hop.

Walk list.  Identical to ego_k_hop_sample: entries 0 .. S-1 are the seeds, entry i belongs to
ego i, hop l expands every entry of hop l - 1, duplicates are kept, a child belongs to its
parent's ego, and every entry of ego g carries T_g for the whole tree.

Eligible set.  A parent holding node v in ego g has E(v, T_g): the entries of row v with
time_of(e) <= T_g, listed by (time, storage position) ascending.  c = |E|.  In node mode the
seed's own time is not checked.

Picks.  The parent at walk index i draws on stream i of `seed`; the result is ranks into E.
    k < 0                                 all c ranks, ascending
    "uniform", replace=True               rank randint(seed, i, t, c) for t < k; none if c == 0
    "uniform", replace=False, c <= k      all c ranks, ascending
    "uniform", replace=False, c > k       the exact Floyd walk: for t = 0 .. k-1, j = c - k + t,
                                          r = randint(seed, i, t, j + 1), pick j if r was
                                          picked before, else r
    "last"                                ranks c-1, c-2, ..., c-min(k, c): the most recent
                                          entries, ties going to the larger storage position
The Floyd walk draws in [0, j], which makes every k-subset equally likely.  sample_adj,
neighbor_sample and ego_k_hop_sample draw in [0, j) as upstream does, a rule that
under-samples the last k ranks; on a time-ordered list those are the freshest entries.

Slots.  For k >= 0 hop l has F * k slots, known without a read; the slots past a parent's
picks are empty and stay empty.  For k < 0 the hop has the sum of the c: one count launch,
one scan and one host read.  k == 0 ends the sampling, [] makes each ego its seed alone.

Result.  n_id, ptr and root are ego_k_hop_sample's: the distinct (ego, node) of the
non-empty walk entries, ascending node id inside an ego.  sub is the [n, n] block-diagonal
matrix of the SAMPLED entries (not the induced ones, which may lie in the future): one entry
per distinct (g, e) emitted by any slot, at row ptr[g] + rank of e's row and column ptr[g] +
rank of col[e] in ego g's node set.  The entries are ordered by (g, e); rows are column-sorted
and local ids ascend with the node id, so this is (row', col') order with stored duplicates
in storage order.  e_id is e, the values are value[e_id], differentiable with a
deterministic backward (one edge may sit in several egos).  Every entry of ego g satisfies
time_of(e_id) <= seed_time[g].  adj and its caches are not modified.

Limits: those of ego_k_hop_sample and S * nnz < 2^62, each a ValueError.  The result is a
function of (seed, inputs) only.  Not capturable in a graph: the sizes depend on the data.
Host reads per call: one per hop run with k < 0, one for n, one for nnz' and the flags.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .saint import _SaintValue
from .storage import SparseStorage
from .tensor import SparseTensor


def _integer(x, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.is_floating_point() or x.is_complex() or x.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor")
    if x.dim() != 1:
        raise ValueError(f"{name} must be 1-D")
    return x


class EdgeTimeOrder:
    """The time order of adj's entries inside every row, built once and held by the user as an
    EdgeCDF is: order (int64[nnz]) and sorted_time (int64[nnz]), see the module text.

    Exactly one of edge_time (integer tensor [nnz], in storage order) and node_time (integer
    tensor [N]; an entry has the time of its column) must be given, else TypeError; a float or
    bool tensor is a TypeError, a wrong length a ValueError.  Times may be negative; max - min
    must stay below 2^62 (ValueError).  One host read finds min and max, the two sorts' fault
    words are read as well.  The object remembers the rowptr it was built from and serves that
    matrix only; adj and its caches are not modified."""

    def __init__(self, adj: SparseTensor, edge_time: Optional[torch.Tensor] = None,
                 node_time: Optional[torch.Tensor] = None):
        if not isinstance(adj, SparseTensor):
            raise TypeError("EdgeTimeOrder needs a SparseTensor")
        if (edge_time is None) == (node_time is None):
            raise TypeError("EdgeTimeOrder needs exactly one of edge_time and node_time")
        rowptr, col, _ = adj.csr()
        nnz = col.numel()
        if edge_time is not None:
            time = _integer(edge_time, "edge_time")
            if time.numel() != nnz:
                raise ValueError(f"edge_time must hold one time per entry ({nnz}), got {time.numel()}")
            time = time.to(device=col.device, dtype=torch.int64).contiguous()
        else:
            node_time = _integer(node_time, "node_time")
            if node_time.numel() != adj.sparse_size(1):
                raise ValueError(f"node_time must hold one time per column ({adj.sparse_size(1)}), "
                                 f"got {node_time.numel()}")
            node_time = node_time.to(device=col.device, dtype=torch.int64).contiguous()
            time = ops._gather_rows_raw(node_time, col) if nnz > 0 else node_time[:0]
        lo, hi = torch.stack(torch.aminmax(time)).tolist() if nnz > 0 else (0, 0)  # the one read of min and max
        if hi - lo >= 2**62:
            raise ValueError(f"EdgeTimeOrder: the times span {hi - lo}, the limit is 2^62 - 1")
        self.rowptr = rowptr
        self.min_time, self.max_time = lo, hi
        self.order, self.sorted_time = ops.edge_time_order(rowptr, time, lo, hi)

    def order_for(self, src: SparseTensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(order, sorted_time), after checking that src is the matrix this object was built from."""
        rowptr = src.storage.rowptr()
        if rowptr is not self.rowptr and (rowptr.data_ptr() != self.rowptr.data_ptr()
                                          or rowptr.numel() != self.rowptr.numel()):
            raise ValueError("this EdgeTimeOrder was built from another matrix")
        return self.order, self.sorted_time


def temporal_neighbor_sample(src: SparseTensor, seeds: torch.Tensor, seed_time: torch.Tensor,
                             num_neighbors: Sequence[int], time: Optional[EdgeTimeOrder] = None,
                             strategy: str = "uniform", replace: bool = False, seed: Optional[int] = None
                             ) -> Tuple[SparseTensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sub, n_id, e_id, ptr, root) — see the module text.  seeds: 1-D, any integer dtype, inside
    the matrix (IndexError), duplicates allowed; seed_time: one integer bound per seed
    (ValueError for another length); num_neighbors: one fan-out per hop, -1 = every eligible
    entry, 0 ends the sampling, [] = each ego is its seed alone; time: the EdgeTimeOrder of src;
    strategy: "uniform" or "last" ("last" with replace=True is a ValueError).  seed=None draws
    one from torch's CPU generator, as sample_adj does."""
    if not src.is_quadratic():
        raise ValueError(f"temporal_neighbor_sample needs a square matrix (got {src.sparse_sizes()})")
    if isinstance(num_neighbors, (str, bytes)) or not isinstance(num_neighbors, (list, tuple)) \
            or any(isinstance(k, bool) or not isinstance(k, int) for k in num_neighbors):
        raise TypeError("num_neighbors must be a list of ints")
    if any(k < -1 for k in num_neighbors):
        raise ValueError(f"num_neighbors must be >= -1 (got {list(num_neighbors)})")
    if not isinstance(time, EdgeTimeOrder):
        raise TypeError("time must be the EdgeTimeOrder of the matrix")
    if strategy not in ops.TEMPORAL_STRATEGY:
        raise ValueError(f"strategy must be 'uniform' or 'last' (got {strategy!r})")
    if strategy == "last" and replace:
        raise ValueError("strategy='last' takes the most recent entries: it has no draws to replace")
    seeds, seed_time = _integer(seeds, "seeds"), _integer(seed_time, "seed_time")
    if seed_time.numel() != seeds.numel():
        raise ValueError(f"seed_time must hold one bound per seed ({seeds.numel()}), got {seed_time.numel()}")
    order, sorted_time = time.order_for(src)
    rowptr, col, value = src.csr()
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    n_id, ptr, root, rowptr_out, col_out, e_id = ops.temporal_neighbor_sample(
        rowptr, col, order, sorted_time, seeds.to(torch.int64).contiguous(),
        seed_time.to(device=seeds.device, dtype=torch.int64).contiguous(), list(num_neighbors), strategy,
        bool(replace), seed)
    if value is not None:
        if ops.needs_grad(value):
            value = _SaintValue.apply(value, e_id, True)  # an edge may sit in several egos: sort + segment sum
        else:
            value = ops._gather_rows_raw(value, e_id)
    n = n_id.numel()
    sub = src.from_storage(SparseStorage(row=None, rowptr=rowptr_out, col=col_out, value=value, sparse_sizes=(n, n),
                                         is_sorted=True, trust_data=True))
    return sub, n_id, e_id, ptr, root


SparseTensor.temporal_neighbor_sample = temporal_neighbor_sample
