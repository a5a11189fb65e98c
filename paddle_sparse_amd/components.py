"""connected_components, largest_connected_components — which nodes of a graph hang together,
on the kernels of csrc/components.hip.

    n, labels = adj.connected_components()                  # labels[i]: the component of node i
    sub, n_id, e_id = adj.largest_connected_components()    # the subgraph of the largest one

Components are weak: every stored entry (u, v) joins u and v, whatever its direction or value
(an explicit zero is still an edge).  The usual route copies the index to the host for
scipy.sparse.csgraph.connected_components and the labels back; here a lock-free union-find
runs over the stored entries in three launches whose number depends on neither the diameter nor
the data (csrc/union_find.h).  The root of a component is its smallest node under
any schedule, so the labels are the same bits on every run, and they are scipy's for
`directed=True, connection="weak"`: component k is the one with the k-th smallest minimum.

Limits: weak connectivity only; one device-to-host read per connected_components call, so it
is not capturable in a graph.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import ops
from .saint import saint_subgraph
from .tensor import SparseTensor


def _host_read(t: torch.Tensor) -> list:
    """The one device-to-host read of connected_components: (number of components, flags)."""
    return t.tolist()


def _square(who: str, adj) -> SparseTensor:
    if not isinstance(adj, SparseTensor):
        raise TypeError(f"{who}: adj must be a SparseTensor")
    if not adj.is_quadratic():
        raise ValueError(f"{who} needs a square matrix (got {adj.sparse_sizes()})")
    return adj


def connected_components(adj: SparseTensor, connection: str = "weak") -> Tuple[int, torch.Tensor]:
    """(n, labels int64[N] on adj's device): the number of weakly connected components and, for
    every node i, labels[i] = the number of components whose smallest node id is below the
    smallest node id of i's component.  Self loops and duplicated entries are harmless and the
    columns of a row need no order.  connection="strong" raises NotImplementedError; a column id
    outside [0, N) raises IndexError (the kernel skips such an entry).  Not capturable in a
    graph: n is a Python int, which costs the call its one host read."""
    adj = _square("connected_components", adj)
    if connection == "strong":
        raise NotImplementedError("connected_components: strong connectivity is not implemented (weak only)")
    if connection != "weak":
        raise ValueError(f"connected_components: connection must be 'weak' (got {connection!r})")
    N = adj.size(0)
    rowptr, col, _ = adj.csr()
    if N == 0:
        return 0, torch.empty(0, dtype=torch.int64, device=col.device)
    parent = ops.components_init(rowptr, col)
    flags = ops.components_hook(adj.storage.row(), col, parent)
    root, is_root = ops.components_flatten(parent)
    rank = ops.count2ptr(is_root)
    labels = ops._gather_rows_raw(rank, root)
    n, flag_bits = _host_read(torch.cat([rank[N:], flags]))
    if flag_bits & ops.COMPONENTS_RANGE:
        raise IndexError(f"connected_components: a stored column lies outside [0, {N})")
    return int(n), labels


def _nodes_of_largest(sizes: torch.Tensor, labels: torch.Tensor, num_components: int) -> torch.Tensor:
    """The ascending nodes whose label is among the num_components largest entries of sizes; a stable
    descending sort, so of two components of one size the smaller label comes first."""
    keep = torch.sort(sizes, descending=True, stable=True).indices[:num_components]
    kept = torch.zeros(sizes.numel(), dtype=torch.bool, device=labels.device)
    kept[keep] = True
    return kept[labels].nonzero().view(-1)


def largest_connected_components(adj: SparseTensor, num_components: int = 1
                                 ) -> Tuple[SparseTensor, torch.Tensor, torch.Tensor]:
    """(sub, n_id, e_id): the subgraph induced by the nodes of the num_components largest
    components (a tie in size goes to the smaller label), n_id int64 ascending the nodes kept and
    (sub, e_id) = adj.saint_subgraph(n_id), so e_id holds the storage position of every kept
    entry.  With num_components at least the number of components the whole graph is returned.
    num_components < 1 raises ValueError; the other errors are those of connected_components.
    Not capturable in a graph."""
    adj = _square("largest_connected_components", adj)
    num_components = int(num_components)
    if num_components < 1:
        raise ValueError(f"largest_connected_components: num_components must be >= 1 (got {num_components})")
    n, labels = connected_components(adj)
    if adj.size(0) == 0:  # no node to select: the empty graph is its own answer
        return adj, labels, labels.clone()
    if num_components >= n:
        n_id = torch.arange(adj.size(0), dtype=torch.int64, device=labels.device)
    else:
        n_id = _nodes_of_largest(ops.bincount(labels, n), labels, num_components)
    sub, e_id = saint_subgraph(adj, n_id)
    return sub, n_id, e_id


SparseTensor.connected_components = connected_components
SparseTensor.largest_connected_components = largest_connected_components
