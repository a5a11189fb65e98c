"""ppr — approximate personalised PageRank rows by the Andersen-Chung-Lang forward push, on the
kernels of csrc/ppr.hip.

    ppr = adj.ppr(source, alpha=0.15, eps=1e-4)            # SparseTensor [S, N], row i belongs to source[i]
    ppr, res = adj.ppr(source, 0.15, 1e-4, return_residual=True)
    gdc = adj.ppr(torch.arange(N, device="cuda"), 0.15, 1e-4).topk(64, dim=0)   # GDC's diffusion, sparsified

The primitive of PPRGo / APPNP precomputation, of GDC's PPR kernel, of ShaDow's PPR sampler and of
PPR node-similarity features; upstream it is a numba loop on the CPU (torch_geometric.utils.ppr.get_ppr).
Only the pattern of adj is read (stored values are ignored, a duplicated entry counts twice, a node
without entries keeps what reaches it).  The push runs in fixed point: a unit of mass is 2^48, alpha is
rounded to a multiple of 2^-32 and eps to a multiple of 2^-48, every update is an integer add, and so the
result is the same bits on every run and equals a serial restatement of the rule (include/
paddle_sparse_hip.h states it).  p + r @ Pi = Pi[source] holds to the flooring of the pushes,
with Pi the exact PPR matrix of the rounded alpha.

One workgroup runs one source from start to finish in a hash table of `cap` slots, in LDS when
cap <= 4096 and in global memory otherwise.  Sources run in batches of `concurrent` tables.

Limits: unweighted transition probabilities only (edge weights would have to be integers); not
differentiable; no CPU path; not capturable in a graph (one host read for the source range, one per
batch for its counts and flags, and the 4-byte fault word of each batch's sort).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .storage import SparseStorage
from .tensor import SparseTensor

_BUDGET = 1 << 30  # bytes of tables in flight; a first value, not swept
_SLOT_BYTES = 32   # key, r, p, s


def _host_read(t: torch.Tensor) -> list:
    """The device-to-host reads of this module: the source range once, a batch's info once."""
    return t.tolist()


def quantise(alpha: float, eps: float):
    """(alpha_q, eps_q) = (round(alpha * 2^32), round(eps * 2^48)), ValueError outside
    [2^-16, 1 - 2^-16] and [2^-32, 1]: the ranges in which every push makes progress."""
    alpha, eps = float(alpha), float(eps)
    if not 2.0 ** -16 <= alpha <= 1 - 2.0 ** -16:
        raise ValueError(f"ppr: alpha must lie in [2^-16, 1 - 2^-16] (got {alpha})")
    if not 2.0 ** -32 <= eps <= 1:
        raise ValueError(f"ppr: eps must lie in [2^-32, 1] (got {eps})")
    return int(alpha * 2.0 ** 32 + 0.5), int(eps * 2.0 ** 48 + 0.5)  # both products are exact doubles


def work_bound(alpha_q: int, eps_q: int) -> int:
    """The most the degrees of all pushes of one source can add up to (csrc/ppr_step.h)."""
    return ops.PPR_ONE // ((alpha_q * eps_q) >> 32)


def table_cap(N: int, alpha_q: int, eps_q: int) -> int:
    """The power of two >= 2 * min(N, 1 + work_bound): a table that cannot fill."""
    need = 2 * min(N, 1 + work_bound(alpha_q, eps_q))
    return 1 << max(need - 1, 0).bit_length()


def _rows(tables, which: int, info_host, field: int, counts: torch.Tensor, nb: int, cap: int, N: int, first: int,
          dtype, stats):
    """(row, col, value) of one batch, sorted by (row, col): write, sort the keys, split, gather."""
    total = sum(info_host[field])
    key, val = ops.ppr_write(tables[0], tables[which], nb, cap, N, ops.count2ptr(counts), total)
    key, perm = ops.index_sort(key, max_value=nb * N, with_sorted_inputs=True, check=True)
    stats["host_reads"] += 1
    slot, node = ops.split_keys(key, N)
    val = ops._gather_rows_raw(val, perm)
    return slot + first, node, val if dtype == torch.float64 else val.to(dtype)


def _assemble(parts, S: int, N: int, rowcount: torch.Tensor) -> SparseTensor:
    row, col, val = (torch.cat(x) for x in zip(*parts))
    return SparseTensor.from_storage(SparseStorage(row=row, col=col, value=val, sparse_sizes=(S, N), rowcount=rowcount,
                                                   is_sorted=True, trust_data=True))


def ppr(adj: SparseTensor, source: torch.Tensor, alpha: float = 0.15, eps: float = 1e-4, *,
        return_residual: bool = False, dtype: torch.dtype = torch.float32, max_rounds: Optional[int] = None,
        concurrent: Optional[int] = None, stats: Optional[dict] = None):
    """The SparseTensor [S, N] whose row i holds the approximate personalised PageRank of source[i]
    (int64[S] on adj's device, repeats allowed and giving equal rows): the nodes with p > 0, columns
    ascending, values p / 2^48 in `dtype` (float32 or float64, rounded once from the exact double).
    A node u stops being pushed once r[u] < eps * max(deg(u), 1); a source below its own threshold
    gives an empty row.  return_residual=True also returns the residuals r > 0 in the same form.
    max_rounds=None runs every source to its end (the work is bounded by 2^48 // ((alpha_q * eps_q)
    >> 32) pushed entries); an int stops after that many rounds and returns the state as it stands.
    concurrent is the number of sources in flight (default: what 1 GiB of tables holds; not swept).
    stats, when a dict, receives per-source tensors `rounds`, `pushes`, `edges`, `touched`, `in_lds`
    and the ints `cap`, `batches`, `host_reads`.
    ValueError: alpha outside [2^-16, 1 - 2^-16], eps outside [2^-32, 1], a source that is not int64
    or lies outside [0, N), S * N >= 2^62, a matrix that is not square."""
    if not isinstance(adj, SparseTensor):
        raise TypeError("ppr: adj must be a SparseTensor")
    if not adj.is_quadratic():
        raise ValueError(f"ppr needs a square matrix (got {adj.sparse_sizes()})")
    alpha_q, eps_q = quantise(alpha, eps)
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"ppr: dtype must be float32 or float64 (got {dtype})")
    if not isinstance(source, torch.Tensor) or source.dtype != torch.int64 or source.dim() != 1:
        raise ValueError("ppr: source must be a 1-D int64 tensor")
    if max_rounds is not None and (not isinstance(max_rounds, int) or max_rounds < 0):
        raise ValueError("ppr: max_rounds must be None or an int >= 0")
    if concurrent is not None and (not isinstance(concurrent, int) or concurrent < 1):
        raise ValueError("ppr: concurrent must be None or an int >= 1")
    N, S = adj.size(0), source.numel()
    if S * N >= 2 ** 62:
        raise ValueError(f"ppr: S * N = {S * N} does not fit the 62-bit sort key")
    rowptr, col, _ = adj.csr()
    source = ops._index(source, "source")
    stats = {} if stats is None else stats
    stats.update(host_reads=0, batches=0, cap=0)
    if S:
        lo, hi = _host_read(torch.stack(torch.aminmax(source)))
        stats["host_reads"] += 1
        if lo < 0 or hi >= N:
            raise ValueError(f"ppr: a source lies outside [0, {N})")
    dev = col.device
    cap = stats["cap"] = table_cap(N, alpha_q, eps_q)
    rounds = work_bound(alpha_q, eps_q) + 1 if max_rounds is None else max_rounds
    B = max(1, min(S, concurrent or max(1, _BUDGET // (_SLOT_BYTES * cap))))
    tables = ops.ppr_tables(B, cap, dev) if S else None
    infos, p_parts, r_parts = [], [], []
    for first in range(0, S, B):
        nb = min(B, S - first)
        _, info = ops.ppr_push(rowptr, col, N, source[first:first + nb], cap, alpha_q, eps_q, rounds, tables)
        host = _host_read(info)
        stats["host_reads"] += 1
        stats["batches"] += 1
        flags = 0
        for f in host[3]:
            flags |= f
        if flags & ops.PPR_BAD_INDEX:
            raise IndexError(f"ppr: a stored column or a row bound lies outside the {N} x {N} matrix")
        if flags & ops.PPR_TABLE_FULL:
            raise RuntimeError(f"ppr: a table of {cap} slots filled up")
        infos.append(info)
        p_parts.append(_rows(tables, 2, host, 0, info[0], nb, cap, N, first, dtype, stats))
        if return_residual:
            r_parts.append(_rows(tables, 1, host, 1, info[1], nb, cap, N, first, dtype, stats))
    if not S:
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        value = torch.empty(0, dtype=dtype, device=dev)
        p_parts = r_parts = [(empty, empty, value)]
        infos = [torch.zeros((8, 0), dtype=torch.int64, device=dev)]
    info = torch.cat(infos, dim=1)
    stats.update(rounds=info[2], pushes=info[4], edges=info[5], touched=info[6],
                 in_lds=(info[3] & ops.PPR_IN_LDS) != 0)
    out = _assemble(p_parts, S, N, info[0].contiguous())
    return (out, _assemble(r_parts, S, N, info[1].contiguous())) if return_residual else out


SparseTensor.ppr = ppr
