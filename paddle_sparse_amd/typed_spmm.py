"""A relational (RGCN-style) layer as one call that forms no message: aggregate first, transform second.

    plan = ps.RelationalPlan(adj, edge_type, num_types)        # once per matrix and type assignment
    out = ps.typed_spmm(plan, x, weight)                       # out[i] = sum_e v_e * x[col_e] @ weight[type_e]
    out = ps.typed_spmm(plan, x, weight, reduce="mean")        # PyG RGCNConv's default: a mean per relation and row

x is [N, K], weight [T, K, F], float32 or bfloat16; `value` is an optional float32 scale per stored entry, in storage
order.  Per tile of 64 destination rows the kernel (csrc/typed_spmm.hip, MFMA) sums H_t = (A_t x)[tile rows] in LDS
and adds H_t @ weight[t] into accumulators that stay in registers: nothing of nnz rows is written, in the forward or
in either gradient, there are no atomics, and two runs give the same bits.  bfloat16 sums in float32, rounds H_t once
to bfloat16 where it becomes the matrix operand and the result once.

    grad_x      = the same kernel on plan.t() with grad_out as the dense operand and weight[t] read transposed
    grad_weight = sum over the tiles of H_t^T @ grad_out[tile rows]              (ops.typed_spmm_bw_weight)

WHEN NOT TO USE IT.  The transform costs S * 64 * K * F multiply-adds, S = plan.segments the number of non-empty
(tile, type) pairs, against nnz * K * F for the message form ps.segment_matmul(x, ptr, W, index=col_by_type) followed
by ops.scatter.  With few types a segment holds many entries and the fused op does about the same work without the
[nnz, F] traffic; when plan.segments approaches plan.nnz (many types, about one entry per segment) it does up to 64
times the flops and loses: prefer the message form there.  The op never switches by itself.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .tensor import SparseTensor


def _with_zero(counts: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=out[1:])
    return out


class RelationalPlan:
    """The stored entries of adj ordered by (tile of 64 rows, type, row), stable (columns keep the storage order), built
    once and held by the user as an EdgeCDF is.  edge_type: int64 [nnz] in storage order, inside [0, num_types)
    (IndexRangeError).  Duplicate (row, col) pairs of different types are entries of their own.  Building reads the
    host (the sort's fault word, the range of the types, three counts); using the plan does not.

    perm          int64 [nnz]   plan order -> storage order of adj (also for plan.t(): adj's order, not its transpose's)
    col, lrow     int32, uint8  column and tile-local row of every entry, plan order
    inv_count     float32 [nnz] 1 / (entries of the same row and type), plan order
    seg_ptr, seg_tile, seg_type the non-empty (tile, type) segments; tile_seg_ptr: the segments of every tile
    by_type, type_seg_ptr       the segments in (type, tile) order; work_ptr, part_ptr: the chunk map of the weight
                                gradient over it (ops.TYPED_SPMM_CS segments per chunk)
    segments, nnz, M, N, T      Python ints; segments / nnz tells the regime (module text)."""

    def __init__(self, adj: SparseTensor, edge_type: torch.Tensor, num_types: int):
        if not isinstance(adj, SparseTensor):
            raise TypeError("RelationalPlan needs a SparseTensor")
        row, col, _ = adj.coo()
        edge_type = ops._index(edge_type, "edge_type")
        T = int(num_types)
        if T < 1:
            raise ValueError("num_types must be at least 1")
        if edge_type.numel() != col.numel() or edge_type.device != col.device:
            raise ValueError(f"edge_type must hold one type per stored entry ({col.numel()}) on adj's device")
        if col.numel() > 0 and bool((edge_type.min() < 0) | (edge_type.max() >= T)):
            raise ops.IndexRangeError(f"RelationalPlan: a type lies outside [0, {T})")
        self._adj, self._edge_type, self._t, self._mean_t = adj, edge_type, None, None
        self._build(row, col, edge_type, adj.sparse_size(0), adj.sparse_size(1), T, None)

    def _build(self, row, col, edge_type, M: int, N: int, T: int, base: Optional[torch.Tensor]):
        BM, CS = ops.TYPED_SPMM_BM, ops.TYPED_SPMM_CS
        dev, nnz, tiles = col.device, col.numel(), -(-M // BM)
        if N >= 2**31 or tiles * T >= 2**31:
            raise ValueError("RelationalPlan keeps 32-bit columns, tiles and types: N and ceil(M / 64) * T must stay "
                             "below 2^31")
        self.M, self.N, self.T, self.nnz = M, N, T, nnz
        if nnz > 0:
            key = ((row // BM) * T + edge_type) * BM + row % BM
            key, perm = ops.index_sort(key, max_value=tiles * T * BM, with_sorted_inputs=True, check=True)
        else:
            key = perm = torch.empty(0, dtype=torch.int64, device=dev)
        self.perm = perm if base is None else base[perm]
        self.col = col[perm].to(torch.int32)
        self.lrow = (key % BM).to(torch.uint8)
        _, run, count = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
        self.inv_count = (1.0 / count.to(torch.float32))[run]
        seg, seg_len = torch.unique_consecutive(key // BM, return_counts=True)
        self.segments = seg.numel()
        self.seg_ptr = _with_zero(seg_len)
        tile, kind = seg // T, seg % T
        self.seg_tile, self.seg_type = tile.to(torch.int32), kind.to(torch.int32)
        self.tile_seg_ptr = torch.searchsorted(tile, torch.arange(tiles + 1, device=dev))
        self.by_type = torch.sort(kind, stable=True)[1]
        per_type = torch.bincount(kind, minlength=T)
        self.type_seg_ptr = _with_zero(per_type)
        chunks = ((per_type + CS - 1) // CS).clamp_(min=1)  # a type without entries keeps one item: it writes zeros
        self.work_ptr = _with_zero(chunks)
        self.part_ptr = _with_zero(torch.where(chunks > 1, chunks, torch.zeros_like(chunks)))
        self.items, self.partial_chunks = int(self.work_ptr[-1]), int(self.part_ptr[-1])

    def t(self) -> "RelationalPlan":
        """The plan of the transposed pattern (lazily, cached), from adj's CSC view with the types carried through
        csr2csc; its perm leads to adj's storage order.  The backward wrt x runs on it."""
        if self._t is None:
            adj = self._adj
            to_csc = adj.storage.csr2csc()
            _, row_csc, _ = adj.csc()
            other = object.__new__(RelationalPlan)
            other._adj, other._edge_type, other._t, other._mean_t = None, None, self, None
            other._build(adj.storage.col()[to_csc], row_csc, self._edge_type[to_csc], self.N, self.M, self.T, to_csc)
            self._t = other
        return self._t

    def _scale(self, value: Optional[torch.Tensor], mean: bool) -> Optional[torch.Tensor]:
        """The kernel's scale vector in plan order: value[perm] (* inv_count), one elementwise pass."""
        scale = None if value is None else value[self.perm]
        if mean:
            scale = self.inv_count if scale is None else scale * self.inv_count
        return scale

    def _scale_t(self, value: Optional[torch.Tensor], mean: bool) -> Optional[torch.Tensor]:
        """The same scales in the order of plan.t(): the mean stays the forward's, per row and type of THIS pattern."""
        other = self.t()
        scale = None if value is None else value[other.perm]
        if mean:
            if self._mean_t is None:
                in_storage = torch.empty_like(self.inv_count)
                in_storage[self.perm] = self.inv_count
                self._mean_t = in_storage[other.perm]
            scale = self._mean_t if scale is None else scale * self._mean_t
        return scale


class _TypedSpmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, value, plan, mean: bool):
        scale = plan._scale(value, mean)
        ctx.plan, ctx.mean = plan, mean
        ctx.save_for_backward(x, weight, value, scale)
        return ops.typed_spmm(plan, x, weight, scale)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, value, scale = ctx.saved_tensors
        plan, g = ctx.plan, grad_out.contiguous()
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            grad_x = ops.typed_spmm(plan.t(), g, weight, plan._scale_t(value, ctx.mean), trans_w=True)
        if ctx.needs_input_grad[1]:
            grad_w = ops.typed_spmm_bw_weight(plan, x, g, scale)
        return grad_x, grad_w, None, None, None


def typed_spmm(plan: RelationalPlan, x: torch.Tensor, weight: torch.Tensor, value: Optional[torch.Tensor] = None,
               reduce: str = "sum") -> torch.Tensor:
    """out [M, F] with out[i] = sum over the stored entries e = (i, j) of type t of v_e * x[j] @ weight[t].  x [N, K] and
    weight [T, K, F] are float32 or bfloat16; value: float32 [nnz] in storage order or None; reduce: "sum", or "mean"
    (every entry also scaled by plan.inv_count: a mean per relation and destination).  Differentiable in x and weight
    (a value that requires grad raises NotImplementedError).  No tensor of nnz rows is formed; with a prebuilt plan
    there is no host read (capturable) and the result is bitwise reproducible.  See the module text for the regime in
    which ps.segment_matmul + ops.scatter is the better route (plan.segments close to plan.nnz)."""
    if not isinstance(plan, RelationalPlan):
        raise TypeError("typed_spmm needs a RelationalPlan")
    if reduce not in ("sum", "mean"):
        raise ValueError(f"reduce must be 'sum' or 'mean' (got {reduce!r})")
    ops._gpu(x, "x")
    ops._gpu(weight, "weight")
    if x.dim() != 2 or weight.dim() != 3 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"x must be [N, K] and weight [T, K, F] (got {tuple(x.shape)} and {tuple(weight.shape)})")
    if value is not None:
        ops._gpu(value, "value")
        if value.requires_grad:
            raise NotImplementedError("typed_spmm has no gradient wrt value")
        if value.dtype != torch.float32 or value.shape != (plan.nnz,):
            raise ValueError(f"value must be float32 [{plan.nnz}] in storage order")
    return _TypedSpmm.apply(x.contiguous(), weight.contiguous(), value, plan, reduce == "mean")
