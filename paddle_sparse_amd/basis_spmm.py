"""A relational (RGCN) layer with the basis decomposition W_t = sum_b comp[t, b] * basis[b], as one call whose cost does
not depend on the number of types.

    plan = ps.BasisPlan(adj, edge_type, num_types)             # once per matrix and type assignment
    out = ps.basis_spmm(plan, x, basis, comp)                  # out[i] = sum_e v_e * x[col_e] @ W_(type_e)
    out = ps.basis_spmm(plan, x, basis, comp, reduce="mean")   # PyG RGCNConv(num_bases=B)'s default aggregation

x is [N, K], basis [B, K, F], float32 or bfloat16; comp is float32 [T, B]; `value` is an optional float32 scale per
stored entry, in storage order.  The decomposition commutes with the aggregation:

    out[i] = sum_b Z_b[i] @ basis[b],     Z_b[i] = sum over the entries e of row i of v_e * comp[type_e, b] * x[col_e]

so the kernel (csrc/basis_spmm.hip, MFMA) reads the entries in CSR order, gathers a row of x once per group of
ops.BASIS_SPMM_G bases, sums the rows Z_b of a tile of 64 destination rows in LDS and adds Z_b @ basis[b] into
accumulators that stay in registers.  No [T, K, F] weight and no [nnz, F] message is formed, nothing is sorted by type,
there are no atomics, and two runs give the same bits.  bfloat16 sums in float32 and rounds Z_b once where it becomes
the matrix operand and the result once.

    grad_x     = the same kernel on plan.t() with grad_out as the dense operand and basis[b] read transposed
    grad_basis = sum over the row tiles of Z_b^T @ grad_out[tile rows]                   (ops.basis_spmm_bw_basis)
    grad_comp  = per type, the sum of s[e, b] = v_e * <x[col_e], grad_out[row_e] @ basis[b]^T>
                 (ops.basis_spmm_bw_comp writes s, float32 [nnz, B], the one tensor of nnz rows of the op; the plan's
                 stable by-type order and two passes of ops.segment_csr sum it without atomics)

The work is 2 nnz K B flops on the vector units plus 2 M B K F on MFMA.  With few types and many bases
(B above T) ps.typed_spmm on the expanded weights does less.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .tensor import SparseTensor
from .typed_spmm import _with_zero


_CHUNK = 2048  # entries of one type that one run of the first stage of grad_comp sums


class BasisPlan:
    """The CSR arrays of adj as the kernels read them, in storage order, with one type per entry.  edge_type: int64
    [nnz] in storage order, inside [0, num_types) (IndexRangeError).  Duplicate (row, col) pairs of different types are
    entries of their own.  Nothing is sorted up front; building reads the host once (the range of the types), and so
    does the first use of inv_count, t() and by_type (the fault word of their sort).  Using the plan does not.

    rowptr, col, etype     int64 [M + 1], int32 [nnz], int32 [nnz]
    inv_count              float32 [nnz]  1 / (entries of the same row and type), storage order (lazily)
    by_type, type_ptr      int64 [nnz], int64 [T + 1]: the entries in a stable order by type, for grad_comp (lazily)
    chunk_ptr, type_chunk_ptr  that order cut into runs of at most 2048 entries of one type, and the runs per type
    perm                   None, and for plan.t() int64 [nnz]: its order -> the storage order of adj
    nnz, M, N, T           Python ints"""

    def __init__(self, adj: SparseTensor, edge_type: torch.Tensor, num_types: int):
        if not isinstance(adj, SparseTensor):
            raise TypeError("BasisPlan needs a SparseTensor")
        rowptr, col, _ = adj.csr()
        edge_type = ops._index(edge_type, "edge_type")
        T = int(num_types)
        if T < 1:
            raise ValueError("num_types must be at least 1")
        if edge_type.numel() != col.numel() or edge_type.device != col.device:
            raise ValueError(f"edge_type must hold one type per stored entry ({col.numel()}) on adj's device")
        if col.numel() > 0 and bool((edge_type.min() < 0) | (edge_type.max() >= T)):
            raise ops.IndexRangeError(f"BasisPlan: a type lies outside [0, {T})")
        self._adj, self._edge_type = adj, edge_type
        self._set(rowptr, col, edge_type, adj.sparse_size(0), adj.sparse_size(1), T, None)

    def _set(self, rowptr, col, edge_type, M: int, N: int, T: int, perm: Optional[torch.Tensor]):
        if N >= 2**31 or T >= 2**31:
            raise ValueError("BasisPlan keeps 32-bit columns and types: N and num_types must stay below 2^31")
        self.M, self.N, self.T, self.nnz, self.perm = M, N, T, col.numel(), perm
        self.rowptr, self.col, self.etype = rowptr.contiguous(), col.to(torch.int32), edge_type.to(torch.int32)
        self._t = self._inv_count = self._inv_count_t = None
        self._by_type = self._type_ptr = self._chunk_ptr = self._type_chunk_ptr = None

    def _sorted(self, key: torch.Tensor, bound: int):
        if key.numel() == 0:
            return key, key
        return ops.index_sort(key, max_value=bound, with_sorted_inputs=True, check=True)

    @property
    def inv_count(self) -> torch.Tensor:
        if self._inv_count is None:
            if self._adj is None:
                raise ValueError("inv_count belongs to the plan that t() was called on")
            row, _, _ = self._adj.coo()
            key, perm = self._sorted(row * self.T + self._edge_type, max(self.M * self.T, 1))
            _, run, count = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
            in_storage = torch.empty(self.nnz, dtype=torch.float32, device=key.device)
            in_storage[perm] = (1.0 / count.to(torch.float32))[run]
            self._inv_count = in_storage
        return self._inv_count

    def _order(self):
        if self._by_type is None:
            kind = self.etype.to(torch.int64)
            self._by_type = self._sorted(kind, self.T)[1]
            count = torch.bincount(kind, minlength=self.T)
            self._type_ptr = _with_zero(count)
            # segment_csr gives a run to one wave: the run of a type is cut into chunks of _CHUNK entries, summed first
            per = (count + _CHUNK - 1) // _CHUNK
            self._type_chunk_ptr = _with_zero(per)
            owner = torch.repeat_interleave(torch.arange(self.T, device=kind.device), per)
            nth = torch.arange(owner.numel(), device=kind.device) - self._type_chunk_ptr[owner]
            self._chunk_ptr = torch.cat([self._type_ptr[owner] + nth * _CHUNK, self._type_ptr[-1:]])
        return self._by_type, self._type_ptr

    @property
    def by_type(self) -> torch.Tensor:
        return self._order()[0]

    @property
    def type_ptr(self) -> torch.Tensor:
        return self._order()[1]

    @property
    def chunk_ptr(self) -> torch.Tensor:
        """int64: the by-type order cut into runs of at most 2048 entries of one type.  grad_comp sums the runs first
        and the runs of a type (type_chunk_ptr) second, both in a fixed order."""
        self._order()
        return self._chunk_ptr

    @property
    def type_chunk_ptr(self) -> torch.Tensor:
        """int64 [T + 1]: the runs of chunk_ptr that every type owns."""
        self._order()
        return self._type_chunk_ptr

    def t(self) -> "BasisPlan":
        """The plan of the transposed pattern (lazily, cached): adj's CSC view with the types carried through csr2csc;
        its perm leads to adj's storage order.  The backward wrt x runs on it."""
        if self._t is None:
            if self._adj is None:
                raise ValueError("t() of a transposed plan: keep the plan it came from")
            adj = self._adj
            to_csc = adj.storage.csr2csc()
            colptr, row_csc, _ = adj.csc()
            other = object.__new__(BasisPlan)
            other._adj, other._edge_type = None, None
            other._set(colptr, row_csc, self._edge_type[to_csc], self.N, self.M, self.T, to_csc)
            self._t = other
        return self._t

    def _scale(self, value: Optional[torch.Tensor], mean: bool) -> Optional[torch.Tensor]:
        """The kernel's scale vector in storage order: value (* inv_count)."""
        if mean:
            return self.inv_count if value is None else value * self.inv_count
        return value

    def _scale_t(self, value: Optional[torch.Tensor], mean: bool) -> Optional[torch.Tensor]:
        """The same scales in the order of plan.t(): the mean stays the forward's, per row and type of THIS pattern."""
        other = self.t()
        scale = None if value is None else value[other.perm]
        if mean:
            if self._inv_count_t is None:
                self._inv_count_t = self.inv_count[other.perm]
            scale = self._inv_count_t if scale is None else scale * self._inv_count_t
        return scale


class _BasisSpmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, basis, comp, value, plan, mean: bool):
        scale = plan._scale(value, mean)
        ctx.plan, ctx.mean = plan, mean
        ctx.save_for_backward(x, basis, comp, value, scale)
        return ops.basis_spmm(plan, x, basis, comp, scale)

    @staticmethod
    def backward(ctx, grad_out):
        x, basis, comp, value, scale = ctx.saved_tensors
        plan, g = ctx.plan, grad_out.contiguous()
        grad_x = grad_basis = grad_comp = None
        if ctx.needs_input_grad[0]:
            grad_x = ops.basis_spmm(plan.t(), g, basis, comp, plan._scale_t(value, ctx.mean), trans=True)
        if ctx.needs_input_grad[1]:
            grad_basis = ops.basis_spmm_bw_basis(plan, x, g, comp, scale)
        if ctx.needs_input_grad[2]:
            s = ops.basis_spmm_bw_comp(plan, x, g, basis, scale)
            chunks = ops.segment_csr(s, plan.chunk_ptr, "sum", perm=plan.by_type)
            grad_comp = ops.segment_csr(chunks, plan.type_chunk_ptr, "sum")
        return grad_x, grad_basis, grad_comp, None, None, None


def basis_spmm(plan: BasisPlan, x: torch.Tensor, basis: torch.Tensor, comp: torch.Tensor,
               value: Optional[torch.Tensor] = None, reduce: str = "sum") -> torch.Tensor:
    """out [M, F] with out[i] = sum over the stored entries e = (i, j) of type t of v_e * x[j] @ W_t,
    W_t = sum_b comp[t, b] * basis[b].  x [N, K] and basis [B, K, F] are float32 or bfloat16, comp is float32 [T, B];
    value: float32 [nnz] in storage order or None; reduce: "sum", or "mean" (every entry also scaled by plan.inv_count:
    a mean per relation and destination).  Differentiable in x, basis and comp (a value that requires grad raises
    NotImplementedError).  With a plan whose lazy parts exist there is no host read (capturable); the result is bitwise
    reproducible and no atomics are used."""
    if not isinstance(plan, BasisPlan):
        raise TypeError("basis_spmm needs a BasisPlan")
    if reduce not in ("sum", "mean"):
        raise ValueError(f"reduce must be 'sum' or 'mean' (got {reduce!r})")
    ops._gpu(x, "x")
    ops._gpu(basis, "basis")
    ops._gpu(comp, "comp")
    if x.dim() != 2 or basis.dim() != 3 or basis.shape[1] != x.shape[1]:
        raise ValueError(f"x must be [N, K] and basis [B, K, F] (got {tuple(x.shape)} and {tuple(basis.shape)})")
    if comp.dim() != 2 or comp.shape != (plan.T, basis.shape[0]):
        raise ValueError(f"comp must be [{plan.T}, {basis.shape[0]}] (got {tuple(comp.shape)})")
    if value is not None:
        ops._gpu(value, "value")
        if value.requires_grad:
            raise NotImplementedError("basis_spmm has no gradient wrt value")
        if value.dtype != torch.float32 or value.shape != (plan.nnz,):
            raise ValueError(f"value must be float32 [{plan.nnz}] in storage order")
    return _BasisSpmm.apply(x.contiguous(), basis.contiguous(), comp.contiguous(), value, plan, reduce == "mean")
