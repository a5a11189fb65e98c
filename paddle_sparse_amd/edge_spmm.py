"""SpMM over per-entry feature vectors on the SparseTensor surface: `edge_spmm`, the aggregation of the
message-passing layers that carry edge features.

    out = adj.edge_spmm(x, edge, op="mul", reduce="sum")       # [M, K]
    m[e]   = x[col(e)] * edge[e]  |  x[col(e)] + edge[e]  |  relu(x[col(e)] + edge[e])      op = mul | add | add_relu
    out[r] = sum of m[e] over the entries of row r             (mean: over their number; a row without entries is 0)

op="mul" is SchNet's CFConv, the MPNN family and CGConv (DGL's u_mul_e_sum), "add" is u_add_e_sum and "add_relu" is
GINE.  The forward is one HIP launch family (psa_edge_spmm, csrc/edge_spmm.hip) that reads the [nnz, K] edge operand
once beside the gather of `x`; nothing of nnz rows is written or kept for the backward.  With g = grad_out (over n
for mean),

    grad_edge[e] = g[row(e)] * x[col(e)]  |  g[row(e)]  |  g[row(e)] * [x[col(e)] + edge[e] > 0]
    grad_x[j]    = sum over the entries of column j of   g[row(e)] * edge[e]  |  g[row(e)]  |  g[row(e)] * [...]

grad_edge is entry-parallel (psa_edge_spmm_bw_edge), grad_x one pass over the CSC view (psa_edge_spmm_bw_x) that
forms the mask of add_relu again from `x` and `edge`; for op="add" it is A^T g, the planned transposed SpMM the
package has.  float32 or bfloat16; bfloat16 forms every message and sum in float32 and rounds once per result.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .matmul import spmm_transposed_planned
from .storage import SparseStorage
from .tensor import SparseTensor


class _EdgeSpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, edge: torch.Tensor, storage: SparseStorage, op: str, mean: bool, track: bool):
        out = ops.edge_spmm(storage.rowptr(), storage.col(), x, edge, op, mean,
                            no_long_rows=storage._longest_row() <= ops.LONG_ROW)
        if track and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            ctx.storage, ctx.op, ctx.mean = storage, op, mean
            ctx.save_for_backward(x, edge)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        x, edge = ctx.saved_tensors
        st, op, mean = ctx.storage, ctx.op, ctx.mean
        g = grad_out.contiguous()
        scale = None
        if mean:  # 1 / float(n) of every row of grad_out; a row without entries has no entry that reads it
            scale = 1.0 / st.rowcount().clamp(min=1).to(torch.float32)
        grad_x = grad_edge = None
        if ctx.needs_input_grad[1]:
            grad_edge = ops.edge_spmm_bw_edge(st.row(), st.col(), g, x, edge, op, scale)
        if ctx.needs_input_grad[0] and op == "add":
            # A^T g: the planned forward over the CSC view.  Its half-width form takes K % 8 == 0; other widths sum
            # the widened g in float32 and are rounded once here
            if g.dtype == torch.float32 or g.shape[1] % 8 == 0:
                grad_x = spmm_transposed_planned(st, None, g, mean)
            else:
                grad_x = spmm_transposed_planned(st, None, g.float(), mean).to(g.dtype)
        elif ctx.needs_input_grad[0]:
            csr2csc = st.csr2csc()  # first: it leaves colptr and row[csr2csc] behind
            grad_x = ops.edge_spmm_bw_x(st.colptr(), st._row_in_csc_order(), csr2csc, g, edge, x, op, scale,
                                        no_long_columns=st._csc_view()._longest_row() <= ops.LONG_ROW)
        return grad_x, grad_edge, None, None, None, None


def edge_spmm(src: SparseTensor, x: torch.Tensor, edge: Optional[torch.Tensor] = None, op: str = "mul",
              reduce: str = "sum") -> torch.Tensor:
    """out [M, K]: for every row of `src` the sum (reduce="sum" / "add") or the mean of the messages
    x[col(e)] * edge[e] (op="mul"), x[col(e)] + edge[e] ("add") or relu(x[col(e)] + edge[e]) ("add_relu") over its
    stored entries.  x [N, K]; edge [nnz, K] in storage (CSR) order, or None for the stored values of `src`, which
    must then be [nnz, K].  Both float32 or both bfloat16, and `out` has their dtype; bfloat16 sums in float32 and
    rounds once.  A row without entries is 0.  Differentiable in `x` and in `edge` (a tracked stored value included).
    No zero skipping (0 * inf is NaN) and relu(NaN) is NaN; the gradients of add_relu are 0 where the message is
    not > 0, a NaN message included.
    The kernels read nothing back, but the storage does once: the longest row, and in the backward the CSC view and
    its longest column, are found on first use (one host read each) and kept on the storage.  Capture a graph after
    one warm-up step on the same `src`.  `adj.set_value(e)` makes a new storage that inherits only what `adj` had
    found by then, so in a loop over changing edge features pass them as `edge` and keep one `adj`."""
    if reduce in ("min", "max"):
        raise NotImplementedError(f"edge_spmm: reduce={reduce!r} is not built (its backward needs the winners); "
                                  "use sum or mean")
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"unknown reduce {reduce!r}: choose from sum (add), mean")
    if op not in ops.EDGE_OP_ID:
        raise ValueError(f"unknown op {op!r}: choose from mul, add, add_relu")
    if edge is None:
        edge = src.storage.value()
        if edge is None:
            raise ValueError("edge_spmm needs `edge` [nnz, K] or stored values of that shape")
    if not isinstance(x, torch.Tensor) or not isinstance(edge, torch.Tensor):
        raise TypeError("x and edge must be torch.Tensors")
    nnz = src.storage.col().numel()
    if x.dim() != 2 or x.shape[0] != src.sparse_size(1):
        raise ValueError(f"x must be [{src.sparse_size(1)}, K] (got {tuple(x.shape)})")
    if edge.dim() != 2 or edge.shape != (nnz, x.shape[1]):
        raise ValueError(f"edge must be [{nnz}, {x.shape[1]}], one row per stored entry (got {tuple(edge.shape)})")
    if x.dtype != edge.dtype or x.dtype not in ops.EDGE_SPMM_DTYPES:
        raise TypeError(f"edge_spmm takes x and edge both float32 or both bfloat16 (got {x.dtype}, {edge.dtype})")
    ops._gpu(x, "x")
    ops._gpu(edge, "edge")
    # forward() sees requires_grad flags only: whether a backward can follow at all is decided here
    return _EdgeSpMM.apply(x, edge, src.storage, op, reduce == "mean", torch.is_grad_enabled())


SparseTensor.edge_spmm = lambda self, x, edge=None, op="mul", reduce="sum": edge_spmm(self, x, edge, op, reduce)
