"""Multi-aggregation on the SparseTensor surface: `spmm_multi`, several reductions of the same
neighbourhood from one gather of the dense operand.

    out = adj.spmm_multi(x, reduce=("mean", "min", "max", "std"), eps=1e-5)   # [M, A, K]

out[:, a] is statistic reduce[a] of the messages value[e] * x[col[e]] of every row, and
out.reshape(M, A * K) is PyG's MultiAggregation(mode="cat") / the aggregator block of a PNA layer.
The forward is one HIP launch family (psa_spmm_multi, csrc/spmm_multi.hip).  The gradient wrt `x`
is built from kernels that exist: with n the row lengths, mu the mean and, per requested statistic,
g_s, g_m, g_v, g_d, g_min, g_max the slices of the upstream gradient,

    gv     = g_v + g_d / (2 std)
    grad_x = A^T (g_s + g_m / n - 2 gv mu / n)  +  x * ((A o A)^T (2 gv / n))  +  [min / max winners]

(the clamp of var at 0 passes the gradient through; a row without entries contributes nothing; where
std is 0, which needs eps = 0, its term is dropped).  The transposed products are planned forwards over the
CSC view (matmul.spmm_transposed_planned), ONE of them over the [M, 2K] concatenation when the tensor
has no values; the winners' part is ops.spmm_minmax_bw through the int64 winners the forward left.
The gradient wrt the values is not built.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .matmul import _csc_weights, spmm_planned, spmm_transposed_planned
from .storage import SparseStorage
from .tensor import SparseTensor

_SUM, _MEAN, _MIN, _MAX, _VAR, _STD = (ops.STAT_ID[n] for n in ("sum", "mean", "min", "max", "var", "std"))


class _SpMMMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, value: Optional[torch.Tensor], storage: SparseStorage, names, eps: float,
                track: bool):
        codes = ops.spmm_multi_stats(names)
        need = track and ctx.needs_input_grad[0]
        moments = _VAR in codes or _STD in codes
        # the backward of var / std reads the mean: out's own slice, or sum / n, or, when `reduce` names neither, one
        # more [M, K] tile that the kernel writes beside out (the mean is in its registers either way)
        extra = need and moments and _MEAN not in codes and _SUM not in codes
        out, arg_min, arg_max, *mean = ops.spmm_multi(storage.rowptr(), storage.col(), value, x, names, eps, want_arg=need,
                                                      no_long_rows=storage._longest_row() <= ops.LONG_ROW, want_mean=extra)
        if need:
            at = {c: a for a, c in enumerate(codes)}
            mu = std = total = None
            if moments:
                mu = mean[0] if extra else (out[:, at[_MEAN]] if _MEAN in at else None)  # None: sum / n in the backward
                std = out[:, at[_STD]] if _STD in at else None
                total = out[:, at[_SUM]] if mu is None else None
            ctx.storage, ctx.at = storage, at
            ctx.save_for_backward(x, value, mu, std, total, arg_min, arg_max)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        x, value, mu, std, total, arg_min, arg_max = ctx.saved_tensors
        st, at = ctx.storage, ctx.at
        g = grad_out.contiguous()

        def part(code):
            return g[:, at[code]] if code in at else None

        n = st.rowcount().to(torch.float32)
        inv_n = torch.where(n > 0, 1.0 / n.clamp(min=1.0), torch.zeros_like(n)).unsqueeze(1)  # 0 for a row without entries
        u = part(_SUM)
        if _MEAN in at:
            gm = part(_MEAN) * inv_n
            u = gm if u is None else u + gm
        w = None
        if _VAR in at or _STD in at:
            gv = part(_VAR)
            if _STD in at:
                gd = part(_STD) * torch.where(std > 0, 0.5 / std, torch.zeros_like(std))
                gv = gd if gv is None else gv + gd
            if mu is None:
                mu = total * inv_n
            w = 2.0 * gv * inv_n
            u = -(w * mu) if u is None else u - w * mu
        grad_x = None
        if u is not None and w is not None and value is None:
            # A o A = A: both transposed products in one pass over the [M, 2K] concatenation
            K = x.shape[1]
            both = spmm_transposed_planned(st, None, torch.cat([u, w], dim=1))
            grad_x = both[:, :K] + x * both[:, K:]
        elif u is not None:
            grad_x = spmm_transposed_planned(st, value, u.contiguous())
            if w is not None:
                # the squared values in CSC order from the memoised value[csr2csc], which stays as it is
                w_csc = _csc_weights(st, value, st.csr2csc(), st._row_in_csc_order(), False)
                grad_x = grad_x + x * spmm_planned(st._csc_view(), w_csc * w_csc, w.contiguous(), "sum")
        for code, arg in ((_MIN, arg_min), (_MAX, arg_max)):
            if code in at:
                _, gw = ops.spmm_minmax_bw(st.col(), value, x, part(code).contiguous(), arg, want_value=False, want_mat=True)
                grad_x = gw if grad_x is None else grad_x + gw
        return grad_x, None, None, None, None, None


def spmm_multi(src: SparseTensor, x: torch.Tensor, reduce: Sequence[str] = ("mean", "min", "max", "std"),
               eps: float = 1e-5) -> torch.Tensor:
    """out [M, A, K] float32 with out[:, a] = statistic reduce[a] over the messages value[e] * x[col[e]] of every
    row of `src` (x[col[e]] when `src` has no values), all from one gather of `x` [N, K] float32.  `reduce`: a
    non-empty sequence of distinct names out of sum (add), mean, min, max, var (population variance, clamped at 0)
    and std = sqrt(var + eps).  A row without entries is 0 in every statistic; ties in min / max go to the earlier
    entry.  Differentiable in `x`; tracked values raise NotImplementedError."""
    ops.spmm_multi_stats(reduce)  # ValueError for an empty, unknown or repeated name
    ops._gpu(x, "x")
    if x.dtype in (torch.float16, torch.bfloat16):
        raise TypeError(f"spmm_multi takes a float32 dense operand; half-width operands are not built yet (x is {x.dtype})")
    if x.dim() == 3:
        raise ValueError(f"spmm_multi takes a 2-D dense operand [N, K]; [N, H, F] operands are not built yet (got {tuple(x.shape)})")
    if x.dim() != 2 or x.shape[0] != src.sparse_size(1):
        raise ValueError(f"dense operand must be [{src.sparse_size(1)}, K]")
    value = src.storage.value()
    if value is not None and value.dim() != 1:
        raise ValueError("spmm needs scalar edge values")
    track = torch.is_grad_enabled()
    if track and value is not None and value.requires_grad:
        raise NotImplementedError("spmm_multi: the gradient wrt the values is not built; detach them "
                                  "(adj.set_value(value.detach())) or use one adj.matmul(x, r) per reduction")
    # forward() sees requires_grad flags only: whether a backward can follow at all is decided here
    return _SpMMMulti.apply(x, None if value is None else value.detach(), src.storage, tuple(reduce), float(eps), track)


SparseTensor.spmm_multi = lambda self, x, reduce=("mean", "min", "max", "std"), eps=1e-5: spmm_multi(self, x, reduce, eps)
