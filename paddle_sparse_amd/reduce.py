"""sum / mean / min / max over a SparseTensor — paddle_sparse/reduce.py:12-93.

dim=1 is a segmented reduction over CSR rows (reduce.py:50-51) and dim=0 a
scatter by column (reduce.py:40-42); both run as HIP kernels.  dim=None and
dim>1 reduce the dense value tensor with the framework's own reducers, as the
reference does.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .storage import _SORT_BEATS_ATOMICS
from .tensor import SparseTensor

# fp16 / bf16 values reduce over dim 0 by CSC segments at every size: the segmented reducer accumulates
# them in fp32 and rounds once, where a scatter would round after every 16-bit atomic (and in an order
# that changes from run to run)
_SEGMENTS_ONLY = (torch.float16, torch.bfloat16)

_DENSE = {"sum": "sum", "add": "sum", "mean": "mean", "min": "amin", "max": "amax"}


def _check(reduce: str) -> None:
    if reduce not in _DENSE:
        raise ValueError(reduce)


def reduction(src: SparseTensor, dim: Optional[int] = None, reduce: str = "sum") -> torch.Tensor:
    _check(reduce)
    value = src.storage.value()
    additive = reduce in ("sum", "add")

    if dim is None:
        if value is not None:
            return getattr(value, {"sum": "sum", "add": "sum", "mean": "mean", "min": "min", "max": "max"}[reduce])()
        return torch.full([], src.nnz() if additive else 1, dtype=src.dtype(), device=src.device())

    if dim < 0:
        dim = src.dim() + dim

    if dim == 0:
        if value is not None:
            st = src.storage
            if ((st.has_csr2csc() and st.has_colptr()) or st.col().numel() >= _SORT_BEATS_ATOMICS
                    or value.dtype in _SEGMENTS_ONLY or ops.needs_grad(value)):
                # Same sums as the scatter of reduce.py:42, taken column by
                # column in CSC order: no atomics (scattered device atomics
                # run ~20 G/s on this chip), and reproducible bit for bit.
                # value[csr2csc] is kept with the storage (st._value_in_csc_order): with it at
                # hand the reduction is a sequential read, 0.05 ms at 20 M entries against
                # 0.56 ms when every call gathers the values through the permutation
                # Values that autograd tracks always come here: ops.scatter has no backward, while
                # _value_in_csc_order and segment_csr are differentiable (and refuse min / max aloud),
                # so a cold and a cached storage give the same gradient
                return ops.segment_csr(st._value_in_csc_order(), st.colptr(), reduce)
            return ops.scatter(value, st.col(), src.size(1), reduce)
        if additive:
            return src.storage.colcount().to(src.dtype())
        return torch.ones(src.size(1), dtype=src.dtype(), device=src.device())
    if dim == 1:
        if value is not None:
            return ops.segment_csr(value, src.storage.rowptr(), reduce)
        if additive:
            return src.storage.rowcount().to(src.dtype())
        return torch.ones(src.size(0), dtype=src.dtype(), device=src.device())
    if value is not None:
        # reduce.py:59-69; the reference indexes `[0]` into paddle's min/max
        # result (a torch idiom that does not hold for Paddle) — the intended
        # value-wise reduction over the dense dim is what is returned here.
        return getattr(value, _DENSE[reduce])(dim - 1)
    raise ValueError


def _named(reduce: str):
    """The public one-reduction form and its SparseTensor method (reduce.py:74-93)."""
    def fn(src: SparseTensor, dim: Optional[int] = None) -> torch.Tensor:
        return reduction(src, dim, reduce=reduce)
    fn.__name__ = fn.__qualname__ = reduce
    setattr(SparseTensor, reduce, lambda self, dim=None: fn(self, dim))
    return fn


sum, mean, min, max = (_named(r) for r in ("sum", "mean", "min", "max"))  # noqa: A001
