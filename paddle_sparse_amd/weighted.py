"""EdgeCDF — what the edge-weighted samplers read: the prefix sums of a matrix's values
inside every row (csrc/weighted.hip), built once and held by the user, as a NeighborSampler
is.  random_walk, sample_adj and neighbor_sample take one as `weighted=`; `weighted=True`
builds one per call (a NeighborSampler: once, at construction).

A weighted pick turns the random word of the uniform draw (csrc/rng.h: stream, draw) into
u in [0, 1) and looks u * total up in the row's prefix sums, so an entry is taken with
probability value / total and an entry of value zero is never taken.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import ops
from .tensor import SparseTensor

_VALUE_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.int64)


class EdgeCDF:
    """The row CDF of adj's stored values, as sampling weights: cum (float64[nnz]) holds the
    inclusive prefix sum of every row, summed strictly left to right in float64.

    adj needs 1-D values of a floating dtype, int32 or int64 (converted with .double());
    no values or [nnz, D] values raise ValueError, and so does a negative weight (-0.0 is
    zero), a NaN or infinite weight, or a row whose total overflows float64: one host read
    at construction.  The object remembers the rowptr it was built from and serves that
    matrix only; it holds the values as they were at construction, so build a new one after
    changing them."""

    def __init__(self, adj: SparseTensor):
        if not isinstance(adj, SparseTensor):
            raise TypeError("EdgeCDF needs a SparseTensor")
        rowptr, _, value = adj.csr()
        if value is None:
            raise ValueError("EdgeCDF needs a matrix with values: they are the sampling weights")
        if value.dim() != 1:
            raise ValueError(f"EdgeCDF needs one weight per entry (1-D values), got values of shape {tuple(value.shape)}")
        if value.dtype not in _VALUE_DTYPES:
            raise ValueError(f"EdgeCDF takes floating, int32 or int64 values (got {value.dtype})")
        cum, flags = ops.row_cdf(rowptr, value.detach().double())
        flags = int(flags.item())
        if flags & ops.CDF_NEGATIVE:
            raise ValueError("EdgeCDF: a weight is negative")
        if flags & ops.CDF_NONFINITE:
            raise ValueError("EdgeCDF: a weight is NaN or infinite")
        if flags & ops.CDF_OVERFLOW:
            raise ValueError("EdgeCDF: the weights of a row sum to infinity in float64 (overflow)")
        self.rowptr = rowptr
        self.cum = cum

    def cum_for(self, src: SparseTensor) -> torch.Tensor:
        """cum, after checking that src is the matrix this object was built from."""
        rowptr = src.storage.rowptr()
        if rowptr is not self.rowptr and (rowptr.data_ptr() != self.rowptr.data_ptr()
                                          or rowptr.numel() != self.rowptr.numel()):
            raise ValueError("this EdgeCDF was built from another matrix")
        return self.cum


def resolve(src: SparseTensor, weighted: Union[bool, EdgeCDF, None]) -> Optional[torch.Tensor]:
    """The cum tensor for an op's `weighted` argument: None for False, a fresh EdgeCDF's for
    True, the given EdgeCDF's after the matrix check."""
    if weighted is None or weighted is False:
        return None
    if weighted is True:
        return EdgeCDF(src).cum
    if isinstance(weighted, EdgeCDF):
        return weighted.cum_for(src)
    raise TypeError("weighted must be a bool or an EdgeCDF")
