"""softmax over the stored entries of every row or column of a SparseTensor — what an
attention layer (GAT, graph transformers) does with its per-edge scores before it
aggregates.  Upstream has no such op; the semantics are torch.softmax on the dense row
with the missing entries at -inf.

One HIP op each way (csrc/softmax.hip: psa_segment_softmax / psa_segment_softmax_bw):
dim = 1 runs over rowptr, dim = 0 over colptr with perm = csr2csc, so nothing is
transposed and the result stays in CSR order.  No atomics: the bits repeat run to run.

Non-finite values: a group (per head) that holds a NaN, a +inf or nothing but -inf is NaN
in every entry; a -inf entry among finite ones gives exactly 0.
"""
from __future__ import annotations

import torch

from . import ops
from .tensor import SparseTensor


def softmax(src: SparseTensor, dim: int = 1) -> SparseTensor:
    """Same pattern as `src`; values = softmax of the stored values over each row (dim = 1 / -1)
    or each column (dim = 0 / -2).  [nnz, H] values give one softmax per head; no values count
    as ones (the result is 1 / degree).  fp32 values only.  Values that autograd tracks stay
    tracked.  The result keeps every cache of `src` that depends on the pattern alone."""
    if not isinstance(dim, int) or isinstance(dim, bool):
        raise TypeError("softmax: dim must be an int")
    if dim < 0:
        dim += 2
    if dim not in (0, 1):
        raise ValueError("softmax: dim must be 0 or 1 (-2 or -1)")
    st = src.storage
    value = st.value()
    if value is None:
        value = torch.ones(st.col().numel(), dtype=torch.float32, device=st.col().device)
    if value.dtype != torch.float32:
        raise TypeError(f"softmax takes float32 values (got {value.dtype})")
    if dim == 1:
        out = ops.segment_softmax(value, st.rowptr())
    else:
        perm = st.csr2csc()  # leaves colptr behind
        out = ops.segment_softmax(value, st.colptr(), perm)
    return src.set_value(out, layout="coo")


SparseTensor.softmax = lambda self, dim=1: softmax(self, dim)
