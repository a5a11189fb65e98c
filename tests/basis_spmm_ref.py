"""float64 restatement of basis_spmm and its three gradients (test infrastructure).  Entries are (row, col, etype) in
storage order; `bf16=True` restates the one rounding of the aggregated rows Z_b and of P_b = grad @ basis[b]^T to
bfloat16."""
import numpy as np

from segment_matmul_ref import round_bf16
from typed_spmm_ref import inv_count  # noqa: F401  (the same rule: 1 / entries of the same row and type)


def _rounded(a, bf16):
    return round_bf16(a).astype(np.float64) if bf16 else a


def aggregate(rows, cols, etype, b, x, comp, value, n_out, bf16):
    """Z_b [n_out, K] = sum over the entries of value * comp[etype, b] * x[cols], summed into rows."""
    x = np.asarray(x, np.float64)
    Z = np.zeros((n_out, x.shape[1]))
    w = np.asarray(comp, np.float64)[etype, b] * (1.0 if value is None else np.asarray(value, np.float64))
    np.add.at(Z, rows, w[:, None] * x[cols])
    return _rounded(Z, bf16)


def forward(row, col, etype, x, basis, comp, value=None, M=None, bf16=False):
    """out [M, F] = sum over b of Z_b @ basis[b]."""
    V = np.asarray(basis, np.float64)
    return sum(aggregate(row, col, etype, b, x, comp, value, M, bf16) @ V[b] for b in range(len(V)))


def backward(row, col, etype, x, basis, comp, grad, value=None, bf16=False):
    """(grad_x [N, K], grad_basis [B, K, F], grad_comp [T, B], s [nnz, B]) of sum(forward * grad)."""
    V, g, x = np.asarray(basis, np.float64), np.asarray(grad, np.float64), np.asarray(x, np.float64)
    B = range(len(V))
    grad_x = sum(aggregate(col, row, etype, b, g, comp, value, len(x), bf16) @ V[b].T for b in B)
    grad_basis = np.stack([aggregate(row, col, etype, b, x, comp, value, len(g), bf16).T @ g for b in B])
    v = np.ones(len(row)) if value is None else np.asarray(value, np.float64)
    s = np.stack([v * np.einsum("ek,ek->e", x[col], _rounded(g @ V[b].T, bf16)[row]) for b in B], axis=1)
    grad_comp = np.zeros(np.shape(comp))
    np.add.at(grad_comp, etype, s)
    return grad_x, grad_basis, grad_comp, s
