"""float64 restatement of typed_spmm and its two gradients (test infrastructure).  Entries are (row, col, etype) in
storage order; `bf16=True` restates the one rounding of the aggregated rows H_t to bfloat16."""
import numpy as np

from segment_matmul_ref import round_bf16


def inv_count(row, etype):
    """float32 1 / (entries of the same row and type), per entry."""
    _, inverse, count = np.unique(np.stack([row, etype]), axis=1, return_inverse=True, return_counts=True)
    return np.float32(1) / count[inverse.reshape(-1)].astype(np.float32)


def aggregate(rows, cols, etype, t, x, value, n_out, bf16):
    """H_t [n_out, K] = sum over the entries of type t of value * x[cols], summed into rows."""
    m, x = etype == t, np.asarray(x, np.float64)
    H = np.zeros((n_out, x.shape[1]))
    v = np.ones(m.sum()) if value is None else np.asarray(value, np.float64)[m]
    np.add.at(H, rows[m], v[:, None] * x[cols[m]])
    return round_bf16(H).astype(np.float64) if bf16 else H


def forward(row, col, etype, x, weight, value=None, M=None, bf16=False):
    """out [M, F] = sum over t of H_t @ weight[t]."""
    w = np.asarray(weight, np.float64)
    return sum(aggregate(row, col, etype, t, x, value, M, bf16) @ w[t] for t in range(len(w)))


def backward(row, col, etype, x, weight, grad, value=None, bf16=False):
    """(grad_x [N, K], grad_weight [T, K, F]) of sum(forward * grad)."""
    w, g = np.asarray(weight, np.float64), np.asarray(grad, np.float64)
    grad_x = sum(aggregate(col, row, etype, t, g, value, len(x), bf16) @ w[t].T for t in range(len(w)))
    grad_w = np.stack([aggregate(row, col, etype, t, x, value, len(g), bf16).T @ g for t in range(len(w))])
    return grad_x, grad_w
