"""float64 restatement of segment_matmul and its two gradients (test infrastructure)."""
import numpy as np


def forward(x, ptr, weight, index=None):
    """out[r] = x_row(r) @ weight[t] for ptr[t] <= r < ptr[t + 1]; weight [T, K, F]."""
    rows = np.asarray(x, np.float64)[slice(None) if index is None else index]
    w = np.asarray(weight, np.float64)
    out = np.zeros((rows.shape[0], w.shape[2]))
    for t in range(len(ptr) - 1):
        out[ptr[t]:ptr[t + 1]] = rows[ptr[t]:ptr[t + 1]] @ w[t]
    return out


def backward(x, ptr, weight, grad, index=None):
    """(grad_x [Nx, K], grad_weight [T, K, F]) of sum(forward * grad)."""
    x, g = np.asarray(x, np.float64), np.asarray(grad, np.float64)
    grad_rows = forward(g, ptr, np.asarray(weight, np.float64).transpose(0, 2, 1))
    rows = x[slice(None) if index is None else index]
    grad_w = np.stack([rows[ptr[t]:ptr[t + 1]].T @ g[ptr[t]:ptr[t + 1]] for t in range(len(ptr) - 1)])
    grad_x = np.zeros_like(x)
    np.add.at(grad_x, np.arange(len(x)) if index is None else index, grad_rows)
    return grad_x, grad_w


def round_bf16(a):
    """a (exact in float32) rounded once to bfloat16, to nearest even, as float32."""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
