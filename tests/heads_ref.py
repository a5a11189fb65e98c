"""float64 restatement of the multi-head ends of the attention path, numpy only: SpMM over
per-head values, sddmm per head and their four gradients in closed form.  The GPU tests hold
the kernels to it; tests/test_heads_ref.py holds it to a hand-worked case and to torch.einsum
autograd on the CPU.

    spmm   out[r, h, f] = sum_{e in row r} value[e, h] * mat[col[e], h, f]
    sddmm  out[e, h]    = <x[row(e), h, :], y[col[e], h, :]>

Plain IEEE arithmetic, no zero skipping: a stored 0 against an inf is NaN."""
import numpy as np


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def _scatter_rows(index, n, weight, dense):
    """out[index[e], h, :] += weight[e, h] * dense[e, h, :]."""
    out = np.zeros((n,) + dense.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out, index, weight[:, :, None] * dense)
    return out


def spmm_heads_ref(rowptr, col, value, mat):
    """[M, H, F] from value [nnz, H] and mat [N, H, F]."""
    value, mat = _f64(value, mat)
    return _scatter_rows(rows_of(rowptr), np.asarray(rowptr).size - 1, value, mat[np.asarray(col, dtype=np.int64)])


def sddmm_heads_ref(rowptr, col, x, y):
    """[nnz, H] from x [M, H, K] and y [N, H, K]."""
    x, y = _f64(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("ehk,ehk->eh", x[rows_of(rowptr)], y[np.asarray(col, dtype=np.int64)])


def spmm_heads_grad_value(rowptr, col, mat, grad_out):
    """d/d value[e, h] of sum(out * grad_out) = <grad_out[row(e), h, :], mat[col[e], h, :]>."""
    return sddmm_heads_ref(rowptr, col, grad_out, mat)


def spmm_heads_grad_mat(rowptr, col, value, grad_out, N):
    """d/d mat[c, h, :] = sum over the entries of column c of value[e, h] * grad_out[row(e), h, :]."""
    value, grad_out = _f64(value, grad_out)
    return _scatter_rows(np.asarray(col, dtype=np.int64), N, value, grad_out[rows_of(rowptr)])


def sddmm_heads_grad_x(rowptr, col, y, grad_out):
    """d/d x[r, h, :] of sum(out * grad_out) = sum over the entries of row r of grad_out[e, h] * y[col[e], h, :]."""
    return spmm_heads_ref(rowptr, col, grad_out, y)


def sddmm_heads_grad_y(rowptr, col, x, grad_out, N):
    """d/d y[c, h, :] = sum over the entries of column c of grad_out[e, h] * x[row(e), h, :]."""
    grad_out, x = _f64(grad_out, x)
    return _scatter_rows(np.asarray(col, dtype=np.int64), N, grad_out, x[rows_of(rowptr)])


def spmm_heads_abs_sum(rowptr, col, value, mat):
    """Per output element: the sum of |value * mat| over the row's terms (the scale of a rounding bound)."""
    value, mat = _f64(value, mat)
    return spmm_heads_ref(rowptr, col, np.abs(value), np.abs(mat))
