"""CPU suite: tests/heads_ref.py against a hand-worked 3 x 4, H = 2 case and against torch.einsum
float64 autograd on the dense [M, N, H] weights."""
import numpy as np
import torch

import heads_ref as hr

# 3 x 4 with an empty row and the cell (2, 1) stored twice
ROWPTR = np.array([0, 2, 2, 5], dtype=np.int64)
COL = np.array([1, 3, 0, 1, 1], dtype=np.int64)
VALUE = np.array([[1, 2], [3, -1], [2, 0], [-1, 1], [4, 2]], dtype=np.float64)
MAT = np.array([[[1, 2], [3, 4]], [[0, 1], [-1, 2]], [[5, 5], [5, 5]], [[2, -2], [1, 0]]], dtype=np.float64)
X = np.array([[[1, 1], [2, 0]], [[7, 7], [7, 7]], [[0, -1], [1, 1]]], dtype=np.float64)
# row 0: h0 1*[0,1] + 3*[2,-2], h1 2*[-1,2] - 1*[1,0]; row 2: h0 2*[1,2] - [0,1] + 4*[0,1], h1 0*[3,4] + [-1,2] + 2*[-1,2]
OUT = np.array([[[6, -5], [-3, 4]], [[0, 0], [0, 0]], [[2, 7], [-3, 6]]], dtype=np.float64)
# <x[row], mat[col]> per head
SCORES = np.array([[1, -2], [0, 2], [-2, 7], [-1, 1], [-1, 1]], dtype=np.float64)
# column 1 collects entries 0 (row 0), 3 and 4 (row 2); column 2 has none
GRAD_DENSE = np.array([[[0, -2], [0, 0]], [[1, -2], [7, 3]], [[0, 0], [0, 0]], [[3, 3], [-2, 0]]], dtype=np.float64)


def test_hand_worked_case():
    assert np.array_equal(hr.spmm_heads_ref(ROWPTR, COL, VALUE, MAT), OUT)
    assert np.array_equal(hr.sddmm_heads_ref(ROWPTR, COL, X, MAT), SCORES)
    # upstream gradient X for the SpMM, VALUE for the sddmm
    assert np.array_equal(hr.spmm_heads_grad_value(ROWPTR, COL, MAT, X), SCORES)
    assert np.array_equal(hr.spmm_heads_grad_mat(ROWPTR, COL, VALUE, X, 4), GRAD_DENSE)
    assert np.array_equal(hr.sddmm_heads_grad_x(ROWPTR, COL, MAT, VALUE), OUT)
    assert np.array_equal(hr.sddmm_heads_grad_y(ROWPTR, COL, X, VALUE, 4), GRAD_DENSE)
    assert np.array_equal(hr.spmm_heads_abs_sum(ROWPTR, COL, VALUE, MAT)[0], [[6, 7], [3, 4]])


def test_no_zero_skipping():
    mat = MAT.copy()
    mat[0, 1, 0] = np.inf  # met by entry 2 only, whose head-1 value is 0
    out = hr.spmm_heads_ref(ROWPTR, COL, VALUE, mat)
    assert np.isnan(out[2, 1, 0]) and np.isnan(out).sum() == 1
    assert np.array_equal(out[~np.isnan(out)], OUT[~np.isnan(out)])


def test_against_einsum_autograd():
    rng = np.random.default_rng(7)
    M, N, H, F, nnz = 6, 5, 3, 4, 40  # 40 entries in 30 cells: duplicates for certain
    row = np.sort(rng.integers(0, M, nnz))
    col = rng.integers(0, N, nnz)
    rowptr = np.searchsorted(row, np.arange(M + 1)).astype(np.int64)
    value, mat = rng.normal(size=(nnz, H)), rng.normal(size=(N, H, F))
    x, g_out, g_val = rng.normal(size=(M, H, F)), rng.normal(size=(M, H, F)), rng.normal(size=(nnz, H))
    ri, ci = torch.from_numpy(row), torch.from_numpy(col)

    vt, mt = torch.from_numpy(value).requires_grad_(), torch.from_numpy(mat).requires_grad_()
    W = torch.zeros(M, N, H, dtype=torch.float64).index_put((ri, ci), vt, accumulate=True)
    out = torch.einsum("mnh,nhf->mhf", W, mt)
    out.backward(torch.from_numpy(g_out))
    assert np.allclose(hr.spmm_heads_ref(rowptr, col, value, mat), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(hr.spmm_heads_grad_value(rowptr, col, mat, g_out), vt.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(hr.spmm_heads_grad_mat(rowptr, col, value, g_out, N), mt.grad.numpy(), rtol=1e-12, atol=1e-12)

    xt, yt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(mat).requires_grad_()
    scores = torch.einsum("mhk,nhk->mnh", xt, yt)[ri, ci]
    scores.backward(torch.from_numpy(g_val))
    assert np.allclose(hr.sddmm_heads_ref(rowptr, col, x, mat), scores.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(hr.sddmm_heads_grad_x(rowptr, col, mat, g_val), xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(hr.sddmm_heads_grad_y(rowptr, col, x, g_val, N), yt.grad.numpy(), rtol=1e-12, atol=1e-12)
