"""CPU suite for typed_spmm: the names are exported and bound, the raw ops refuse CPU tensors, and the float64
restatement the GPU suite compares against gives a hand-worked answer and agrees with dense autograd."""
import types

import numpy as np
import pytest
import torch

import typed_spmm_ref as ref


def test_names_are_exported_and_bound():
    import paddle_sparse_amd as ps
    from paddle_sparse_amd import _lib, ops

    assert {"RelationalPlan", "typed_spmm"} <= set(ps.__all__) and callable(ps.typed_spmm)
    assert {"psa_typed_spmm", "psa_typed_spmm_bw_weight", "psa_typed_spmm_bw_fold",
            "psa_typed_spmm_tile"} <= set(_lib.SIGNATURES)
    assert ops.TYPED_SPMM_BM == 64 and ops.TYPED_SPMM_KS % ops.TYPED_SPMM_BK == 0
    assert min(ops.TYPED_SPMM_CS, ops.TYPED_SPMM_PASS) > 0
    # an unknown dtype code is refused before anything is touched
    assert _lib.load().psa_typed_spmm(1, *[None] * 8, 0, 0, 0, 0, 1, 1, 0, None, None) == 1


@pytest.mark.parametrize("op", ("typed_spmm", "typed_spmm_bw_weight"))
def test_ops_refuse_cpu_tensors(op):
    from paddle_sparse_amd import ops

    plan = types.SimpleNamespace(N=3, M=3, T=1, nnz=0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        getattr(ops, op)(plan, torch.zeros(3, 2), torch.zeros(1, 2, 2))


def test_reference_gives_the_hand_worked_answer():
    """Three nodes, two types: 0 <- 1 (type 0, value 2), 0 <- 2 (type 1), 0 <- 1 again under type 1, 2 <- 0 (type 0)."""
    row, col, etype = np.array([0, 0, 0, 2]), np.array([1, 1, 2, 0]), np.array([0, 1, 1, 0])
    x = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    w = np.stack([np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]])])  # identity, swap
    value = np.array([2.0, 1.0, 1.0, 1.0])
    out = ref.forward(row, col, etype, x, w, value, 3)
    # row 0: 2 * x[1] + swap(x[1] + x[2]) = (6, 8) + (10, 8); row 2: x[0]
    assert out.tolist() == [[16.0, 16.0], [0.0, 0.0], [1.0, 2.0]]
    assert ref.inv_count(row, etype).tolist() == [1.0, 0.5, 0.5, 1.0]
    g = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 1.0]])
    grad_x, grad_w = ref.backward(row, col, etype, x, w, g, value)
    assert grad_x.tolist() == [[0.0, 1.0], [2.0, 1.0], [0.0, 1.0]]
    assert grad_w[0].tolist() == [[6.0, 1.0], [8.0, 2.0]] and grad_w[1].tolist() == [[8.0, 0.0], [10.0, 0.0]]
    # H of row 0, type 0 is 2 * 128.5 = 257, which bfloat16 rounds (a tie, to even) to 256
    assert ref.forward(row[:1], col[:1], etype[:1], [[0.0], [128.5]], [[[1.0]]], value[:1], 1, bf16=True) == 256.0


def test_reference_agrees_with_dense_autograd():
    rng = np.random.default_rng(0)
    n, T, K, F, nnz = 20, 3, 4, 5, 90
    row, col, etype = rng.integers(0, n, nnz), rng.integers(0, n, nnz), rng.integers(0, T, nnz)
    value, g = rng.standard_normal(nnz), rng.standard_normal((n, F))
    x = torch.tensor(rng.standard_normal((n, K)), requires_grad=True)
    w = torch.tensor(rng.standard_normal((T, K, F)), requires_grad=True)
    A = torch.zeros(T, n, n, dtype=torch.float64)
    A.index_put_((torch.tensor(etype), torch.tensor(row), torch.tensor(col)), torch.tensor(value), accumulate=True)
    out = torch.einsum("tij,jk,tkf->if", A, x, w)
    out.backward(torch.tensor(g))
    xn, wn = x.detach().numpy(), w.detach().numpy()
    assert np.allclose(ref.forward(row, col, etype, xn, wn, value, n), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    grad_x, grad_w = ref.backward(row, col, etype, xn, wn, g, value)
    assert np.allclose(grad_x, x.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(grad_w, w.grad.numpy(), rtol=1e-12, atol=1e-12)
