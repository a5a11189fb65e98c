"""CPU suite for spmm_multi: the names are exported and bound, and the float64 restatement the GPU suite
compares against (tests/multi_aggr_ref.py) agrees with torch autograd of the dense formulation."""
import ctypes

import numpy as np
import torch

import multi_aggr_ref as ref


def test_names_are_exported_and_bound():
    import paddle_sparse_amd as ps
    from paddle_sparse_amd import SparseTensor, _lib, ops

    assert "spmm_multi" in ps.__all__ and callable(ps.spmm_multi) and callable(SparseTensor.spmm_multi)
    lib = _lib.load()
    assert "psa_spmm_multi" in _lib.SIGNATURES
    # partial rows per chunk: ("mean", "std") keeps two sums; all six with the winners 4 + 2
    assert ops.spmm_multi_partials((1, 5), True) == 2 and ops.spmm_multi_partials((0, 1, 2, 3, 4, 5), True) == 6
    assert ops.spmm_multi_partials((1, 3), False) == 2 and ops.spmm_multi_partials((2,), True) == 2
    # one row of 300 entries with a workspace one byte short: refused before anything is touched
    need = lib.psa_spmm_heads_workspace_bytes(300, 6, 8)
    rowptr, col = torch.tensor([0, 300, 300]), torch.arange(300)
    buf = [torch.zeros(65536, dtype=torch.uint8) for _ in range(5)]
    order = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    status = lib.psa_spmm_multi(rowptr.data_ptr(), col.data_ptr(), None, buf[0].data_ptr(), 2, 320, 8, 300, 63, 1e-5,
                                ctypes.addressof(order), 6, buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(),
                                None, buf[4].data_ptr(), need - 1, None)
    assert status == 3 and lib.psa_last_error().decode() == "psa_spmm_multi: workspace too small"
    assert ops.spmm_multi_stats(("std", "add")) == (5, 0)
    assert [ops.spmm_multi_lanes(k) for k in (1, 4, 20, 64, 128, 256, 257)] == [4, 4, 8, 16, 32, 64, 64]


def test_reference_agrees_with_dense_autograd():
    rng = np.random.default_rng(0)
    rowptr, col = np.array([0, 3, 3, 4, 9]), np.array([0, 2, 5, 1, 0, 1, 3, 4, 5])
    value, x = rng.standard_normal(9), rng.standard_normal((6, 3))  # continuous data: no ties
    reduce, eps = ("std", "max", "sum", "var", "min", "mean"), 1e-5
    g = rng.standard_normal((4, 6, 3))
    xt = torch.tensor(x, requires_grad=True)
    rows = []
    for i in range(4):
        m = torch.tensor(value[rowptr[i]:rowptr[i + 1], None]) * xt[col[rowptr[i]:rowptr[i + 1]]]
        if m.shape[0] == 0:
            rows.append(torch.zeros(6, 3, dtype=torch.float64))
            continue
        var = (m.var(0, unbiased=False)).clamp(min=0)
        rows.append(torch.stack([(var + eps).sqrt(), m.amax(0), m.sum(0), var, m.amin(0), m.mean(0)]))
    dense = torch.stack(rows)
    dense.backward(torch.tensor(g))
    out, arg, _ = ref.forward(rowptr, col, value, x, reduce, eps)
    assert np.allclose(out, dense.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert arg["max"][0, 0] == int(np.argmax(value[:3] * x[col[:3], 0])) and np.all(arg["min"][1] == 9)
    grad, terms, _, _ = ref.grad_x(rowptr, col, value, x, reduce, eps, g)
    assert np.allclose(grad, xt.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert terms.tolist() == [2, 2, 1, 1, 1, 2]
