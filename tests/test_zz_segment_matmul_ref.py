"""CPU suite for segment_matmul: the names are exported and bound, the raw ops refuse CPU tensors, the float64
restatement the GPU suite compares against agrees with numpy.matmul per segment, and the chunk bound holds."""
import numpy as np
import pytest
import torch

import segment_matmul_ref as ref


def test_names_are_exported_and_bound():
    import paddle_sparse_amd as ps
    from paddle_sparse_amd import _lib, ops

    assert {"segment_matmul", "typed_matmul"} <= set(ps.__all__)
    assert callable(ps.segment_matmul) and callable(ps.typed_matmul)
    assert {"psa_segment_matmul", "psa_segment_matmul_bw_weight", "psa_segment_matmul_bw_chunks",
            "psa_segment_matmul_tile"} <= set(_lib.SIGNATURES)
    assert min(ops.SEGMENT_MATMUL_BM, ops.SEGMENT_MATMUL_BN, ops.SEGMENT_MATMUL_BK, ops.SEGMENT_MATMUL_CH) > 0
    # an unknown dtype code is refused before anything is touched
    assert _lib.load().psa_segment_matmul(1, None, None, None, None, None, 0, 0, 0, 1, 1, 0, None, None, None) == 1


@pytest.mark.parametrize("op", ("segment_matmul", "segment_matmul_bw_weight"))
def test_ops_refuse_cpu_tensors(op):
    from paddle_sparse_amd import ops

    other = torch.zeros(1, 2, 2) if op == "segment_matmul" else torch.zeros(3, 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        getattr(ops, op)(torch.zeros(3, 2), torch.tensor([0, 3]), other)


def test_reference_matches_matmul_per_segment():
    x = np.arange(12.0).reshape(4, 3)
    w = np.stack([np.eye(3), 2 * np.ones((3, 3)), np.arange(9.0).reshape(3, 3)])
    ptr, index, g = np.array([0, 1, 1, 5]), np.array([3, 0, 0, 2, 1]), np.arange(15.0).reshape(5, 3)
    out = ref.forward(x, ptr, w, index)
    assert np.array_equal(out[:1], np.matmul(x[[3]], w[0]))
    assert np.array_equal(out[1:], np.matmul(x[[0, 0, 2, 1]], w[2]))
    grad_x, grad_w = ref.backward(x, ptr, w, g, index)
    assert np.array_equal(grad_w[1], np.zeros((3, 3))) and np.array_equal(grad_w[2], x[[0, 0, 2, 1]].T @ g[1:])
    assert np.array_equal(grad_x[0], (g[1] + g[2]) @ w[2].T) and np.array_equal(grad_x[3], g[0] @ w[0].T)
    assert ref.round_bf16(np.array([1.00390625, 1.01171875, 257.0])).tolist() == [1.0, 1.015625, 256.0]  # ties to even


def test_chunk_bound_covers_the_true_count():
    from paddle_sparse_amd import ops

    BM, CH = ops.SEGMENT_MATMUL_BM, ops.SEGMENT_MATMUL_CH
    lengths = (0, 1, BM - 1, 0, BM, BM + 1, 2 * BM + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 0)
    true = sum(-(-n // CH) for n in lengths if n > CH)
    assert true == 5 and ops.segment_matmul_bw_chunks(sum(lengths)) >= true
    assert ops.segment_matmul_bw_chunks(0) == 0 and ops.segment_matmul_bw_chunks(CH + 1) >= 2
