"""CPU suite for reverse_cuthill_mckee: the reference restatement of tests/rcm_ref.py
against the hand-checked known answer and against an independent level-form restatement,
and the host-side surface (symbols, exports, argument errors).  No kernel runs."""
import numpy as np
import pytest
import torch

import rcm_ref as R


def test_known_answer():
    rowptr, col = R.undirected(R.KAT_N, R.KAT_EDGES)
    assert rowptr.tolist() == R.KAT_ROWPTR and col.tolist() == R.KAT_COL
    assert R.cuthill_mckee(rowptr, col).tolist() == [8, 0, 3, 5, 7, 2, 1, 4, 6]
    assert R.reverse_cuthill_mckee(rowptr, col).tolist() == R.KAT_PERM
    assert R.cuthill_mckee_levels(rowptr, col).tolist() == [8, 0, 3, 5, 7, 2, 1, 4, 6]


@pytest.mark.parametrize("N,per_row,seed", [(1, 2, 0), (7, 2, 1), (60, 1, 2), (300, 2, 3), (300, 6, 4), (1500, 3, 5),
                                            (3000, 4, 6)])
def test_serial_and_level_form_agree(N, per_row, seed):
    rowptr, col = R.random_symmetric(N, per_row, seed)
    order = R.cuthill_mckee(rowptr, col)
    assert sorted(order.tolist()) == list(range(N))  # a permutation
    assert np.array_equal(order, R.cuthill_mckee_levels(rowptr, col))


def test_forms_agree_on_a_non_symmetric_pattern_with_duplicates():
    rng = np.random.default_rng(11)
    N = 200
    row, col = rng.integers(0, N, 500), rng.integers(0, N, 500)
    row, col = np.concatenate([row, row[:50], np.arange(0, N, 7)]), np.concatenate([col, col[:50], np.arange(0, N, 7)])
    rowptr, col = R.csr_of(N, row, col)
    order = R.cuthill_mckee(rowptr, col)
    assert sorted(order.tolist()) == list(range(N))
    assert np.array_equal(order, R.cuthill_mckee_levels(rowptr, col))


@pytest.mark.parametrize("n", [8, 33])
def test_shuffled_grid(n):
    rowptr, col = R.grid_graph(n, seed=n)
    perm = R.reverse_cuthill_mckee(rowptr, col)
    assert np.array_equal(perm[::-1], R.cuthill_mckee_levels(rowptr, col))
    before, after = R.bandwidth(rowptr, col), R.bandwidth(rowptr, col, perm)
    print(f"grid {n} x {n}: bandwidth {before} -> {after}")
    assert after == n            # the anti-diagonal levels of the grid: the widest has n nodes
    assert before > 10 * n or n < 33


def test_bandwidth_helper():
    rowptr, col = R.undirected(4, [(0, 3), (1, 2)])
    assert R.bandwidth(rowptr, col) == 3
    assert R.bandwidth(rowptr, col, [0, 3, 1, 2]) == 1
    assert R.bandwidth([0, 0, 0], []) == 0


def test_symbols_and_exports():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import _lib, ops

    for name in ("psa_rcm_workspace_bytes", "psa_rcm_init", "psa_rcm_small", "psa_rcm_level_count",
                 "psa_rcm_level_write", "psa_rcm_finish", "psa_rcm_small_capacity", "psa_rcm_tile",
                 "psa_rcm_set_variant"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "reverse_cuthill_mckee" in psa.__all__ and callable(psa.reverse_cuthill_mckee)
    assert callable(psa.SparseTensor.reverse_cuthill_mckee)
    assert callable(ops.reverse_cuthill_mckee)


def test_host_constants_and_variant_hook():
    from paddle_sparse_amd import _lib, ops

    lib = _lib.load()
    assert ops.rcm_set_variant(0) == 0
    assert ops.rcm_small_capacity() == 4096 and ops.rcm_tile() == 1024
    assert ops.rcm_set_variant(1) == 0 and ops.rcm_small_capacity() == 0
    assert ops.rcm_set_variant(2) == 1 and ops.rcm_small_capacity() == 8
    assert ops.rcm_set_variant(0) == 2
    # N outside [1, 2^31): no workspace, and every entry point refuses before a launch
    assert lib.psa_rcm_workspace_bytes(0, 0) == 0 and lib.psa_rcm_workspace_bytes(2**31, 10) == 0
    assert lib.psa_rcm_workspace_bytes(1000, 4000) > 1000 * 52
    assert lib.psa_rcm_finish(2**31, 10, None, 0, None, None) != 0
    assert b"2^31" in lib.psa_last_error()


def _cpu_adj(M=3, N=3):
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.tensor([0, 2, 3, 3]), col=torch.tensor([0, 2, 1]), value=torch.ones(3),
                        sparse_sizes=(M, N), is_sorted=True, trust_data=True)


def test_argument_errors():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    with pytest.raises(ValueError, match="square"):
        psa.reverse_cuthill_mckee(_cpu_adj(3, 4))
    with pytest.raises(ValueError, match="square"):
        _cpu_adj(3, 4).reverse_cuthill_mckee(is_symmetric=True)
    for bad in (1, "yes", 0.0, torch.tensor(True)):
        with pytest.raises(TypeError, match="is_symmetric"):
            psa.reverse_cuthill_mckee(_cpu_adj(), bad)
    with pytest.raises(TypeError):
        psa.reverse_cuthill_mckee(torch.ones(3, 3))
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path
        psa.reverse_cuthill_mckee(_cpu_adj(), is_symmetric=True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.reverse_cuthill_mckee(torch.tensor([0, 1, 2]), torch.tensor([1, 0]))
