"""CPU suite for the diagonal ops (remove_diag / set_diag / fill_diag / get_diag): the
public surface, the C-ABI entry points and the diagonal arithmetic.  No kernel runs."""
import ctypes

import pytest
import torch

DIAG_SYMBOLS = ("psa_diag_workspace_bytes", "psa_diag_count", "psa_diag_write", "psa_get_diag", "psa_diag_gather",
                "psa_diag_scatter")
NAMES = ("remove_diag", "set_diag", "fill_diag", "get_diag")


def test_the_four_ops_are_exported_and_attached():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, diag

    for name in NAMES:
        assert name in psa.__all__
        assert getattr(psa, name) is getattr(diag, name)
        assert callable(getattr(SparseTensor, name))


def test_the_entry_points_are_declared_exported_and_bound():
    from test_abi import declared_functions

    from paddle_sparse_amd import _lib

    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in DIAG_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().psa_diag_workspace_bytes(1000) >= 8 * 1000


def _cpu_csr():
    from paddle_sparse_amd import SparseTensor

    rowptr = torch.tensor([0, 2, 3, 3])
    col = torch.tensor([0, 2, 1])
    return SparseTensor(rowptr=rowptr, col=col, value=torch.ones(3), sparse_sizes=(3, 3), is_sorted=True,
                        trust_data=True)


@pytest.mark.parametrize("name", NAMES)
def test_the_ops_reject_cpu_tensors(name):
    import paddle_sparse_amd as psa

    a = _cpu_csr()
    args = (1.0,) if name == "fill_diag" else ()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        getattr(psa, name)(a, *args)


def test_the_raw_ops_reject_cpu_tensors():
    from paddle_sparse_amd import ops

    ptr, col = torch.tensor([0, 1]), torch.tensor([0])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.diag_count(ptr, col, 1, 1, 0, True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.get_diag(ptr, col, None, 1, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.diag_gather(torch.ones(1), col)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.diag_scatter(torch.ones(1), col, 1)


@pytest.mark.parametrize("M,N", [(5, 5), (3, 7), (7, 3), (1, 1), (0, 4), (4, 0)])
def test_num_diag_and_start(M, N):
    from paddle_sparse_amd.diag import diag_start, num_diag

    for k in (-M - 1, -M, -1, 0, 1, N - 1, N, N + 5):
        cells = [r for r in range(M) if 0 <= r + k < N]
        assert num_diag(M, N, k) == len(cells), (M, N, k)
        if cells:
            assert diag_start(k) == cells[0]
            assert cells == list(range(diag_start(k), diag_start(k) + len(cells)))
