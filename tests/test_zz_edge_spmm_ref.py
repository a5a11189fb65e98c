"""CPU suite for edge_spmm: the names are exported, declared and bound, no workspace size function was added, and
every argument error is raised before anything is launched (none of this needs a GPU)."""
from pathlib import Path

import pytest
import torch

import paddle_sparse_amd as ps
from paddle_sparse_amd import SparseTensor, _lib

SYMBOLS = ("psa_edge_spmm", "psa_edge_spmm_bw_x", "psa_edge_spmm_bw_edge", "psa_edge_spmm_tile")
F32, F64, BF16 = 0, 1, 5  # psa_dtype


def test_names_are_exported_declared_and_bound():
    assert "edge_spmm" in ps.__all__ and callable(ps.edge_spmm) and callable(SparseTensor.edge_spmm)
    header = (Path(__file__).resolve().parent.parent / "include" / "paddle_sparse_hip.h").read_text()
    lib = _lib.load()
    for name in SYMBOLS:
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert not [n for n in _lib.SIGNATURES if "edge_spmm" in n and n.endswith("_workspace_bytes")]


def adjacency():
    return SparseTensor(rowptr=torch.tensor([0, 2, 2, 3]), col=torch.tensor([0, 3, 1]), sparse_sizes=(3, 4),
                        is_sorted=True, trust_data=True)


@pytest.mark.parametrize("kwargs,x,edge,error", [
    (dict(reduce="max"), (4, 2), (3, 2), NotImplementedError),
    (dict(reduce="min"), (4, 2), (3, 2), NotImplementedError),
    (dict(reduce="prod"), (4, 2), (3, 2), ValueError),
    (dict(op="sub"), (4, 2), (3, 2), ValueError),
    (dict(), (5, 2), (3, 2), ValueError),     # x rows != N
    (dict(), (4, 2), (2, 2), ValueError),     # edge rows != nnz
    (dict(), (4, 2), (3, 3), ValueError),     # widths differ
    (dict(), (4, 2), (3,), ValueError),       # scalar entries: that is spmm
    (dict(), (4, 2), None, ValueError),       # no edge and no stored values
    (dict(), (4, 2), (3, 2, torch.bfloat16), TypeError),
    (dict(), (4, 2, torch.float64), (3, 2, torch.float64), TypeError),
    (dict(), (4, 2), (3, 2), RuntimeError),   # all in order, but on the CPU: the ops._gpu error
])
def test_argument_errors(kwargs, x, edge, error):
    def tensor(spec):
        dtype = spec[-1] if isinstance(spec[-1], torch.dtype) else torch.float32
        return torch.zeros([d for d in spec if isinstance(d, int)], dtype=dtype)

    with pytest.raises(error):
        ps.edge_spmm(adjacency(), tensor(x), None if edge is None else tensor(edge), **kwargs)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    rowptr, col = torch.tensor([0, 300, 300]), torch.arange(300) % 4
    buf = [torch.zeros(65536, dtype=torch.uint8).data_ptr() for _ in range(5)]
    need = lib.psa_spmm_heads_workspace_bytes(300, 1, 8)

    def forward(dtype=F32, op=0, mean=0, K=8, out=buf[2], ws_bytes=need):
        return lib.psa_edge_spmm(dtype, op, mean, rowptr.data_ptr(), col.data_ptr(), buf[0], buf[1], 2, 4, K, 300, out,
                                 buf[4], ws_bytes, None)
    assert forward(dtype=F64) == 1 and forward(op=3) == 1 and forward(mean=2) == 1 and forward(K=-1) == 1
    assert forward(out=None) == 1
    assert forward(dtype=BF16, ws_bytes=need - 1) == 3
    assert lib.psa_last_error().decode() == "psa_edge_spmm: workspace too small"
    assert forward(K=0) == 0  # nothing to write, nothing launched

    def bw_x(dtype=F32, op=0, x=buf[2]):
        return lib.psa_edge_spmm_bw_x(dtype, op, rowptr.data_ptr(), col.data_ptr(), col.data_ptr(), buf[0], buf[1], x, None,
                                      4, 2, 8, 300, buf[3], buf[4], need - 1, None)
    assert bw_x(dtype=F64) == 1 and bw_x(op=1) == 1 and bw_x(op=2, x=None) == 1 and bw_x() == 3

    def bw_edge(dtype=F32, op=0, x=buf[2], nnz=300):
        return lib.psa_edge_spmm_bw_edge(dtype, op, col.data_ptr(), col.data_ptr(), buf[0], x, buf[1], None, 4, 4, 8, nnz,
                                         buf[3], None)
    assert bw_edge(dtype=4) == 1 and bw_edge(op=-1) == 1 and bw_edge(x=None) == 1 and bw_edge(nnz=-1) == 1
    assert bw_edge(nnz=0) == 0
