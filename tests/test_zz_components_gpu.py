"""GPU suite for connected_components and largest_connected_components (csrc/components.hip).  The
result does not depend on the schedule (the root of a component is its smallest node), so every
comparison is bit-exact against the serial restatement of tests/components_ref.py (pinned to hand
answers and to scipy by test_zz_components_ref.py, which also holds the kernels' steps, run on the
host, to it), on the case table of that file: N and nnz either side of a wave and a workgroup, no
edges, self loops, duplicates, one directed edge in either direction, paths of 20 000 nodes in three
numberings (the identity one is a single chain of depth N after init), stars, a matching, a
shuffled grid, two cliques joined by the last stored entry, a random graph of about 10 000
components, and columns left unsorted inside the rows.

NOT exercised: node ids above 2^32 (parent alone would be 32 GiB) and rowptr values above 2^31 (a
matrix of that many entries cannot be allocated and filled in a few seconds).  The grids are not
capped, so there is no second trip to drive.

The file name sorts behind every other GPU file on purpose: the new tests are collected last."""
import numpy as np
import pytest
import torch

import components_ref as cr
from test_weighted_walk_gpu import adj_of, gpu

pytestmark = pytest.mark.gpu

_ADJ = {}
POISON = -(2**61) - 5


def case_adj(name):
    if name not in _ADJ:
        N, rowptr, _, col = cr.case_graph(name)
        _ADJ[name] = adj_of(rowptr, col, N=N)
    return _ADJ[name]


def same(got, want):
    assert got.dtype == torch.int64 and got.is_cuda
    return np.array_equal(got.cpu().numpy(), want)


def poisoned(n):
    return torch.full((n,), POISON, dtype=torch.int64, device="cuda")


# ---- the case table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.CASES)
def test_case_table_bit_exact(name):
    import paddle_sparse_amd as psa

    N = cr.case_graph(name)[0]
    want_n, want, _, _ = cr.case_ref(name)
    adj = case_adj(name)
    for n, labels in (psa.connected_components(adj), adj.connected_components(), adj.connected_components("weak")):
        assert type(n) is int and n == want_n
        assert tuple(labels.shape) == (N,) and same(labels, want)


@pytest.mark.parametrize("name", cr.CASES)
def test_raw_ops_overwrite_poisoned_outputs(name):
    from paddle_sparse_amd import ops

    N, _, _, _ = cr.case_graph(name)
    root_want = cr.case_ref(name)[2]
    adj = case_adj(name)
    rowptr, col, _ = adj.csr()
    parent = ops.components_init(rowptr, col, out=poisoned(N))
    first = parent.cpu().numpy()
    assert ((first >= 0) & (first <= np.arange(N))).all()
    flags = ops.components_hook(adj.storage.row(), col, parent)
    root, is_root = ops.components_flatten(parent, out_root=poisoned(N), out_is_root=poisoned(N))
    assert flags.tolist() == [0] and same(root, root_want)
    assert same(is_root, (root_want == np.arange(N)).astype(np.int64))
    after = parent.cpu().numpy()
    assert ((after >= 0) & (after <= np.arange(N))).all() and np.array_equal(root_want[after], root_want)


@pytest.mark.parametrize("name", ["random", "path_identity", "path_shuffled", "grid", "cliques", "star_hub_last"])
def test_three_runs_give_the_same_bits(name):
    adj = case_adj(name)
    runs = [adj.connected_components() for _ in range(3)]
    assert runs[0][0] == runs[1][0] == runs[2][0] == cr.case_ref(name)[0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])


def test_entries_in_any_order_and_direction():
    """The hook reads a COO pair per lane and asks nothing of its order: the entries as written down,
    shuffled and reversed, over a parent that init left as the identity (rowptr of an empty matrix)."""
    from paddle_sparse_amd import ops

    for name in ("random", "grid", "path_shuffled"):
        N, row, col = cr.case_edges(name)
        p = np.random.default_rng(3).permutation(len(col))
        for r, c in ((row, col), (col[p], row[p])):
            parent = ops.components_init(torch.zeros(N + 1, dtype=torch.int64, device="cuda"), gpu([]))
            assert same(parent, np.arange(N))
            assert ops.components_hook(gpu(r), gpu(c), parent).tolist() == [0]
            assert same(ops.components_flatten(parent)[0], cr.case_ref(name)[2])


def test_empty_matrices():
    adj = case_adj("size_0_0")
    n, labels = adj.connected_components()
    assert n == 0 and type(n) is int and tuple(labels.shape) == (0,) and labels.dtype == torch.int64 and labels.is_cuda
    sub, n_id, e_id = adj.largest_connected_components()
    assert sub.sparse_sizes() == (0, 0) and n_id.numel() == 0 and e_id.numel() == 0
    n, labels = case_adj("no_edges").connected_components()
    assert n == 70 and labels.tolist() == list(range(70))


def test_values_do_not_matter_and_an_explicit_zero_is_an_edge():
    N, rowptr, _, col = cr.case_graph("triangles")
    value = torch.zeros(len(col), device="cuda")
    n, labels = adj_of(rowptr, col, value=value, N=N).connected_components()
    assert (n, labels.tolist()) == cr.TINY["triangles"]


# ---- largest_connected_components -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["triangles", "random", "size_1000_257", "unsorted", "cliques"])
@pytest.mark.parametrize("k", [1, 2, 10**6])
def test_largest_is_saint_subgraph_of_the_reference_nodes(name, k):
    import paddle_sparse_amd as psa

    N = cr.case_graph(name)[0]
    n, labels, _, _ = cr.case_ref(name)
    want = cr.ref_largest(n, labels, k)
    if k > n:
        assert np.array_equal(want, np.arange(N))
    adj = case_adj(name)
    ref_sub, ref_e = adj.saint_subgraph(gpu(want))
    for sub, n_id, e_id in (psa.largest_connected_components(adj, k), adj.largest_connected_components(k)):
        assert same(n_id, want) and torch.equal(e_id, ref_e) and e_id.dtype == torch.int64
        assert sub.sparse_sizes() == ref_sub.sparse_sizes() == (len(want), len(want))
        assert torch.equal(sub.storage.row(), ref_sub.storage.row())
        assert torch.equal(sub.storage.col(), ref_sub.storage.col())
        assert torch.equal(sub.storage.rowptr(), ref_sub.storage.rowptr())
    if k == 1:  # the default, and the largest component is connected
        assert same(adj.largest_connected_components()[1], want)
        assert sub.connected_components()[0] == 1


def test_largest_tie_goes_to_the_smaller_label():
    adj = case_adj("triangles")  # {1, 3, 8} and {2, 6, 7}
    sub, n_id, e_id = adj.largest_connected_components(1)
    assert n_id.tolist() == [1, 3, 8] and sub.nnz() == 3
    N, _, row, col = cr.case_graph("triangles")
    assert sorted(zip(row[e_id.cpu().numpy()].tolist(), col[e_id.cpu().numpy()].tolist())) == [(1, 3), (3, 8), (8, 1)]
    assert adj.largest_connected_components(2)[1].tolist() == [1, 2, 3, 6, 7, 8]
    assert adj.largest_connected_components(3)[1].tolist() == [0, 1, 2, 3, 6, 7, 8]
    # every component of the matching has two nodes: the one that holds node 0 wins
    n_id = case_adj("matching").largest_connected_components()[1]
    labels = cr.case_ref("matching")[1]
    assert n_id.tolist() == np.flatnonzero(labels == 0).tolist() and n_id[0].item() == 0 and n_id.numel() == 2


def test_values_follow_the_kept_entries():
    N, rowptr, _, col = cr.case_graph("size_1000_257")
    value = torch.arange(len(col), device="cuda", dtype=torch.float32)
    sub, n_id, e_id = adj_of(rowptr, col, value=value, N=N).largest_connected_components(2)
    assert torch.equal(sub.storage.value(), value[e_id])


# ---- errors ------------------------------------------------------------------------------------------------
def test_errors():
    import paddle_sparse_amd as psa

    adj = case_adj("triangles")
    rect = adj_of(np.array([0, 1, 2]), np.array([0, 2]), N=3)
    with pytest.raises(ValueError, match="square"):
        rect.connected_components()
    with pytest.raises(ValueError, match="square"):
        psa.largest_connected_components(rect)
    with pytest.raises(NotImplementedError, match="strong"):
        adj.connected_components(connection="strong")
    with pytest.raises(ValueError, match="connection"):
        adj.connected_components(connection="feeble")
    for k in (0, -1):
        with pytest.raises(ValueError, match="num_components"):
            adj.largest_connected_components(k)
    with pytest.raises(TypeError):
        psa.connected_components(torch.zeros(3, 3))


@pytest.mark.parametrize("bad", [10, -1, 2**62, -2**63])
def test_a_column_outside_the_matrix_is_skipped_and_flagged(bad):
    from paddle_sparse_amd import ops

    N, rowptr, row, col = cr.case_graph("triangles")
    want = cr.case_ref("triangles")[2]
    at, ptr = rowptr[4], rowptr.copy()  # the first and only entry of row 4, where init reads it too
    ptr[5:] += 1
    r, c = np.insert(row, at, 4), np.insert(col, at, bad)
    parent = ops.components_init(gpu(ptr), gpu(c), out=poisoned(N))
    flags = ops.components_hook(gpu(r), gpu(c), parent)
    root, _ = ops.components_flatten(parent)
    assert flags.tolist() == [cr.RANGE] and same(root, want)
    # a bad row (no storage can hold one; the raw op still must not write through it)
    parent = ops.components_init(gpu(rowptr), gpu(col))
    assert ops.components_hook(gpu(np.r_[row, bad]), gpu(np.r_[col, 5]), parent).tolist() == [cr.RANGE]
    assert same(ops.components_flatten(parent)[0], want)
    with pytest.raises(IndexError, match="connected_components"):
        adj_of(ptr, c, N=N).connected_components()
    with pytest.raises(IndexError):
        adj_of(ptr, c, N=N).largest_connected_components()


# ---- the operand is left as it was ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["size_1000_1000", "grid"])
def test_the_operand_is_not_mutated(name):
    from test_storage_invariants_gpu import audit, present

    N, rowptr, row, col = cr.case_graph(name)
    value = torch.arange(len(col), device="cuda", dtype=torch.float32)
    adj = adj_of(rowptr, col, value=value.clone(), N=N)
    adj.connected_components()
    sub, n_id, e_id = adj.largest_connected_components(2)
    st = adj.storage
    assert same(st.rowptr(), rowptr) and same(st.row(), row) and same(st.col(), col) and torch.equal(st.value(), value)
    assert present(st) == frozenset()  # no cache beyond the row / rowptr views was filled
    audit(adj, present(st), f"{name} after both calls", check_ref=False, run_downstream=False)
    audit(sub, present(sub.storage), f"{name}: the subgraph", check_ref=False, run_downstream=False)
