"""CPU suite for connected components: the serial restatement of tests/components_ref.py against hand
answers and scipy, and the host export psa_components_host (the kernels' own steps of
csrc/union_find.h, run serially) against the restatement, bit for bit, on the whole case table.
No GPU is needed."""
import numpy as np
import pytest
import scipy.sparse
from scipy.sparse.csgraph import connected_components as scipy_components

import components_ref as cr


def host(N, rowptr, row, col):
    from paddle_sparse_amd import ops

    return ops.components_host(rowptr, row, col)


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cr.TINY))
def test_restatement_hand_answers(name):
    n, labels, root, flags = cr.case_ref(name)
    want_n, want = cr.TINY[name]
    assert (n, labels.tolist(), flags) == (want_n, want, 0)
    # the root of every node is the smallest node of its component
    for c in range(n):
        assert (root[labels == c] == np.flatnonzero(labels == c).min()).all()


@pytest.mark.parametrize("name", cr.CASES)
def test_restatement_is_scipy(name):
    N, _, row, col = cr.case_graph(name)
    n, labels, root, flags = cr.case_ref(name)
    assert flags == 0 and labels.shape == (N,) and labels.dtype == np.int64
    if N == 0:
        assert n == 0  # scipy refuses a 0 x 0 matrix
        return
    graph = scipy.sparse.csr_matrix((np.zeros(len(col)), (row, col)), shape=(N, N))  # explicit zeros are edges
    want_n, want = scipy_components(graph, directed=True, connection="weak")
    assert n == want_n and np.array_equal(labels, want)
    assert np.array_equal(root, np.flatnonzero(root == np.arange(N))[labels])


@pytest.mark.parametrize("name", cr.CASES)
def test_restatement_does_not_depend_on_the_entry_order(name):
    N, row, col = cr.case_edges(name)
    n, labels, root, _ = cr.case_ref(name)
    p = np.random.default_rng(5).permutation(len(col))
    got = cr.ref_components(N, row[p], col[p])
    assert got[0] == n and np.array_equal(got[1], labels) and np.array_equal(got[2], root)
    got = cr.ref_components(N, col, row)  # nor on the direction of the entries
    assert got[0] == n and np.array_equal(got[1], labels)


# ---- the host export ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.CASES)
def test_host_export_is_the_restatement(name):
    N, rowptr, row, col = cr.case_graph(name)
    n, labels, root, _ = cr.case_ref(name)
    parent, got_root, is_root, flags = host(N, rowptr, row, col)
    assert flags == 0
    assert np.array_equal(got_root, root) and np.array_equal(is_root, (root == np.arange(N)).astype(np.int64))
    assert (parent <= np.arange(N)).all() and (parent >= 0).all()  # written everywhere, parent[x] <= x
    rank = np.concatenate([[0], np.cumsum(is_root)])
    assert rank[N] == n and np.array_equal(rank[got_root], labels)
    # the entries as written down (any order; rowptr of the stored order only seeds parent)
    _, erow, ecol = cr.case_edges(name)
    assert np.array_equal(host(N, np.zeros(N + 1, np.int64), erow, ecol)[1], root)


def test_host_export_skips_and_flags_an_entry_outside_the_matrix():
    N, rowptr, row, col = cr.case_graph("triangles")
    want = cr.case_ref("triangles")[2]
    for bad in (N, -1, 2**62, -2**63):
        # a bad row behind the last entry (no rowptr can describe it), next to a column that would join 4 and 5
        r, c, ptr = np.r_[row, bad], np.r_[col, 5], rowptr
        ref = cr.ref_components(N, r, c)
        assert ref[3] == cr.RANGE and np.array_equal(ref[2], want)
        _, root, _, flags = host(N, ptr, r, c)
        assert flags == cr.RANGE and np.array_equal(root, want), bad
        # a bad column as the first and only entry of row 4, where init reads it
        at, ptr = rowptr[4], rowptr.copy()
        ptr[5:] += 1
        r, c = np.insert(row, at, 4), np.insert(col, at, bad)
        assert np.array_equal(np.searchsorted(r, np.arange(N + 1)), ptr)
        ref = cr.ref_components(N, r, c)
        assert ref[3] == cr.RANGE and np.array_equal(ref[2], want)
        parent, root, _, flags = host(N, ptr, r, c)
        assert flags == cr.RANGE and np.array_equal(root, want) and parent[4] == 4, bad
    # a rowptr that points outside col reads nothing
    wild = np.full(N + 1, 2**40, np.int64)
    assert np.array_equal(host(N, wild, row, col)[1], want)
    assert np.array_equal(host(N, -wild, row, col)[1], want)


def test_argument_checks_of_the_entry_points():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    OK, INVALID = 0, 1
    a = np.zeros(8, np.int64).ctypes.data
    assert lib.psa_components_host(a, a, a, 3, 2, a, a, a, a) == OK
    assert lib.psa_components_host(a, a, a, -1, 2, a, a, a, a) == INVALID
    assert b"psa_components_host" in lib.psa_last_error()
    assert lib.psa_components_host(a, a, a, 3, -1, a, a, a, a) == INVALID
    assert lib.psa_components_host(None, a, a, 3, 2, a, a, a, a) == INVALID
    assert lib.psa_components_host(a, a, a, 3, 2, a, None, a, a) == INVALID
    assert lib.psa_components_host(a, a, a, 3, 2, a, a, a, None) == INVALID
    assert lib.psa_components_host(None, None, None, 0, 0, None, None, None, None) == OK
    # the device forms refuse before anything is launched; a zero count is nothing to do
    assert lib.psa_components_init(None, None, 3, 2, None, None) == INVALID
    assert lib.psa_components_init(1, 1, -1, 2, 1, None) == INVALID
    assert lib.psa_components_init(1, 1, 3, -2, 1, None) == INVALID
    assert lib.psa_components_init(None, None, 0, 0, None, None) == OK
    assert lib.psa_components_hook(None, None, 2, 3, None, None, None) == INVALID
    assert lib.psa_components_hook(1, 1, -2, 3, 1, 1, None) == INVALID
    assert lib.psa_components_hook(1, 1, 2, -3, 1, 1, None) == INVALID
    assert lib.psa_components_hook(None, None, 0, 3, None, None, None) == OK
    assert lib.psa_components_flatten(None, 3, None, None, None) == INVALID
    assert lib.psa_components_flatten(1, -3, 1, 1, None) == INVALID
    assert b"psa_components_flatten" in lib.psa_last_error()
    assert lib.psa_components_flatten(None, 0, None, None, None) == OK
    assert lib.psa_components_init(1, 1, 2**40, 2, 1, None) == INVALID  # more than 2^31 - 1 workgroups
    assert b"too many nodes" in lib.psa_last_error()


# ---- the selection of largest_connected_components ------------------------------------------------------
def test_largest_selection_hand_answers_with_a_tie():
    n, labels, _, _ = cr.case_ref("triangles")  # {1, 3, 8} (label 1) and {2, 6, 7} (label 2) tie at 3 nodes
    assert cr.ref_largest(n, labels, 1).tolist() == [1, 3, 8]
    assert cr.ref_largest(n, labels, 2).tolist() == [1, 2, 3, 6, 7, 8]
    assert cr.ref_largest(n, labels, 3).tolist() == [0, 1, 2, 3, 6, 7, 8]  # then the isolated nodes, by label
    assert cr.ref_largest(n, labels, 99).tolist() == list(range(10))


@pytest.mark.parametrize("name", ["random", "size_1000_257", "matching", "triangles", "unsorted"])
@pytest.mark.parametrize("k", [1, 2, 7])
def test_largest_selection_is_the_numpy_statement(name, k):
    """The ranking that components.py builds from torch ops, run on the CPU: the same node set as the
    (-size, label) ordering."""
    import torch

    from paddle_sparse_amd.components import _nodes_of_largest

    n, labels, _, _ = cr.case_ref(name)
    t = torch.from_numpy(labels.copy())
    got = _nodes_of_largest(torch.bincount(t, minlength=n), t, k).numpy()
    want = cr.ref_largest(n, labels, k)
    assert np.array_equal(got, want)
    if name == "matching":  # every component has two nodes: the smallest labels win
        assert sorted(set(labels[want].tolist())) == list(range(k))


# ---- the public surface, and the errors raised before anything runs on the GPU ---------------------------
def test_the_public_surface():
    import paddle_sparse_amd as psa

    for name in ("connected_components", "largest_connected_components"):
        assert name in psa.__all__ and getattr(psa, name) is getattr(psa.components, name)
        assert getattr(psa.SparseTensor, name) is getattr(psa, name)
        assert "capturable" in getattr(psa, name).__doc__


def test_argument_errors_need_no_gpu():
    import torch
    import paddle_sparse_amd as psa

    def cpu_adj(M, N):
        return psa.SparseTensor(rowptr=torch.arange(M + 1), col=torch.arange(M), sparse_sizes=(M, N), is_sorted=True,
                                trust_data=True)

    for f in (psa.connected_components, psa.largest_connected_components):
        with pytest.raises(TypeError, match="SparseTensor"):
            f(torch.zeros(3, 3))
        with pytest.raises(ValueError, match="square"):
            f(cpu_adj(4, 5))
    with pytest.raises(NotImplementedError, match="strong"):
        cpu_adj(4, 4).connected_components(connection="strong")
    with pytest.raises(ValueError, match="connection"):
        cpu_adj(4, 4).connected_components("feeble")
    for k in (0, -3):
        with pytest.raises(ValueError, match="num_components"):
            cpu_adj(4, 4).largest_connected_components(k)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path
        cpu_adj(4, 4).connected_components()
