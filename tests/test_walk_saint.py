"""CPU suite for random_walk and saint_subgraph: a restatement of both ops in numpy (the
GPU suite compares the kernels with it bit for bit), pinned to hand-checked known
answers, and the public surface / C-ABI entry points.  No kernel runs."""
import ctypes

import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1
SYMBOLS = ("psa_random_walk", "psa_random_walk_set_variant", "psa_saint_workspace_bytes", "psa_saint_count",
           "psa_saint_write")


# ---- the semantics, restated -------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def randint(seed, i, t, n):
    """Draw t of stream i in [0, n): csrc/rng.h (the stream of sample_adj)."""
    r = mix64((mix64((seed & M64) ^ mix64(i & M64)) + t) & M64)
    return (r * n) >> 64


def ref_random_walk(rowptr, col, start, L, seed):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    out = np.empty((len(start), L + 1), np.int64)
    for n, cur in enumerate(np.asarray(start, np.int64).tolist()):
        out[n, 0] = cur
        for l in range(L):
            s, deg = int(rowptr[cur]), int(rowptr[cur + 1] - rowptr[cur])
            if deg > 0:
                cur = int(col[s + randint(seed, n, l, deg)])
            out[n, l + 1] = cur
    return out


def ref_saint_candidates(rowptr, col, node_idx, N):
    """torch_sparse's CPU text: (row', col', edge) in candidate order."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    assoc = np.full(N, -1, np.int64)
    for i, v in enumerate(np.asarray(node_idx, np.int64).tolist()):
        assoc[v] = i  # the last duplicate wins
    rows, cols, edges = [], [], []
    for i, v in enumerate(np.asarray(node_idx, np.int64).tolist()):
        for e in range(int(rowptr[v]), int(rowptr[v + 1])):
            if assoc[col[e]] >= 0:
                rows.append(i)
                cols.append(int(assoc[col[e]]))
                edges.append(e)
    return np.array(rows, np.int64), np.array(cols, np.int64), np.array(edges, np.int64)


def ref_saint_subgraph(rowptr, col, node_idx, N):
    """(rowptr', col', edge_index) sorted by (row', col'), ties in candidate order."""
    row, c, e = ref_saint_candidates(rowptr, col, node_idx, N)
    order = np.lexsort((c, row))  # stable
    S = len(node_idx)
    new_rowptr = np.searchsorted(row[order], np.arange(S + 1), side="left").astype(np.int64)
    return new_rowptr, c[order], e[order]


# ---- known answers -----------------------------------------------------------------
KAT_ROW = [0, 0, 1, 1, 2, 2, 2, 3, 3, 4]
KAT_COL = [1, 2, 0, 2, 0, 1, 3, 2, 4, 3]
KAT_ROWPTR = [0, 2, 4, 7, 9, 10, 10]
KAT_N = 6
KAT_WALK = dict(start=[0, 2, 4, 5, 3], L=5, seed=12345,
                out=[[0, 1, 0, 2, 1, 0], [2, 0, 1, 2, 0, 2], [4, 3, 2, 0, 1, 2], [5, 5, 5, 5, 5, 5],
                     [3, 2, 1, 0, 1, 0]])
KAT_SAINT = [
    ([0, 1, 2], [0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [0, 1, 2, 3, 4, 5]),
    ([2, 1, 0], [0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [5, 4, 3, 2, 1, 0]),
    ([2, 0, 2], [0, 1, 2, 3], [1, 2, 1], [4, 1, 4]),
    ([5, 4, 3], [0, 0, 1, 2], [2, 1], [9, 8]),
]


def test_kat_graph_is_the_stated_csr():
    assert np.searchsorted(KAT_ROW, np.arange(KAT_N + 1), side="left").tolist() == KAT_ROWPTR


def test_random_walk_restatement_kat():
    k = KAT_WALK
    assert ref_random_walk(KAT_ROWPTR, KAT_COL, k["start"], k["L"], k["seed"]).tolist() == k["out"]


@pytest.mark.parametrize("node_idx,rowptr,col,edge", KAT_SAINT)
def test_saint_subgraph_restatement_kat(node_idx, rowptr, col, edge):
    p, c, e = ref_saint_subgraph(KAT_ROWPTR, KAT_COL, node_idx, KAT_N)
    assert p.tolist() == rowptr and c.tolist() == col and e.tolist() == edge


def test_walk_step_zero_is_sample_adjs_pick():
    """Step 0 of walk n draws what sample_adj(start, 1, replace=True, seed) draws for
    subset row n: the C oracle of sample_adj agrees with the restatement."""
    import oracle

    k = KAT_WALK
    start = np.array([s for s in k["start"] if KAT_ROWPTR[s + 1] > KAT_ROWPTR[s]], np.int64)
    res = oracle.sample_adj(np.array(KAT_ROWPTR, np.int64), np.array(KAT_COL, np.int64), start, 1, True,
                            k["seed"])
    walk = ref_random_walk(KAT_ROWPTR, KAT_COL, start, 1, k["seed"])
    e_id = res[3]  # one pick per row: storage order is row order
    assert np.array(KAT_COL)[e_id].tolist() == walk[:, 1].tolist()


def test_unsorted_restatement_is_a_relabelled_permutation():
    """For a permutation p, the subgraph is A[p][:, p]."""
    rng = np.random.default_rng(0)
    N = 40
    row = np.sort(rng.integers(0, N, 300))
    col = rng.integers(0, N, 300)
    order = np.lexsort((col, row))
    row, col = row[order], col[order]
    rowptr = np.searchsorted(row, np.arange(N + 1), side="left")
    p = rng.permutation(N)
    dense = np.zeros((N, N), np.int64)
    np.add.at(dense, (row, col), 1)
    sp, sc, se = ref_saint_subgraph(rowptr, col, p, N)
    sub = np.zeros((N, N), np.int64)
    np.add.at(sub, (np.repeat(np.arange(N), np.diff(sp)), sc), 1)
    assert np.array_equal(sub, dense[p][:, p])
    assert np.array_equal(row[se], p[np.repeat(np.arange(N), np.diff(sp))]) and np.array_equal(col[se], p[sc])


# ---- the surface ---------------------------------------------------------------------
def test_both_ops_are_exported_attached_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, rw, saint

    assert "random_walk" in psa.__all__ and psa.random_walk is rw.random_walk
    assert "saint_subgraph" in psa.__all__ and psa.saint_subgraph is saint.saint_subgraph
    assert callable(SparseTensor.random_walk) and callable(SparseTensor.saint_subgraph)
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().psa_saint_workspace_bytes(1000, 5000) >= 8 * (5000 + 2 * 1000)


def _cpu_csr(M=3, N=3):
    from paddle_sparse_amd import SparseTensor

    rowptr = torch.tensor([0, 2, 3, 3])
    col = torch.tensor([0, 2, 1])
    return SparseTensor(rowptr=rowptr, col=col, value=torch.ones(3), sparse_sizes=(M, N), is_sorted=True,
                        trust_data=True)


def test_the_ops_reject_cpu_tensors():
    import paddle_sparse_amd as psa

    a = _cpu_csr()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.random_walk(a, torch.tensor([0, 1]), 3, seed=1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.saint_subgraph(a, torch.tensor([0, 1]))


def test_non_square_and_bad_arguments_raise_before_any_launch():
    import paddle_sparse_amd as psa

    a = _cpu_csr(3, 4)
    with pytest.raises(ValueError, match="square"):
        psa.random_walk(a, torch.tensor([0]), 2, seed=1)
    with pytest.raises(ValueError, match="square"):
        psa.saint_subgraph(a, torch.tensor([0]))
    b = _cpu_csr()
    with pytest.raises(TypeError):
        psa.random_walk(b, torch.tensor([0.0]), 2, seed=1)
    with pytest.raises(ValueError):
        psa.random_walk(b, torch.tensor([[0]]), 2, seed=1)
    with pytest.raises(ValueError):
        psa.random_walk(b, torch.tensor([0]), -1, seed=1)
    with pytest.raises(TypeError):
        psa.saint_subgraph(b, torch.tensor([True]))
