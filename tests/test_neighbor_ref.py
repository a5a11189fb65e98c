"""CPU suite for neighbor_sample: the serial restatement of tests/neighbor_ref.py (the GPU
suite compares the kernels with it bit for bit) against known answers, against the
sample_adj oracle for one hop, and its hop structure; plus the public surface and the
C-ABI entry points.  No kernel runs.

Known answers derived by hand: the fourth (fan-out -1, no draws) in full.  The second
(seeds [0, 5], [2, 2]) in full but for the value of one draw: node 0 and node 1 have 2 <= k
entries and take both, node 5 has none, and node 2 (deg 3 > 2) walks Floyd's two steps, the
first from [0, 1), which is e4, the second from [0, 2), where 0 collides with e4 and gives
e6 (the pinned answer, so the draw is 0) and 1 would give e5.  The first (seed [4],
[1, 1, 1]) likewise: hop 1 takes the only entry, hop 2 is Floyd with k = 1 over deg 2, a
draw from [0, 1), and hop 3 draws once from [0, 2).  The values of the two free draws come
from randint, which test_walk_saint.py pins against the C oracle."""
import ctypes

import numpy as np
import pytest
import torch

from neighbor_ref import neighbor_sample_ref
from test_walk_saint import KAT_COL, KAT_ROWPTR
from util import random_csr

SYMBOLS = ("psa_neighbor_workspace_bytes", "psa_neighbor_hop_workspace_bytes", "psa_neighbor_init",
           "psa_neighbor_hop_count", "psa_neighbor_hop_pick", "psa_neighbor_hop_write", "psa_neighbor_reset")

# (seeds, fan-outs, replace, seed) -> (n_id, rowptr', col', e_id, nodes_per_hop, edges_per_hop)
KAT_NEIGHBOR = [
    (([4], [1, 1, 1], False, 12345),
     ([4, 3, 2, 1], [0, 1, 2, 3, 3], [1, 2, 3], [9, 7, 5], [1, 1, 1, 1], [1, 1, 1])),
    (([0, 5], [2, 2], False, 7),
     ([0, 5, 1, 2, 3], [0, 2, 2, 4, 6, 6], [2, 3, 0, 3, 0, 4], [0, 1, 2, 3, 4, 6], [2, 2, 1], [2, 4])),
    (([3], [2, 2], True, 7),
     ([3, 2], [0, 2, 4], [1, 1, 0, 0], [7, 7, 6, 6], [1, 1, 0], [2, 2])),
    (([5, 1], [-1, -1], False, 0),
     ([5, 1, 0, 2, 3], [0, 0, 2, 4, 7, 7], [2, 3, 1, 3, 1, 2, 4], [2, 3, 0, 1, 5, 4, 6], [2, 2, 1], [2, 5])),
]


def as_lists(res):
    return tuple(np.asarray(x).tolist() if isinstance(x, np.ndarray) else list(x) for x in res)


@pytest.mark.parametrize("args,want", KAT_NEIGHBOR)
def test_restatement_known_answers(args, want):
    seeds, fanouts, replace, seed = args
    assert as_lists(neighbor_sample_ref(KAT_ROWPTR, KAT_COL, seeds, fanouts, replace, seed)) == want


@pytest.mark.parametrize("graph_seed", [1, 2, 3])
def test_one_hop_is_sample_adj(graph_seed):
    """L = 1 against oracle.sample_adj: n_id, e_id, the columns and the first S + 1 pointers."""
    import oracle

    _, rowptr, col, _ = random_csr(400, 400, 2500, seed=graph_seed, sort_cols=True)
    seeds = np.random.default_rng(graph_seed).permutation(400)[:37]
    S = len(seeds)
    for k in (-1, 1, 3, 7, 12):
        for replace in (False, True):
            for seed in (0, 12345, 2**63 + 11):
                out_rowptr, out_col, n_id, e_id = oracle.sample_adj(rowptr, col, seeds, k, replace, seed, num_nodes=400)
                got = neighbor_sample_ref(rowptr, col, seeds, [k], replace, seed)
                assert np.array_equal(got[0], n_id), (k, replace, seed)
                assert np.array_equal(got[1][:S + 1], out_rowptr)
                assert got[1][-1] == out_rowptr[-1]  # rows past the seeds are empty
                assert np.array_equal(got[2], out_col)
                assert np.array_equal(got[3], e_id)


def test_hop_structure():
    """Hop l's entries are the contiguous range given by edges_per_hop, their rows are hop
    l - 1's nodes, and rows past the last frontier are empty."""
    _, rowptr, col, _ = random_csr(3000, 3000, 20000, seed=1, sort_cols=True)
    seeds = np.random.default_rng(5).permutation(3000)[:257]
    n_id, p, c, e, nodes, edges = neighbor_sample_ref(rowptr, col, seeds, [5, 3, 2], False, 99)
    assert nodes[0] == 257 and len(nodes) == 4 and len(edges) == 3 and sum(nodes) == len(n_id)
    assert len(np.unique(n_id)) == len(n_id)
    row = np.repeat(np.arange(len(n_id)), np.diff(p))
    node_lo = np.concatenate([[0], np.cumsum(nodes)])
    edge_lo = np.concatenate([[0], np.cumsum(edges)])
    assert edge_lo[-1] == len(e) == p[-1]
    for hop in range(3):
        r = row[edge_lo[hop]:edge_lo[hop + 1]]
        assert len(r) > 0 and r.min() >= node_lo[hop] and r.max() < node_lo[hop + 1]
        assert c[edge_lo[hop]:edge_lo[hop + 1]].max() < node_lo[hop + 2]
    assert np.all(np.diff(p)[node_lo[3]:] == 0)
    orig_row = np.repeat(np.arange(3000), np.diff(rowptr))
    assert np.array_equal(orig_row[e], n_id[row]) and np.array_equal(np.asarray(col)[e], n_id[c])


def test_zero_fanout_empties_the_later_hops():
    _, rowptr, col, _ = random_csr(300, 300, 3000, seed=4, sort_cols=True)
    n_id, p, c, e, nodes, edges = neighbor_sample_ref(rowptr, col, np.arange(10), [4, 0, 4], False, 1)
    assert nodes[2:] == [0, 0] and edges[1:] == [0, 0] and edges[0] == len(e) > 0
    assert len(n_id) == 10 + nodes[1]
    first = neighbor_sample_ref(rowptr, col, np.arange(10), [4], False, 1)
    assert all(np.array_equal(a, b) for a, b in zip((n_id, p, c, e), first[:4]))


def test_restatement_rejects_bad_seeds():
    with pytest.raises(ValueError):
        neighbor_sample_ref(KAT_ROWPTR, KAT_COL, [1, 2, 1], [2])
    for bad in (-1, 6):
        with pytest.raises(IndexError):
            neighbor_sample_ref(KAT_ROWPTR, KAT_COL, [1, bad], [2])


# ---- the surface ---------------------------------------------------------------------
def test_the_op_is_exported_attached_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, neighbor

    assert "neighbor_sample" in psa.__all__ and psa.neighbor_sample is neighbor.neighbor_sample
    assert "NeighborSampler" in psa.__all__ and psa.NeighborSampler is neighbor.NeighborSampler
    assert SparseTensor.neighbor_sample is neighbor.neighbor_sample
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    loaded = _lib.load()
    assert loaded.psa_neighbor_workspace_bytes(1000) >= 4 * 1000
    assert loaded.psa_neighbor_workspace_bytes(2**31) == 0  # the map holds int32 ids
    assert loaded.psa_neighbor_hop_workspace_bytes(1000) >= 28 * 1000
    assert loaded.psa_neighbor_hop_workspace_bytes(2**31) == 0


def _cpu_csr(M=3, N=3):
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.tensor([0, 2, 3, 3]), col=torch.tensor([0, 2, 1]), value=torch.ones(3),
                        sparse_sizes=(M, N), is_sorted=True, trust_data=True)


def test_bad_arguments_raise_before_any_launch():
    import paddle_sparse_amd as psa

    with pytest.raises(ValueError, match="square"):
        psa.neighbor_sample(_cpu_csr(3, 4), torch.tensor([0]), [2])
    a = _cpu_csr()
    with pytest.raises(TypeError):
        psa.neighbor_sample(a, torch.tensor([0.0]), [2])
    with pytest.raises(ValueError):
        psa.neighbor_sample(a, torch.tensor([[0]]), [2])
    with pytest.raises(ValueError):
        psa.neighbor_sample(a, torch.tensor([0]), [2, -2])
    with pytest.raises(TypeError):
        psa.neighbor_sample(a, torch.tensor([0]), 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        psa.neighbor_sample(a, torch.tensor([0, 1]), [2], seed=1)
