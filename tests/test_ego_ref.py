"""CPU suite for ego_k_hop_sample: the serial restatement of tests/ego_ref.py (the GPU suite
compares the kernels with it bit for bit) against known answers, against the sample_adj
oracle for one hop and against a BFS ball with scipy's induced subgraph for all -1 fan-outs;
plus the public surface and the C-ABI entry points.  No kernel runs.

Known answers derived by hand on the 6-node graph of test_walk_saint.py (rows 0: [1, 2],
1: [0, 2], 2: [0, 1, 3], 3: [2, 4], 4: [3], 5: []; entries e0 .. e9 in that order).
  k = -1   seeds [4, 5], [-1, -1]: ego 0 reaches 3, then 2 and 4: nodes {2, 3, 4}; ego 1 is
           the isolated node 5.  Node 2 keeps (2, 3) = e6 only, node 3 both entries, node 4 e9.
  Floyd    seeds [5, 5, 5, 2], [2], seed 7: node 2 sits at walk index 3 and has 3 > 2 entries.
           Floyd's first step draws from [0, 1), which is e4; the second draws from [0, 2): the
           draw of stream 3 under seed 7 is 0 (the value test_neighbor_ref.py pins for the same
           stream), collides with e4 and gives e6.  Nodes {0, 2, 3}: node 0 keeps (0, 2) = e1,
           node 2 keeps e4 and e6, node 3 keeps (3, 2) = e7.  The three egos of node 5 are
           three rows of their own.
  twice    seeds [3, 3], [1], replace, seed 7: streams 0 and 1 draw 0 and 1 from [0, 2) (the
           values of randint, pinned against the C oracle in test_walk_saint.py), so ego 0 is
           {2, 3} and ego 1 is {3, 4}: the same seed, two different egos."""
import ctypes

import numpy as np
import pytest
import torch

from ego_ref import ego_k_hop_sample_ref, ego_walk_ref
from test_walk_saint import KAT_COL, KAT_ROWPTR, randint
from util import random_csr

SYMBOLS = ("psa_ego_set_threshold", "psa_ego_init", "psa_ego_hop_count", "psa_ego_hop_pick", "psa_ego_induce_count",
           "psa_ego_total", "psa_ego_induce_write")

# (seeds, fan-outs, replace, seed) -> (n_id, ptr, root, rowptr', col', e_id)
KAT_EGO = [
    (([4, 5], [-1, -1], False, 0),
     ([2, 3, 4, 5], [0, 3, 4], [2, 3], [0, 1, 3, 4, 4], [1, 0, 2, 1], [6, 7, 8, 9])),
    (([5, 5, 5, 2], [2], False, 7),
     ([5, 5, 5, 0, 2, 3], [0, 1, 2, 3, 6], [0, 1, 2, 4], [0, 0, 0, 0, 1, 3, 4], [4, 3, 5, 4], [1, 4, 6, 7])),
    (([3, 3], [1], True, 7),
     ([2, 3, 3, 4], [0, 2, 4], [1, 2], [0, 1, 2, 3, 4], [1, 0, 3, 2], [6, 7, 8, 9])),
]


@pytest.mark.parametrize("args,want", KAT_EGO)
def test_restatement_known_answers(args, want):
    seeds, fanouts, replace, seed = args
    got = ego_k_hop_sample_ref(KAT_ROWPTR, KAT_COL, seeds, fanouts, replace, seed)
    assert tuple(x.tolist() for x in got) == want


def test_the_draws_the_known_answers_lean_on():
    assert randint(7, 3, 1, 2) == 0 and [randint(7, i, 0, 2) for i in (0, 1)] == [0, 1]


def test_empty_slots_keep_their_index():
    """[2, 1] from node 4 (one entry): hop 1 has 2 slots, the second empty; hop 2 has one slot
    per slot of hop 1 and the child of the empty one is empty.  Stream = walk index."""
    hops = ego_walk_ref(KAT_ROWPTR, KAT_COL, [4], [2, 1], False, 3)
    assert hops[0] == [(4, 0)] and hops[1] == [(3, 0), (-1, 0)]
    assert len(hops[2]) == 2 and hops[2][1] == (-1, 0)
    assert hops[2][0] == (2, 0)  # node 3 at walk index 1: Floyd with k = 1 over deg 2 draws from [0, 1), e7
    assert ego_walk_ref(KAT_ROWPTR, KAT_COL, [4], [2, 0, 5], False, 3) == hops[:2]
    assert ego_walk_ref(KAT_ROWPTR, KAT_COL, [4], [], False, 3) == hops[:1]


@pytest.mark.parametrize("graph_seed", [1, 2, 3])
def test_one_hop_is_sample_adj(graph_seed):
    """[k]: ego g's node set is {seeds[g]} joined with the columns oracle.sample_adj picks for row g."""
    import oracle

    _, rowptr, col, _ = random_csr(400, 400, 2500, seed=graph_seed, sort_cols=True)
    seeds = np.random.default_rng(graph_seed).permutation(400)[:37]
    for k in (-1, 1, 3, 7, 12):
        for replace in (False, True):
            for seed in (0, 12345, 2**63 + 11):
                out_rowptr, _, _, e_id = oracle.sample_adj(rowptr, col, seeds, k, replace, seed, num_nodes=400)
                n_id, ptr, root, _, _, _ = ego_k_hop_sample_ref(rowptr, col, seeds, [k], replace, seed)
                for g, s in enumerate(seeds):
                    want = sorted({int(s)} | set(col[e_id[out_rowptr[g]:out_rowptr[g + 1]]].tolist()))
                    assert n_id[ptr[g]:ptr[g + 1]].tolist() == want, (k, replace, seed, g)
                    assert n_id[root[g]] == s and ptr[g] <= root[g] < ptr[g + 1]


@pytest.mark.parametrize("L", [1, 2, 3])
def test_all_entries_is_the_bfs_ball_and_scipys_induced_subgraph(L):
    import scipy.sparse as sp

    row, rowptr, col, _ = random_csr(300, 300, 700, seed=L, sort_cols=True)
    keep = np.concatenate([[True], (row[1:] != row[:-1]) | (col[1:] != col[:-1])])  # scipy sums duplicates
    row, col = row[keep], col[keep]
    rowptr = np.searchsorted(row, np.arange(301), side="left").astype(np.int64)
    A = sp.csr_matrix((np.arange(1, len(col) + 1), col, rowptr), shape=(300, 300))  # data = e + 1
    seeds = np.array([7, 250, 7, 13, 299, 0])
    n_id, ptr, root, p, c, e = ego_k_hop_sample_ref(rowptr, col, seeds, [-1] * L)
    assert p[-1] == len(c) == len(e) and len(p) == len(n_id) + 1
    for g, s in enumerate(seeds):
        ball, frontier = {int(s)}, {int(s)}
        for _ in range(L):
            frontier = {int(x) for v in frontier for x in col[rowptr[v]:rowptr[v + 1]]} - ball
            ball |= frontier
        ball = np.array(sorted(ball))
        assert np.array_equal(n_id[ptr[g]:ptr[g + 1]], ball) and n_id[root[g]] == s
        B = A[ball][:, ball].tocsr()
        B.sort_indices()
        lo, hi = p[ptr[g]], p[ptr[g + 1]]
        assert np.array_equal(p[ptr[g]:ptr[g + 1] + 1] - lo, B.indptr)
        assert np.array_equal(c[lo:hi] - ptr[g], B.indices) and np.array_equal(e[lo:hi] + 1, B.data)


def test_restatement_rejects_seeds_outside():
    for bad in (-1, 6):
        with pytest.raises(IndexError):
            ego_k_hop_sample_ref(KAT_ROWPTR, KAT_COL, [1, bad], [2])


# ---- the surface ---------------------------------------------------------------------
def test_the_op_is_exported_attached_and_bound():
    from test_abi import declared_functions

    import paddle_sparse_amd as psa
    from paddle_sparse_amd import SparseTensor, _lib, ego

    assert "ego_k_hop_sample" in psa.__all__ and psa.ego_k_hop_sample is ego.ego_k_hop_sample
    assert SparseTensor.ego_k_hop_sample is ego.ego_k_hop_sample
    declared = declared_functions()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert sorted(n for n in declared if n.startswith("psa_ego_")) == sorted(SYMBOLS)
    # scratch is plain typed buffers: the op adds no workspace-size function
    assert not [n for n in list(declared) + list(_lib.SIGNATURES) if n.endswith("_workspace_bytes") and "ego" in n]
    loaded = _lib.load()
    assert loaded.psa_ego_set_threshold(32) == 32  # the default; no kernel runs


def _cpu_csr(M=3, N=3):
    from paddle_sparse_amd import SparseTensor

    return SparseTensor(rowptr=torch.tensor([0, 2, 3, 3]), col=torch.tensor([0, 2, 1]), value=torch.ones(3),
                        sparse_sizes=(M, N), is_sorted=True, trust_data=True)


def test_bad_arguments_raise_before_any_launch():
    import paddle_sparse_amd as psa

    with pytest.raises(ValueError, match="square"):
        psa.ego_k_hop_sample(_cpu_csr(3, 4), torch.tensor([0]), [2])
    a = _cpu_csr()
    with pytest.raises(TypeError):
        a.ego_k_hop_sample(torch.tensor([0.0]), [2])
    with pytest.raises(ValueError):
        a.ego_k_hop_sample(torch.tensor([[0]]), [2])
    with pytest.raises(ValueError):
        a.ego_k_hop_sample(torch.tensor([0]), [2, -2])
    with pytest.raises(TypeError):
        a.ego_k_hop_sample(torch.tensor([0]), 2)
    with pytest.raises(TypeError):
        a.ego_k_hop_sample(torch.tensor([0]), [2, True])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        a.ego_k_hop_sample(torch.tensor([0, 1]), [2], seed=1)


def test_entry_points_refuse_short_buffers_and_bad_sizes():
    """Argument checks run before any launch, so they can be called without a GPU."""
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    codes = [
        lib.psa_ego_init(p, 8, 10, p, p, p, 7, p, None),                       # out_count < S
        lib.psa_ego_init(p, 2**31, 10, p, p, p, 2**31, p, None),               # S out of range
        lib.psa_ego_init(p, 2**30, 2**33, p, p, p, 2**30, p, None),            # S * N >= 2^62
        lib.psa_ego_hop_count(p, 10, p, 8, p, 7, None),                        # counts short
        lib.psa_ego_hop_pick(p, p, 10, p, 4, p, p, 4, None, 0, 2, 0, 0, 8, p, p, p, 7, p, None),   # out_count < slots
        lib.psa_ego_hop_pick(p, p, 10, p, 4, p, p, 4, None, 0, 2, 0, 0, 9, p, p, p, 9, p, None),   # slots != F * k
        lib.psa_ego_hop_pick(p, p, 10, p, 4, p, p, 4, None, 0, -1, 0, 0, 9, p, p, p, 9, p, None),  # k < 0 without ptr
        lib.psa_ego_hop_pick(p, p, 10, p, 4, p, p, 4, None, 0, 2**31, 0, 0, 2**33, p, p, p, 2**33, p, None),
        lib.psa_ego_induce_count(p, p, 10, p, 4, p, p, p, 8, p, 3, p, 8, None),                   # root short
        lib.psa_ego_induce_count(p, p, 10, p, 4, p, p, p, 8, p, 4, p, 7, None),                   # counts short
        lib.psa_ego_induce_write(p, p, 10, 4, p, p, p, 8, p, 5, p, p, 4, None),                   # outputs short
    ]
    assert all(c == 1 for c in codes), codes  # PSA_ERR_INVALID_ARG
