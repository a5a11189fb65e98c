"""GPU suite for the node2vec (p, q) walk (csrc/node2vec.hip).  The walk is index work and
integer compares, so every comparison is bit-exact, on nodes and edge ids, against the serial
restatement of tests/node2vec_ref.py (pinned by test_zz_node2vec_ref.py, which also holds the
kernel's step, run on the host, to it).  The kite statistics carry the CPU suite's bound.

The file name sorts behind every other GPU file on purpose: the new tests are collected last."""
import numpy as np
import pytest
import torch

import node2vec_ref as nr
import weighted_ref as wr
from test_weighted_walk_gpu import adj_of, gpu

pytestmark = pytest.mark.gpu

ONE = nr.ONE
_ADJ = {}


def case_adj(symmetric):
    """(adj with the weights as values, its EdgeCDF, rowptr, col as GPU tensors), made once."""
    import paddle_sparse_amd as psa

    if symmetric not in _ADJ:
        rowptr, col, w, cum = nr.case_graph(symmetric)
        adj = adj_of(rowptr, col, gpu(w, torch.float32))
        cdf = psa.EdgeCDF(adj)
        assert np.array_equal(cdf.cum.cpu().numpy().view(np.int64), cum.view(np.int64))
        _ADJ[symmetric] = (adj, cdf, *adj.csr()[:2])
    return _ADJ[symmetric]


def same(got, want):
    nodes, e_id = got
    assert nodes.dtype == torch.int64 and e_id.dtype == torch.int64
    return np.array_equal(nodes.cpu().numpy(), want[0]) and np.array_equal(e_id.cpu().numpy(), want[1])


# ---- the case table --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(nr.CASES)))
def test_case_table_bit_exact(k):
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    symmetric, S, L, (p, q), mode, edges = nr.CASES[k]
    adj, cdf, rowptr, col = case_adj(symmetric)
    start, seed = gpu(nr.case_start(S)), nr.CASE_SEED + k
    want = nr.case_ref(k)
    if (p, q) == (1, 1):  # the public call would take the existing walk: the new kernel directly
        got = ops.node2vec_walk(rowptr, col, None if mode == "uniform" else cdf.cum, start, L, seed, (ONE,) * 3, 32,
                                edges)
    else:
        weighted = {"uniform": False, "weighted": True, "cdf": cdf}[mode]
        call = adj.random_walk if k % 2 else (lambda *a, **kw: psa.random_walk(adj, *a, **kw))
        got = call(start, L, seed=seed, weighted=weighted, return_edge_ids=edges, p=p, q=q)
    if edges:
        assert tuple(got[0].shape) == (S, L + 1) and tuple(got[1].shape) == (S, L)
        assert same(got, want)
    else:
        assert got.dtype == torch.int64 and tuple(got.shape) == (S, L + 1)
        assert np.array_equal(got.cpu().numpy(), want[0])


# ---- raw thresholds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_raw_thresholds_with_zeros(weighted):
    from paddle_sparse_amd import ops

    _, cdf, rowptr, col = case_adj(True)
    rowptr_np, col_np, _, cum_np = nr.case_graph(True)
    start = nr.case_start(65)
    for thr in ((0, ONE, ONE), (ONE, 0, ONE), (ONE, ONE, 0)):
        for max_tries in (1, 2, 64):
            got = ops.node2vec_walk(rowptr, col, cdf.cum if weighted else None, gpu(start), 9, 3, thr, max_tries, True)
            want = nr.ref_node2vec_walk(rowptr_np, col_np, cum_np if weighted else None, start, 9, 3, thr, max_tries)
            assert same(got, want), (thr, max_tries)


def test_the_path_walk_goes_straight_on_and_turns_at_the_end():
    from paddle_sparse_amd import ops

    rowptr, col = nr.path_graph(10)
    nodes = ops.node2vec_walk(gpu(rowptr), gpu(col), None, gpu([0]), 12, 5, (0, ONE, ONE), 64)
    assert nodes.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 7, 6]]


# ---- equality with the existing walks ------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("edges", [False, True])
def test_p_q_one_is_todays_walk_and_so_is_the_new_kernel_at_one(weighted, edges):
    from paddle_sparse_amd import ops

    adj, cdf, rowptr, col = case_adj(False)
    start = gpu(nr.case_start(2 * nr.N_NODES))
    today = adj.random_walk(start, 17, seed=77, weighted=cdf if weighted else False, return_edge_ids=edges)
    public = adj.random_walk(start, 17, seed=77, weighted=cdf if weighted else False, return_edge_ids=edges, p=1, q=1.0)
    kernel = ops.node2vec_walk(rowptr, col, cdf.cum if weighted else None, start, 17, 77, (ONE,) * 3, 32, edges)
    for other in (public, kernel):
        if edges:
            assert torch.equal(today[0], other[0]) and torch.equal(today[1], other[1])
        else:
            assert torch.equal(today, other)


@pytest.mark.parametrize("weighted", [False, True])
def test_step_zero_is_sample_adjs_pick(weighted):
    from paddle_sparse_amd import ops

    adj, cdf, rowptr, col = case_adj(True)
    rowptr_np, _, _, cum_np = nr.case_graph(True)
    start = np.arange(nr.N_NODES)
    deg = np.diff(rowptr_np)
    picks = deg > 0
    if weighted:
        picks &= cum_np[np.maximum(rowptr_np[1:] - 1, 0)] > 0
    start = start[picks]
    _, e_walk = adj.random_walk(gpu(start), 1, seed=321, weighted=cdf if weighted else False, return_edge_ids=True,
                                p=0.25, q=4)
    out_rowptr, _, _, e_id = ops.sample_adj(rowptr, col, gpu(start), 1, True, seed=321,
                                            cum=cdf.cum if weighted else None)
    assert out_rowptr.tolist() == list(range(len(start) + 1))
    assert torch.equal(e_id, e_walk[:, 0])


# ---- reproducibility and inputs ---------------------------------------------------------------------------
def test_seeds_start_forms_and_errors():
    adj, cdf, _, _ = case_adj(True)
    rowptr_np, col_np, w, cum_np = nr.case_graph(True)
    start = nr.case_start(257)
    big = 2**63 + 11
    kw = dict(weighted=cdf, return_edge_ids=True, p=4, q=0.25)
    a = adj.random_walk(gpu(start), 16, seed=big, **kw)
    b = adj.random_walk(gpu(start), 16, seed=big, **kw)
    c = adj.random_walk(gpu(start), 16, seed=big + 1, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    want = nr.ref_node2vec_walk(rowptr_np, col_np, cum_np, start, 16, big, *nr.bias(4, 0.25))
    assert same(a, want)
    assert same(adj.random_walk(gpu(start, torch.int32), 16, seed=big, **kw), want)
    strided = gpu(np.stack([start, start + 1], 1))[:, 0]
    assert not strided.is_contiguous()
    assert same(adj.random_walk(strided, 16, seed=big, **kw), want)
    nodes, e_id = adj.random_walk(gpu(start[:0]), 5, seed=1, **kw)
    assert tuple(nodes.shape) == (0, 6) and tuple(e_id.shape) == (0, 5)
    for bad in ([0, nr.N_NODES], [-1, 0]):
        with pytest.raises(IndexError):
            adj.random_walk(gpu(bad), 3, seed=1, p=2)
        with pytest.raises(IndexError):
            adj.random_walk(gpu(bad), 3, seed=1, **kw)
    wide = adj_of(rowptr_np, col_np, gpu(w, torch.float32), N=nr.N_NODES + 3)
    with pytest.raises(ValueError, match="square"):
        wide.random_walk(gpu(start), 3, seed=1, p=2)


@pytest.mark.parametrize("symmetric", [True, False])
def test_edge_ids_lead_to_the_next_node_or_the_walk_stays(symmetric):
    adj, cdf, _, _ = case_adj(symmetric)
    _, col_np, w, _ = nr.case_graph(symmetric)
    start = gpu(np.arange(nr.N_NODES))
    for weighted in (False, cdf):
        nodes, e_id = adj.random_walk(start, 6, seed=9, weighted=weighted, return_edge_ids=True, p=0.5, q=2)
        nodes, e_id = nodes.cpu().numpy(), e_id.cpu().numpy()
        moved = e_id >= 0
        assert moved.any() and (~moved).any() and (e_id[~moved] == -1).all()
        assert np.array_equal(col_np[e_id[moved]], nodes[:, 1:][moved])
        assert np.array_equal(nodes[:, :-1][~moved], nodes[:, 1:][~moved])
        if weighted is not False:
            assert (w[e_id[moved]] > 0).all()


@pytest.mark.parametrize("p,q,weighted,seed", nr.KITE_CASES)
def test_kite_third_nodes_follow_the_bias(p, q, weighted, seed):
    rowptr, col, w = nr.kite_graph()
    adj = adj_of(rowptr, col, gpu(w, torch.float64))
    start = torch.zeros(nr.KITE_WALKS, dtype=torch.int64, device="cuda")
    nodes = adj.random_walk(start, 2, seed=seed, weighted=weighted, p=p, q=q).cpu().numpy()
    sigma, n = nr.kite_sigmas(nodes, p, q, weighted)
    print(f"kite p={p} q={q} weighted={weighted}: {n} walks through node 2, largest deviation {sigma:.2f} sigma")
    assert n > nr.KITE_WALKS // 3 and sigma < 5


# ---- graph capture -------------------------------------------------------------------------------------------
def test_the_walk_replays_from_a_hip_graph():
    from paddle_sparse_amd import _lib

    lib = _lib.load()
    _, cdf, rowptr, col = case_adj(True)
    rowptr_np, col_np, _, cum_np = nr.case_graph(True)
    S, L = 257, 17
    thr, max_tries = nr.bias(0.25, 4)
    start = gpu(nr.case_start(S))
    out = torch.empty((S, L + 1), dtype=torch.int64, device="cuda")
    e_id = torch.empty((S, L), dtype=torch.int64, device="cuda")
    flags = torch.zeros(1, dtype=torch.int64, device="cuda")

    def run():
        _lib.check(lib.psa_node2vec_walk(rowptr.data_ptr(), col.data_ptr(), cdf.cum.data_ptr(), nr.N_NODES,
                                         start.data_ptr(), S, L, 4242, *thr, max_tries, out.data_ptr(), e_id.data_ptr(),
                                         flags.data_ptr(), torch.cuda.current_stream().cuda_stream))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = (out.clone(), e_id.clone())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.fill_(-3)
    e_id.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    assert int(flags.item()) == 0
    assert torch.equal(out, eager[0]) and torch.equal(e_id, eager[1])
    assert same(eager, nr.ref_node2vec_walk(rowptr_np, col_np, cum_np, nr.case_start(S), L, 4242, thr, max_tries))
    start.copy_(gpu(nr.case_start(S)[::-1].copy()))  # new starts in the captured buffer
    g.replay()
    torch.cuda.synchronize()
    assert same((out, e_id), nr.ref_node2vec_walk(rowptr_np, col_np, cum_np, nr.case_start(S)[::-1], L, 4242, thr,
                                                   max_tries))
