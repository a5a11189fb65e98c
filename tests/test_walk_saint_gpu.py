"""GPU suite for random_walk and saint_subgraph.  Both ops are index work, so every
comparison is bit-exact against the restatement of tests/test_walk_saint.py (a
vectorised form of it for the walks, checked against the scalar one here), except the
end-to-end training step, whose SpMM follows test_spmm_gpu.py's tolerance."""
import numpy as np
import pytest
import torch

from test_walk_saint import (KAT_COL, KAT_N, KAT_ROW, KAT_SAINT, KAT_WALK, M64, ref_random_walk,
                             ref_saint_candidates, ref_saint_subgraph)
from util import random_csr, skewed_csr

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64]
RTOL = 1e-5


def mix64_np(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ref_random_walk_np(rowptr, col, start, L, seed, walk_ids=None):
    """ref_random_walk over all walks at once (degrees < 2^32); walk_ids: the walk
    numbers n of the given starts (default 0..S-1)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    cur = np.asarray(start, np.int64).copy()
    n = np.arange(cur.size, dtype=np.uint64) if walk_ids is None else np.asarray(walk_ids).astype(np.uint64)
    with np.errstate(over="ignore"):
        stream = mix64_np(np.uint64(seed & M64) ^ mix64_np(n))
        out = np.empty((cur.size, L + 1), np.int64)
        out[:, 0] = cur
        for l in range(L):
            s = rowptr[cur]
            deg = (rowptr[cur + 1] - s).astype(np.uint64)
            r = mix64_np(stream + np.uint64(l))
            pick = ((r >> np.uint64(32)) * deg + (((r & np.uint64(0xFFFFFFFF)) * deg) >> np.uint64(32))) >> np.uint64(32)
            move = deg > 0
            cur = np.where(move, col[np.where(move, s + pick.astype(np.int64), 0)], cur)
            out[:, l + 1] = cur
    return out


def gpu(x, dtype=torch.int64):
    return torch.as_tensor(np.asarray(x), dtype=dtype).cuda()


def adj_of(rowptr, col, value=None, N=None):
    from paddle_sparse_amd import SparseTensor

    N = len(rowptr) - 1 if N is None else N
    return SparseTensor(rowptr=gpu(rowptr), col=gpu(col), value=value, sparse_sizes=(len(rowptr) - 1, N),
                        is_sorted=True, trust_data=True)


def kat_adj(value=None):
    rowptr = np.searchsorted(KAT_ROW, np.arange(KAT_N + 1), side="left")
    return adj_of(rowptr, KAT_COL, value)


def sorted_csr(row, col, N):
    order = np.lexsort((col, row))
    row, col = row[order], col[order]
    return np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64), col


def graph(name):
    """(rowptr, col) of a square test graph, columns sorted inside rows."""
    rng = np.random.default_rng(7)
    if name == "uniform":
        row, _, col, _ = random_csr(3000, 3000, 20000, seed=1)
        return sorted_csr(row, col, 3000)
    if name == "hub":  # a 70 000-entry row, empty rows
        row, _, col, _ = skewed_csr(4000, 4000, seed=2, long_rows=(17,), long_deg=70_000)
        return sorted_csr(row, col, 4000)
    if name == "loops_multi_isolated":  # self loops, repeated entries, isolated nodes
        N = 500
        row = rng.integers(0, N // 2, 3000)
        col = rng.integers(0, N // 2, 3000)
        loops = rng.integers(0, N // 2, 200)
        row = np.concatenate([row, loops, row[:400]])
        col = np.concatenate([col, loops, col[:400]])
        return sorted_csr(row, col, N)
    raise KeyError(name)


GRAPHS = ["uniform", "hub", "loops_multi_isolated"]


# ---- random_walk -----------------------------------------------------------------------
def test_vectorised_restatement_matches_the_scalar_one():
    rowptr, col = graph("loops_multi_isolated")
    start = np.random.default_rng(3).integers(0, len(rowptr) - 1, 50)
    assert np.array_equal(ref_random_walk_np(rowptr, col, start, 7, 99), ref_random_walk(rowptr, col, start, 7, 99))


def test_random_walk_kat_functions_and_methods():
    import paddle_sparse_amd as psa

    k = KAT_WALK
    adj = kat_adj()
    start = gpu(k["start"])
    assert psa.random_walk(adj, start, k["L"], seed=k["seed"]).tolist() == k["out"]
    assert adj.random_walk(start, k["L"], seed=k["seed"]).tolist() == k["out"]


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("L", [1, 13, 40])
def test_random_walk_bit_exact(name, L):
    rowptr, col = graph(name)
    N = len(rowptr) - 1
    start = np.random.default_rng(L).integers(0, N, 3000)
    adj = adj_of(rowptr, col)
    out = adj.random_walk(gpu(start), L, seed=2024 + L)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3000, L + 1)
    ref = ref_random_walk_np(rowptr, col, start, L, 2024 + L)
    assert np.array_equal(out.cpu().numpy(), ref)
    # every step follows a stored entry, or stays at a node without entries
    a, b = ref[:, :-1].ravel(), ref[:, 1:].ravel()
    deg = np.diff(rowptr)
    dense = set(zip(np.repeat(np.arange(N), deg).tolist(), col.tolist()))
    assert all((x, y) in dense or (deg[x] == 0 and x == y) for x, y in zip(a.tolist(), b.tolist()))


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_every_store_scheme_gives_the_same_bits(variant):
    from paddle_sparse_amd import ops

    rowptr, col = graph("hub")
    start = gpu(np.random.default_rng(5).integers(0, len(rowptr) - 1, 7001))
    adj = adj_of(rowptr, col)
    want = adj.random_walk(start, 37, seed=5)
    prev = ops.random_walk_set_variant(variant)
    try:
        got = adj.random_walk(start, 37, seed=5)
    finally:
        ops.random_walk_set_variant(prev)
    assert torch.equal(got, want)


def test_step_zero_is_sample_adjs_pick():
    from paddle_sparse_amd import ops

    rowptr, col = graph("hub")
    deg = np.diff(rowptr)
    start = np.random.default_rng(9).integers(0, len(rowptr) - 1, 5000)
    start = start[deg[start] > 0]
    walk = adj_of(rowptr, col).random_walk(gpu(start), 3, seed=777)
    _, _, _, e_id = ops.sample_adj(gpu(rowptr), gpu(col), gpu(start), 1, replace=True, seed=777)
    assert torch.equal(walk[:, 1], gpu(col)[e_id])


def test_star_graph_frequencies():
    """Walks from the centre of a star: each leaf is drawn with probability 1/K."""
    K, S = 37, 370_000
    rowptr = np.concatenate([[0], np.full(K + 1, K)]).astype(np.int64)
    col = np.arange(1, K + 1, dtype=np.int64)
    out = adj_of(rowptr, col).random_walk(torch.zeros(S, dtype=torch.int64, device="cuda"), 2, seed=31337)
    assert torch.all(out[:, 2] == out[:, 1])  # leaves have no entries: the walk stays
    counts = torch.bincount(out[:, 1], minlength=K + 1).cpu().numpy()
    assert counts[0] == 0
    expect = S / K
    sigma = np.sqrt(expect * (1 - 1 / K))
    assert np.all(np.abs(counts[1:] - expect) < 5 * sigma), counts
    chi2 = float(((counts[1:] - expect) ** 2 / expect).sum())
    assert chi2 < 80.0, chi2  # 36 degrees of freedom: p < 1e-4 above 80


def test_random_walk_edge_cases():
    import paddle_sparse_amd as psa

    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col)
    start = gpu([5, 0, 2999, 17])
    assert torch.equal(adj.random_walk(start, 0, seed=1), start[:, None])
    empty = adj.random_walk(start[:0], 6, seed=1)
    assert tuple(empty.shape) == (0, 7) and empty.dtype == torch.int64
    ref = adj.random_walk(start, 9, seed=3)
    assert torch.equal(adj.random_walk(start.to(torch.int32), 9, seed=3), ref)
    wide = torch.stack([start, start + 1], dim=1)[:, 0]  # non-contiguous
    assert not wide.is_contiguous()
    assert torch.equal(adj.random_walk(wide, 9, seed=3), ref)
    torch.manual_seed(11)
    a = psa.random_walk(adj, start, 9)
    torch.manual_seed(11)
    b = psa.random_walk(adj, start, 9)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="square"):
        adj_of(rowptr, col, N=3001).random_walk(start, 3, seed=1)
    for bad in ([0, 3000], [-1, 0]):
        with pytest.raises(IndexError):
            adj.random_walk(gpu(bad), 3, seed=1)


# ---- saint_subgraph ------------------------------------------------------------------
@pytest.mark.parametrize("node_idx,rowptr,col,edge", KAT_SAINT)
def test_saint_kat_functions_and_methods(node_idx, rowptr, col, edge):
    import paddle_sparse_amd as psa

    value = torch.arange(10, dtype=torch.float32, device="cuda")
    adj = kat_adj(value)
    for sub, e in (psa.saint_subgraph(adj, gpu(node_idx)), adj.saint_subgraph(gpu(node_idx))):
        assert sub.sparse_sizes() == (3, 3)
        assert sub.storage.rowptr().tolist() == rowptr and sub.storage.col().tolist() == col
        assert e.tolist() == edge
        assert sub.storage.value().tolist() == [float(x) for x in edge]


def _node_sets(N, rng):
    sample = np.sort(rng.choice(N, N // 5, replace=False))
    return {
        "sorted": sample,
        "unsorted": rng.permutation(sample),
        "duplicated": rng.choice(sample, sample.size + 300),
        "sorted_with_repeats": np.sort(rng.choice(sample, sample.size)),
        "every_node": np.arange(N),
        "isolated_only": np.array([N - 1, N - 2]),
    }


@pytest.mark.parametrize("name", GRAPHS)
def test_saint_subgraph_bit_exact(name):
    rowptr, col = graph(name)
    N = len(rowptr) - 1
    value = torch.randn(col.size, device="cuda")
    adj = adj_of(rowptr, col, value)
    for how, idx in _node_sets(N, np.random.default_rng(4)).items():
        sub, e = adj.saint_subgraph(gpu(idx))
        p, c, er = ref_saint_subgraph(rowptr, col, idx, N)
        S = idx.size
        assert sub.sparse_sizes() == (S, S), how
        assert np.array_equal(sub.storage.rowptr().cpu().numpy(), p), how
        assert np.array_equal(sub.storage.col().cpu().numpy(), c), how
        assert np.array_equal(e.cpu().numpy(), er), how
        assert np.array_equal(sub.storage.row().cpu().numpy(), np.repeat(np.arange(S), np.diff(p))), how
        assert torch.equal(sub.storage.value(), value[e]), how


def test_saint_hub_row_candidates_in_order():
    """Unsorted candidates of a 70 000-entry row keep candidate order among equal keys."""
    rowptr, col = graph("hub")
    N = len(rowptr) - 1
    idx = np.concatenate([[17], np.arange(N - 1, 17, -3)])
    sub, e = adj_of(rowptr, col).saint_subgraph(gpu(idx))
    p, c, er = ref_saint_subgraph(rowptr, col, idx, N)
    assert sub.nnz() > 3000
    assert np.array_equal(sub.storage.col().cpu().numpy(), c) and np.array_equal(e.cpu().numpy(), er)
    row, cc, ee = ref_saint_candidates(rowptr, col, idx, N)
    assert row.size == er.size and set(ee.tolist()) == set(er.tolist())


def test_saint_empty_and_errors():
    rowptr, col = graph("uniform")
    adj = adj_of(rowptr, col, torch.ones(col.size, device="cuda"))
    sub, e = adj.saint_subgraph(gpu(np.zeros(0, np.int64)))
    assert sub.sparse_sizes() == (0, 0) and sub.nnz() == 0 and e.numel() == 0
    assert sub.storage.rowptr().tolist() == [0]
    sub, e = adj.saint_subgraph(gpu([4], dtype=torch.int32))
    assert sub.sparse_sizes() == (1, 1)
    with pytest.raises(ValueError, match="square"):
        adj_of(rowptr, col, N=3001).saint_subgraph(gpu([0]))
    for bad in ([0, 3000], [-1]):
        with pytest.raises(IndexError):
            adj.saint_subgraph(gpu(bad))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trailing", [(), (3,), (2, 5)])
def test_values_of_every_dtype(dtype, trailing):
    rowptr, col = graph("loops_multi_isolated")
    N = len(rowptr) - 1
    base = torch.randint(-1000, 1000, (col.size,) + trailing)
    value = base.to(dtype).cuda()
    adj = adj_of(rowptr, col, value)
    idx = np.random.default_rng(1).choice(N, 300)
    sub, e = adj.saint_subgraph(gpu(idx))
    v = sub.storage.value()
    assert v.dtype == dtype and tuple(v.shape) == (sub.nnz(),) + trailing
    assert torch.equal(v.cpu(), value.cpu()[e.cpu()])


def _dense(t):
    return t.to_dense().cpu()


def test_permutation_and_distinct_selection_equal_existing_ops():
    row, _, col, _ = random_csr(800, 800, 9000, seed=12)
    rowptr, col = sorted_csr(row, col, 800)
    value = torch.randint(-50, 50, (col.size,)).float().cuda()
    adj = adj_of(rowptr, col, value)
    rng = np.random.default_rng(2)
    perm = gpu(rng.permutation(800))
    sub, _ = adj.saint_subgraph(perm)
    assert torch.equal(_dense(sub), _dense(adj.permute(perm)))
    idx = gpu(rng.choice(800, 250, replace=False))
    sub, _ = adj.saint_subgraph(idx)
    assert torch.equal(_dense(sub), _dense(adj.index_select(0, idx).index_select(1, idx)))


@pytest.mark.parametrize("how", ["distinct", "duplicated"])
@pytest.mark.parametrize("trailing", [(), (4,)])
def test_value_gradient_is_exact_and_deterministic(how, trailing):
    rowptr, col = graph("hub")
    N = len(rowptr) - 1
    rng = np.random.default_rng(8)
    idx = rng.choice(N, 900, replace=False)
    if how == "duplicated":
        idx = np.concatenate([idx, idx[:300], [17, 17, 17]])
        rng.shuffle(idx)
    value = torch.randint(-8, 8, (col.size,) + trailing).float().cuda().requires_grad_()
    adj = adj_of(rowptr, col, value)

    def grad_once():
        value.grad = None
        sub, e = adj.saint_subgraph(gpu(idx))
        w = torch.arange(sub.nnz() * max(1, int(np.prod(trailing))), device="cuda").float().remainder(13)
        (sub.storage.value() * w.view((sub.nnz(),) + trailing)).sum().backward()
        return value.grad.clone(), e, w

    g1, e, w = grad_once()
    g2, _, _ = grad_once()
    assert torch.equal(g1, g2)
    want = torch.zeros((col.size,) + trailing).index_add_(0, e.cpu(), w.cpu().view((e.numel(),) + trailing))
    assert torch.equal(g1.cpu(), want)


def test_graphsaint_step_end_to_end():
    """walk -> unique -> subgraph -> matmul -> backward with trainable values, against the
    same step built from the CPU restatement and the existing SpMM."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from bench import rmat_graph
    from paddle_sparse_amd import SparseTensor

    N, rowptr, _, col, val = rmat_graph(14, 200_000, torch.device("cuda"), seed=21)
    adj = SparseTensor(rowptr=rowptr, col=col, value=val.clone().requires_grad_(), sparse_sizes=(N, N),
                       is_sorted=True, trust_data=True)
    start = torch.randint(0, N, (500,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    node_idx = adj.random_walk(start, 2, seed=99).view(-1).unique()
    x = torch.randn(N, 32, device="cuda")
    sub, e = adj.saint_subgraph(node_idx)
    out = sub @ x[node_idx]
    out.square().sum().backward()
    g = adj.storage.value().grad

    rp, cl = rowptr.cpu().numpy(), col.cpu().numpy()
    walks = ref_random_walk_np(rp, cl, start.cpu().numpy(), 2, 99)
    nodes = np.unique(walks)
    assert np.array_equal(nodes, node_idx.cpu().numpy())
    p, c, er = ref_saint_subgraph(rp, cl, nodes, N)
    leaf = val.clone().requires_grad_()
    ref_sub = SparseTensor(rowptr=gpu(p), col=gpu(c), value=leaf[gpu(er)], sparse_sizes=(nodes.size, nodes.size),
                           is_sorted=True, trust_data=True)
    ref_out = ref_sub @ x[gpu(nodes)]
    ref_out.square().sum().backward()
    absum = SparseTensor(rowptr=gpu(p), col=gpu(c), value=ref_sub.storage.value().detach().abs(),
                         sparse_sizes=ref_sub.sparse_sizes(), is_sorted=True, trust_data=True) @ x[gpu(nodes)].abs()
    assert torch.all((out - ref_out).abs() <= RTOL * absum + 1e-30)
    assert np.array_equal(e.cpu().numpy(), er)
    assert torch.allclose(g, leaf.grad, rtol=1e-4, atol=1e-4 * float(leaf.grad.abs().max()))


def test_full_size_deepwalk():
    """Every node of a config-3-shaped graph (2 M nodes, 20 M entries) as a start, L = 80:
    a seeded sample of walks is bit-exact, and every step of it follows a stored entry."""
    from paddle_sparse_amd import SparseTensor, ops

    M = 2_000_000
    g = torch.Generator(device="cuda").manual_seed(3)
    keys = torch.sort(torch.randint(0, M, (20_000_000,), generator=g, device="cuda") * M
                      + torch.randint(0, M, (20_000_000,), generator=g, device="cuda"))[0]
    row, col = keys // M, keys % M
    rowptr = ops.ind2ptr(row, M)
    del row
    adj = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(M, M), is_sorted=True, trust_data=True)
    out = adj.random_walk(torch.arange(M, device="cuda"), 80, seed=123)
    assert tuple(out.shape) == (M, 81)
    sample = torch.from_numpy(np.sort(np.random.default_rng(0).choice(M, 2000, replace=False))).cuda()
    walks = out[sample]
    del out
    a, b = walks[:, :-1].reshape(-1), walks[:, 1:].reshape(-1)
    hit = torch.searchsorted(keys, a * M + b)
    found = keys[hit.clamp(max=keys.numel() - 1)] == a * M + b
    deg = (rowptr[1:] - rowptr[:-1])[a]
    assert bool(torch.all(found | ((deg == 0) & (a == b))))
    ref = ref_random_walk_np(rowptr.cpu().numpy(), col.cpu().numpy(), sample.cpu().numpy(), 80, 123,
                             walk_ids=sample.cpu().numpy())
    assert np.array_equal(walks.cpu().numpy(), ref)
