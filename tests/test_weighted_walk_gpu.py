"""GPU suite for the edge-weighted samplers: psa_row_cdf, the weighted random walk with edge
ids, the uniform walk with edge ids and weighted sample_adj.  Everything here is either
float64 sums in a pinned order or index work, so every comparison is bit-exact against the
numpy restatement of tests/weighted_ref.py; the statistical checks carry the bounds of the
CPU suite (tests/test_weighted_ref.py), which the restatement meets with 2.19 and 1.89 sigma."""
import numpy as np
import pytest
import torch

import weighted_ref as wr
from paddle_sparse_amd import EdgeCDF  # noqa: F401  (no test here means anything without it)
from util import random_csr, skewed_csr

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]


def gpu(x, dtype=torch.int64):
    return torch.as_tensor(np.array(x), dtype=dtype).cuda()  # a copy: the cached graphs are read-only


def adj_of(rowptr, col, value=None, N=None):
    from paddle_sparse_amd import SparseTensor

    N = len(rowptr) - 1 if N is None else N
    return SparseTensor(rowptr=gpu(rowptr), col=gpu(col), value=value, sparse_sizes=(len(rowptr) - 1, N),
                        is_sorted=True, trust_data=True)


def sorted_csr(row, col, N):
    order = np.lexsort((col, row))
    row, col = row[order], col[order]
    return np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64), col


def graph(name):
    """(rowptr, col) of a square test graph, columns sorted inside rows: the graphs of
    test_walk_saint_gpu.py, built the same way."""
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


def weights(kind, nnz, seed=0):
    """float32 weights, 30 % exact zeros: "unit" uniform in [0, 1), "spread" magnitudes over
    2^-30 .. 2^30."""
    rng = np.random.default_rng(seed)
    w = rng.random(nnz, dtype=np.float32)
    if kind == "spread":
        w = np.ldexp(0.5 + 0.5 * w, rng.integers(-29, 31, nnz)).astype(np.float32)
    w[rng.random(nnz) < 0.3] = 0
    return w


def lengths_csr(lengths):
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(rowptr[-1])
    return rowptr, np.random.default_rng(1).integers(0, len(lengths), nnz)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


_GRAPH_CACHE = {}


def weighted_graph(name):
    """(rowptr, col, w float32, cum float64) of a test graph, made once; every seventh row of
    the small graph weighs nothing at all."""
    if name not in _GRAPH_CACHE:
        rowptr, col = graph(name)
        w = weights("unit", len(col), seed=11)
        if name == "loops_multi_isolated":
            for r in range(0, len(rowptr) - 1, 7):
                w[rowptr[r]:rowptr[r + 1]] = 0
        for a in (rowptr, col, w):
            a.setflags(write=False)
        cum = wr.row_cdf(rowptr, w)
        cum.setflags(write=False)
        _GRAPH_CACHE[name] = (rowptr, col, w, cum)
    return _GRAPH_CACHE[name]


def weighted_adj(name, requires_grad=False):
    rowptr, col, w, cum = weighted_graph(name)
    value = gpu(w, torch.float32)
    if requires_grad:
        value.requires_grad_(True)
    return adj_of(rowptr, col, value), rowptr, col, w, cum


# ---- psa_row_cdf ------------------------------------------------------------------------------
def check_cdf(rowptr, w):
    from paddle_sparse_amd import ops

    cum, flags = ops.row_cdf(gpu(rowptr), gpu(w, torch.float64))
    assert int(flags.item()) == 0
    assert np.array_equal(bits(cum.cpu().numpy()), bits(wr.row_cdf(rowptr, w)))


@pytest.mark.parametrize("kind", ["unit", "spread"])
def test_row_cdf_is_cumsum_at_every_length(kind):
    rowptr, _ = lengths_csr(LENGTHS)
    check_cdf(rowptr, weights(kind, int(rowptr[-1]), seed=3))


@pytest.mark.parametrize("kind", ["unit", "spread"])
def test_row_cdf_with_shuffled_lengths_and_runs_of_empty_rows(kind):
    rng = np.random.default_rng(5)
    lengths = [0] * 70
    for n in rng.permutation(LENGTHS * 2).tolist():
        lengths += [n] + [0] * int(rng.integers(0, 130))
    lengths += [0] * 300
    rowptr, _ = lengths_csr(lengths)
    check_cdf(rowptr, weights(kind, int(rowptr[-1]), seed=4))


def test_row_cdf_around_the_length_where_a_wave_takes_the_row():
    rowptr, _ = lengths_csr([15, 16, 17, 18, 0, 16, 17] * 40)
    check_cdf(rowptr, weights("spread", int(rowptr[-1]), seed=9))


@pytest.mark.parametrize("N", [63, 64, 65, 128, 129, 256, 257, 1000])
def test_row_cdf_when_every_row_is_a_waves_row(N):
    """The long rows are dealt to the waves by an odd stride: every row must be taken once,
    whatever N is against the 64 rows of a wave and the 256 of a workgroup."""
    rowptr, _ = lengths_csr([17 + 24 * (r % 3) for r in range(N)])
    check_cdf(rowptr, weights("unit", int(rowptr[-1]), seed=N))


@pytest.mark.parametrize("kind", ["unit", "spread"])
def test_row_cdf_on_the_hub_graph(kind):
    rowptr, col = graph("hub")
    assert np.diff(rowptr).max() == 70_000
    check_cdf(rowptr, weights(kind, len(col), seed=6))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int32])
def test_edge_cdf_takes_every_value_dtype(dtype):
    import paddle_sparse_amd as psa

    rowptr, col = lengths_csr(LENGTHS)
    w = weights("unit", len(col), seed=8)
    value = gpu(np.floor(w * 10), dtype) if dtype == torch.int32 else gpu(w, torch.float32).to(dtype)
    cdf = psa.EdgeCDF(adj_of(rowptr, col, value, N=len(LENGTHS)))
    assert cdf.cum.dtype == torch.float64
    want = wr.row_cdf(rowptr, value.double().cpu().numpy())
    assert np.array_equal(bits(cdf.cum.cpu().numpy()), bits(want))


@pytest.mark.parametrize("deg", [5, 200])  # a lane's row, a wave's row
@pytest.mark.parametrize("bad,flag,message", [([-1.0], 1, "negative"), ([float("nan")], 2, "NaN or infinite"),
                                              ([float("inf")], 2, "NaN or infinite"),
                                              ([1e308, 1e308], 4, "overflow")])
def test_each_flag_is_raised_by_its_cause(deg, bad, flag, message):
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    rowptr = np.array([0, 3, 3 + deg, 3 + deg + 2], np.int64)
    w = np.ones(int(rowptr[-1]))
    w[3 + deg - len(bad):3 + deg] = bad
    _, flags = ops.row_cdf(gpu(rowptr), gpu(w, torch.float64))
    assert int(flags.item()) == flag
    col = np.zeros(len(w), np.int64)
    with pytest.raises(ValueError, match=message):
        psa.EdgeCDF(adj_of(rowptr, col, gpu(w, torch.float64)))


@pytest.mark.parametrize("deg", [5, 200])
def test_negative_zero_is_a_zero_weight(deg):
    import paddle_sparse_amd as psa

    rowptr = np.array([0, deg, deg + 1], np.int64)
    w = np.ones(deg + 1)
    w[[0, deg // 2, deg]] = -0.0
    cdf = psa.EdgeCDF(adj_of(rowptr, np.zeros(deg + 1, np.int64), gpu(w, torch.float64)))
    assert np.array_equal(bits(cdf.cum.cpu().numpy()), bits(wr.row_cdf(rowptr, w)))


def test_an_edge_cdf_serves_its_own_matrix_only():
    import paddle_sparse_amd as psa

    adj, rowptr, col, w, _ = weighted_adj("uniform")
    other = adj_of(rowptr, col, gpu(w, torch.float32))
    cdf = psa.EdgeCDF(adj)
    start = gpu(np.arange(10))
    adj.random_walk(start, 2, seed=1, weighted=cdf)
    with pytest.raises(ValueError, match="another matrix"):
        other.random_walk(start, 2, seed=1, weighted=cdf)
    with pytest.raises(ValueError, match="another matrix"):
        other.sample_adj(start, 2, replace=True, seed=1, weighted=cdf)


# ---- the weighted walk ---------------------------------------------------------------------------
def check_steps(nodes, e_id, rowptr, col, w):
    """Every taken entry lies in the current row, leads to the next node and weighs > 0; the
    walk stays, with e_id -1, exactly where the row is empty or weighs nothing (a self loop
    repeats the node too, with e_id >= 0)."""
    a, b, e = nodes[:, :-1].ravel(), nodes[:, 1:].ravel(), e_id.ravel()
    moved = e >= 0
    assert np.all(e[moved] >= rowptr[a[moved]]) and np.all(e[moved] < rowptr[a[moved] + 1])
    assert np.array_equal(col[e[moved]], b[moved])
    if w is not None:
        assert np.all(w[e[moved]] > 0)
        total = np.add.reduceat(np.concatenate([w.astype(np.float64), [0.0]]), np.minimum(rowptr[:-1], len(w)))
        total[np.diff(rowptr) == 0] = 0
        dead = total == 0
    else:
        dead = np.diff(rowptr) == 0
    assert np.array_equal(~moved, dead[a]) and np.array_equal(a[~moved], b[~moved])
    assert np.all(e[~moved] == -1)


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("L", [1, 13, 40])
def test_weighted_walk_bit_exact(name, L):
    import paddle_sparse_amd as psa

    adj, rowptr, col, w, cum = weighted_adj(name)
    N = len(rowptr) - 1
    start = np.random.default_rng(L).integers(0, N, 3000)
    nodes, e_id = adj.random_walk(gpu(start), L, seed=2024 + L, weighted=True, return_edge_ids=True)
    assert nodes.dtype == torch.int64 and tuple(nodes.shape) == (3000, L + 1)
    assert e_id.dtype == torch.int64 and tuple(e_id.shape) == (3000, L)
    ref_nodes, ref_e = wr.ref_weighted_walk(rowptr, col, cum, start, L, 2024 + L)
    assert np.array_equal(nodes.cpu().numpy(), ref_nodes) and np.array_equal(e_id.cpu().numpy(), ref_e)
    check_steps(ref_nodes, ref_e, rowptr, col, w)
    if name == "loops_multi_isolated":
        loops = (ref_e >= 0) & (ref_nodes[:, :-1] == ref_nodes[:, 1:])
        assert loops.any() and (ref_e < 0).any()  # both ways of repeating a node happen
    # without the edge ids: the same nodes, from the function as from the method
    assert torch.equal(psa.random_walk(adj, gpu(start), L, seed=2024 + L, weighted=True), nodes)


def star_counts_gpu(weights_):
    rowptr, col, w = wr.star(weights_)
    adj = adj_of(rowptr, col, gpu(w, torch.float64))
    S = 370_000
    nodes = adj.random_walk(torch.zeros(S, dtype=torch.int64, device="cuda"), 1, seed=31337, weighted=True)
    return np.bincount(nodes[:, 1].cpu().numpy(), minlength=len(weights_) + 1)[1:], S


def test_draws_follow_the_weights_on_a_star():
    w = np.arange(1, 38, dtype=np.float64)
    counts, S = star_counts_gpu(w)
    sigma, chi2 = wr.star_bounds(counts, w, S)
    print(f"star of 37: largest deviation {sigma:.2f} sigma, chi^2 {chi2:.1f}")
    assert sigma < 5 and chi2 < 80


def test_zero_weight_leaves_are_never_visited():
    w = [0, 1, 0, 2, 4, 0, 8, .5, .25, 0]
    counts, S = star_counts_gpu(w)
    sigma, _ = wr.star_bounds(counts, w, S)
    print(f"star with zeros: counts {counts.tolist()}, largest deviation {sigma:.2f} sigma")
    assert counts[np.array(w) == 0].tolist() == [0, 0, 0, 0] and counts.sum() == S
    assert sigma < 5


def test_walk_edge_shapes_and_start_forms():
    import paddle_sparse_amd as psa

    adj, rowptr, col, w, cum = weighted_adj("loops_multi_isolated")
    cdf = psa.EdgeCDF(adj)
    start = np.random.default_rng(2).integers(0, len(rowptr) - 1, 77)
    nodes, e_id = adj.random_walk(gpu(start), 0, seed=1, weighted=cdf, return_edge_ids=True)
    assert nodes.cpu().numpy().tolist() == start.reshape(-1, 1).tolist() and tuple(e_id.shape) == (77, 0)
    nodes, e_id = adj.random_walk(gpu(start[:0]), 5, seed=1, weighted=cdf, return_edge_ids=True)
    assert tuple(nodes.shape) == (0, 6) and tuple(e_id.shape) == (0, 5)
    want = wr.ref_weighted_walk(rowptr, col, cum, start, 9, 3)
    got = adj.random_walk(gpu(start, torch.int32), 9, seed=3, weighted=cdf, return_edge_ids=True)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    strided = gpu(np.stack([start, start + 1], 1))[:, 0]
    assert not strided.is_contiguous()
    got = adj.random_walk(strided, 9, seed=3, weighted=cdf, return_edge_ids=True)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    for bad in ([0, len(rowptr) - 1], [-1, 0]):
        with pytest.raises(IndexError):
            adj.random_walk(gpu(bad), 3, seed=1, weighted=cdf)
        with pytest.raises(IndexError):
            adj.random_walk(gpu(bad), 3, seed=1, return_edge_ids=True)
    wide = adj_of(rowptr, col, gpu(w, torch.float32), N=len(rowptr) + 3)
    with pytest.raises(ValueError, match="square"):
        wide.random_walk(gpu(start), 3, seed=1, weighted=True)


def test_same_seed_same_bits_and_true_equals_an_edge_cdf():
    import paddle_sparse_amd as psa

    adj, rowptr, _, _, _ = weighted_adj("hub")
    start = gpu(np.random.default_rng(5).integers(0, len(rowptr) - 1, 7001))
    cdf = psa.EdgeCDF(adj)
    a = adj.random_walk(start, 37, seed=5, weighted=cdf, return_edge_ids=True)
    b = adj.random_walk(start, 37, seed=5, weighted=cdf, return_edge_ids=True)
    c = adj.random_walk(start, 37, seed=5, weighted=True, return_edge_ids=True)
    d = adj.random_walk(start, 37, seed=6, weighted=cdf, return_edge_ids=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[0], d[0])


# ---- the uniform walk with edge ids -----------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_uniform_walk_with_edge_ids(name):
    adj, rowptr, col, _, _ = weighted_adj(name)
    start = np.random.default_rng(4).integers(0, len(rowptr) - 1, 3000)
    for L in (1, 13, 40):
        want = adj.random_walk(gpu(start), L, seed=77 + L)
        nodes, e_id = adj.random_walk(gpu(start), L, seed=77 + L, return_edge_ids=True)
        assert torch.equal(nodes, want)
        nodes, e_id = nodes.cpu().numpy(), e_id.cpu().numpy()
        ref_nodes, ref_e = wr.ref_weighted_walk(rowptr, col, None, start, L, 77 + L)
        assert np.array_equal(nodes, ref_nodes) and np.array_equal(e_id, ref_e)
        check_steps(nodes, e_id, rowptr, col, None)


# ---- sample_adj --------------------------------------------------------------------------------------
def test_step_zero_is_weighted_sample_adjs_pick():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    adj, rowptr, col, w, cum = weighted_adj("hub")
    start = np.random.default_rng(9).integers(0, len(rowptr) - 1, 5000)
    start = start[cum[np.maximum(rowptr[start + 1] - 1, 0)] * (np.diff(rowptr)[start] > 0) > 0]  # rows that pick
    cdf = psa.EdgeCDF(adj)
    _, e_walk = adj.random_walk(gpu(start), 1, seed=321, weighted=cdf, return_edge_ids=True)
    out_rowptr, _, _, e_id = ops.sample_adj(gpu(rowptr), gpu(col), gpu(start), 1, True, seed=321, cum=cdf.cum)
    assert out_rowptr.tolist() == list(range(len(start) + 1))  # one pick per row: storage order is row order
    assert torch.equal(e_id, e_walk[:, 0])


def test_weighted_sample_adj_bit_exact_through_the_chain():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    adj, rowptr, col, w, cum = weighted_adj("loops_multi_isolated")
    idx = np.random.default_rng(12).integers(0, len(rowptr) - 1, 400)  # duplicates, empty and zero-total rows
    n_id, out_rowptr, out_col, e_id = wr.ref_weighted_select(rowptr, col, cum, idx, 5, 99)
    cdf = psa.EdgeCDF(adj)
    got = ops.sample_adj(gpu(rowptr), gpu(col), gpu(idx), 5, True, seed=99, cum=cdf.cum)
    assert np.array_equal(got[0].cpu().numpy(), out_rowptr) and np.array_equal(got[1].cpu().numpy(), out_col)
    assert np.array_equal(got[2].cpu().numpy(), n_id) and np.array_equal(got[3].cpu().numpy(), e_id)
    assert np.all(w[e_id] > 0)
    # rows that weigh nothing make no picks; every other row makes 5
    total = np.array([cum[rowptr[n + 1] - 1] if rowptr[n + 1] > rowptr[n] else 0.0 for n in idx])
    assert (total == 0).any() and np.array_equal(np.diff(out_rowptr), np.where(total > 0, 5, 0))
    # the SparseTensor form carries the picked values
    out, n_id2 = adj.sample_adj(gpu(idx), 5, replace=True, seed=99, weighted=cdf)
    assert np.array_equal(n_id2.cpu().numpy(), n_id) and np.array_equal(out.storage.col().cpu().numpy(), out_col)
    assert np.array_equal(out.storage.value().cpu().numpy(), w[e_id])
    out3, _ = psa.sample_adj(adj, gpu(idx), 5, replace=True, seed=99, weighted=True)
    assert torch.equal(out3.storage.col(), out.storage.col()) and torch.equal(out3.storage.value(), out.storage.value())


def test_taking_every_entry_ignores_the_weights():
    adj, rowptr, _, _, _ = weighted_adj("loops_multi_isolated")
    idx = gpu(np.random.default_rng(13).integers(0, len(rowptr) - 1, 300))
    want, want_n = adj.sample_adj(idx, -1, seed=1)
    for replace in (False, True):
        got, n_id = adj.sample_adj(idx, -1, replace=replace, seed=1, weighted=True)
        assert torch.equal(n_id, want_n) and torch.equal(got.storage.rowptr(), want.storage.rowptr())
        assert torch.equal(got.storage.col(), want.storage.col()) and torch.equal(got.storage.value(), want.storage.value())


def test_weighted_picks_without_replacement_are_refused():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    adj, rowptr, col, _, _ = weighted_adj("uniform")
    cdf = psa.EdgeCDF(adj)
    idx = gpu(np.arange(50))
    for k in (0, 1, 3):
        with pytest.raises(NotImplementedError):
            adj.sample_adj(idx, k, replace=False, seed=1, weighted=cdf)
        with pytest.raises(NotImplementedError):
            ops.sample_adj(gpu(rowptr), gpu(col), idx, k, False, seed=1, cum=cdf.cum)


def test_value_gradient_through_a_weighted_sample():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    adj, rowptr, col, w, _ = weighted_adj("uniform", requires_grad=True)
    value = adj.storage.value()
    cdf = psa.EdgeCDF(adj)
    idx = gpu(np.random.default_rng(14).integers(0, len(rowptr) - 1, 500))
    out, _ = adj.sample_adj(idx, 4, replace=True, seed=8, weighted=cdf)
    e_id = ops.sample_adj(gpu(rowptr), gpu(col), idx, 4, True, seed=8, cum=cdf.cum)[3]
    picked = out.storage.value()
    assert torch.equal(picked.detach(), value.detach()[e_id])
    g = torch.arange(1, picked.numel() + 1, dtype=torch.float32, device="cuda")  # integers: any order adds exactly
    picked.backward(g)
    want = torch.zeros_like(value).index_add_(0, e_id, g)
    assert torch.equal(value.grad, want) and int((want != 0).sum()) < e_id.numel()  # some entry was picked twice


# ---- graph capture -----------------------------------------------------------------------------------
def test_row_cdf_and_the_weighted_walk_replay_from_a_hip_graph():
    from paddle_sparse_amd import _lib, ops

    lib = _lib.load()
    _, rowptr_np, col_np, w_np, _ = weighted_adj("hub")
    rowptr, col = gpu(rowptr_np), gpu(col_np)
    N, S, L = len(rowptr_np) - 1, 3000, 13
    weight = gpu(w_np, torch.float64)
    start = gpu(np.random.default_rng(15).integers(0, N, S))
    out = torch.empty((S, L + 1), dtype=torch.int64, device="cuda")
    e_id = torch.empty((S, L), dtype=torch.int64, device="cuda")
    walk_flags = torch.zeros(1, dtype=torch.int64, device="cuda")

    def run():
        cum, flags = ops.row_cdf(rowptr, weight)
        _lib.check(lib.psa_random_walk_weighted(rowptr.data_ptr(), col.data_ptr(), cum.data_ptr(), N, start.data_ptr(),
                                                S, L, 4242, out.data_ptr(), e_id.data_ptr(), walk_flags.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
        return cum, flags

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cum, flags = run()
    for trial in range(3):  # new weights and starts in the captured buffers, replay
        w_new = weights("unit", len(col_np), seed=100 + trial)
        weight.copy_(gpu(w_new, torch.float64))
        start_new = np.random.default_rng(200 + trial).integers(0, N, S)
        start.copy_(gpu(start_new))
        g.replay()
        torch.cuda.synchronize()
        want_cum = wr.row_cdf(rowptr_np, w_new)
        assert int(flags.item()) == 0 and int(walk_flags.item()) == 0
        assert np.array_equal(bits(cum.cpu().numpy()), bits(want_cum))
        nodes, edges = wr.ref_weighted_walk(rowptr_np, col_np, want_cum, start_new, L, 4242)
        assert np.array_equal(out.cpu().numpy(), nodes) and np.array_equal(e_id.cpu().numpy(), edges)
