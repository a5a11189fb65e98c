"""GPU suite for edge lookup and negative sampling (csrc/negative.hip).  Both kernels are index work
on integers, so every comparison is bit-exact against the serial restatement of
tests/negative_ref.py (pinned by test_zz_negative_ref.py, which also holds the kernels' steps, run
on the host, to it), on the case tables of that file: row lengths 0, 1, 2, 3, 63, 64, 65 and 1000,
duplicated entries, counts either side of a lane, a wave and a workgroup, k of 1 and 3, both modes,
no_self_loops on and off, a 40 x 70 matrix, and column ids above 2^32 (N = 2^40), which catch a
32-bit index anywhere.  rowptr values above 2^31 are NOT exercised: a matrix of that many entries
cannot be allocated and filled in a few seconds.

The file name sorts behind every other GPU file on purpose: the new tests are collected last."""
import numpy as np
import pytest
import torch

import negative_ref as nr
from test_weighted_walk_gpu import adj_of, gpu

pytestmark = pytest.mark.gpu

_ADJ = {}


def case_adj(name):
    if name not in _ADJ:
        rowptr, col, _, N = nr.case_graph(name)
        _ADJ[name] = adj_of(rowptr, col, N=N)
    return _ADJ[name]


def same(got, want):
    assert got.dtype == torch.int64 and got.is_cuda
    return np.array_equal(got.cpu().numpy().reshape(-1), want)


# ---- the case tables ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(nr.LOOKUP_CASES)))
def test_lookup_case_table_bit_exact(k):
    import paddle_sparse_amd as psa

    name, Q = nr.LOOKUP_CASES[k]
    adj = case_adj(name)
    r, c = nr.case_queries(name, Q)
    narrow = torch.int32 if name != "huge" and k % 2 else torch.int64
    row, col = gpu(r, narrow), gpu(c, narrow)
    want = nr.lookup_ref(k)[0]
    got = adj.edge_ids(row, col) if k % 2 else psa.edge_ids(adj, row, col)
    assert tuple(got.shape) == (Q,) and same(got, want)
    has = adj.has_edge(row, col, trust_data=True) if k % 2 else psa.has_edge(adj, row, col)
    assert has.dtype == torch.bool and np.array_equal(has.cpu().numpy(), want >= 0)


@pytest.mark.parametrize("k", range(len(nr.SAMPLE_CASES)))
def test_sample_case_table_bit_exact(k):
    import paddle_sparse_amd as psa

    name, given, S, kk, loops = nr.SAMPLE_CASES[k]
    adj = case_adj(name)
    row, cols, flags = nr.sample_ref(k)
    assert flags == 0  # no failed sample in the restatement: none on the GPU, by equality
    kw = dict(no_self_loops=loops, max_tries=nr.CASE_MAX_TRIES, seed=nr.CASE_SEED + k)
    if given:
        src = gpu(nr.case_src(name, S), torch.int32 if k % 2 else torch.int64)
        got = adj.structured_negative_sampling(src, kk, **kw) if k % 2 else \
            psa.structured_negative_sampling(adj, src, kk, **kw)
        assert tuple(got.shape) == (S, kk) and same(got, cols)
    else:
        got = adj.negative_sampling(S, **kw) if k % 2 else psa.negative_sampling(adj, S, **kw)
        assert tuple(got[0].shape) == tuple(got[1].shape) == (S,)
        assert same(got[0], row) and same(got[1], cols)


# ---- hand answers --------------------------------------------------------------------------------------
def test_tiny_matrix_answers():
    rowptr, col, M, N = nr.tiny()
    adj = adj_of(rowptr, col, N=N)
    assert adj.edge_ids(gpu([0, 3, 0, 0, 1, 1, 0, 2, 4, 4]), gpu([3, 2, 1, 6, 0, 7, 7, 3, 4, 5])).tolist() \
        == [1, 7, 0, 4, 5, 6, -1, -1, 9, -1]
    assert adj.has_edge(gpu([0, 2]), gpu([3, 3])).tolist() == [True, False]
    empty = adj.edge_ids(gpu([]), gpu([]))
    assert empty.dtype == torch.int64 and tuple(empty.shape) == (0,) and empty.is_cuda


@pytest.mark.parametrize("free", [0, 5, 7])
def test_one_free_column_a_full_row_and_a_free_diagonal(free):
    rowptr, col, M, N = nr.one_free(free)
    adj = adj_of(rowptr, col, N=N)
    src = gpu(np.arange(N).repeat(3))
    got = adj.structured_negative_sampling(src, 2, max_tries=32768, seed=11)
    assert got[:-3].tolist() == [[free, free]] * (3 * (N - 1)) and got[-3:].tolist() == [[-1, -1]] * 3  # the full row
    if free < N - 1:
        # row `free` has only its diagonal free
        got = adj.structured_negative_sampling(gpu([free, (free + 1) % (N - 1)]), 4, no_self_loops=True,
                                               max_tries=2048, seed=2)
        assert got.tolist() == [[-1] * 4, [free] * 4]


def test_matrices_without_rows_columns_or_entries():
    for M, N in ((0, 0), (0, 5), (5, 0)):
        adj = adj_of(np.zeros(M + 1, np.int64), np.zeros(0, np.int64), N=N)
        row, col = adj.negative_sampling(70, seed=1)
        assert row.tolist() == [-1] * 70 and col.tolist() == [-1] * 70
    assert adj.structured_negative_sampling(gpu([0, 4]), 2, seed=1).tolist() == [[-1, -1], [-1, -1]]
    row, col = adj.negative_sampling(0, seed=1)
    assert tuple(row.shape) == tuple(col.shape) == (0,) and row.dtype == col.dtype == torch.int64
    out = case_adj("empty").structured_negative_sampling(gpu([]), 3, seed=1)
    assert tuple(out.shape) == (0, 3) and out.dtype == torch.int64


# ---- out-of-range queries and sources --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "huge"])
def test_queries_outside_the_matrix(name):
    from paddle_sparse_amd import ops

    adj = case_adj(name)
    rowptr, col, M, N = nr.case_graph(name)
    r, c = (a.copy() for a in nr.case_queries(name, 257))
    want = nr.ref_edge_lookup(rowptr, col, M, N, r, c)[0]
    assert torch.equal(adj.edge_ids(gpu(r), gpu(c)), gpu(want))
    for at, (br, bc) in ((0, (-1, 0)), (64, (M, 0)), (255, (0, -1)), (256, (0, N)), (100, (2**62, -2**63))):
        rr, cc = r.copy(), c.copy()
        rr[at], cc[at] = br, bc
        ref, flags = nr.ref_edge_lookup(rowptr, col, M, N, rr, cc)
        assert flags == 1 and ref[at] == -1
        got = adj.edge_ids(gpu(rr), gpu(cc), trust_data=True)
        assert same(got, ref)
        assert np.array_equal(adj.has_edge(gpu(rr), gpu(cc), trust_data=True).cpu().numpy(), ref >= 0)
        pos, f = ops.edge_lookup(*adj.csr()[:2], N, gpu(rr), gpu(cc))
        assert f.tolist() == [1] and same(pos, ref)
        with pytest.raises(IndexError, match="edge_ids"):
            adj.edge_ids(gpu(rr), gpu(cc))
        with pytest.raises(IndexError):
            adj.has_edge(gpu(rr), gpu(cc))


@pytest.mark.parametrize("name", ["rect", "degs"])
def test_sources_outside_the_matrix(name):
    from paddle_sparse_amd import ops

    adj = case_adj(name)
    rowptr, col, M, N = nr.case_graph(name)
    for at, bad in ((0, -1), (64, M), (86, 2**62), (5, -2**63)):
        src = nr.case_src(name, 87).copy()
        src[at] = bad
        _, ref, flags = nr.ref_negative_sample(rowptr, col, M, N, src, 3, False, 64, 17)
        assert flags == 1 and ref[3 * at:3 * at + 3].tolist() == [-1] * 3 and (ref >= 0).sum() == 3 * 86
        got = adj.structured_negative_sampling(gpu(src), 3, seed=17, trust_data=True)
        assert tuple(got.shape) == (87, 3) and same(got, ref)
        cols, f = ops.negative_sample(*adj.csr()[:2], N, gpu(src), 3, False, 64, 17)
        assert f.tolist() == [1] and same(cols, ref)
        with pytest.raises(IndexError, match="structured_negative_sampling"):
            adj.structured_negative_sampling(gpu(src), 3, seed=17)


# ---- properties that do not depend on the restatement ---------------------------------------------------------
@pytest.mark.parametrize("name,loops", [("degs", False), ("degs", True), ("rect", False), ("huge", False)])
def test_returned_pairs_are_not_stored(name, loops):
    adj = case_adj(name)
    rowptr, col, M, N = nr.case_graph(name)
    stored = nr.stored_pairs(name)
    n = 20000
    row, cols = adj.negative_sampling(n, no_self_loops=loops, seed=41)
    row, cols = row.cpu().numpy(), cols.cpu().numpy()
    src = np.arange(n // 4) % M
    tails = adj.structured_negative_sampling(gpu(src), 4, no_self_loops=loops, seed=42).cpu().numpy()
    for r, c in ((row, cols), (src.repeat(4), tails.reshape(-1))):
        assert ((c >= 0) & (c < N) & (r >= 0) & (r < M)).all()  # no failed sample: the share the restatement has
        assert not stored.intersection(zip(r.tolist(), c.tolist()))
        if loops:
            assert (r != c).all()
        assert len(set(zip(r.tolist(), c.tolist()))) > (100 if name != "rect" else 50)
    # the restatement, asked the same: no failure either, and the same bits
    ref = nr.ref_negative_sample(rowptr, col, M, N, None, 2000, loops, 64, 41)
    assert ref[2] == 0 and np.array_equal(ref[0], row[:2000]) and np.array_equal(ref[1], cols[:2000])


@pytest.mark.parametrize("name", ["degs", "rect", "huge"])
def test_edge_ids_lead_to_the_query_and_minus_one_means_not_stored(name):
    adj = case_adj(name)
    rowptr, col, M, N = nr.case_graph(name)
    stored = nr.stored_pairs(name)
    r = np.concatenate([nr.coo_rows(rowptr), nr.case_queries(name, 1000)[0]])
    c = np.concatenate([col, nr.case_queries(name, 1000)[1]])
    e = adj.edge_ids(gpu(r), gpu(c)).cpu().numpy()
    found = e >= 0
    assert found[:len(col)].all() and (~found).any()
    srow, scol = nr.coo_rows(rowptr), col  # the storage's order
    assert np.array_equal(srow[e[found]], r[found]) and np.array_equal(scol[e[found]], c[found])
    assert (e[~found] == -1).all() and not stored.intersection(zip(r[~found].tolist(), c[~found].tolist()))
    # every stored entry finds the FIRST of its duplicates: no earlier position holds the same pair
    first = e[:len(col)]
    assert (first <= np.arange(len(col))).all()
    dup = first < np.arange(len(col))
    assert dup.any() or name == "rect"
    assert np.array_equal(scol[first], col)
    assert ((first == 0) | (scol[first - 1] != col) | (srow[first - 1] != srow[first])).all()
    # a value tensor is indexed by the result
    value = torch.arange(len(col), device="cuda", dtype=torch.float32)
    weighted = adj.set_value(value, layout="coo")
    ids = weighted.edge_ids(gpu(r[found]), gpu(c[found]))
    assert torch.equal(weighted.storage.value()[ids], gpu(e[found], torch.float32))


def test_uniformity_on_the_gpu_is_the_cpu_suites():
    rowptr, col, M, N = nr.row16()
    cols = adj_of(rowptr, col, N=N).structured_negative_sampling(
        torch.zeros(nr.UNIFORM_S, dtype=torch.int64, device="cuda"), seed=nr.ROW16_SEED).cpu().numpy().reshape(-1)
    sigma = nr.row16_sigmas(cols)
    print(f"row of 16 with 6 stored: largest deviation {sigma:.2f} sigma")
    assert sigma < 5
    rowptr, col, M, N = nr.square12()
    row, cols = adj_of(rowptr, col, N=N).negative_sampling(nr.UNIFORM_S, seed=nr.SQUARE12_SEED)
    sigma = nr.square12_sigmas(row.cpu().numpy(), cols.cpu().numpy())
    print(f"12 x 12 at density 0.5: largest deviation {sigma:.2f} sigma")
    assert sigma < 5


# ---- determinism, capture, poison ------------------------------------------------------------------------------
def test_seeds_and_the_default_seed():
    adj = case_adj("degs")
    src = gpu(nr.case_src("degs", 257))
    big = 2**63 + 11
    a, b, c = (adj.negative_sampling(1000, seed=s) for s in (big, big, big + 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    a, b, c = (adj.structured_negative_sampling(src, 3, seed=s) for s in (big, big, big + 1))
    assert torch.equal(a, b) and not torch.equal(a, c)
    strided = torch.stack([src, src + 1], 1)[:, 0]
    assert not strided.is_contiguous() and torch.equal(adj.structured_negative_sampling(strided, 3, seed=big), a)
    # seed=None: torch's CPU generator
    torch.manual_seed(5)
    a = adj.negative_sampling(1000)
    b = adj.negative_sampling(1000)
    torch.manual_seed(5)
    c = adj.negative_sampling(1000)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and not torch.equal(a[1], b[1])


def test_the_trusting_forms_replay_from_a_hip_graph():
    adj = case_adj("degs")
    rowptr, col, M, N = nr.case_graph("degs")
    r, c = nr.case_queries("degs", 257)
    row_q, col_q, src = gpu(r), gpu(c), gpu(nr.case_src("degs", 257))
    adj.csr()
    out = {}

    def run():  # a single chain on one stream
        out["e"] = adj.edge_ids(row_q, col_q, trust_data=True)
        out["h"] = adj.has_edge(row_q, col_q, trust_data=True)
        out["neg"] = adj.negative_sampling(257, no_self_loops=True, seed=4242)
        out["tails"] = adj.structured_negative_sampling(src, 3, seed=4243, trust_data=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = {k: (tuple(x.clone() for x in v) if isinstance(v, tuple) else v.clone()) for k, v in out.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for v in out.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            x.fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for k in ("e", "h", "tails"):
        assert torch.equal(out[k], eager[k]), k
    assert torch.equal(out["neg"][0], eager["neg"][0]) and torch.equal(out["neg"][1], eager["neg"][1])
    assert same(out["e"], nr.ref_edge_lookup(rowptr, col, M, N, r, c)[0])
    ref = nr.ref_negative_sample(rowptr, col, M, N, None, 257, True, 64, 4242)
    assert same(out["neg"][0], ref[0]) and same(out["neg"][1], ref[1])
    src_np = nr.case_src("degs", 257)
    assert same(out["tails"], nr.ref_negative_sample(rowptr, col, M, N, src_np, 3, False, 64, 4243)[1])
    # new queries and sources in the captured buffers
    row_q.copy_(gpu(r[::-1].copy())), col_q.copy_(gpu(c[::-1].copy())), src.copy_(gpu(src_np[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert same(out["e"], nr.ref_edge_lookup(rowptr, col, M, N, r[::-1], c[::-1])[0])
    assert same(out["tails"], nr.ref_negative_sample(rowptr, col, M, N, src_np[::-1], 3, False, 64, 4243)[1])


@pytest.fixture
def poisoned():
    from paddle_sparse_amd import ops

    old, ops._POISON_WORKSPACE = ops._POISON_WORKSPACE, True
    yield ops
    ops._POISON_WORKSPACE = old


@pytest.mark.parametrize("name", ["degs", "empty"])
def test_every_output_element_is_written(name, poisoned):
    ops = poisoned
    adj = case_adj(name)
    rowptr, col, M, N = nr.case_graph(name)
    csr = adj.csr()[:2]
    SENTINEL = -(2**61) - 5
    for n in (1, 255, 257, 1000):
        r, c = (a.copy() for a in nr.case_queries(name, n))
        r[0], c[-1] = -1, N  # out-of-range queries are written too
        src = nr.case_src(name, n).copy()
        src[0] = M
        full = lambda: torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")  # noqa: E731
        pos, _ = ops.edge_lookup(*csr, N, gpu(r), gpu(c), out=full())
        assert same(pos, nr.ref_edge_lookup(rowptr, col, M, N, r, c)[0])
        row, cols, _ = ops.negative_sample(*csr, N, None, n, True, 64, 3, out_row=full(), out_col=full())
        tails, _ = ops.negative_sample(*csr, N, gpu(src), 1, False, 64, 3, out_col=full())
        ref = nr.ref_negative_sample(rowptr, col, M, N, src, 1, False, 64, 3)
        assert same(tails, ref[1]) and ref[2] == 1
        for x in (pos, row, cols, tails):
            assert not (x == SENTINEL).any()
        # outputs allocated by the ops start as poison under the hook
        outs = (adj.edge_ids(gpu(r), gpu(c), trust_data=True), *adj.negative_sampling(n, seed=3),
                adj.structured_negative_sampling(gpu(src), 2, seed=3, trust_data=True))
        for x in outs:
            assert not (x == ops.NEGATIVE_POISON).any() and (x >= -1).all()
