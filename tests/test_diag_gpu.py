"""GPU suite for the diagonal ops.  The results are pure data movement, so every
comparison is bit-exact against a restatement of the semantics (numpy for the
structure, CPU torch indexing for the value bytes) kept in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64]


# ---- the semantics, restated -------------------------------------------------------
def extent(M, N, k):
    n = min(M, N - k) if k >= 0 else min(M + k, N)
    return max(-k, 0), max(n, 0)


def ref_rewrite(rowptr, col, value, M, N, k, insert, diag_values):
    """(rowptr', col', value', out_pos, diag_pos) of remove_diag (insert=False) / set_diag."""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    row = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr))
    keep = np.nonzero(col != row + k)[0]
    start, nd = extent(M, N, k)
    d_rows = np.arange(start, start + nd, dtype=np.int64) if insert else np.zeros(0, np.int64)
    all_row = np.concatenate([row[keep], d_rows])
    all_col = np.concatenate([col[keep], d_rows + k])
    order = np.lexsort((all_col, all_row))  # stable: kept duplicates keep their order
    new_row, new_col = all_row[order], all_col[order]
    slot = np.empty_like(order)
    slot[order] = np.arange(order.size)
    out_pos = np.full(col.size, -1, np.int64)
    out_pos[keep] = slot[:keep.size]
    diag_pos = slot[keep.size:]
    new_rowptr = np.searchsorted(new_row, np.arange(M + 1), side="left").astype(np.int64)
    new_value = None
    if value is not None:
        v = value.cpu()
        new_value = torch.empty((order.size,) + tuple(v.shape[1:]), dtype=v.dtype)
        new_value[torch.from_numpy(out_pos[keep])] = v[torch.from_numpy(keep)]
        if insert:
            new_value[torch.from_numpy(diag_pos)] = diag_values.cpu()
    return new_rowptr, new_col, new_value, out_pos, diag_pos


def ref_get_diag(rowptr, col, value, M, N):
    D = min(M, N)
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    pos = np.full(D, -1, np.int64)
    for r in range(D):
        hit = np.nonzero(col[rowptr[r]:rowptr[r + 1]] == r)[0]
        if hit.size:
            pos[r] = rowptr[r] + hit[-1]
    if value is None:
        return torch.from_numpy((pos >= 0).astype(np.float32)), pos
    v = value.cpu()
    out = torch.zeros((D,) + tuple(v.shape[1:]), dtype=v.dtype)
    got = np.nonzero(pos >= 0)[0]
    out[torch.from_numpy(got)] = v[torch.from_numpy(pos[got])]
    return out, pos


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)


def random_values(nnz, dtype, trailing=(), seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        v = torch.randn((nnz,) + trailing, generator=g, dtype=torch.float64).to(dtype)
    else:
        v = torch.randint(-1000, 1000, (nnz,) + trailing, generator=g, dtype=dtype)
    return v.cuda()


def diag_matrix(M, N, seed, nnz=None, k=0):
    """Sorted (rowptr, col) with rows that hold one diagonal entry, several duplicate ones,
    none, and empty rows (before and after the diagonal)."""
    rng = np.random.default_rng(seed)
    nnz = 4 * max(M, 1) if nnz is None else nnz
    row = rng.integers(0, M, nnz) if M and N else np.zeros(0, np.int64)
    col = rng.integers(0, N, nnz) if M and N else np.zeros(0, np.int64)
    start, nd = extent(M, N, k)
    if nd:
        r = rng.integers(start, start + nd, max(nd // 2, 1))
        dup = r[: max(r.size // 3, 1)]
        row = np.concatenate([row, r, dup, dup])
        col = np.concatenate([col, r + k, dup + k, dup + k])
    keep_rows = rng.random(row.size) < 0.8  # empty rows appear
    row, col = row[keep_rows], col[keep_rows]
    if M > 3:  # a row empty on both sides of the diagonal and a row with only the diagonal
        sel = (row != 1) & (row != 2)
        row, col = row[sel], col[sel]
        if on(2, M, N, k):
            row, col = np.append(row, [2, 2]), np.append(col, [2 + k, 2 + k])
    order = np.lexsort((col, row))
    row, col = row[order].astype(np.int64), col[order].astype(np.int64)
    rowptr = np.searchsorted(row, np.arange(M + 1), side="left").astype(np.int64)
    return row, rowptr, col


def on(r, M, N, k):
    return 0 <= r < M and 0 <= r + k < N


def build(row, rowptr, col, value, M, N, how):
    from paddle_sparse_amd import SparseTensor

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if how == "coo":
        return SparseTensor(row=d(row), col=d(col), value=value, sparse_sizes=(M, N), is_sorted=True)
    return SparseTensor(rowptr=d(rowptr), col=d(col), value=value, sparse_sizes=(M, N), is_sorted=True)


def check_result(out, M, N, ref_rowptr, ref_col, ref_value):
    st = out.storage
    assert st.sparse_sizes() == (M, N)
    assert np.array_equal(st.rowptr().cpu().numpy(), ref_rowptr)
    assert np.array_equal(st.col().cpu().numpy(), ref_col)
    if ref_value is None:
        assert st.value() is None
    else:
        assert st.value().dtype == ref_value.dtype and tuple(st.value().shape) == tuple(ref_value.shape)
        assert np.array_equal(bits(st.value()), bits(ref_value))
    # caches equal recomputation, the order is sorted
    assert np.array_equal(st._rowcount.cpu().numpy(), np.diff(ref_rowptr))
    row = st.row().cpu().numpy()
    assert np.array_equal(row, np.repeat(np.arange(M), np.diff(ref_rowptr)))
    keys = row * max(N, 1) + ref_col
    assert np.all(keys[1:] >= keys[:-1])
    if st._colcount is not None:
        assert np.array_equal(st._colcount.cpu().numpy(), np.bincount(ref_col, minlength=N))
    assert st._colptr is None and st._csr2csc is None and st._csc2csr is None


SHAPES = [(40, 40), (30, 50), (50, 30), (0, 5), (6, 0), (1, 1)]
KS = [-3, -1, 0, 2, 60, -60]


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("how", ["coo", "csr"])
def test_remove_and_set_diag_structure_and_caches(M, N, k, how):
    import paddle_sparse_amd as psa

    row, rowptr, col = diag_matrix(M, N, seed=M * 7 + N + k % 11, k=k)
    value = random_values(col.size, torch.float32, seed=1)
    a = build(row, rowptr, col, value, M, N, how)
    a.storage.colcount()  # cached: the result carries it, adjusted
    before = (a.storage.col().clone(), value.clone(), a.storage.rowptr().clone())
    start, nd = extent(M, N, k)
    vals = random_values(nd, torch.float32, seed=2)
    for op, insert, dv in (("remove_diag", False, None), ("set_diag", True, vals)):
        out = psa.remove_diag(a, k) if op == "remove_diag" else psa.set_diag(a, vals, k)
        ref = ref_rewrite(rowptr, col, value, M, N, k, insert, dv)
        check_result(out, M, N, ref[0], ref[1], ref[2])
        assert out.storage._colcount is not None
    # the method forms, and the input untouched
    assert torch.equal(a.remove_diag(k).storage.col(), psa.remove_diag(a, k).storage.col())
    assert torch.equal(a.fill_diag(3.0, k).storage.value(), psa.set_diag(a, torch.full((nd,), 3.0), k).storage.value())
    assert torch.equal(a.storage.col(), before[0]) and torch.equal(a.storage.value(), before[1])
    assert torch.equal(a.storage.rowptr(), before[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("trailing", [(), (3,)])
@pytest.mark.parametrize("k", [-1, 0, 2])
def test_values_of_every_dtype(dtype, trailing, k):
    import paddle_sparse_amd as psa

    M, N = 45, 38
    row, rowptr, col = diag_matrix(M, N, seed=5, k=k)
    value = random_values(col.size, dtype, trailing, seed=3)
    a = build(row, rowptr, col, value, M, N, "csr")
    start, nd = extent(M, N, k)
    given = random_values(nd, dtype, trailing, seed=4)
    cases = {
        "remove": (psa.remove_diag(a, k), False, None),
        "set_given": (psa.set_diag(a, given, k), True, given),
        "set_none": (psa.set_diag(a, None, k), True, torch.ones((nd,) + trailing, dtype=dtype)),
        "fill": (psa.fill_diag(a, 7, k), True, torch.full((nd,) + trailing, 7, dtype=dtype)),
    }
    if trailing:  # one value per diagonal cell, broadcast along the trailing dimension
        col_vals = random_values(nd, dtype, (1,), seed=6)
        cases["set_broadcast"] = (psa.set_diag(a, col_vals, k), True, col_vals.expand(nd, *trailing))
    cases["set_cast"] = (psa.set_diag(a, torch.full((nd,) + trailing, 2.0, dtype=torch.float64), k), True,
                         torch.full((nd,) + trailing, 2.0, dtype=torch.float64).to(dtype))
    for name, (out, insert, dv) in cases.items():
        ref = ref_rewrite(rowptr, col, value, M, N, k, insert, dv)
        check_result(out, M, N, ref[0], ref[1], ref[2])
    got = psa.get_diag(a)
    want, _ = ref_get_diag(rowptr, col, value, M, N)
    assert got.dtype == dtype and np.array_equal(bits(got), bits(want)), name


@pytest.mark.parametrize("k", [-2, 0, 1])
def test_value_less_matrices_stay_value_less(k):
    import paddle_sparse_amd as psa

    M, N = 33, 29
    row, rowptr, col = diag_matrix(M, N, seed=9, k=k)
    a = build(row, rowptr, col, None, M, N, "coo")
    for out, insert in ((psa.remove_diag(a, k), False), (psa.set_diag(a, torch.ones(3), k), True),
                        (psa.fill_diag(a, 2.0, k), True)):
        ref = ref_rewrite(rowptr, col, None, M, N, k, insert, None)
        check_result(out, M, N, ref[0], ref[1], None)
    got = psa.get_diag(a)
    want, _ = ref_get_diag(rowptr, col, None, M, N)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)


def test_empty_matrices():
    import paddle_sparse_amd as psa

    for M, N in ((0, 0), (0, 3), (3, 0), (4, 4)):
        a = build(np.zeros(0, np.int64), np.zeros(M + 1, np.int64), np.zeros(0, np.int64),
                  torch.zeros(0, device="cuda"), M, N, "csr")
        r = psa.remove_diag(a)
        assert r.nnz() == 0 and r.storage.rowptr().tolist() == [0] * (M + 1)
        f = psa.fill_diag(a, 5.0)
        assert f.storage.col().tolist() == list(range(min(M, N)))
        assert f.storage.value().tolist() == [5.0] * min(M, N)
        assert psa.get_diag(a).tolist() == [0.0] * min(M, N)


def test_hub_row_is_split_over_tiles():
    """A row of 70 000 entries with its diagonal entry in the middle (twice) next to short
    rows: the write pass must split it over many workgroups."""
    import paddle_sparse_amd as psa

    M = N = 80_000
    hub = 40_000
    hub_cols = np.sort(np.concatenate([np.delete(np.arange(70_000, dtype=np.int64), hub), [hub, hub]]))
    deg = np.full(M, 2, np.int64)
    deg[hub] = hub_cols.size
    rowptr = np.zeros(M + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = np.empty(rowptr[-1], np.int64)
    rng = np.random.default_rng(1)
    short = np.sort(rng.integers(0, N, (M, 2)), axis=1)
    short[::3, 0] = np.arange(0, M, 3)  # a diagonal entry in every third row
    short = np.sort(short, axis=1)
    for r in range(M):
        if r != hub:
            col[rowptr[r]:rowptr[r + 1]] = short[r]
    col[rowptr[hub]:rowptr[hub + 1]] = hub_cols
    assert hub_cols.size > 65_535
    value = random_values(col.size, torch.float32, seed=8)
    a = build(None, rowptr, col, value, M, N, "csr")
    for out, insert, dv in ((psa.remove_diag(a), False, None),
                            (psa.fill_diag(a, -1.0), True, torch.full((M,), -1.0))):
        ref = ref_rewrite(rowptr, col, value, M, N, 0, insert, dv)
        check_result(out, M, N, ref[0], ref[1], ref[2])
    want, _ = ref_get_diag(rowptr, col, value, M, N)
    assert torch.equal(psa.get_diag(a).cpu(), want)


# ---- autograd --------------------------------------------------------------------
@pytest.mark.parametrize("k", [-1, 0, 3])
@pytest.mark.parametrize("trailing", [(), (2,)])
def test_gradients_flow_through_every_op(k, trailing):
    import paddle_sparse_amd as psa

    M, N = 60, 50
    row, rowptr, col = diag_matrix(M, N, seed=11, k=k)
    start, nd = extent(M, N, k)
    for op in ("remove_diag", "set_diag", "fill_diag"):
        value = random_values(col.size, torch.float32, trailing, seed=12).requires_grad_(True)
        vals = random_values(nd, torch.float32, trailing, seed=13).requires_grad_(True)
        a = build(row, rowptr, col, value, M, N, "csr")
        out = {"remove_diag": lambda: psa.remove_diag(a, k), "set_diag": lambda: psa.set_diag(a, vals, k),
               "fill_diag": lambda: psa.fill_diag(a, 0.5, k)}[op]()
        w = random_values(out.nnz(), torch.float32, trailing, seed=14)
        (out.storage.value() * w).sum().backward()
        _, _, _, out_pos, diag_pos = ref_rewrite(rowptr, col, None, M, N, k, op != "remove_diag", None)
        wc = w.cpu()
        want = torch.zeros_like(value.cpu())
        kept = np.nonzero(out_pos >= 0)[0]
        want[torch.from_numpy(kept)] = wc[torch.from_numpy(out_pos[kept])]
        assert torch.equal(value.grad.cpu(), want), op
        if op == "set_diag":
            assert torch.equal(vals.grad.cpu(), wc[torch.from_numpy(diag_pos)])
    value = random_values(col.size, torch.float32, trailing, seed=15).requires_grad_(True)
    a = build(row, rowptr, col, value, M, N, "coo")
    d = psa.get_diag(a)
    w = random_values(d.shape[0], torch.float32, trailing, seed=16)
    (d * w).sum().backward()
    _, pos = ref_get_diag(rowptr, col, None, M, N)
    want = torch.zeros_like(value.cpu())
    got = np.nonzero(pos >= 0)[0]
    want[torch.from_numpy(pos[got])] = w.cpu()[torch.from_numpy(got)]
    assert torch.equal(value.grad.cpu(), want)


def test_fill_diag_then_matmul_trains_both_operands():
    """fp32 fill_diag -> matmul, both gradients against a float64 dense computation."""
    import paddle_sparse_amd as psa

    M, N, K = 300, 300, 16
    row, rowptr, col = diag_matrix(M, N, seed=21)
    value = random_values(col.size, torch.float32, seed=22).requires_grad_(True)
    X = random_values(N, torch.float32, (K,), seed=23).requires_grad_(True)
    G = random_values(M, torch.float32, (K,), seed=24)
    a = build(row, rowptr, col, value, M, N, "csr")
    out = psa.fill_diag(a, 2.0).matmul(X)
    out.backward(G)

    v64 = value.detach().double().requires_grad_(True)
    X64 = X.detach().double().requires_grad_(True)
    r, c = torch.from_numpy(row).cuda(), torch.from_numpy(col).cuda()
    dense = torch.zeros(M, N, dtype=torch.float64, device="cuda").index_put((r, c), v64, accumulate=True)
    eye = torch.eye(M, N, dtype=torch.float64, device="cuda")
    ref = ((dense * (1 - eye) + 2.0 * eye) @ X64)
    ref.backward(G.double())
    scale = (dense.abs() + eye) @ X64.abs()
    assert torch.all((out.double() - ref).abs() <= 1e-5 * scale + 1e-30)
    assert torch.allclose(X.grad.double(), X64.grad, rtol=1e-5, atol=1e-5)
    assert torch.allclose(value.grad.double(), v64.grad, rtol=1e-5, atol=1e-5)
    off = torch.from_numpy(row != col).cuda()
    assert torch.all(value.grad[~off] == 0)


def test_gcn_normalisation_end_to_end():
    """fill_diag(1) -> sum(dim=1) -> pow(-1/2) -> mul by rows and columns -> @ x against float64
    scipy D^-1/2 (A + I) D^-1/2 X."""
    import scipy.sparse as sp

    import paddle_sparse_amd as psa

    rng = np.random.default_rng(31)
    n, e, K = 3000, 20_000, 32
    r, c = rng.integers(0, n, e), rng.integers(0, n, e)
    A = sp.coo_matrix((np.ones(e), (r, c)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64)
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    x = rng.standard_normal((n, K))
    adj = psa.SparseTensor(rowptr=torch.from_numpy(A.indptr.astype(np.int64)).cuda(),
                           col=torch.from_numpy(A.indices.astype(np.int64)).cuda(),
                           value=torch.ones(A.nnz, device="cuda"), sparse_sizes=(n, n), is_sorted=True)
    adj = psa.fill_diag(adj, 1.0)
    deg = psa.sum(adj, dim=1)
    dis = deg.pow(-0.5)
    adj = psa.mul(adj, dis.view(-1, 1))
    adj = psa.mul(adj, dis.view(1, -1))
    out = (adj @ torch.from_numpy(x).float().cuda()).double().cpu().numpy()
    Ah = A + sp.identity(n)
    d = np.asarray(Ah.sum(axis=1)).ravel() ** -0.5
    ref = sp.diags(d) @ Ah @ sp.diags(d) @ x
    scale = abs(sp.diags(d) @ Ah @ sp.diags(d)) @ np.abs(x)
    assert np.all(np.abs(out - ref) <= 1e-5 * scale + 1e-30)


# ---- full size -----------------------------------------------------------------------
def torch_remove(rowptr, col, value, M, N, k):
    row = torch.repeat_interleave(torch.arange(M, device=col.device), rowptr[1:] - rowptr[:-1])
    mask = col != row + k
    new_row, new_col, new_val = row[mask], col[mask], value[mask]
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=col.device),
                      torch.cumsum(torch.bincount(new_row, minlength=M), 0)]), new_col, new_val


def torch_fill(rowptr, col, value, M, N, k, fill):
    start, nd = extent(M, N, k)
    row = torch.repeat_interleave(torch.arange(M, device=col.device), rowptr[1:] - rowptr[:-1])
    mask = col != row + k
    d = torch.arange(start, start + nd, device=col.device)
    keys = torch.cat([row[mask] * N + col[mask], d * N + d + k])
    vals = torch.cat([value[mask], torch.full((nd,), fill, dtype=value.dtype, device=col.device)])
    keys, order = torch.sort(keys, stable=True)
    new_row = keys // N
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=col.device),
                      torch.cumsum(torch.bincount(new_row, minlength=M), 0)]), keys % N, vals[order]


def rmat21():
    from paddle_sparse_amd import coalesce, ops

    scale, n = 21, 20_000_000
    size = 1 << scale
    g = torch.Generator(device="cuda").manual_seed(4)
    row = torch.zeros(n, dtype=torch.int64, device="cuda")
    col = torch.zeros(n, dtype=torch.int64, device="cuda")
    for bit in range(scale):
        r = torch.rand(n, generator=g, device="cuda")
        row |= (r >= 0.76).to(torch.int64) << bit
        col |= (((r >= 0.57) & (r < 0.76)) | (r >= 0.95)).to(torch.int64) << bit
    index, val = coalesce(torch.stack([row, col]), torch.randn(n, generator=g, device="cuda"), size, size)
    return size, size, ops.ind2ptr(index[0].contiguous(), size), index[1].contiguous(), val


def config3():
    M = N = 2_000_000
    nnz = 20_000_000
    g = torch.Generator(device="cuda").manual_seed(3)
    keys = torch.sort(torch.randint(0, M, (nnz,), generator=g, device="cuda") * N
                      + torch.randint(0, N, (nnz,), generator=g, device="cuda"))[0]
    row, col = keys // N, keys % N
    # a diagonal entry in every tenth row (twice in every thirtieth)
    d = torch.arange(0, M, 10, device="cuda")
    dd = torch.arange(0, M, 30, device="cuda")
    keys = torch.sort(torch.cat([keys, d * N + d, dd * N + dd]))[0]
    from paddle_sparse_amd import ops

    return M, N, ops.ind2ptr(keys // N, M), keys % N, torch.randn(keys.numel(), generator=g, device="cuda")


@pytest.mark.parametrize("graph", ["config3", "rmat21"])
def test_full_size_equals_the_torch_composition(graph):
    import paddle_sparse_amd as psa

    M, N, rowptr, col, val = config3() if graph == "config3" else rmat21()
    a = psa.SparseTensor(rowptr=rowptr, col=col, value=val, sparse_sizes=(M, N), is_sorted=True, trust_data=True)
    for k in (0, -1):
        out = psa.remove_diag(a, k)
        p, c, v = torch_remove(rowptr, col, val, M, N, k)
        assert torch.equal(out.storage.rowptr(), p) and torch.equal(out.storage.col(), c)
        assert torch.equal(out.storage.value().view(torch.int32), v.view(torch.int32))
        out = psa.fill_diag(a, 1.0, k)
        p, c, v = torch_fill(rowptr, col, val, M, N, k, 1.0)
        assert torch.equal(out.storage.rowptr(), p) and torch.equal(out.storage.col(), c)
        assert torch.equal(out.storage.value().view(torch.int32), v.view(torch.int32))
    row = torch.repeat_interleave(torch.arange(M, device="cuda"), rowptr[1:] - rowptr[:-1])
    diag = torch.zeros(min(M, N), device="cuda")
    mask = row == col
    idx = torch.nonzero(mask).view(-1)
    # the last stored entry wins: keep, per row, the largest position
    last = torch.full((M,), -1, dtype=torch.int64, device="cuda").scatter_reduce(0, row[idx], idx, "amax")
    have = last >= 0
    diag[have] = val[last[have]]
    assert torch.equal(psa.get_diag(a), diag)
