"""GPU suite of the multi-head ends of the attention path: SpMM over per-head values [nnz, H] with a
dense operand [N, H, F] (psa_spmm_heads) and sddmm with x [M, H, K], y [N, H, K] (psa_sddmm_heads).

Exact wherever it says so: values, dense operands and upstream gradients are small integers in
[-4, 4] / [-2, 2], so every sum stays below 2^24 (the longest row: 4099 * 16 * 1 for the forward, the
gradients are smaller) and the fp32 results must equal the float64 reference of tests/heads_ref.py bit
for bit, whatever the order of the additions.  One CSR pattern serves those tests: row lengths at the
lane-group and step edges, either side of the 128-entry chunk edge, and 33 chunks in one row."""
import numpy as np
import pytest
import torch

import heads_ref as hr

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4099]
N = 4200
# smallest shapes; a 4-byte form with nothing a power of two; several entries per wave step; exactly one
# 256-float tile; a head that straddles the tile edge; four tiles; one lane per head; more heads than lanes
SHAPES = [(1, 1), (1, 4), (2, 4), (3, 5), (4, 16), (8, 8), (8, 32), (5, 64), (16, 64), (64, 4), (65, 4), (2, 200)]
U = 2.0 ** -24


def pattern(rng, lens, n):
    """Sorted CSR pattern with the given row lengths, distinct columns inside a row."""
    cols = [np.sort(rng.choice(n, size=ln, replace=False)) for ln in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, dtype=np.int64)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def dev(a):
    return torch.from_numpy(a).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def offset_copy(t):
    """The same numbers in a view that starts 4 bytes into its allocation."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.fixture(scope="module")
def big():
    rowptr, col = pattern(np.random.default_rng(61), LENGTHS, N)
    return rowptr, col


def tensor_of(rowptr, col, n, value=None):
    import paddle_sparse_amd as psa

    return psa.SparseTensor(rowptr=dev(rowptr), col=dev(col), value=value, sparse_sizes=(rowptr.size - 1, n),
                            is_sorted=True)


# ---- SpMM over per-head values --------------------------------------------------------------------

@pytest.mark.parametrize("H,F", SHAPES)
def test_spmm_heads_exact_forward_and_gradients(big, H, F):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    rng = np.random.default_rng(1000 * H + F)
    value, mat, g = ints(rng, (nnz, H), -4, 4), ints(rng, (N, H, F), -4, 4), ints(rng, (M, H, F), -2, 2)
    want = hr.spmm_heads_ref(rowptr, col, value, mat)
    want_gv = hr.spmm_heads_grad_value(rowptr, col, mat, g)
    want_gm = hr.spmm_heads_grad_mat(rowptr, col, value, g, N)
    assert np.abs(want).max() < 2 ** 24 and np.abs(want_gm).max() < 2 ** 24 and np.abs(want_gv).max() < 2 ** 24

    vd, md = dev(value).requires_grad_(), dev(mat).requires_grad_()
    A = tensor_of(rowptr, col, N, vd)
    out = A @ md
    assert out.shape == (M, H, F) and out.dtype == torch.float32
    out.backward(dev(g))
    assert np.array_equal(host(out), want)
    assert not host(out)[0].any()  # the row without entries
    assert np.array_equal(host(vd.grad), want_gv)
    assert np.array_equal(host(md.grad), want_gm)
    assert torch.equal(A.matmul(md.detach(), "add"), out.detach())

    # bare (rowptr, col): the backward of mat sorts col itself
    vb, mb = dev(value).requires_grad_(), dev(mat).requires_grad_()
    out_b = ops.spmm_heads(dev(rowptr), dev(col), vb, mb)
    out_b.backward(dev(g))
    assert torch.equal(out_b.detach(), out.detach())
    assert torch.equal(vb.grad, vd.grad) and torch.equal(mb.grad, md.grad)

    # operands that start 4 bytes into an allocation
    out_o = ops.spmm_heads(dev(rowptr), dev(col), offset_copy(vd.detach()), offset_copy(md.detach()))
    assert torch.equal(out_o, out.detach())


# ---- sddmm per head -------------------------------------------------------------------------------

@pytest.mark.parametrize("H,K", SHAPES)
def test_sddmm_heads_exact_forward_and_gradients(big, H, K):
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    rng = np.random.default_rng(2000 * H + K)
    x, y, g = ints(rng, (M, H, K), -4, 4), ints(rng, (N, H, K), -4, 4), ints(rng, (nnz, H), -2, 2)
    want = hr.sddmm_heads_ref(rowptr, col, x, y)
    want_gx = hr.sddmm_heads_grad_x(rowptr, col, y, g)
    want_gy = hr.sddmm_heads_grad_y(rowptr, col, x, g, N)
    assert np.abs(want_gx).max() < 2 ** 24

    # the existing values of src are not read
    A = tensor_of(rowptr, col, N, torch.full((nnz,), float("nan"), device=DEV))
    xd, yd = dev(x).requires_grad_(), dev(y).requires_grad_()
    v = psa.sddmm(A, xd, yd).storage.value()
    assert v.shape == (nnz, H) and v.dtype == torch.float32
    v.backward(dev(g))
    assert np.array_equal(host(v), want)
    assert np.array_equal(host(xd.grad), want_gx)
    assert np.array_equal(host(yd.grad), want_gy)

    # bare (rowptr, col): the backward of y sorts col itself
    xb, yb = dev(x).requires_grad_(), dev(y).requires_grad_()
    vb = ops.sddmm(dev(rowptr), dev(col), xb, yb)
    vb.backward(dev(g))
    assert torch.equal(vb.detach(), v.detach())
    assert torch.equal(xb.grad, xd.grad) and torch.equal(yb.grad, yd.grad)

    # the method form, without autograd, on operands that start 4 bytes into an allocation
    assert torch.equal(A.sddmm(offset_copy(xd.detach()), offset_copy(yd.detach())).storage.value(), v.detach())


def test_sddmm_heads_duplicate_entries_score_alike():
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(62)
    row = np.array([0, 0, 0, 1, 3, 3, 3, 3, 4], dtype=np.int64)
    col = np.array([1, 1, 6, 0, 2, 2, 2, 5, 6], dtype=np.int64)
    M, n, H, K = 5, 7, 3, 5
    rowptr = np.searchsorted(row, np.arange(M + 1)).astype(np.int64)
    x, y, g = ints(rng, (M, H, K), -4, 4), ints(rng, (n, H, K), -4, 4), ints(rng, (col.size, H), -2, 2)
    A = psa.SparseTensor(row=dev(row), col=dev(col), sparse_sizes=(M, n), is_sorted=True)
    xd, yd = dev(x).requires_grad_(), dev(y).requires_grad_()
    out = A.sddmm(xd, yd)
    assert out.nnz() == col.size
    v = out.storage.value()
    v.backward(dev(g))
    got = host(v)
    assert np.array_equal(got, hr.sddmm_heads_ref(rowptr, col, x, y))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[4], got[5]) and np.array_equal(got[5], got[6])
    assert np.array_equal(host(xd.grad), hr.sddmm_heads_grad_x(rowptr, col, y, g))
    assert np.array_equal(host(yd.grad), hr.sddmm_heads_grad_y(rowptr, col, x, g, n))


@pytest.mark.parametrize("K", [4, 5, 64])
def test_one_head_given_as_3d_equals_the_2d_call(big, K):
    rowptr, col = big
    M = rowptr.size - 1
    rng = np.random.default_rng(63 + K)
    x, y = dev(ints(rng, (M, K), -4, 4)), dev(ints(rng, (N, K), -4, 4))
    A = tensor_of(rowptr, col, N)
    flat = A.sddmm(x, y).storage.value()
    heads = A.sddmm(x.view(M, 1, K), y.view(N, 1, K)).storage.value()
    assert flat.shape == (col.size,) and heads.shape == (col.size, 1)
    assert torch.equal(heads[:, 0], flat)


# ---- the multi-head attention step ----------------------------------------------------------------

def test_multi_head_attention_step_exact():
    """softmax(sddmm(A, q, k), 1) @ v with k identical across nodes per head: equal scores within a row and head,
    degrees that are powers of two, small integers everywhere, so the softmax is a dyadic rational.  Output,
    grad_v, grad_q (exactly 0) and grad_k equal dense float64 autograd bit for bit, and so does the per-head
    loop over the 2-D ops."""
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(64)
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 4, 2, 256, 1]
    M, n, H, K, F = len(lens), 300, 4, 4, 8
    rowptr, col = pattern(rng, lens, n)
    row = hr.rows_of(rowptr)
    q = ints(rng, (M, H, K), -2, 2)
    k = np.tile(ints(rng, (1, H, K), -2, 2), (n, 1, 1))
    v = ints(rng, (n, H, F), -2, 2)
    go = ints(rng, (M, H, F), -2, 2)

    qt, kt, vt = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (q, k, v))
    mask = torch.zeros(M, n, dtype=torch.bool)
    mask[torch.from_numpy(row), torch.from_numpy(col)] = True
    mask = mask[:, :, None]
    # missing entries at -inf; the row without entries at 0 instead, so that no NaN enters the dense backward
    fill = torch.where(mask.any(1, keepdim=True), torch.tensor(float("-inf"), dtype=torch.float64),
                       torch.tensor(0.0, dtype=torch.float64))
    scores = torch.where(mask, torch.einsum("mhk,nhk->mnh", qt, kt), fill.expand(M, n, H))
    att = torch.softmax(scores, dim=1)
    att = torch.where(mask, att, torch.zeros_like(att))
    dense = torch.einsum("mnh,nhf->mhf", att, vt)
    dense.backward(torch.from_numpy(go.astype(np.float64)))

    A = tensor_of(rowptr, col, n)
    qd, kd, vd = (dev(a).requires_grad_() for a in (q, k, v))
    out = psa.sddmm(A, qd, kd).softmax(dim=1) @ vd
    assert out.shape == (M, H, F)
    out.backward(dev(go))
    assert np.array_equal(host(out), dense.detach().numpy())
    assert np.array_equal(host(vd.grad), vt.grad.numpy())
    assert not host(qd.grad).any() and not qt.grad.numpy().any()
    assert np.array_equal(host(kd.grad), kt.grad.numpy())

    # one head at a time through the 2-D ops
    ql, kl, vl = (dev(a).requires_grad_() for a in (q, k, v))
    loop = torch.stack([psa.sddmm(A, ql[:, h], kl[:, h]).softmax(dim=1) @ vl[:, h] for h in range(H)], dim=1)
    loop.backward(dev(go))
    assert torch.equal(loop.detach(), out.detach())
    assert torch.equal(ql.grad, qd.grad) and torch.equal(kl.grad, kd.grad) and torch.equal(vl.grad, vd.grad)


# ---- scalar and absent values with a 3-D operand --------------------------------------------------

@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("with_value", [False, True])
def test_scalar_or_absent_values_with_a_3d_operand(reduce, with_value):
    rng = np.random.default_rng(65)
    lens = [0, 5, 130, 1, 0, 64, 3]
    M, n, H, F = len(lens), 150, 3, 4
    rowptr, col = pattern(rng, lens, n)
    value = dev(ints(rng, col.size, -4, 4)) if with_value else None
    A = tensor_of(rowptr, col, n, value)
    mat, g = ints(rng, (n, H, F), -4, 4), ints(rng, (M, H, F), -2, 2)
    m3 = dev(mat).requires_grad_()
    m2 = dev(mat.reshape(n, H * F)).requires_grad_()
    out3 = A.matmul(m3, reduce)
    out2 = A.matmul(m2, reduce)
    assert out3.shape == (M, H, F)
    assert torch.equal(out3.reshape(M, H * F), out2)
    out3.backward(dev(g))
    out2.backward(dev(g.reshape(M, H * F)))
    assert torch.equal(m3.grad.reshape(n, H * F), m2.grad)


# ---- rounding on non-integer data -----------------------------------------------------------------

@pytest.mark.parametrize("H,F", [(8, 32), (3, 5)])
def test_rounding_bound_on_normal_data(big, H, F):
    """|got - ref64| <= (L + 2) * 2^-24 * sum |terms|: the bound of any summation order of L fp32 products, with or
    without fma.  L = the row length for the SpMM, K for the sddmm."""
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    rng = np.random.default_rng(66 + H)
    value = rng.normal(size=(nnz, H)).astype(np.float32)
    mat = rng.normal(size=(N, H, F)).astype(np.float32)
    x = rng.normal(size=(M, H, F)).astype(np.float32)
    rp, cl = dev(rowptr), dev(col)

    got = host(ops.spmm_heads(rp, cl, dev(value), dev(mat)))
    L = np.diff(rowptr).astype(np.float64)[:, None, None]
    err = np.abs(got - hr.spmm_heads_ref(rowptr, col, value, mat))
    bound = (L + 2) * U * hr.spmm_heads_abs_sum(rowptr, col, value, mat)
    print(f"spmm_heads ({H}, {F}): worst error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)

    got = host(ops.sddmm(rp, cl, dev(x), dev(mat)))
    err = np.abs(got - hr.sddmm_heads_ref(rowptr, col, x, mat))
    bound = (F + 2) * U * hr.sddmm_heads_ref(rowptr, col, np.abs(x), np.abs(mat))
    print(f"sddmm_heads ({H}, {F}): worst error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


# ---- non-finite -----------------------------------------------------------------------------------

@pytest.mark.parametrize("H,F", [(8, 32), (3, 5)])
def test_non_finite_reaches_its_rows_head_and_column_only(big, H, F):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    row = hr.rows_of(rowptr)
    rng = np.random.default_rng(67 + H)
    value, mat = ints(rng, (nnz, H), -4, 4), ints(rng, (N, H, F), -4, 4)
    value[value == 0] = 1
    e_inf, e_nan = int(rowptr[13]) + 7, int(rowptr[12]) + 11  # entries of the two longest rows
    c_inf, c_nan = int(col[e_inf]), int(col[e_nan])
    assert c_inf != c_nan
    h_inf, f_inf, h_nan, f_nan = H - 1, F - 1, 0, 1
    mat[c_inf, h_inf, f_inf] = np.inf
    mat[c_nan, h_nan, f_nan] = np.nan
    value[e_inf, h_inf] = 0.0  # a stored 0 against the inf: NaN, no zero skipping
    want = hr.spmm_heads_ref(rowptr, col, value, mat)
    got = host(ops.spmm_heads(dev(rowptr), dev(col), dev(value), dev(mat)))
    assert np.isnan(got[13, h_inf, f_inf])
    touched = np.zeros((M, H, F), dtype=bool)
    touched[row[col == c_inf], h_inf, f_inf] = True
    touched[row[col == c_nan], h_nan, f_nan] = True
    assert touched.sum() > 2
    assert np.array_equal(~np.isfinite(got), touched)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)

    # sddmm: the same mat as y; the entries of those two columns, in that head
    x = ints(rng, (M, H, F), -4, 4)
    x[x == 0] = 1
    x[13, h_inf, f_inf] = 0.0
    want = hr.sddmm_heads_ref(rowptr, col, x, mat)
    got = host(ops.sddmm(dev(rowptr), dev(col), dev(x), dev(mat)))
    touched = np.zeros((nnz, H), dtype=bool)
    touched[col == c_inf, h_inf] = True
    touched[col == c_nan, h_nan] = True
    assert np.isnan(got[e_inf, h_inf])
    assert np.array_equal(~np.isfinite(got), touched)
    assert np.array_equal(got, want, equal_nan=True)


# ---- reproducibility and capture ------------------------------------------------------------------

def test_two_calls_give_the_same_bits_and_a_graph_replays_them(big):
    from paddle_sparse_amd import ops

    rowptr, col = big
    M, nnz = rowptr.size - 1, col.size
    H, F = 8, 32
    rng = np.random.default_rng(68)
    rp, cl = dev(rowptr), dev(col)
    value = dev(rng.normal(size=(nnz, H)).astype(np.float32))
    mat = dev(rng.normal(size=(N, H, F)).astype(np.float32))
    g = dev(rng.normal(size=(M, H, F)).astype(np.float32))

    def both_ways():
        v, m = value.detach().requires_grad_(), mat.detach().requires_grad_()
        out = ops.spmm_heads(rp, cl, v, m)
        out.backward(g)
        return out.detach(), v.grad, m.grad

    first, second = both_ways(), both_ways()
    for a, b in zip(first, second):
        assert torch.equal(a, b)

    def forward():
        return ops.spmm_heads(rp, cl, value, mat), ops.sddmm(rp, cl, g, mat)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        forward()  # the workspaces are in the allocator before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, score_g = forward()
    value.copy_(dev(rng.normal(size=(nnz, H)).astype(np.float32)))
    mat.copy_(dev(rng.normal(size=(N, H, F)).astype(np.float32)))
    graph.replay()
    out_e, score_e = forward()
    assert torch.equal(out_g, out_e) and torch.equal(score_g, score_e)


# ---- empty shapes ---------------------------------------------------------------------------------

def test_empty_shapes():
    import paddle_sparse_amd as psa
    from paddle_sparse_amd import ops

    H, F = 3, 4
    i64 = dict(dtype=torch.int64, device=DEV)
    none = torch.zeros(0, **i64)
    mat = torch.ones(5, H, F, device=DEV)
    # nnz = 0: a matrix of only empty rows
    rp = torch.zeros(4, **i64)
    out = ops.spmm_heads(rp, none, torch.zeros(0, H, device=DEV), mat)
    assert out.shape == (3, H, F) and not out.any()
    assert ops.sddmm(rp, none, torch.ones(3, H, F, device=DEV), mat).shape == (0, H)
    A = psa.SparseTensor(rowptr=rp, col=none, value=torch.zeros(0, H, device=DEV), sparse_sizes=(3, 5), is_sorted=True)
    out = A @ mat
    assert out.shape == (3, H, F) and not out.any()
    assert A.sddmm(torch.ones(3, H, F, device=DEV), mat).storage.value().shape == (0, H)
    # M = 0
    rp0 = torch.zeros(1, **i64)
    assert ops.spmm_heads(rp0, none, torch.zeros(0, H, device=DEV), mat).shape == (0, H, F)
    assert ops.sddmm(rp0, none, torch.ones(0, H, F, device=DEV), mat).shape == (0, H)
    # empty rows around one entry
    rp1 = torch.tensor([0, 0, 1, 1], **i64)
    out = ops.spmm_heads(rp1, torch.tensor([2], **i64), torch.full((1, H), 2.0, device=DEV), mat)
    assert out.shape == (3, H, F) and not out[0].any() and not out[2].any() and bool((out[1] == 2).all())


# ---- errors ---------------------------------------------------------------------------------------

def test_errors():
    import paddle_sparse_amd as psa

    H, K = 2, 4
    row, col = torch.tensor([0, 1], device=DEV), torch.tensor([1, 2], device=DEV)
    A = psa.SparseTensor(row=row, col=col, sparse_sizes=(2, 3))
    x, y = torch.zeros(2, H, K, device=DEV), torch.zeros(3, H, K, device=DEV)
    assert A.sddmm(x, y).storage.value().tolist() == [[0.0, 0.0], [0.0, 0.0]]
    with pytest.raises(ValueError):
        A.sddmm(x, y[:, 0])  # mixed ranks
    with pytest.raises(ValueError):
        A.sddmm(x[:, 0], y)
    with pytest.raises(ValueError):
        A.sddmm(x, torch.zeros(3, H + 1, K, device=DEV))  # H
    with pytest.raises(ValueError):
        A.sddmm(x, torch.zeros(3, H, K + 1, device=DEV))  # K
    with pytest.raises(ValueError):
        A.sddmm(torch.zeros(3, H, K, device=DEV), y)  # M
    with pytest.raises(ValueError):
        A.sddmm(x, torch.zeros(2, H, K, device=DEV))  # N
    with pytest.raises(ValueError):
        A.sddmm(x[:, :, :, None], y[:, :, :, None])  # rank 4
    with pytest.raises(TypeError):
        A.sddmm(x.half(), y.half())
    with pytest.raises(TypeError):
        A.sddmm(x.double(), y)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.sddmm(x.cpu(), y)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.sddmm(x, y.cpu())

    Ah = psa.SparseTensor(row=row, col=col, value=torch.ones(2, H, device=DEV), sparse_sizes=(2, 3))
    v = torch.ones(3, H, K, device=DEV)
    assert (Ah @ v).shape == (2, H, K)
    for reduce in ("mean", "min", "max"):
        with pytest.raises(NotImplementedError):
            Ah.matmul(v, reduce)
    with pytest.raises(ValueError):
        Ah.matmul(v, "prod")
    with pytest.raises(ValueError):
        Ah @ torch.ones(3, K, device=DEV)  # per-head values with a 2-D operand
    with pytest.raises(ValueError):
        Ah @ torch.ones(3, H + 1, K, device=DEV)  # H
    with pytest.raises(ValueError):
        Ah @ torch.ones(4, H, K, device=DEV)  # N
    with pytest.raises(ValueError):
        psa.SparseTensor(row=row, col=col, value=torch.ones(2, H, 2, device=DEV), sparse_sizes=(2, 3)) @ v  # rank 3
    with pytest.raises(TypeError):
        Ah @ v.half()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        Ah @ v.cpu()
    # the functional form follows the same rule after its coalesce
    index = torch.stack([row, col])
    assert torch.equal(psa.spmm(index, torch.ones(2, H, device=DEV), 2, 3, v), Ah @ v)
    with pytest.raises(NotImplementedError):
        psa.spmm(index, torch.ones(2, H, device=DEV), 2, 3, v, "max")
